"""NumPy float32 restatement of the product-quantisation rules of include/polus_hip.h (polus_pq_encode, polus_pq_update,
polus_pq_decode, polus_pq_lut, polus_pq_scores) and of the Lloyd loop of CorpusIndex.fit_pq, written from the rules, not
from the kernels (test infrastructure; the product never imports it).  Every operation is one float32 rounding, in the
order the header states, so the kernels are compared with it in bits.  Inputs are float32 arrays (bf16 data is widened by
the caller, which is exact)."""
import numpy as np

f32 = np.float32
LANES = 64


def _split(x, m):
    """x [T, m * dsub] as [T, m, dsub]."""
    return np.ascontiguousarray(x, dtype=f32).reshape(x.shape[0], m, -1)


def distances(x, cb):
    """dist [T, m, ksub]: the sequential f32 sum over t ascending, from +0.0, of fl(fl(x_t - cb_t)^2)."""
    m, ksub, dsub = cb.shape
    xs = _split(x, m)
    acc = np.zeros((x.shape[0], m, ksub), f32)
    with np.errstate(all="ignore"):
        for t in range(dsub):
            d = (xs[:, :, None, t] - cb[None, :, :, t]).astype(f32)
            acc = (acc + (d * d).astype(f32)).astype(f32)
    return acc


def encode(x, cb):
    """codes uint8 [T, m]: the lowest code minimising the distance, a NaN distance counting as +inf."""
    d = distances(x, cb)
    return np.where(np.isnan(d), np.inf, d).argmin(-1).astype(np.uint8)


def decode(codes, cb):
    """f32 [T, m * dsub]: the codewords named by the codes, zeros for a code >= ksub (round to the target dtype outside)."""
    m, ksub, dsub = cb.shape
    ok = codes < ksub
    y = cb[np.arange(m)[None], np.where(ok, codes, 0)]
    return np.where(ok[:, :, None], y, f32(0)).astype(f32).reshape(codes.shape[0], m * dsub)


def lut(q, cb):
    """f32 [Q, m, ksub]: the sequential f32 sum over t ascending, from +0.0, of fl(q_t * cb_t)."""
    m, ksub, dsub = cb.shape
    qs = _split(q, m)
    acc = np.zeros((q.shape[0], m, ksub), f32)
    with np.errstate(all="ignore"):
        for t in range(dsub):
            acc = (acc + (qs[:, :, None, t] * cb[None, :, :, t]).astype(f32)).astype(f32)
    return acc


def scores(table, codes):
    """f32 [Q, N]: the sequential f32 sum over j ascending, from +0.0, of table[b, j, codes[n, j]]; a byte >= ksub reads -inf."""
    Q, m, ksub = table.shape
    padded = np.full((Q, m, 256), -np.inf, f32)
    padded[:, :, :ksub] = table
    acc = np.zeros((Q, codes.shape[0]), f32)
    with np.errstate(all="ignore"):
        for j in range(m):
            acc = (acc + padded[:, j, :][:, codes[:, j]]).astype(f32)
    return acc


def update(x, codes, prev):
    """(out f32 [m, ksub, dsub], counts int32 [m, ksub]) of one Lloyd update.  Partial l of 64 adds, from +0.0, the rows t in
    [l * P, (l + 1) * P), P = ceil(T / 64), whose code is c, in ascending t; six rounds p_l = fl(p_l + p_(l xor o)), o = 32 .. 1,
    leave the sum in every partial; out = fl(sum / f32(count)), or prev where the count is 0; codes >= ksub are skipped."""
    m, ksub, dsub = prev.shape
    T = x.shape[0]
    per = -(-T // LANES)
    xs = _split(x, m)
    part = np.zeros((m, ksub, LANES, dsub), f32)
    counts = np.zeros((m, ksub), np.int32)
    for t in range(T):                                       # ascending t: every partial sees its rows in order
        c = codes[t].astype(np.int64)
        ok = c < ksub
        j = np.arange(m)[ok]
        part[j, c[ok], t // per] = (part[j, c[ok], t // per] + xs[t, ok]).astype(f32)
        counts[j, c[ok]] += 1
    lane = np.arange(LANES)
    for o in (32, 16, 8, 4, 2, 1):
        part = (part + part[:, :, lane ^ o]).astype(f32)
    assert (part == part[:, :, :1]).all() or np.isnan(part).any()
    out = prev.copy()
    has = counts > 0
    with np.errstate(all="ignore"):
        out[has] = (part[:, :, 0][has] / counts[has].astype(f32)[:, None]).astype(f32)
    return out, counts


def sample_rows(N, sample, seed):
    """The sampled documents of CorpusIndex.fit_pq, in the order drawn."""
    r = np.random.Generator(np.random.PCG64(int(seed)))
    return r.permutation(N) if N <= sample else r.choice(N, size=sample, replace=False)


def fit(x, m, ksub, iters):
    """The Lloyd loop of CorpusIndex.fit_pq over the sampled rows x [T, E] (f32, in the order drawn): the first ksub rows are
    the initial codewords of every sub-space, each round is encode then update."""
    cb = np.ascontiguousarray(_split(x[:ksub], m).transpose(1, 0, 2))
    for _ in range(iters):
        cb, _ = update(x, encode(x, cb), cb)
    return cb
