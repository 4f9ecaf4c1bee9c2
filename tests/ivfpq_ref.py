"""NumPy float32 restatement of the IVF-PQ rules of include/polus_hip.h (polus_ivfpq_residual, polus_ivfpq_coarse_update,
polus_ivfpq_scores_ids) and of CorpusIndex.fit_ivfpq / add / search on an IVF-PQ index, written from the rules, not from the
kernels (test infrastructure; the product never imports it).  Every f32 operation is one rounding in the order the header
states, so the kernels are compared with it in bits.  Inputs are float32 arrays (bf16 data is widened by the caller, which is
exact); `round_to(a)` rounds an f32 array once to the index's dtype and widens it again (the identity for f32)."""
import numpy as np

from tests import pq_ref as pr

f32 = np.float32
LANES = 64


def half_norms(cent):
    """f32 [K]: -|c|^2 / 2, summed in float64 and rounded once."""
    c = np.asarray(cent, np.float64)
    return (-0.5 * (c * c).sum(axis=1)).astype(f32)


def similarities(x, cent):
    """float64 [T, K]: x . c - |c|^2 / 2 with the f32 half norms; its arg-max is the L2-nearest centroid."""
    return np.asarray(x, np.float64) @ np.asarray(cent, np.float64).T + half_norms(cent).astype(np.float64)[None]


def assign(x, cent):
    """uint16 [T]: the lowest centroid maximising the similarity (float64: the device's GEMM is f32, so a case must keep its
    best and second-best similarity apart, see `gap`)."""
    return similarities(x, cent).argmax(axis=1).astype(np.uint16)


def gap(x, cent):
    """(the smallest difference between the best and the second-best similarity of a row, max |similarity|)."""
    s = similarities(x, cent)
    if s.shape[1] == 1:
        return np.inf, float(np.abs(s).max())
    top = np.sort(s, axis=1)[:, -2:]
    return float((top[:, 1] - top[:, 0]).min()), float(np.abs(s).max())


def residual(x, cent, coarse):
    """f32 [T, E]: fl(x - cent[coarse]); zeros for a row whose coarse code is >= K."""
    K = cent.shape[0]
    ok = coarse < K
    with np.errstate(all="ignore"):
        r = (np.asarray(x, f32) - np.asarray(cent, f32)[np.where(ok, coarse, 0)]).astype(f32)
    return np.where(ok[:, None], r, f32(0)).astype(f32)


def coarse_update(x, coarse, prev, round_to):
    """(out f32 [K, E] holding values of the index's dtype, counts int32 [K]) of one Lloyd update of whole vectors: partial l
    of 64 adds, from +0.0, the rows t in [l * P, (l + 1) * P), P = ceil(T / 64), whose code is k, in ascending t; six rounds
    p_l = fl(p_l + p_(l xor o)), o = 32 .. 1; out = round_to(fl(sum / f32(count))), or prev where the count is 0."""
    K, E = prev.shape
    T = x.shape[0]
    per = -(-T // LANES)
    part = np.zeros((K, LANES, E), f32)
    counts = np.zeros((K,), np.int32)
    with np.errstate(all="ignore"):
        for t in range(T):
            k = int(coarse[t])
            if k < K:
                part[k, t // per] = (part[k, t // per] + x[t]).astype(f32)
                counts[k] += 1
        lane = np.arange(LANES)
        for o in (32, 16, 8, 4, 2, 1):
            part = (part + part[:, lane ^ o]).astype(f32)
        out = np.array(prev, f32, copy=True)
        has = counts > 0
        out[has] = round_to((part[:, 0][has] / counts[has].astype(f32)[:, None]).astype(f32))
    return out, counts


def full_scores(lut, cdot, coarse, codes):
    """f32 [Q, N]: fl(cdot[b, coarse[n]] + acc[b, n]) with acc pq_ref.scores' sequential sum; -inf where coarse[n] >= K."""
    K = cdot.shape[1]
    acc = pr.scores(lut, codes)
    ok = coarse < K
    with np.errstate(all="ignore"):
        s = (np.asarray(cdot, f32)[:, np.where(ok, coarse, 0)] + acc).astype(f32)
    return np.where(ok[None], s, f32(-np.inf)).astype(f32)


def scores_ids(lut, cdot, coarse, codes, cand):
    """f32 [Q, C]: full_scores at (b, cand[b, c]); -inf for an id outside [0, N)."""
    N = codes.shape[0]
    full = full_scores(lut, cdot, coarse, codes)
    ok = (cand >= 0) & (cand < N)
    got = np.take_along_axis(full, np.where(ok, cand, 0).astype(np.int64), axis=1)
    return np.where(ok, got, f32(-np.inf)).astype(f32)


def decode(coarse, codes, cent, cb):
    """f32 [N, E]: fl(cent[coarse] + decoded residual) (round to the index's dtype outside)."""
    return (np.asarray(cent, f32)[coarse] + pr.decode(codes, cb)).astype(f32)


def encode(x, cent, cb):
    """(coarse uint16 [T], codes uint8 [T, m]) of `add`."""
    coarse = assign(x, cent)
    return coarse, pr.encode(residual(x, cent, coarse), cb)


def fit(x, K, m, ksub, iters, pq_iters, round_to):
    """(centroids f32 [K, E] holding values of the index's dtype, codebook f32 [m, ksub, dsub]) of CorpusIndex.fit_ivfpq over
    the sampled rows x [T, E] (f32, in the order drawn)."""
    cent = np.array(x[:K], f32, copy=True)
    for _ in range(iters):
        cent, _ = coarse_update(x, assign(x, cent), cent, round_to)
    res = residual(x, cent, assign(x, cent))
    return cent, pr.fit(res, m, ksub, pq_iters)


def probes(cdot, nprobe):
    """int [Q, nprobe]: each query's best centroids by (cdot descending, lower id)."""
    cdot = np.asarray(cdot)
    return np.stack([np.lexsort((np.arange(cdot.shape[1]), -row))[:nprobe] for row in cdot])


def probed(scores, coarse, probe_ids):
    """scores [Q, N] with -inf wherever the document's list is not among the query's probes."""
    keep = (coarse[None, :, None] == probe_ids[:, None, :]).any(-1)
    return np.where(keep, scores, scores.dtype.type(-np.inf))
