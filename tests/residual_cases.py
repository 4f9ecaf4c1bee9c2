"""Shapes and planted inputs of the residual codec tests (tests/test_residual_cpu.py, tests/test_residual_gpu.py)."""
import numpy as np
import torch

from tests import residual_ref as ref

NBITS = (1, 2, 4)
MODES = ("f32", "bf16")
# (rows, E): one row, a few rows, a row count that is no multiple of the 256-thread block's rows at any E, more than
# one block, the E limit
CODEC_SHAPES = [(1, 32), (5, 32), (7, 96), (130, 128), (3, 256)]
K_EDGES = (1, 65535)                  # with E = 32
K_DEFAULT = 7
# integer anchor: (Q, N, Lq, Ld, E); the second is the rounds route at the E limit
INT_SHAPES = [(3, 40, 5, 17, 32), (2, 12, 130, 40, 256)]


def codec_tables(nbits):
    """cutoffs f32 [2^nbits - 1] and weights f32 [2^nbits].  The cutoffs are dyadic, (j - n / 2) / 16 + 1 / 64, so that
    1 + cutoff is a bf16 number and a residual can be planted exactly ON one; the weights are not bf16 numbers."""
    n = 1 << nbits
    cutoffs = ((np.arange(1, n) - n / 2) / 16.0 + 1.0 / 64.0).astype(np.float32)
    weights = ((np.arange(n) - (n - 1) / 2) / n * 0.9 + 0.001 * np.pi).astype(np.float32)
    assert (ref.to_mode(1.0 + cutoffs, "bf16") == 1.0 + cutoffs).all() and (ref.to_mode(weights, "bf16") != weights).all()
    return cutoffs, weights


def _step(v, mode, up):
    """The neighbour of the positive number v among the numbers of `mode`."""
    if mode == "f32":
        return np.nextafter(np.float32(v), np.float32(np.inf if up else -np.inf))
    bits = torch.tensor([float(v)]).to(torch.bfloat16).view(torch.int16) + (1 if up else -1)
    return np.float32(bits.view(torch.bfloat16).float().item())


def codec_case(rows, E, nbits, mode, K=K_DEFAULT, seed=0):
    """dict(x [rows, E], codes int16 [rows], centroids [K', E], cutoffs, weights, planted): float32 arrays holding
    numbers of `mode`.  K' = min(K, 64) centroid rows are drawn and tiled up to K (K = 65535 needs no 8 MB of noise).
    With 3 rows or more the last row has code K and the one before it 0xFFFF.  Planted into the leading valid rows, as
    far as they have room (`planted` lists what went in): for every cutoff c a residual exactly c and one step of x
    either side (the centroid element under it is 1.0), then NaN, +inf and -inf."""
    r = np.random.Generator(np.random.PCG64(4100 + 13 * seed + rows * 7 + E + 1000 * nbits + (K % 1000)))
    cutoffs, weights = codec_tables(nbits)
    base = ref.to_mode(r.standard_normal((min(K, 64), E)) * 0.5, mode)
    centroids = np.ascontiguousarray(np.tile(base, (-(-K // len(base)), 1))[:K])
    codes = r.integers(0, K, size=rows).astype(np.int64)
    codes[0] = K - 1
    valid = rows
    if rows >= 3:
        codes[rows - 1], codes[rows - 2] = K, 0xFFFF
        valid = rows - 2
    ok = codes < K
    x = np.zeros((rows, E), np.float32)
    x[ok] = centroids[codes[ok]] + r.standard_normal((int(ok.sum()), E)).astype(np.float32) * 0.3
    x[~ok] = r.standard_normal((int((~ok).sum()), E)).astype(np.float32)
    x = ref.to_mode(x, mode)
    plants = [(f"cut{j}{tag}", c, side) for j, c in enumerate(cutoffs) for tag, side in (("", None), ("+", True), ("-", False))]
    plants += [("nan", np.nan, None), ("+inf", np.inf, None), ("-inf", -np.inf, None)]
    planted = []
    for p, (name, v, side) in enumerate(plants[:valid * E]):
        row, col = divmod(p, E)
        if name.startswith("cut"):
            centroids[codes[row], col] = 1.0
            xv = np.float32(1.0) + np.float32(v)
            x[row, col] = xv if side is None else _step(xv, mode, side)
        else:
            x[row, col] = v
        planted.append(name)
    # a planted centroid element changes the residuals of other rows with the same code: nothing here depends on them
    return dict(x=x, codes=codes.astype(np.uint16).view(np.int16), centroids=centroids, cutoffs=cutoffs, weights=weights,
                planted=planted, K=K)


def corpus_codes(shape, dmask, K, nbits, seed=0):
    """codes int16 [N, Ld] and packed uint8 [N, Ld, E * nbits / 8] of a corpus of `shape` (Q, N, Lq, Ld, E): codes
    random in [0, K), and >= K (0xFFFF, K and values between) exactly where dmask is 0; every byte value occurs."""
    Q, N, Lq, Ld, E = shape
    r = np.random.Generator(np.random.PCG64(4700 + seed + N * 3 + Ld * 5 + E + nbits))
    codes = r.integers(0, K, size=(N, Ld)).astype(np.int64)
    if dmask is not None:
        absent = r.choice(np.array([0xFFFF, K, (K + 0xFFFF) // 2]), size=(N, Ld))
        codes = np.where(np.asarray(dmask) != 0, codes, absent)
    packed = r.integers(0, 256, size=(N, Ld, E * nbits // 8)).astype(np.uint8)
    return codes.astype(np.uint16).view(np.int16), packed


def gaussian_codec(K, E, nbits, mode, seed=0):
    """centroids [K, E] N(0, 1) as numbers of `mode` and weights f32 [2^nbits] ~ N(0, 0.3)."""
    r = np.random.Generator(np.random.PCG64(4800 + seed + K + E + nbits))
    return ref.to_mode(r.standard_normal((K, E)), mode), (r.standard_normal(1 << nbits) * 0.3).astype(np.float32)


_GAUSSIAN = {}


def gaussian_case(shape, masks, K, nbits, mode, seed=0):
    """(q, qmask, dmask, codes, packed, centroids, weights): the N(0, 1) queries and corpus of
    tests/rerank_cases.make_case with the corpus put through a codec.  The codes are given, not searched for: random in
    [0, K), and >= K exactly where dmask is 0 (no dependence on near ties of a GEMM).  Centroids are N(0, 1) rows, the
    cutoffs and weights the quantiles of the first 512 valid tokens' residuals (residual_ref.fit_tables) and the bits the
    reference compressor's.  The decoded corpus keeps what the tolerance of tests/maxsim_cases.py was measured on:
    every document token is its own Gaussian-like vector, so a score is a sum of maxima over many distinct tokens.
    (Random bits around K points would not: at Ld = 512 every document would hold the same K directions, the scores
    would shrink against the vectors' norms, and with them the rounding error relative to max|score| would grow.)"""
    from tests.rerank_cases import make_case
    Q, N, Lq, Ld, E = shape
    key = (shape, masks, mode, seed)
    if key not in _GAUSSIAN:                                  # shared by the three nbits (nothing writes to them)
        q, d, qm, dm = make_case(shape, masks, seed)
        _GAUSSIAN[key] = (q, qm, dm, ref.to_mode(d, mode).reshape(N * Ld, E))
    q, qm, dm, flat = _GAUSSIAN[key]
    codes, _ = corpus_codes(shape, dm, K, nbits, seed)
    centroids, _ = gaussian_codec(K, E, nbits, mode, seed)
    c = codes.reshape(-1)
    ok = ref.codes_u16(c) < K
    fit = np.flatnonzero(ok)[:512]                             # the codec is fitted on a sample, as CorpusIndex.fit_codec does
    cutoffs, weights = ref.fit_tables(flat[fit] - centroids[ref.codes_u16(c)[fit]], nbits)
    packed = ref.compress(flat, c, centroids, cutoffs, nbits).reshape(N, Ld, -1)
    return q, qm, dm, codes, packed, centroids, weights


def integer_case(shape, nbits, seed=0):
    """q [Q, Lq, E] and centroids [K, E] integers in [-3, 3], integer weights in [-8, 8) (distinct, asymmetric),
    random codes and bits, ragged masks, document N - 1 empty.  A decoded element is an integer of magnitude <= 11, so
    every product and sum is an integer below 2^24: f32, bf16 x bf16 -> f32 and float64 agree exactly."""
    Q, N, Lq, Ld, E = shape
    K = 11
    r = np.random.Generator(np.random.PCG64(4900 + seed + Q + 3 * N + 5 * Lq + 7 * Ld + E + nbits))
    q = r.integers(-3, 4, size=(Q, Lq, E)).astype(np.float32)
    centroids = r.integers(-3, 4, size=(K, E)).astype(np.float32)
    weights = {1: [-2, 1], 2: [-5, -1, 2, 7], 4: list(range(-8, 8))}[nbits]
    weights = np.asarray(weights, np.float32)
    ql, dl = r.integers(1, Lq + 1, size=Q), r.integers(1, Ld + 1, size=N)
    qm = (np.arange(Lq)[None] < ql[:, None]).astype(np.int32)
    dm = (np.arange(Ld)[None] < dl[:, None]).astype(np.int32)
    dm[r.random((N, Ld)) < 0.15] = 0
    dm[:, 0] = 1
    dm[N - 1] = 0
    codes, packed = corpus_codes(shape, dm, K, nbits, seed)
    assert 3 * 11 * E * Lq < 2 ** 24
    return q, centroids, weights, codes, packed, qm, dm
