"""Cases and bounds of the SPLADE tests (tests/test_splade_gpu.py, tests/test_splade_cpu.py).

Pooling: logits drawn from the halves in [-2, 3] (exact in bf16, so both dtypes see the same values and ties are
frequent), a mask with holes, the last sequence fully masked (B > 1), column 0 negative everywhere, column 1 with a
maximum of exactly 0.  Two layouts per shape: "vec", rows padded to whole 16-byte chunks from an aligned base, and
"scalar", ldl = V from a base one element past an aligned address.
Scores: (a) eighths, every sum exact in f32; (b) random f32 against the bound of any summation order."""
import functools

import numpy as np

ESIZE = {"f32": 4, "bf16": 2}
POOL_SHAPES = ((2, 5, 64), (3, 17, 1001), (1, 1, 8), (2, 33, 30522))          # B, S, V
POOL_LAYOUTS = ("vec", "scalar")

# |rep - log1p(xmax)| in ulps of the f32 result, log1p in float64 of the device's own xmax: 2 x the worst seen over
# POOL_SHAPES x both dtypes x both layouts on an MI355X.  The positive values of the grid are the six halves 0.5 .. 3,
# so the kernel's log1pf is exercised on six arguments.
REP_ULP_MEASURED = 0.4725       # every one of the six comes out correctly rounded (<= 0.5 ulp)
REP_ULP_BOUND = 2 * REP_ULP_MEASURED

FLOPS_ROWS = (1, 3, 64)
FLOPS_V = (64, 1001, 30522)

SCORE_M = (1, 64, 65, 200, 1024)
SCORE_V = (64, 30522)
SCORE_B, SCORE_N = 3, 300          # 300 documents: five workgroups per query (64 documents each at the least)
LDS_LIMIT_V = 160 * 1024 // 4      # the widest query row polus_sparse_scores takes

# the model tests: V, H, layers, heads, intermediate, max positions.  The engine's attention kernels take head_dim 64
# only, so four heads mean H = 256.
MODEL_SHAPE = (1000, 256, 2, 4, 512, 16)
MODEL_B, MODEL_S = 3, 16


def padded_ld(V, dtype):
    E = 16 // ESIZE[dtype]
    return (V + E - 1) // E * E


@functools.lru_cache(maxsize=None)
def pool_case(B, S, V):
    """(x float64 [B, S, V] on the grid of halves, mask int32 [B, S])."""
    rng = np.random.Generator(np.random.PCG64(100 * B + 10 * S + V))
    x = rng.integers(-4, 7, size=(B, S, V)).astype(np.float64) / 2
    mask = (rng.random((B, S)) < 0.7).astype(np.int32)
    mask[:, 0] = 1                                             # every sequence starts with a valid token ...
    if B > 1:
        mask[B - 1] = 0                                        # ... but the last one is masked out whole
    x[:, :, 0] = -np.abs(x[:, :, 0]) - 0.5
    if V > 1:
        x[:, :, 1] = -np.abs(x[:, :, 1])
        x[:, 0, 1] = 0.0
    x.setflags(write=False)
    mask.setflags(write=False)
    return x, mask


def flops_case(rows, V):
    """Non-negative representations with about half the entries zero, and a non-negative pre-filled gradient."""
    rng = np.random.Generator(np.random.PCG64(7 * rows + V))
    rep = np.log1p(np.maximum(rng.standard_normal((rows, V)), 0.0)).astype(np.float32)
    pre = rng.random((rows, V)).astype(np.float32)
    return rep, pre


def flops_rtol(rows, V):
    return (rows + V + 8) * 2.0 ** -24


def score_case(M, V, exact, B=SCORE_B, N=SCORE_N):
    """q [B, V], ids [N, M] with -1, V and repeated terms, w [N, M]."""
    rng = np.random.Generator(np.random.PCG64(31 * M + V + (1 if exact else 0)))
    ids = rng.integers(-1, V + 1, size=(N, M)).astype(np.int32)
    ids[0, 0], ids[1, 0] = -1, V
    if M > 1:
        ids[:, 1] = ids[:, 0]                                  # a term twice in every document
        ids[2, :] = 5                                          # one document of a single term, M times
    if exact:
        q = rng.integers(0, 17, size=(B, V)).astype(np.float32) / 8
        w = rng.integers(0, 17, size=(N, M)).astype(np.float32) / 8
    else:
        q = rng.standard_normal((B, V)).astype(np.float32)
        w = rng.standard_normal((N, M)).astype(np.float32)
    return q, ids, w


def gamma(n):
    u = n * 2.0 ** -24
    return u / (1 - u)
