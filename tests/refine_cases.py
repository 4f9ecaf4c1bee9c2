"""Cases of the refine tests (tests/test_refine_cpu.py, tests/test_refine_gpu.py).  Needs no GPU to import."""
import functools

import numpy as np

f32 = np.float32
INT_MAX = 2 ** 31 - 1

# the kernel: E / 8 = 2, 6, 96 and 130 feature groups: fewer groups than a wave has lanes, more than 64 (a lane holds two),
# a ragged last round (130 = 2 * 64 + 2); C = 1 (one wave works), 7 (fewer columns than two rounds of a workgroup's waves)
# and 257 (several workgroups per query)
ES = (16, 48, 768, 1040)
B, N = 5, 300
CS = (1, 7, 257)
FP8_ES = (16, 768, 1040)
WIDE_ES = (2064, 5120)                           # past 2048 features the kernel holds its groups under a guard: 258 and 640 groups
INDEX_E = 32                                     # the width of the planted PQ / IVF-PQ corpora


def rng(seed):
    return np.random.Generator(np.random.PCG64(9800 + seed))


def err_bound(E):
    """The multiple of 2^-24 * sum |q_e d_e| the rule's score stays within of float64: one rounding of the product (1), the
    longest partial of 8 ceil(E / 512) terms (one rounding per add, the first exact: < 8 ceil(E / 512)), six tree adds, and one
    for second order."""
    return 8 * -(-E // 512) + 8


def gaussian(E, Bq=B, n=N, seed=0):
    """(q f32 [B, E], d f32 [N, E]) of N(0, 1) entries."""
    r = rng(seed + E)
    return r.standard_normal((Bq, E)).astype(f32), r.standard_normal((n, E)).astype(f32)


def summable(E, Bq=B, n=N, seed=0):
    """(q, d) with entries drawn from the multiples of 1/8 in [-2, 2]: exact in bf16; a product is a multiple of 1/64 of
    magnitude <= 4 and any sum of up to 1040 of them a multiple of 1/64 below 2^13, exact in f32 (2^19 < 2^24 steps).  So the
    true score is the same in every order and in float64, and ties are real."""
    assert E <= 1040
    r = rng(50 + seed + E)
    return (r.integers(-16, 17, size=(Bq, E)) / 8).astype(f32), (r.integers(-16, 17, size=(n, E)) / 8).astype(f32)


def candidates(Bq, C, n, seed=0):
    """int32 [B, C]: per query ids drawn with replacement; from C >= 7 on a row holds -1, N, INT_MAX, -INT_MAX - 1 and a
    repeat of its column 0.  At C = 1 query 1 holds -1 and query 2 holds N."""
    r = rng(200 + seed + C)
    cand = r.integers(0, n, size=(Bq, C)).astype(np.int32)
    if C >= 7:
        cand[:, 1], cand[:, 2], cand[:, 3], cand[:, 4], cand[:, 5] = -1, n, INT_MAX, -INT_MAX - 1, cand[:, 0]
    else:
        cand[1 % Bq, 0] = -1
        if Bq > 2:
            cand[2, 0] = n
    return cand


@functools.lru_cache(maxsize=None)
def index_corpus(n=700, Q=5, E=INDEX_E):
    """An exactly-summable [CLS] corpus for the index tests (q f32 [Q, E], docs f32 [n, E]) with planted ties: document 11 is
    a copy of document 400 and document 650 a copy of document 3, so each pair ties for every query and must come back lower
    id first."""
    q, d = summable(E, Q, n, seed=7)
    d[11], d[650] = d[400], d[3]
    return q, d
