"""Cases of the IVF-PQ tests (tests/test_ivfpq_cpu.py, tests/test_ivfpq_gpu.py).  Needs no GPU to import."""
import functools

import numpy as np

from tests import ivfpq_ref as ir
from tests import pq_cases as pc
from tests import pq_ref as pr

f32 = np.float32

# the scan: (m, ksub): 4 sub-spaces (the least), 20 (no multiple of 16: 4-byte pieces), 96 (the benchmark's) and 160 (the
# whole LDS); C around the wave and over the whole corpus; K = 1 (one list), 7 and 300 (more lists than a wave has lanes)
SCAN_FORMATS = ((4, 256), (20, 16), (96, 256), (160, 256))
SCAN_Q = (1, 3)
SCAN_C = (1, 63, 64, 65, 1000)
SCAN_N = 1000
SCAN_K = (1, 7, 300)
SCAN_PADS = (16, 3, 0)                           # ldc = m + pad: 16-byte pieces where m allows, single bytes, 4-byte pieces

RESIDUAL_ROWS = (1, 65)
RESIDUAL_E = (4, 768)
UPDATE_T = (1, 63, 64, 65, 1000)
UPDATE_K = 16

PLANTED = dict(seed=2, K=12, N=700, Q=5)         # m = 8, ksub = 16, dsub = 4: the codebook of pq_cases.planted
FIT = dict(seed=6, N=600, E=32, K=6, m=8, ksub=16, sample=500, pq_iters=2, iters=(1, 3))
KS = (10, 100)


def rng(seed):
    return np.random.Generator(np.random.PCG64(9500 + seed))


def scan_case(m, ksub, Q, K, N=SCAN_N, seed=0):
    """(lut f32 [Q, m, ksub], cdot f32 [Q, K], coarse uint16 [N], codes uint8 [N, m]) of N(0, 1) entries and valid codes."""
    r = rng(seed + 7 * m + Q + 13 * K)
    return (r.standard_normal((Q, m, ksub)).astype(f32), r.standard_normal((Q, K)).astype(f32),
            r.integers(0, K, size=N).astype(np.uint16), r.integers(0, ksub, size=(N, m)).astype(np.uint8))


def candidates(Q, C, N, seed=0):
    """int32 [Q, C]: per query C ids drawn without replacement in shuffled order; from C >= 4 on column 1 is -1, column 2 an
    id >= N and column 3 repeats column 0."""
    r = rng(100 + seed + Q + C)
    cand = np.stack([r.permutation(N)[:C] for _ in range(Q)]).astype(np.int32)
    if C >= 4:
        cand[:, 1], cand[:, 2], cand[:, 3] = -1, N + 5, cand[:, 0]
    return cand


@functools.lru_cache(maxsize=None)
def planted():
    """The planted integer corpus: K centroids with entries in multiples of 8 within [-32, 32], pairwise distinct in some
    coordinate; the residual codebook of pq_cases.planted (distinct integer codewords in [-3, 3]); documents = centroid +
    decoded residual; integer queries in [-3, 3].  Every value is exact in bf16 and every sum is exact in f32, and
    |residual| <= 3 < 5 <= the distance to any other centroid's differing coordinate, so the planted centroid is strictly
    L2-nearest."""
    p = PLANTED
    r = rng(p["seed"])
    cb = pc.planted()["cb"]
    m, ksub, dsub = cb.shape
    E, K, N, Q = m * dsub, p["K"], p["N"], p["Q"]
    seen = set()
    while len(seen) < K:
        seen.add(tuple(int(v) for v in 8 * r.integers(-4, 5, size=E)))
    cent = np.array(sorted(seen), f32)[r.permutation(K)]
    coarse = r.integers(0, K, size=N).astype(np.uint16)
    codes = r.integers(0, ksub, size=(N, m)).astype(np.uint8)
    docs = ir.decode(coarse, codes, cent, cb)
    q = r.integers(-3, 4, size=(Q, E)).astype(f32)
    return dict(cent=cent, cb=cb, coarse=coarse, codes=codes, docs=docs, q=q)


@functools.lru_cache(maxsize=None)
def fit_case():
    """Well-separated clusters for fit_ivfpq: K centres with entries in {-4, 0, 4}, documents = centre + N(0, 0.1^2) noise.
    The documents the sample draws first belong to clusters 0, 1, ... K - 1 in turn, so the initial centroids (the first K
    sampled rows) sit in K different clusters and no Lloyd round meets a near tie.  Returns the table rows of the N documents
    (f32) and the sampled rows for seed 3."""
    f = FIT
    r = rng(f["seed"])
    centres = (4 * r.integers(-1, 2, size=(f["K"], f["E"]))).astype(f32)
    rows = pr.sample_rows(f["N"], f["sample"], 3)
    label = r.integers(0, f["K"], size=f["N"])
    label[rows] = np.arange(len(rows)) % f["K"]
    docs = (centres[label] + 0.1 * r.standard_normal((f["N"], f["E"]))).astype(f32)
    return dict(docs=docs, rows=rows, label=label, centres=centres)
