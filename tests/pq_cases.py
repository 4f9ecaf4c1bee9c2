"""Cases of the product-quantisation tests (tests/test_pq_cpu.py, tests/test_pq_gpu.py).  Needs no GPU to import."""
import functools

import numpy as np

from tests import pq_ref as pr

f32 = np.float32

# the scan: (m, ksub): 4 sub-spaces (the least), 20 (no multiple of 16: 4-byte pieces), 16 (small tables: qt > 1), 96 (the
# benchmark's) and 160 (the whole LDS).  Some Q is no multiple of the route's qt; N around the wave and beyond one workgroup
SCAN_FORMATS = ((4, 256), (20, 16), (16, 256), (96, 256), (160, 256))
SCAN_Q = (1, 3, 5)
SCAN_N = (1, 63, 64, 65, 1000)

# lut / encode / decode: dsub, with rows in ROWS and both dtypes
DSUBS = (1, 4, 8, 32)
ROWS = (1, 65)
UPDATE_T = (1, 63, 64, 65, 1000)

PLANTED = dict(seed=1, m=8, ksub=16, dsub=4, N=700, Q=5)
FIT = dict(seed=5, N=600, E=32, m=8, ksub=16, iters=3, sample=500)
KS = (10, 100)


def rng(seed):
    return np.random.Generator(np.random.PCG64(9000 + seed))


def scan_case(m, ksub, Q, N, seed=0):
    """(table f32 [Q, m, ksub], codes uint8 [N, m]) of N(0, 1) entries and valid codes."""
    r = rng(seed + 7 * m + Q + N)
    return r.standard_normal((Q, m, ksub)).astype(f32), r.integers(0, ksub, size=(N, m)).astype(np.uint8)


def codebook(m, ksub, dsub, seed=0):
    return rng(seed + m + ksub + dsub).standard_normal((m, ksub, dsub)).astype(f32)


@functools.lru_cache(maxsize=None)
def planted():
    """The planted integer corpus: a codebook of distinct integer codewords in [-3, 3], documents assembled from random codes
    and integer queries.  Every product and sum is a small integer, so f32, bf16 storage and float64 agree exactly, and a
    document's nearest codewords are the planted ones at distance 0."""
    p = PLANTED
    r, (m, ksub, dsub, N, Q) = rng(p["seed"]), (p[k] for k in ("m", "ksub", "dsub", "N", "Q"))
    cb = np.zeros((m, ksub, dsub), f32)
    for j in range(m):
        seen = set()
        while len(seen) < ksub:
            seen.add(tuple(int(v) for v in r.integers(-3, 4, size=dsub)))
        cb[j] = np.array(sorted(seen), f32)[r.permutation(ksub)]
    codes = r.integers(0, ksub, size=(N, m)).astype(np.uint8)
    docs = pr.decode(codes, cb)
    q = r.integers(-3, 4, size=(Q, m * dsub)).astype(f32)
    return dict(cb=cb, codes=codes, docs=docs, q=q)


def as_search_case(q, docs):
    """The dict tests/search_cases.py's cls_case gives: queries and documents as rows of one table, one token each."""
    Q, N = len(q), len(docs)
    return dict(table=np.concatenate([q, docs]).astype(f32), q_ids=np.arange(Q, dtype=np.int32)[:, None],
                d_ids=(Q + np.arange(N, dtype=np.int32))[:, None], q_mask=np.ones((Q, 1), np.int32), d_mask=np.ones((N, 1), np.int32))
