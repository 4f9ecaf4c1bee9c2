"""Shapes, masks, candidate tables and row selections for the pair-packing tests (tests/test_pairs_cpu.py on the
reference, tests/test_pairs_gpu.py on the kernels).  NumPy only.

The shapes are the smallest that reach every branch of pairs.hip: Lq / Ld below one 64-token step, exactly one, and
more than one (5, 64, 70; 7, 130); S below a step, below two and above three (16, 48, 200); one and several queries
and candidates; one workgroup (4 rows) and more.  max_q follows S so that at S = 16 and 48 the long query and the
long document are both truncated in the same row, and at S = 200 neither the short ones nor the 130-token document."""
import itertools
import zlib

import numpy as np

LQ, LD, SS, BS, NS = (5, 64, 70), (7, 130), (16, 48, 200), (1, 3), (1, 4)
MAX_Q = {16: 6, 48: 20, 200: 64}
MASKS = ("none", "prefix", "left", "holes", "zero_row")
STRIPS = ((0, 0, 0, 0), (1, 1, 1, 1), (8, 8, 8, 8))
ROWS = ("all", "perm", "subset_repeat")
N_DOCS = 6
SPECIAL = (101, 102, 0)
VOCAB = 1000                  # ordinary tokens are drawn from [200, VOCAB): never a special id


def shapes():
    return list(itertools.product(LQ, LD, SS, BS, NS))


def _rng(*key):
    return np.random.Generator(np.random.PCG64(zlib.crc32(repr(key).encode())))


def make_mask(kind, rows, L, rng):
    """int32 [rows, L] or None.  prefix: 1s then 0s; left: 0s then 1s (left padding); holes: random, non-zero values
    other than 1 among the kept; zero_row: prefix with one row all zero."""
    if kind == "none":
        return None
    m = np.zeros((rows, L), np.int32)
    for r in range(rows):
        k = int(rng.integers(0, L + 1))
        if kind in ("prefix", "zero_row"):
            m[r, :k] = 1
        elif kind == "left":
            m[r, L - k:] = 1
        elif kind == "holes":
            m[r] = (rng.uniform(size=L) < 0.6) * rng.integers(1, 4, size=L)      # any non-zero value keeps a token
        else:
            raise ValueError(kind)
    if kind == "zero_row":
        m[int(rng.integers(0, rows))] = 0
    return m


def make_case(Lq, Ld, S, B, n, mask_kind, rows_kind):
    """dict of host arrays for one case; `rows` is None or an int32 array."""
    rng = _rng(Lq, Ld, S, B, n, mask_kind, rows_kind)
    q_ids = rng.integers(200, VOCAB, size=(B, Lq)).astype(np.int32)
    d_ids = rng.integers(200, VOCAB, size=(N_DOCS, Ld)).astype(np.int32)
    cand = rng.integers(0, N_DOCS, size=(B, n)).astype(np.int32)
    absent = rng.uniform(size=(B, n))
    cand[absent < 0.15] = -1
    cand[absent > 0.85] = N_DOCS
    P = B * n
    if rows_kind == "all":
        rows = None
    elif rows_kind == "perm":
        rows = rng.permutation(P).astype(np.int32)
    else:
        rows = rng.choice(P, size=max(1, P - 1), replace=False).astype(np.int32)
        rows = np.concatenate([rows, rows[:1]])                                   # the first pair once more
    return dict(q_ids=q_ids, qmask=make_mask(mask_kind, B, Lq, rng), d_ids=d_ids, dmask=make_mask(mask_kind, N_DOCS, Ld, rng),
                cand=cand, rows=rows, max_q=MAX_Q[S], S=S)
