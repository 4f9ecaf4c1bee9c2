"""Cases of the centroid kernel and index tests (tests/test_centroid_cpu.py, tests/test_centroid_gpu.py,
tests/test_centroid_index_gpu.py): the smallest shapes at which each mechanism can go wrong."""
import numpy as np

NONE = 0xFFFF
LDS_BYTES = 160 * 1024                 # the LDS route's budget: (K + 1) * Lq * 4 bytes

# (B, N, Lq, Ld, K).  Lq = 1 / 5: several document tokens per step; 31: two per step with an idle lane; 64 / 65 / 512:
# one per step in 1, 2 and 8 rounds of lanes; Ld = 65 / 180 / 512: more than one block of 64 codes.
SCORE_SHAPES = [(1, 1, 1, 1, 1), (3, 40, 5, 17, 64), (4, 70, 31, 65, 300), (2, 33, 64, 180, 1000), (2, 9, 65, 512, 70),
                (2, 5, 512, 3, 40)]
# (K + 1) * Lq * 4 > 160 KiB: the global route under each of the three lane mappings (Lq > 32, 17 .. 32, <= 16)
GLOBAL_SHAPES = [(2, 9, 65, 70, 700), (2, 12, 20, 33, 2100), (3, 20, 5, 17, 9000)]
CODE_SHAPES = [(1, 1), (5, 7), (67, 64), (9, 1000), (3, 65535)]       # rows x K
UPDATE_SHAPES = [(1, 1, 32), (70, 5, 128), (3001, 64, 256)]           # T, K, E


def score_case(B, N, Lq, Ld, K, seed=0, integer=True):
    """table [K, B*Lq + 3] (three guard columns: ldt > B*Lq), ragged qmask, codes with holes.  Document 1 has no present
    token and query 1 no valid token (where they exist); 0xFFFF and out-of-range codes sit in the middle of documents."""
    r = np.random.Generator(np.random.PCG64(9100 + seed))
    shape = (K, B * Lq + 3)
    table = r.integers(-8, 9, size=shape).astype(np.float32) if integer else r.standard_normal(shape).astype(np.float32)
    ql = r.integers(1, Lq + 1, size=B)
    qmask = (np.arange(Lq)[None] < ql[:, None]).astype(np.int32)
    qmask[r.random((B, Lq)) < 0.1] = 0
    if B > 1:
        qmask[1] = 0
    codes = r.integers(0, K, size=(N, Ld)).astype(np.uint16)
    dl = r.integers(1, Ld + 1, size=N)
    codes[np.arange(Ld)[None] >= dl[:, None]] = NONE
    u = r.random((N, Ld))
    codes[u < 0.08] = NONE
    if K < NONE - 1:
        codes[(u >= 0.08) & (u < 0.14)] = r.integers(K, NONE, size=int(((u >= 0.08) & (u < 0.14)).sum())).astype(np.uint16)
    if N > 1:
        codes[1] = NONE
    if N > 2:
        codes[2, :] = NONE
        codes[2, Ld - 1] = K - 1                                       # only the last slot present
    return table, qmask, codes


def code_case(rows, K, seed=0):
    """sim [rows, K + 5] (lds > K, guard columns hold +inf: reading past K would win), planted ties, a NaN entry, an
    all-NaN row, a masked row."""
    r = np.random.Generator(np.random.PCG64(9200 + seed))
    sim = np.full((rows, K + 5), np.inf, np.float32)
    sim[:, :K] = r.standard_normal((rows, K)).astype(np.float32)
    mask = np.ones(rows, np.int32)
    for i in range(rows):
        if K >= 3 and i % 2 == 0:                                      # the maximum twice (or three times): the first wins
            cols = np.sort(r.choice(K, size=min(3, K), replace=False))
            sim[i, cols] = 7.5
        if K >= 2 and i % 3 == 1:
            sim[i, int(r.integers(0, K))] = np.nan
    if rows >= 3:
        sim[rows - 1, :K] = np.nan
        mask[rows - 2] = 0
    if rows >= 5:
        sim[2, :K] = -np.inf                                           # every entry -inf: the first column
    return sim, mask


def update_case(T, K, E, seed=0):
    """x [T, E] N(0, 1) rows, codes uint16 [T]: cluster 0 holds nearly all tokens, the last cluster (K >= 5) is empty,
    cluster 1 (K >= 5) holds integer-valued pairs x, -x (sum exactly 0: prev is kept), some codes are absent."""
    r = np.random.Generator(np.random.PCG64(9300 + seed))
    x = r.standard_normal((T, E)).astype(np.float32)
    codes = np.zeros(T, np.uint16)
    if K >= 5 and T >= 20:
        few = r.choice(T, size=T // 5, replace=False)
        codes[few] = r.integers(2, K - 1, size=len(few)).astype(np.uint16)
        pair = few[:8]
        codes[pair] = 1
        x[pair[:4]] = r.integers(-4, 5, size=(4, E)).astype(np.float32)
        x[pair[4:]] = -x[pair[:4]]
        codes[few[8:12]] = NONE
        codes[few[12:14]] = K                                          # out of range: absent too
    prev = r.standard_normal((K, E)).astype(np.float32)
    return x, codes, prev


def planted_corpus(seed=0, directions=24, tokens=3000, E=32, noise=0.35):
    """Unit token vectors around `directions` unit directions: direction + noise * N(0, I) / sqrt(E), renormalised."""
    r = np.random.Generator(np.random.PCG64(9400 + seed))
    d = r.standard_normal((directions, E))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    x = d[r.integers(0, directions, size=tokens)] + noise * r.standard_normal((tokens, E)) / np.sqrt(E)
    return (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float32)
