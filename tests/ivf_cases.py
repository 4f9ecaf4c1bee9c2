"""Cases of the inverted-list tests (tests/test_ivf_cpu.py, tests/test_ivf_gpu.py, tests/test_ivf_index_gpu.py): the
smallest shapes at which each mechanism can go wrong."""
import numpy as np

from tests.centroid_cases import NONE, score_case

# (N, Ld, K).  Ld = 65 / 180 / 512: more than one block of 64 codes per document; (9, 512, 70): Ld >> K, many duplicates
# inside a document; K = 65535: the largest code that is a token; (1, 1, 1): one of everything.
LIST_SHAPES = [(1, 1, 1), (40, 17, 64), (70, 65, 300), (33, 180, 1000), (9, 512, 70), (5, 33, 65535)]
MARK_N = [1, 31, 32, 33, 70, 300]                  # the last bitmap word is partial, full, and one bit into the next
MARK_K, MARK_LD = 40, 9


def list_codes(N, Ld, K, seed=0):
    """centroid_cases.score_case's codes: holes, codes >= K, document 1 all absent, document 2 only its last slot."""
    return score_case(1, N, 1, Ld, K, seed=seed)[2]


def hot_codes(N=5000, Ld=12, K=50, seed=0):
    """Every document holds code 0 (twice) among others: all documents meet on one counter and one cursor."""
    r = np.random.Generator(np.random.PCG64(9500 + seed))
    codes = r.integers(1, K, size=(N, Ld)).astype(np.uint16)
    codes[r.random((N, Ld)) < 0.2] = NONE
    slot = r.integers(0, Ld - 1, size=N)
    codes[np.arange(N), slot] = 0
    codes[np.arange(N), slot + 1] = 0
    return codes


def mark_case(N, seed=0, B=4, Lq=6, nprobe=5, K=MARK_K, Ld=MARK_LD):
    """codes [N, Ld] whose centroid K - 2 has an empty list, probes int32 [B, Lq, nprobe] and qmask int32 [B, Lq].
    Probes hold -1, K, K + 7 and 70000 (skipped), the empty list's centroid, and tokens 0 and 1 of query 0 probe the
    same centroids; qmask has holes and query 1 (B > 1) has no valid token."""
    r = np.random.Generator(np.random.PCG64(9600 + seed + 17 * N))
    codes = list_codes(N, Ld, K, seed=seed + N)
    codes[codes == K - 2] = K - 3
    probes = r.integers(0, K, size=(B, Lq, nprobe)).astype(np.int32)
    u = r.random(probes.shape)
    probes[u < 0.10] = -1
    probes[(u >= 0.10) & (u < 0.15)] = K
    probes[(u >= 0.15) & (u < 0.18)] = K + 7
    probes[(u >= 0.18) & (u < 0.20)] = 70000
    probes[0, 0] = r.permutation(K)[:nprobe]       # valid, distinct; shared by two tokens
    probes[0, 1] = probes[0, 0]
    probes[B - 1, Lq - 1, 0] = K - 2               # an empty list
    qmask = (r.random((B, Lq)) >= 0.25).astype(np.int32)
    qmask[0, :2] = 1
    qmask[B - 1, Lq - 1] = 1
    if B > 1:
        qmask[1] = 0
    return codes, probes, qmask


def ids_case(B, N, seed=0):
    """cand int32 [B, N + 7]: per query a shuffle of all ids with three of them repeated, and -1, -9, N and N + 5."""
    r = np.random.Generator(np.random.PCG64(9700 + seed))
    rows = []
    for _ in range(B):
        row = np.concatenate([r.permutation(N), r.integers(0, N, size=3), [-1, -9, N, N + 5]]).astype(np.int32)
        rows.append(r.permutation(row))
    return np.stack(rows)
