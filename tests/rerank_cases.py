"""Cases of the re-ranking tests (tests/test_rerank_gpu.py, tests/test_rerank_cpu.py): the MaxSim shapes with a free
corpus size, masks drawn by the rules of tests/maxsim_cases.make_case, and candidate lists that hold what a first
stage can hand over: any order, shared and repeated documents, the empty document, -1 padding and ids past the corpus."""
import numpy as np

# (Q, N, Lq, Ld, E)
SHAPES = [(1, 1, 1, 1, 32),            # the smallest case
          (3, 40, 5, 17, 32),          # a partial 16-token tile
          (4, 64, 31, 65, 64),         # one token past a tile edge
          (5, 50, 33, 180, 128),       # query tile edge, production Ld
          (2, 20, 130, 512, 256)]      # the long-query route, limit Ld and E
MASKS = ["none", "ragged"]
CS = (1, 7, 70)
INT_MAX = 2 ** 31 - 1


def make_case(shape, masks, seed=0):
    """q [Q, Lq, E], d [N, Ld, E] (float32, N(0, 1)), qmask [Q, Lq] / dmask [N, Ld] int32 or None.  "ragged": prefix
    lengths (1 among them), holes, document N - 1 and query Q - 1 without a valid token, padding holding large values."""
    Q, N, Lq, Ld, E = shape
    r = np.random.Generator(np.random.PCG64(5000 + 7 * seed + Q * 31 + N * 13 + Lq * 17 + Ld * 5 + E))
    q = r.standard_normal((Q, Lq, E)).astype(np.float32)
    d = r.standard_normal((N, Ld, E)).astype(np.float32)
    if masks == "none":
        return q, d, None, None
    ql = r.integers(1, Lq + 1, size=Q)
    dl = r.integers(1, Ld + 1, size=N)
    ql[0], dl[0] = 1, 1
    qm = (np.arange(Lq)[None] < ql[:, None]).astype(np.int32)
    dm = (np.arange(Ld)[None] < dl[:, None]).astype(np.int32)
    if Ld > 4:
        dm[r.random((N, Ld)) < 0.15] = 0
        dm[np.arange(N), 0] = 1
    if Lq > 4:
        qm[r.random((Q, Lq)) < 0.15] = 0
        qm[np.arange(Q), 0] = 1
    if N > 1:
        dm[N - 1] = 0
    if Q > 1:
        qm[Q - 1] = 0
    d[dm == 0] *= 4.0
    q[qm == 0] *= 4.0
    return q, d, qm, dm


def candidates(Q, N, C, seed=0):
    """int32 [Q, C]: ids of [0, N) in any order (documents shared between queries and repeated inside a row), and
    planted in every row that has the room: the empty document N - 1, -1 in the middle and at the end, one id equal to
    N and one equal to 2^31 - 1.  With C = 1 the rows take these in turn."""
    r = np.random.Generator(np.random.PCG64(6000 + 11 * seed + Q * 3 + N * 5 + C))
    cand = r.integers(0, N, size=(Q, C)).astype(np.int64)
    special = [N - 1, -1, N, INT_MAX]
    if C >= 7:
        cand[:, 0] = N - 1
        cand[:, 1] = r.integers(0, N)                  # one document for every query
        cand[:, 2] = -1
        cand[:, 3] = N
        cand[:, 4] = INT_MAX
        cand[:, C - 1] = -1
    else:
        for b in range(1, Q):
            cand[b, 0] = special[(b - 1) % 4]
    return cand.astype(np.int32)


def present(cand, N):
    return (cand >= 0) & (cand < N)


# Several documents per wave.  A wave of the rerank kernel takes candidates c, c + 4, ... of its workgroup's block of
# 4 * dpw columns, and the launch (maxsim_common.h rr_launch) halves dpw from 8 while fewer than 1024 workgroups result, so
# dpw exceeds 1 only from Q * ceil(C / 8) >= 1024 on.  (Q, N, Lq, Ld, E), [(C, dpw), ...]: every C leaves a partial
# last block, where waves hold fewer documents than dpw.  Ld = 70 is five tiles, an odd number.
WAVE_SHAPES = [((16, 48, 20, 70, 64), [(507, 2), (1011, 4), (2021, 8)]),       # the query stays in registers
               ((16, 48, 70, 70, 128), [(507, 2), (1011, 4), (2021, 8)]),      # rounds over the query: 2 (bf16), 3 (f32)
               ((64, 60, 32, 180, 128), [(131, 2), (1000, 8)])]                # the production shape over a small corpus


def docs_per_wave(Q, C):
    """The launch's rule, restated."""
    dpw = 8
    while dpw > 1 and Q * -(-C // (4 * dpw)) < 1024:
        dpw //= 2
    return dpw


def wave_candidates(Q, N, C, seed=0):
    """int32 [Q, C]: random ids of [0, N) among which a third of the entries are the empty document N - 1, -1, N or
    2^31 - 1, so that a wave's sequence c, c + 4, ... keeps passing from absent and empty documents to present ones and
    back.  Row 0 begins with one planted sequence of eight."""
    r = np.random.Generator(np.random.PCG64(7000 + 11 * seed + Q * 3 + N * 5 + C))
    cand = r.integers(0, N, size=(Q, C)).astype(np.int64)
    u = r.random((Q, C))
    for lo, hi, v in ((0.00, 0.13, N - 1), (0.13, 0.23, -1), (0.23, 0.28, N), (0.28, 0.33, INT_MAX)):
        cand[(u >= lo) & (u < hi)] = v
    plant = [1, N - 1, 2, -1, N - 1, N, 0, INT_MAX]
    n = min(len(plant), (C + 3) // 4)
    cand[0, 0:4 * n:4] = plant[:n]
    return cand.astype(np.int32)


def wave_transitions(cand, N, dpw, empty):
    """{(kind of a document, kind of the next document of the same wave)}, kinds "present", "empty", "absent"."""
    Q, C = cand.shape
    kind = np.where(present(cand, N), np.where(cand == empty, 1, 0), 2)
    c = np.arange(C - 4)
    same = c // (4 * dpw) == (c + 4) // (4 * dpw)
    names = ("present", "empty", "absent")
    return {(names[a], names[b]) for a, b in set(zip(kind[:, :-4][:, same].ravel().tolist(), kind[:, 4:][:, same].ravel().tolist()))}
