"""Cases and bounds of the postings tests (tests/test_postings_cpu.py, tests/test_postings_gpu.py).  NumPy only.

Shapes are the smallest at which each kernel can still go wrong: N = 300 at block_docs = 64 gives five blocks, the last
with 44 documents; N = 64 is exactly one block and N = 40 less than one; V = 97 is no multiple of anything; V = 50 000 is
past the 40 960 columns the forward route can hold.

The float64 bound of the reference's scores.  A score is a recursive f32 sum of n products, each product rounded once
before it is added: n roundings of the products and n - 1 of the partial sums (the first sum, +0.0 + p, is exact), each
of relative size at most u = 2^-24 on a quantity bounded by the sum of the |products|.  To first order the error is at
most (2 n - 1) u sum|p| < n 2^-23 sum|p|, which is the bound used; it is derived, not tuned."""
import numpy as np

BUILD = dict(M=8, V=97, block_docs=64)
BUILD_N = (300, 64, 40)
HOT = 3                         # the term every document holds
EMPTY_BLOCK = 2                 # at N = 300: the block without a posting
COMPACT_V = (97, 200, 50000)
CAP = 12


def score_bound(n, mass):
    """|f32 score - exact score| <= n 2^-23 sum|products| for a sum of n products (derivation above)."""
    return n * 2.0 ** -23 * mass


def forward_case(N, M=BUILD["M"], V=BUILD["V"], block_docs=BUILD["block_docs"], seed=0, special=True, dyadic=False):
    """(ids int32 [N, M], w f32 [N, M]): distinct ids per document, term HOT in slot 0 of every document.  With
    `special`: -1 slots, ids >= V, +0.0 and -0.0 weights, one NaN weight, (-inf, -1) filler slots, and at more than
    EMPTY_BLOCK blocks one block whose slots are all no postings.  `dyadic`: weights are multiples of 1/8 in (0, 4]."""
    rng = np.random.Generator(np.random.PCG64(1000 + 7 * N + seed))
    others = np.array([t for t in range(V) if t != HOT])
    ids = np.stack([np.concatenate([[HOT], rng.permutation(others)[:M - 1]]) for _ in range(N)]).astype(np.int32)
    if dyadic:
        w = (rng.integers(1, 33, size=(N, M)) / 8.0).astype(np.float32)
    else:
        w = (0.05 + 2.0 * rng.random((N, M))).astype(np.float32)
    if special:
        for d in range(N):
            kind = d % 7
            m = 1 + d % (M - 1)                      # never slot 0: the hot term stays
            if kind == 0:
                ids[d, m] = -1
            elif kind == 1:
                ids[d, m] = V + (d % 3) * 1000       # V itself and far beyond
            elif kind == 2:
                w[d, m] = 0.0
            elif kind == 3:
                w[d, m] = -0.0
            elif kind == 4:
                ids[d, m], w[d, m] = -1, -np.inf     # the filler of a short SPLADE document
        if not dyadic:
            w[min(5, N - 1), 0] = np.nan             # on the hot term: every query holding it meets the NaN
        if N > (EMPTY_BLOCK + 1) * block_docs:
            a, b = EMPTY_BLOCK * block_docs, (EMPTY_BLOCK + 1) * block_docs
            ids[a:b:2] = -1                          # half the block by its ids,
            w[a + 1:b:2] = np.where(np.arange(M) % 2 == 0, 0.0, -0.0).astype(np.float32)   # half by its weights
    return ids, w


def empty_case(N=100, M=BUILD["M"]):
    """A corpus without a posting: P = 0."""
    return np.full((N, M), -1, np.int32), np.full((N, M), -np.inf, np.float32)


def query_lists(V=BUILD["V"], cap=CAP, seed=0, dyadic=False):
    """Five query lists (q_terms int32 [5, cap], q_w f32 [5, cap], q_count int32 [5]) in ascending id: a full row whose
    count claims more than cap, a short row with the hot term, an empty row, a row of one entry, and a row of cap - 2."""
    rng = np.random.Generator(np.random.PCG64(50 + seed))
    q_terms, q_w = np.full((5, cap), -1, np.int32), np.zeros((5, cap), np.float32)
    sizes = (cap, 4, 0, 1, cap - 2)
    for r, n in enumerate(sizes):
        t = np.sort(rng.permutation(V)[:n])
        if r == 1:
            t = np.sort(np.concatenate([[HOT], [x for x in t if x != HOT][:n - 1]]))
        q_terms[r, :n] = t
        q_w[r, :n] = (rng.integers(1, 33, size=n) / 8.0) if dyadic else (0.1 + 3.0 * rng.random(n))
    q_w[4, 1] = -1.5                                  # a negative query weight: the sums are not monotone
    q_count = np.array([100, 4, 0, 1, cap - 2], np.int32)
    return q_terms, q_w.astype(np.float32), q_count


def odd_query_list(V=BUILD["V"], cap=CAP):
    """One row that breaks the list's own promises: a -1 in the middle, an id >= V, a repeated term (it counts twice),
    descending ids, and live entries behind q_count that must not be read."""
    q_terms = np.full((1, cap), -1, np.int32)
    q_w = np.zeros((1, cap), np.float32)
    q_terms[0, :8] = [HOT, 10, -1, V, 10, 50, 7, V + 5]
    q_w[0, :8] = [0.5, 1.25, 9.0, 9.0, 0.75, 2.0, 1.0, 9.0]
    q_terms[0, 8], q_w[0, 8] = 20, 100.0              # behind the count
    return q_terms, q_w, np.array([8], np.int32)


def compact_rows_case(V, seed=0):
    """f32 [6, V]: all zero; all non-zero; sparse with -0.0 among the zeros; a NaN, an inf and a denormal kept; the first
    and last column only; a few dozen non-zeros."""
    rng = np.random.Generator(np.random.PCG64(70 + V + seed))
    q = np.zeros((6, V), np.float32)
    q[1] = 0.5 + rng.random(V)
    cols = rng.permutation(V)[:9]
    q[2, cols] = 1.0 + rng.random(9)
    q[2, rng.permutation(V)[:20]] = -0.0
    q[2, cols] = 1.0 + rng.random(9)
    q[3, [1, V // 2, V - 2]] = [np.nan, np.inf, 1e-42]
    q[4, [0, V - 1]] = [2.0, -3.0]
    q[5, rng.permutation(V)[:40]] = rng.random(40) + 0.25
    return q


def counted_queries(M, V, seed=0):
    """terms / tf int32 [4, M] as polus_bm25_term_counts leaves queries: distinct ids ordered by (count descending, id
    ascending), (-1, 0) in the unused slots; row 0 is full, row 1 half full, row 2 empty, row 3 holds an id >= V and
    (where there is room) a negative id other than -1 among its used slots."""
    rng = np.random.Generator(np.random.PCG64(90 + M + seed))
    terms, tf = np.full((4, M), -1, np.int32), np.zeros((4, M), np.int32)
    for r, n in enumerate((M, (M + 1) // 2, 0, M)):
        t = rng.permutation(V)[:n]
        c = rng.integers(1, 4, size=n)
        order = np.lexsort((t, -c))
        terms[r, :n], tf[r, :n] = t[order], c[order]
    terms[3, 0] = V
    if M > 2:
        terms[3, M // 2] = -5
    return terms, tf


def dyadic_reps(n, V, nnz, seed):
    """f32 [n, V]: at most `nnz` non-zeros per row, multiples of 1/8 in (0, 4]: every product of two of them is a
    multiple of 1/64 below 16 and every sum of up to 32 products is exact in f32, with or without fma, in any order."""
    rng = np.random.Generator(np.random.PCG64(seed))
    rep = np.zeros((n, V), np.float32)
    for r in range(n):
        k = int(rng.integers(0, nnz + 1)) if r % 5 else nnz
        cols = rng.permutation(min(V, 60))[:k]        # a small active vocabulary: shared terms and many tied scores
        rep[r, cols] = rng.integers(1, 33, size=k) / 8.0
    return rep
