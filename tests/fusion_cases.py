"""Cases of the rank-fusion tests (tests/test_fusion_cpu.py, tests/test_fusion_gpu.py).  NumPy only.

A case is a dict: ids int32 [L, Q, C], scores f32 [L, Q, C], n_docs, weights (a list of L floats or None) and rrf_k.
Rows are what a search returns unless the case says otherwise: ids distinct within a list row, scores descending.  Every
case runs in the three modes; `reference(name, mode)` computes tests/fusion_ref.py's answer once per process.

The float64 bound of the CPU test.  Against exact arithmetic on the same f32 inputs a contribution carries at most four
f32 roundings (minmax: s - lo, hi - lo, the division, the product with w; rrf: the sum and the division; sum: the
product), each of relative size at most u = 2^-24, and the fused score of a document adds at most L - 1 more, each
relative to a partial sum that is at most the sum of the contributions' magnitudes.  Bound: (L + 3) u (1 + 2^-20) times
that sum of magnitudes, for documents without repeated copies (a row with r copies has r - 1 more additions; the bound
counts the copies)."""
import functools

import numpy as np

from tests import fusion_ref as fr

MODE_NAMES = ("rrf", "sum", "minmax")
U = 2.0 ** -24


def value_bound(n_terms):
    """Relative to the sum of the magnitudes of a document's n_terms contributions (derivation above)."""
    return (n_terms + 3) * U * (1.0 + 2.0 ** -20)


def _rng(seed):
    return np.random.Generator(np.random.PCG64(seed))


def ranked_lists(seed, L, Q, C, pool=None, kind="partial"):
    """ids, scores [L, Q, C] as L searches would return them.  kind: "partial" draws every list row from the same pool of
    `pool` documents (default 2 C: about half of a row's documents are in another list too), "identical" gives every list
    the same ids in its own order, "disjoint" gives list l the ids [l C, (l + 1) C).  Returns (ids, scores, n_docs)."""
    rng = _rng(seed)
    pool = max(2 * C, 2) if pool is None else pool
    ids = np.empty((L, Q, C), np.int32)
    for r in range(Q):
        base = rng.permutation(pool)[:C]
        for l in range(L):
            if kind == "identical":
                ids[l, r] = base[rng.permutation(C)]
            elif kind == "disjoint":
                ids[l, r] = l * C + rng.permutation(C)
            else:
                ids[l, r] = rng.permutation(pool)[:C]
    scores = -np.sort(-(rng.standard_normal((L, Q, C)) * 3.0 + 5.0), axis=2)
    n_docs = L * C if kind == "disjoint" else pool
    return ids, scores.astype(np.float32), n_docs


def _case(ids, scores, n_docs, weights=None, rrf_k=60.0):
    return dict(ids=np.ascontiguousarray(ids, np.int32), scores=np.ascontiguousarray(scores, np.float32), n_docs=int(n_docs),
                weights=weights, rrf_k=rrf_k)


def _holes():
    """L = 3, Q = 4, C = 130.  Row 0: clean.  Row 1: -1 in the middle of a list, ids >= n_docs, and NaN, +inf and -inf
    scores, so the ranks behind them move up.  Row 2: the holes at the first and last column and across the 64-column
    edge.  Row 3: every entry dropped (negative or too large an id in every list, so in every mode and without scores)."""
    ids, scores, n = ranked_lists(41, 3, 4, 130)
    ids[0, 1, 50] = -1
    ids[1, 1, 7], ids[1, 1, 8] = n, n + 1000
    ids[2, 1, 100] = -5
    scores[0, 1, 20], scores[1, 1, 64], scores[2, 1, 3] = np.nan, np.inf, -np.inf
    ids[0, 2, 0], ids[0, 2, 129], ids[1, 2, 63], ids[1, 2, 64] = -1, -1, n, -2
    scores[2, 2, 0], scores[2, 2, 128:] = np.nan, -np.inf
    ids[:, 3] = -1
    ids[1, 3, ::2] = n
    ids[2, 3, 5] = 2 ** 31 - 1
    return _case(ids, scores, n)


def _repeats():
    """A repeated id inside one list row: twice in list 0 of row 0, three times in list 1 of row 1 (one copy across the
    64-column edge), and a row whose list 0 holds one id only."""
    ids, scores, n = ranked_lists(43, 2, 3, 66)
    ids[0, 0, 5] = ids[0, 0, 3]
    ids[1, 1, 10] = ids[1, 1, 65] = ids[1, 1, 2]
    ids[0, 2, :] = 9
    return _case(ids, scores, n)


def _minmax_edges():
    """L = 3, Q = 4, C = 5.  Row 0: list 0 has hi == lo (five equal scores), list 1 one kept entry, list 2 negative
    scores only.  Row 1: every list has hi == lo.  Row 2: scores of both signs.  Row 3: one kept entry in all."""
    ids, scores, n = ranked_lists(47, 3, 4, 5, pool=8)
    scores[0, 0, :] = 2.5
    ids[1, 0, 1:] = -1
    scores[2, 0, :] = [-1.0, -1.5, -2.25, -7.0, -1e3]
    scores[:, 1, :] = np.array([[0.75], [-3.0], [0.0]], np.float32)
    scores[:, 2, :] = [4.0, 1.5, 0.0, -0.125, -6.0]
    ids[:, 3, 1:] = -1
    return _case(ids, scores, n)


def _symmetric():
    """Two rrf lists: document 7 is rank 1 / rank 2 and document 3 is rank 2 / rank 1.  Under rrf the fused bits are equal
    (a + b and b + a are the same rounding), so a search must return document 3 first."""
    ids = np.array([[[7, 3]], [[3, 7]]], np.int32)
    scores = np.array([[[2.0, 1.0]], [[9.0, 8.0]]], np.float32)
    return _case(ids, scores, 10)


WEIGHTS3 = [0.0, -1.5, 0.3]           # a zero, a negative and a non-dyadic weight (0.3f)

BUILDERS = {
    "one entry": lambda: _case(np.array([[[4]]]), np.array([[[1.25]]]), 5),
    "C = 63": lambda: _case(*ranked_lists(1, 2, 3, 63)),
    "C = 64": lambda: _case(*ranked_lists(2, 2, 3, 64)),
    "C = 65": lambda: _case(*ranked_lists(3, 2, 3, 65), weights=[2.0, 0.3]),
    "4095 slots": lambda: _case(*ranked_lists(4, 3, 2, 1365), weights=WEIGHTS3),
    "4096 slots, L = 4": lambda: _case(*ranked_lists(5, 4, 2, 1024)),
    "4096 slots, L = 8": lambda: _case(*ranked_lists(6, 8, 2, 512, pool=700), rrf_k=0.0),
    "Q = 300": lambda: _case(*ranked_lists(7, 2, 300, 12)),
    "Q = 600": lambda: _case(*ranked_lists(8, 2, 600, 3)),          # more rows than the grid has workgroups
    "identical": lambda: _case(*ranked_lists(9, 3, 2, 70, kind="identical"), weights=WEIGHTS3),
    "disjoint": lambda: _case(*ranked_lists(10, 3, 2, 70, kind="disjoint")),
    "partial": lambda: _case(*ranked_lists(11, 3, 2, 70), weights=WEIGHTS3, rrf_k=1.5),
    "holes": _holes,
    "repeats": _repeats,
    "minmax edges": _minmax_edges,
    "symmetric": _symmetric,
}
NAMES = tuple(BUILDERS)


@functools.lru_cache(maxsize=None)
def case(name):
    return BUILDERS[name]()


@functools.lru_cache(maxsize=None)
def reference(name, mode, with_scores=True):
    """tests/fusion_ref.py on the case: (out_id, out_val, count); computed once, not to be written to."""
    c = case(name)
    return fr.fuse_lists(c["ids"], c["scores"] if with_scores else None, c["n_docs"], mode, c["weights"], c["rrf_k"])


# ---------------------------------------------------------------- the end-to-end corpus
E2E = dict(N=200, L=24, V=300, Q=8, Lq=10, depth=50, k=10, params=((0.9, 0.4), (2.0, 1.0)))


def corpus():
    """(doc ids, doc mask, query ids, query mask): 200 short Zipf documents and 8 queries (tests/bm25_cases.py)."""
    from tests import bm25_cases as bc
    ids, mask = bc.main_case(seed=13, N=E2E["N"], L=E2E["L"], V=E2E["V"])
    q_ids, q_mask = bc.query_case(4, E2E["Q"], E2E["Lq"], E2E["V"])
    return ids, mask, q_ids, q_mask
