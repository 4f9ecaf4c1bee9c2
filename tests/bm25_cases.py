"""Cases and bounds of the BM25 / mining tests (tests/test_bm25_cpu.py, tests/test_bm25_gpu.py).  NumPy only.

The float64 bound of test (b).  The index computes a score as polus_sparse_scores over (q, terms, w); against the
textbook formula in exact arithmetic every summand q[t] w[d, t] carries ten f32 roundings, each of relative size at
most u = 2^-24:
  two on the constants c0 = f32(k1 (1 - b)) and c1 = f32(k1 b / avgdl) (they enter K = c1 len + c0, a sum of
      non-negative terms, and K enters w through tf / (tf + K): a relative error of K moves w by at most as much);
  five in w: c1 * len, + c0, tf * k1p1, tf + K, and the division;
  one on k1p1 = f32(k1 + 1);
  two in q: idf = f32(idf64) and tf_q * idf.
To first order that is 10 u per summand.  The sum itself is an fma chain of at most ceil(M / 64) steps per lane and a
six-level tree, far fewer than the M + 1 operations gamma_{M+1} allows for, and every summand is non-negative, so the
summation error is at most gamma_{M+1} times the score.  Bound: (gamma_{M+1} + 10 u) * score, gamma as in
tests/splade_cases.py."""
import numpy as np

from tests.splade_cases import gamma

MAIN = dict(N=200, L=40, V=500, M=16, head=1, tail=1)
PARAMS = ((0.9, 0.4), (1.2, 0.75), (1.2, 0.0), (0.0, 0.75))
TERM_L = (1, 2, 63, 64, 65, 257, 2048)
MINE_C, MINE_K, MINE_P = (1, 63, 64, 65, 200, 1500), (1, 8, 64, 100), (0, 1, 3, 40)


def score_bound(M):
    """Relative bound of an index score against the float64 textbook score (derivation above)."""
    return gamma(M + 1) + 10 * 2.0 ** -24


def zipf_ids(rng, shape, V, s=1.1):
    """ids with probability proportional to rank^-s, rank 1 = id 0."""
    p = np.arange(1, V + 1, dtype=np.float64) ** -s
    return rng.choice(V, size=shape, p=p / p.sum()).astype(np.int32)


def main_case(seed=5, N=MAIN["N"], L=MAIN["L"], V=MAIN["V"]):
    """(ids int32 [N, L], mask int32 [N, L]): Zipf ids, prefix masks of lengths uniform in 0..L with rows of length 0, 2
    and L forced, one mask hole, one id >= V and one negative id among the counted tokens."""
    rng = np.random.Generator(np.random.PCG64(seed))
    ids = zipf_ids(rng, (N, L), V)
    lens = rng.integers(0, L + 1, size=N)
    lens[0], lens[1], lens[2] = 0, 2, L
    if N > 4:
        lens[3], lens[4] = L, L
    mask = (np.arange(L)[None] < lens[:, None]).astype(np.int32)
    if N > 4 and L >= 8:
        mask[2, L // 2] = 0               # a hole: the tokens behind it move up one rank
        ids[3, 3] = V                     # rejected (inside the strip's remainder)
        ids[4, 5] = -7                    # rejected
    return ids, mask


def main_conditions(ids, mask, V, M, head, tail):
    """What the main case must show before anything is compared: (truncated documents, documents with a count above 1,
    empty documents, rejected tokens)."""
    from tests import bm25_ref as br
    trunc = multi = empty = rejected = 0
    for r in range(len(ids)):
        kept, rej = br.remaining_tokens(ids[r], mask[r], V, head, tail)
        rejected += rej
        empty += len(kept) == 0
        vals, cnt = np.unique(kept, return_counts=True) if kept else (np.array([]), np.array([0]))
        trunc += len(vals) > M
        multi += cnt.max() > 1
    return trunc, multi, empty, rejected


def query_case(seed, Q, Lq, V):
    """Short Zipf queries with prefix masks of 3..Lq tokens (the strip takes two)."""
    rng = np.random.Generator(np.random.PCG64(100 + seed))
    ids = zipf_ids(rng, (Q, Lq), V, s=0.7)
    lens = rng.integers(min(3, Lq), Lq + 1, size=Q)
    return ids, (np.arange(Lq)[None] < lens[:, None]).astype(np.int32)


MINE_TARGETS = ("zero", "below", "equal", "one_more", "many")


def mine_case(C, k, P, seed=0):
    """One launch of polus_mine_negatives: (cand int32 [Q, C], score f32 [Q, C], exclude int32 [Q, P] or None, skip_top,
    min_score).  One row per target pool size R = 0, k - 1, k, k + 1 and "as many as there are" (each capped by the
    columns the row has).  Columns below skip_top look like good candidates; the other columns that must fail do so in
    turn by a negative id, an excluded id (while the exclude row has room), a score equal to min_score, a NaN score and
    a lower score.  The exclude row also holds an id absent from the row, a repeated entry and -1 padding."""
    rng = np.random.Generator(np.random.PCG64(1000 * C + 10 * k + P + seed))
    skip_top = (0, 3)[(C + k + P) % 2] if C > 3 else 0
    min_score = np.float32(0.5)
    want = {"zero": 0, "below": max(k - 1, 0), "equal": k, "one_more": k + 1, "many": C}
    Q = len(MINE_TARGETS)
    cand = np.stack([rng.permutation(3 * C)[:C] for _ in range(Q)]).astype(np.int32)
    score = (1.0 + rng.random((Q, C))).astype(np.float32)
    exclude = np.full((Q, P), -1, np.int32) if P else None
    for r, name in enumerate(MINE_TARGETS):
        eligible = np.arange(skip_top, C)
        keep = set(rng.choice(eligible, size=min(want[name], len(eligible)), replace=False).tolist()) if len(eligible) else set()
        banned, kind = [], 0
        room = max(P - 2, 0)              # two slots go to the absent id and the repeat
        for c in eligible:
            if c in keep:
                continue
            while True:
                kind = (kind + 1) % 5
                if kind != 1 or len(banned) < room:
                    break
            if kind == 0:
                cand[r, c] = -1 - (c % 3)
            elif kind == 1:
                banned.append(int(cand[r, c]))
            elif kind == 2:
                score[r, c] = min_score
            elif kind == 3:
                score[r, c] = np.nan
            else:
                score[r, c] = np.float32(0.25)
        if P:
            row = banned + [3 * C + 5]                   # an id no row holds
            if len(row) < P:
                row.append(row[0])                       # a repeated entry
            exclude[r, :len(row)] = row[:P]
            exclude[r] = exclude[r][rng.permutation(P)]
    return cand, score, exclude, skip_top, min_score
