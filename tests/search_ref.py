"""float64 / NumPy reference of corpus search (test infrastructure; the product never imports it): the exact top-k
selection rule of polus_topk_merge, brute-force scoring, and the ranking metrics.

Selection rule, per row: drop candidates whose score is NaN or -inf, order by score descending (IEEE comparison, so
-0.0 == +0.0) with ties to the lower id, keep k, pad with (-inf, -1)."""
import numpy as np

from tests import maxsim_ref


def topk_merge(scores, ids, k, state=None):
    """scores [rows, n] (any float dtype, kept), ids [n] or [rows, n]; `state` = (vals [rows, k'], ids [rows, k'])
    of an earlier call, entries with id < 0 ignored.  Returns (vals [rows, k] in scores' dtype, ids int32 [rows, k])."""
    scores = np.asarray(scores)
    rows = scores.shape[0]
    ids = np.broadcast_to(np.asarray(ids, np.int64), scores.shape)
    out_v = np.full((rows, k), -np.inf, scores.dtype)
    out_i = np.full((rows, k), -1, np.int32)
    for r in range(rows):
        s, i = scores[r], ids[r]
        if state is not None:
            keep = np.asarray(state[1][r]) >= 0
            s = np.concatenate([np.asarray(state[0][r], scores.dtype)[keep], s])
            i = np.concatenate([np.asarray(state[1][r], np.int64)[keep], i])
        ok = ~np.isnan(s) & (s != -np.inf)
        s, i = s[ok] + scores.dtype.type(0), i[ok]                     # + 0: -0.0 comes back as +0.0
        order = np.lexsort((i, -s))[:k]
        out_v[r, :len(order)] = s[order]
        out_i[r, :len(order)] = i[order]
    return out_v, out_i


def topk(scores, k, id0=0):
    scores = np.asarray(scores)
    return topk_merge(scores, id0 + np.arange(scores.shape[1]), k)


def dot_scores(q, d):
    return np.asarray(q, np.float64) @ np.asarray(d, np.float64).T


def maxsim_scores(q, d, qmask=None, dmask=None, block=64):
    """float64 MaxSim scores [Q, N], computed over blocks of documents (the 4-d similarity tensor stays small)."""
    out = np.empty((q.shape[0], d.shape[0]))
    for a in range(0, d.shape[0], block):
        out[:, a:a + block] = maxsim_ref.maxsim_fwd(q, d[a:a + block], qmask, None if dmask is None else dmask[a:a + block])[0]
    return out


def check_against_float64(got_val, got_id, s64, k, t):
    """The three tolerance rules of a search against float64 scores s64 [Q, N] with tolerance t (absolute):
    every returned score within t of the float64 score of the returned id; every document whose float64 score exceeds
    the float64 k-th best by more than 2t is returned; no returned document more than 2t below the k-th best.
    Returns a list of violations (empty = pass)."""
    bad = []
    Q, N = s64.shape
    kk = min(k, N)
    for r in range(Q):
        ids = got_id[r]
        real = ids[ids >= 0]
        if len(real) != kk or len(set(real.tolist())) != kk or (ids[kk:] != -1).any():
            bad.append((r, "ids", ids.tolist()))
            continue
        kth = np.sort(s64[r])[::-1][kk - 1]
        err = np.abs(got_val[r, :kk].astype(np.float64) - s64[r, real])
        if err.max() > t:
            bad.append((r, "score", float(err.max())))
        must = np.nonzero(s64[r] > kth + 2 * t)[0]
        if not set(must.tolist()) <= set(real.tolist()):
            bad.append((r, "missing", sorted(set(must.tolist()) - set(real.tolist()))))
        if (s64[r, real] < kth - 2 * t).any():
            bad.append((r, "intruder", real[s64[r, real] < kth - 2 * t].tolist()))
    return bad


def recall_at_k(ranked, relevant, k):
    vals = []
    for row, rel in zip(np.asarray(ranked)[:, :k], relevant):
        rel = set(int(x) for x in rel)
        vals.append(len(rel & set(int(x) for x in row if x >= 0)) / len(rel))
    return float(np.mean(vals))


def mrr_at_k(ranked, relevant, k):
    vals = []
    for row, rel in zip(np.asarray(ranked)[:, :k], relevant):
        rel = set(int(x) for x in rel)
        hit = [i for i, x in enumerate(row, 1) if int(x) in rel and x >= 0]
        vals.append(1.0 / hit[0] if hit else 0.0)
    return float(np.mean(vals))


def ndcg_at_k(ranked, relevant, k):
    vals = []
    for row, rel in zip(np.asarray(ranked)[:, :k], relevant):
        gains = dict(rel) if isinstance(rel, dict) else {int(x): 1.0 for x in rel}
        dcg = sum(gains.get(int(x), 0.0) / np.log2(i + 1) for i, x in enumerate(row, 1) if x >= 0)
        ideal = sorted(gains.values(), reverse=True)[:k]
        idcg = sum(g / np.log2(i + 1) for i, g in enumerate(ideal, 1))
        vals.append(dcg / idcg)
    return float(np.mean(vals))
