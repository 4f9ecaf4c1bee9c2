"""NumPy float32 restatement of the rank-fusion rule of include/polus_hip.h (polus_fuse_lists), written from the rule
and not from the kernel, as plain loops: one np.float32 operation per rounding of the rule, in the rule's order."""
import numpy as np

RRF, SUM, MINMAX = 0, 1, 2
MODES = {"rrf": RRF, "sum": SUM, "minmax": MINMAX}
F = np.float32


def kept_columns(ids_row, scores_row, n_docs):
    """The columns of one list row that take part, in order."""
    return [c for c in range(len(ids_row))
            if 0 <= int(ids_row[c]) < n_docs and (scores_row is None or np.isfinite(scores_row[c]))]


def contribution(mode, w, rrf_k, rank, s, lo, hi):
    """One kept entry's f32 contribution; every np.float32 operation is one rounding."""
    if mode == RRF:
        return F(w) / (F(rrf_k) + F(rank))
    if mode == SUM:
        return F(w) * F(s)
    if hi == lo:
        return F(w) * F(1.0)
    return F(w) * ((F(s) - F(lo)) / (F(hi) - F(lo)))


def fuse_lists(ids, scores, n_docs, mode, weights=None, rrf_k=60.0):
    """(out_id int32 [Q, L*C], out_val f32 [Q, L*C], count int32 [Q]) from ids int32 [L, Q, C] and scores f32 [L, Q, C]
    (None under rrf): the distinct kept ids of each query ascending with their fused scores, then (-1, -inf)."""
    mode = MODES.get(mode, mode)
    ids = np.asarray(ids)
    L, Q, C = ids.shape
    w = np.ones(L, F) if weights is None else np.asarray(weights, F)
    out_id = np.full((Q, L * C), -1, np.int32)
    out_val = np.full((Q, L * C), -np.inf, F)
    count = np.zeros(Q, np.int32)
    with np.errstate(all="ignore"):
        for r in range(Q):
            fused = {}
            for l in range(L):
                srow = None if scores is None else scores[l, r]
                cols = kept_columns(ids[l, r], srow, n_docs)
                lo = hi = None
                if mode == MINMAX and cols:
                    lo, hi = min(srow[c] for c in cols), max(srow[c] for c in cols)
                for rank, c in enumerate(cols, 1):
                    v = contribution(mode, w[l], rrf_k, rank, None if srow is None else srow[c], lo, hi)
                    d = int(ids[l, r, c])
                    fused[d] = F(fused[d] + v) if d in fused else F(v)
            for m, d in enumerate(sorted(fused)):
                out_id[r, m], out_val[r, m] = d, fused[d]
            count[r] = len(fused)
    return out_id, out_val, count


def topk(out_id, out_val, k):
    """The selection rule of polus_topk_merge_ids over a fused row: score descending, ties to the lower id, NaN, -inf and
    negative ids dropped, the tail (-inf, -1).  Returns (values f32 [Q, k], ids int32 [Q, k])."""
    Q = out_id.shape[0]
    val = np.full((Q, k), -np.inf, F)
    idx = np.full((Q, k), -1, np.int32)
    for r in range(Q):
        rows = [(float(v), int(d)) for v, d in zip(out_val[r], out_id[r]) if d >= 0 and not np.isnan(v) and v != -np.inf]
        rows.sort(key=lambda vd: (-vd[0], vd[1]))
        for m, (v, d) in enumerate(rows[:k]):
            val[r, m], idx[r, m] = F(v), d               # float(f32) and back is exact
    return val, idx
