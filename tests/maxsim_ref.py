"""float64 NumPy reference of token-level late interaction (ColBERT MaxSim) and row L2 normalisation
(test infrastructure; the product never imports it).

    score[b, c]     = sum over valid i of max over valid j of <q[b, i], d[c, j]>
    argmax[b, c, i] = the lowest j reaching that max; -1 for an invalid query token or an empty document
"""
import numpy as np


def _ones(mask, shape):
    return np.ones(shape, bool) if mask is None else (np.asarray(mask) != 0)


def sim(q, d):
    """S[b, c, i, j] = <q[b, i], d[c, j]> in float64 (one matrix product; a strided view)."""
    q, d = np.asarray(q, np.float64), np.asarray(d, np.float64)
    B, Lq, E = q.shape
    N, Ld, _ = d.shape
    return (q.reshape(B * Lq, E) @ d.reshape(N * Ld, E).T).reshape(B, Lq, N, Ld).transpose(0, 2, 1, 3)


def maxsim_fwd(q, d, qmask=None, dmask=None, s=None):
    """(score [B, N], argmax int32 [B, N, Lq]); `s` = a precomputed sim(q, d)."""
    B, Lq, _ = q.shape
    N, Ld, _ = d.shape
    qm, dm = _ones(qmask, (B, Lq)), _ones(dmask, (N, Ld))
    s = sim(q, d) if s is None else s
    s = np.where(dm[None, :, None, :], s, -np.inf)
    am = np.argmax(s, axis=3).astype(np.int32)                       # first occurrence = lowest j
    mx = np.max(s, axis=3)
    valid = qm[:, None, :] & dm.any(1)[None, :, None]
    am = np.where(valid, am, -1).astype(np.int32)
    score = np.where(valid, mx, 0.0).sum(2)
    return score, am


def maxsim_bwd(q, d, dscore, argmax):
    """(dq [B, Lq, E], dd [N, Ld, E]) of sum(dscore * score) given the argmax."""
    q, d, dscore = (np.asarray(a, np.float64) for a in (q, d, dscore))
    B, Lq, E = q.shape
    N, Ld, _ = d.shape
    dq, dd = np.zeros_like(q), np.zeros_like(d)
    for b in range(B):
        for c in range(N):
            j = argmax[b, c]
            hit = j >= 0
            if not hit.any():
                continue
            dq[b, hit] += dscore[b, c] * d[c, j[hit]]
            np.add.at(dd[c], j[hit], dscore[b, c] * q[b, hit])
    return dq, dd


def top2_gap(q, d, qmask=None, dmask=None, s=None):
    """[B, N, Lq] gap between the best and the second-best valid document token (inf where there is no second)."""
    N, Ld, _ = d.shape
    dm = _ones(dmask, (N, Ld))
    s = sim(q, d) if s is None else s
    s = np.where(dm[None, :, None, :], s, -np.inf)
    if Ld < 2:
        return np.full(s.shape[:3], np.inf)
    part = -np.partition(-s, 1, axis=3)
    with np.errstate(invalid="ignore"):
        gap = part[..., 0] - part[..., 1]
    return np.where(np.isfinite(gap), gap, np.inf)


def l2norm_fwd(x, eps=1e-12):
    """(y, rnorm): torch.nn.functional.normalize(x, dim=-1, eps) and 1 / max(|x|, eps)."""
    x = np.asarray(x, np.float64)
    n = np.sqrt((x * x).sum(-1, keepdims=True))
    r = 1.0 / np.maximum(n, eps)
    return x * r, r[..., 0]


def l2norm_bwd(x, dy, eps=1e-12):
    """dx of y = normalize(x): (dy - y <y, dy>) / |x| where |x| > eps, dy / eps otherwise."""
    x, dy = np.asarray(x, np.float64), np.asarray(dy, np.float64)
    n = np.sqrt((x * x).sum(-1, keepdims=True))
    y = x / np.maximum(n, eps)
    inner = (dy - y * (y * dy).sum(-1, keepdims=True)) / np.maximum(n, eps)
    return np.where(n > eps, inner, dy / eps)


def error_scales(q, d, qmask=None, dmask=None, floor=0.0):
    """How much the most affected score [B, N] changes, as a fraction of max|score|, under the least visible instance
    of each of these mistakes (the tolerance checks of tests/test_maxsim_cpu.py):
      second_best         one query token of one (query, document) pair takes the second-best document token
                          (counted where the top-two gap exceeds `floor`, the rounding below which either is right);
      masked_doc_token    one masked token of one document is counted as valid (for every query token);
      dropped_query_token one valid token of one query is left out (for every document)."""
    B, Lq, _ = q.shape
    N, Ld, _ = d.shape
    qm, dm = _ones(qmask, (B, Lq)), _ones(dmask, (N, Ld))
    s = sim(q, d)
    score, am = maxsim_fwd(q, d, qmask, dmask, s)
    scale = np.abs(score).max() + 1e-300
    valid = am >= 0
    gap = top2_gap(q, d, qmask, dmask, s)[valid]
    gap = gap[np.isfinite(gap) & (gap > floor)]
    out = {"second_best": float(gap.min() / scale) if gap.size else np.inf}
    # a masked token j of document c counted: score[b, c] gains sum over valid i of max(s_ij - max_i, 0)
    # (an empty document: sum over valid i of s_ij)
    worst = {}
    for b in range(B):
        sb = s[b]                                                   # [N, Lq, Ld]
        mx = np.where(dm[:, None, :], sb, -np.inf).max(2)           # [N, Lq]
        base = np.where(np.isfinite(mx), mx, 0.0)
        gain = np.where(np.isfinite(mx)[..., None], np.maximum(sb - base[..., None], 0.0), sb)
        gain = np.abs((gain * qm[b][None, :, None]).sum(1))         # [N, Ld]
        for c, j in zip(*np.nonzero(~dm)):
            worst[(c, j)] = max(worst.get((c, j), 0.0), gain[c, j])
    w = np.array([v for v in worst.values() if v > 0])
    out["masked_doc_token"] = float(w.min() / scale) if w.size else np.inf
    # a valid query token i of query b dropped: score[b, c] loses max_i (documents with a valid token)
    mxv = np.where(dm[None, :, None, :], s, -np.inf).max(3)         # [B, N, Lq]
    lost = np.where(np.isfinite(mxv), np.abs(mxv), 0.0).max(1)      # [B, Lq]
    lost = lost[qm & (lost > 0)]
    out["dropped_query_token"] = float(lost.min() / scale) if lost.size else np.inf
    return out
