"""NumPy float32 restatement of the refine score rule (include/polus_hip.h "refine", polus_cls_rerank): bit for bit what the
kernel computes, every operation one float32 rounding.

    features in groups of 8 consecutive ones; partial l = 0 .. 63 adds, from +0.0 and in ascending e, fl(q_e * d_e) for
    every e with (e div 8) mod 64 == l; six rounds p_l = fl(p_l + p_(l xor o)), o = 32, 16, 8, 4, 2, 1; the score is p_0.

The FP8 route goes through tests/fp8_ref.py: the same sum over f32(q_e) * f32(code_e), then fl(scale * sum)."""
import numpy as np

from tests import fp8_ref

f32 = np.float32
LANES, GROUP = 64, 8


def pair_scores(q, d):
    """f32 [...]: the rule's score of every pair of rows q [..., E] and d [..., E] (float32 values; broadcast)."""
    q, d = np.asarray(q, f32), np.asarray(d, f32)
    E = q.shape[-1]
    assert E % GROUP == 0 and d.shape[-1] == E
    prod = (q * d).astype(f32)                                       # one rounding per product
    G = E // GROUP
    prod = prod.reshape(prod.shape[:-1] + (G, GROUP))
    p = np.zeros(prod.shape[:-2] + (LANES,), f32)
    for g0 in range(0, G, LANES):                                    # lane l: groups l, l + 64, ... in ascending e
        n = min(LANES, G - g0)
        for i in range(GROUP):
            p[..., :n] = p[..., :n] + prod[..., g0:g0 + n, i]
    lane = np.arange(LANES)
    for o in (32, 16, 8, 4, 2, 1):
        p = p + p[..., lane ^ o]
    return p[..., 0]


def scores(q, d):
    """f32 [B, N]: every query against every document."""
    return pair_scores(np.asarray(q, f32)[:, None, :], np.asarray(d, f32)[None, :, :])


def rerank(q, d, cand, scale=None):
    """f32 [B, C]: score of query b and document cand[b, c]; -inf where the id is outside [0, N).  With `scale` (f32 [N]) d
    holds the decoded codes and the sum is multiplied by the document's scale, one more rounding."""
    q, d, cand = np.asarray(q, f32), np.asarray(d, f32), np.asarray(cand, np.int64)
    N = d.shape[0]
    ok = (cand >= 0) & (cand < N)
    at = np.where(ok, cand, 0)
    s = pair_scores(q[:, None, :], d[at])
    if scale is not None:
        s = (np.asarray(scale, f32)[at] * s).astype(f32)
    return np.where(ok, s, f32(-np.inf)).astype(f32)


def rerank_fp8(q, codes, scale, cand):
    """The FP8 route: codes uint8 [N, E] (e4m3fn), scale f32 [N]."""
    return rerank(q, fp8_ref.decode(codes), cand, scale=scale)


def quantize(x):
    """(codes uint8 [N, E], scale f32 [N]) of float32 rows: tests/fp8_ref.py's rule on whole rows."""
    codes, scale, _ = fp8_ref.quantize(x)
    return codes, scale


def exact(q, d):
    """float64 [B, N]."""
    return np.asarray(q, np.float64) @ np.asarray(d, np.float64).T
