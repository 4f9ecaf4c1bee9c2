"""float64 NumPy references of the SPLADE path: the four kernels of polus_amd/csrc/splade.hip, the model (oracle.bert
encoder + the masked-LM head of tests/mlm_ref.py + pooling) and the trainer's objective."""
import numpy as np

from tests import mlm_ref as mr


def pool_fwd(x, mask=None):
    """x [B, S, V], mask [B, S] or None -> (rep, xmax, arg) of polus_splade_pool_fwd: the lowest s attaining the
    maximum over the valid tokens; no valid token or a maximum <= 0 gives (0, 0, -1)."""
    x = np.asarray(x, np.float64)
    B, S, V = x.shape
    valid = np.ones((B, S), bool) if mask is None else np.asarray(mask) != 0
    xm = np.where(valid[:, :, None], x, -np.inf)
    arg = xm.argmax(1)                                         # the first maximum
    m = np.take_along_axis(xm, arg[:, None, :], 1)[:, 0, :]
    won = m > 0
    xmax = np.where(won, m, 0.0)
    return np.log1p(xmax), xmax, np.where(won, arg, -1).astype(np.int32)


def pool_bwd(drep, xmax, arg, S):
    """dlogits [B, S, V] float64."""
    g = np.asarray(drep, np.float64) / (1.0 + np.asarray(xmax, np.float64))
    return np.where(np.arange(S)[None, :, None] == np.asarray(arg)[:, None, :], g[:, None, :], 0.0)


def pool_bwd_f32(drep, xmax, arg, S):
    """The kernel's arithmetic in NumPy f32: f32(drep) / f32(1 + xmax), before the one rounding to the storage type."""
    g = np.asarray(drep, np.float32) / (np.float32(1) + np.asarray(xmax, np.float32))
    return np.where(np.arange(S)[None, :, None] == np.asarray(arg)[:, None, :], g[:, None, :], np.float32(0)).astype(np.float32)


def flops_reg(rep, lam):
    """(value, gradient) of lam * sum_v (mean_b rep[b, v])^2."""
    rep = np.asarray(rep, np.float64)
    mean = rep.mean(0)
    return lam * float((mean ** 2).sum()), np.broadcast_to(lam * (2.0 / rep.shape[0]) * mean, rep.shape).copy()


def sparse_scores(q, ids, w):
    """(score [B, N], sum |w q| [B, N]) with ids outside [0, V) skipped."""
    q, w, ids = np.asarray(q, np.float64), np.asarray(w, np.float64), np.asarray(ids, np.int64)
    V = q.shape[1]
    ok = (ids >= 0) & (ids < V)
    g = q[:, np.where(ok, ids, 0)] * np.where(ok, w, 0.0)[None]          # [B, N, M]
    return g.sum(-1), np.abs(g).sum(-1)


def truncate(rep, terms):
    """The (ids, weights) [n, terms] SparseCorpusIndex.add keeps: weight descending, ties to the lower term id."""
    rep = np.asarray(rep)
    order = np.lexsort((np.arange(rep.shape[1])[None].repeat(rep.shape[0], 0), -rep), axis=1)[:, :terms]
    return order.astype(np.int32), np.take_along_axis(rep, order, 1)


def rank(scores, k):
    """(values, ids) [Q, k]: score descending, ties to the lower id."""
    scores = np.asarray(scores)
    order = np.lexsort((np.arange(scores.shape[1])[None].repeat(scores.shape[0], 0), -scores), axis=1)[:, :k]
    return np.take_along_axis(scores, order, 1), order.astype(np.int32)


# ------------------------------------------------------------------------------------------------- model
def splade_fwd(p, cfg, ids, mask, token_type=None):
    """(rep [B, V], state): encoder -> masked-LM head on all B S rows -> pooling."""
    from oracle import bert as ob
    B, S = np.asarray(ids).shape
    last, _, cache = ob.bert_fwd(p, cfg, ids, mask, token_type)
    logits, hc = mr.head_fwd(p, last.reshape(B * S, cfg.hidden_size), cfg.layer_norm_eps)
    logits = logits.reshape(B, S, -1)
    rep, xmax, arg = pool_fwd(logits, mask)
    return rep, dict(cache=cache, hc=hc, logits=logits, xmax=xmax, arg=arg, shape=(B, S))


def splade_bwd(drep, p, cfg, state, arg=None):
    """Parameter gradients of sum(drep * rep).  With `arg` (the device's winners, -1 = none) the gradient flows through
    those tokens: the reference's own logit there, floored at 0, stands in for the maximum.  grads["emb.word"] is the
    tied total with its shares beside it, as tests/mlm_ref.py mlm_fwd_bwd gives them."""
    from oracle import bert as ob
    B, S = state["shape"]
    logits = state["logits"]
    if arg is None:
        arg, xmax = state["arg"], state["xmax"]
    else:
        arg = np.asarray(arg)
        at = np.take_along_axis(logits, np.maximum(arg, 0)[:, None, :], 1)[:, 0, :]
        xmax = np.where(arg >= 0, np.maximum(at, 0.0), 0.0)
    dlogits = pool_bwd(drep, xmax, arg, S).reshape(B * S, -1)
    dhm, hg = mr.head_bwd(dlogits, p, state["hc"])
    grads = ob.bert_bwd(dhm.reshape(B, S, cfg.hidden_size), p, cfg, state["cache"])
    dec = hg.pop("decoder")
    grads.update(hg)
    grads["emb.word/embedding"], grads["emb.word/decoder"] = grads["emb.word"], dec
    grads["emb.word"] = grads["emb.word"] + dec
    return grads


def splade_batch(cfg, B, S, seed=21):
    """ids / mask / token types: ragged tails under the mask, one hole."""
    rng = np.random.Generator(np.random.PCG64(seed))
    ids = rng.integers(5, cfg.vocab_size, size=(B, S)).astype(np.int32)
    mask = np.ones((B, S), np.int32)
    for b in range(B):
        mask[b, S - 2 * b:] = 0
    mask[0, S // 2] = 0
    tt = np.zeros((B, S), np.int32)
    tt[:, S // 2:] = 1
    return ids, mask, tt


def objective(rep, B, k, lam_q, lam_d):
    """(loss, contrastive, reg_q, reg_d) of SparseRetrievalTrainer for rep [(2 + k) B, V]: softmax cross-entropy of each
    query's row of [positives | negatives] scores with its own positive as the label, plus the two regularisers."""
    from oracle import losses as ol
    q, docs = rep[:B], rep[B:]
    con, _ = ol.sparse_softmax_xent_fwd(q @ docs.T, np.arange(B))
    rq, rd = flops_reg(q, lam_q)[0], flops_reg(docs, lam_d)[0]
    return float(con) + rq + rd, float(con), rq, rd
