"""float64 NumPy references of the masked-LM path: the vocabulary-wide cross-entropy with ignored rows, the row gather /
scatter, and an f32 restatement of the loss kernel's arithmetic (the tolerance meta-test of test_mlm_cpu.py)."""
import numpy as np


def xent_wide(x, labels):
    """x [R, V] float64, labels int [R]: (loss, dlogits, counted, rejected) of polus_softmax_xent_wide.  Rows with a label
    outside [0, V) add nothing and get a zero gradient row; label >= V is counted in `rejected`."""
    x = np.asarray(x, np.float64)
    labels = np.asarray(labels, np.int64)
    R, V = x.shape
    keep = (labels >= 0) & (labels < V)
    counted, rejected = int(keep.sum()), int((labels >= V).sum())
    n = max(counted, 1)
    d = np.zeros_like(x)
    loss = 0.0
    for r in np.nonzero(keep)[0]:
        mx = x[r].max()
        e = np.exp(x[r] - mx)
        se = e.sum()
        loss += (mx + np.log(se)) - x[r, labels[r]]
        p = e / se
        p[labels[r]] -= 1.0
        d[r] = p / n
    return loss / n, d, counted, rejected


def xent_wide_f32(x, labels, drop_last_column=False, wrong_count=False):
    """The kernel's arithmetic restated in f32 NumPy: max, sum of expf(x - max), logf, gradient exp((x - max) - log(sum)),
    everything divided by max(counted, 1).  The two switches plant the faults the bounds must see: the row's last column
    left out of max / sum / gradient, and the mean taken over all rows instead of the counted ones."""
    f = np.float32
    x = np.asarray(x, f)
    labels = np.asarray(labels, np.int64)
    R, V = x.shape
    keep = (labels >= 0) & (labels < V)
    n = f(R if wrong_count else max(int(keep.sum()), 1))
    W = V - 1 if drop_last_column else V
    d = np.zeros_like(x)
    loss = f(0)
    for r in np.nonzero(keep)[0]:
        row = x[r, :W]
        mx = row.max() if W else f(0)
        se = np.exp(row - mx, dtype=f).sum(dtype=f) if W else f(1)
        lz = np.log(se, dtype=f)
        loss = f(loss + (lz - (x[r, labels[r]] - mx)))
        g = np.exp((row - mx) - lz, dtype=f)
        d[r, :W] = g
        if labels[r] < W:
            d[r, labels[r]] -= f(1)
        d[r, :W] = d[r, :W] * (f(1) / n)
    return float(loss / n), d


def gather_rows(x, idx):
    x = np.asarray(x)
    y = np.zeros((len(idx),) + x.shape[1:], x.dtype)
    for i, j in enumerate(idx):
        if 0 <= j < x.shape[0]:
            y[i] = x[j]
    return y


def scatter_rows(dy, idx, rows):
    """dense [rows, H]: row idx[i] = dy[i] in order of i (the last of a repeated target wins), zeros elsewhere."""
    dy = np.asarray(dy)
    out = np.zeros((rows,) + dy.shape[1:], dy.dtype)
    for i, j in enumerate(idx):
        if 0 <= j < rows:
            out[j] = dy[i]
    return out


# ------------------------------------------------------------------------------------------------- head and whole model
def head_fwd(p, hm, eps=1e-12):
    """The masked-LM head of HF BertForMaskedLM on gathered rows hm [R, H]: Dense(gelu) -> LayerNorm -> decoder against the
    word table + bias.  p: emb.word, mlm.dense.{w,b}, mlm.ln.{g,b}, mlm.bias."""
    from oracle import bert as ob
    u = ob.linear_fwd(hm, p["mlm.dense.w"], p["mlm.dense.b"])
    a = ob.gelu(u)
    t, mean, rstd = ob.layer_norm_fwd(a, p["mlm.ln.g"], p["mlm.ln.b"], eps)
    logits = ob.linear_fwd(t, p["emb.word"], p["mlm.bias"])
    return logits, (hm, u, a, t, mean, rstd)


def head_bwd(dlogits, p, cache):
    """(dhm, grads): grads has the head's five tensors and "decoder", the decoder's share dlogits^T t of emb.word's gradient."""
    from oracle import bert as ob
    hm, u, a, t, mean, rstd = cache
    dt, dtable, dbias = ob.linear_bwd(dlogits, t, p["emb.word"])
    da, dg, db = ob.layer_norm_bwd(dt, a, p["mlm.ln.g"], mean, rstd)
    du = da * ob.gelu_grad(u)
    dhm, dw, dbd = ob.linear_bwd(du, hm, p["mlm.dense.w"])
    return dhm, {"mlm.dense.w": dw, "mlm.dense.b": dbd, "mlm.ln.g": dg, "mlm.ln.b": db, "mlm.bias": dbias, "decoder": dtable}


def flat_positions(positions, S):
    positions = np.asarray(positions, np.int64)
    return np.where(positions >= 0, positions + np.arange(positions.shape[0])[:, None] * S, -1).reshape(-1)


def mlm_fwd_bwd(p, cfg, ids, mask, token_type, positions, labels):
    """Whole model: oracle.bert encoder -> gather -> head -> wide loss, and back.  Returns (loss, logits [B, P, V], grads);
    grads["emb.word"] is the TIED total, with its two shares beside it as "emb.word/embedding" and "emb.word/decoder"."""
    from oracle import bert as ob
    B, S = np.asarray(ids).shape
    H = cfg.hidden_size
    last, _, cache = ob.bert_fwd(p, cfg, ids, mask, token_type)
    flat = flat_positions(positions, S)
    hm = gather_rows(last.reshape(B * S, H), flat)
    logits, hc = head_fwd(p, hm, cfg.layer_norm_eps)
    loss, dlogits, _, _ = xent_wide(logits, np.asarray(labels).reshape(-1))
    dhm, hg = head_bwd(dlogits, p, hc)
    dlast = scatter_rows(dhm, flat, B * S).reshape(B, S, H)
    grads = ob.bert_bwd(dlast, p, cfg, cache)
    dec = hg.pop("decoder")
    grads.update(hg)
    grads["emb.word/embedding"], grads["emb.word/decoder"] = grads["emb.word"], dec
    grads["emb.word"] = grads["emb.word"] + dec
    return loss, logits.reshape(B, -1, logits.shape[-1]), grads


def mlm_params(cfg, seed=5):
    """Seeded float64 parameters of encoder + head; LayerNorm gains and every bias carry signal."""
    from oracle import bert as ob
    p = ob.init_params(cfg, seed=1234, dtype=np.float64)
    rng = np.random.Generator(np.random.PCG64(seed))
    H, V = cfg.hidden_size, cfg.vocab_size
    p["mlm.dense.w"] = np.clip(rng.standard_normal((H, H)), -2, 2) * 0.05
    p["mlm.dense.b"] = np.zeros(H)
    p["mlm.ln.g"], p["mlm.ln.b"] = np.ones(H), np.zeros(H)
    p["mlm.bias"] = np.zeros(V)
    for k in p:
        if k.endswith(".g"):
            p[k] = p[k] + 0.1 * rng.standard_normal(p[k].shape)
        elif k.endswith(".b") or k == "mlm.bias":
            p[k] = 0.05 * rng.standard_normal(p[k].shape)
    return {k: np.asarray(v, np.float64) for k, v in p.items()}


def mlm_batch(cfg, B, S, P, seed=11):
    """ids / mask / token types / positions / labels with one sequence without a masked position and one with a padded
    tail under the attention mask."""
    rng = np.random.Generator(np.random.PCG64(seed))
    V = cfg.vocab_size
    ids = rng.integers(5, V, size=(B, S)).astype(np.int32)
    mask = np.ones((B, S), np.int32)
    mask[B - 1, S - 5:] = 0
    tt = np.zeros((B, S), np.int32)
    tt[:, S // 2:] = 1
    pos = np.full((B, P), -1, np.int32)
    lab = np.full((B, P), -1, np.int32)
    for b in range(B):
        if b == 1:
            continue                                   # no masked position in this sequence
        k = P if b == 0 else max(1, P - 2)
        n = S - 5 if b == B - 1 else S
        pos[b, :k] = np.sort(rng.choice(n, size=k, replace=False))
        lab[b, :k] = rng.integers(5, V, size=k)
        ids[b, pos[b, :k]] = 4
    return ids, mask, tt, pos, lab


HF_LAYER_NAMES = [("attention.output.dense.weight", "out.w"), ("attention.output.dense.bias", "out.b"),
                  ("attention.output.LayerNorm.weight", "ln1.g"), ("attention.output.LayerNorm.bias", "ln1.b"),
                  ("intermediate.dense.weight", "ffn1.w"), ("intermediate.dense.bias", "ffn1.b"),
                  ("output.dense.weight", "ffn2.w"), ("output.dense.bias", "ffn2.b"),
                  ("output.LayerNorm.weight", "ln2.g"), ("output.LayerNorm.bias", "ln2.b")]


def hf_state(cfg, p, tied=True, with_head=True):
    """The state dict HF BertForMaskedLM would save for parameters p (f32), decoder included."""
    H = cfg.hidden_size
    f = lambda a: np.ascontiguousarray(np.asarray(a, np.float32))
    st = {"bert.embeddings.word_embeddings.weight": f(p["emb.word"]), "bert.embeddings.position_embeddings.weight": f(p["emb.pos"]),
          "bert.embeddings.token_type_embeddings.weight": f(p["emb.type"]), "bert.embeddings.LayerNorm.weight": f(p["emb.ln.g"]),
          "bert.embeddings.LayerNorm.bias": f(p["emb.ln.b"])}
    for i in range(cfg.num_hidden_layers):
        q, o = f"bert.encoder.layer.{i}.", f"layer{i}."
        for j, n in enumerate(("query", "key", "value")):
            st[q + f"attention.self.{n}.weight"] = f(p[o + "qkv.w"][j * H:(j + 1) * H])
            st[q + f"attention.self.{n}.bias"] = f(p[o + "qkv.b"][j * H:(j + 1) * H])
        for hf, ours in HF_LAYER_NAMES:
            st[q + hf] = f(p[o + ours])
    if with_head:
        st["cls.predictions.transform.dense.weight"], st["cls.predictions.transform.dense.bias"] = f(p["mlm.dense.w"]), f(p["mlm.dense.b"])
        st["cls.predictions.transform.LayerNorm.weight"], st["cls.predictions.transform.LayerNorm.bias"] = f(p["mlm.ln.g"]), f(p["mlm.ln.b"])
        st["cls.predictions.bias"] = f(p["mlm.bias"])
        dec = f(p["emb.word"]).copy()
        if not tied:
            dec[3, 2] += 1.0
        st["cls.predictions.decoder.weight"] = dec
    return st


def write_hf_checkpoint(path, cfg, p, **kw):
    """config.json + model.safetensors of a tiny HF BertForMaskedLM directory under `path`."""
    import json
    import os
    from safetensors.numpy import save_file
    os.makedirs(path, exist_ok=True)
    with open(os.path.join(path, "config.json"), "w") as f:
        json.dump({"vocab_size": cfg.vocab_size, "hidden_size": cfg.hidden_size, "num_hidden_layers": cfg.num_hidden_layers,
                   "num_attention_heads": cfg.num_attention_heads, "intermediate_size": cfg.intermediate_size,
                   "max_position_embeddings": cfg.max_position_embeddings, "type_vocab_size": cfg.type_vocab_size,
                   "layer_norm_eps": cfg.layer_norm_eps, "hidden_dropout_prob": 0.0, "attention_probs_dropout_prob": 0.0}, f)
    save_file(hf_state(cfg, p, **kw), os.path.join(path, "model.safetensors"))
    return path
