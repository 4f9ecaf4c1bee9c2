"""GPU: the cross-encoder against the float64 oracle (oracle.bert bert_fwd / pooler_fwd / pooler_bwd / bert_bwd + a
linear head over the reference's pair rows): model scores, one CrossEncoderTrainer step under every loss, the head's
dropout, CrossEncoderIndex with and without bucketing, rerank, TwoStageSearch and the checkpoint import.

Tolerances are tests/test_model_gpu.TOLS, the project's figures for a Dense head over the same small models against
the same oracle, relative to max|reference| (tests/util.relerr).

Conditioning.  The bounds are relative to max|reference|, which says something only where the reference is not what is
left of a cancellation.  All figures below come from the float64 oracle alone.

Scores.  The golden parameters are an initialisation (matrices of std 0.02): through two such layers the [CLS] state
hardly depends on the text and all scores lie within 0.42 +- 0.01, so a model that ignored the document would pass.  The
encoder matrices are the golden ones times SHARPEN = 6: attention logits of std 1.9 instead of 0.05, what a trained
model has, and scores that spread over 2.3 .. 4.0.  A score is ONE 128-term sum per pair and a test sees 9 to 18 of them,
where TOLS["logits"] was set on the largest of hundreds of token logits: what an independent relative error of the
features does to such a sum, over the scale the tolerance is taken of, is sqrt(sum_i (w_i x_i)^2) / max|score| = 0.42,
0.51 and 0.37 for the three golden heads and 2.0 for a zero-mean classifier over these few pairs.  The classifier's bias
is HEAD_BIAS = 3 (a reranker's scores are not centred on zero either), and every score check first requires the ratio
to be at most the golden heads' worst, 0.51.

Gradients.  Under a softmax-type loss every row of dscore sums to zero, so each parameter gradient sum_p ds_p G_p keeps
only what DIFFERS between the pairs of a query.  With the golden matrices and a pooler in its linear range (weights of
std 0.05) G_p is nearly the same vector for every pair: the per-pair terms add up to 69 x (contrastive) and 81 x (KL) the
result for the worst tensor and 26 x for the median one.  HF's pooler saturates; with POOLER_STD = 0.3
ROUNDINGS = 12                # stored bf16 tensors between a pair's ids and its score, at least (pre-activations
of std 3) tanh' differs from pair to pair, and with the sharpened attention the pairs themselves differ: the worst
ratios are 5.6 and 4.8.  What bf16 can deliver is the ratio times a pair's own error, and between a pair's ids and its
score the two-layer engine stores at least ROUNDINGS = 12 bf16 tensors (the embedding output; per layer the fused
projections, the context, the two LayerNorm outputs and the activated FFN state; the pooled state), each good to 2^-9, whose
independent errors add as the square root.  _check_grads recomputes the ratio of every tensor in the oracle (one backward
per pair) and, for the bf16 runs, requires sqrt(12) x 2^-9 x ratio <= the tolerance (ratio <= 8.9), so the data cannot
drift to where the bound is out of the format's reach.  Measured on an MI355X before the data met that: misses of 0.12 ..
0.18 at ratio 69 .. 81 and of 6.5e-2 .. 7.8e-2 at ratio 11.6 .. 12.4, against 1.2e-5 for the same steps in f32 and 1.6e-2 in
bf16 under PointwiseBCELoss, whose terms add without cancelling.  classifier.b's gradient is sum_p ds_p, exactly zero
under those losses: it is held to the same tolerance of sum_p |ds_p|, as tests/test_boundary_gpu.py holds the vanishing
bias gradient of its contrastive step."""
import numpy as np
import pytest
import torch

from oracle import bert as ob
from oracle import losses as ol
from tests import pair_ref as pr
from tests import tuple_ref as tr
from tests.test_model_gpu import TOLS, _oracle_drop, load_case
from tests.tuple_cases import TOL as TUPLE_TOL
from tests.util import assert_close, host, relerr

pytestmark = pytest.mark.gpu
CLS, SEP, PAD = 1, 2, 0
SP = (CLS, SEP, PAD)
STRIP4 = (1, 1, 1, 1)
SHARPEN = 6.0                 # see "Conditioning" above
BF16_EPS = 2.0 ** -9          # half an ulp of a stored bf16 activation, relative
HEAD_BIAS = 3.0               # see "Conditioning"
POOLER_STD = 0.3
ROUNDINGS = 12                # stored bf16 tensors between a pair's ids and its score, at least
HEAD_CONDITION = 0.51         # the worst of the golden token-classifier heads TOLS["logits"] was set on


def _params(case):
    """(oracle config, float64 parameters in the model's names), host only: the golden case's seeded encoder, sharpened,
    plus a seeded pooler and classifier."""
    _, ocfg, params, _, _ = load_case(case)
    r = np.random.Generator(np.random.PCG64(31))
    H = ocfg.hidden_size
    params = {k: v * SHARPEN if k.startswith("layer") and k.endswith(".w") else v for k, v in params.items()}
    p = dict(params, **{"pooler.w": r.standard_normal((H, H)) * POOLER_STD, "pooler.b": r.standard_normal(H) * 0.05,
                        "classifier.w": r.standard_normal((1, H)) / np.sqrt(H), "classifier.b": np.array([HEAD_BIAS])})
    return ocfg, p


def _model(case, mode, dropout=0.0):
    """(CrossEncoder, oracle config, float64 parameters)."""
    from polus_amd.ir.models import CrossEncoder
    from polus_amd.models import BertConfig
    ocfg, p = _params(case)
    cfg = BertConfig(ocfg.vocab_size, ocfg.hidden_size, ocfg.num_hidden_layers, ocfg.num_attention_heads,
                     ocfg.intermediate_size, ocfg.max_position_embeddings, ocfg.type_vocab_size,
                     hidden_dropout_prob=dropout, attention_probs_dropout_prob=dropout)
    m = CrossEncoder(cfg, compute_dtype=mode)
    m.load_numpy_params(p)
    assert [v.name for v in m.trainable_weights][-4:] == ["pooler.w", "pooler.b", "classifier.w", "classifier.b"]
    return m, ocfg, p


def _texts(ocfg, shape, L, r, lo=2):
    """HF-shaped rows `cls w.. sep pad..`: {"input_ids", "attention_mask"} int32 shape + (L,), lengths in [lo, L]."""
    ids = r.integers(3, ocfg.vocab_size, size=shape + (L,)).astype(np.int32)
    lens = r.integers(lo, L + 1, size=shape)
    col = np.arange(L)
    ids[..., 0] = CLS
    ids = np.where(col == lens[..., None] - 1, SEP, ids)
    mask = (col < lens[..., None]).astype(np.int32)
    return {"input_ids": np.where(mask > 0, ids, PAD).astype(np.int32), "attention_mask": mask}


def _oracle(p, ocfg, rows, drop=None, head_keep=None):
    """float64 scores [P] of the pair rows (ids, types, mask) and what the backward needs."""
    ids, tt, am = rows
    last, _, cache = ob.bert_fwd(p, ocfg, ids, am, tt, drop)
    pooled, pcache = ob.pooler_fwd(last, p["pooler.w"], p["pooler.b"])
    x = pooled if head_keep is None else pooled * head_keep
    s = (x @ p["classifier.w"].T + p["classifier.b"])[:, 0]
    return s, (x, pcache, cache, head_keep, ids.shape[1])


def _oracle_grads(p, ocfg, ds, back):
    x, pcache, cache, head_keep, S = back
    d = np.asarray(ds, np.float64).reshape(-1, 1)
    g = {"classifier.w": d.T @ x, "classifier.b": d.sum(0)}
    dpooled = d @ p["classifier.w"]
    if head_keep is not None:
        dpooled = dpooled * head_keep
    dlast, g["pooler.w"], g["pooler.b"] = ob.pooler_bwd(dpooled, p["pooler.w"], pcache, S)
    g.update(ob.bert_bwd(dlast, p, ocfg, cache))
    return g


def _head_condition(p, back, s):
    """sqrt(sum_i (w_i x_i)^2) of the worst row over max|score|: how much of an independent relative error of the
    pooled features reaches the scores, relative to the scale the tolerance is taken of."""
    rss = np.sqrt(((back[0] * p["classifier.w"]) ** 2).sum(1)).max()
    return float(rss / np.abs(s).max())


def _assert_scores(got, ref, p, back, mode, what):
    cond = _head_condition(p, back, ref)
    print(f"[cross] {what} {mode}: scores rel err {relerr(got, ref):.3e} (max|ref| {np.abs(ref).max():.3f}, head condition {cond:.2f})")
    assert cond <= HEAD_CONDITION, f"{what}: the head is conditioned worse ({cond:.2f}) than the heads TOLS was set on"
    assert_close(got, ref, TOLS[mode]["logits"], f"{what} scores")


@pytest.mark.parametrize("mode", ["f32", "bf16"])
@pytest.mark.parametrize("case,S", [("bert_small_b3_s48", 48), ("bert_base1_b2_s64", 64)])
def test_scores_match_the_oracle(case, S, mode):
    from polus_amd import ops
    m, ocfg, p = _model(case, mode)
    r = np.random.Generator(np.random.PCG64(7))
    q, d = _texts(ocfg, (3,), 12, r), _texts(ocfg, (5,), 40, r)
    cand = np.array([[0, 1, 2, -1], [4, 3, 5, 0], [2, 2, 1, 4]], np.int32)
    ref_rows = pr.pair_pack(q["input_ids"], q["attention_mask"], d["input_ids"], d["attention_mask"], cand, STRIP4, 8, S, SP)
    buf = torch.empty((3, 12, S), dtype=torch.int32, device="cuda")
    dev = lambda a: torch.as_tensor(a).cuda()
    ops.pair_pack(dev(q["input_ids"]), dev(q["attention_mask"]), dev(d["input_ids"]), dev(d["attention_mask"]), dev(cand),
                  buf[0], buf[1], buf[2], STRIP4, 8, SP)
    for k in range(3):
        assert np.array_equal(buf[k].cpu().numpy(), ref_rows[k])
    s = m(input_ids=buf[0], attention_mask=buf[2], token_type_ids=buf[1], training=False)
    assert s.dtype == torch.float32 and tuple(s.shape) == (12,)
    ref, back = _oracle(p, ocfg, ref_rows[:3])
    _assert_scores(host(s), ref, p, back, mode, f"model {case}")
    # the dict protocol of the other models
    s2 = m({"input_ids": buf[0], "attention_mask": buf[2], "token_type_ids": buf[1]}).clone()
    assert torch.equal(s2, m(input_ids=buf[0], attention_mask=buf[2], token_type_ids=buf[1]))
    with pytest.raises(RuntimeError):
        m.backward(torch.zeros(12, device="cuda"))


def _step_data(ocfg, k=2):
    """Host only: a batch (question, positive, negatives [B, k, L]) and the reference's pair rows for it: positives then
    negative block i in one buffer padded to one width, cand[b, j] = j B + b."""
    r = np.random.Generator(np.random.PCG64(13))
    B, Ld = 3, 24
    q, d, neg = _texts(ocfg, (B,), 10, r), _texts(ocfg, (B,), Ld, r), _texts(ocfg, (B, k), 20, r)
    d_ids, d_mask = np.zeros(((1 + k) * B, Ld), np.int32), np.zeros(((1 + k) * B, Ld), np.int32)
    d_ids[:B], d_mask[:B] = d["input_ids"], d["attention_mask"]
    for i in range(k):
        d_ids[(1 + i) * B:(2 + i) * B, :20] = neg["input_ids"][:, i]
        d_mask[(1 + i) * B:(2 + i) * B, :20] = neg["attention_mask"][:, i]
    cand = (np.arange(1 + k)[None, :] * B + np.arange(B)[:, None]).astype(np.int32)
    rows = pr.pair_pack(q["input_ids"], q["attention_mask"], d_ids, d_mask, cand, STRIP4, 6, 32, SP)
    return (q, d, neg), rows[:3], B


def _step_setup(mode, loss, dropout=0.0, k=2):
    from polus_amd.ir.training import CrossEncoderTrainer
    from polus_amd.optimizers import Adam
    m, ocfg, p = _model("bert_small_b3_s48", mode, dropout)
    batch, rows, B = _step_data(ocfg, k)
    t = CrossEncoderTrainer(m, Adam(1e-3), loss, strip=(1, 1), max_query_tokens=6, max_length=32, cls_token_id=CLS,
                            sep_token_id=SEP, pad_token_id=PAD)
    return dict(trainer=t, model=m, ocfg=ocfg, p=p, batch=batch, rows=rows, B=B, k=k)


def _check_step(c, mode, loss, dloss, what):
    """Scores, loss and every gradient of the step just taken against the oracle."""
    t, m, B, k = c["trainer"], c["model"], c["B"], c["k"]
    for i in range(3):
        assert np.array_equal(t.pairs[i].cpu().numpy(), c["rows"][i]), "the trainer's pair rows"
    s_ref, back = _oracle(c["p"], c["ocfg"], c["rows"])
    s_ref = s_ref.reshape(B, 1 + k)
    loss_ref, ds = dloss(s_ref)
    tol = TOLS[mode]
    print(f"[cross] {what} {mode}: loss {loss:.6f} (reference {float(loss_ref):.6f})")
    _assert_scores(host(t.scores), s_ref, c["p"], back, mode, what)
    assert abs(loss - float(loss_ref)) < tol["loss"], (loss, float(loss_ref))
    g_ref = _oracle_grads(c["p"], c["ocfg"], ds, back)
    got = {v.name: host(v.grad) for v in m.trainable_weights}
    assert set(got) == set(g_ref)
    bf16 = mode == "bf16"
    _check_grads(got, g_ref, ds, back, tol["grad"], f"{what} {mode}", c["p"] if bf16 else None, c["ocfg"] if bf16 else None)


def _cancellation(p, ocfg, ds, back, g_ref):
    """{tensor: max sum_p |ds_p G_p| / max |sum_p ds_p G_p|}: how many times its result a gradient adds up."""
    flat = np.asarray(ds, np.float64).reshape(-1)
    total = {n: np.zeros_like(v) for n, v in g_ref.items()}
    for i, v in enumerate(flat):
        one = np.zeros_like(flat)
        one[i] = v
        for n, g in _oracle_grads(p, ocfg, one.reshape(np.shape(ds)), back).items():
            total[n] += np.abs(g)
    return {n: float(total[n].max() / max(np.abs(g_ref[n]).max(), 1e-300)) for n in g_ref}


def _check_grads(got, g_ref, ds, back, tol, what, p=None, ocfg=None):
    """Every gradient within `tol` of the oracle's, relative to max|reference|; with `p` (the bf16 runs) the data must
    first leave bf16 room to meet the bound; see "Conditioning" in the module docstring."""
    d = np.abs(np.asarray(ds, np.float64)).reshape(-1, 1)
    zero_sum = np.abs(np.asarray(ds).sum(1)).max() < 1e-12          # a softmax-type loss: classifier.b's gradient vanishes
    names = [n for n in g_ref if not (zero_sum and n == "classifier.b")]
    if p is not None:
        cancel = _cancellation(p, ocfg, ds, back, g_ref)
        worst = max(names, key=cancel.get)
        print(f"[cross] {what}: the worst-conditioned gradient, {worst}, adds {cancel[worst]:.1f} x its result")
        assert np.sqrt(ROUNDINGS) * BF16_EPS * cancel[worst] <= TOLS["bf16"]["grad"], f"the data leaves bf16 no room: {worst} {cancel[worst]:.0f}"
    errs = {n: relerr(got[n], g_ref[n]) for n in names}
    worst = max(errs, key=errs.get)
    print(f"[cross] {what}: worst gradient rel err {errs[worst]:.3e} ({worst})")
    for n, e in errs.items():
        assert np.isfinite(e) and e <= tol, f"{what}: grad {n}: rel err {e:.3e} > {tol:.1e}"
    if zero_sum:
        assert np.abs(g_ref["classifier.b"]).max() < 1e-12
        assert np.abs(got["classifier.b"]).max() <= tol * d.sum(), (what, got["classifier.b"], d.sum())


@pytest.mark.parametrize("mode", ["f32", "bf16"])
def test_trainer_step_contrastive_matches_the_oracle(mode):
    from polus_amd.ir.training import TupleContrastiveLoss
    c = _step_setup(mode, TupleContrastiveLoss())
    before = c["model"].arena.params.clone()
    loss = float(c["trainer"].train_step(*c["batch"]))
    torch.cuda.synchronize()
    assert c["trainer"].optimizer.iterations == 1 and not torch.equal(before, c["model"].arena.params)
    assert str(c["trainer"]) == "CrossEncoderTrainer" and c["model"].dropout_step == 1
    _check_step(c, mode, loss, lambda s: ol.sparse_softmax_xent_fwd(s, np.zeros(s.shape[0], np.int64)), "contrastive step")
    with pytest.raises(NotImplementedError):
        c["trainer"].enable_step_graph()


@pytest.mark.parametrize("mode", ["f32", "bf16"])
def test_trainer_step_distillation_kl_with_an_absent_teacher_column(mode):
    from polus_amd.ir.training import DistillKLLoss
    c = _step_setup(mode, DistillKLLoss())
    teacher = np.random.Generator(np.random.PCG64(5)).uniform(-2.0, 2.0, size=(3, 3)).astype(np.float32)
    teacher[1, 2] = -np.inf
    loss = float(c["trainer"].train_step(*c["batch"], teacher))
    torch.cuda.synchronize()
    # the loss on the DEVICE scores: the loss kernel's own error only
    on_dev, _ = tr.distill_kl(host(c["trainer"].scores), teacher)
    print(f"[cross] KL step {mode}: loss {loss:.7f}, reference on the device scores {float(on_dev):.7f}")
    assert relerr(loss, on_dev) <= TUPLE_TOL["kl"]["loss"], (loss, on_dev)
    dpos, dneg = c["trainer"].loss.backward()
    assert tuple(dpos.shape) == (3, 1) and tuple(dneg.shape) == (3, 2) and float(dneg[1, 1]) == 0.0
    _check_step(c, mode, loss, lambda s: tr.distill_kl(s, teacher), "KL step")
    with pytest.raises(ValueError):
        c["trainer"].train_step(*c["batch"], teacher[:, :2])
    with pytest.raises(ValueError):
        c["trainer"].train_step(c["batch"][0], c["batch"][1], None, teacher)


def _bce(s):
    """float64 restatement of PointwiseBCELoss: BCE-with-logits against label 1 in column 0, summed over the columns,
    averaged over the rows."""
    y = np.zeros_like(s); y[:, 0] = 1.0
    per = np.maximum(s, 0) - s * y + np.log1p(np.exp(-np.abs(s)))
    return per.sum(1).mean(), (1.0 / (1.0 + np.exp(-s)) - y) / s.shape[0]


@pytest.mark.parametrize("mode", ["f32", "bf16"])
def test_trainer_step_pointwise_bce(mode):
    from polus_amd.ir.training import PointwiseBCELoss
    c = _step_setup(mode, PointwiseBCELoss())
    loss = float(c["trainer"].train_step(*c["batch"]))
    torch.cuda.synchronize()
    # on the device scores: 1e-5 is tests/test_kernels_gpu.py's bound for polus_sigmoid_xent against float64
    on_dev, d_dev = _bce(host(c["trainer"].scores))
    assert abs(loss - on_dev) < 1e-5 * max(1.0, abs(on_dev)), (loss, on_dev)
    assert_close(host(c["trainer"].loss.d), d_dev, 1e-5, "BCE gradient")
    _check_step(c, mode, loss, _bce, "BCE step")


def test_pointwise_bce_without_negatives():
    from polus_amd.ir.training import PointwiseBCELoss
    s = torch.tensor([[0.5], [-1.0]], device="cuda")
    l = PointwiseBCELoss()
    loss = float(l(s, None))
    ref, d = _bce(host(s))
    assert abs(loss - ref) < 1e-5
    dpos, dneg = l.backward()
    assert dneg is None
    assert_close(host(dpos), d, 1e-5, "BCE gradient, k = 0")


def test_head_dropout_matches_the_oracle_with_regenerated_masks():
    """f32, p = 0.1 at every site: the encoder's masks as tests/test_model_gpu.py regenerates them, the head's from
    site 3 of the last layer; scores, loss and every gradient, at twice the dropout-free tolerances as there."""
    from polus_amd import ops
    from polus_amd.ir.training import TupleContrastiveLoss
    p_drop = 0.1
    c = _step_setup("f32", TupleContrastiveLoss(), dropout=p_drop)
    t, m, ocfg = c["trainer"], c["model"], c["ocfg"]
    out = t.forward_with_grads(*c["batch"])
    loss = float(t.loss(*out))
    t.backward_from_loss()
    torch.cuda.synchronize()
    P, S, H = 9, 32, ocfg.hidden_size
    drop = _oracle_drop(m.bert, ocfg, P, S, p_drop, p_drop, 0)
    keep = ops.dropout_mask(m.site_seed(ocfg.num_hidden_layers - 1, 3, 0), p_drop, P * H).cpu().numpy().reshape(P, H)
    assert 0.8 < keep.mean() < 0.97
    s_ref, back = _oracle(c["p"], ocfg, c["rows"], drop, keep.astype(np.float64) / (1.0 - p_drop))
    loss_ref, ds = ol.sparse_softmax_xent_fwd(s_ref.reshape(3, 3), np.zeros(3, np.int64))
    tol = TOLS["f32"]
    print(f"[cross] dropout step: loss {loss:.6f} (reference {float(loss_ref):.6f})")
    assert_close(host(t.scores).reshape(-1), s_ref, tol["logits"] * 2, "scores behind dropout")
    assert abs(loss - float(loss_ref)) < tol["loss"] * 2
    g_ref = _oracle_grads(c["p"], ocfg, ds, back)
    _check_grads({v.name: host(v.grad) for v in m.trainable_weights}, g_ref, ds, back, tol["grad"] * 2, "dropout step")
    # inference ignores the dropout
    clean, _ = _oracle(c["p"], ocfg, c["rows"])
    s = m(input_ids=t.pairs[0], attention_mask=t.pairs[2], token_type_ids=t.pairs[1], training=False)
    assert_close(host(s), clean, tol["logits"], "inference scores")


def test_deterministic_mode_is_bitwise_reproducible():
    from polus_amd.ir.training import TupleContrastiveLoss
    c = _step_setup("bf16", TupleContrastiveLoss(), dropout=0.1)
    t, m = c["trainer"], c["model"]
    m.deterministic = True
    runs, scores = [], []
    for _ in range(2):
        m.dropout_step = 0
        out = t.forward_with_grads(*c["batch"])
        t.loss(*out)
        t.backward_from_loss()
        runs.append(m.arena.grads.clone()); scores.append(t.scores.clone())
    assert torch.equal(runs[0], runs[1]) and torch.equal(scores[0], scores[1])
    assert float(runs[0].abs().max()) > 0
    out = t.forward_with_grads(*c["batch"])                       # the next step draws other masks
    assert not torch.equal(t.scores, scores[0])


def test_gradient_accumulation_adds():
    from polus_amd.ir.training import TupleContrastiveLoss
    c = _step_setup("f32", TupleContrastiveLoss())
    t, m = c["trainer"], c["model"]
    out = t.forward_with_grads(*c["batch"]); t.loss(*out); t.backward_from_loss()
    once = m.arena.grads.clone()
    out = t.forward_with_grads(*c["batch"]); t.loss(*out); t.backward_from_loss(accumulate=True)
    assert_close(host(m.arena.grads), 2 * host(once), 1e-5, "accumulate")


# ---------------------------------------------------------------- index
def _index_data(ocfg):
    """Host only: queries, eight documents in three groups of lengths (so that the pairs fall into buckets of S = 16, 32
    and 64) and candidate rows with a missing column."""
    r = np.random.Generator(np.random.PCG64(17))
    Q, Ld = 3, 46
    q = _texts(ocfg, (Q,), 10, r, lo=4)
    lens = np.array([4, 5, 20, 22, 44, 46, 6, 21])
    col = np.arange(Ld)
    mask = (col < lens[:, None]).astype(np.int32)
    ids = r.integers(3, ocfg.vocab_size, size=(len(lens), Ld))
    ids[:, 0] = CLS
    ids = np.where(col == lens[:, None] - 1, SEP, ids)
    d = {"input_ids": np.where(mask > 0, ids, PAD).astype(np.int32), "attention_mask": mask}
    cand = np.array([[0, 2, 4, -1, 6, 1], [5, 3, 1, -1, 7, 0], [4, 5, 2, -1, 3, 6]], np.int32)
    return q, d, cand


def _index_setup(mode, **kw):
    from polus_amd.ir.cross import CrossEncoderIndex
    m, ocfg, p = _model("bert_small_b3_s48", mode)
    q, d, cand = _index_data(ocfg)
    index = CrossEncoderIndex(m, strip=(1, 1), max_query_tokens=8, max_length=64, cls_token_id=CLS, sep_token_id=SEP,
                              pad_token_id=PAD, tokens_per_batch=256, round_to=16, **kw)
    return dict(index=index, model=m, ocfg=ocfg, p=p, q=q, d=d, cand=cand, Q=3)


def _fill(c):
    index, d = c["index"], c["d"]
    index.doc_tokens = 46
    # rows 0..3 are short enough for a 30-column batch; the rest goes in at full width
    a = index.add({k: v[:4, :30] for k, v in d.items()})
    b = index.add({k: v[4:] for k, v in d.items()})
    assert a.dtype == torch.int32 and a.tolist() == [0, 1, 2, 3] and b.tolist() == [4, 5, 6, 7]
    assert len(index) == 8 and index.nbytes == 8 * 46 * 8
    assert np.array_equal(index.token_ids.cpu().numpy(), d["input_ids"]) and np.array_equal(index.mask.cpu().numpy(), d["attention_mask"])
    with pytest.raises(ValueError):
        index.add({k: np.zeros((1, 47), np.int32) for k in d})
    return index


@pytest.mark.parametrize("mode", ["f32", "bf16"])
def test_index_scores_bucketed_and_not_match_the_oracle(mode):
    from polus_amd import ops
    c = _index_setup(mode)
    index, q, d, cand = _fill(c), c["q"], c["d"], c["cand"]
    rows = pr.pair_pack(q["input_ids"], q["attention_mask"], d["input_ids"], d["attention_mask"], cand, STRIP4, 8, 64, SP)
    ref, back = _oracle(c["p"], c["ocfg"], rows[:3])
    assert _head_condition(c["p"], back, ref) <= HEAD_CONDITION
    ref = ref.reshape(cand.shape)
    present = cand >= 0
    got = {}
    for bucket in (True, False):
        s = index.score(q, cand, bucket=bucket)
        assert s.dtype == torch.float32 and tuple(s.shape) == cand.shape
        h = s.cpu().numpy().astype(np.float64)
        assert np.isneginf(h[~present]).all() and np.isfinite(h[present]).all()
        print(f"[cross] index {mode} bucket={bucket}: rel err {relerr(h[present], ref[present]):.3e}, plan {index.last_plan}")
        assert_close(h[present], ref[present], TOLS[mode]["logits"], f"index scores, bucket={bucket}")
        got[bucket] = (h, list(index.last_plan))
    plan = got[True][1]
    assert len({S for S, _ in plan}) >= 3, plan                     # at least three buckets of different S
    assert sum(n for _, n in plan) == cand.size and all(n * S <= 256 for S, n in plan)
    assert all(S == 64 for S, _ in got[False][1]) and sum(n for _, n in got[False][1]) == cand.size
    # a device tensor of candidates is taken as it is; an id beyond the index is absent too
    dc = torch.as_tensor(cand).cuda()
    dc[0, 0] = 8
    s = index.score(q, dc)
    assert np.isneginf(float(s[0, 0]))
    assert_close(host(s[1:])[present[1:]], ref[1:][present[1:]], TOLS[mode]["logits"], "index scores, device candidates")
    with pytest.raises(ValueError):
        index.score(q, dc.long())
    with pytest.raises(ValueError):
        index.score(q, np.array([[0, 8, 1, 1, 1, 1]] * 3))
    # rerank is topk_merge over score's own matrix
    s = index.score(q, cand)
    tv, ti = torch.empty((3, 4), device="cuda"), torch.empty((3, 4), dtype=torch.int32, device="cuda")
    ops.topk_merge(s, tv, ti, init=True, ids=torch.as_tensor(cand).cuda())
    rv, ri = index.rerank(q, cand, 4)
    assert torch.equal(rv, tv) and torch.equal(ri, ti) and (ri >= 0).all()
    rv, ri = index.rerank(q, cand, 6)
    assert (ri[:, 5] == -1).all() and np.isneginf(rv[:, 5].cpu().numpy()).all()
    index.clear()
    assert len(index) == 0 and index.nbytes == 0


def test_two_stage_search_with_a_cross_encoder_second_stage():
    from polus_amd.ir.models import DualEncoder
    from polus_amd.ir.search import CorpusIndex, TwoStageSearch
    from polus_amd.ir.training import InBatchDotScores
    from polus_amd.models import BertConfig, BertModel
    c = _index_setup("bf16")
    ocfg = c["ocfg"]
    cfg = BertConfig(ocfg.vocab_size, ocfg.hidden_size, ocfg.num_hidden_layers, ocfg.num_attention_heads,
                     ocfg.intermediate_size, ocfg.max_position_embeddings, ocfg.type_vocab_size)
    enc = BertModel(cfg, compute_dtype="bf16")
    enc.load_numpy_params(c["p"])
    first = CorpusIndex(DualEncoder(enc, projection_dim=64, compute_dtype="bf16"), InBatchDotScores())
    two = TwoStageSearch(first, c["index"], candidates=5)
    ids = two.add(c["d"])
    assert ids.tolist() == list(range(8)) and len(two) == 8
    scores, top = two.search(c["q"], 3)
    cand = first.search(c["q"], 5)[1]
    rv, ri = c["index"].rerank(c["q"], cand, 3)
    assert torch.equal(top, ri) and torch.equal(scores, rv)
    assert (top >= 0).all() and all(set(top[b].tolist()) <= set(cand[b].tolist()) for b in range(3))
    # three stages: a two-stage search is a first stage ("anything with search and add")
    three = TwoStageSearch(two, c["index"], candidates=3)
    s3, t3 = three.search(c["q"], 2)
    assert torch.equal(t3, top[:, :2]) and torch.equal(s3, scores[:, :2])


def test_rerank_validation_callback_ranks_with_the_trainers_model():
    from polus_amd.ir.cross import RerankValidationCallback
    from polus_amd.ir.training import CrossEncoderTrainer, TupleContrastiveLoss
    from polus_amd.optimizers import Adam
    c = _index_setup("f32")
    t = CrossEncoderTrainer(c["model"], Adam(1e-3), TupleContrastiveLoss(), strip=(1, 1), max_query_tokens=8, max_length=64,
                            cls_token_id=CLS, sep_token_id=SEP, pad_token_id=PAD)

    class Metric:
        name = "seen"

        def __init__(self):
            self.got = []

        def samples_from_batch(self, pred):
            self.got.append(pred)

        def evaluate(self):
            return len(self.got)

    class Coordinator:
        trainer, shared_dict, output_streamers = t, {}, []
    t.metrics = [Metric()]
    relevant = [[0], [3], [2]]
    cb = RerankValidationCallback([c["d"]], [(c["q"], c["cand"], relevant)], k=2, name="val", tokens_per_batch=256, round_to=16)
    cb.coordinator = Coordinator()
    cb.on_train_begin()
    cb.on_epoch_end(0)
    cb.on_epoch_end(1)
    assert len(cb.index) == 8 and cb.index.model is c["model"] and cb.index.max_length == 64 and cb.index.special == SP
    assert Coordinator.shared_dict["validation"]["val"]["seen"] == [1, 2]
    ids, rel = t.metrics[0].got[0]
    assert rel == relevant and torch.equal(ids, cb.index.rerank(c["q"], c["cand"], 2)[1])


def test_checkpoint_import_and_save_round_trip(tmp_path):
    """load_cross_encoder_from_local on a random HF BertForSequenceClassification(num_labels=1): the variables equal the
    state dict's and the scores the HF model's own (f32, eval mode); save / load_model rebuild the same model."""
    import transformers
    from polus_amd.checkpoint import load_cross_encoder_from_local
    from polus_amd.ir import models as irm
    from polus_amd.models import load_model
    from tests.test_cross_cpu import _save_hf
    sd = _save_hf(tmp_path)
    m = load_cross_encoder_from_local(str(tmp_path), compute_dtype="f32")
    got = {v.name: v.numpy() for v in m.trainable_weights}
    assert np.array_equal(got["classifier.w"], sd["classifier.weight"]) and np.array_equal(got["classifier.b"], sd["classifier.bias"])
    assert np.array_equal(got["pooler.w"], sd["bert.pooler.dense.weight"])
    assert np.array_equal(got["layer1.ffn1.w"], sd["bert.encoder.layer.1.intermediate.dense.weight"])
    assert m.config.hidden_dropout_prob == 0.1
    hf = transformers.BertForSequenceClassification(transformers.BertConfig(
        vocab_size=60, hidden_size=128, num_hidden_layers=2, num_attention_heads=2, intermediate_size=256,
        max_position_embeddings=32, pad_token_id=None, num_labels=1)).eval()
    hf.load_state_dict({k: torch.as_tensor(v) for k, v in sd.items()}, strict=False)
    r = np.random.Generator(np.random.PCG64(2))
    ids = r.integers(3, 60, size=(4, 20)).astype(np.int32)
    am = (np.arange(20) < np.array([20, 11, 5, 16])[:, None]).astype(np.int32)
    tt = ((np.arange(20) >= 6) & (am > 0)).astype(np.int32)
    with torch.no_grad():
        ref = hf(input_ids=torch.as_tensor(ids).long(), attention_mask=torch.as_tensor(am).long(),
                 token_type_ids=torch.as_tensor(tt).long()).logits[:, 0].numpy()
    s = m(input_ids=ids, attention_mask=am, token_type_ids=tt, training=False)
    print(f"[cross] HF parity: rel err {relerr(host(s), ref):.3e}")
    assert_close(host(s), ref, TOLS["f32"]["logits"], "scores against HF")
    path = m.save(base_path=str(tmp_path / "saved"))
    again = load_model(path + ".cfg", external_module=irm)
    assert isinstance(again, irm.CrossEncoder) and again.compute_dtype == torch.float32
    assert torch.equal(again(input_ids=ids, attention_mask=am, token_type_ids=tt), s)
