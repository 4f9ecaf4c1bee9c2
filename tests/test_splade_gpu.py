"""GPU: the SPLADE kernels (splade.hip), SpladeEncoder, SparseRetrievalTrainer and SparseCorpusIndex against the
float64 references of tests/splade_ref.py.  Cases and bounds live in tests/splade_cases.py.  Every output is poisoned
before the call and every check prints its figure before it asserts (pytest -s shows them)."""
import functools

import numpy as np
import pytest
import torch

from oracle import bert as ob
from tests import mlm_ref as mr
from tests import splade_cases as sc
from tests import splade_ref as sr
from tests.test_model_gpu import TOLS              # the per-engine bounds of tests/test_model_gpu.py
from tests.util import dev, host, relerr

pytestmark = pytest.mark.gpu

DT = {"f32": torch.float32, "bf16": torch.bfloat16}
NAN = float("nan")


@pytest.fixture(scope="module")
def ops():
    from polus_amd import ops as _ops
    return _ops


def _bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def _framed(rows, cols, ld, dtype, off=0, fill=NAN):
    """(flat buffer, [rows, cols] view with row stride ld starting `off` elements in), poisoned."""
    flat = torch.full((off + rows * ld,), fill, dtype=dtype, device="cuda")
    return flat, flat[off:].as_strided((rows, cols), (ld, 1))


def _layout(V, dtype, layout):
    """(row stride, base offset in elements, row stride of the [B, V] arrays)."""
    if layout == "vec":
        return sc.padded_ld(V, dtype) + 16 // sc.ESIZE[dtype], 0, (V + 3) // 4 * 4 + 4
    return V, 1, V + 3 if V % 4 != 1 else V + 2


@functools.lru_cache(maxsize=None)
def _pool_ref(B, S, V):
    x, mask = sc.pool_case(B, S, V)
    return x, mask, sr.pool_fwd(x, mask)


# ------------------------------------------------------------------------------------------------- pooling
def _run_pool_fwd(ops, dtype, shape, layout, masked=True):
    B, S, V = shape
    x, mask, _ = _pool_ref(B, S, V)
    ld, off, ldo = _layout(V, dtype, layout)
    flat, logits = _framed(B * S, V, ld, DT[dtype], off)
    logits.copy_(dev(x.reshape(B * S, V), DT[dtype]))
    outs = [_framed(B, V, ldo, t, 4 if layout == "vec" else 1, f) for t, f in ((torch.float32, NAN), (torch.float32, NAN), (torch.int32, -77))]
    ops.splade_pool_fwd(logits, dev(mask) if masked else None, outs[0][1], outs[1][1], outs[2][1], B, S)
    torch.cuda.synchronize()
    o = 4 if layout == "vec" else 1
    for (buf, _), poison in zip(outs, (NAN, NAN, -77)):               # nothing outside the [B, V] views was written
        probe = buf.clone()
        probe[o:].as_strided((B, V), (ldo, 1)).fill_(poison)
        assert probe.isnan().all() if probe.is_floating_point() else (probe == poison).all(), "pool_fwd wrote outside its outputs"
    return flat, logits, [v for _, v in outs]


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("shape", sc.POOL_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_pool_forward(ops, dtype, shape):
    B, S, V = shape
    x, mask, (ref_rep, ref_xmax, ref_arg) = _pool_ref(B, S, V)
    got = {}
    for layout in sc.POOL_LAYOUTS:
        _, logits, (rep, xmax, arg) = _run_pool_fwd(ops, dtype, shape, layout)
        assert torch.equal(logits.float().cpu(), torch.as_tensor(x.reshape(B * S, V)).float()), "the logits were modified"
        assert np.array_equal(arg.cpu().numpy(), ref_arg), f"{layout}: arg"
        assert np.array_equal(host(xmax), ref_xmax), f"{layout}: xmax"
        r = host(rep)
        assert np.isfinite(r).all() and (r[ref_arg < 0] == 0).all()
        want = np.log1p(host(xmax))
        ulp = np.spacing(np.abs(want).astype(np.float32)).astype(np.float64)
        worst = float((np.abs(r - want) / ulp).max())
        print(f"[splade] pool_fwd {dtype} {shape} {layout}: rep worst {worst:.4f} ulp (bound {sc.REP_ULP_BOUND:.4f}, measured {sc.REP_ULP_MEASURED:.4f})")
        assert worst <= sc.REP_ULP_BOUND, (layout, worst)
        got[layout] = (rep, xmax, arg)
    for a, b in zip(got["vec"], got["scalar"]):
        assert torch.equal(_bits(a), _bits(b)), "the two access routes differ"
    if B > 1:
        assert (ref_arg[B - 1] == -1).all() and (ref_arg[:, 0] == -1).all() and (ref_arg[:, 1] == -1).all()      # masked sequence, negative column, maximum 0
    assert (ref_arg >= 0).any() or B * S * V < 100


def test_pool_forward_without_a_mask_and_nan_never_wins(ops):
    B, S, V = 2, 5, 64
    x, _ = sc.pool_case(B, S, V)
    x = x.copy()
    for dtype in ("f32", "bf16"):
        flat, logits = _framed(B * S, V, V, DT[dtype])
        logits.copy_(dev(x.reshape(B * S, V), DT[dtype]))
        logits.view(B, S, V)[0, :, 7] = NAN                            # a column of NaN: (0, 0, -1)
        logits.view(B, S, V)[1, 2, 9] = NAN                            # one NaN among numbers: skipped
        x2 = x.copy()
        x2[0, :, 7] = -1.0
        x2[1, 2, 9] = -9.0
        ref = sr.pool_fwd(x2, None)
        rep, xmax, arg = (torch.full((B, V), NAN, device="cuda"), torch.full((B, V), NAN, device="cuda"),
                          torch.full((B, V), -77, dtype=torch.int32, device="cuda"))
        ops.splade_pool_fwd(logits, None, rep, xmax, arg, B, S)
        assert np.array_equal(arg.cpu().numpy(), ref[2]) and np.array_equal(host(xmax), ref[1])
        assert arg[0, 7].item() == -1 and rep[0, 7].item() == 0.0


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("shape", sc.POOL_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_pool_backward(ops, dtype, shape):
    B, S, V = shape
    x, mask, (_, ref_xmax, ref_arg) = _pool_ref(B, S, V)
    rng = np.random.Generator(np.random.PCG64(V + S))
    drep_h = rng.standard_normal((B, V)).astype(np.float32)
    want = torch.as_tensor(sr.pool_bwd_f32(drep_h, ref_xmax, ref_arg, S)).to(DT[dtype]).reshape(B * S, V)
    assert (want != 0).any() or B * S * V < 100
    for layout in sc.POOL_LAYOUTS:
        ld, off, ldo = _layout(V, dtype, layout)
        ins = [_framed(B, V, ldo, t, 4 if layout == "vec" else 1, 0)[1] for t in (torch.float32, torch.float32, torch.int32)]
        ins[0].copy_(dev(drep_h)); ins[1].copy_(dev(ref_xmax.astype(np.float32))); ins[2].copy_(dev(ref_arg))
        for inplace in (False, True):
            flat, d = _framed(B * S, V, ld, DT[dtype], off)
            if inplace:                                                # over the logits of the forward pass
                d.copy_(dev(x.reshape(B * S, V), DT[dtype]))
            ops.splade_pool_bwd(ins[0], ins[1], ins[2], d, B, S)
            torch.cuda.synchronize()
            assert not d.float().isnan().any(), f"{layout}: an element of dlogits was not written"
            assert torch.equal(_bits(d), _bits(want.cuda())), f"{layout} inplace={inplace}: values"
            if ld > V:
                pad = flat[off:off + B * S * ld].view(B * S, ld)[:, V:]
                assert pad.float().isnan().all(), f"{layout}: columns past V were written"
            assert off == 0 or flat[:off].float().isnan().all()
    print(f"[splade] pool_bwd {dtype} {shape}: {int((want != 0).sum())} non-zero entries of {want.numel()}, exact on both routes, out of place and in place")


# ------------------------------------------------------------------------------------------------- FLOPS regulariser
@pytest.mark.parametrize("rows", sc.FLOPS_ROWS)
@pytest.mark.parametrize("V", sc.FLOPS_V)
def test_flops_regulariser(ops, rows, V):
    lam = 0.37
    rep_h, pre_h = sc.flops_case(rows, V)
    ref_val, ref_g = sr.flops_reg(rep_h, lam)
    rtol = sc.flops_rtol(rows, V)
    runs = []
    for ld, off in ((V + 3) // 4 * 4, 0), (V + 1, 1), ((V + 3) // 4 * 4, 0):   # aligned, unaligned, aligned again
        _, rep = _framed(rows, V, ld, torch.float32, off)
        rep.copy_(dev(rep_h))
        _, drep = _framed(rows, V, ld, torch.float32, off)
        drep.copy_(dev(pre_h))
        loss = torch.full((1,), NAN, device="cuda")
        ops.flops_reg(rep, lam, loss, drep=drep)
        acc = torch.full((1,), 1.5, device="cuda")
        ops.flops_reg(rep, lam, acc, accumulate=True)
        torch.cuda.synchronize()
        e_val = abs(loss.item() - ref_val) / ref_val
        want = pre_h.astype(np.float64) + ref_g                        # every term is non-negative: no cancellation
        diff = np.abs(host(drep) - want)
        e_g = float((diff[want > 0] / want[want > 0]).max())
        e_acc = abs(acc.item() - (1.5 + ref_val)) / (1.5 + ref_val)
        print(f"[splade] flops rows={rows} V={V} ld={ld}: value rel err {e_val:.3e}, gradient {e_g:.3e}, accumulated loss {e_acc:.3e} (bound {rtol:.3e})")
        assert e_val <= rtol and e_g <= rtol and e_acc <= rtol and (diff[want == 0] == 0).all()
        assert torch.equal(rep.cpu(), torch.as_tensor(rep_h)), "rep was modified"
        runs.append((loss.clone(), drep.contiguous().clone()))
    for other in runs[1:]:                                              # two runs, and both access widths: the same bits
        assert torch.equal(_bits(runs[0][0]), _bits(other[0])) and torch.equal(_bits(runs[0][1]), _bits(other[1]))


# ------------------------------------------------------------------------------------------------- sparse scores
def _scores(ops, q, ids, w, lds=None):
    B, N = q.shape[0], ids.shape[0]
    lds = N + 3 if lds is None else lds
    flat, s = _framed(B, N, lds, torch.float32)
    ops.sparse_scores(q, ids, w, s)
    torch.cuda.synchronize()
    assert flat.view(B, lds)[:, N:].isnan().all(), "columns past N were written"
    return s


@pytest.mark.parametrize("M", sc.SCORE_M)
@pytest.mark.parametrize("V", sc.SCORE_V)
def test_sparse_scores(ops, M, V):
    # (a) eighths: exact in every order
    q, ids, w = sc.score_case(M, V, exact=True)
    ref, _ = sr.sparse_scores(q, ids, w)
    got = host(_scores(ops, dev(q), dev(ids), dev(w)))
    assert np.array_equal(got, ref), f"exact data: max |diff| {np.abs(got - ref).max()}"
    # (b) random data against the bound of any summation order
    q, ids, w = sc.score_case(M, V, exact=False)
    ref, mag = sr.sparse_scores(q, ids, w)
    dq, di, dw = dev(q), dev(ids), dev(w)
    whole = _scores(ops, dq, di, dw)
    ratio = float((np.abs(host(whole) - ref) / (sc.gamma(M + 1) * mag + 1e-300)).max())
    print(f"[splade] sparse_scores M={M} V={V}: worst error {ratio:.4f} x gamma_{M + 1} sum|w q|")
    assert ratio <= 1.0
    # (c) the bits of an entry do not depend on the launch: halves of the documents, one query at a time, strided rows
    N, h = sc.SCORE_N, sc.SCORE_N // 2
    halves = torch.cat([_scores(ops, dq, di[:h], dw[:h]), _scores(ops, dq, di[h:], dw[h:])], 1)
    assert torch.equal(_bits(whole), _bits(halves)), "a launch over N documents differs from two over its halves"
    single = torch.cat([_scores(ops, dq[b:b + 1], di, dw) for b in range(sc.SCORE_B)], 0)
    assert torch.equal(_bits(whole), _bits(single)), "B = 1 launches differ"
    _, qs = _framed(sc.SCORE_B, V, V + 1, torch.float32, 1)
    qs.copy_(dq)
    assert torch.equal(_bits(whole), _bits(_scores(ops, qs, di, dw))), "an unaligned query row differs"


# ------------------------------------------------------------------------------------------------- model
def _close(got, ref, tol, what):
    g = host(got) if torch.is_tensor(got) else np.asarray(got, np.float64)
    e = relerr(g.reshape(np.shape(ref)), ref)
    print(f"[splade] {what}: rel err {e:.3e} (tol {tol:.1e})")
    assert np.isfinite(g).all(), f"{what}: not fully written (or not finite)"
    assert e <= tol, f"{what}: rel err {e:.3e} > {tol:.1e}"


def _model(mode, params=None, **cfg_kw):
    from polus_amd.ir.models import SpladeEncoder
    from polus_amd.models import BertConfig, BertForMaskedLM
    ocfg = ob.BertConfig(*sc.MODEL_SHAPE)
    model = SpladeEncoder(BertForMaskedLM(BertConfig(*sc.MODEL_SHAPE, **cfg_kw), compute_dtype=mode))
    p = _params() if params is None else params
    model.load_numpy_params(p)
    return model, ocfg, p


@functools.lru_cache(maxsize=None)
def _params():
    p = mr.mlm_params(ob.BertConfig(*sc.MODEL_SHAPE))
    rng = np.random.Generator(np.random.PCG64(8))
    # logits of both signs with most of them negative: about one term in seven is active, as in a trained SPLADE model, and
    # the scores of the trainer test stay of order 1, where the absolute f32 loss bound of TOLS means something
    p["mlm.bias"] = p["mlm.bias"] + 0.3 * rng.standard_normal(p["mlm.bias"].shape) - 0.8
    return p


@functools.lru_cache(maxsize=None)
def _model_ref():
    ocfg = ob.BertConfig(*sc.MODEL_SHAPE)
    batch = sr.splade_batch(ocfg, sc.MODEL_B, sc.MODEL_S)
    rep, state = sr.splade_fwd(_params(), ocfg, *batch)
    return batch, rep, state


@pytest.mark.parametrize("mode", ["f32", "bf16"])
def test_model_matches_the_reference(mode):
    tol = TOLS[mode]
    (ids, mask, tt), ref_rep, state = _model_ref()
    model, ocfg, p = _model(mode)
    B, S, V = sc.MODEL_B, sc.MODEL_S, sc.MODEL_SHAPE[0]
    model.arena.grads.fill_(NAN)
    rep = model(input_ids=ids, attention_mask=mask, token_type_ids=tt, training=True)
    assert tuple(rep.shape) == (B, V) and rep.dtype == torch.float32
    _close(rep, ref_rep, tol["logits"], f"model {mode} rep")
    # the device's winners reach the reference's maxima to within the logits' own bound
    arg = model._stash[2].cpu().numpy()
    logits = state["logits"]
    t = tol["logits"] * np.abs(logits).max()
    at = np.take_along_axis(logits, np.maximum(arg, 0)[:, None, :], 1)[:, 0, :]
    valid = np.asarray(mask)[np.arange(B)[:, None], np.maximum(arg, 0)] != 0
    short = np.where(arg >= 0, state["xmax"] - at, state["xmax"])
    print(f"[splade] model {mode}: winners fall short of the reference maximum by at most {short.max():.3e} (bound {t:.3e}); "
          f"{int((arg != state['arg']).sum())} of {arg.size} differ from the reference's")
    assert (valid | (arg < 0)).all(), "a masked token won"
    assert short.max() <= t
    rng = np.random.Generator(np.random.PCG64(17))
    c = rng.standard_normal((B, V)).astype(np.float32)
    ref_g = sr.splade_bwd(c.astype(np.float64), p, ocfg, state, arg=arg)
    model.backward(dev(c))
    torch.cuda.synchronize()
    got = {v.name: host(v.grad) for v in model.trainable_weights}
    assert set(got) == {k for k in ref_g if "/" not in k}
    for k in sorted(got):
        _close(got[k], ref_g[k], tol["grad"], f"model {mode} grad {k}")
    for part in ("emb.word/embedding", "emb.word/decoder"):             # each share alone is far from the total
        assert relerr(got["emb.word"], ref_g[part]) > 0.5 * relerr(ref_g["emb.word"], ref_g[part])


def test_model_save_and_load(tmp_path):
    import polus_amd.ir.models as irm
    from polus_amd.models import load_model
    (ids, mask, tt), _, _ = _model_ref()
    keys = ("vocab_size", "hidden_size", "num_hidden_layers", "num_attention_heads", "intermediate_size", "max_position_embeddings")
    model = irm.splade_encoder(model=dict(zip(keys, sc.MODEL_SHAPE), compute_dtype="f32"))
    model.load_numpy_params(_params())
    x = {"input_ids": ids, "attention_mask": mask, "token_type_ids": tt}
    before = model.encode_document(x)
    path = model.save(base_path=str(tmp_path))
    again = load_model(path + ".cfg", external_module=irm)
    assert type(again) is irm.SpladeEncoder and [v.name for v in again.trainable_weights] == [v.name for v in model.trainable_weights]
    assert torch.equal(again.encode_query(x), before) and before.data_ptr() != model.encode_query(x).data_ptr()


# ------------------------------------------------------------------------------------------------- trainer
LAM_Q, LAM_D = 0.1, 0.05           # regularisers of the contrastive loss's size (0.73 and 0.22 beside 0.90 at step 0)


def _step_batch(ocfg, seed, B=2, k=1, S=16):
    ids, mask, tt = sr.splade_batch(ocfg, (2 + k) * B, S, seed)
    mask = np.maximum(mask, (np.arange(S)[None] < 4).astype(np.int32))     # at least four valid tokens everywhere
    part = lambda a, b: {"input_ids": dev(ids[a:b]), "attention_mask": dev(mask[a:b])}
    neg = {"input_ids": dev(ids[2 * B:].reshape(k, B, S).transpose(1, 0, 2)), "attention_mask": dev(mask[2 * B:].reshape(k, B, S).transpose(1, 0, 2))}
    return (part(0, B), part(B, 2 * B), neg), (ids, mask)


def _train(mode, graph, steps=3):
    from polus_amd.ir.training import SparseRetrievalTrainer
    from polus_amd.optimizers import AdamWeightDecay
    model, ocfg, _ = _model(mode)
    model.deterministic = True
    t = SparseRetrievalTrainer(model, AdamWeightDecay(learning_rate=1e-3, weight_decay_rate=0.01), lambda_q=LAM_Q, lambda_d=LAM_D)
    if graph:
        t.enable_step_graph(warmup=1)
    losses, first = [], None
    for s in range(steps):
        batch, _ = _step_batch(ocfg, 60 + s)
        losses.append(float(t.train_step(*batch)))
        if s == 0:
            first = t.reps.clone()
    torch.cuda.synchronize()
    assert t.optimizer.iterations == steps
    return t, losses, first, model.arena.params.clone()


def test_trainer_steps_against_the_reference_and_bitwise(ops):
    t, losses, reps, params = _train("f32", graph=False)
    ocfg = ob.BertConfig(*sc.MODEL_SHAPE)
    _, (ids, mask) = _step_batch(ocfg, 60)
    ref_rep, _ = sr.splade_fwd(_params(), ocfg, ids, mask, None)
    ref = sr.objective(ref_rep, 2, 1, LAM_Q, LAM_D)
    tol = TOLS["f32"]["loss"]
    rq, rd = torch.empty(1, device="cuda"), torch.empty(1, device="cuda")
    ops.flops_reg(reps[:2], LAM_Q, rq)
    ops.flops_reg(reps[2:], LAM_D, rd)
    print(f"[splade] trainer step 0: loss {losses[0]:.6f} (reference {ref[0]:.6f} = {ref[1]:.6f} + {ref[2]:.6f} + {ref[3]:.6f}), "
          f"regularisers {rq.item():.6f}, {rd.item():.6f}; losses {losses}")
    assert abs(losses[0] - ref[0]) < tol and abs(rq.item() - ref[2]) < tol and abs(rd.item() - ref[3]) < tol
    assert ref[2] > 100 * tol and ref[3] > 100 * tol, "the regularisers are too small to be seen in the loss"
    _, losses2, _, params2 = _train("f32", graph=False)
    assert losses == losses2 and torch.equal(params, params2), "two runs from one seed differ"
    tg, losses3, _, params3 = _train("f32", graph=True)
    assert tg._graphed.graph is not None, "the step was not captured"
    assert losses == losses3 and torch.equal(params, params3), "the replayed step graph differs from eager steps"


def test_trainer_accumulates_and_refuses_mixed_lengths():
    from polus_amd.ir.training import SparseRetrievalTrainer
    from polus_amd.optimizers import Adam
    ocfg = ob.BertConfig(*sc.MODEL_SHAPE)
    (q, d, n), _ = _step_batch(ocfg, 70)
    grads = []
    for accum in (1, 2):
        model, _, _ = _model("f32")
        model.deterministic = True
        t = SparseRetrievalTrainer(model, Adam(learning_rate=0.0), lambda_q=LAM_Q, lambda_d=LAM_D)
        t.grad_accum_steps = accum
        model.arena.grads.fill_(NAN)
        for _ in range(accum):
            t.train_step(q, d, n)
        torch.cuda.synchronize()
        grads.append(np.concatenate([host(v.grad).reshape(-1) for v in model.trainable_weights]) / accum)
    e = relerr(grads[1], grads[0])
    print(f"[splade] two accumulated micro-steps of one batch against one step: rel err {e:.3e}")
    assert e <= TOLS["f32"]["grad"]
    short = {k: v[:, :8] for k, v in d.items()}
    with pytest.raises(ValueError, match="one padded length"):
        t.train_step(q, short, n)


# ------------------------------------------------------------------------------------------------- index
class BagModel:
    """A stand-in encoder with exact arithmetic: rep[v] = (valid tokens equal to v) * (v % 7 + 1) / 8."""

    def __init__(self, V):
        self.V = V

    def _encode(self, x, training=False):
        ids = torch.as_tensor(np.asarray(x["input_ids"])).long().cuda()
        m = torch.as_tensor(np.asarray(x["attention_mask"])).float().cuda()
        rep = torch.zeros((ids.shape[0], self.V), device="cuda")
        rep.scatter_add_(1, ids, m)
        return rep * ((torch.arange(self.V, device="cuda") % 7 + 1).float() / 8)

    encode_query = encode_document = _encode

    def query_projection(self, rep, training=False):
        return rep

    document_projection = query_projection


def test_sparse_index_and_two_stage_search():
    from polus_amd.ir.search import CorpusIndex, SparseCorpusIndex, TwoStageSearch
    from polus_amd.ir.training import MaxSimScores
    from tests.search_cases import TableModel, batches, token_case
    case = dict(seed=3, Q=16, N=300, Lq=8, Ld=24, E=64, V=4096)
    c = token_case(**case)
    N, V, terms = case["N"], case["V"], 8
    bag = BagModel(V)
    index = SparseCorpusIndex(bag, terms=terms, scratch_bytes=4 * case["Q"] * 128)      # three chunks of documents
    docs = batches(c["d_ids"], c["d_mask"], [N // 2, N - N // 2])
    got_ids = [index.add(b) for b in docs]
    assert torch.cat(got_ids).cpu().tolist() == list(range(N)) and len(index) == N and len(index.chunks(case["Q"])) == 3
    assert index.nbytes == N * terms * 8
    queries = {"input_ids": c["q_ids"], "attention_mask": c["q_mask"]}
    rep_d = np.concatenate([bag.encode_document(b).cpu().numpy() for b in docs]).astype(np.float64)
    rep_q = bag.encode_query(queries).cpu().numpy().astype(np.float64)
    t_ids, t_w = sr.truncate(rep_d, terms)
    assert np.array_equal(index.term_ids.cpu().numpy(), t_ids) and np.array_equal(index.weights.cpu().numpy().astype(np.float64), t_w)
    assert (rep_d > 0).sum(1).max() > terms, "no document is truncated"
    scores, _ = sr.sparse_scores(rep_q, t_ids, t_w)
    for k in (10, 100):
        val, idx = index.search(queries, k)
        ref_val, ref_idx = sr.rank(scores, k)
        assert np.array_equal(idx.cpu().numpy(), ref_idx) and np.array_equal(val.cpu().numpy().astype(np.float64), ref_val), f"k = {k}"
    second = CorpusIndex(TableModel(c["table"], torch.float32, True), MaxSimScores(normalize=False))
    for b in docs:
        second.add(b)
    two = TwoStageSearch(index, second, candidates=50)
    val, idx = two.search(queries, 10)
    want_val, want_idx = second.rerank(queries, index.search(queries, 50)[1], 10)
    assert torch.equal(idx, want_idx) and torch.equal(_bits(val), _bits(want_val))
    assert two.add({"input_ids": c["d_ids"][:4], "attention_mask": c["d_mask"][:4]}).cpu().tolist() == list(range(N, N + 4))
    index.clear()
    assert len(index) == 0 and index.nbytes == 0
    with pytest.raises(ValueError, match="empty"):
        index.search(queries, 5)
