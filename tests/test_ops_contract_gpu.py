"""GPU: the extents the wrappers of polus_amd/ops.py enforce are what the kernels really touch.

Every good call of tests/ops_contract_cases.py runs against the real library with each output carved, at exactly the extent
the table states, out of a larger sentinel-filled buffer (64 guard elements in front, behind and between the rows of a
row-strided output).  The results match the float64 reference of the operation within the bounds the project already uses
for that kernel, and every guard element is intact: a wrapper check that is lax by one row passes the CPU test and fails
here.  Every bad call runs with device tensors under the recording library: it raises, and nothing is recorded."""
import math

import numpy as np
import pytest
import torch

from oracle import bert as ob
from oracle import losses as ol
from tests import attention_cases as ac
from tests import centroid_ref as cr
from tests import fp8_ref
from tests import ivf_ref
from tests import layer_cases as lc
from tests import maxsim_cases as mc
from tests import maxsim_ref as mr
from tests import ops_contract_cases as oc
from tests import residual_ref as rr
from tests import rowwise_cases as rc
from tests import search_ref as sr
from tests import tuple_cases as tc
from tests import tuple_ref as tr
from tests.fakes import RecordingLib
from tests.util import TOL, dropout_keep_np, host, relerr

pytestmark = pytest.mark.gpu

GUARD = 64
T32 = TOL[torch.float32]


@pytest.fixture(scope="module")
def ops():
    from polus_amd import ops as _ops
    _ops.set_dynamic_params(None)
    return _ops


@pytest.fixture
def rec(monkeypatch):
    from polus_amd import _lib, ops as _ops
    proxy = RecordingLib(_lib.load())
    monkeypatch.setattr(_lib, "load", lambda: proxy)
    monkeypatch.setattr(_ops, "_WS", {})
    prev = _lib._CUR_STREAM[0]
    _lib._CUR_STREAM[0] = oc.STREAM
    try:
        yield proxy
    finally:
        _lib._CUR_STREAM[0] = prev


# ------------------------------------------------------------------------------------------------- bad calls, device tensors
@pytest.mark.parametrize("key", list(oc.CASES))
def test_bad_calls_with_device_tensors_are_refused_before_any_entry_point(key, rec):
    from polus_amd import ops as _ops
    bads = [b for b in oc.bad_cases() if b.key == key]
    assert bads
    for bad in bads:
        oc.check_refused(_ops, bad, bad.args(place=lambda t: t.cuda()), rec)


# ------------------------------------------------------------------------------------------------- guarded outputs
class Carved:
    """`t` (a device tensor) re-homed inside a sentinel-filled buffer: the view has t's shape and values, row-strided with
    GUARD elements between rows if `strided`, and GUARD elements in front of and behind it."""

    def __init__(self, t, strided):
        rows = t.shape[0] if strided else 1
        cols = t.numel() // rows if rows else 0
        ld = cols + GUARD if strided else cols
        self.buf = torch.empty(GUARD + rows * ld + GUARD, dtype=t.dtype, device=t.device)
        self.buf.fill_(77)
        if strided:
            self.view = self.buf.as_strided((rows, cols), (ld, 1), GUARD)
            idx = torch.arange(self.buf.numel(), device=t.device).as_strided((rows, cols), (ld, 1), GUARD)
        else:
            self.view = self.buf[GUARD:GUARD + t.numel()].view(t.shape)
            idx = torch.arange(GUARD, GUARD + t.numel(), device=t.device)
        self.view.copy_(t)
        self.outside = torch.ones(self.buf.numel(), dtype=torch.bool, device=t.device)
        self.outside[idx.reshape(-1)] = False
        self.before = self._bits().clone()

    def _bits(self):
        return self.buf.view({1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[self.buf.element_size()])

    def intact(self):
        return bool(torch.equal(self._bits()[self.outside], self.before[self.outside]))


def run_good(ops, key, prepare=None):
    """Runs the good call of `key` on the device with carved outputs; returns (CPU arguments, device arguments)."""
    case = oc.CASES[key]
    cpu = case.good()
    args = oc.map_tensors(cpu, lambda t: t.cuda())
    if prepare is not None:
        prepare(args)
    carved = {}
    for path, spec in case.tensors.items():
        if spec.out:
            carved[path] = Carved(oc.get(args, path), strided=spec.layout == "inner")
            oc.put(args, path, carved[path].view)
    getattr(ops, oc.op_of(key))(**args)
    torch.cuda.synchronize()
    for path, c in carved.items():
        assert c.intact(), f"{key}: {path} was written outside the extent the table states"
    return cpu, args


def close(got, ref, tol, what):
    g = host(got) if torch.is_tensor(got) else np.asarray(got, np.float64)
    ref = np.asarray(ref, np.float64)
    assert np.isfinite(g).all(), f"{what}: not fully written (or not finite)"
    e = relerr(g.reshape(ref.shape), ref)
    print(f"[contract] {what}: rel err {e:.3e} (tol {tol:.1e})")
    assert e <= tol, f"{what}: rel err {e:.3e} > {tol:.1e}"


def loss_close(loss, ref, what):
    got = float(loss)
    print(f"[contract] {what}: loss {got:.7g} (oracle {float(ref):.7g})")
    assert np.isfinite(got) and abs(got - ref) < 1e-5 * max(1, abs(ref)), (what, got, ref)      # the bound of test_rowwise_gpu.py


def f64(t):
    return t.double().numpy()


# ------------------------------------------------------------------------------------------------- GEMM family
def test_gemm(ops):
    cpu, d = run_good(ops, "gemm")
    v = f64(cpu["a"]) @ f64(cpu["b"]).T + f64(cpu["bias"])
    close(d["aux"], v, T32, "gemm aux")
    close(d["out"], ob.gelu(v) + f64(cpu["resid"]), T32, "gemm out")


def _dw_check(dy, x, dw, db, what):
    close(dw, f64(dy).T @ f64(x), lc.GEMM_DW_TOL["f32"], f"{what} dw")
    close(db, f64(dy).sum(0), lc.GEMM_DB_TOL["f32"], f"{what} db")


def test_dense_bwd_params(ops):
    cpu, d = run_good(ops, "dense_bwd_params")
    _dw_check(cpu["dy"], cpu["x"], d["dw"], d["db"], "dense_bwd_params")


def test_dense_bwd_params_grouped(ops):
    cpu, d = run_good(ops, "dense_bwd_params_grouped")
    for k, ((dy, x, _, _), (_, _, dw, db)) in enumerate(zip(cpu["problems"], d["problems"])):
        _dw_check(dy, x, dw, db, f"dense_bwd_params_grouped[{k}]")


def test_dense_thin(ops):
    cpu, d = run_good(ops, "dense_thin_fwd")
    close(d["y"], f64(cpu["x"]) @ f64(cpu["w"]).T + f64(cpu["bias"]), T32, "dense_thin_fwd y")
    cpu, d = run_good(ops, "dense_thin_bwd")
    close(d["dx"], f64(cpu["dy"]) @ f64(cpu["w"]), T32, "dense_thin_bwd dx")
    close(d["dw"], f64(cpu["dy"]).T @ f64(cpu["x"]), lc.THIN_PARAM_TOL, "dense_thin_bwd dw")
    close(d["db"], f64(cpu["dy"]).sum(0), lc.THIN_PARAM_TOL, "dense_thin_bwd db")


# ------------------------------------------------------------------------------------------------- attention
def test_attention(ops):
    B, S, A, H = oc.ATT_B, oc.ATT_S, oc.ATT_A, 64 * oc.ATT_A
    assert (ac.fwd_path("f32", S), ac.bwd_path("f32", S)) == ("F4", "B7")
    cpu, d = run_good(ops, "attention_fwd")
    qkv, mask = f64(cpu["qkv"]).reshape(B, S, 3 * H), cpu["mask"].numpy()
    ctx_ref, lse_ref, _ = ac.oracle(qkv, mask, np.zeros((B, S, H)), A)
    tol = ac.TOL["F4"]
    assert ac.violation(host(d["ctx"]).reshape(B, S, H), ctx_ref, tol["ctx"]) <= 1.0
    assert np.abs(host(d["lse"]).reshape(B, A, S) - lse_ref).max() <= tol["lse"]
    fwd = d

    def forward_outputs(args):           # the backward's ctx and lse are what the forward wrote
        args["ctx"], args["lse"] = fwd["ctx"].contiguous(), fwd["lse"].contiguous()
    cpu, d = run_good(ops, "attention_bwd", forward_outputs)
    _, _, dqkv_ref = ac.oracle(qkv, mask, f64(cpu["dctx"]).reshape(B, S, H), A, ctx_in=host(d["ctx"]))
    got, ref = ac.split(host(d["dqkv"]).reshape(B, S, 3 * H), H), ac.split(dqkv_ref, H)
    for nm in ("dq", "dk", "dv"):
        assert np.isfinite(got[nm]).all() and ac.violation(got[nm], ref[nm], ac.TOL["B7"][nm]) <= 1.0, nm


# ------------------------------------------------------------------------------------------------- LayerNorm and embeddings
def _ln_reference(cpu):
    keep = rc.keep_scale(oc.LN_SEED, oc.LN_DROP_P, oc.LN_ROWS, oc.LN_H)
    return rc.ln_bwd_reference(f64(cpu["x"]), f64(cpu["dy"]), f64(cpu["gamma"]), f64(cpu["mean"]), f64(cpu["rstd"]), keep)


def test_layernorm(ops):
    tol = rc.ln_tol("f32")
    cpu, d = run_good(ops, "layernorm_fwd")
    y, mean, rstd = rc.ln_fwd_reference(f64(cpu["x"]), f64(cpu["gamma"]), f64(cpu["beta"]))
    for nm, ref in (("y", y), ("mean", mean), ("rstd", rstd)):
        close(d[nm], ref, tol[nm], f"layernorm_fwd {nm}")
    cpu, d = run_good(ops, "layernorm_bwd")
    ref = _ln_reference(cpu)
    for nm, key in (("dx", "dx"), ("dx_masked", "dxm"), ("dgamma", "dgamma"), ("dbeta", "dbeta"), ("dbias", "dbias")):
        close(d[nm], ref[key], tol[key], f"layernorm_bwd {nm}")
    # the deferred form leaves its partial sums in `partials`; the finalize call reduces exactly those
    cpu, d = run_good(ops, "layernorm_bwd:deferred")
    close(d["dx"], ref["dx"], tol["dx"], "layernorm_bwd deferred dx")
    close(d["dx_masked"], ref["dxm"], tol["dxm"], "layernorm_bwd deferred dx_masked")
    partials = d["partials"].contiguous()

    def deferred_partials(args):
        args["partials"] = partials
    _, d = run_good(ops, "layernorm_bwd_finalize", deferred_partials)
    for nm in ("dgamma", "dbeta", "dbias"):
        close(d[nm], ref[nm], tol[nm], f"layernorm_bwd_finalize {nm}")


def test_embeddings(ops):
    tol = rc.emb_tol("f32")
    cfg = ob.BertConfig(vocab_size=oc.EMB_V, hidden_size=oc.EMB_H, max_position_embeddings=oc.EMB_S, type_vocab_size=oc.EMB_T)
    cpu, d = run_good(ops, "embed_ln_fwd")
    p = {"emb.word": f64(cpu["word"]), "emb.pos": f64(cpu["pos"]), "emb.type": f64(cpu["typ"]), "emb.ln.g": f64(cpu["gamma"]),
         "emb.ln.b": f64(cpu["beta"])}
    ids, tt = cpu["ids"].numpy(), cpu["type_ids"].numpy()
    y, cache = ob.embeddings_fwd(p, cfg, ids, tt)
    n = oc.EMB_B * oc.EMB_S
    close(d["y"], y.reshape(n, oc.EMB_H), tol["y"], "embed_ln_fwd y")
    close(d["mean"], cache[1].reshape(n), tol["mean"], "embed_ln_fwd mean")
    close(d["rstd"], cache[2].reshape(n), tol["rstd"], "embed_ln_fwd rstd")
    cpu, d = run_good(ops, "embed_ln_bwd")
    cache = (cache[0], f64(cpu["mean"]).reshape(oc.EMB_B, oc.EMB_S), f64(cpu["rstd"]).reshape(oc.EMB_B, oc.EMB_S)) + tuple(cache[3:])
    g = ob.embeddings_bwd(f64(cpu["dy"]).reshape(oc.EMB_B, oc.EMB_S, oc.EMB_H), p, cfg, cache)
    for nm, key in (("gword", "emb.word"), ("gpos", "emb.pos"), ("gtyp", "emb.type"), ("ggamma", "emb.ln.g"), ("gbeta", "emb.ln.b")):
        close(d[nm], g[key], tol[key], f"embed_ln_bwd {nm}")


# ------------------------------------------------------------------------------------------------- reductions, losses, metrics
def test_colsum_and_argmax(ops):
    cpu, d = run_good(ops, "colsum")
    close(d["out"], f64(cpu["x"]).sum(0), rc.COLSUM_TOL, "colsum")
    cpu, d = run_good(ops, "argmax")
    assert np.array_equal(d["out"].cpu().numpy(), f64(cpu["x"]).argmax(1))


def test_losses(ops):
    dtol = rc.loss_dlogits_tol("f32")
    cpu, d = run_good(ops, "softmax_xent")
    loss, dl = ol.weighted_softmax_xent_fwd(f64(cpu["class_weights"]), np.eye(3)[cpu["labels"].numpy()], f64(cpu["logits"]))
    loss_close(d["loss"], loss, "softmax_xent")
    close(d["dlogits"], dl, dtol, "softmax_xent dlogits")
    cpu, d = run_good(ops, "sigmoid_xent")
    loss, dl = ol.weighted_sigmoid_xent_fwd(f64(cpu["class_weights"]), cpu["negative_weight"], f64(cpu["y_true"]), f64(cpu["logits"]))
    loss_close(d["loss"], loss, "sigmoid_xent")
    close(d["dlogits"], dl, dtol, "sigmoid_xent dlogits")


def test_confusion_matrix(ops):
    cpu, d = run_good(ops, "confusion_matrix")
    r, c = cpu["row_idx"].numpy(), cpu["col_idx"].numpy()
    ok = (r >= 0) & (r < 3) & (c >= 0) & (c < 3)
    want = np.zeros((3, 3), np.int64)
    np.add.at(want, (r[ok], c[ok]), 1)
    assert np.array_equal(d["cm"].cpu().numpy(), want) and int(d["rejected"]) == int((~ok).sum()) == 2


# ------------------------------------------------------------------------------------------------- optimizer
def test_adam_step(ops):
    h = oc.ADAM_HYPER
    assert (h["lr"], h["beta1"], h["beta2"], h["eps"], h["weight_decay"], h["grad_scale"], oc.ADAM_CLIP) == (
        rc.ADAM_LR, rc.ADAM_B1, rc.ADAM_B2, rc.ADAM_EPS, rc.ADAM_WD, rc.ADAM_GRAD_SCALE, rc.ADAM_CLIP)
    assert math.isclose(h["lr_t"], rc.adam_lr_t(1), rel_tol=1e-12)
    cpu, d = run_good(ops, "adam_step")
    seg = np.array(oc.ADAM_SEG, np.int64)
    st = {"p": f64(cpu["p"]), "m": f64(cpu["m"]), "v": f64(cpu["v"]), "g": [f64(cpu["g"])]}
    ref = rc.adam_reference(seg, st, [rc.ADAM_GRAD_SCALE * rc.ADAM_CLIP])[0]
    inside, shadow_mask = rc.seg_masks(seg, 8)
    for nm in ("p", "m", "v"):
        close(d[nm], ref[nm], rc.ADAM_TOL, f"adam_step {nm}")
        assert np.array_equal(host(d[nm])[~inside], st[nm][~inside]), f"adam_step: {nm} touched outside the windows"
    want = torch.where(torch.as_tensor(shadow_mask).cuda(), d["p"].to(torch.bfloat16), torch.zeros_like(d["shadow"]))
    assert torch.equal(d["shadow"], want)


def test_norms_and_clip(ops):
    cpu, d = run_good(ops, "sqnorm")
    close(d["out"], [(f64(cpu["g"]) ** 2).sum()], rc.SQNORM_TOL, "sqnorm")
    cpu, d = run_good(ops, "sqnorm_segments")
    close(d["out"], [(f64(cpu["g"])[:7] ** 2).sum()], rc.SQNORM_TOL, "sqnorm_segments")
    cpu, d = run_good(ops, "clip_scale")
    norm = math.sqrt(float(f64(cpu["sq"]).sum())) * abs(cpu["grad_scale"])
    assert abs(float(d["out"]) - cpu["clip_norm"] / max(norm, cpu["clip_norm"])) < 1e-6          # the bound of test_kernels_gpu.py


# ------------------------------------------------------------------------------------------------- element-wise
def test_elementwise(ops):
    cpu, d = run_good(ops, "cast")
    assert torch.equal(d["dst"].cpu(), cpu["src"].to(torch.bfloat16))
    cpu, d = run_good(ops, "scale_")
    assert torch.equal(d["x"].cpu(), cpu["x"] * 0.3)
    cpu, d = run_good(ops, "act_bwd")
    close(d["du"], f64(cpu["dy"]) * rc.act_grad("gelu", f64(cpu["u"])), T32, "act_bwd")
    cpu, d = run_good(ops, "dropout")
    keep = dropout_keep_np(cpu["seed"], cpu["drop_p"], 0, 8).reshape(2, 4)
    close(d["y"], f64(cpu["x"]) * keep / (1.0 - cpu["drop_p"]), T32, "dropout")
    assert 0 < keep.sum() < 8


def test_transposes(ops):
    cpu, d = run_good(ops, "transpose_bf16")
    assert torch.equal(d["dst"].cpu(), cpu["src"].t().contiguous())
    cpu, d = run_good(ops, "transpose_bf16_batched")
    want = cpu["dst_base"].clone()
    for off, R, C, _ in oc.TR_SEGS:
        want[off:off + R * C] = cpu["src_base"][off:off + R * C].view(R, C).t().reshape(-1)
    assert torch.equal(d["dst_base"].cpu().view(torch.int16), want.view(torch.int16)), "a transposed matrix is wrong or the gap was written"


def test_set_dynamic_params(ops):
    args = oc.map_tensors(oc.CASES["set_dynamic_params"].good(), lambda t: t.cuda())
    try:
        ops.set_dynamic_params(**args)
    finally:
        ops.set_dynamic_params(None)
        torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------- token retrieval
MS = mc.TOL["f32"]


def bits(t):
    """The int32 bit patterns of an f32 device tensor (or host array)."""
    a = t.detach().cpu().contiguous().numpy() if torch.is_tensor(t) else np.ascontiguousarray(t, np.float32)
    return a.view(np.int32)


def u16(t):
    return t.cpu().contiguous().numpy().view(np.uint16)


def within(got, want, bound, what):
    """|got - want| <= bound element by element, the form of the derived bounds of tests/test_centroid_gpu.py."""
    g = host(got) if torch.is_tensor(got) else np.asarray(got, np.float64)
    assert np.isfinite(g).all(), f"{what}: not fully written (or not finite)"
    worst = float((np.abs(g - want) / np.maximum(bound, 1e-300)).max())
    print(f"[contract] {what}: worst |got - ref| / bound {worst:.3f}")
    assert (np.abs(g - want) <= bound).all(), f"{what}: {worst:.3f} times the bound"


def reranked(score, full, cand, n_docs, what):
    """score[b, c] has the bits of full[b, cand[b, c]] (a device [B, N] score matrix); -inf for a candidate outside [0, N)."""
    got, cand = score.cpu().numpy(), cand.numpy()
    ok = (cand >= 0) & (cand < n_docs)
    assert ok.any() and (~ok).any()
    want = full.cpu().numpy()[np.arange(cand.shape[0])[:, None], np.where(ok, cand, 0)]
    assert np.array_equal(bits(got[ok]), bits(want[ok])), f"{what}: not the bits of the all-pairs scorer"
    assert np.isneginf(got[~ok]).all(), f"{what}: a candidate outside [0, N) must score -inf"
    return ok


def _ms_arrays(cpu):
    return f64(cpu["q"]), cpu["qmask"].numpy(), cpu["dmask"].numpy()


def _argmax_is_decided(q, d, qm, dm):
    """Every top-two gap of the case exceeds the rounding of one f32 dot product (tests/maxsim_cases.gap_floor), so the
    device's argmax must be the reference's."""
    am = mr.maxsim_fwd(q, d, qm, dm)[1]
    return mr.top2_gap(q, d, qm, dm)[am >= 0].min() > mc.gap_floor(q, d)


def test_maxsim_and_normalisation(ops):
    cpu, dv = run_good(ops, "maxsim_fwd")
    (q, qm, dm), d = _ms_arrays(cpu), f64(cpu["d"])
    s_ref, am_ref = mr.maxsim_fwd(q, d, qm, dm)
    assert _argmax_is_decided(q, d, qm, dm) and (am_ref < 0).any() and np.unique(am_ref).size > 3
    close(dv["score"], s_ref, MS["score"], "maxsim_fwd score")
    assert np.array_equal(dv["argmax"].cpu().numpy(), am_ref), "maxsim_fwd argmax"
    fwd_score = dv["score"]

    cpu, dv = run_good(ops, "maxsim_scores")
    close(dv["score"], s_ref, MS["score"], "maxsim_scores score")
    assert np.array_equal(bits(dv["score"]), bits(fwd_score)), "maxsim_scores must give maxsim_fwd's bits"
    full = dv["score"]

    cpu, dv = run_good(ops, "maxsim_bwd")
    assert np.array_equal(cpu["argmax"].numpy(), am_ref)
    dq_ref, dd_ref = mr.maxsim_bwd(q, d, f64(cpu["dscore"]), am_ref)
    close(dv["dq"], dq_ref, MS["grad"], "maxsim_bwd dq")
    close(dv["dd"], dd_ref, MS["grad"], "maxsim_bwd dd")

    cpu, dv = run_good(ops, "maxsim_rerank")
    reranked(dv["score"], full, cpu["cand"], oc.R_N, "maxsim_rerank")

    cpu, fw = run_good(ops, "l2norm_fwd")
    x = f64(cpu["x"])
    y_ref, r_ref = mr.l2norm_fwd(x)
    close(fw["y"], y_ref, MS["norm"], "l2norm_fwd y")
    close(fw["rnorm"], r_ref, MS["norm"], "l2norm_fwd rnorm")

    def forward_outputs(args):             # the backward's y and rnorm are what the forward wrote
        args["y"], args["rnorm"] = fw["y"].contiguous(), fw["rnorm"].contiguous()
    cpu, dv = run_good(ops, "l2norm_bwd", forward_outputs)
    close(dv["dx"], mr.l2norm_bwd(x, f64(cpu["dy"])), MS["norm"], "l2norm_bwd dx")


def test_fp8_index(ops):
    cpu, dv = run_good(ops, "fp8_quantize")
    codes_ref, scale_ref, _ = fp8_ref.quantize(cpu["x"].numpy())
    assert np.array_equal(dv["codes"].cpu().numpy(), codes_ref), "fp8_quantize codes"
    assert np.array_equal(bits(dv["scale"]), bits(scale_ref)) and np.unique(scale_ref).size > 3, "fp8_quantize scale"

    cpu, dv = run_good(ops, "fp8_dequantize")
    assert np.array_equal(cpu["codes"].numpy(), codes_ref)
    corpus = fp8_ref.dequantize(codes_ref, scale_ref)
    assert np.array_equal(bits(dv["y"]), bits(corpus)), "fp8_dequantize is exact"
    corpus_dev = dv["y"].contiguous()

    cpu, dv = run_good(ops, "maxsim_scores_fp8")
    q, qm, dm = _ms_arrays(cpu)
    plain = torch.full((oc.R_B, oc.R_N), float("nan"), device="cuda")
    ops.maxsim_scores(dv["q"], corpus_dev, dv["qmask"], dv["dmask"], plain)
    assert np.array_equal(bits(dv["score"]), bits(plain)), "maxsim_scores_fp8 must give maxsim_scores' bits over the dequantised corpus"
    close(dv["score"], mr.maxsim_fwd(q, corpus.astype(np.float64), qm, dm)[0], MS["score"], "maxsim_scores_fp8 score")
    full = dv["score"]

    cpu, dv = run_good(ops, "maxsim_rerank_fp8")
    reranked(dv["score"], full, cpu["cand"], oc.R_N, "maxsim_rerank_fp8")


def test_residual_index(ops):
    rows, nb = oc.R_N * oc.R_LD, oc.R_NBITS
    cpu, dv = run_good(ops, "residual_compress")
    packed_ref = rr.compress(cpu["x"].numpy().reshape(rows, -1), cpu["codes"].numpy().reshape(rows), cpu["centroids"].numpy(),
                             cpu["cutoffs"].numpy(), nb)
    assert np.array_equal(dv["packed"].cpu().numpy().reshape(rows, -1), packed_ref) and np.unique(packed_ref).size > 8, "residual_compress"

    cpu, dv = run_good(ops, "residual_decompress")
    assert np.array_equal(cpu["packed"].numpy().reshape(rows, -1), packed_ref)
    corpus = rr.decompress(cpu["codes"].numpy().reshape(rows), packed_ref, cpu["centroids"].numpy(), cpu["weights"].numpy(), nb, "f32")
    assert np.array_equal(bits(dv["y"]).reshape(rows, -1), bits(corpus)), "residual_decompress is exact"
    assert (corpus == 0).all(1).sum() == 5, "the rows without a token decompress to zeros"
    corpus_dev = dv["y"].contiguous()

    cpu, dv = run_good(ops, "maxsim_rerank_res")
    q, qm, dm = _ms_arrays(cpu)
    plain = torch.full((oc.R_B, oc.R_C), float("nan"), device="cuda")
    ops.maxsim_rerank(dv["q"], corpus_dev, dv["qmask"], dv["dmask"], dv["cand"], plain)
    assert np.array_equal(bits(dv["score"]), bits(plain)), "maxsim_rerank_res must give maxsim_rerank's bits over the decompressed corpus"
    full = mr.maxsim_fwd(q, corpus.reshape(oc.R_N, oc.R_LD, -1).astype(np.float64), qm, dm)[0]
    cand = cpu["cand"].numpy()
    ok = (cand >= 0) & (cand < oc.R_N)
    got = dv["score"].cpu().numpy()
    assert np.isneginf(got[~ok]).all() and (~ok).sum() == 2
    close(got[ok], full[np.arange(oc.R_B)[:, None], np.where(ok, cand, 0)][ok], MS["score"], "maxsim_rerank_res score")


def test_topk_merge(ops):
    cpu, dv = run_good(ops, "topk_merge")
    scores = cpu["scores"].numpy()
    val, idx = sr.topk_merge(scores, oc.TOPK_ID0 + np.arange(oc.R_C), oc.R_K, state=(cpu["top_val"].numpy(), cpu["top_id"].numpy()))
    assert (idx < oc.TOPK_ID0).any() and (idx >= oc.TOPK_ID0).any(), "the merge keeps entries of both the state and the new scores"
    assert np.array_equal(bits(dv["top_val"]), bits(val)) and np.array_equal(dv["top_id"].cpu().numpy(), idx), "topk_merge"
    cpu, dv = run_good(ops, "topk_merge:ids")
    ids = cpu["ids"].numpy()
    val, idx = sr.topk_merge(np.where(ids >= 0, scores, -np.inf).astype(np.float32), ids, oc.R_K)
    assert np.array_equal(bits(dv["top_val"]), bits(val)) and np.array_equal(dv["top_id"].cpu().numpy(), idx), "topk_merge with ids"


def test_centroids(ops):
    u = 2.0 ** -24
    cpu, dv = run_good(ops, "centroid_scores")
    codes = rr.codes_u16(cpu["codes"].numpy())
    want, mag = cr.centroid_scores(cpu["table"].numpy(), cpu["qmask"].numpy(), codes, oc.R_B, oc.R_LQ)
    # the bound of tests/test_centroid_gpu.py: the maxima are exact, only the f32 sum of the Lq terms rounds
    within(dv["score"], want, 1.01 * (oc.R_LQ - 1) * u * mag, "centroid_scores")
    full = dv["score"]

    cpu, dv = run_good(ops, "centroid_scores_ids")
    reranked(dv["score"], full, cpu["cand"], oc.R_N, "centroid_scores_ids")

    cpu, dv = run_good(ops, "centroid_codes")
    want = cr.centroid_codes(cpu["sim"].numpy(), cpu["mask"].numpy())
    assert want[4] == 0 and want[5] == cr.NONE and np.unique(want).size > 3
    assert np.array_equal(u16(dv["codes"]), want), "centroid_codes"

    cpu, dv = run_good(ops, "centroid_update")
    x, prev, E = f64(cpu["x"]), f64(cpu["prev"]), oc.R_E
    want, counts, sums, mags = cr.centroid_update(x, u16(cpu["codes"]), prev)
    assert np.array_equal(dv["counts"].cpu().numpy(), counts) and counts[2] == 0 and counts.sum() == oc.R_T - 1
    got = host(dv["out"])
    assert np.array_equal(got[2], prev[2]), "a centroid without rows keeps prev"
    # the bound of tests/test_centroid_gpu.py (test_update_counts_exact_centroids_within_the_derived_bound), f32
    live = counts > 0
    nrm = np.sqrt((sums ** 2).sum(1, keepdims=True))[live]
    es = 1.01 * (counts[live, None] - 1) * u * mags[live]
    bound = es / nrm + np.abs(want[live]) * (np.linalg.norm(es, axis=1, keepdims=True) / nrm + 1.01 * (E + 4) * u + u)
    within(got[live], want[live], bound, "centroid_update out")


def test_inverted_lists(ops):
    counts, offsets, members = ivf_ref.lists(rr.codes_u16(oc._tok_codes().numpy()), oc.R_K)
    assert offsets[-1] == oc.IVF_PAIRS and [len(m) for m in members] == [2, 2, 1, 1]
    cpu, dv = run_good(ops, "ivf_count")
    assert np.array_equal(dv["counts"].cpu().numpy(), counts), "ivf_count"
    cpu, dv = run_good(ops, "ivf_offsets")
    assert np.array_equal(dv["offsets"].cpu().numpy(), offsets), "ivf_offsets"
    cpu, dv = run_good(ops, "ivf_fill")
    assert ivf_ref.split(offsets, dv["docs"].cpu().numpy()) == members, "ivf_fill: the lists as sorted sets"

    cpu, dv = run_good(ops, "ivf_mark")
    sets = ivf_ref.candidates(cpu["probes"].numpy().reshape(oc.R_B, oc.R_LQ, oc.R_P), cpu["qmask"].numpy(), members, oc.R_N)
    assert sets == [{1}, {2}], "the masked tokens' probes and the probe past K add nothing"
    assert np.array_equal(dv["bitmap"].cpu().numpy().view(np.uint32), ivf_ref.bitmap(sets, oc.R_N)), "ivf_mark"

    cpu, dv = run_good(ops, "ivf_compact")
    count, cand = ivf_ref.compact(cpu["bitmap"].numpy().view(np.uint32), oc.R_N, cpu["cand"].shape[1])
    assert count.tolist() == [3, 1] and cand.tolist() == [[0, 1], [1, -1]]
    assert np.array_equal(dv["count"].cpu().numpy(), count) and np.array_equal(dv["cand"].cpu().numpy(), cand), "ivf_compact"


TUPLE_KEYS = (("maxsim_tuples_fwd", "maxsim_tuples_bwd", "dot_tuples_fwd", "dot_tuples_bwd", 0),
              ("maxsim_tuples_fwd:query_major", "maxsim_tuples_bwd:query_major", "dot_tuples_fwd:query_major",
               "dot_tuples_bwd:query_major", 1))


def test_tuples_and_distillation(ops):
    seen = []
    for k_fwd, k_bwd, k_dot, k_dot_bwd, layout in TUPLE_KEYS:
        what = f"layout {layout}"
        cpu, dv = run_good(ops, k_fwd)
        assert cpu["layout"] == layout
        (q, qm, dm), d = _ms_arrays(cpu), f64(cpu["d"])
        s_ref, am_ref = tr.maxsim_tuples_fwd(q, d, qm, dm, layout)
        assert _argmax_is_decided(q, d, qm, dm)
        close(dv["score"], s_ref, MS["score"], f"maxsim_tuples_fwd {what} score")
        assert np.array_equal(dv["argmax"].cpu().numpy(), am_ref), f"maxsim_tuples_fwd {what} argmax"
        seen.append(s_ref)

        cpu, dv = run_good(ops, k_bwd)
        assert np.array_equal(cpu["argmax"].numpy(), am_ref)
        dq_ref, dd_ref = tr.maxsim_tuples_bwd(q, d, f64(cpu["dscore"]), am_ref, layout)
        close(dv["dq"], dq_ref, MS["grad"], f"maxsim_tuples_bwd {what} dq")
        close(dv["dd"], dd_ref, MS["grad"], f"maxsim_tuples_bwd {what} dd")

        tol = tc.TOL["dot_f32"]
        cpu, dv = run_good(ops, k_dot)
        q, d = f64(cpu["q"]), f64(cpu["d"])
        close(dv["score"], tr.dot_tuples_fwd(q, d, layout), tol["score"], f"dot_tuples_fwd {what} score")
        cpu, dv = run_good(ops, k_dot_bwd)
        dq_ref, dd_ref = tr.dot_tuples_bwd(q, d, f64(cpu["dscore"]), layout)
        close(dv["dq"], dq_ref, tol["grad"], f"dot_tuples_bwd {what} dq")
        close(dv["dd"], dd_ref, tol["grad"], f"dot_tuples_bwd {what} dd")
    assert not np.allclose(seen[0], seen[1]), "the two layouts pair queries and documents differently"

    for key, kind, ref in (("distill_kl", "kl", tr.distill_kl), ("margin_mse", "mse", tr.margin_mse)):
        cpu, dv = run_good(ops, key)
        loss_ref, g_ref = ref(f64(cpu["student"]), f64(cpu["teacher"]))
        close(dv["loss"], [loss_ref], tc.TOL[kind]["loss"], f"{key} loss")
        close(dv["dstudent"], g_ref, tc.TOL[kind]["grad"], f"{key} dstudent")
        assert (dv["dstudent"].cpu().numpy()[np.isneginf(cpu["teacher"].numpy())] == 0).all(), f"{key}: an absent column gets zero gradient"


def test_every_good_case_runs_on_the_device():
    import inspect
    import sys
    src = inspect.getsource(sys.modules[__name__])
    for key in oc.CASES:
        assert f'"{key}"' in src, f"no GPU test runs the good call of {key}"
