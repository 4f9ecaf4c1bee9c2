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
from tests import layer_cases as lc
from tests import ops_contract_cases as oc
from tests import rowwise_cases as rc
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


def test_every_good_case_runs_on_the_device():
    import inspect
    import sys
    src = inspect.getsource(sys.modules[__name__])
    for key in oc.CASES:
        assert f'"{key}"' in src, f"no GPU test runs the good call of {key}"
