"""The layers (polus_amd/layers.py Dense and Dropout) and the arena's transposed shadows (polus_amd/tensor.py) on every dispatch
path, against the float64 reference of tests/layer_cases.py.

A stand-alone layer is Sequential([Dense(...)], compute_dtype=mode, input_dim=H); weights are set with Variable.assign, so the
bf16 shadow and its transposed twin are refreshed the way the product refreshes them.  Every output and gradient buffer is
NaN- or sentinel-filled before the call, every check prints the path taken and the error it measured before it asserts
(pytest -s shows them), and `layer._thin` is held to the restated gate after every forward, so that no test compares the GEMM
path with itself.  The bounds are those of tests/layer_cases.py."""
import collections

import numpy as np
import pytest
import torch

from tests import layer_cases as lc
from tests.util import TOL, dev, dropout_keep_np, host, relerr, rounded

pytestmark = pytest.mark.gpu

F32, BF16 = torch.float32, torch.bfloat16
SENTINEL = -1536.0             # finite, exact in bf16, far outside every reference's range
ENV = "POLUS_DENSE_THIN"
PATHS = (None, "0")            # POLUS_DENSE_THIN unset: the thin kernels where the gate allows; "0": the GEMM path


@pytest.fixture(scope="module")
def ops():
    from polus_amd import ops as _ops
    _ops.set_dynamic_params(None)            # the dropout seed as passed (no per-step salt)
    return _ops


def _path(monkeypatch, env):
    if env is None:
        monkeypatch.delenv(ENV, raising=False)
    else:
        monkeypatch.setenv(ENV, env)


def _build(engine, H, C, act=None, use_bias=True, out="f32"):
    from polus_amd.layers import Dense
    from polus_amd.models import Sequential
    odt = None if act else (F32 if out == "f32" else lc.DT[engine])
    model = Sequential([Dense(C, activation=act, use_bias=use_bias, out_dtype=odt)], compute_dtype=engine, input_dim=H)
    return model, model.layers[0]


def _assign(layer, w, b):
    layer.w.assign(w.astype(np.float32))
    if b is not None:
        layer.b.assign(b.astype(np.float32))
    if layer.w.compute_t is not None:
        assert torch.equal(layer.w.compute_t, layer.w.compute.t())


def _poison(layer, rows, engine, y_dtype):
    """NaN into every buffer the layer hands out or goes through for this shape (they are cached by shape and dtype)."""
    H, C, dt = layer.in_features, layer.units, lc.DT[engine]
    for key, shape, d in (("y", (rows, C), lc.DT[y_dtype]), ("dx", (rows, H), dt), ("dy_cast", (rows, C), dt),
                          ("u", (rows, C), dt), ("du", (rows, C), dt)):
        layer._buf(key, shape, d, "cuda").fill_(float("nan"))


def _run(layer, engine, x_t, dy_t, accumulate=False, need_dx=True, resid=None, y_dtype="f32"):
    """One forward and backward; every result cloned (the layer reuses its buffers)."""
    rows = x_t.numel() // layer.in_features
    _poison(layer, rows, engine, y_dtype)
    y = layer.forward(x_t)
    thin = layer._thin
    dx = layer.backward(dy_t, accumulate, need_dx=need_dx, dx_resid=resid)
    torch.cuda.synchronize()
    return {"y": y.clone(), "dx": None if dx is None else dx.clone(), "dw": layer.w.grad.clone(),
            "db": None if layer.b is None else layer.b.grad.clone(), "thin": thin}


def _check(tag, got, ref, bnd, keys=("y", "dx", "dw", "db")):
    path = "thin" if got["thin"] else "gemm"
    for k in keys:
        if got[k] is None and k == "db":
            continue
        g = host(got[k]).reshape(ref[k].shape)
        e = relerr(g, ref[k])
        print(f"[layers] {tag} [{path}] {k}: rel err {e:.3e} (bound {bnd[k]:.1e})")
        assert np.isfinite(g).all(), f"{tag} [{path}] {k}: not fully written (or not finite)"
        assert e <= bnd[k], f"{tag} [{path}] {k}: rel err {e:.3e} > {bnd[k]:.1e}"


def _spy(monkeypatch, ops, names=("dense_thin_fwd", "dense_thin_bwd", "dense_bwd_params", "gemm", "cast", "act_bwd")):
    """Count the calls the layers make into polus_amd.ops (they look the functions up on the module at call time)."""
    calls = collections.Counter()
    for n in names:
        def wrap(*a, _orig=getattr(ops, n), _n=n, **k):
            calls[_n] += 1
            return _orig(*a, **k)
        monkeypatch.setattr(ops, n, wrap)
    return calls


# ------------------------------------------------------------------------------------------------- 1. the gate
@pytest.mark.parametrize("engine,hs", [("bf16", (0, 4, 8, 12, 504, 512, 520, 1024, 1032)),
                                       ("f32", (0, 2, 4, 6, 252, 256, 260, 1024, 1028))])
def test_gate_equals_its_restatement(ops, engine, hs):
    seen = set()
    for H in hs:
        for C in (0, 1, 4, 5, 8, 9):
            got, want = ops.dense_thin_supported(lc.DT[engine], H, C), lc.thin_supported(engine, H, C)
            seen.add(got)
            assert got == want, f"polus_dense_thin_supported({engine}, H={H}, C={C}) = {got}, restated {want}"
    for H, C in lc.SHAPES:
        assert ops.dense_thin_supported(lc.DT[engine], H, C) == lc.thin_supported(engine, H, C), (H, C)
    assert seen == {True, False}
    print(f"[layers] gate {engine}: {len(hs) * 6} boundary shapes agree")


# ------------------------------------------------------------------------------------------------- 2. both paths, every case
@pytest.mark.parametrize("case", lc.CASES, ids=lambda c: c.name)
def test_thin_and_gemm_paths_match_the_reference_and_each_other(ops, case, monkeypatch):
    e, H, C = case.engine, case.H, case.C
    x, w, b, dy = lc.dense_inputs(e, case.rows, H, C, case.seed, case.use_bias)
    model, layer = _build(e, H, C, use_bias=case.use_bias, out=case.out)
    _assign(layer, w, b)
    x_t = dev(x, lc.DT[e])
    # An f32 dy reaches the two paths of the bf16 engine as two different tensors (the thin backward reads it as it is, the
    # GEMM backward casts it to bf16), so there the paths are held to each other twice: on a dy of bf16 values, which both
    # see alike, within the sum of their two bounds; and on the general dy within that sum plus the distance between their
    # two float64 references (the triangle inequality; up to 6e-2 of max|db| at 4099 rows, where db is a sum of 4099 signs).
    for dy_kind in (("f32",) if e == "f32" else ("f32", "bf16 values")):
        dyk = dy if dy_kind == "f32" else rounded(dy, BF16)
        dy_t = dev(dyk, F32)
        runs = []
        for env in PATHS:
            _path(monkeypatch, env)
            model.arena.grads.fill_(float("nan"))
            got = _run(layer, e, x_t, dy_t, y_dtype=case.y_dtype)
            want = lc.layer_thin(e, H, C, env=env)
            assert got["thin"] == want, f"{case.name} under {ENV}={env}: _thin is {got['thin']}, the gate says {want}"
            assert got["y"].dtype == lc.DT[case.y_dtype] and got["dx"].dtype == lc.DT[e]
            ref = lc.dense_reference(x, w, b, dyk, **lc.path_roundings(e, want, "f32"))
            bnd = lc.bounds(e, want, case.y_dtype)
            _check(f"{case.name} dy {dy_kind}", got, ref, bnd)
            runs.append((got, bnd, ref))
        assert runs[0][0]["thin"] == case.thin and not runs[1][0]["thin"]
        (a, ba, ra), (g, bg, rg) = runs
        for k in ("y", "dx", "dw", "db"):
            if a[k] is None:
                continue
            apart = relerr(ra[k], rg[k])
            if e == "f32" or dy_kind != "f32":
                assert apart == 0.0
            d = relerr(host(a[k]), host(g[k]))
            allowed = ba[k] + bg[k] + apart
            print(f"[layers] {case.name} dy {dy_kind} {k}: {'thin' if a['thin'] else 'gemm'} vs gemm {d:.3e} "
                  f"(bound {ba[k] + bg[k]:.1e} + references apart {apart:.1e})")
            assert d <= allowed, f"{case.name} {k}: the two paths differ by {d:.3e} > {allowed:.1e}"


# ------------------------------------------------------------------------------------------------- 3. views
def _framed(a, dtype, width, off, fill=1e4):
    """`a` [rows, cols] as a column slice of a wider device buffer filled with `fill`."""
    rows, cols = a.shape
    buf = torch.full((rows, width), fill, dtype=dtype, device="cuda")
    buf[:, off:off + cols] = dev(a, dtype)
    v = buf[:, off:off + cols]
    assert v.data_ptr() == buf.data_ptr() + off * buf.element_size() and buf.data_ptr() % 256 == 0
    return v


def _x_geometry(kind, engine, H):
    """(buffer width, column offset) of an x view; q = elements per 16 bytes."""
    q = 16 // lc.ES[engine]
    return {"aligned": (H + 2 * q, q),             # 16-byte aligned base and row stride, ldx != H: still thin
            "shift1": (H + 2 * q, q + 1),          # the same slice one element on: base misaligned
            "stride": (H + q + 1, 0)}[kind]        # aligned base, row stride no multiple of 16 bytes


@pytest.mark.parametrize("kind", ["aligned", "shift1", "stride"])
@pytest.mark.parametrize("H,C", [(264, 8), (768, 4)])
@pytest.mark.parametrize("engine", lc.ENGINES)
def test_x_as_a_column_slice_of_a_wider_buffer(ops, engine, H, C, kind, monkeypatch):
    _path(monkeypatch, None)
    rows = 37
    x, w, b, dy = lc.dense_inputs(engine, rows, H, C, seed=H + C)
    model, layer = _build(engine, H, C)
    _assign(layer, w, b)
    width, off = _x_geometry(kind, engine, H)
    xv = _framed(x, lc.DT[engine], width, off)
    want = lc.layer_thin(engine, H, C, base_elems=off, row_stride=width)
    assert want == (kind == "aligned")
    dy_t = dev(dy, F32)
    model.arena.grads.fill_(float("nan"))
    got = _run(layer, engine, xv, dy_t)
    assert got["thin"] == want, f"{kind}: _thin is {got['thin']}, the gate says {want}"
    assert xv.stride(0) != H
    ref = lc.dense_reference(x, w, b, dy, **lc.path_roundings(engine, want, "f32"))
    _check(f"x view {kind} {engine} H{H} C{C}", got, ref, lc.bounds(engine, want, "f32"))
    if want:                                       # the same kernels on the contiguous copy: the same bits
        model.arena.grads.fill_(float("nan"))
        flat = _run(layer, engine, xv.contiguous(), dy_t)
        assert flat["thin"]
        for k in ("y", "dx", "dw", "db"):
            assert torch.equal(got[k], flat[k]), f"{k} depends on the row stride of x"


@pytest.mark.parametrize("env", PATHS, ids=["thin", "gemm"])
@pytest.mark.parametrize("engine", lc.ENGINES)
def test_three_dimensional_input(ops, engine, env, monkeypatch):
    _path(monkeypatch, env)
    B, S, H, C = 3, 13, 264, 8
    x, w, b, dy = lc.dense_inputs(engine, B * S, H, C, seed=77)
    model, layer = _build(engine, H, C)
    _assign(layer, w, b)
    model.arena.grads.fill_(float("nan"))
    got = _run(layer, engine, dev(x, lc.DT[engine]).view(B, S, H), dev(dy, F32).view(B, S, C))
    want = lc.layer_thin(engine, H, C, env=env)
    assert got["thin"] == want
    assert tuple(got["y"].shape) == (B, S, C) and got["dx"].numel() == B * S * H
    ref = lc.dense_reference(x, w, b, dy, **lc.path_roundings(engine, want, "f32"))
    _check(f"3-D x {engine}", got, ref, lc.bounds(engine, want, "f32"))


@pytest.mark.parametrize("kind", ["slice", "stride2"])
@pytest.mark.parametrize("env", PATHS, ids=["thin", "gemm"])
@pytest.mark.parametrize("engine", lc.ENGINES)
def test_dy_as_a_non_contiguous_view(ops, engine, env, kind, monkeypatch):
    """slice: unit column stride, row stride != C (passed on as lddy); stride2: every other column (the .contiguous() branch)."""
    _path(monkeypatch, env)
    rows, H, C = 37, 264, 8
    x, w, b, dy = lc.dense_inputs(engine, rows, H, C, seed=91)
    model, layer = _build(engine, H, C)
    _assign(layer, w, b)
    if kind == "slice":
        dyv = _framed(dy, F32, C + 3, 1)
        assert dyv.stride() == (C + 3, 1)
    else:
        buf = torch.full((rows, 2 * C), 1e4, dtype=F32, device="cuda")
        buf[:, ::2] = dev(dy, F32)
        dyv = buf[:, ::2]
        assert dyv.stride() == (2 * C, 2)
    assert not dyv.is_contiguous()
    model.arena.grads.fill_(float("nan"))
    got = _run(layer, engine, dev(x, lc.DT[engine]), dyv)
    want = lc.layer_thin(engine, H, C, env=env)
    assert got["thin"] == want
    ref = lc.dense_reference(x, w, b, dy, **lc.path_roundings(engine, want, "f32"))
    _check(f"dy {kind} {engine}", got, ref, lc.bounds(engine, want, "f32"))


# ------------------------------------------------------------------------------------------------- 4. backward choices
# dX = dY . W + resid in the epilogue of the dX GEMM.  f32 engine: a tensor stored in f32, tests.util.TOL (measured 7.5e-8).
# bf16 engine: no bound existed; measured against the float64 reference on an MI355X 2.07e-3 of max|ref| (one rounding of the
# f32 sum to bf16: half an ulp is 2e-3 to 3.9e-3 of an element).  Bound = twice the measured value: a second rounding
# step, say of dY . W before resid is added, costs up to another half ulp of every element, a dropped term all of it.
RESID_DX_TOL = {"f32": TOL[F32], "bf16": 4.2e-3}


def _thin_layer(engine, monkeypatch, rows=37, H=264, C=8, seed=123):
    _path(monkeypatch, None)
    x, w, b, dy = lc.dense_inputs(engine, rows, H, C, seed=seed)
    model, layer = _build(engine, H, C)
    _assign(layer, w, b)
    return model, layer, x, w, b, dy


@pytest.mark.parametrize("dy_dtype", ["f32", "compute"])
@pytest.mark.parametrize("engine", lc.ENGINES)
def test_thin_backward_after_a_thin_forward(ops, engine, dy_dtype, monkeypatch):
    model, layer, x, w, b, dy = _thin_layer(engine, monkeypatch)
    dyd = "f32" if dy_dtype == "f32" else engine
    dy = rounded(dy, lc.DT[dyd])
    calls = _spy(monkeypatch, ops)
    model.arena.grads.fill_(float("nan"))
    got = _run(layer, engine, dev(x, lc.DT[engine]), dev(dy, lc.DT[dyd]))
    assert got["thin"]
    assert calls == {"dense_thin_fwd": 1, "dense_thin_bwd": 1}, dict(calls)
    ref = lc.dense_reference(x, w, b, dy, **lc.path_roundings(engine, True, dyd))
    _check(f"thin backward, dy {dyd}, {engine}", got, ref, lc.bounds(engine, True, "f32"))


def test_dy_of_another_dtype_falls_back_to_the_gemm_backward(ops, monkeypatch):
    """bf16 dy in the f32 engine after a thin forward: cast (widening, exact), then dense_bwd_params and the dX GEMM, so the
    f32 GEMM-path bounds hold against the reference on the bf16-rounded dy."""
    engine = "f32"
    model, layer, x, w, b, dy = _thin_layer(engine, monkeypatch)
    calls = _spy(monkeypatch, ops)
    model.arena.grads.fill_(float("nan"))
    got = _run(layer, engine, dev(x, F32), dev(dy, BF16))
    assert got["thin"]
    assert calls == {"dense_thin_fwd": 1, "cast": 1, "dense_bwd_params": 1, "gemm": 1}, dict(calls)
    ref = lc.dense_reference(x, w, b, dy, **lc.path_roundings(engine, False, "bf16"))
    assert not np.array_equal(ref["du"], dy)
    bnd = dict(lc.bounds(engine, False, "f32"), y=lc.bounds(engine, True, "f32")["y"])
    _check("bf16 dy, f32 engine (fallback)", got, ref, bnd)


@pytest.mark.parametrize("engine", lc.ENGINES)
def test_dx_resid_falls_back_and_is_added(ops, engine, monkeypatch):
    """dx_resid as the strided d3[:, 0, :] of BertModel.backward's pooler call: dx = dy . W + resid, dW and db unchanged."""
    model, layer, x, w, b, dy = _thin_layer(engine, monkeypatch)
    rows, H = x.shape
    r = np.random.Generator(np.random.PCG64(4))
    d3 = rounded(r.standard_normal((rows, 3, H)) * 0.05, lc.DT[engine])      # the size of dy . W: neither term hides the other
    d3_t = dev(d3, lc.DT[engine])
    resid = d3_t[:, 0, :]
    assert resid.stride() == (3 * H, 1)
    calls = _spy(monkeypatch, ops)
    model.arena.grads.fill_(float("nan"))
    got = _run(layer, engine, dev(x, lc.DT[engine]), dev(dy, F32), resid=resid)
    assert got["thin"]
    want_calls = {"dense_thin_fwd": 1, "dense_bwd_params": 1, "gemm": 1}
    if engine == "bf16":
        want_calls["cast"] = 1
    assert calls == want_calls, dict(calls)
    ref = lc.dense_reference(x, w, b, dy, resid=d3[:, 0, :], **lc.path_roundings(engine, False, "f32"))
    plain = lc.dense_reference(x, w, b, dy, **lc.path_roundings(engine, False, "f32"))
    assert relerr(plain["dx"], ref["dx"]) > 0.3 and relerr(d3[:, 0, :], ref["dx"]) > 0.3      # the bound sees either term missing
    bnd = dict(lc.bounds(engine, False, "f32"), y=lc.bounds(engine, True, "f32")["y"], dx=RESID_DX_TOL[engine])
    _check(f"dx_resid {engine} (fallback)", got, ref, bnd)
    assert torch.equal(d3_t, dev(d3, lc.DT[engine])), "dx_resid was written to"


@pytest.mark.parametrize("env", PATHS, ids=["thin", "gemm"])
@pytest.mark.parametrize("engine", lc.ENGINES)
def test_need_dx_false_returns_none_and_leaves_the_parameter_gradients_alone(ops, engine, env, monkeypatch):
    model, layer, x, w, b, dy = _thin_layer(engine, monkeypatch)
    _path(monkeypatch, env)
    x_t, dy_t = dev(x, lc.DT[engine]), dev(dy, F32)
    model.arena.grads.fill_(float("nan"))
    full = _run(layer, engine, x_t, dy_t)
    model.arena.grads.fill_(float("nan"))
    none = _run(layer, engine, x_t, dy_t, need_dx=False)
    want = lc.layer_thin(engine, 264, 8, env=env)
    assert full["thin"] == want and none["thin"] == want
    assert none["dx"] is None and full["dx"] is not None
    ref = lc.dense_reference(x, w, b, dy, **lc.path_roundings(engine, want, "f32"))
    _check(f"need_dx=False {engine}", none, ref, lc.bounds(engine, want, "f32"), keys=("y", "dw", "db"))
    if want:       # dense_thin.hip: fixed summation order, the same whether dx is written or not
        assert torch.equal(full["dw"], none["dw"]) and torch.equal(full["db"], none["db"]), "thin dW / db depend on dx"


@pytest.mark.parametrize("lead", [False, True], ids=["dense_first", "dropout_first"])
def test_sequential_skips_dx_of_the_first_parameterised_layer_only(ops, lead, monkeypatch):
    from polus_amd.layers import Dense, Dropout
    from polus_amd.models import Sequential
    _path(monkeypatch, None)
    rows, H, U, C = 37, 24, 16, 4
    layers = ([Dropout(0.0)] if lead else []) + [Dense(U, activation="relu"), Dense(C)]
    model = Sequential(layers, compute_dtype="f32", input_dim=H)
    d1, d2 = model.layers[-2], model.layers[-1]
    r = np.random.Generator(np.random.PCG64(8))
    f = lambda a: rounded(a, F32)
    x, w1, b1 = f(r.standard_normal((rows, H))), f(r.standard_normal((U, H)) * 0.3), f(r.standard_normal(U))
    w2, b2, dy = f(r.standard_normal((C, U)) * 0.3), f(r.standard_normal(C)), f(r.standard_normal((rows, C)) * 0.1)
    _assign(d1, w1, b1)
    _assign(d2, w2, b2)
    seen = {}
    for name, l in (("d1", d1), ("d2", d2)):
        def rec(dy_, accumulate=False, need_dx=True, dx_resid=None, _l=l, _n=name, _orig=l.backward):
            seen[_n] = need_dx
            return _orig(dy_, accumulate, need_dx=need_dx, dx_resid=dx_resid)
        monkeypatch.setattr(l, "backward", rec)
    model.arena.grads.fill_(float("nan"))
    y = model(dev(x, F32), training=True)
    out = model.backward(dev(dy, F32))
    torch.cuda.synchronize()
    assert seen == {"d1": False, "d2": True}, seen
    assert out is None
    assert d2._thin and not d1._thin
    top = lc.dense_reference(x, w1, b1, act="relu")
    ref2 = lc.dense_reference(top["y"], w2, b2, dy)
    ref1 = lc.dense_reference(x, w1, b1, ref2["dx"], act="relu")
    for tag, got, ref, tol in (("y", y, ref2["y"], TOL[F32]), ("d2.dw", d2.w.grad, ref2["dw"], lc.THIN_PARAM_TOL),
                               ("d2.db", d2.b.grad, ref2["db"], lc.THIN_PARAM_TOL),
                               ("d1.dw", d1.w.grad, ref1["dw"], lc.GEMM_DW_TOL["f32"]), ("d1.db", d1.b.grad, ref1["db"], lc.GEMM_DB_TOL["f32"])):
        e = relerr(host(got), ref)
        print(f"[layers] two stacked Dense {tag}: rel err {e:.3e} (bound {tol:.1e})")
        assert np.isfinite(e) and e <= tol, tag


# ------------------------------------------------------------------------------------------------- 5. accumulate, containment
@pytest.mark.parametrize("accumulate", [False, True], ids=["write", "accumulate"])
@pytest.mark.parametrize("env", PATHS, ids=["thin", "gemm"])
@pytest.mark.parametrize("H,C", [(264, 5), (136, 3)])
@pytest.mark.parametrize("engine", lc.ENGINES)
def test_gradient_windows_accumulate_and_nothing_else_is_written(ops, engine, H, C, env, accumulate, monkeypatch):
    _path(monkeypatch, env)
    rows = 37
    x, w, b, dy = lc.dense_inputs(engine, rows, H, C, seed=H * C)
    model, layer = _build(engine, H, C)
    _assign(layer, w, b)
    grads, wv, bv = model.arena.grads, layer.w, layer.b
    assert wv.offset + wv.size < bv.offset, "no alignment gap between the two windows"
    assert bv.offset + bv.size < grads.numel(), "no padded tail"
    inside = torch.zeros(grads.numel(), dtype=torch.bool, device="cuda")
    inside[wv.offset:wv.offset + wv.size] = True
    inside[bv.offset:bv.offset + bv.size] = True
    r = np.random.Generator(np.random.PCG64(17))
    g0w, g0b = r.integers(-4, 5, size=(C, H)).astype(np.float64) / 4, r.integers(-4, 5, size=C).astype(np.float64) / 4
    if accumulate:
        grads.fill_(SENTINEL)
        wv.grad.copy_(dev(g0w, F32))
        bv.grad.copy_(dev(g0b, F32))
    else:
        grads.fill_(float("nan"))
    got = _run(layer, engine, dev(x, lc.DT[engine]), dev(dy, F32), accumulate=accumulate)
    want = lc.layer_thin(engine, H, C, env=env)
    assert got["thin"] == want
    ref = lc.dense_reference(x, w, b, dy, **lc.path_roundings(engine, want, "f32"))
    bnd = lc.bounds(engine, want, "f32")
    tag = f"{'accumulate' if accumulate else 'write'} {engine} H{H} C{C}"
    if accumulate:
        # g0 + dW: the kernel's own error, plus one f32 rounding of the final addition
        for k, g0 in (("dw", g0w), ("db", g0b)):
            g = host(got[k])
            err = np.abs(g - (g0 + ref[k])).max()
            allowed = bnd[k] * np.abs(ref[k]).max() + 2.0 ** -24 * np.abs(g0 + ref[k]).max()
            print(f"[layers] {tag} [{'thin' if want else 'gemm'}] {k}: abs err {err:.3e} (allowed {allowed:.3e})")
            assert np.isfinite(g).all() and err <= allowed, f"{tag} {k}: {err:.3e} > {allowed:.3e}"
        outside = grads[~inside]
        assert bool((outside == SENTINEL).all()), f"{tag}: {int((outside != SENTINEL).sum())} elements written outside the windows"
    else:
        _check(tag, got, ref, bnd, keys=("dw", "db"))
        outside = grads[~inside]
        assert bool(torch.isnan(outside).all()), f"{tag}: {int((~torch.isnan(outside)).sum())} elements written outside the windows"
    print(f"[layers] {tag}: {int((~inside).sum())} elements outside the windows untouched "
          f"(gap {bv.offset - wv.offset - wv.size}, tail {grads.numel() - bv.offset - bv.size})")


# ------------------------------------------------------------------------------------------------- 6. activated layers
@pytest.mark.parametrize("act", lc.ACTS)
@pytest.mark.parametrize("engine", lc.ENGINES)
def test_activated_dense_stays_on_the_gemm_path(ops, engine, act, monkeypatch):
    _path(monkeypatch, None)
    rows, H, C = 37, 264, 4
    x, w, b, dy = lc.dense_inputs(engine, rows, H, C, seed=len(act) + 40)
    dy = rounded(dy, lc.DT[engine])                 # an activated layer gets its dy from the layer above, in the compute dtype
    model, layer = _build(engine, H, C, act=act)
    _assign(layer, w, b)
    assert lc.thin_supported(engine, H, C) and not lc.layer_thin(engine, H, C, activation=act)
    calls = _spy(monkeypatch, ops)
    model.arena.grads.fill_(float("nan"))
    got = _run(layer, engine, dev(x, lc.DT[engine]), dev(dy, lc.DT[engine]), y_dtype=engine)
    assert got["thin"] is False
    assert calls == {"gemm": 2, "act_bwd": 1, "dense_bwd_params": 1}, dict(calls)
    ref = lc.dense_reference(x, w, b, dy, act=act, **lc.path_roundings(engine, False, engine, act=act))
    _check(f"Dense(4, {act}) {engine}", got, ref, lc.bounds(engine, False, engine))


# ------------------------------------------------------------------------------------------------- 7. transposed shadows
TR_MATS = ((4, 768),       # 8-byte vector body
           (3, 128),       # scalar body
           (132, 68),      # vector body, ragged tiles in both directions
           (65, 63),       # scalar body, ragged tiles
           (1, 8),         # scalar body, a single row
           (64, 64))       # vector body, one full tile
TR_SENTINEL = 0x7A5C


def test_transpose_bf16_batched_every_body_and_nothing_outside(ops):
    r = np.random.Generator(np.random.PCG64(64))
    segs, off, t0 = [], 64, 0                       # a 64-element gap in front, 64-aligned offsets, a gap behind
    for R, C in TR_MATS:
        segs.append((off, R, C, t0))
        off += (R * C + 63) // 64 * 64 + (64 if R == 3 else 0)
        t0 += ((R + 63) // 64) * ((C + 63) // 64)
    n = off + 64
    assert [((R | C) & 3) == 0 for R, C in TR_MATS] == [True, False, True, False, False, True]
    bits = r.integers(0, 0x7F80, size=n).astype(np.int16)                 # finite bf16 bit patterns, no two windows alike
    src = torch.from_numpy(bits).cuda().view(BF16)
    dst = torch.full((n,), TR_SENTINEL, dtype=torch.int16, device="cuda").view(BF16)
    table = torch.tensor(segs, dtype=torch.int64).cuda()
    ops.transpose_bf16_batched(src, dst, table, len(segs), t0)
    torch.cuda.synchronize()
    s16, d16 = src.view(torch.int16), dst.view(torch.int16)
    assert np.array_equal(s16.cpu().numpy(), bits), "the source was written to"
    inside = torch.zeros(n, dtype=torch.bool, device="cuda")
    for o, R, C, _ in segs:
        want = s16[o:o + R * C].view(R, C).t().contiguous().view(-1)
        got = d16[o:o + R * C]
        bad = int((got != want).sum())
        print(f"[layers] transpose_bf16_batched ({R}, {C}) [{'vector' if ((R | C) & 3) == 0 else 'scalar'} body]: {bad} of {R * C} elements differ")
        assert bad == 0, f"({R}, {C}): {bad} elements differ from src.t()"
        inside[o:o + R * C] = True
    stray = int((d16[~inside] != TR_SENTINEL).sum())
    print(f"[layers] transpose_bf16_batched: {stray} of {int((~inside).sum())} elements outside the windows written")
    assert stray == 0


def _shadow_model():
    from polus_amd.layers import Dense
    from polus_amd.models import SequentialPolusClassifier
    # W [132, 68]: vector body, ragged tiles; W [65, 132]: scalar body, ragged tiles; W [3, 65]: scalar body, one tile
    return SequentialPolusClassifier([Dense(132, activation="relu"), Dense(65, activation="relu"), Dense(3)],
                                     compute_dtype="bf16", input_dim=68)


def _shadows_consistent(model, tag):
    arena = model.arena
    torch.cuda.synchronize()
    inside = torch.zeros(arena.size, dtype=torch.bool, device="cuda")
    mats = [v for v in arena.vars if v.matrix and len(v.shape) == 2]
    assert [v.shape for v in mats] == [(132, 68), (65, 132), (3, 65)]
    for v in mats:
        assert torch.equal(v.compute, v.value.to(BF16)), f"{tag}: bf16 shadow of {v.name} is stale"
        assert torch.equal(v.compute_t, v.compute.t()), f"{tag}: transposed shadow of {v.name} differs from its shadow"
        inside[v.offset:v.offset + v.size] = True
    stray = int((arena.shadow_t[~inside].view(torch.int16) != 0).sum())
    print(f"[layers] {tag}: 3 transposed shadows equal their shadows, {stray} elements written outside them")
    assert stray == 0


def test_transposed_shadows_follow_assign(ops):
    model = _shadow_model()
    _shadows_consistent(model, "after finalize")
    r = np.random.Generator(np.random.PCG64(12))
    for v in model.trainable_weights:
        v.assign(r.standard_normal(v.shape).astype(np.float32))
    _shadows_consistent(model, "after Variable.assign")


@pytest.mark.parametrize("in_backward", ["1", "0"], ids=["sublist", "whole_arena"])
def test_transposed_shadows_follow_an_optimizer_step(ops, in_backward, monkeypatch):
    """POLUS_UPDATE_IN_BACKWARD=1: refresh_transposed_of on each window's variables; 0: refresh_transposed on the whole arena."""
    from polus_amd.losses import SparseCategoricalCrossentropy
    from polus_amd.optimizers import Adam
    from polus_amd.training import ClassifierTrainer
    monkeypatch.setenv("POLUS_UPDATE_IN_BACKWARD", in_backward)
    model = _shadow_model()
    r = np.random.Generator(np.random.PCG64(13))
    before = [v.compute.clone() for v in model.trainable_weights]
    trainer = ClassifierTrainer(model, Adam(1e-2), SparseCategoricalCrossentropy(grad_dtype=model.compute_dtype))
    x = r.standard_normal((32, 68)).astype(np.float32)
    labels = r.integers(0, 3, size=32).astype(np.int32)
    loss = float(trainer.train_step(x, labels))
    assert np.isfinite(loss)
    assert (trainer._updater() is not None) == (in_backward == "1")
    for v, old in zip(model.trainable_weights, before):
        if v.matrix:
            assert not torch.equal(v.compute, old), f"{v.name} did not move: the step checks nothing"
    _shadows_consistent(model, f"after a step, POLUS_UPDATE_IN_BACKWARD={in_backward}")


# ------------------------------------------------------------------------------------------------- 8. Dropout
def _drop_seed(seed, calls):
    return (seed + 0x9E3779B1 * calls) & 0xFFFFFFFF


def _drop_check(tag, y, x64, keep, rate, dtype):
    inv = np.float32(1.0) / (np.float32(1.0) - np.float32(rate))
    g = host(y).reshape(-1)
    k = keep.astype(bool)
    assert np.array_equal(g != 0, k), f"{tag}: {int(((g != 0) != k).sum())} elements kept / dropped against the mask definition"
    if dtype == F32:
        want = (x64.astype(np.float32) * inv).astype(np.float64)          # one f32 multiply
        assert np.array_equal(g[k], want[k]), f"{tag}: kept values are not x * f32(1 / (1 - rate)) bitwise"
        err = 0.0
    else:
        want = x64 * float(inv)
        err = float((np.abs(g[k] - want[k]) / np.abs(want[k])).max())
        assert err <= 2.0 ** -8, f"{tag}: kept values are {err:.3e} from x / (1 - rate), more than one bf16 rounding"
    assert not g[~k].any()
    print(f"[layers] {tag}: {int(k.sum())} of {k.size} kept, as the mask definition says; kept values rel err {err:.3e}")


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("rate", [0.1, 0.5])
def test_dropout_layer_is_the_mask_definition(ops, rate, dtype):
    from polus_amd.layers import Dropout
    n, seed = 4099, 0xC0FFEE
    p = float(np.float32(rate))                      # the rate as the kernel's float argument holds it
    r = np.random.Generator(np.random.PCG64(n))
    x64 = rounded(r.uniform(0.5, 1.5, size=n) * r.choice([-1.0, 1.0], size=n), dtype)        # never zero
    x_t = dev(x64, dtype)
    layer = Dropout(rate, seed=seed)
    keep1, keep2 = (dropout_keep_np(_drop_seed(seed, c), p, 0, n) for c in (1, 2))
    assert not np.array_equal(keep1, keep2) and abs(keep1.mean() - (1 - rate)) < 0.03
    y1 = layer.forward(x_t, training=True).clone()
    assert layer.calls == 1
    _drop_check(f"Dropout({rate}) first forward", y1, x64, keep1, rate, dtype)
    # a non-contiguous x (every other column of [n, 2]) on the second call: the second mask, the contiguous copy's values
    wide = torch.full((n, 2), 1e4, dtype=dtype, device="cuda")
    wide[:, 0] = x_t
    y2 = layer.forward(wide[:, 0], training=True).clone()
    assert layer.calls == 2 and not wide[:, 0].is_contiguous()
    _drop_check(f"Dropout({rate}) second forward, strided x", y2, x64, keep2, rate, dtype)
    twin = Dropout(rate, seed=seed)
    twin.calls = 1
    assert torch.equal(twin.forward(x_t, training=True), y2), "a strided x gives other values than its contiguous copy"
    # backward regenerates the mask of the last forward
    dy64 = rounded(r.uniform(0.5, 1.5, size=n), dtype)
    dx = layer.backward(dev(dy64, dtype))
    _drop_check(f"Dropout({rate}) backward after two forwards", dx, dy64, keep2, rate, dtype)


@pytest.mark.parametrize("rate,training", [(0.5, False), (0.0, True)])
def test_inactive_dropout_returns_its_arguments(ops, rate, training):
    from polus_amd.layers import Dropout
    layer = Dropout(rate, seed=5)
    x, dy = torch.ones(16, device="cuda"), torch.ones(16, device="cuda")
    if rate:
        layer.forward(x, training=True)              # an active call before: the inactive one must clear it
    assert layer.forward(x, training=training) is x
    assert layer.backward(dy) is dy
    print(f"[layers] Dropout({rate}) training={training}: identity path, x and dy handed back as they are")
