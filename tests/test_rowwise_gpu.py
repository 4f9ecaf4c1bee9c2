"""The row-wise kernels (norm.hip, embed.hip, optim.hip, runtime.hip, loss.hip) against the float64 oracle, on every kernel path.

The cases, the map from case to kernel path, the references and the tolerances live in tests/rowwise_cases.py; a case's
id starts with its path (W32 / WB / HW LayerNorm families, A1-A4 / AW / OWN word-table scatters).  Every output is
NaN-filled before the call; the dropout keep-scale comes from the numpy restatement of the hash, never from the engine's
own mask kernel.  Each check prints its error before it asserts (pytest -s shows them).
test_rowwise_cases_cpu.py checks that these tolerances see one mask index off, a dropped tail row, an ignored scale."""
import os
import struct
from contextlib import contextmanager

import numpy as np
import pytest
import torch

from oracle import losses as ol
from tests import rowwise_cases as rc
from tests.util import TOL, dev, dropout_keep_np, host, relerr, rounded

pytestmark = pytest.mark.gpu

F32 = torch.float32


@pytest.fixture(scope="module")
def ops():
    from polus_amd import ops as _ops
    _ops.set_dynamic_params(None)            # the dropout seed as passed (no per-step salt)
    return _ops


@contextmanager
def _env(ops, pairs):
    """POLUS_* switches set for the block, each put back to what it was."""
    old = {k: os.environ.get(k) for k, _ in pairs}
    try:
        for k, v in pairs:
            ops.set_env(k, v)
        yield
    finally:
        for k, v in old.items():
            ops.set_env(k, v)


@contextmanager
def _dyn(ops, salt=0, lr=0.0, lr_t=0.0):
    """A registered dynamic block {salt, lr, lr_t, 0}; unregistered afterwards."""
    words = struct.unpack("4i", struct.pack("Iffi", salt & 0xFFFFFFFF, lr, lr_t, 0))
    block = torch.tensor(words, dtype=torch.int32, device="cuda")
    try:
        ops.set_dynamic_params(block)
        yield block
    finally:
        ops.set_dynamic_params(None)
        torch.cuda.synchronize()


def _nan(shape, dtype=F32):
    return torch.full(shape if isinstance(shape, tuple) else (shape,), float("nan"), dtype=dtype, device="cuda")


def _close(got, ref, tol, what):
    g = host(got) if torch.is_tensor(got) else np.asarray(got, np.float64)
    e = relerr(g.reshape(np.shape(ref)), ref)
    print(f"[rowwise] {what}: rel err {e:.3e} (tol {tol:.1e})")
    assert np.isfinite(g).all(), f"{what}: not fully written (or not finite)"
    assert e <= tol, f"{what}: rel err {e:.3e} > {tol:.1e}"


# ------------------------------------------------------------------------------------------------- LayerNorm
def _ln_device(case):
    dt = rc.DT[case.dtype]
    x, g, b, dy, prior = rc.ln_inputs(case)
    t = {"x": dev(x, dt), "g": dev(g, F32), "b": dev(b, F32), "dy": None if dy is None else dev(dy, dt)}
    r = {"x": rounded(x, dt), "g": rounded(g, F32), "b": rounded(b, F32), "dy": None if dy is None else rounded(dy, dt),
         "prior": rounded(prior, F32)}
    return t, r


def _ln_fwd(ops, case, t, r):
    rows, H = case.rows, case.H
    y, mean, rstd = _nan((rows, H), rc.DT[case.dtype]), _nan(rows), _nan(rows)
    ops.layernorm_fwd(t["x"], t["g"], t["b"], y, mean, rstd, rc.EPS)
    y_ref, mean_ref, rstd_ref = rc.ln_fwd_reference(r["x"], r["g"], r["b"])
    tol = rc.ln_tol(case.dtype)
    _close(y, y_ref, tol["y"], f"{case.name} y")
    _close(mean, mean_ref, tol["mean"], f"{case.name} mean")
    _close(rstd, rstd_ref, tol["rstd"], f"{case.name} rstd")
    return mean, rstd, mean_ref, rstd_ref


def _ln_bwd(ops, case, t, mean, rstd, want_bias, p=0.0, prior=None, partials=None):
    """One layernorm_bwd call into NaN-filled (or `prior`-filled, accumulate) outputs."""
    rows, H = case.rows, case.H
    dt = rc.DT[case.dtype]
    out = {"dx": _nan((rows, H), dt), "dxm": _nan((rows, H), dt) if p > 0 else None}
    for k, nm in enumerate(("dgamma", "dbeta", "dbias")):
        out[nm] = _nan(H) if prior is None else dev(prior[k], F32)
    if not want_bias:
        out["dbias"] = None
    ops.layernorm_bwd(t["dy"], t["x"], t["g"], mean, rstd, out["dx"], out["dgamma"], out["dbeta"], out["dbias"],
                      accumulate=prior is not None, dx_masked=out["dxm"], drop_p=p, seed=case.seed, partials=partials)
    return out


def _ln_check(case, out, ref, prior, what):
    tol = rc.ln_tol(case.dtype)
    for k, nm in enumerate(("dgamma", "dbeta", "dbias")):
        if out[nm] is not None:
            _close(out[nm], ref[nm] + (0 if prior is None else prior[k]), tol[nm], f"{case.name} {what} {nm}")
    _close(out["dx"], ref["dx"], tol["dx"], f"{case.name} {what} dx")
    if out["dxm"] is not None:
        _close(out["dxm"], ref["dxm"], tol["dxm"], f"{case.name} {what} dx_masked")


@pytest.mark.parametrize("case", rc.LN_CASES, ids=lambda c: c.name)
def test_layernorm_path_matches_oracle(ops, case):
    t, r = _ln_device(case)
    with _env(ops, case.env):
        mean, rstd, mean_ref, rstd_ref = _ln_fwd(ops, case, t, r)
        if case.fwd_only:
            return
        plain = rc.ln_bwd_reference(r["x"], r["dy"], r["g"], mean_ref, rstd_ref)
        _ln_check(case, _ln_bwd(ops, case, t, mean, rstd, False), plain, None, "plain")
        _ln_check(case, _ln_bwd(ops, case, t, mean, rstd, True), plain, None, "dbias")
        for p in rc.LN_DROP_P:
            ref = rc.ln_bwd_reference(r["x"], r["dy"], r["g"], mean_ref, rstd_ref, rc.keep_scale(case.seed, p, case.rows, case.H))
            _ln_check(case, _ln_bwd(ops, case, t, mean, rstd, True, p), ref, None, f"dropout {p}")
            if p == rc.LN_DROP_P[0]:
                _ln_check(case, _ln_bwd(ops, case, t, mean, rstd, True, p, r["prior"]), ref, r["prior"], "accumulate")
    torch.cuda.synchronize()


@pytest.mark.parametrize("fin_single", [None, rc.LN_FIN_SINGLE], ids=["one-stage", "two-stage"])
@pytest.mark.parametrize("case", rc.LN_FINALIZE_CASES, ids=lambda c: c.name)
def test_layernorm_deferred_finalize_equals_direct(ops, case, fin_single):
    """layernorm_bwd(partials=) + layernorm_bwd_finalize is the direct call, bit for bit, in one finalize launch and
    (POLUS_LN_FIN_SINGLE below the 250 workgroups) in two stages; both match the oracle."""
    t, r = _ln_device(case)
    rows, H = case.rows, case.H
    env = case.env + ((("POLUS_LN_FIN_SINGLE", fin_single),) if fin_single else ())
    with _env(ops, env):
        mean, rstd, mean_ref, rstd_ref = _ln_fwd(ops, case, t, r)
        for what, want_bias, p, prior in (("no dbias", False, 0.0, None), ("accumulate", True, 0.0, r["prior"]),
                                          ("dropout", True, 0.1, None)):
            keep = rc.keep_scale(case.seed, p, rows, H) if p > 0 else None
            ref = rc.ln_bwd_reference(r["x"], r["dy"], r["g"], mean_ref, rstd_ref, keep)
            direct = _ln_bwd(ops, case, t, mean, rstd, want_bias, p, prior)
            _ln_check(case, direct, ref, prior, f"direct, {what}")
            partials = _nan(ops.layernorm_bwd_partial_floats(rows, H))
            deferred = _ln_bwd(ops, case, t, mean, rstd, want_bias, p, prior, partials=partials)
            ops.layernorm_bwd_finalize(partials, rows, H, deferred["dgamma"], deferred["dbeta"], deferred["dbias"],
                                       accumulate=prior is not None)
            _ln_check(case, deferred, ref, prior, f"deferred, {what}")
            for nm in ("dx", "dxm", "dgamma", "dbeta", "dbias"):
                if direct[nm] is not None:
                    assert torch.equal(direct[nm], deferred[nm]), f"{case.name} {what}: {nm} differs between direct and deferred"
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------- embeddings
def _emb_bwd(ops, case, args, tables, accumulate=False, out=None):
    if out is None:
        out = {k: _nan(tuple(v.shape)) for k, v in tables.items()}
    ops.embed_ln_bwd(*args, out["emb.word"], out["emb.pos"], out["emb.type"], out["emb.ln.g"], out["emb.ln.b"],
                     accumulate=accumulate, deterministic=case.deterministic, drop_p=case.p, seed=case.seed)
    return out


@pytest.mark.parametrize("case", rc.EMB_CASES, ids=lambda c: c.name)
def test_embeddings_path_matches_oracle(ops, case):
    B, S, H, rows = rc.EMB_B, rc.EMB_S, case.H, case.rows
    dt = rc.DT[case.dtype]
    p = rc.emb_tables(H, case.seed)
    tables = {k: dev(v, F32) for k, v in p.items()}
    dy = rc.emb_dy(case)
    dy_t, dy_r = dev(dy.reshape(rows, H), dt), rounded(dy, dt)
    keep = rc.keep_scale(case.seed, case.p, rows, H).reshape(B, S, H) if case.p > 0 else None
    tol = rc.emb_tol(case.dtype)
    grads = ("emb.word", "emb.pos", "emb.type", "emb.ln.g", "emb.ln.b")
    for idk in rc.EMB_ID_PATTERNS:
        for ttk in rc.EMB_TYPE_PATTERNS:
            what = f"{case.name} ids={idk} types={ttk}"
            ids, tt = rc.emb_ids(idk, case.seed), rc.emb_types(ttk, case.seed)
            ref = rc.emb_reference(p, H, rc.emb_clamp(ids), tt, dy_r, keep)
            ids_t, tt_t = dev(ids), None if tt is None else dev(tt)
            y, mean, rstd = _nan((rows, H), dt), _nan(rows), _nan(rows)
            ops.embed_ln_fwd(ids_t, tt_t, tables["emb.word"], tables["emb.pos"], tables["emb.type"], tables["emb.ln.g"],
                             tables["emb.ln.b"], y, mean, rstd, rc.EPS, drop_p=case.p, seed=case.seed)
            _close(y, ref["y"].reshape(rows, H), tol["y"], f"{what} y")
            _close(mean, ref["mean"].reshape(rows), tol["mean"], f"{what} mean")
            _close(rstd, ref["rstd"].reshape(rows), tol["rstd"], f"{what} rstd")
            args = (dy_t, ids_t, tt_t, tables["emb.word"], tables["emb.pos"], tables["emb.type"], tables["emb.ln.g"], mean, rstd)
            out = _emb_bwd(ops, case, args, tables)
            for nm in grads:
                _close(out[nm], ref[nm], tol[nm], f"{what} {nm}")
            assert not out["emb.pos"][S:].any(), f"{what}: gpos rows at or beyond S are not zero"
            if ttk != "mixed":
                assert not out["emb.type"][1].any(), f"{what}: gtype[1] is not zero"
            if case.deterministic:
                again = _emb_bwd(ops, case, args, tables)
                for nm in grads:
                    assert torch.equal(out[nm], again[nm]), f"{what}: {nm} differs between two deterministic calls"
            out["emb.pos"][S:] = 7.0
            _emb_bwd(ops, case, args, tables, accumulate=True, out=out)
            assert (out["emb.pos"][S:] == 7.0).all(), f"{what}: accumulate touched gpos rows at or beyond S"
            out["emb.pos"][S:] = 0.0
            for nm in grads:
                _close(out[nm], 2 * ref[nm], tol[nm], f"{what} {nm} accumulate")
    torch.cuda.synchronize()


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_embeddings_forward_above_the_grid_cap(ops, dtype):
    B, S, H = rc.EMB_FWD_LARGE
    assert B * S > rc.LN_FWD_CAP_ROWS
    dt = rc.DT[dtype]
    p = rc.emb_tables(H, 77, max_pos=S)
    tables = {k: dev(v, F32) for k, v in p.items()}
    ids, tt = rc.emb_ids("random", 77, B, S), rc.emb_types("mixed", 77, B, S)
    y, mean, rstd = _nan((B * S, H), dt), _nan(B * S), _nan(B * S)
    ops.embed_ln_fwd(dev(ids), dev(tt), tables["emb.word"], tables["emb.pos"], tables["emb.type"], tables["emb.ln.g"],
                     tables["emb.ln.b"], y, mean, rstd, rc.EPS)
    tol = rc.emb_tol(dtype)
    got = {"y": host(y), "mean": host(mean), "rstd": host(rstd)}
    assert all(np.isfinite(v).all() for v in got.values()), "not fully written"
    err = {k: 0.0 for k in got}
    for b0 in range(0, B, 26):                     # the reference in row chunks
        ref = rc.emb_reference(p, H, ids[b0:b0 + 26], tt[b0:b0 + 26], None)
        sl = slice(b0 * S, (b0 + 26) * S)
        for k in got:
            err[k] = max(err[k], relerr(got[k][sl].reshape(ref[k].shape), ref[k]))
    print(f"[rowwise] embed fwd {dtype} {B}x{S}x{H}: {err}")
    for k in got:
        assert err[k] <= tol[k], (k, err[k], tol[k])


# ------------------------------------------------------------------------------------------------- optimizer
def _adam_check(what, p, m, v, shadow, ref, st, inside, shadow_mask):
    for nm, got in (("p", p), ("m", m), ("v", v)):
        _close(got, ref[nm], rc.ADAM_TOL, f"adam {what} {nm}")
        assert np.array_equal(host(got)[~inside], st[nm][~inside]), f"adam {what}: {nm} touched outside the segments"
    want = torch.where(dev(shadow_mask), p.to(torch.bfloat16), torch.zeros_like(shadow))
    assert torch.equal(shadow, want), f"adam {what}: the bf16 shadow is not bf16(p) on the flagged segments and 0 elsewhere"


def test_adam_segments_scales_and_dynamic_block(ops):
    seg, n = rc.adam_table()
    st = rc.adam_state(n)
    inside, shadow_mask = rc.seg_masks(seg, n)
    refs = rc.adam_reference(seg, st, [rc.ADAM_GRAD_SCALE * rc.ADAM_CLIP, 1.0])
    p, m, v = dev(st["p"], F32), dev(st["m"], F32), dev(st["v"], F32)
    shadow = torch.zeros(n, dtype=torch.bfloat16, device="cuda")
    seg_t = dev(seg)
    hyper = (rc.ADAM_B1, rc.ADAM_B2, rc.ADAM_EPS, rc.ADAM_WD)
    # (a) grad_scale and a clip scale read from device memory
    ops.adam_step(p, dev(st["g"][0], F32), m, v, shadow, seg_t, len(seg), rc.ADAM_LR, rc.adam_lr_t(1), *hyper,
                  grad_scale=rc.ADAM_GRAD_SCALE, clip_scale=torch.tensor([rc.ADAM_CLIP], dtype=F32, device="cuda"))
    _adam_check("(a) scales", p, m, v, shadow, refs[0], st, inside, shadow_mask)
    # (b) lr and lr_t from the dynamic block; the scalar arguments must not be read
    with _dyn(ops, salt=5, lr=rc.ADAM_LR, lr_t=rc.adam_lr_t(2)):
        ops.adam_step(p, dev(st["g"][1], F32), m, v, shadow, seg_t, len(seg), float("nan"), float("nan"), *hyper)
        torch.cuda.synchronize()
    _adam_check("(b) dynamic block", p, m, v, shadow, refs[1], st, inside, shadow_mask)


@pytest.mark.parametrize("n_seg", [rc.ADAM_SEGMENTS, 1100])
def test_sqnorm_segments(ops, n_seg):
    seg, n = rc.adam_table(n_seg)
    inside, _ = rc.seg_masks(seg, n)
    g = rc.adam_state(n, seed=n_seg)["g"][1]
    g[~inside] = 1000.0                          # the gaps between segments are not part of the sum
    out = _nan(1)
    ops.sqnorm_segments(dev(g, F32), dev(seg), n_seg, out)
    _close(out, np.array([(g[inside] ** 2).sum()]), rc.SQNORM_TOL, f"sqnorm_segments {n_seg}")


def test_sqnorm_above_the_grid_cap(ops):
    n = rc.SQNORM_N
    g = np.random.Generator(np.random.PCG64(3)).standard_normal(n).astype(np.float32).astype(np.float64)
    g[-3:] = 100.0                               # the ragged tail and the first quad of the second sweep carry weight
    g[2 ** 20:2 ** 20 + 4] = 100.0
    out = _nan(1)
    ops.sqnorm(dev(g, F32), out)
    _close(out, np.array([(g ** 2).sum()]), rc.SQNORM_TOL, "sqnorm")


@pytest.mark.parametrize("n", rc.CAST_SIZES)
def test_cast_and_scale(ops, n):
    x = torch.as_tensor(np.random.Generator(np.random.PCG64(n)).standard_normal(n) * 3).to(F32).cuda()
    for src_dt in (F32, torch.bfloat16):
        for dst_dt in (F32, torch.bfloat16):
            src = x.to(src_dt)
            dst = _nan(n, dst_dt)
            ops.cast(src, dst)
            assert torch.equal(dst, src.to(dst_dt)), f"cast {src_dt} -> {dst_dt} at n={n}"
    want = x * 0.3                               # one f32 multiply either way: exact
    ops.scale_(x, 0.3)
    assert torch.equal(x, want), f"scale_ at n={n}"


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("act", rc.ACTS)
def test_act_bwd(ops, act, dtype):
    dt = rc.DT[dtype]
    for n in rc.ACT_SIZES:
        dy, u = rc.act_inputs(n)
        du = _nan(n, dt)
        ops.act_bwd(dev(dy, dt), dev(u, dt), du, act)
        _close(du, rounded(dy, dt) * rc.act_grad(act, rounded(u, dt)), TOL[dt], f"act_bwd {act} {dtype} n={n}")


@pytest.mark.parametrize("R,C", rc.TRANSPOSE_SHAPES)
def test_transpose_bf16(ops, R, C):
    src = torch.as_tensor(np.random.Generator(np.random.PCG64(R * C)).standard_normal((R, C))).to(torch.bfloat16).cuda()
    dst = _nan((C, R), torch.bfloat16)
    ops.transpose_bf16(src, dst)
    assert torch.equal(dst, src.t().contiguous())


def test_dropout_mask_with_a_registered_salt(ops):
    seed, salt, p, n = 0x1234567, 0x9ABCDEF1, 0.1, 4099
    with _dyn(ops, salt=salt):
        got = ops.dropout_mask(seed, p, n, idx0=5).cpu().numpy()
    assert np.array_equal(got, dropout_keep_np(rc.eff_seed_np(seed, salt), p, 5, n))
    assert not np.array_equal(got, dropout_keep_np(seed, p, 5, n))
    assert np.array_equal(ops.dropout_mask(seed, p, n, idx0=5).cpu().numpy(), dropout_keep_np(seed, p, 5, n))


# ------------------------------------------------------------------------------------------------- losses
def _wide(a, fill, dtype=F32):
    """`a` [rows, C] as the column slice [:, 3:3+C] of a wider device buffer filled with `fill`."""
    rows, C = a.shape
    buf = torch.full((rows, C + rc.LOSS_PAD), fill, dtype=dtype, device="cuda")
    view = buf[:, rc.LOSS_PAD_LEFT:rc.LOSS_PAD_LEFT + C]
    view.copy_(torch.as_tensor(a).to(dtype))
    return buf, view


def _outside_untouched(buf, C, fill):
    return bool((buf[:, :rc.LOSS_PAD_LEFT] == fill).all() and (buf[:, rc.LOSS_PAD_LEFT + C:] == fill).all())


def _loss_close(loss, ref, what):
    got = float(loss)
    print(f"[rowwise] {what}: loss {got:.7g} (oracle {float(ref):.7g})")
    assert np.isfinite(got) and abs(got - ref) < 1e-5 * max(1, abs(ref)), (what, got, ref)


@pytest.mark.parametrize("rows,C,big", rc.LOSS_CASES)
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_losses_on_column_slices(ops, dtype, rows, C, big):
    dt = rc.DT[dtype]
    dtol = rc.loss_dlogits_tol(dtype)
    logits, labels, y, cw = rc.loss_inputs(rows, C, big)
    _, x_v = _wide(logits, 1e4)                  # a kernel that ignored the row stride would read these
    lab_t, cw_t = dev(labels), dev(cw, F32)
    what = f"rows={rows} C={C} big={big} {dtype}"
    for weights in (None, cw):
        if weights is None:
            loss_ref, d_ref = ol.sparse_softmax_xent_fwd(logits, labels)
        else:
            loss_ref, d_ref = ol.weighted_softmax_xent_fwd(cw, np.eye(C)[labels], logits)
        d_buf, d_v = _wide(np.full((rows, C), np.nan), 123.0, dt)
        loss = _nan(1)
        ops.softmax_xent(x_v, lab_t, loss, d_v, class_weights=None if weights is None else cw_t)
        _loss_close(loss, loss_ref, f"softmax_xent {what} weighted={weights is not None}")
        _close(d_v, d_ref, dtol, f"softmax_xent {what} dlogits")
        assert _outside_untouched(d_buf, C, 123.0), f"softmax_xent {what}: wrote outside the slice"
    loss_ref, d_ref = ol.weighted_sigmoid_xent_fwd(cw, 0.3, y, logits)
    _, y_v = _wide(y, 1.0)
    d_buf, d_v = _wide(np.full((rows, C), np.nan), 123.0, dt)
    loss = _nan(1)
    ops.sigmoid_xent(x_v, y_v, cw_t, 0.3, loss, d_v)
    _loss_close(loss, loss_ref, f"sigmoid_xent {what}")
    _close(d_v, d_ref, dtol, f"sigmoid_xent {what} dlogits")
    assert _outside_untouched(d_buf, C, 123.0), f"sigmoid_xent {what}: wrote outside the slice"
    if dtype == "f32":
        out = torch.full((rows,), -1, dtype=torch.int32, device="cuda")
        ops.argmax(x_v, out)
        assert np.array_equal(out.cpu().numpy(), logits.argmax(-1)), f"argmax {what}"     # ties (the all-equal row): the first
