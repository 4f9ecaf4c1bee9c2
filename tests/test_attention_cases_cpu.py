"""The tolerances of test_attention_gpu.py can see the bugs they are there to catch (float64 oracle only, no GPU).

For every case of tests/attention_cases.py, each of these changes must move the oracle's ctx, and its dqkv (the
backward's one output: one of dq, dk, dv), by at least 5x the tolerance the GPU test applies to that output on that
case's kernel path:
  (a) the last kept key of a sample masked;
  (b) the padded key next to a sample's kept region kept;
  (c) the dropout index shifted by one element, and by one quad (idx + 4);
  (d) the dropout index taken key-major (((b A + h) S + key) S + q).
"Moves by k x the tolerance" means the perturbed output, checked against the unperturbed one by the GPU test's two
bounds (max-relative and per-element), fails the tighter of them by a factor k.  Attention treats the samples of a
batch independently, so (a) and (b) recompute only the sample they change.  (mask=None without dropout has nothing to
perturb.)

The paths those tolerances belong to come from attention_cases.fwd_path / bwd_path, a restatement of the library's
routing: test_attention_route_matches_cases holds the restatement to the library (polus_attention_route, host only)."""
import ctypes

import numpy as np
import pytest

from tests import attention_cases as ac
from tests.util import rounded

MARGIN = 5.0


def _round(case, a):
    import torch
    return rounded(a, torch.bfloat16 if case.dtype == "bf16" else torch.float32)


def _oracle(case, q_r, mask, d_r, keep):
    """The GPU test's reference, with the backward given the forward's ctx as the device would store it."""
    ctx, _, _ = ac.oracle(q_r, mask, d_r, case.A, keep)
    return ac.oracle(q_r, mask, d_r, case.A, keep, ctx_in=_round(case, ctx))


def _outputs(case, ctx, dqkv):
    return {"ctx": ctx, **ac.split(dqkv, case.A * 64)}


def _check(case, base, pert, what):
    v = {nm: ac.violation(pert[nm], ref, ac.TOL[case.fwd if nm == "ctx" else case.bwd][nm]) for nm, ref in base.items()}
    assert v["ctx"] >= MARGIN, f"{case.name}: {what} moves ctx by only {v['ctx']:.2f}x its tolerance"
    d = max(v["dq"], v["dk"], v["dv"])
    assert d >= MARGIN, f"{case.name}: {what} moves dqkv by only {d:.2f}x its tolerance (dq {v['dq']:.2f}, dk {v['dk']:.2f}, dv {v['dv']:.2f})"


@pytest.mark.parametrize("case", [c for c in ac.CASES if not (c.no_mask and c.p == 0)], ids=lambda c: c.name)
def test_tolerances_see_an_off_by_one(case):
    qkv, mask, dctx = ac.make_inputs(case)
    q_r, d_r = _round(case, qkv), _round(case, dctx)
    keep = ac.keep_scale(case) if case.p > 0 else None
    ctx, _, dqkv = _oracle(case, q_r, mask, d_r, keep)
    base = _outputs(case, ctx, dqkv)
    n_checked = 0
    if not case.no_mask:
        for b in range(case.B):
            last, first_pad = ac.edge_keys(mask[b])
            for what, key, val in (("(a) last kept key masked", last, 0), ("(b) first padded key kept", first_pad, 1)):
                if key is None:
                    continue
                m = mask[b:b + 1].copy()
                m[0, key] = val
                c1, _, d1 = _oracle(case, q_r[b:b + 1], m, d_r[b:b + 1], None if keep is None else keep[b:b + 1])
                ctx2, dqkv2 = ctx.copy(), dqkv.copy()
                ctx2[b], dqkv2[b] = c1[0], d1[0]
                _check(case, base, _outputs(case, ctx2, dqkv2), f"{what} (sample {b}, {case.masks[b]}, key {key})")
                n_checked += 1
    if case.p > 0:
        for what, k in (("(c) dropout index + 1", ac.keep_scale(case, idx0=1)),
                        ("(c) dropout index + 4", ac.keep_scale(case, idx0=4)),
                        ("(d) dropout index key-major", ac.keep_scale(case, key_major=True))):
            c1, _, d1 = _oracle(case, q_r, mask, d_r, k)
            _check(case, base, _outputs(case, c1, d1), what)
            n_checked += 1
    assert n_checked > 0


def test_every_path_has_a_dropout_case_and_a_short_mask_case():
    short = {"len:1", "len:2"}
    for p in ac.PATHS:
        mine = [c for c in ac.CASES if p in (c.fwd, c.bwd)]
        assert {0.1, 0.5} <= {c.p for c in mine}, p
        assert any(short & set(c.masks) for c in mine), p
        if p not in ("F4", "B7"):
            assert any(c.no_mask for c in mine), p
    assert {768, 1024, 2048, 1088} <= {c.S for c in ac.CASES}
    assert all(c.B * c.A * c.S * c.S <= 16 << 20 for c in ac.CASES)


def test_path_selection_matches_the_host_code():
    assert [ac.fwd_path("bf16", S) for S in (17, 95, 96, 1024, 1025)] == ["F1", "F1", "F2", "F2", "F3"]
    assert ac.bwd_path("bf16", 256) == "B3" and ac.bwd_path("bf16", 256, kres=2) == "B4"
    assert ac.bwd_path("bf16", 256, kres=0) == "B3" and ac.bwd_path("bf16", 512) == "B5"
    assert ac.bwd_path("bf16", 2304) == "B6" and ac.bwd_path("bf16", 768, fused=0) == "B6"
    assert ac.bwd_path("bf16", 64) == "B1" and ac.bwd_path("bf16", 128) == "B2" and ac.bwd_path("bf16", 200) == "B6"


def test_every_path_is_reached_by_a_case():
    assert set(ac.PATHS) == {c.fwd for c in ac.CASES} | {c.bwd for c in ac.CASES}


ROUTE_ENVS = ((), (("POLUS_ATTN_FUSED", 0),), (("POLUS_ATTN_BWD_KRES", 0),), (("POLUS_ATTN_BWD_KRES", 2),),
              (("POLUS_ATTN_FUSED", 0), ("POLUS_ATTN_BWD_KRES", 2)))


@pytest.mark.parametrize("env", ROUTE_ENVS, ids=lambda e: "-".join(f"{k.split('_')[-1].lower()}{v}" for k, v in e) or "default")
def test_attention_route_matches_cases(env):
    """polus_attention_route (the library's own routing, no device touched) against fwd_path / bwd_path for both dtypes and
    every S in 1..2304 (past the key-resident range and the forward's LDS-DMA range), under each switch setting."""
    from polus_amd import _lib, build, ops
    build.build(verbose=False)
    lib = _lib.load()
    e = dict(env)
    fused, kres = e.get("POLUS_ATTN_FUSED", 1), e.get("POLUS_ATTN_BWD_KRES", 1)
    fwd, bwd = ctypes.c_int(), ctypes.c_int()
    try:
        for k, v in env:
            ops.set_env(k, v)
        for dtype, code in (("bf16", _lib.BF16), ("f32", _lib.F32)):
            for S in range(1, 2305):
                assert lib.polus_attention_route(code, S, ctypes.byref(fwd), ctypes.byref(bwd)) == 0
                want = (int(ac.fwd_path(dtype, S)[1:]), int(ac.bwd_path(dtype, S, fused, kres)[1:]))
                assert (fwd.value, bwd.value) == want, (dtype, S, env)
    finally:
        for k, _ in env:
            ops.set_env(k)
    assert lib.polus_attention_route(2, 128, ctypes.byref(fwd), ctypes.byref(bwd)) != 0 and b"bad dtype" in lib.polus_last_error()
    assert lib.polus_attention_route(_lib.BF16, 0, ctypes.byref(fwd), ctypes.byref(bwd)) != 0


def test_edge_keys():
    r = np.random.Generator(np.random.PCG64(0))
    assert ac.edge_keys(ac.mask_row("len:5", 20, r)) == (4, 5)
    assert ac.edge_keys(ac.mask_row("left:7", 20, r)) == (19, 6)
    assert ac.edge_keys(ac.mask_row("zero", 20, r)) == (None, 0)
    assert ac.edge_keys(ac.mask_row("full", 20, r)) == (19, None)
    m = ac.mask_row("holes", 64, r)
    last, pad = ac.edge_keys(m)
    assert last == 63 and m[pad] == 0 and m[:pad].all() and 0 < pad < 63
