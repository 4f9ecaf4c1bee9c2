"""The tolerances of test_rowwise_gpu.py can see the bugs they are there to catch (float64 oracle only, no GPU).

Each perturbation below is applied to the reference alone, for every case of tests/rowwise_cases.py it applies to, and
must move at least one output by 5x the tolerance the GPU test applies to that output on that case:
  LayerNorm dropout      the mask index shifted by 1 and by 4; the mask taken with row stride H + 4; dbias summed from
                         the unmasked dx; dx and dx_masked exchanged
  LayerNorm column sums  the last row left out; the rows of the last (partial) group of four left out
  embeddings             position taken as row // S; type ignored; the last rows % 8 tokens left out of gword; a
                         duplicate id inside a run of 8 counted once; an out-of-range id dropped instead of clamped; the
                         dropout index shifted by 1
  Adam                   grad_scale or clip_scale ignored; a segment's last len % 4 elements left unchanged; decay
                         applied to a no-decay segment
and the case table reaches every kernel path with a dropout case, an accumulate case and a ragged tail.

The case table restates two things of the launchers that decide what a case covers: the route (ln_path, scatter_path) and
the grid caps (LN_*_CAP_ROWS).  test_rowwise_route_matches_cases and test_restated_caps_are_the_launchers_caps hold both
to the library's own report, polus_rowwise_route (host only: the same functions the launchers call)."""
import ctypes
from contextlib import contextmanager

import numpy as np
import pytest
import torch

from oracle import bert as ob
from oracle import losses as ol
from tests import rowwise_cases as rc
from tests.util import dropout_keep_np, relerr, rounded

MARGIN = 5.0


def _moves(pert, base, tol, what):
    v = rc.violation(pert, base, tol)
    assert v >= MARGIN, f"{what} moves the reference by only {v:.2f}x the tolerance"


# ------------------------------------------------------------------------------------------------- LayerNorm
LN_BWD_CASES = [c for c in rc.LN_CASES + rc.LN_FINALIZE_CASES if not c.fwd_only]


@pytest.mark.parametrize("case", LN_BWD_CASES, ids=lambda c: c.name)
def test_layernorm_tolerances_see_the_perturbations(case):
    dt = rc.DT[case.dtype]
    rows, H = case.rows, case.H
    x, g, b, dy, _ = rc.ln_inputs(case)
    x_r, dy_r, g_r, b_r = rounded(x, dt), rounded(dy, dt), rounded(g, torch.float32), rounded(b, torch.float32)
    _, mean, rstd = rc.ln_fwd_reference(x_r, g_r, b_r)
    tol = {k: v for k, v in rc.ln_tol(case.dtype).items() if k in ("dx", "dxm", "dgamma", "dbeta", "dbias")}
    ref = lambda keep=None, sl=slice(None): rc.ln_bwd_reference(x_r[sl], dy_r[sl], g_r, mean[sl], rstd[sl], keep)
    for p in rc.LN_DROP_P:
        base = ref(rc.keep_scale(case.seed, p, rows, H))
        for what, kw in (("mask index + 1", {"shift": 1}), ("mask index + 4", {"shift": 4}), ("mask row stride H + 4", {"row_stride": H + 4})):
            if "row_stride" in kw and rows == 1:
                continue                                  # one row: its base index is 0 under any stride
            _moves(ref(rc.keep_scale(case.seed, p, rows, H, **kw)), base, tol, f"{case.name} p={p}: {what}")
        _moves({**base, "dbias": base["dx"].sum(0)}, base, tol, f"{case.name} p={p}: dbias from the unmasked dx")
        _moves({**base, "dx": base["dxm"], "dxm": base["dx"]}, base, tol, f"{case.name} p={p}: dx and dx_masked exchanged")
    base = ref()
    sums = lambda n: {**base, **{k: v for k, v in ref(sl=slice(0, n)).items() if k in ("dgamma", "dbeta", "dbias")}} if n else \
        {**base, "dgamma": 0 * base["dgamma"], "dbeta": 0 * base["dbeta"], "dbias": 0 * base["dbias"]}
    _moves(sums(rows - 1), base, tol, f"{case.name}: the last row left out of the column sums")
    if rows % 4:
        _moves(sums(rows - rows % 4), base, tol, f"{case.name}: the last block's rows left out of the column sums")


def test_every_path_has_a_dropout_an_accumulate_and_a_ragged_case():
    # every backward LayerNorm case runs the plain, dbias, dropout (both p) and accumulate forms; every embedding case
    # runs accumulate and has 129 rows (no multiple of the scatter's runs of 8 or of a 16-wave workgroup)
    for path in rc.LN_PATHS:
        mine = [c for c in rc.LN_CASES if c.path == path]
        assert any(not c.fwd_only for c in mine), path
        assert any(c.ragged and not c.fwd_only for c in mine), path
        assert any(c.fwd_only for c in mine), path
        assert any(not c.fwd_only and c.rows > (rc.LN_BWD_HW_CAP_ROWS if path == "HW" else rc.LN_BWD_CAP_ROWS) for c in mine), path
        assert any(c.path == path for c in rc.LN_FINALIZE_CASES), path
    for c in rc.LN_CASES:
        if c.fwd_only:
            assert c.rows > (rc.LN_FWD_HW_CAP_ROWS if c.path == "HW" else rc.LN_FWD_CAP_ROWS), c.name
    for path in rc.SCATTER_PATHS:
        mine = [c for c in rc.EMB_CASES if c.path == path]
        assert all(c.rows % 8 and c.rows % 16 for c in mine), path
        assert {0.0, 0.1} <= {c.p for c in mine}, path
        assert {"f32", "bf16"} <= {c.dtype for c in mine}, path
    # the LayerNorm chunk counts: a ragged two-chunk row (H = 260), NC = 8 with ragged H (1280), every exact NC
    assert {64, 260, 768, 1024, 1280, 2048} <= {c.H for c in rc.LN_CASES if c.path == "W32"}
    assert {64, 260, 768, 1024, 1280, 2048} <= {c.H for c in rc.LN_CASES if c.path == "WB"}
    assert {256, 512, 768, 1024} <= {c.H for c in rc.LN_CASES if c.path == "HW"}
    assert rc.LNCase("bf16", 39, 768).path == "WB"
    blocks = (rc.LN_FINALIZE_CASES[0].rows + 3) // 4
    assert blocks == 250 and blocks > rc.LN_FIN_SINGLE and 0 < blocks % 128 < 128


def test_path_selection_matches_the_host_code():
    assert rc.ln_path("f32", 38, 768) == "W32" and rc.ln_path("f32", 2, 256) == "W32"
    assert rc.ln_path("bf16", 38, 768) == "HW" and rc.ln_path("bf16", 39, 768) == "WB"
    assert rc.ln_path("bf16", 38, 768, halfwave=0) == "WB"
    assert rc.ln_path("bf16", 38, 1280) == "WB" and rc.ln_path("bf16", 38, 260) == "WB" and rc.ln_path("bf16", 38, 64) == "WB"
    assert rc.ln_path("bf16", 2, 1024) == "HW" and rc.ln_path("bf16", 2, 2048) == "WB"
    assert [rc.scatter_path(H, False) for H in (128, 256, 260, 512, 768, 772, 1024, 1028, 2048)] == \
        ["A1", "A1", "A2", "A2", "A3", "A4", "A4", "AW", "AW"]
    assert rc.scatter_path(128, True) == "OWN" and rc.scatter_path(1280, True) == "OWN"


@pytest.fixture(scope="module")
def lib():
    from polus_amd import _lib, build
    build.build(verbose=False)
    return _lib.load()


@contextmanager
def _switches(env):
    from polus_amd import ops
    try:
        for k, v in env:
            ops.set_env(k, v)
        yield
    finally:
        for k, _ in env:
            ops.set_env(k)


def _route(lib, dtype, rows, H, deterministic=0):
    """polus_rowwise_route: [0] LayerNorm path, [1] / [2] forward / backward workgroups, [3] finalize stages, [4] scatter path,
    [5] / [6] workgroups of the embedding forward / backward."""
    out = (ctypes.c_int * 7)()
    rc = lib.polus_rowwise_route({"f32": 0, "bf16": 1}[dtype], rows, H, deterministic, out)
    assert rc == 0, (dtype, rows, H, lib.polus_last_error())
    return list(out)


ROUTE_ENVS = ((), (("POLUS_LN_HALFWAVE", 0),), (("POLUS_LN_BWD_BLOCKS", 64),))


@pytest.mark.parametrize("env", ROUTE_ENVS, ids=lambda e: "-".join(f"{k.split('_', 1)[1].lower()}{v}" for k, v in e) or "default")
def test_rowwise_route_matches_cases(lib, env):
    """The library's own routing (no device touched) against ln_path / scatter_path: both dtypes, rows 1..40 and the three
    large row counts of the case table, every H the entry points take, both scatter forms, under each switch setting."""
    e = dict(env)
    halfwave, bwd_cap = e.get("POLUS_LN_HALFWAVE", 1), e.get("POLUS_LN_BWD_BLOCKS", 512)
    out = (ctypes.c_int * 7)()
    with _switches(env):
        for code, dtype in enumerate(("f32", "bf16")):
            for rows in list(range(1, 41)) + [4106, 65538, 131080]:
                for H in range(4, 2049, 4):
                    want_ln = 1 + rc.LN_PATHS.index(rc.ln_path(dtype, rows, H, halfwave))
                    for det in (0, 1):
                        assert lib.polus_rowwise_route(code, rows, H, det, out) == 0
                        want = (want_ln, 1 + rc.SCATTER_PATHS.index(rc.scatter_path(H, det)))
                        assert (out[0], out[4]) == want, (dtype, rows, H, det, env)
                        assert out[2] == min((rows + 3) // 4, bwd_cap), (dtype, rows, H, env)      # the switch reaches the report
    assert lib.polus_rowwise_route(2, 8, 256, 0, out) != 0 and b"bad dtype" in lib.polus_last_error()
    for H in (0, 258, 2052):
        assert lib.polus_rowwise_route(1, 8, H, 0, out) != 0 and b"bad arguments" in lib.polus_last_error(), H
    assert lib.polus_rowwise_route(1, 0, 256, 0, out) != 0


def test_restated_caps_are_the_launchers_caps(lib):
    """The "above the cap" cases take a second trip round a grid-stride loop only while LN_*_CAP_ROWS are the launchers' caps.
    Per cap: (dtype, index of the workgroup count in the report, rows a workgroup covers per trip, rows per workgroup the
    launcher sizes its grid by).  The two differ for the half-wave backward alone: it runs on the wave-per-row grid,
    ceil(rows / 4) workgroups, while its workgroups cover 8 rows each, so its grid is full from 2048 rows on and the
    "one workgroup fewer" check is made there; where the cap lies is fixed by the other two checks."""
    H = 256
    caps = {"LN_FWD_CAP_ROWS": ("f32", 1, 16, 16), "LN_FWD_HW_CAP_ROWS": ("bf16", 1, 8, 8),
            "LN_BWD_CAP_ROWS": ("f32", 2, 4, 4), "LN_BWD_HW_CAP_ROWS": ("bf16", 2, 8, 4)}
    for name, (dtype, k, covers, sized_by) in caps.items():
        cap = getattr(rc, name)
        path = 1 + rc.LN_PATHS.index("HW" if "HW" in name else "W32")
        at_cap, above = _route(lib, dtype, cap, H), _route(lib, dtype, cap + covers, H)
        assert at_cap[0] == above[0] == path, name
        assert at_cap[k] == above[k], (name, "the grid still grows at the cap")
        assert at_cap[k] * covers == cap, (name, "the full grid does not cover exactly the cap in one trip")
        below = _route(lib, dtype, (at_cap[k] - 1) * sized_by, H)
        assert below[0] == path and below[k] == at_cap[k] - 1, (name, "the grid is full before its last workgroup is needed")
    # every case meant to exceed a cap does: the backward of the 4106-row cases, the forward of the fwd_only ones
    over_bwd = [c for c in rc.LN_CASES if c.rows == 4106]
    over_fwd = [c for c in rc.LN_CASES if c.fwd_only]
    assert {c.path for c in over_bwd} == {c.path for c in over_fwd} == set(rc.LN_PATHS)
    for c in over_bwd + over_fwd + rc.LN_FINALIZE_CASES:
        with _switches(c.env):
            r = _route(lib, c.dtype, c.rows, c.H)
        assert r[0] == 1 + rc.LN_PATHS.index(c.path), c.name
        if c in over_bwd:
            assert not c.fwd_only and r[2] * (8 if c.path == "HW" else 4) < c.rows, c.name
        if c in over_fwd:
            assert r[1] * (8 if c.path == "HW" else 16) < c.rows, c.name
    B, S, H = rc.EMB_FWD_LARGE
    assert _route(lib, "f32", B * S, H)[5] * 16 < B * S
    # the finalize cases: one stage by default, two under the switch their test sets (and never for the embedding, whose
    # backward grid the report gives apart)
    for c in rc.LN_FINALIZE_CASES:
        with _switches(c.env):
            assert _route(lib, c.dtype, c.rows, c.H)[2:4] == [250, 1], c.name
        with _switches(c.env + (("POLUS_LN_FIN_SINGLE", rc.LN_FIN_SINGLE),)):
            assert _route(lib, c.dtype, c.rows, c.H)[2:4] == [250, 2], c.name
    assert _route(lib, "bf16", 16384, 768) == [3, 2048, 512, 1, 3, 1024, 256]


def test_eff_seed_restates_the_host_mix():
    from polus_amd.models import dropout_salt, dropout_seed, dropout_seed_static
    for base, step, layer, site in ((1, 0, -1, 0), (12345, 7, 3, 2), (0xFFFFFFFF, 100000, 11, 1)):
        assert rc.eff_seed_np(dropout_seed_static(base, layer, site), dropout_salt(step)) == dropout_seed(base, step, layer, site)
    assert rc.eff_seed_np(0xFFFFFFFF, 2) == rc.eff_seed_np(1, 0)
    k = rc.keep_scale(9, 0.5, 3, 8)
    assert np.array_equal(k != 0, dropout_keep_np(9, 0.5, 0, 24).reshape(3, 8) != 0) and set(np.unique(k)) <= {0.0, 2.0}


# ------------------------------------------------------------------------------------------------- embeddings
def _scatter(de, ids, H):
    gw = np.zeros((rc.EMB_VOCAB, H))
    np.add.at(gw, ids, de)
    return gw


@pytest.mark.parametrize("case", [c for c in rc.EMB_CASES if not c.deterministic], ids=lambda c: f"{c.dtype}-H{c.H}-p{c.p}")
def test_embedding_tolerances_see_the_perturbations(case):
    B, S, H, rows = rc.EMB_B, rc.EMB_S, case.H, case.rows
    dt = rc.DT[case.dtype]
    p = rc.emb_tables(H, case.seed)
    dy_r = rounded(rc.emb_dy(case), dt)
    keep = rc.keep_scale(case.seed, case.p, rows, H).reshape(B, S, H) if case.p > 0 else None
    tol = rc.emb_tol(case.dtype)
    for idk in rc.EMB_ID_PATTERNS:
        raw = rc.emb_ids(idk, case.seed)
        ids = rc.emb_clamp(raw)
        flat = ids.reshape(-1)
        for ttk in rc.EMB_TYPE_PATTERNS:
            what = f"{case.dtype} H={H} p={case.p} ids={idk} types={ttk}"
            tt = rc.emb_types(ttk, case.seed)
            base = rc.emb_reference(p, H, ids, tt, dy_r, keep)
            # position taken as row // S: the oracle with the position table's rows permuted accordingly
            pos_of = (np.arange(rows) // S).reshape(B, S)
            e = p["emb.word"][ids] + p["emb.type"][np.zeros_like(ids) if tt is None else tt] + p["emb.pos"][pos_of]
            y, mean, rstd = ob.layer_norm_fwd(e, p["emb.ln.g"], p["emb.ln.b"], rc.EPS)
            _moves({**base, "y": y if keep is None else y * keep, "mean": mean, "rstd": rstd}, base, tol, f"{what}: position = row // S")
            if ttk == "mixed":
                _moves(rc.emb_reference(p, H, ids, None, dy_r, keep), base, tol, f"{what}: type ignored")
            # the word-table scatter, from the oracle's de (recovered through a one-row-per-token vocabulary)
            dyk = dy_r if keep is None else dy_r * keep
            de, _, _ = ob.layer_norm_bwd(dyk, p["emb.word"][ids] + p["emb.type"][np.zeros_like(ids) if tt is None else tt] + p["emb.pos"][:S][None],
                                         p["emb.ln.g"], base["mean"], base["rstd"])
            de = de.reshape(rows, H)
            assert relerr(_scatter(de, flat, H), base["emb.word"]) < 1e-12
            tail = rows % 8
            _moves({**base, "emb.word": _scatter(de[:rows - tail], flat[:rows - tail], H)}, base, tol, f"{what}: the last rows % 8 tokens left out")
            first = np.ones(rows, bool)
            for r0 in range(0, rows, 8):
                run = flat[r0:r0 + 8]
                first[r0:r0 + 8] = [i == list(run).index(v) for i, v in enumerate(run)]
            assert not first.all(), f"{what}: no duplicate id inside a run of 8"
            _moves({**base, "emb.word": _scatter(de[first], flat[first], H)}, base, tol, f"{what}: a duplicate inside a run of 8 counted once")
            if idk == "oor":
                ok = (raw.reshape(-1) >= 0) & (raw.reshape(-1) < rc.EMB_VOCAB)
                assert (~ok).sum() == 4
                _moves({**base, "emb.word": _scatter(de[ok], flat[ok], H)}, base, tol, f"{what}: an out-of-range id dropped")
            if case.p > 0:
                k1 = rc.keep_scale(case.seed, case.p, rows, H, shift=1).reshape(B, S, H)
                _moves(rc.emb_reference(p, H, ids, tt, dy_r, k1), base, tol, f"{what}: dropout index + 1")


def test_embedding_id_patterns():
    for kind in ("random", "oor"):
        ids = rc.emb_ids(kind, 5)
        assert (ids[:, -11:] == 0).all() and ids.shape == (rc.EMB_B, rc.EMB_S)
    assert len(np.unique(rc.emb_ids("same", 5))) == 1
    raw = rc.emb_ids("oor", 5).reshape(-1)
    assert raw[3] == -3 and raw[10] == rc.EMB_VOCAB + 5 and raw[11] == rc.EMB_VOCAB + 9 and 10 // 8 == 11 // 8
    assert rc.emb_clamp(raw)[10] == rc.emb_clamp(raw)[11] == rc.EMB_VOCAB - 1 and rc.emb_clamp(raw)[3] == 0
    assert rc.emb_types("none", 5) is None and not rc.emb_types("zero", 5).any() and len(np.unique(rc.emb_types("mixed", 5))) == 2
    B, S, H = rc.EMB_FWD_LARGE
    assert B * S > rc.LN_FWD_CAP_ROWS


# ------------------------------------------------------------------------------------------------- optimizer
def test_adam_table_and_tolerance():
    seg, n = rc.adam_table()
    assert len(seg) == rc.ADAM_SEGMENTS > 4096 and n % 4 == 0 and seg[-1][1] <= n
    assert (seg[1:, 0] >= seg[:-1, 1]).all() and (seg[1:, 0] > seg[:-1, 1]).any()       # disjoint, some gaps
    lens = seg[:, 1] - seg[:, 0]
    assert set(lens) == set(range(1, 14))
    assert {(int(b) % 4, int(l) % 4) for b, l in zip(seg[:, 0], lens)} == {(a, l) for a in range(4) for l in range(4)}
    assert {(int(b) % 4, int(l)) for b, l in zip(seg[:, 0], lens) if l < 4} == {(a, l) for a in range(4) for l in (1, 2, 3)}
    assert set(seg[:, 2]) == {0, 1, 2, 3}
    inside, shadow = rc.seg_masks(seg, n)
    assert (~inside).sum() >= rc.ADAM_SEGMENTS // 3 and shadow.any() and (inside & ~shadow).any()

    st = rc.adam_state(n)
    clip = rc.ADAM_CLIP
    scales = [rc.ADAM_GRAD_SCALE * clip, 1.0]
    base = rc.adam_reference(seg, st, scales)
    tol = {"p": rc.ADAM_TOL, "m": rc.ADAM_TOL, "v": rc.ADAM_TOL}
    for what, pert in (("grad_scale ignored", rc.adam_reference(seg, st, [clip, 1.0])),
                       ("clip_scale ignored", rc.adam_reference(seg, st, [rc.ADAM_GRAD_SCALE, 1.0])),
                       ("a segment's last len % 4 elements left unchanged", rc.adam_reference(seg, st, scales, tail_skip=True)),
                       ("decay applied to a no-decay segment", rc.adam_reference(seg, st, scales, decay_all=True))):
        for k in range(2):
            if k == 1 and "ignored" in what:
                continue                                    # step (b) runs without scales; (a)'s error is already in its state
            v = relerr(pert[k]["p"], base[k]["p"]) / rc.ADAM_TOL
            assert v >= MARGIN, f"step {k}: {what} moves p by only {v:.2f}x the tolerance"
            assert rc.violation(pert[k], base[k], tol) >= MARGIN
    # elements outside every segment stay as they were
    assert all(np.array_equal(base[k][nm][~inside], st[nm][~inside]) for k in range(2) for nm in ("p", "m", "v"))


def test_elementwise_sizes_cross_the_grid_caps():
    assert min(rc.CAST_SIZES) < 4 and max(rc.CAST_SIZES) > 2048 * 256 * 4 and max(rc.CAST_SIZES) % 4
    assert min(rc.ACT_SIZES) < 4 and max(rc.ACT_SIZES) > 2048 * 256 * 4 and max(rc.ACT_SIZES) % 4
    assert rc.SQNORM_N > 1024 * 256 * 4 and rc.SQNORM_N % 4 == 3
    assert rc.adam_table(1100)[0].shape[0] > 1024
    for n in rc.ACT_SIZES:
        _, u = rc.act_inputs(n)
        assert (u == 0).any() and u.min() == -9 and u.max() == 9
    # the activation derivatives against a central difference of the activations
    u = np.linspace(-6, 6, 1001) + 1e-3
    fwd = {"gelu": ob.gelu, "swish": ob.swish, "relu": lambda a: np.maximum(a, 0), "tanh": np.tanh}
    for act in rc.ACTS:
        num = (fwd[act](u + 1e-6) - fwd[act](u - 1e-6)) / 2e-6
        assert np.abs(num - rc.act_grad(act, u)).max() < 1e-8, act


def test_loss_cases_and_their_bound():
    f32 = lambda a: a.astype(np.float32)
    for rows, C, big in rc.LOSS_CASES:
        logits, labels, y, cw = rc.loss_inputs(rows, C, big)
        assert set(labels) == set(range(min(rows, C))) and (y.sum(-1) == 0).any()
        if big:
            assert np.abs(logits).max() > 89 and (logits[rows // 2] == logits[rows // 2, 0]).all()
            with np.errstate(over="ignore"):
                assert not np.isfinite(np.exp(f32(logits)).sum(-1)).all()       # overflows without the max subtracted
        # float32 arithmetic can meet the f32 dlogits bound on every case: the oracle's own functions on float32 inputs
        tol = rc.loss_dlogits_tol("f32")
        with np.errstate(over="ignore"):                    # the oracle's sigmoid forms exp(90) in float32: inf, then 0
            pairs = (("softmax", ol.sparse_softmax_xent_fwd(logits, labels)[1], ol.sparse_softmax_xent_fwd(f32(logits), labels)[1]),
                     ("weighted softmax", ol.weighted_softmax_xent_fwd(cw, np.eye(C)[labels], logits)[1],
                      ol.weighted_softmax_xent_fwd(f32(cw), f32(np.eye(C)[labels]), f32(logits))[1]),
                     ("sigmoid", ol.weighted_sigmoid_xent_fwd(cw, 0.3, y, logits)[1],
                      ol.weighted_sigmoid_xent_fwd(f32(cw), np.float32(0.3), f32(y), f32(logits))[1]))
        for what, d64, d32 in pairs:
            assert d32.dtype == np.float32
            assert relerr(d32, d64) <= tol / 2, (what, rows, C, big, relerr(d32, d64))
