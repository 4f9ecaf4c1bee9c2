"""CPU, no device: the GEMM case list (tests/gemm_cases.py) is held to the library's own routing, its exact cases to the
preconditions that make them exact, and its comparator to the bugs it is for.

routing: every case's expected route (the Python restatement in gemm_cases.py) against polus_gemm_route /
polus_dense_bwd_params_route / polus_dense_bwd_params_grouped_route, asked with made-up addresses that have the case's
alignment; every kernel x reduce combination gemm_route can return, and every value of the two dW reports, is reached.
comparator: a numpy emulation of a framed GEMM (same frames, same leading dimensions) run once correctly and once per planted
fault; check() passes the first and reports every other."""
import ctypes

import numpy as np
import pytest

from tests import gemm_cases as gc
from tests.gemm_cases import BY_NAME, CASES, EPI, build, check, expected_route, reference, switches
from tests.util import dropout_keep_np


@pytest.fixture(scope="module")
def lib():
    from polus_amd import build as b
    b.build(verbose=False)
    from polus_amd import _lib
    return _lib.load()


def _vp(frames, name):
    return ctypes.c_void_p(frames[name].address()) if name in frames else None


def _ld(frames, name):
    return frames[name].ld if name in frames else 0


def report(lib, case, frames):
    """The library's route report for a case, asked with made-up addresses; a dict with the fields of expected_route."""
    from polus_amd import _lib, ops
    code = {"f32": _lib.F32, "bf16": _lib.BF16}
    if case.op == "gemm":
        kw, out = gc.gemm_keywords(case), (ctypes.c_int * 12)()
        M, N, K = case.shape
        rc = lib.polus_gemm_route(code[case.dtype], kw["a_layout"], kw["b_layout"], code[case.c_dtype], _vp(frames, "A"), _ld(frames, "A"),
                                  _vp(frames, "B"), _ld(frames, "B"), _vp(frames, "C"), _ld(frames, "C"), M, N, K, kw["alpha"],
                                  _vp(frames, "bias"), _vp(frames, "resid"), _ld(frames, "resid"), _vp(frames, "aux"), _ld(frames, "aux"),
                                  ops.ACT_CODES[kw["act"]], kw["flags"], kw["split_k"], kw["drop_p"], out)
        assert rc == 0, lib.polus_last_error()
        r = ops.GemmRoute(ops.GEMM_KERNELS[out[0]], out[1], out[2], out[3], out[4], ops.GEMM_REDUCES[out[5]], out[6], *map(bool, out[7:12]))
        return r._asdict()
    if case.op == "dw":
        T, no, ni = case.shape
        out = (ctypes.c_int * 2)()
        rc = lib.polus_dense_bwd_params_route(code[case.dtype], _vp(frames, "dY"), _ld(frames, "dY"), _vp(frames, "X"), _ld(frames, "X"),
                                              _vp(frames, "dW"), _ld(frames, "dW"), _vp(frames, "db"), T, no, ni, case.split_k, out)
        assert rc == 0, lib.polus_last_error()
        return dict(ring=bool(out[0]), splits=out[1])
    T, probs = case.shape
    arr = (_lib.DwProblem * len(probs))()
    for k, (no, ni) in enumerate(probs):
        db = frames[f"db{k}"].address() if case.db else None
        arr[k] = _lib.DwProblem(frames[f"dY{k}"].address(), frames[f"dY{k}"].ld, frames[f"X{k}"].address(), frames[f"X{k}"].ld,
                                frames[f"dW{k}"].address(), frames[f"dW{k}"].ld, db, no, ni)
    out = (ctypes.c_int * (2 + len(probs)))()
    rc = lib.polus_dense_bwd_params_grouped_route(code[case.dtype], len(probs), arr, T, case.split_k, out)
    assert rc == 0, lib.polus_last_error()
    return dict(kernel=ops.DW_GROUPED_KERNELS[out[0]], fused_reduce=bool(out[1]), eff=tuple(out[2:]))


ROUTED = [c for c in CASES if c.op in ("gemm", "dw", "dwg")]


def test_routes_match_the_library_and_cover_every_route(lib):
    seen_gemm, seen_dw, seen_dwg = set(), set(), set()
    for case in ROUTED:
        frames = build(case)
        want = expected_route(case, frames)
        with switches(case):
            got = report(lib, case, frames)
        assert got == want, (case.name, got, want)
        if case.op == "gemm":
            seen_gemm.add((got["kernel"], got["reduce"]))
            if got["kernel"] == "v1":
                seen_gemm.add(("v1", "vec" if got["v1_vec"] else "elem"))
            if got["kernel"] in ("ring", "ring128", "pp", "pp_persist") and got["reduce"] == "none":
                seen_gemm.add((got["kernel"], got["tn"], got["mode"]))
            assert (got["persist_cus"] > 0) == (got["kernel"] == "pp_persist")
        elif case.op == "dw":
            seen_dw.add((got["ring"], got["splits"] > 1))
        else:
            seen_dwg.add((got["kernel"], got["fused_reduce"]))
            if case.split_k <= 0:
                seen_dwg.add((got["kernel"], "auto"))
                if len(set(got["eff"])) > 1:
                    seen_dwg.add((got["kernel"], "handout"))
        if not case.views:                  # the table's route: what the all-dense variant must run
            kernel = got.get("kernel", {True: "ring", False: "fallback"}.get(got.get("ring")))
            assert kernel == case.want, (case.name, got)
    # everything gemm_route can return: V1 never reduces with an epilogue (REDUCE_EPI needs `fast`), and only the 256 x 128
    # ring kernel writes slabs
    assert {k for k in seen_gemm if len(k) == 2} == {
        ("v1", "none"), ("v1", "plain"), ("v1", "vec"), ("v1", "elem"), ("ring", "none"), ("ring", "plain"), ("ring", "epi"),
        ("ring128", "none"), ("ring_drop", "none"), ("pp", "none"), ("pp_persist", "none")}
    modes = {k for k in seen_gemm if len(k) == 3}
    assert modes >= {("ring", 128, m) for m in (-1, 0, 1, 2, 3)} | {("ring128", 128, m) for m in range(4)} \
        | {("pp", tn, m) for tn in (256, 192) for m in range(4)} | {("pp_persist", 192, m) for m in range(4)}
    assert seen_dw == {(True, False), (True, True), (False, False), (False, True)}
    assert seen_dwg == {("one_by_one", False), ("ring_grouped", True), ("ring_grouped", False), ("pp_grouped", True),
                        ("pp_grouped", False), ("pp_streamk", True),
                        # split_k <= 0, the library's own slices: on each grouped kernel, and with grouped_splits' hand-out
                        # of one extra slice visible in the report on both even-split kernels
                        ("ring_grouped", "auto"), ("pp_grouped", "auto"), ("pp_streamk", "auto"),
                        ("ring_grouped", "handout"), ("pp_grouped", "handout")}


def test_every_view_kind_flips_the_predicate_it_is_for():
    case = BY_NAME["ring_resid/dense"]
    base = expected_route(case, build(case))
    assert base["kernel"] == "ring" and all(base[f] for f in ("a_vec", "b_vec", "epi_vec", "epi_vec16"))

    def route(**views):
        c = gc._with(case, views.items())
        return expected_route(c, build(c))
    for kind in ("pad16", "cls"):
        for t in ("A", "B", "C", "resid"):
            assert route(**{t: kind}) == base, (t, kind)
    for t in ("C", "resid"):
        r = route(**{t: "pad4"})
        assert r["epi_vec"] and not r["epi_vec16"] and r["kernel"] == "ring"
        for kind in ("pad1", "shift1"):
            r = route(**{t: kind})
            assert not r["epi_vec"] and not r["epi_vec16"] and r["kernel"] == "ring", (t, kind)
    for t, flag in (("A", "a_vec"), ("B", "b_vec")):
        for kind in ("pad1", "shift1"):
            r = route(**{t: kind})
            assert not r[flag] and r["kernel"] == "v1" and not r["v1_vec"], (t, kind)
    pp = BY_NAME["pp256_resid_k192/dense"]
    assert expected_route(pp, build(pp))["kernel"] == "pp"
    c = gc._with(pp, [("resid", "pad4")])
    assert expected_route(c, build(c))["kernel"] == "ring128"       # pp_tile needs epi_vec16; so few tiles take the 128 x 128 one


def test_route_reports_fail_where_the_calls_fail(lib):
    p = ctypes.c_void_p(1 << 20)
    out = (ctypes.c_int * 12)()
    ok = [1, 0, 0, 1, p, 64, p, 64, p, 64, 64, 64, 64, 1.0, None, None, 0, None, 0, 0, 0, 1, 0.0, out]

    def gemm(**kw):
        a = list(ok)
        for i, v in kw.items():
            a[int(i[1:])] = v
        rc = lib.polus_gemm_route(*a)
        return rc, lib.polus_last_error()
    assert gemm()[0] == 0
    for kw, msg in ((dict(_4=None), b"null operand"), (dict(_5=32), b"lda 32 too small"), (dict(_9=8), b"ldc 8 < N 64"),
                    (dict(_0=3), b"bad dtype"), (dict(_20=4), b"ACT_BWD needs aux"), (dict(_20=8), b"use polus_gemm_dropout"),
                    (dict(_22=1.5), b"0 <= p < 1"), (dict(_22=0.5, _1=1), b"needs K-contiguous operands"),
                    (dict(_15=p, _16=64, _21=2, _3=0, _12=128, _5=128, _7=128), b"split_k with a residual")):
        rc, err = gemm(**kw)
        assert rc != 0 and msg in err, (kw, err)
    two = (ctypes.c_int * 2)()
    assert lib.polus_dense_bwd_params_route(1, None, 64, p, 64, p, 64, p, 64, 64, 64, 1, two) != 0 and b"null pointer" in lib.polus_last_error()
    assert lib.polus_dense_bwd_params_route(1, p, 64, p, 64, p, 64, p, 0, 64, 64, 1, two) != 0 and b"bad shape" in lib.polus_last_error()
    assert lib.polus_dense_bwd_params_grouped_route(1, 0, None, 64, 1, two) != 0 and b"bad arguments" in lib.polus_last_error()


# ------------------------------------------------------------------------------------------------ exactness
def _bf16_round_trips(x):
    import torch
    t = torch.as_tensor(np.ascontiguousarray(x, dtype=np.float64))
    return bool((t.to(torch.bfloat16).double() == t).all())


def test_exact_cases_meet_the_preconditions_of_exactness():
    checked = 0
    for case in CASES:
        if not case.exact or case.refused or case.views:          # the data depends on the base alone
            continue
        frames = build(case)
        ref = reference(case, frames)
        depth = case.shape[{"gemm": 2, "thin_fwd": 1}.get(case.op, 0)]          # the contraction length
        for name, r in ref.items():
            assert np.isfinite(r).all(), (case.name, name)
            if frames[name].dtype == "bf16":
                assert _bf16_round_trips(r), (case.name, name, float(np.abs(r).max()))
            else:
                assert (r.astype(np.float32).astype(np.float64) == r).all(), (case.name, name)
            assert np.abs(r).max() * depth < 2 ** 24, (case.name, name)      # no sum on the way can leave f32's integers
            assert np.abs(r).max() < abs(gc.SENTINEL)
            checked += 1
    assert checked > 100


def test_dropping_a_k_chunk_changes_most_elements():
    case = BY_NAME["ring_resid/dense"]
    f = build(case)
    a, b = f["A"].view.astype(np.float64), f["B"].view.astype(np.float64)
    assert ((a @ b.T) != (a[:, :-8] @ b[:, :-8].T)).mean() > 0.7


# ------------------------------------------------------------------------------------------------ the comparator
def emulate(case, fault=None):
    """A framed GEMM / dW in numpy on the case's allocations, addressed like the kernels: flat buffers, offset + row * ld +
    col.  `fault` plants one bug.  Returns frames_after for check()."""
    frames = build(case)
    flat = {n: fr.buf.copy().reshape(-1) for n, fr in frames.items()}

    def idx(n, rows, cols, ld=None):
        fr = frames[n]
        return fr.offset + np.arange(rows)[:, None] * (fr.ld if ld is None else ld) + np.arange(cols)[None, :]

    def read(n, rows, cols, ld=None):
        return flat[n][idx(n, rows, cols, ld)].astype(np.float64)

    if case.op == "dw":
        T, no, ni = case.shape
        dy, x = read("dY", T, no), read("X", T, ni)
        flat["dW"][idx("dW", no, ni)] = dy.T @ x + (read("dW", no, ni) if case.accumulate else 0.0)
        db = (dy[:-1] if fault == "db_short" else dy).sum(0, keepdims=True)
        flat["db"][idx("db", 1, no)] = db + (read("db", 1, no) if case.accumulate else 0.0)
        return {n: flat[n].reshape(frames[n].buf.shape) for n in ("dW", "db")}

    M, N, K = case.shape
    assert case.layouts == (0, 0)
    e = EPI[case.epi]
    ldc = frames["C"].ld
    kk = K - 8 if fault == "k_chunk" else K
    a = read("A", M, kk, K if fault == "operand_ld" else None)
    b = read("B", N, kk)
    acc = a @ b.T
    if fault == "pad_column":                       # an operand chunk fetched from beyond K, its partner zero-filled
        acc = acc + read("A", M, K + 1)[:, K:] * 0.0
    v = (1.0 if fault == "alpha" else e.get("alpha", 1.0)) * acc
    if e.get("bias"):
        v = v + read("bias", 1, N)
    out = {}
    if e.get("aux") == "w":
        flat["aux"][idx("aux", M, N)] = v
        out["aux"] = None
        v = np.maximum(v, 0.0)
    if e.get("aux") == "r":
        v = v * (read("aux", M, N, ldc if fault == "aux_ld" else None) > 0)
    if e.get("drop"):
        w = ldc if fault == "drop_index" else N
        v = v * dropout_keep_np(case.drop_seed, gc.DROP_P, 0, M * w).reshape(M, w)[:, :N] * 2.0
    if e.get("resid"):
        v = v + read("resid", M, N, ldc if fault == "resid_ld" else None)
    if e.get("accum") and fault != "accum":
        v = v + read("C", M, N)
    rows = M - 1 if fault == "last_row" else M
    flat["C"][idx("C", rows, N)] = v[:rows]
    if fault == "store_past_n":
        flat["C"][idx("C", M, N + 4)[:, N:]] = 0.0
    if fault == "row_at_m":
        flat["C"][idx("C", M + 1, N)[M]] = v[0]
    out["C"] = None
    return {n: flat[n].reshape(frames[n].buf.shape) for n in out}


FAULTS = [  # (fault, the smallest case whose views make it visible)
    ("operand_ld", "v1_f32_00_vec_resid/A=pad16"),
    ("resid_ld", "v1_f32_00_vec_resid/resid=cls"),
    ("aux_ld", "v1_f32_act_bwd/A=cls+B=pad16+C=pad16+aux=cls"),
    ("drop_index", "v1_bf16_drop/C=pad16"),
    ("k_chunk", "v1_f32_00_vec_resid/dense"),
    ("pad_column", "v1_f32_00_vec_resid/A=pad16"),
    ("store_past_n", "v1_f32_00_vec_resid/C=pad16"),
    ("row_at_m", "v1_f32_00_vec_resid/dense"),
    ("last_row", "v1_f32_00_vec_resid/dense"),
    ("accum", "v1_f32_accum/dense"),
    ("alpha", "v1_f32_alpha/dense"),
    ("db_short", "dw_fallback_small_bf16/dense"),
]


@pytest.mark.parametrize("fault,name", FAULTS)
def test_comparator_sees_the_planted_fault(fault, name):
    case = BY_NAME[name]
    ref = reference(case, build(case))
    assert check(case, emulate(case), ref) == []
    found = check(case, emulate(case, fault), ref)
    assert found, f"{fault} on {name} went unnoticed"


def test_comparator_passes_the_correct_emulation_of_every_small_gemm_case():
    n = 0
    for case in CASES:
        if case.op == "gemm" and case.exact and case.layouts == (0, 0) and case.shape[0] <= 100:
            assert check(case, emulate(case), reference(case, build(case))) == [], case.name
            n += 1
    assert n > 30


def test_case_list_is_well_formed():
    assert 200 <= len(CASES) <= 520
    for case in CASES:
        assert not case.fast or gc.dense_twin(case).views == ()
        frames = build(case)
        for fr in frames.values():
            assert fr.buf.shape[0] == fr.rows + 2 * gc.GUARD and fr.ld >= fr.c0 + fr.cols
            if fr.role != "in":
                assert (fr.buf[~fr.inside()] == gc.SENTINEL).all()
            else:
                assert np.isnan(fr.buf[~fr.inside()]).all() and np.isfinite(fr.view).all()
