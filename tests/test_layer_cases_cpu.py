"""The float64 Dense reference and the case table of tests/layer_cases.py, checked without a GPU: the reference's gradients
against central finite differences, and the table against the dispatch it is meant to cover."""
import numpy as np
import pytest

from tests import layer_cases as lc

FD_TOL = 1e-6                  # float64 against float64, relative to max|gradient|: not a device tolerance
FD_STEP = 1e-6


def _fd_inputs(act, with_resid):
    r = np.random.Generator(np.random.PCG64(11 + len(act or "") + (100 if with_resid else 0)))
    rows, H, C = 5, 7, 3
    x, w, b = r.standard_normal((rows, H)), r.standard_normal((C, H)) * 0.5, r.standard_normal(C)
    dy = r.standard_normal((rows, C))
    resid = r.standard_normal((rows, H)) if with_resid else None
    return x, w, b, dy, resid


@pytest.mark.parametrize("with_resid", [False, True], ids=["plain", "resid"])
@pytest.mark.parametrize("act", [None] + list(lc.ACTS), ids=lambda a: a or "linear")
def test_reference_gradients_match_finite_differences(act, with_resid):
    """L = sum(y * dy) has dL/dx = du W, dL/dW = du^T x, dL/db = sum du; dx_resid is added to dx and to nothing else."""
    x, w, b, dy, resid = _fd_inputs(act, with_resid)
    ref = lc.dense_reference(x, w, b, dy, act=act, resid=resid)
    if act == "relu":          # precondition: no pre-activation within reach of the kink
        assert np.abs(ref["u"]).min() > 100 * FD_STEP * max(np.abs(x).max(), np.abs(w).max(), 1.0) * x.shape[1]
    loss = lambda x_, w_, b_: float((lc.dense_reference(x_, w_, b_, act=act)["y"] * dy).sum())

    def fd(k):
        args = [x, w, b]
        g = np.zeros_like(args[k])
        for idx in np.ndindex(*args[k].shape):
            hi, lo = [a.copy() for a in args], [a.copy() for a in args]
            hi[k][idx] += FD_STEP
            lo[k][idx] -= FD_STEP
            g[idx] = (loss(*hi) - loss(*lo)) / (2 * FD_STEP)
        return g
    dx = ref["dx"] - (resid if with_resid else 0.0)
    for name, got, k in (("dx", dx, 0), ("dw", ref["dw"], 1), ("db", ref["db"], 2)):
        num = fd(k)
        err = np.abs(got - num).max() / np.abs(num).max()
        print(f"[layer-ref] {act or 'linear'} {'resid' if with_resid else 'plain'} {name}: rel err {err:.3e} vs finite differences")
        assert err <= FD_TOL, f"{name}: {err:.3e}"
    if with_resid:
        plain = lc.dense_reference(x, w, b, dy, act=act)
        assert np.array_equal(ref["dw"], plain["dw"]) and np.array_equal(ref["db"], plain["db"]) and np.array_equal(ref["y"], plain["y"])


def test_reference_roundings_are_applied_where_the_paths_apply_them():
    x, w, b, dy = lc.dense_inputs("bf16", 9, 16, 3, seed=3)
    exact = lc.dense_reference(x, w, b, dy)
    cast = lc.dense_reference(x, w, b, dy, **lc.path_roundings("bf16", False, "f32"))
    assert np.array_equal(exact["y"], cast["y"])
    assert np.array_equal(cast["du"], lc.rounded(dy, lc.DT["bf16"])) and not np.array_equal(cast["du"], dy)
    assert lc.path_roundings("bf16", True, "f32") == {"dy_dtype": "f32"}
    assert lc.path_roundings("f32", False, "bf16") == {"dy_dtype": "bf16"}          # widening cast: bf16 values, exactly
    assert lc.path_roundings("f32", False, "f32") == {"dy_dtype": "f32"}
    assert lc.path_roundings("bf16", False, "f32", act="gelu") == {"dy_dtype": "bf16", "u_dtype": "bf16", "du_dtype": "bf16"}
    no_bias = lc.dense_reference(x, w, None, dy)
    assert np.array_equal(no_bias["y"], x @ w.T)


def test_gate_restatement_on_known_shapes():
    # heads the product builds: BERT token classification, the NER MLP head, the cross-encoder's Dense(1)
    for dtype in lc.ENGINES:
        assert lc.thin_supported(dtype, 768, 4) and lc.thin_supported(dtype, 128, 3) and lc.thin_supported(dtype, 1024, 1)
        assert not lc.thin_supported(dtype, 768, 10)                                 # the tutorial's Dense(10)
        assert not lc.thin_supported(dtype, 768, 0) and not lc.thin_supported(dtype, 768, 9)
        assert not lc.thin_supported(dtype, 0, 4) and not lc.thin_supported(dtype, 1032, 4)
    assert lc.thin_supported("f32", 4, 1) and not lc.thin_supported("bf16", 4, 1)
    assert lc.thin_supported("f32", 260, 4) and not lc.thin_supported("bf16", 260, 4)
    assert not lc.thin_supported("f32", 1028, 4) and not lc.thin_supported("f16", 768, 4)
    # the layer's own conditions
    assert lc.layer_thin("bf16", 768, 4) and not lc.layer_thin("bf16", 768, 4, env="0") and lc.layer_thin("bf16", 768, 4, env="1")
    assert not lc.layer_thin("bf16", 768, 4, activation="relu")
    assert not lc.layer_thin("bf16", 768, 4, col_stride=2)
    assert lc.layer_thin("bf16", 768, 4, base_elems=8, row_stride=784) and not lc.layer_thin("bf16", 768, 4, base_elems=9, row_stride=784)
    assert lc.layer_thin("f32", 768, 4, base_elems=4, row_stride=776) and not lc.layer_thin("f32", 768, 4, row_stride=773)


def test_case_table_reaches_every_path_and_instantiation():
    names = [c.name for c in lc.CASES]
    assert len(set(names)) == len(names)
    for engine in lc.ENGINES:
        mine = [c for c in lc.CASES if c.engine == engine]
        assert {c.thin for c in mine} == {True, False}, engine
        hit = {c.instance for c in mine if c.thin}
        want = {"bf16": {(4, 1), (4, 2), (8, 1), (8, 2)}, "f32": {(4, 2), (4, 4), (8, 2), (8, 4)}}[engine]
        assert want == lc.THIN_INSTANCES[engine]
        assert hit == want, f"{engine}: THIN_DISPATCH instantiations without a case: {sorted(want - hit)}"
        # every instantiation at every row count, with a bias
        for inst in want:
            assert {c.rows for c in mine if c.instance == inst and c.use_bias} >= set(lc.ROWS), (engine, inst)
        assert any(not c.use_bias and c.thin for c in mine) and any(not c.use_bias and not c.thin for c in mine)
    bf = [c for c in lc.CASES if c.engine == "bf16"]
    assert {c.out for c in bf if c.thin} == {"f32", "compute"} and {c.out for c in bf if not c.thin} == {"f32", "compute"}
    # the shapes and row counts the table must keep
    shapes = {(c.H, c.C) for c in lc.CASES}
    assert shapes >= {(128, 3), (264, 8), (768, 4), (1024, 1), (768, 10), (1032, 4)}
    for e in lc.ENGINES:
        for H, C in shapes:
            assert {c.rows for c in lc.CASES if (c.engine, c.H, c.C) == (e, H, C)} >= {5, 37, 513, 4099}
    expect = {("bf16", 128, 3): (4, 1), ("bf16", 264, 8): (8, 1), ("bf16", 768, 4): (4, 2), ("bf16", 1024, 1): (4, 2),
              ("bf16", 520, 5): (8, 2), ("f32", 128, 3): (4, 2), ("f32", 264, 8): (8, 2), ("f32", 768, 4): (4, 4),
              ("f32", 1024, 1): (4, 4), ("f32", 520, 5): (8, 4)}
    for (e, H, C), inst in expect.items():
        assert lc.thin_instance(e, H, C) == inst, (e, H, C)
    for e in lc.ENGINES:
        assert not lc.layer_thin(e, 768, 10) and not lc.layer_thin(e, 1032, 4)


@pytest.fixture(scope="module")
def lib():
    from polus_amd import _lib, build
    build.build(verbose=False)
    return _lib.load()


def test_restatement_equals_the_library(lib):
    """polus_dense_thin_supported and polus_dense_thin_bwd_workspace_bytes are host-only: the gate, the workgroup count and
    the chunk count of the chosen instantiation (the pitch of the partial sums), restated in layer_cases.py, against them."""
    import ctypes
    lib.polus_dense_thin_bwd_workspace_bytes.restype = ctypes.c_size_t
    code = {"f32": 0, "bf16": 1}
    for dtype in lc.ENGINES:
        for H in sorted({0, 2, 4, 6, 8, 12, 252, 256, 260, 504, 512, 520, 1024, 1028, 1032} | {h for h, _ in lc.SHAPES}):
            for C in (0, 1, 3, 4, 5, 8, 9, 10):
                got = bool(lib.polus_dense_thin_supported(code[dtype], H, C))
                assert got == lc.thin_supported(dtype, H, C), (dtype, H, C)
                if not got:
                    continue
                nch = lc.thin_instance(dtype, H, C)[1]
                for rows in lc.ROWS + (1, 4096, 100000):
                    want = lc.thin_blocks(rows) * (C + 1) * nch * 64 * lc.THIN_VEC[dtype] * 4
                    assert lib.polus_dense_thin_bwd_workspace_bytes(code[dtype], rows, H, C) == want, (dtype, rows, H, C)
    assert not lib.polus_dense_thin_supported(2, 768, 4)


def test_row_counts_reach_the_grid_stride_loop():
    assert lc.thin_blocks(5) == 1 and lc.thin_sweeps(5) == (2, 1)            # one workgroup of 4 waves, wave 0 takes row 4 too
    assert lc.thin_blocks(37) == 5 and lc.thin_sweeps(37) == (2, 17)
    assert lc.thin_blocks(513) == 65 and lc.thin_sweeps(513)[0] == 2
    assert lc.thin_blocks(4099) == lc.THIN_MAX_BLOCKS and lc.thin_sweeps(4099) == (3, 3)
