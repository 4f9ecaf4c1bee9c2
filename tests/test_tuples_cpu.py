"""CPU: the float64 references of tests/tuple_ref.py against finite differences and against the all-pairs MaxSim
reference, the host-side refusals of the tuple and distillation entry points, and the tolerances of
tests/tuple_cases.py: the float32 restatement passes each of them, and each sits at least 5x below the change the
least visible instance of a kernel mistake would cause."""
import ctypes

import numpy as np
import pytest

from tests import maxsim_ref
from tests import tuple_cases as tc
from tests import tuple_ref as tr
from tests.util import relerr


def _fd(f, x, on, h=1e-5):
    """Central differences of the scalar f over the entries of x where `on`."""
    g = np.zeros_like(x)
    for idx in zip(*np.nonzero(on)):
        xp, xm = x.copy(), x.copy()
        xp[idx] += h
        xm[idx] -= h
        g[idx] = (f(xp) - f(xm)) / (2 * h)
    return g


@pytest.mark.parametrize("kind", ["kl", "mse"])
@pytest.mark.parametrize("shape", [(1, 2), (3, 3), (5, 65)], ids=lambda s: "x".join(map(str, s)))
def test_loss_references_agree_with_finite_differences(kind, shape):
    fn = tr.distill_kl if kind == "kl" else tr.margin_mse
    s, t = tc.loss_case(*shape, kind)
    s = s.astype(np.float64)
    loss, g = fn(s, t)
    on = ~np.isneginf(t)
    assert np.isfinite(loss) and np.isfinite(g).all() and (g[~on] == 0).all()
    fd = _fd(lambda x: fn(x, t)[0], s, on)
    assert relerr(g[on], fd[on]) < 1e-6, relerr(g[on], fd[on])
    if shape[0] >= 3:
        assert (g[1] == 0).all(), "the all-absent row"
    if kind == "mse" and shape[0] >= 5:
        assert (g[2] == 0).all(), "the row without a positive"


def test_dot_and_maxsim_tuple_references_agree_with_finite_differences():
    q, d, ds = tc.dot_case(33)
    q, d = q.astype(np.float64), d.astype(np.float64)
    for layout in tc.LAYOUTS:
        dq, dd = tr.dot_tuples_bwd(q, d, ds, layout)
        f = lambda a, b: float((tr.dot_tuples_fwd(a, b, layout) * ds).sum())
        assert relerr(dq, _fd(lambda x: f(x, d), q, np.ones_like(q, bool))) < 1e-8
        assert relerr(dd, _fd(lambda x: f(q, x), d, np.ones_like(d, bool))) < 1e-8
    # MaxSim is piecewise linear: away from ties a small step keeps every argmax
    shape = (3, 2, 5, 17, 32)
    q, d, qm, dm = tc.tuple_case(shape, "ragged")
    q, d = q.astype(np.float64), d.astype(np.float64)
    ds = np.random.Generator(np.random.PCG64(2)).standard_normal((3, 2))
    for layout in tc.LAYOUTS:
        _, am = tr.maxsim_tuples_fwd(q, d, qm, dm, layout)
        dq, dd = tr.maxsim_tuples_bwd(q, d, ds, am, layout)
        f = lambda a, b: float((tr.maxsim_tuples_fwd(a, b, qm, dm, layout)[0] * ds).sum())
        onq = np.zeros_like(q, bool); onq[:, :, :3] = True             # a few columns of every row
        ond = np.zeros_like(d, bool); ond[:, :, :2] = True
        assert relerr(dq[onq], _fd(lambda x: f(x, d), q, onq, 1e-7)[onq]) < 1e-6
        assert relerr(dd[ond], _fd(lambda x: f(q, x), d, ond, 1e-7)[ond]) < 1e-6
        assert (dq[qm == 0] == 0).all() and (dd[dm == 0] == 0).all()


@pytest.mark.parametrize("masks", tc.MASKS)
@pytest.mark.parametrize("shape", tc.SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_tuple_maxsim_reference_is_the_diagonal_pick_of_all_pairs(shape, masks):
    q, d, qm, dm = tc.tuple_case(shape, masks)
    B, n = shape[:2]
    score, am = maxsim_ref.maxsim_fwd(q, d, qm, dm)
    for layout in tc.LAYOUTS:
        rows = tr.doc_rows(B, n, layout)
        assert sorted(rows.reshape(-1)) == list(range(B * n)), "a layout is a bijection"
        s_t, am_t = tr.maxsim_tuples_fwd(q, d, qm, dm, layout)
        b = np.arange(B)[:, None]
        assert np.allclose(s_t, score[b, rows], rtol=1e-13, atol=1e-12) and np.array_equal(am_t, am[b, rows])


# ---------------------------------------------------------------------------------------------- host-side refusals
@pytest.fixture(scope="module")
def lib():
    from polus_amd import build
    build.build(verbose=False)
    from polus_amd import _lib
    return _lib.load()


def test_every_limit_is_refused_on_the_host_by_name(lib):
    p, q = ctypes.c_void_p(1 << 20), ctypes.c_void_p((1 << 20) + 4)     # dummy pointers: nothing is dereferenced

    def fwd(dtype=0, Q=p, D=p, score=p, lds=4, am=p, B=2, n=3, layout=0, Lq=8, Ld=8, E=32):
        return lib.polus_maxsim_tuples_fwd(dtype, Q, D, None, None, score, lds, am, B, n, layout, Lq, Ld, E, None)

    def bwd(dtype=0, Q=p, D=p, ds=p, lds=4, am=p, dQ=p, dD=p, B=2, n=3, layout=0, Lq=8, Ld=8, E=32):
        return lib.polus_maxsim_tuples_bwd(dtype, Q, D, ds, lds, am, dQ, dD, B, n, layout, Lq, Ld, E, None)

    shared = [(dict(dtype=7), b"dtype"), (dict(E=48), b"multiple of 32"), (dict(E=288), b"multiple of 32"),
              (dict(E=0), b"multiple of 32"), (dict(Lq=0), b"Lq <= 512"), (dict(Lq=513), b"Lq <= 512"),
              (dict(Ld=0), b"Ld <= 512"), (dict(Ld=513), b"Ld <= 512"), (dict(B=0), b"B <= 65535"),
              (dict(B=65536), b"B <= 65535"), (dict(n=0), b"n <= 65535"), (dict(n=65536, lds=65536), b"n <= 65535"),
              (dict(B=65535, n=65535, lds=65535, Lq=1), b"2^31 - 1"), (dict(B=4096, n=4096, lds=4096, Lq=128), b"B*n*Lq"),
              (dict(lds=2), b"lds"), (dict(layout=2), b"layout"), (dict(layout=-1), b"layout"), (dict(Q=None), b"null"),
              (dict(D=None), b"null"), (dict(am=None), b"null")]
    for call in (fwd, bwd):
        for kw, msg in shared:
            assert call(**kw) != 0 and msg in lib.polus_last_error(), (call.__name__, kw, lib.polus_last_error())
    assert fwd(score=None) != 0 and b"null" in lib.polus_last_error()
    assert fwd(Q=q) != 0 and b"16-byte" in lib.polus_last_error()
    assert fwd(D=q) != 0 and b"16-byte" in lib.polus_last_error()
    for kw in (dict(ds=None), dict(dQ=None), dict(dD=None)):
        assert bwd(**kw) != 0 and b"null" in lib.polus_last_error()

    def dfwd(dtype=0, a=p, ldq=40, d=p, ldd=40, score=p, lds=4, B=2, n=3, layout=0, W=33):
        return lib.polus_dot_tuples_fwd(dtype, a, ldq, d, ldd, score, lds, B, n, layout, W, None)

    def dbwd(dtype=0, a=p, ldq=40, d=p, ldd=40, ds=p, lds=4, dq=p, lddq=40, dd=p, lddd=40, B=2, n=3, layout=0, W=33):
        return lib.polus_dot_tuples_bwd(dtype, a, ldq, d, ldd, ds, lds, dq, lddq, dd, lddd, B, n, layout, W, None)

    dshared = [(dict(dtype=7), b"dtype"), (dict(W=0), b"W >= 1"), (dict(B=0), b"B <= 65535"), (dict(B=65536), b"B <= 65535"),
               (dict(n=0), b"n <= 65535"), (dict(n=65536, lds=65536), b"n <= 65535"),
               (dict(B=65535, n=65535, lds=65535), b"2^31 - 1"), (dict(lds=2), b"lds"), (dict(layout=2), b"layout"),
               (dict(ldq=32), b"row strides"), (dict(ldd=32), b"row strides"), (dict(a=None), b"null"), (dict(d=None), b"null")]
    for call in (dfwd, dbwd):
        for kw, msg in dshared:
            assert call(**kw) != 0 and msg in lib.polus_last_error(), (call.__name__, kw, lib.polus_last_error())
    for kw, msg in ((dict(lddq=32), b"row strides"), (dict(lddd=32), b"row strides"), (dict(dq=None), b"null"),
                    (dict(dd=None), b"null"), (dict(ds=None), b"null")):
        assert dbwd(**kw) != 0 and msg in lib.polus_last_error()
    assert dfwd(score=None) != 0 and b"null" in lib.polus_last_error()

    for name in ("polus_distill_kl", "polus_margin_mse"):
        fn = getattr(lib, name)

        def loss(s=p, lds=8, t=p, ldt=8, out=p, g=p, ldd=8, rows=3, n=8, ws=p, nb=1 << 20):
            return fn(s, lds, t, ldt, out, g, ldd, rows, n, ws, nb, None)
        for kw, msg in ((dict(rows=0), b"rows >= 1"), (dict(n=0), b"n <= 1024"), (dict(n=1025, lds=1025, ldt=1025, ldd=1025), b"n <= 1024"),
                        (dict(lds=7), b"row strides"), (dict(ldt=7), b"row strides"), (dict(ldd=7), b"row strides"),
                        (dict(s=None), b"null"), (dict(t=None), b"null"), (dict(out=None), b"null"), (dict(g=None), b"null"),
                        (dict(ws=None), b"workspace"), (dict(nb=8), b"workspace")):
            assert loss(**kw) != 0 and msg in lib.polus_last_error(), (name, kw, lib.polus_last_error())
            assert name.encode() in lib.polus_last_error()
    assert lib.polus_distill_workspace_bytes(32) >= 32 * 8


# ---------------------------------------------------------------------------------------------- tolerances
def _change(a, ref):
    """relerr with a non-finite result counted as infinitely visible (assert_close refuses it)."""
    e = relerr(a, ref)
    return e if np.isfinite(e) else np.inf


def test_loss_tolerances_hold_for_f32_and_sit_below_every_mistake():
    worst = {k: dict(loss=0.0, grad=0.0) for k in ("kl", "mse")}
    least = {}

    def seen(name, kind, what, change):
        key = (name, kind, what)
        least[key] = min(least.get(key, np.inf), change)

    for kind, fn in (("kl", tr.distill_kl), ("mse", tr.margin_mse)):
        for rows, n in tc.LOSS_SHAPES:
            s, t = tc.loss_case(rows, n, kind)
            loss, g = fn(s, t)
            l32, g32 = fn(s, t, dtype=np.float32)
            worst[kind]["loss"] = max(worst[kind]["loss"], relerr(l32, loss))
            worst[kind]["grad"] = max(worst[kind]["grad"], relerr(g32, g))
            on = ~np.isneginf(t)
            for cell in zip(*np.nonzero(~on)):
                if kind == "mse" and (cell[1] == 0 or not on[cell[0], 0]):
                    continue                                   # a negative of a row that has its positive
                l2, g2 = fn(s, t, count_absent=cell)
                seen("absent column counted", kind, "loss", _change(l2, loss))
                seen("absent column counted", kind, "grad", _change(g2, g))
            live = int(on.any(1).sum()) if kind == "kl" else int((on[:, 1:] & on[:, :1]).sum())
            if live > 1:                                       # else the factor is 1
                l2, g2 = fn(s, t, drop_mean=True)
                seen("mean factor dropped", kind, "loss", _change(l2, loss))
                seen("mean factor dropped", kind, "grad", _change(g2, g))
            if kind == "kl":
                seen("teacher and student swapped", kind, "grad", _change(fn(s, t, swap=True)[1], g))
            elif n > 2:
                l2, g2 = fn(s, t, positive=1)
                seen("column 0 not the positive", kind, "loss", _change(l2, loss))
                seen("column 0 not the positive", kind, "grad", _change(g2, g))
    print("f32 restatement, worst relative error:", worst)
    for key, change in sorted(least.items()):
        print(f"least visible {key}: {change:.3e}")
    for kind in worst:
        for what in ("loss", "grad"):
            assert worst[kind][what] <= tc.TOL[kind][what], (kind, what, worst[kind][what])
    for (name, kind, what), change in least.items():
        assert change >= 5 * tc.TOL[kind][what], (name, kind, what, change)
    assert {k[0] for k in least} == {"absent column counted", "mean factor dropped", "teacher and student swapped",
                                     "column 0 not the positive"}


def test_dot_tolerances_hold_for_f32_and_sit_below_a_dropped_term():
    worst = dict(score=0.0, grad=0.0)
    least = np.inf
    B, n = tc.DOT_BN
    for W in tc.DOT_W:
        q, d, ds = tc.dot_case(W)
        for layout in tc.LAYOUTS:
            ref = tr.dot_tuples_fwd(q, d, layout)
            worst["score"] = max(worst["score"], relerr(tr.dot_tuples_fwd(q, d, layout, np.float32), ref))
            for a, b in zip(tr.dot_tuples_bwd(q, d, ds, layout, np.float32), tr.dot_tuples_bwd(q, d, ds, layout)):
                worst["grad"] = max(worst["grad"], relerr(a, b))
            # the smallest term of every pair dropped
            prod = np.abs(q.astype(np.float64)[:, None, :] * d.astype(np.float64)[tr.doc_rows(B, n, layout)])
            for b in range(B):
                for j in range(n):
                    w = int(prod[b, j].argmin())
                    least = min(least, relerr(tr.dot_tuples_fwd(q, d, layout, skip=(b, j, w)), ref))
    print("f32 restatement, worst relative error:", worst, "least visible dropped term:", least)
    for mode in ("dot_f32", "dot_bf16"):
        assert worst["score"] <= tc.TOL[mode]["score"] and least >= 5 * tc.TOL[mode]["score"]
    assert worst["grad"] <= tc.TOL["dot_f32"]["grad"]
