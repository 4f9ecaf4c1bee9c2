"""CPU: the NumPy reference of rank fusion (tests/fusion_ref.py) against an independent float64 statement of the rule and
a hand-worked example, the host-side argument checks of polus_fuse_lists, the host logic of HybridSearch with stub
stages, and the polus.ir re-export."""
import collections
import ctypes

import numpy as np
import pytest

from tests import fusion_cases as fc
from tests import fusion_ref as fr


def _fuse64(c, mode):
    """The rule in float64, vectorised per list row and joined through dicts: per query {id: (value, sum of the
    contributions' magnitudes, number of contributions)}.  Takes the f32 inputs as they are (weights and rrf_k rounded to
    f32 first, as the entry point receives them)."""
    ids, scores = c["ids"], c["scores"].astype(np.float64)
    L, Q, C = ids.shape
    w = np.ones(L) if c["weights"] is None else np.asarray(c["weights"], np.float32).astype(np.float64)
    k = float(np.float32(c["rrf_k"]))
    rows = []
    for r in range(Q):
        acc = collections.defaultdict(lambda: [0.0, 0.0, 0])
        for l in range(L):
            ok = (ids[l, r] >= 0) & (ids[l, r] < c["n_docs"]) & np.isfinite(scores[l, r])
            if not ok.any():
                continue
            rank = np.cumsum(ok)
            s = scores[l, r]
            if mode == "rrf":
                v = w[l] / (k + rank)
            elif mode == "sum":
                v = w[l] * s
            else:
                lo, hi = s[ok].min(), s[ok].max()
                v = w[l] * ((s - lo) / (hi - lo) if hi > lo else np.ones(C))
            for col in np.nonzero(ok)[0]:
                e = acc[int(ids[l, r, col])]
                e[0] += v[col]
                e[1] += abs(v[col])
                e[2] += 1
        rows.append(acc)
    return rows


@pytest.mark.parametrize("mode", fc.MODE_NAMES)
def test_reference_against_float64(mode):
    worst, seen = 0.0, 0
    for name in fc.NAMES:
        c = fc.case(name)
        out_id, out_val, count = fc.reference(name, mode)
        L, Q, C = c["ids"].shape
        with np.errstate(all="ignore"):
            want = _fuse64(c, mode)
        for r in range(Q):
            n = int(count[r])
            assert out_id[r, :n].tolist() == sorted(want[r]), (name, r)
            assert (out_id[r, n:] == -1).all() and (out_val[r, n:] == -np.inf).all() and n == len(want[r]), (name, r)
            for d, got in zip(out_id[r, :n], out_val[r, :n]):
                v, mag, terms = want[r][int(d)]
                err, bound = abs(float(got) - v), fc.value_bound(terms) * mag
                assert err <= bound, (name, r, int(d), err, bound)
                if bound > 0:
                    worst = max(worst, err / bound)
            seen += n
    print(f"[fusion] reference vs float64, {mode}: {seen} fused scores over {len(fc.NAMES)} cases, worst error / bound {worst:.3f}")


def test_cases_show_what_they_are_for():
    out_id, out_val, count = fc.reference("disjoint", "sum")
    L, Q, C = fc.case("disjoint")["ids"].shape
    assert (count == L * C).all()
    _, _, count = fc.reference("identical", "sum")
    assert (count == fc.case("identical")["ids"].shape[2]).all()
    _, _, count = fc.reference("partial", "sum")
    assert ((count > 70) & (count < 210)).all()
    for mode in fc.MODE_NAMES:
        out_id, out_val, count = fc.reference("holes", mode)
        assert count[3] == 0 and (out_id[3] == -1).all() and (out_val[3] == -np.inf).all()
    # a hole moves the ranks behind it up: the entries after a dropped column, a NaN and an id >= n_docs are ranks 1, 2
    ids = np.array([[[-1, 4, 8, 6, 9, 2]]], np.int32)
    scores = np.array([[[5.0, 4.0, np.nan, 3.0, 2.0, 1.0]]], np.float32)
    out_id, out_val, count = fr.fuse_lists(ids, scores, 9, "rrf")
    assert count.tolist() == [3] and out_id[0, :3].tolist() == [2, 4, 6]
    assert out_val[0, :3].tolist() == [np.float32(1) / np.float32(63), np.float32(1) / np.float32(61), np.float32(1) / np.float32(62)]
    # the symmetric pair ties bit for bit under rrf, and a search returns the lower id first
    out_id, out_val, count = fc.reference("symmetric", "rrf")
    assert out_id[0, :2].tolist() == [3, 7] and out_val[0, 0].view(np.int32) == out_val[0, 1].view(np.int32)
    val, idx = fr.topk(out_id, out_val, 2)
    assert idx.tolist() == [[3, 7]]
    # scores = None under rrf is the rule with every score finite
    for name in ("C = 65", "partial", "repeats"):
        a, b = fc.reference(name, "rrf"), fc.reference(name, "rrf", False)
        assert all(np.array_equal(x.view(np.int32), y.view(np.int32)) for x, y in zip(a, b))
    a, b = fc.reference("holes", "rrf"), fc.reference("holes", "rrf", False)
    assert not np.array_equal(a[2], b[2])


def test_hand_worked_two_lists_of_three():
    ids = np.array([[[5, 2, 9]], [[2, 7, 5]]], np.int32)
    scores = np.array([[[3.0, 2.0, 1.0]], [[10.0, 6.0, 2.0]]], np.float32)
    w = [1.0, 0.5]
    # rrf_k = 1: list 0 gives 1/2, 1/3, 1/4 to documents 5, 2, 9; list 1 gives 0.5/2, 0.5/3, 0.5/4 to 2, 7, 5
    want = {"rrf": [1.0 / 3.0 + 0.25, 0.5 + 0.125, 0.5 / 3.0, 0.25],
            # sum: 3, 2, 1 and 5, 3, 1
            "sum": [2.0 + 5.0, 3.0 + 1.0, 3.0, 1.0],
            # minmax: list 0 over [1, 3] gives 1, 0.5, 0; list 1 over [2, 10] gives 0.5 * (1, 0.5, 0)
            "minmax": [0.5 + 0.5, 1.0 + 0.0, 0.25, 0.0]}
    for mode in fc.MODE_NAMES:
        out_id, out_val, count = fr.fuse_lists(ids, scores, 10, mode, w, rrf_k=1.0)
        assert count.tolist() == [4] and out_id.tolist() == [[2, 5, 7, 9, -1, -1]]
        assert np.allclose(out_val[0, :4], want[mode], rtol=2.0 ** -22, atol=0) and (out_val[0, 4:] == -np.inf).all()
        if mode != "rrf":
            assert out_val[0, :4].tolist() == want[mode]               # dyadic values: exact
    val, idx = fr.topk(*fr.fuse_lists(ids, scores, 10, "minmax", w)[:2], 3)
    assert idx.tolist() == [[2, 5, 7]] and val.tolist() == [[1.0, 1.0, 0.25]]


@pytest.fixture(scope="module")
def lib():
    from polus_amd import build
    build.build(verbose=False)
    from polus_amd import _lib
    return _lib.load()


def test_entry_point_refuses_bad_arguments_on_the_host(lib):
    p = ctypes.c_void_p(16)
    names = ("ids", "lsi", "ldi", "scores", "lss", "lds", "L", "Q", "C", "n_docs", "mode", "weights", "rrf_k", "out_id",
             "ldoi", "out_val", "ldov", "count", "stream")
    base = dict(ids=p, lsi=4000, ldi=1000, scores=p, lss=4000, lds=1000, L=2, Q=4, C=1000, n_docs=50000, mode=0,
                weights=None, rrf_k=60.0, out_id=p, ldoi=2000, out_val=p, ldov=2000, count=p, stream=None)
    call = lambda **kw: lib.polus_fuse_lists(*[dict(base, **kw)[a] for a in names])
    f3 = lambda *v: (ctypes.c_float * len(v))(*v)
    for kw, msg in ((dict(L=9, C=100, ldoi=900, ldov=900), b"L <= 8"), (dict(L=0), b"1 <= L"),
                    (dict(L=1, C=4097, ldi=5000, lds=5000, ldoi=5000, ldov=5000), b"L*C <= 4096"),
                    (dict(L=4, C=1025, ldi=2000, lds=2000, lsi=9000, lss=9000, ldoi=5000, ldov=5000), b"L*C <= 4096"),
                    (dict(scores=None, mode=1), b"scores"), (dict(scores=None, mode=2), b"scores"),
                    (dict(weights=f3(1.0, float("nan"))), b"weights must be finite"),
                    (dict(weights=f3(float("inf"), 1.0)), b"weights must be finite"),
                    (dict(rrf_k=-1.0), b"rrf_k"), (dict(rrf_k=float("inf")), b"rrf_k"), (dict(rrf_k=float("nan")), b"rrf_k"),
                    (dict(ldi=999), b"ldi"), (dict(lds=999), b"lds"), (dict(lsi=3999), b"lsi"), (dict(lss=3999), b"lss"),
                    (dict(ldoi=1999), b"ldoi"), (dict(ldov=1999), b"ldoi"),
                    (dict(mode=3), b"mode"), (dict(mode=-1), b"mode"), (dict(Q=0), b"Q >= 1"), (dict(C=0), b"C >= 1"),
                    (dict(n_docs=0), b"n_docs"), (dict(ids=None), b"null pointer"), (dict(out_id=None), b"null pointer"),
                    (dict(out_val=None), b"null pointer"), (dict(count=None), b"null pointer")):
        assert call(**kw) != 0, kw
        err = lib.polus_last_error()
        assert b"polus_fuse_lists" in err and msg in err, (kw, err)
    # a negative rrf_k is nobody's business outside rrf, and scores may be absent under rrf: refused for the next reason
    assert call(mode=1, rrf_k=-1.0, ldoi=1999) != 0 and b"ldoi" in lib.polus_last_error()
    assert call(scores=None, ldoi=1999) != 0 and b"ldoi" in lib.polus_last_error()


def test_ops_wrapper_has_no_cpu_path():
    import torch
    from polus_amd import ops
    from polus_amd._lib import PolusHipError
    ids = torch.zeros((2, 1, 4), dtype=torch.int32)
    with pytest.raises(PolusHipError):
        ops.fuse_lists(ids, None, torch.zeros((1, 8), dtype=torch.int32), torch.zeros((1, 8)), torch.zeros(1, dtype=torch.int32), 10, "rrf")


class _Stage:
    """A stage that numbers documents from `start` and must never be searched."""

    def __init__(self, start=0):
        self.n = start

    def __len__(self):
        return self.n

    def add(self, documents):
        import torch
        k = len(documents["input_ids"])
        out = torch.arange(self.n, self.n + k, dtype=torch.int32)
        self.n += k
        return out

    def search(self, queries, k):
        raise AssertionError("searched before the arguments were checked")


def test_hybrid_search_host_logic():
    from polus_amd.ir import HybridSearch, fusion
    from polus_amd.ir.search import CorpusIndex
    ok = HybridSearch([_Stage(), _Stage()], 2048, method="minmax", weights=[1, 0.25], rrf_k=0)
    assert ok.depth == 2048 and ok.weights == [1.0, 0.25] and len(ok) == 0
    for stages, kw in (([], dict(depth=10)), ([_Stage()] * 9, dict(depth=10)), ([_Stage()] * 2, dict(depth=2049)),
                       ([_Stage()] * 8, dict(depth=513)), ([_Stage()], dict(depth=0)), ([_Stage()], dict(depth=10, method="zscore")),
                       ([_Stage()] * 2, dict(depth=10, weights=[1.0])), ([_Stage()] * 2, dict(depth=10, weights=[1.0, float("nan")])),
                       ([_Stage()], dict(depth=10, rrf_k=-1.0)), ([_Stage()], dict(depth=10, rrf_k=float("inf"))),
                       ([_Stage(), CorpusIndex(None, object())], dict(depth=1025))):
        with pytest.raises(ValueError):
            HybridSearch(stages, **kw)
    assert HybridSearch([_Stage(), CorpusIndex(None, object())], 1024).depth == 1024
    assert HybridSearch([_Stage()] * 8, 512).depth == 512
    with pytest.raises(ValueError, match="1 <= k"):
        ok.search(None, 1025)
    with pytest.raises(ValueError, match="1 <= k"):
        ok.search(None, 0)
    docs = {"input_ids": np.zeros((3, 4), np.int32)}
    assert ok.add(docs).tolist() == [0, 1, 2] and ok.add(docs).tolist() == [3, 4, 5] and len(ok) == 6
    bad = HybridSearch([_Stage(), _Stage(), _Stage(1)], 10)
    with pytest.raises(ValueError, match="different ids"):
        bad.add(docs)
    import torch
    pair = (torch.zeros((2, 3)), torch.zeros((2, 3), dtype=torch.int32))
    with pytest.raises(ValueError):
        fusion.fuse([pair] * 9, 10)
    with pytest.raises(ValueError):
        fusion.fuse([pair, (torch.zeros((2, 4)), torch.zeros((3, 4), dtype=torch.int32))], 10)
    with pytest.raises(ValueError, match="4096"):
        fusion.fuse([(torch.zeros((2, 2049)), torch.zeros((2, 2049), dtype=torch.int32))] * 2, 10)


def test_reexports():
    import polus.ir.fusion as pf
    import polus_amd.ir as ir
    from polus_amd.ir import fusion
    assert pf.HybridSearch is fusion.HybridSearch and pf.fuse is fusion.fuse
    assert ir.HybridSearch is fusion.HybridSearch and ir.fuse is fusion.fuse
    from polus_amd import _lib
    assert "polus_fuse_lists" in _lib.SIGNATURES
