"""CPU: the NumPy restatement of the IVF-PQ rules (tests/ivfpq_ref.py) against float64, the conditions under which the planted
corpus and the fit case are exact (checked on the reference alone), IVFPQCodec and the constructor's refusals, the route, the new
symbols in the binding and the host-side refusals of every polus_ivfpq_* entry point and wrapper (no launch without a GPU)."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from tests import ivfpq_cases as ic
from tests import ivfpq_ref as ir
from tests import pq_ref as pr
from tests import search_ref as sr
from tests.util import rounded

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("polus_ivfpq_scores_ids", "polus_ivfpq_scores_ids_route", "polus_ivfpq_residual", "polus_ivfpq_coarse_update")
LDS_BYTES = 160 * 1024


@pytest.fixture(scope="module")
def lib():
    from polus_amd import build
    build.build(verbose=False)
    from polus_amd import _lib
    return _lib.load()


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, np.float32)).view(np.int32)


# ---------------------------------------------------------------- the reference itself
def test_reference_scores_against_float64():
    m, ksub, Q, K = 20, 16, 3, 7
    lut, cdot, coarse, codes = ic.scan_case(m, ksub, Q, K)
    got = ir.full_scores(lut, cdot, coarse, codes)
    want = cdot.astype(np.float64)[:, coarse] + sum(lut.astype(np.float64)[:, j, codes[:, j]] for j in range(m))
    worst = float(np.abs(got - want).max())
    tol = (m + 1) * 2.0 ** -24 * float(np.abs(want).max() + np.abs(lut).max() * m)      # m + 1 roundings of sums below that
    print(f"[ivfpq] reference scores against float64: worst {worst:.3e}, bound {tol:.3e}")
    assert worst <= tol
    cand = ic.candidates(Q, 65, ic.SCAN_N)
    ids = ir.scores_ids(lut, cdot, coarse, codes, cand)
    assert (ids[:, 1] == -np.inf).all() and (ids[:, 2] == -np.inf).all() and np.array_equal(_bits(ids[:, 3]), _bits(ids[:, 0]))
    ok = (cand >= 0) & (cand < ic.SCAN_N)
    assert np.array_equal(_bits(ids[ok]), _bits(got[np.nonzero(ok)[0], cand[ok]]))
    coarse2 = coarse.copy()
    coarse2[::9], coarse2[1::9] = 0xFFFF, K
    foreign = ir.full_scores(lut, cdot, coarse2, codes)
    assert (foreign[:, ::9] == -np.inf).all() and (foreign[:, 1::9] == -np.inf).all()
    keep = np.ones(ic.SCAN_N, bool)
    keep[::9] = keep[1::9] = False
    assert np.array_equal(_bits(foreign[:, keep]), _bits(got[:, keep]))


def test_reference_residual_and_update_against_float64():
    r = ic.rng(11)
    T, K, E = 300, 5, 12
    x, cent = r.standard_normal((T, E)).astype(np.float32), r.standard_normal((K, E)).astype(np.float32)
    coarse = r.integers(0, K, size=T).astype(np.uint16)
    coarse[coarse == 3] = 2                                   # an empty cluster
    coarse[::11] = 0xFFFF
    res = ir.residual(x, cent, coarse)
    assert (res[::11] == 0).all()
    ok = coarse < K
    assert np.array_equal(res[ok], (x[ok] - cent[coarse[ok]]).astype(np.float32))
    out, counts = ir.coarse_update(x, coarse, cent, lambda a: a)
    assert counts[3] == 0 and np.array_equal(_bits(out[3]), _bits(cent[3])) and counts.sum() == ok.sum()
    for k in (0, 1, 2, 4):
        want = x[coarse == k].astype(np.float64).mean(axis=0)
        assert np.abs(out[k] - want).max() <= 64 * 2.0 ** -24 * np.abs(x[coarse == k]).sum(axis=0).max()
    b16 = lambda a: rounded(a, torch.bfloat16).astype(np.float32)                       # noqa: E731
    out16, _ = ir.coarse_update(b16(x), coarse, b16(cent), b16)
    assert np.array_equal(out16, b16(out16)) and not np.array_equal(out16, out)


def test_planted_corpus_conditions_hold_for_the_reference():
    p = ic.planted()
    cent, cb, docs, q = p["cent"], p["cb"], p["docs"], p["q"]
    K, N = len(cent), len(docs)
    assert (cent % 8 == 0).all() and np.abs(cent).max() <= 32 and len({tuple(c) for c in cent}) == K
    res = docs - cent[p["coarse"]]
    assert np.abs(res).max() <= 3
    for a in range(K):
        for b in range(a + 1, K):
            d = np.abs(cent[a] - cent[b])
            assert (d > 0).any() and d[d > 0].min() - 3 >= 5          # |residual| <= 3 < 5 <= what is left of a differing coordinate
    gap, most = ir.gap(docs, cent)
    assert gap > 0 and np.array_equal(ir.assign(docs, cent), p["coarse"])
    coarse, codes = ir.encode(docs, cent, cb)
    assert np.array_equal(coarse, p["coarse"]) and np.array_equal(codes, p["codes"])
    assert np.array_equal(ir.decode(coarse, codes, cent, cb), docs)
    for a in (cent, cb, docs, q):                                     # exact in bf16
        assert np.array_equal(rounded(a, torch.bfloat16), a.astype(np.float64))
    exact = q.astype(np.float64) @ docs.astype(np.float64).T
    cdot = (q.astype(np.float64) @ cent.astype(np.float64).T).astype(np.float32)
    s = ir.full_scores(pr.lut(q, cb), cdot, coarse, codes)
    assert np.array_equal(s.astype(np.float64), exact) and np.abs(exact).max() < 2 ** 24
    ties = [N - len(np.unique(row)) for row in exact]
    assert min(ties) > 50, ties
    # nprobe = 2: the reference's restricted top-k returns documents of the two best lists only, and fewer than all
    pro = ir.probes(cdot, 2)
    val, idx = sr.topk(ir.probed(s, coarse, pro), 100)
    for b in range(len(q)):
        assert set(coarse[idx[b][idx[b] >= 0]].tolist()) <= set(pro[b].tolist())
        assert cdot[b, pro[b, 0]] >= cdot[b, pro[b, 1]] >= np.delete(cdot[b], pro[b]).max()
    print(f"[ivfpq] planted corpus: assignment gap {gap:.1f} of max |sim| {most:.1f}; encode returns the planted codes; scores equal "
          f"float64 exactly; tied scores per query {ties}")


@pytest.mark.parametrize("mode", ["f32", "bf16"])
def test_fit_case_keeps_every_assignment_away_from_a_tie(mode):
    """The condition of the GPU test of fit_ivfpq: at every assignment of the reference loop the smallest gap between the best
    and the second-best similarity exceeds 1e-2 * max |similarity|, so the rounding of the f32 GEMM cannot move a code."""
    f, c = ic.FIT, ic.fit_case()
    dt = {"f32": torch.float32, "bf16": torch.bfloat16}[mode]
    rt = lambda a: rounded(a, dt).astype(np.float32)                  # noqa: E731
    x = rt(c["docs"])[c["rows"]]
    assert len({int(v) for v in c["label"][c["rows"][:f["K"]]]}) == f["K"]
    cent = x[:f["K"]].copy()
    worst = np.inf
    for it in range(max(f["iters"]) + 1):
        gap, most = ir.gap(x, cent)
        worst = min(worst, gap / most)
        assert gap > 1e-2 * most, (it, gap, most)
        coarse = ir.assign(x, cent)
        assert np.array_equal(coarse, c["label"][c["rows"]])           # centroid i starts in cluster i and stays there
        cent, counts = ir.coarse_update(x, coarse, cent, rt)
        assert counts.min() > 0
    for iters in f["iters"]:
        cent_i, cb = ir.fit(x, f["K"], f["m"], f["ksub"], iters, f["pq_iters"], rt)
        assert cent_i.shape == (f["K"], f["E"]) and cb.shape == (f["m"], f["ksub"], f["E"] // f["m"])
        assert np.array_equal(cent_i, rt(cent_i))
    print(f"[ivfpq] fit case {mode}: smallest (best - second best) / max |sim| over {max(f['iters']) + 1} assignments = {worst:.3f}")


# ---------------------------------------------------------------- IVFPQCodec and the index without a device
def test_ivfpq_codec_validates_its_parts():
    from polus_amd.ir.search import IVFPQCodec, PQCodec
    import polus.ir.search as alias
    assert alias.IVFPQCodec is IVFPQCodec and callable(alias.CorpusIndex.fit_ivfpq)
    cent = np.arange(5 * 32, dtype=np.float32).reshape(5, 32) / 7
    c = IVFPQCodec(cent, np.zeros((8, 16, 4), np.float32))
    assert (c.K, c.m, c.ksub, c.dsub, c.E) == (5, 8, 16, 4, 32) and c.codebooks.dtype == torch.float32
    assert not isinstance(c, PQCodec)
    assert c.half_norms.dtype == torch.float32 and np.array_equal(c.half_norms.numpy(), ir.half_norms(cent))
    assert IVFPQCodec(torch.zeros((1, 4), dtype=torch.bfloat16), torch.zeros((4, 1, 1))).K == 1
    for shape in ((6, 16, 4), (8, 257, 4), (8, 16, 33), (8, 16)):
        with pytest.raises(ValueError, match="codebooks"):
            IVFPQCodec(cent, np.zeros(shape, np.float32))
    for bad in (np.zeros((0, 32), np.float32), np.zeros((65536, 32), np.float32), np.zeros((32,), np.float32),
                np.zeros((5, 32), np.int32)):
        with pytest.raises(ValueError, match="centroids must be"):
            IVFPQCodec(bad, np.zeros((8, 16, 4), np.float32))
    with pytest.raises(ValueError, match="centroids have 31 features"):
        IVFPQCodec(np.zeros((5, 31), np.float32), np.zeros((8, 16, 4), np.float32))


def test_storage_codec_and_nprobe_pairing():
    from polus_amd.ir.search import CorpusIndex, IVFPQCodec, PQCodec
    pq = PQCodec(np.zeros((8, 16, 4), np.float32))
    ivf = IVFPQCodec(np.zeros((5, 32), np.float32), np.zeros((8, 16, 4), np.float32))
    for kw in (dict(storage="ivfpq"), dict(codec=ivf), dict(storage="fp8", codec=ivf)):
        with pytest.raises(ValueError, match="needs a codec"):
            CorpusIndex(None, object(), **kw)
    with pytest.raises(ValueError, match="must be a IVFPQCodec"):
        CorpusIndex(None, object(), storage="ivfpq", codec=pq)
    with pytest.raises(ValueError, match="must be a PQCodec"):
        CorpusIndex(None, object(), storage="pq", codec=ivf)
    for kw in (dict(), dict(storage="pq", codec=pq), dict(storage="fp8")):
        with pytest.raises(ValueError, match="nprobe belongs to storage='ivfpq'"):
            CorpusIndex(None, object(), nprobe=2, **kw)
    for bad in (0, 6, -1):
        with pytest.raises(ValueError, match=r"need 1 <= nprobe <= min\(K, 1024\) = 5"):
            CorpusIndex(None, object(), storage="ivfpq", codec=ivf, nprobe=bad)
    ix = CorpusIndex(None, object(), storage="ivfpq", codec=ivf, nprobe=5)
    assert ix.nprobe == 5 and CorpusIndex(None, object(), storage="ivfpq", codec=ivf).nprobe is None
    assert len(ix) == 0 and ix.nbytes == 0 and ix.pq_codes is None and ix.coarse_codes is None and ix.representations is None
    assert ix.lists is None and ix.centroids is ivf.centroids and CorpusIndex(None, object()).coarse_codes is None
    for call in (lambda: ix.search({}, 3), lambda: ix.search({}, 3, nprobe=2), lambda: ix.fit_ivfpq(4, 8), lambda: ix.fit_pq(8),
                 lambda: ix.rerank({}, [[0]], 1), lambda: ix.fit_centroids(4), lambda: ix.search_pruned({}, 3, 10),
                 lambda: ix.probe({}, 2), lambda: ix.refresh_lists()):
        with pytest.raises(ValueError, match="empty"):
            call()
    with pytest.raises(ValueError, match="nprobe belongs to storage='ivfpq'"):
        CorpusIndex(None, object()).search({}, 3, nprobe=2)
    ix._n, ix.tokens = 5, False
    for call in (lambda: ix.fit_centroids(4), lambda: ix.set_centroids(np.zeros((4, 32), np.float32)), lambda: ix.rerank({}, [[0]], 1),
                 lambda: ix.search_pruned({}, 3, 10), lambda: ix.search_pruned({}, 3, 10, nprobe=2), lambda: ix.probe({}, 2)):
        with pytest.raises(ValueError, match=r"\[CLS\]"):
            call()
    for call in (lambda: ix.fit_pq(8), lambda: ix.fit_ivfpq(4, 8)):
        with pytest.raises(ValueError, match="plain \\[CLS\\] index"):
            call()


def test_fit_ivfpq_refusals():
    from polus_amd.ir.search import CorpusIndex
    ix = CorpusIndex(None, object())
    with pytest.raises(ValueError, match="empty"):
        ix.fit_ivfpq(4, 8)
    ix._n, ix.tokens = 40, True
    with pytest.raises(ValueError, match="fit_ivfpq trains on a plain \\[CLS\\] index"):
        ix.fit_ivfpq(4, 8)
    ix.tokens = False
    ix._reps = torch.zeros((64, 48))
    for m, ksub, msg in ((6, 16, "multiple of 4"), (8, 257, "ksub <= 256"), (32, 16, "must divide")):
        with pytest.raises(ValueError, match=msg):
            ix.fit_ivfpq(4, m, ksub)
    for K in (0, 65536):
        with pytest.raises(ValueError, match="need 1 <= K <= 65535 centroids"):
            ix.fit_ivfpq(K, 8, 16)
    with pytest.raises(ValueError, match=r"max\(K, ksub\) = 41"):
        ix.fit_ivfpq(41, 8, 16)
    with pytest.raises(ValueError, match=r"max\(K, ksub\) = 41"):
        ix.fit_ivfpq(4, 8, 41)
    with pytest.raises(ValueError, match=r"max\(K, ksub\) = 16"):
        ix.fit_ivfpq(4, 8, 16, sample=15)


# ---------------------------------------------------------------- the route and the binding
def test_route_at_the_edges(lib):
    from polus_amd import ops
    out = (ctypes.c_int * 2)()
    assert lib.polus_ivfpq_scores_ids_route(1, 1, 160, 256, out) == 0 and (out[0], out[1]) == (LDS_BYTES, 1)
    for m in range(4, 161, 4):
        for Q, C in ((1, 1), (1, 255), (1, 65535), (64, 1000), (65535, 65535)):
            nbytes, cols = ops.ivfpq_scores_ids_route(Q, C, m, 256)
            assert nbytes == m * 1024 <= LDS_BYTES                     # one table per workgroup, whatever Q
            assert cols == C if C <= 256 else (256 <= cols <= C and cols % 64 == 0 or cols == C)
    assert ops.ivfpq_scores_ids_route(5, 1000, 16, 1) == ops.ivfpq_scores_ids_route(5, 1000, 16, 256)   # ksub does not move it
    for m in (164, 6, 0, 2):
        assert lib.polus_ivfpq_scores_ids_route(1, 1, m, 256, out) != 0 and b"multiple of 4" in lib.polus_last_error(), m


def test_new_symbols_are_declared_and_bound():
    from polus_amd import _lib, ops
    txt = open(os.path.join(ROOT, "include", "polus_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    for name in NEW:
        assert re.search(r"\bint\s+%s\s*\(" % name, code), name
        assert name in _lib.SIGNATURES, name
        n_args = len(re.search(r"%s\s*\((.*?)\)" % name, code, flags=re.S).group(1).split(","))
        assert n_args == len(_lib.SIGNATURES[name][1]), name
        assert callable(getattr(ops, name[len("polus_"):]))


def test_entry_points_refuse_on_the_host(lib):
    p, p2 = ctypes.c_void_p(256), ctypes.c_void_p(1 << 20)
    out = (ctypes.c_int * 2)()

    def err(rc, name):
        assert rc != 0
        msg = lib.polus_last_error()
        assert name in msg, msg
        return msg

    def sc(lut=p, cdot=p, ldd=7, coarse=p, codes=p, ldc=8, cand=p, ldcand=4, score=p, lds=4, Q=1, C=4, N=9, m=8, ksub=16, K=7):
        return err(lib.polus_ivfpq_scores_ids(lut, cdot, ldd, coarse, codes, ldc, cand, ldcand, score, lds, Q, C, N, m, ksub, K, None),
                   b"polus_ivfpq_scores_ids")

    def route(Q=1, C=1, m=8, ksub=16, o=out):
        return err(lib.polus_ivfpq_scores_ids_route(Q, C, m, ksub, o), b"polus_ivfpq_scores_ids_route")

    def res(dtype=0, x=p, ldx=32, cent=p, coarse=p, r=p, ldr=32, rows=1, K=7, E=32):
        return err(lib.polus_ivfpq_residual(dtype, x, ldx, cent, coarse, r, ldr, rows, K, E, None), b"polus_ivfpq_residual")

    def upd(dtype=0, x=p, ldx=32, coarse=p, prev=p, o=p2, counts=p, T=1, K=7, E=32):
        return err(lib.polus_ivfpq_coarse_update(dtype, x, ldx, coarse, prev, o, counts, T, K, E, None), b"polus_ivfpq_coarse_update")

    for call in (sc, route):
        for m in (0, 6, 164):
            assert b"multiple of 4 in [4, 160]" in call(m=m)
        assert b"ksub <= 256" in call(ksub=0) and b"ksub <= 256" in call(ksub=257)
        assert b"Q <= 65535" in call(Q=0) and b"Q <= 65535" in call(Q=65536)
        assert b"C <= 65535" in call(C=0) and b"C <= 65535" in call(C=65536)
    assert b"null pointer" in route(o=None)
    for call in (sc, res, upd):
        assert b"K <= 65535" in call(K=0) and b"K <= 65535" in call(K=65536)
    assert b"N >= 1" in sc(N=0)
    assert b"C must be N" in sc(cand=None) and b"null pointer" in sc(cand=None, C=9, lds=9, score=None)
    assert b"ldd must be >= K" in sc(ldd=6) and b"ldc must be >= m" in sc(ldc=7)
    assert b"ldcand must be >= C" in sc(ldcand=3) and b"lds must be >= C" in sc(lds=3)
    for call in (res, upd):
        assert b"unknown dtype" in call(dtype=2)
        assert b"E <= 5120" in call(E=0, ldx=0) and b"E <= 5120" in call(E=5121, ldx=5121)
        assert b"ldx must be >= E" in call(ldx=31)
    assert b"rows >= 1" in res(rows=0) and b"ldr must be >= E" in res(ldr=31) and b"T >= 1" in upd(T=0)
    assert b"must not overlap" in upd(o=p) and b"must not overlap" in upd(o=ctypes.c_void_p(256 + 7 * 32 * 4 - 4))
    for call, names in ((sc, ("lut", "cdot", "coarse", "codes", "score")), (res, ("x", "cent", "coarse", "r")),
                        (upd, ("x", "coarse", "prev", "o", "counts"))):
        for name in names:
            assert b"null pointer" in call(**{name: None}), (call, name)


def test_wrappers_refuse_what_the_kernels_would_misread():
    """Host tensors reach the shared device check; everything else is refused before it, by name."""
    from polus_amd import ops
    from polus_amd._lib import PolusHipError
    with pytest.raises(PolusHipError, match="device"):
        ops.ivfpq_residual(torch.zeros((5, 32)), torch.zeros((7, 32)), torch.zeros(5, dtype=torch.int16), torch.zeros((5, 32)))

    class D:
        """A host tensor that claims to be on the device (tests/test_pq_cpu.py): a call that passed every check would fail
        loudly in ptr()."""

        def __init__(self, t):
            self.t = t

        is_cuda = True

        def __getattr__(self, name):
            return getattr(self.t, name)

        def data_ptr(self):
            raise AssertionError("reached the entry point")

    x, cent, co, r = torch.zeros((5, 32)), torch.zeros((7, 32)), torch.zeros(5, dtype=torch.int16), torch.zeros((5, 32))
    lut, cdot, codes = torch.zeros((2, 8, 16)), torch.zeros((2, 7)), torch.zeros((9, 8), dtype=torch.uint8)
    co9, cand, score = torch.zeros(9, dtype=torch.int16), torch.zeros((2, 4), dtype=torch.int32), torch.zeros((2, 4))
    cnt = torch.zeros(7, dtype=torch.int32)

    def scan(lut=lut, cdot=cdot, coarse=co9, codes=codes, cand=cand, score=score):
        return lambda: ops.ivfpq_scores_ids(D(lut), D(cdot), D(coarse), D(codes), None if cand is None else D(cand), D(score))

    bad = [
        ("ivfpq_residual: x", lambda: ops.ivfpq_residual(D(x.double()), D(cent), D(co), D(r))),
        ("ivfpq_residual: x", lambda: ops.ivfpq_residual(D(x[:, :31]), D(cent), D(co), D(r))),
        ("ivfpq_residual: x", lambda: ops.ivfpq_residual(D(torch.zeros((5, 64))[:, ::2]), D(cent), D(co), D(r))),
        ("ivfpq_residual: cent", lambda: ops.ivfpq_residual(D(x), D(cent.bfloat16()), D(co), D(r))),
        ("ivfpq_residual: cent", lambda: ops.ivfpq_residual(D(x), D(torch.zeros((7, 64))[:, :32]), D(co), D(r))),
        ("ivfpq_residual: coarse", lambda: ops.ivfpq_residual(D(x), D(cent), D(co.int()), D(r))),
        ("ivfpq_residual: coarse", lambda: ops.ivfpq_residual(D(x), D(cent), D(co[:4]), D(r))),
        ("ivfpq_residual: coarse", lambda: ops.ivfpq_residual(D(x), D(cent), D(torch.zeros(10, dtype=torch.int16)[::2]), D(r))),
        ("ivfpq_residual: r", lambda: ops.ivfpq_residual(D(x), D(cent), D(co), D(r.bfloat16()))),
        ("ivfpq_residual: r", lambda: ops.ivfpq_residual(D(x), D(cent), D(co), D(torch.zeros((4, 32))))),
        ("ivfpq_coarse_update: x", lambda: ops.ivfpq_coarse_update(D(x.half()), D(co), D(cent), D(cent.clone()), D(cnt))),
        ("ivfpq_coarse_update: prev", lambda: ops.ivfpq_coarse_update(D(x), D(co), D(cent.bfloat16()), D(cent.clone()), D(cnt))),
        ("ivfpq_coarse_update: out", lambda: ops.ivfpq_coarse_update(D(x), D(co), D(cent), D(torch.zeros((6, 32))), D(cnt))),
        ("ivfpq_coarse_update: coarse", lambda: ops.ivfpq_coarse_update(D(x), D(co[:4]), D(cent), D(cent.clone()), D(cnt))),
        ("ivfpq_coarse_update: counts", lambda: ops.ivfpq_coarse_update(D(x), D(co), D(cent), D(cent.clone()), D(cnt.long()))),
        ("ivfpq_scores_ids: lut", scan(lut=lut.double())),
        ("ivfpq_scores_ids: lut", scan(lut=torch.zeros((2, 6, 16)), codes=codes[:, :6])),
        ("ivfpq_scores_ids: codes", scan(codes=codes[:, :7])),
        ("ivfpq_scores_ids: cdot", scan(cdot=cdot.double())),
        ("ivfpq_scores_ids: cdot", scan(cdot=torch.zeros((3, 7)))),
        ("ivfpq_scores_ids: cdot", scan(cdot=torch.zeros((2, 14))[:, ::2])),
        ("ivfpq_scores_ids: coarse", scan(coarse=co)),
        ("ivfpq_scores_ids: cand", scan(cand=cand.long())),
        ("ivfpq_scores_ids: cand", scan(cand=torch.zeros((3, 4), dtype=torch.int32))),
        ("ivfpq_scores_ids: cand", scan(cand=torch.zeros((2, 8), dtype=torch.int32)[:, ::2])),
        ("ivfpq_scores_ids: cand", scan(cand=torch.zeros((2, 65536), dtype=torch.int32), score=torch.zeros((2, 65536)))),
        ("ivfpq_scores_ids: score", scan(score=torch.zeros((2, 3)))),
        ("ivfpq_scores_ids: score", scan(cand=None)),                                            # C = N = 9 without cand
        ("ivfpq_scores_ids: score", scan(score=torch.zeros((2, 8))[:, ::2])),
    ]
    for start, call in bad:
        with pytest.raises(AssertionError) as e:
            call()
        assert str(e.value).startswith(start), (start, str(e.value))
    with pytest.raises(AssertionError, match="reached the entry point"):                        # what is right passes every check
        scan()()
