"""CPU: the NumPy restatement of the product-quantisation rules (tests/pq_ref.py) against float64 on the planted corpus and
its invariance to chunking; PQCodec and fit_pq refusals and the sampling rule; the route of polus_pq_scores at its edges; the
new symbols in the binding; and the host-side refusals of every polus_pq_* entry point (no launch is made without a GPU)."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from tests import pq_cases as pc
from tests import pq_ref as pr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("polus_pq_encode", "polus_pq_update", "polus_pq_decode", "polus_pq_lut", "polus_pq_scores", "polus_pq_scores_route")
LDS_BYTES = 160 * 1024


@pytest.fixture(scope="module")
def lib():
    from polus_amd import build
    build.build(verbose=False)
    from polus_amd import _lib
    return _lib.load()


# ---------------------------------------------------------------- the reference itself
def test_reference_is_exact_on_the_planted_corpus():
    p = pc.planted()
    assert np.array_equal(pr.encode(p["docs"], p["cb"]), p["codes"])
    assert np.array_equal(pr.decode(p["codes"], p["cb"]), p["docs"])
    s = pr.scores(pr.lut(p["q"], p["cb"]), p["codes"])
    exact = p["q"].astype(np.float64) @ p["docs"].astype(np.float64).T
    assert np.array_equal(s.astype(np.float64), exact)
    ties = [len(row) - len(np.unique(row)) for row in s]
    assert min(ties) > 100, ties                             # the tie-to-lower-id rule of a search is exercised
    print(f"[pq] planted corpus: encode returns the planted codes, scores equal float64 exactly; tied scores per query {ties}")


def test_reference_does_not_depend_on_the_chunking():
    table, codes = pc.scan_case(20, 16, 3, 1000)
    codes[5, 3], table[1, 2, 7], table[2, 0, 1] = 200, np.nan, -np.inf
    whole = pr.scores(table, codes)
    parts = np.concatenate([pr.scores(table, codes[a:b]) for a, b in ((0, 1), (1, 640), (640, 1000))], axis=1)
    assert np.array_equal(whole.view(np.int32), parts.view(np.int32))
    one = np.concatenate([pr.scores(table[b:b + 1], codes) for b in range(3)])
    assert np.array_equal(whole.view(np.int32), one.view(np.int32))
    assert (whole[:, 5] == -np.inf).all() and np.isnan(whole[1]).any() and not np.isnan(whole[0]).any()


def test_reference_lloyd_rounds_lower_the_distortion():
    x = pc.rng(3).standard_normal((300, 32)).astype(np.float32)
    cb = np.ascontiguousarray(x[:16].reshape(16, 8, 4).transpose(1, 0, 2))
    errs = []
    for _ in range(4):
        codes = pr.encode(x, cb)
        cb, counts = pr.update(x, codes, cb)
        assert counts.sum() == 300 * 8
        errs.append(float(((x.astype(np.float64) - pr.decode(pr.encode(x, cb), cb)) ** 2).sum()))
    assert errs == sorted(errs, reverse=True) and errs[-1] < errs[0], errs
    assert np.array_equal(pr.fit(x, 8, 16, 4).view(np.int32), cb.view(np.int32))


# ---------------------------------------------------------------- PQCodec, fit_pq, the index without a device
def test_pq_codec_validates_its_codebooks():
    from polus_amd.ir.search import PQCodec
    import polus.ir.search as alias
    assert alias.PQCodec is PQCodec and callable(alias.CorpusIndex.fit_pq)
    c = PQCodec(np.zeros((8, 16, 4), np.float32))
    assert (c.m, c.ksub, c.dsub, c.E) == (8, 16, 4, 32) and c.codebooks.dtype == torch.float32
    assert PQCodec(torch.zeros((160, 256, 32))).E == 5120 and PQCodec(torch.zeros((4, 1, 1))).E == 4
    for shape in ((6, 16, 4), (164, 16, 4), (0, 16, 4), (8, 257, 4), (8, 0, 4), (8, 16, 33), (8, 16, 0), (8, 16), (8, 16, 4, 1)):
        with pytest.raises(ValueError, match="codebooks"):
            PQCodec(np.zeros(shape, np.float32))
    with pytest.raises(ValueError, match="codebooks must be f32"):
        PQCodec(np.zeros((8, 16, 4), np.float64))


def test_storage_and_codec_pairing():
    from polus_amd.ir.search import CorpusIndex, PQCodec, ResidualCodec
    from polus_amd.ir.training import MaxSimScores
    pq = PQCodec(np.zeros((8, 16, 4), np.float32))
    res = ResidualCodec(torch.zeros((5, 64)), [0.0], [-1.0, 1.0], 1)
    with pytest.raises(ValueError, match="^storage must be None or 'fp8'"):
        CorpusIndex(None, object(), storage="opq")
    for kw in (dict(storage="pq"), dict(codec=pq), dict(storage="fp8", codec=pq)):
        with pytest.raises(ValueError, match="needs a codec"):
            CorpusIndex(None, object(), **kw)
    with pytest.raises(ValueError, match="must be a PQCodec"):
        CorpusIndex(None, object(), storage="pq", codec=res)
    with pytest.raises(ValueError, match="must be a ResidualCodec"):
        CorpusIndex(None, MaxSimScores(normalize=True), storage="residual", codec=pq)
    ix = CorpusIndex(None, object(), storage="pq", codec=pq)
    assert len(ix) == 0 and ix.nbytes == 0 and ix.pq_codes is None and ix.representations is None and ix.codes is None
    assert ix.centroids is None and CorpusIndex(None, object()).pq_codes is None
    for call in (lambda: ix.search({}, 3), lambda: ix.fit_pq(8), lambda: ix.rerank({}, [[0]], 1), lambda: ix.fit_centroids(4)):
        with pytest.raises(ValueError, match="empty"):
            call()
    ix._n, ix.tokens = 5, False
    with pytest.raises(ValueError, match=r"\[CLS\]"):           # keyed on the storage, not on "has a codec"
        ix.fit_centroids(4)
    with pytest.raises(ValueError, match=r"\[CLS\]"):
        ix.rerank({}, [[0]], 1)
    with pytest.raises(ValueError, match="needs centroids"):
        ix.search_pruned({}, 3, 10)
    with pytest.raises(ValueError, match="plain \\[CLS\\] index"):
        ix.fit_pq(8)


def test_fit_pq_refusals_and_the_sampling_rule():
    from polus_amd.ir.search import CorpusIndex
    ix = CorpusIndex(None, object())
    with pytest.raises(ValueError, match="empty"):
        ix.fit_pq(8)
    ix._n, ix.tokens = 40, True
    with pytest.raises(ValueError, match="plain \\[CLS\\] index"):
        ix.fit_pq(8)
    ix.tokens = False
    ix._reps = torch.zeros((64, 48))
    for m, ksub, msg in ((6, 16, "multiple of 4"), (164, 16, "multiple of 4"), (8, 257, "ksub <= 256"), (8, 0, "ksub <= 256"),
                         (32, 16, "must divide"), (20, 16, "must divide")):
        with pytest.raises(ValueError, match=msg):
            ix.fit_pq(m, ksub)
    ix._reps = torch.zeros((64, 4 * 33))
    with pytest.raises(ValueError, match="at most 32"):
        ix.fit_pq(4, 16)
    ix._reps = torch.zeros((64, 48))
    with pytest.raises(ValueError, match="at least as many sampled documents"):
        ix.fit_pq(8, 41)
    with pytest.raises(ValueError, match="at least as many sampled documents"):
        ix.fit_pq(8, 16, sample=15)
    # the rule: a permutation of everything while it fits the sample, a choice without replacement beyond; seed and N only
    for N, sample, seed in ((40, 40, 0), (40, 1 << 16, 3), (1000, 64, 3), (41, 40, 9)):
        ix._n = N
        r = np.random.Generator(np.random.PCG64(seed))
        want = r.permutation(N) if N <= sample else r.choice(N, size=sample, replace=False)
        got = ix._sample_rows(sample, seed)
        assert np.array_equal(got, want) and np.array_equal(got, pr.sample_rows(N, sample, seed))
        assert len(got) == min(N, sample) and len(set(got.tolist())) == len(got)


# ---------------------------------------------------------------- the route
def test_route_at_the_edges(lib):
    from polus_amd import ops
    out = (ctypes.c_int * 2)()
    assert lib.polus_pq_scores_route(1, 1, 160, 256, out) == 0 and (out[0], out[1]) == (1, LDS_BYTES)
    assert ops.pq_scores_route(64, 65535, 160, 256) == (1, LDS_BYTES)
    for m in (164, 6, 0, 2):
        assert lib.polus_pq_scores_route(1, 1, m, 256, out) != 0 and b"multiple of 4" in lib.polus_last_error(), m
    for Q in (1, 2, 3, 4, 5, 64):
        qts = []
        for m in range(4, 161, 4):
            qt, nbytes = ops.pq_scores_route(Q, 1000, m, 256)
            assert qt in (1, 2, 4) and qt <= Q and nbytes == qt * m * 1024 <= LDS_BYTES
            assert qt == 4 or 2 * qt > Q or 2 * qt * m * 1024 > LDS_BYTES         # the largest that fits
            qts.append(qt)
        assert qts == sorted(qts, reverse=True), (Q, qts)      # qt shrinks as m grows
    assert [ops.pq_scores_route(64, 1000, m, 256).qt for m in (24, 40, 44, 48, 80, 84, 96)] == [4, 4, 2, 2, 2, 1, 1]
    # ksub and N do not move it: a function of Q, m and the LDS budget
    assert ops.pq_scores_route(5, 1, 16, 1) == ops.pq_scores_route(5, 65535, 16, 256) == (4, 65536)


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


# ---------------------------------------------------------------- host-side refusals of the entry points
def test_entry_points_refuse_on_the_host(lib):
    p = ctypes.c_void_p(256)
    out = (ctypes.c_int * 2)()

    def err(rc, name):
        assert rc != 0
        msg = lib.polus_last_error()
        assert name in msg, msg
        return msg

    def enc(dtype=0, x=p, ldx=32, cb=p, codes=p, ldc=8, rows=1, m=8, ksub=16, dsub=4):
        return err(lib.polus_pq_encode(dtype, x, ldx, cb, codes, ldc, rows, m, ksub, dsub, None), b"polus_pq_encode")

    def upd(dtype=0, x=p, ldx=32, codes=p, ldc=8, prev=p, o=ctypes.c_void_p(4096), counts=p, T=1, m=8, ksub=16, dsub=4):
        return err(lib.polus_pq_update(dtype, x, ldx, codes, ldc, prev, o, counts, T, m, ksub, dsub, None), b"polus_pq_update")

    def dec(codes=p, ldc=8, cb=p, dtype=0, y=p, ldy=32, rows=1, m=8, ksub=16, dsub=4):
        return err(lib.polus_pq_decode(codes, ldc, cb, dtype, y, ldy, rows, m, ksub, dsub, None), b"polus_pq_decode")

    def lut(dtype=0, q=p, ldq=32, cb=p, t=p, Q=1, m=8, ksub=16, dsub=4):
        return err(lib.polus_pq_lut(dtype, q, ldq, cb, t, Q, m, ksub, dsub, None), b"polus_pq_lut")

    def sc(t=p, codes=p, ldc=8, score=p, lds=1, Q=1, N=1, m=8, ksub=16):
        return err(lib.polus_pq_scores(t, codes, ldc, score, lds, Q, N, m, ksub, None), b"polus_pq_scores")

    def route(Q=1, N=1, m=8, ksub=16, o=out):
        return err(lib.polus_pq_scores_route(Q, N, m, ksub, o), b"polus_pq_scores_route")

    for call in (enc, upd, dec, lut):
        assert b"unknown dtype" in call(dtype=2)
        for m in (0, 6, 164):
            assert b"multiple of 4 in [4, 160]" in call(m=m)
        assert b"ksub <= 256" in call(ksub=0) and b"ksub <= 256" in call(ksub=257)
        assert b"dsub <= 32" in call(dsub=0) and b"dsub <= 32" in call(dsub=33)
    for call in (sc, route):
        for m in (0, 6, 164):
            assert b"multiple of 4 in [4, 160]" in call(m=m)
        assert b"ksub <= 256" in call(ksub=0) and b"ksub <= 256" in call(ksub=257)
        assert b"Q <= 65535" in call(Q=0) and b"Q <= 65535" in call(Q=65536)
        assert b"N <= 65535" in call(N=0) and b"N <= 65535" in call(N=65536)
    assert b"null pointer" in route(o=None)
    assert b"rows >= 1" in enc(rows=0) and b"rows >= 1" in dec(rows=0) and b"T >= 1" in upd(T=0) and b"Q >= 1" in lut(Q=0)
    assert b"ldx must be >= m*dsub" in enc(ldx=31) and b"ldx must be >= m*dsub" in upd(ldx=31)
    assert b"ldy must be >= m*dsub" in dec(ldy=31) and b"ldq must be >= m*dsub" in lut(ldq=31)
    assert b"ldc must be >= m" in enc(ldc=7) and b"ldc must be >= m" in upd(ldc=7) and b"ldc must be >= m" in dec(ldc=7)
    assert b"ldc must be >= m" in sc(ldc=7) and b"lds must be >= N" in sc(N=4, lds=3)
    assert b"must not alias" in upd(o=p)
    for call, names in ((enc, ("x", "cb", "codes")), (upd, ("x", "codes", "prev", "o", "counts")), (dec, ("codes", "cb", "y")),
                        (lut, ("q", "cb", "t")), (sc, ("t", "codes", "score"))):
        for name in names:
            assert b"null pointer" in call(**{name: None}), (call, name)


def test_wrappers_refuse_what_the_kernels_would_misread():
    """Host tensors reach the shared device check; everything else is refused before it, by name."""
    from polus_amd import ops
    from polus_amd._lib import PolusHipError
    cb, x, codes = torch.zeros((8, 16, 4)), torch.zeros((5, 32)), torch.zeros((5, 8), dtype=torch.uint8)
    with pytest.raises(PolusHipError, match="device"):
        ops.pq_encode(x, cb, codes)

    class Dev:
        """A host tensor that claims to be on the device: the checks behind the device check can be reached on the CPU, and a
        call that passed them all would fail loudly in ptr()."""

        def __init__(self, t):
            self.t = t

        is_cuda = True

        def __getattr__(self, name):
            return getattr(self.t, name)

        def data_ptr(self):
            raise AssertionError("reached the entry point")

    D = Dev
    bad = [
        ("pq_encode: x", lambda: ops.pq_encode(D(x.double()), D(cb), D(codes))),
        ("pq_encode: x", lambda: ops.pq_encode(D(x[:, :31]), D(cb), D(codes))),
        ("pq_encode: x", lambda: ops.pq_encode(D(torch.zeros((5, 64))[:, ::2]), D(cb), D(codes))),
        ("pq_encode: codebook", lambda: ops.pq_encode(D(x), D(cb.double()), D(codes))),
        ("pq_encode: codebook", lambda: ops.pq_encode(D(x), D(torch.zeros((8, 16, 8))[:, :, ::2]), D(codes))),
        ("pq_encode: codebook", lambda: ops.pq_encode(D(torch.zeros((5, 24))), D(torch.zeros((6, 16, 4))), D(codes))),
        ("pq_encode: codes", lambda: ops.pq_encode(D(x), D(cb), D(codes.to(torch.int8)))),
        ("pq_encode: codes", lambda: ops.pq_encode(D(x), D(cb), D(codes[:4]))),
        ("pq_encode: codes", lambda: ops.pq_encode(D(x), D(cb), D(codes[:, :7]))),
        ("pq_decode: y", lambda: ops.pq_decode(D(codes), D(cb), D(torch.zeros((5, 31))))),
        ("pq_decode: y", lambda: ops.pq_decode(D(codes), D(cb), D(torch.zeros((5, 32), dtype=torch.float16)))),
        ("pq_decode: codes", lambda: ops.pq_decode(D(torch.zeros((5, 16), dtype=torch.uint8)[:, ::2]), D(cb), D(x))),
        ("pq_lut: lut", lambda: ops.pq_lut(D(x), D(cb), D(torch.zeros((5, 8, 15))))),
        ("pq_lut: lut", lambda: ops.pq_lut(D(x), D(cb), D(torch.zeros((5, 8, 32))[:, :, ::2]))),
        ("pq_lut: q", lambda: ops.pq_lut(D(x.to(torch.float16)), D(cb), D(torch.zeros((5, 8, 16))))),
        ("pq_update: out", lambda: ops.pq_update(D(x), D(codes), D(cb), D(torch.zeros((8, 16, 3))), D(torch.zeros((8, 16), dtype=torch.int32)))),
        ("pq_update: counts", lambda: ops.pq_update(D(x), D(codes), D(cb), D(torch.zeros((8, 16, 4))), D(torch.zeros((8, 16), dtype=torch.int64)))),
        ("pq_update: codes", lambda: ops.pq_update(D(x), D(codes[:4]), D(cb), D(torch.zeros((8, 16, 4))), D(torch.zeros((8, 16), dtype=torch.int32)))),
        ("pq_scores: lut", lambda: ops.pq_scores(D(torch.zeros((2, 8, 16)).double()), D(codes), D(torch.zeros((2, 5))))),
        ("pq_scores: lut", lambda: ops.pq_scores(D(torch.zeros((2, 6, 16))), D(codes[:, :6]), D(torch.zeros((2, 5))))),
        ("pq_scores: codes", lambda: ops.pq_scores(D(torch.zeros((2, 8, 16))), D(codes[:, :7]), D(torch.zeros((2, 5))))),
        ("pq_scores: score", lambda: ops.pq_scores(D(torch.zeros((2, 8, 16))), D(codes), D(torch.zeros((2, 4))))),
        ("pq_scores: score", lambda: ops.pq_scores(D(torch.zeros((2, 8, 16))), D(codes), D(torch.zeros((2, 10))[:, ::2]))),
        ("pq_scores: score", lambda: ops.pq_scores(D(torch.zeros((2, 8, 16))), D(codes), D(torch.zeros((3, 5))))),
    ]
    for start, call in bad:
        with pytest.raises(AssertionError) as e:
            call()
        assert str(e.value).startswith(start), (start, str(e.value))
