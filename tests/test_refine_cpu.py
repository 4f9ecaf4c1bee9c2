"""CPU: the refine reference against float64, the refusals of CorpusIndex(refine=...), of the wrappers and of the C entry
points, and the bookkeeping of a refine store.  No kernel runs here."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from tests import fp8_ref
from tests import refine_cases as rc
from tests import refine_ref as rr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("polus_cls_rerank", "polus_cls_rerank_fp8", "polus_cls_fp8_quantize", "polus_cls_fp8_dequantize")


@pytest.fixture(scope="module")
def lib():
    from polus_amd import build
    build.build(verbose=False)
    from polus_amd import _lib
    return _lib.load()


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, np.float32)).view(np.int32)


# ---------------------------------------------------------------- the reference itself
@pytest.mark.parametrize("E", rc.ES)
def test_reference_against_float64(E):
    """|err| <= (8 ceil(E / 512) + 8) * 2^-24 * sum |q_e d_e| on N(0, 1) inputs (tests/refine_cases.err_bound)."""
    q, d = rc.gaussian(E)
    got = rr.scores(q, d).astype(np.float64)
    want = rr.exact(q, d)
    room = rc.err_bound(E) * 2.0 ** -24 * (np.abs(q.astype(np.float64)) @ np.abs(d.astype(np.float64)).T)
    worst = float((np.abs(got - want) / room).max())
    print(f"[refine] reference E={E}: worst |err| / bound = {worst:.3f}")
    assert worst <= 1.0


@pytest.mark.parametrize("E", rc.ES)
def test_reference_is_exact_on_the_summable_inputs(E):
    q, d = rc.summable(E)
    want = rr.exact(q, d)
    assert np.array_equal(rr.scores(q, d).astype(np.float64), want)
    assert np.array_equal(want.astype(np.float32).astype(np.float64), want)
    bf = lambda a: torch.as_tensor(a).to(torch.bfloat16).float().numpy()
    assert np.array_equal(bf(q), q) and np.array_equal(bf(d), d), "the inputs are exact in bf16"
    # and through the FP8 route: the quantiser loses nothing on them, a power-of-two scale commutes with the sum
    codes, scale = rr.quantize(d)
    assert np.array_equal(fp8_ref.dequantize(codes, scale), d)
    cand = rc.candidates(len(q), 7, len(d))
    full = rr.rerank(q, d, cand)
    assert np.array_equal(_bits(rr.rerank_fp8(q, codes, scale, cand)), _bits(full))
    ok = (cand >= 0) & (cand < len(d))
    assert np.isneginf(full[~ok]).all() and (~ok).sum() == 4 * len(q)
    assert np.array_equal(full[ok].astype(np.float64), np.take_along_axis(want, np.where(ok, cand, 0), 1)[ok])


def test_reference_depends_on_the_pair_only():
    q, d = rc.gaussian(768)
    whole = rr.scores(q, d)
    cand = rc.candidates(len(q), 257, len(d))
    got = rr.rerank(q, d, cand)
    ok = (cand >= 0) & (cand < len(d))
    assert np.array_equal(_bits(got[ok]), _bits(np.take_along_axis(whole, np.where(ok, cand, 0), 1)[ok]))
    assert np.array_equal(_bits(rr.rerank(q[2:3], d, cand[2:3, 9:10])), _bits(got[2:3, 9:10]))


def test_index_corpus_has_its_planted_ties():
    q, d = rc.index_corpus()
    s = rr.exact(q, d)
    assert np.array_equal(s[:, 11], s[:, 400]) and np.array_equal(s[:, 650], s[:, 3]) and d.shape == (700, rc.INDEX_E)


# ---------------------------------------------------------------- the index's constructor, bookkeeping and refusals
def _codecs():
    from polus_amd.ir.search import IVFPQCodec, PQCodec
    cb = np.zeros((8, 16, 4), np.float32)
    return PQCodec(cb), IVFPQCodec(np.zeros((5, 32), np.float32), cb)


def test_constructor_refusals():
    from polus_amd.ir.search import CorpusIndex, IVFPQCodec, PQCodec, ResidualCodec
    pq, ivf = _codecs()
    for bad in ("half", True, 8):
        with pytest.raises(ValueError, match="refine must be None or 'full' or 'fp8'"):
            CorpusIndex(None, object(), refine=bad)
    res = ResidualCodec(np.zeros((4, 32), np.float32), np.zeros(3, np.float32), np.zeros(4, np.float32), 2)
    norm = type("S", (), dict(normalize=True))()
    for kw, scorer in ((dict(storage="fp8"), object()), (dict(storage="residual", codec=res), norm)):
        for refine in ("full", "fp8"):
            with pytest.raises(ValueError, match="refine belongs to a \\[CLS\\] index"):
                CorpusIndex(None, scorer, refine=refine, **kw)
    with pytest.raises(ValueError, match="refine='fp8' belongs to storage='pq' or 'ivfpq'"):
        CorpusIndex(None, object(), refine="fp8")
    # a width the kernel does not take: m * dsub = 8 * 3 = 24, 40
    for codec, storage in ((PQCodec(np.zeros((8, 16, 3), np.float32)), "pq"),
                           (IVFPQCodec(np.zeros((5, 40), np.float32), np.zeros((8, 16, 5), np.float32)), "ivfpq")):
        for refine in ("full", "fp8"):
            with pytest.raises(ValueError, match="multiple of 16 features"):
                CorpusIndex(None, object(), storage=storage, codec=codec, refine=refine)
    for kw in (dict(), dict(storage="pq", codec=pq), dict(storage="ivfpq", codec=ivf), dict(storage="fp8"), dict(refine="full")):
        with pytest.raises(ValueError, match="candidates belongs to"):
            CorpusIndex(None, object(), candidates=100, **kw)
    for bad in (0, -1, 1025):
        with pytest.raises(ValueError, match="<= candidates <= 1024"):
            CorpusIndex(None, object(), storage="pq", codec=pq, refine="full", candidates=bad)
    ix = CorpusIndex(None, object(), storage="ivfpq", codec=ivf, refine="fp8", candidates=1024, nprobe=2)
    assert (ix.refine, ix.candidates, ix.nprobe) == ("fp8", 1024, 2)
    assert CorpusIndex(None, object(), storage="pq", codec=pq, refine="full").candidates is None
    assert CorpusIndex(None, object()).refine is None


def test_refine_on_a_token_index_and_a_bad_width_are_refused_at_the_first_add():
    from polus_amd.ir.models import TokenReps
    from polus_amd.ir.search import CorpusIndex

    class Model:
        def __init__(self, rep):
            self.rep = rep

        def encode_document(self, x, training=False):
            return self.rep

        def document_projection(self, rep, training=False):
            return rep

    tok = TokenReps(torch.zeros((2, 3, 32)), torch.ones((2, 3), dtype=torch.int32))
    with pytest.raises(ValueError, match="refine belongs to a \\[CLS\\] index"):
        CorpusIndex(Model(tok), object(), refine="full").add({})
    with pytest.raises(ValueError, match="multiple of 16 features.*E = 24"):
        CorpusIndex(Model(torch.zeros((2, 24))), object(), refine="full").add({})


def test_an_empty_index_with_a_refine_store():
    from polus_amd.ir.search import CorpusIndex
    pq, ivf = _codecs()
    for kw in (dict(refine="full"), dict(storage="pq", codec=pq, refine="full"), dict(storage="ivfpq", codec=ivf, refine="fp8")):
        ix = CorpusIndex(None, object(), **kw)
        assert len(ix) == 0 and ix.nbytes == 0
        assert ix.refine_vectors is None and ix.refine_codes is None and ix.refine_scales is None
        for call in (lambda: ix.rerank({}, [[0]], 1), lambda: ix.search({}, 3)):
            with pytest.raises(ValueError, match="empty"):
                call()
    plain = CorpusIndex(None, object())
    assert plain.refine_vectors is None and plain.refine_codes is None and plain.refine_scales is None


def test_rerank_without_a_refine_store_is_still_refused():
    from polus_amd.ir.search import CorpusIndex
    pq, ivf = _codecs()
    for kw in (dict(), dict(storage="pq", codec=pq), dict(storage="ivfpq", codec=ivf)):
        ix = CorpusIndex(None, object(), **kw)
        ix._n, ix.tokens = 5, False
        with pytest.raises(ValueError, match=r"\[CLS\]") as e:
            ix.rerank({}, [[0]], 1)
        assert "refine=" in str(e.value)


def test_search_refuses_candidates_where_there_is_no_first_stage_to_refine():
    from polus_amd.ir.search import CorpusIndex
    pq, ivf = _codecs()
    for kw in (dict(), dict(refine="full"), dict(storage="pq", codec=pq), dict(storage="ivfpq", codec=ivf), dict(storage="fp8")):
        ix = CorpusIndex(None, object(), **kw)
        ix._n, ix.tokens = 5, kw.get("storage") == "fp8"
        with pytest.raises(ValueError, match="candidates belongs to the search"):
            ix.search({}, 3, candidates=10)
    for kw in (dict(storage="pq", codec=pq, refine="full"), dict(storage="ivfpq", codec=ivf, refine="fp8", candidates=8)):
        ix = CorpusIndex(None, object(), **kw)
        ix._n, ix.tokens = 5, False
        for k, R in ((3, 2), (3, 1025), (3, 0), (1025, None), (9 if ix.candidates else 1025, None)):
            with pytest.raises(ValueError, match="<= candidates <= 1024"):
                ix.search({}, k, candidates=R)


def _fill(ix, n, fields):
    """Stand-in buffers of a filled index: `fields` = name -> (tail, dtype)."""
    ix._store.declare(**{name: (tail, dtype, 0) for name, (tail, dtype) in fields.items()})
    ix._store.reserve(2 * n, "cpu")
    ix._n, ix.tokens = n, False


def test_nbytes_counts_the_refine_store():
    from polus_amd.ir.search import CorpusIndex
    pq, ivf = _codecs()
    n, E = 10, 32
    plain = CorpusIndex(None, object(), refine="full")
    _fill(plain, n, dict(reps=((E,), torch.bfloat16)))
    assert plain.nbytes == n * E * 2, "no second copy on a plain index"
    for dtype, size in ((torch.bfloat16, 2), (torch.float32, 4)):
        full = CorpusIndex(None, object(), storage="pq", codec=pq, refine="full")
        _fill(full, n, dict(reps=((pq.m,), torch.uint8), rvec=((E,), dtype)))
        assert full.nbytes == n * (pq.m + E * size)
        assert full.refine_codes is None and full.refine_scales is None
    f8 = CorpusIndex(None, object(), storage="ivfpq", codec=ivf, refine="fp8")
    _fill(f8, n, dict(reps=((ivf.m,), torch.uint8), coarse=((), torch.int16), rcodes=((E,), torch.uint8), rscale=((), torch.float32)))
    assert f8.nbytes == n * (ivf.m + 2 + E + 4)
    assert tuple(f8.refine_codes.shape) == (n, E) and f8.refine_codes.dtype == torch.uint8
    assert tuple(f8.refine_scales.shape) == (n,) and f8.refine_scales.dtype == torch.float32
    none = CorpusIndex(None, object(), storage="ivfpq", codec=ivf)
    _fill(none, n, dict(reps=((ivf.m,), torch.uint8), coarse=((), torch.int16)))
    assert none.nbytes == n * (ivf.m + 2), "an index without refine stores what it stored before"


def test_the_declared_fields_of_each_refine_store():
    from polus_amd.ir import search as S
    pq, ivf = _codecs()
    v = torch.zeros((3, 32), dtype=torch.bfloat16)
    plain = S.CorpusIndex(None, object(), refine="full")
    assert plain._refine.fields(v) == {} and plain._refine.field == "reps"
    full = S.CorpusIndex(None, object(), storage="pq", codec=pq, refine="full")
    assert full._refine.fields(v) == dict(rvec=((32,), torch.bfloat16, 0))
    f8 = S.CorpusIndex(None, object(), storage="ivfpq", codec=ivf, refine="fp8")
    assert f8._refine.fields(v) == dict(rcodes=((32,), torch.uint8, 0), rscale=((), torch.float32, 0))
    assert S.CorpusIndex(None, object(), storage="pq", codec=pq)._refine is None


# ---------------------------------------------------------------- the binding and the entry points
def test_new_symbols_are_declared_and_bound():
    from polus_amd import _lib, ops, refine_ops
    txt = open(os.path.join(ROOT, "include", "polus_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    for name in NEW:
        assert re.search(r"\bint\s+%s\s*\(" % name, code), name
        assert name in _lib.SIGNATURES, name
        n_args = len(re.search(r"%s\s*\((.*?)\)" % name, code, flags=re.S).group(1).split(","))
        assert n_args == len(_lib.SIGNATURES[name][1]), name
        fn = getattr(ops, name[len("polus_"):])
        assert fn is getattr(refine_ops, name[len("polus_"):]) and fn.__module__ == "polus_amd.refine_ops" and fn.__doc__


def test_entry_points_refuse_on_the_host(lib):
    p = ctypes.c_void_p(256)
    odd = ctypes.c_void_p(264)

    def err(rc_, name):
        assert rc_ != 0
        msg = lib.polus_last_error()
        assert msg.startswith(name + b": "), msg
        return msg

    def full(dtype=0, Q=p, ldq=32, D=p, ldd=32, cand=p, ldcand=4, score=p, lds=4, B=1, C=4, N=9, E=32):
        return err(lib.polus_cls_rerank(dtype, Q, ldq, D, ldd, cand, ldcand, score, lds, B, C, N, E, None), b"polus_cls_rerank")

    def f8(dtype=0, Q=p, ldq=32, D=p, ldd=32, scale=p, cand=p, ldcand=4, score=p, lds=4, B=1, C=4, N=9, E=32):
        return err(lib.polus_cls_rerank_fp8(dtype, Q, ldq, D, ldd, scale, cand, ldcand, score, lds, B, C, N, E, None),
                   b"polus_cls_rerank_fp8")

    def quant(dtype=0, x=p, codes=p, scale=p, rows=1, E=32):
        return err(lib.polus_cls_fp8_quantize(dtype, x, codes, scale, rows, E, None), b"polus_cls_fp8_quantize")

    def dequant(dtype=0, codes=p, scale=p, y=p, rows=1, E=32):
        return err(lib.polus_cls_fp8_dequantize(dtype, codes, scale, y, rows, E, None), b"polus_cls_fp8_dequantize")

    for call in (full, f8, quant, dequant):
        assert b"unknown dtype" in call(dtype=2) and b"unknown dtype" in call(dtype=-1)
    for call in (full, f8):
        for E in (0, 8, 24, 5136, 5121):
            assert b"E must be a multiple of 16 in [16, 5120]" in call(E=E, ldq=6000, ldd=6000), E
        assert b"B <= 65535" in call(B=0) and b"B <= 65535" in call(B=65536)
        assert b"C <= 65535" in call(C=0) and b"C <= 65535" in call(C=65536, ldcand=65536, lds=65536)
        assert b"N <= 2^31 - 1" in call(N=0) and b"N <= 2^31 - 1" in call(N=-5)
        assert b"ldq must be >= E" in call(ldq=31) and b"ldd must be >= E" in call(ldd=31)
        assert b"ldcand must be >= C" in call(ldcand=3) and b"lds must be >= C" in call(lds=3)
        for name in ("Q", "D", "cand", "score"):
            assert b"null pointer" in call(**{name: None}), (call, name)
        assert b"16-byte aligned" in call(Q=odd) and b"16-byte aligned" in call(D=odd)
    assert b"null pointer" in f8(scale=None)
    # row strides that leave a row off a 16-byte boundary: f32 needs multiples of 4, bf16 of 8, codes of 16
    assert b"every row 16-byte aligned" in full(ldq=34) and b"every row 16-byte aligned" in full(ldd=33)
    assert b"every row 16-byte aligned" in full(dtype=1, ldq=36) and b"every row 16-byte aligned" in full(dtype=1, ldd=36)
    assert b"every row 16-byte aligned" in f8(ldd=40) and b"every row 16-byte aligned" in f8(dtype=1, ldq=36)
    for call, names in ((quant, ("x", "codes", "scale")), (dequant, ("codes", "scale", "y"))):
        for E in (0, 8, 24, 5136):
            assert b"E must be a multiple of 16 in [16, 5120]" in call(E=E), E
        assert b"rows >= 1" in call(rows=0)
        for name in names:
            assert b"null pointer" in call(**{name: None}), (call, name)
    assert b"16-byte aligned" in quant(x=odd) and b"16-byte aligned" in quant(codes=odd)
    assert b"16-byte aligned" in dequant(y=odd) and b"16-byte aligned" in dequant(codes=odd)


# ---------------------------------------------------------------- the wrappers
class D:
    """A host tensor that claims to be on the device: the recording library never dereferences its address."""

    def __init__(self, t):
        self.t = t

    is_cuda = True

    def __getattr__(self, name):
        return getattr(self.t, name)


@pytest.fixture
def rec(lib, monkeypatch):
    from tests.fakes import recording_lib
    yield from recording_lib(lib, monkeypatch, 0)


def test_wrappers_pass_what_the_header_declares(rec):
    from polus_amd import ops
    q, d = torch.zeros((3, 48), dtype=torch.bfloat16), torch.zeros((9, 64), dtype=torch.bfloat16)[:, :48]
    cand, score = torch.zeros((3, 7), dtype=torch.int32)[:, :5], torch.zeros((3, 6))[:, :5]
    ops.cls_rerank(D(q), D(d), D(cand), D(score))
    name, a = rec.calls[-1]
    assert name == "polus_cls_rerank" and a[0] == 1 and (a[2], a[4], a[6], a[8]) == (48, 64, 7, 6) and a[9:13] == (3, 5, 9, 48)
    assert (a[1], a[3], a[5], a[7]) == (q.data_ptr(), d.data_ptr(), cand.data_ptr(), score.data_ptr())
    codes, scale = torch.zeros((9, 48), dtype=torch.uint8), torch.zeros(9)
    ops.cls_rerank_fp8(D(q.float()), D(codes), D(scale), D(cand), D(score))
    name, a = rec.calls[-1]
    assert name == "polus_cls_rerank_fp8" and a[0] == 0 and (a[2], a[4], a[7], a[9]) == (48, 48, 7, 6) and a[10:14] == (3, 5, 9, 48)
    x = torch.zeros((9, 48))
    ops.cls_fp8_quantize(D(x), D(codes), D(scale))
    ops.cls_fp8_dequantize(D(codes), D(scale), D(x.bfloat16()))
    assert [n for n, _ in rec.calls[-2:]] == ["polus_cls_fp8_quantize", "polus_cls_fp8_dequantize"]
    assert rec.calls[-2][1][4:6] == (9, 48) and rec.calls[-1][1][0] == 1
    one = torch.zeros((1, 48))                                          # one row: its stride is never used
    ops.cls_rerank(D(one), D(one), D(torch.zeros((1, 1), dtype=torch.int32)), D(torch.zeros((1, 1))))
    assert rec.calls[-1][1][9:13] == (1, 1, 1, 48)


def test_wrappers_refuse_what_the_kernels_would_misread(rec):
    from polus_amd import ops
    from polus_amd._lib import PolusHipError
    with pytest.raises(PolusHipError, match="device"):
        ops.cls_rerank(torch.zeros((3, 32)), torch.zeros((9, 32)), torch.zeros((3, 4), dtype=torch.int32), torch.zeros((3, 4)))
    q, d = torch.zeros((3, 32)), torch.zeros((9, 32))
    cand, score = torch.zeros((3, 4), dtype=torch.int32), torch.zeros((3, 4))
    codes, scale = torch.zeros((9, 32), dtype=torch.uint8), torch.zeros(9)

    def full(q=q, d=d, cand=cand, score=score):
        return lambda: ops.cls_rerank(D(q), D(d), D(cand), D(score))

    def f8(q=q, codes=codes, scale=scale, cand=cand, score=score):
        return lambda: ops.cls_rerank_fp8(D(q), D(codes), D(scale), D(cand), D(score))

    bad = []
    for op, call in (("cls_rerank", full), ("cls_rerank_fp8", f8)):
        bad += [
            (f"{op}: q", call(q=q.double())), (f"{op}: q", call(q=q.half())), (f"{op}: q", call(q=q[0])),
            (f"{op}: q", call(q=torch.zeros((3, 24)))), (f"{op}: q", call(q=torch.zeros((3, 5136)))),
            (f"{op}: q", call(q=torch.zeros((3, 64))[:, ::2])), (f"{op}: q", call(q=torch.zeros((3, 34))[:, :32])),
            (f"{op}: q", call(q=torch.zeros((3, 33))[:, 1:])),
            (f"{op}: cand", call(cand=cand.long())), (f"{op}: cand", call(cand=cand[0])), (f"{op}: cand", call(cand=cand[:2])),
            (f"{op}: cand", call(cand=torch.zeros((3, 8), dtype=torch.int32)[:, ::2])),
            (f"{op}: cand", call(cand=torch.zeros((3, 0), dtype=torch.int32))),
            (f"{op}: score", call(score=score.double())), (f"{op}: score", call(score=torch.zeros((3, 5)))),
            (f"{op}: score", call(score=torch.zeros((2, 4)))), (f"{op}: score", call(score=torch.zeros((3, 8))[:, ::2])),
        ]
    bad += [
        ("cls_rerank: d", full(d=d.bfloat16())), ("cls_rerank: d", full(d=torch.zeros((9, 48)))),
        ("cls_rerank: d", full(d=torch.zeros((9, 34))[:, :32])), ("cls_rerank: d", full(d=torch.zeros((9, 64))[:, ::2])),
        ("cls_rerank: d", full(d=torch.zeros((9, 2, 32)))),
        ("cls_rerank_fp8: codes", f8(codes=codes.float())), ("cls_rerank_fp8: codes", f8(codes=codes[:, :16])),
        ("cls_rerank_fp8: codes", f8(codes=torch.zeros((9, 40), dtype=torch.uint8)[:, :32])),
        ("cls_rerank_fp8: scale", f8(scale=scale.double())), ("cls_rerank_fp8: scale", f8(scale=scale[:8])),
        ("cls_rerank_fp8: scale", f8(scale=torch.zeros(18)[::2])),
    ]
    x = torch.zeros((9, 32))
    for op, call in (("cls_fp8_quantize", lambda x=x, codes=codes, scale=scale: lambda: ops.cls_fp8_quantize(D(x), D(codes), D(scale))),
                     ("cls_fp8_dequantize", lambda x=x, codes=codes, scale=scale: lambda: ops.cls_fp8_dequantize(D(codes), D(scale), D(x)))):
        xn = "x" if op == "cls_fp8_quantize" else "y"
        bad += [
            (f"{op}: {xn}", call(x=x.double())), (f"{op}: {xn}", call(x=torch.zeros((9, 64))[:, :32])),
            (f"{op}: {xn}", call(x=torch.zeros((9, 24)), codes=torch.zeros((9, 24), dtype=torch.uint8))),
            (f"{op}: {xn}", call(x=x[0])),
            (f"{op}: codes", call(codes=codes.int())), (f"{op}: codes", call(codes=codes[:8])),
            (f"{op}: codes", call(codes=torch.zeros((9, 48), dtype=torch.uint8)[:, :32])),
            (f"{op}: scale", call(scale=scale.double())), (f"{op}: scale", call(scale=scale[:8])),
        ]
    before = len(rec.calls)
    for prefix, call in bad:
        with pytest.raises(AssertionError) as e:
            call()
        assert str(e.value).startswith(prefix), (prefix, str(e.value))
    assert len(rec.calls) == before, "a refused call reached the library"
    for call in (full(), f8()):
        call()
    assert len(rec.calls) == before + 2
