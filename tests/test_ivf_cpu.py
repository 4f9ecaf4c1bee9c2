"""CPU: the inverted-list reference against brute-force set comprehensions, host-side refusals of polus_ivf_* and
polus_centroid_scores_ids (one violating call per limit, no device needed), and the Python surface."""
import ctypes

import numpy as np
import pytest

from tests import ivf_ref as ir
from tests.centroid_cases import NONE
from tests.ivf_cases import MARK_K, hot_codes, ids_case, list_codes, mark_case


@pytest.fixture(scope="module")
def lib():
    from polus_amd import build
    build.build(verbose=False)
    from polus_amd import _lib
    return _lib.load()


def test_reference_equals_the_definition():
    for N in (7, 33):
        K = MARK_K
        codes, probes, qmask = mark_case(N)
        counts, offsets, per_centroid = ir.lists(codes, K)
        for c in range(K):
            assert per_centroid[c] == sorted({n for n in range(N) for j in range(codes.shape[1]) if codes[n, j] == c})
        assert counts.tolist() == [len(x) for x in per_centroid] and offsets[0] == 0 and offsets[K] == counts.sum()
        assert np.array_equal(np.diff(offsets), counts) and per_centroid[K - 2] == []
        docs = np.concatenate([np.asarray(x[::-1], np.int64) for x in per_centroid])      # any order inside a list
        assert ir.split(offsets, docs) == per_centroid
        B, Lq, nprobe = probes.shape
        for m in (qmask, None):
            want = [{n for n in range(N) for i in range(Lq) for p in range(nprobe)
                     if (m is None or m[b, i]) and 0 <= probes[b, i, p] < K and probes[b, i, p] in codes[n].tolist()}
                    for b in range(B)]
            assert ir.candidates(probes, m, per_centroid, N) == want
        assert ir.candidates(probes, qmask, per_centroid, N)[1] == set()                   # the query without a valid token
        bits = ir.bitmap(want, N)
        count, cand = ir.compact(bits, N, 5)
        for b in range(B):
            assert count[b] == len(want[b]) and cand[b].tolist() == (sorted(want[b]) + [-1] * 5)[:5]
    assert (hot_codes()[:, :] == 0).sum(axis=1).min() == 2 and ids_case(2, 9).shape == (2, 16)


def test_every_centroid_probed_names_exactly_the_documents_with_a_token():
    for N, Ld, K in ((40, 17, 64), (9, 33, 7)):
        codes = list_codes(N, Ld, K)
        per_centroid = ir.lists(codes, K)[2]
        probes = np.arange(K, dtype=np.int32)[None, None]                  # one query, one token, every centroid
        got = ir.candidates(probes, None, per_centroid, N)[0]
        assert got == {n for n in range(N) if (codes[n] < K).any()} and 1 not in got and 2 in got
        assert (codes[1] == NONE).all()


def test_ivf_entry_points_refuse_on_the_host(lib):
    p = ctypes.c_void_p(256)                                           # never dereferenced: every call below is refused

    def msg(rc, name):
        assert rc != 0
        m = lib.polus_last_error()
        assert name in m
        return m

    def count(N=1, Ld=1, K=1, codes=p, counts=p):
        return msg(lib.polus_ivf_count(codes, N, Ld, K, counts, None), b"polus_ivf_count")

    def fill(N=1, Ld=1, K=1, P=1, codes=p, offsets=p, cursor=p, docs=p):
        return msg(lib.polus_ivf_fill(codes, N, Ld, K, offsets, P, cursor, docs, None), b"polus_ivf_fill")
    for call in (count, fill):
        assert b"N >= 1" in call(N=0) and b"Ld <= 512" in call(Ld=0) and b"Ld <= 512" in call(Ld=513)
        assert b"K <= 65535" in call(K=0) and b"K <= 65535" in call(K=65536) and b"null pointer" in call(codes=None)
    assert b"null pointer" in count(counts=None)
    assert b"P < 2^31" in fill(P=-1)
    for kw in (dict(offsets=None), dict(cursor=None), dict(docs=None)):
        assert b"null pointer" in fill(**kw)

    def offsets(K=1, counts=p, out=p):
        return msg(lib.polus_ivf_offsets(counts, K, out, None), b"polus_ivf_offsets")
    assert b"K <= 65535" in offsets(K=0) and b"K <= 65535" in offsets(K=65536)
    assert b"null pointer" in offsets(counts=None) and b"null pointer" in offsets(out=None)

    def mark(P=1, K=1, N=1, B=1, Lq=1, nprobe=1, ldp=None, ldb=None, probes=p, offs=p, docs=p, bitmap=p):
        return msg(lib.polus_ivf_mark(probes, nprobe if ldp is None else ldp, None, offs, docs, P, K, N, bitmap,
                                      (N + 31) // 32 if ldb is None else ldb, B, Lq, nprobe, None), b"polus_ivf_mark")
    assert b"K <= 65535" in mark(K=0) and b"K <= 65535" in mark(K=65536)
    assert b"N >= 1" in mark(N=0) and b"B >= 1" in mark(B=0)
    assert b"Lq <= 512" in mark(Lq=0) and b"Lq <= 512" in mark(Lq=513)
    assert b"nprobe <= 1024" in mark(nprobe=0) and b"nprobe <= 1024" in mark(nprobe=1025)
    assert b"P < 2^31" in mark(P=-1)
    assert b"ldp must be >= nprobe" in mark(nprobe=4, ldp=3) and b"ldb must be >= ceil(N/32)" in mark(N=33, ldb=1)
    for kw in (dict(probes=None), dict(offs=None), dict(docs=None), dict(bitmap=None)):
        assert b"null pointer" in mark(**kw)

    def compact(B=1, N=1, cap=1, ldb=None, ldc=None, bitmap=p, cand=p, cnt=p):
        return msg(lib.polus_ivf_compact(bitmap, (N + 31) // 32 if ldb is None else ldb, B, N, cand, cap if ldc is None else ldc,
                                         cap, cnt, None), b"polus_ivf_compact")
    assert b"N >= 1" in compact(N=0) and b"B >= 1" in compact(B=0) and b"ldb must be >= ceil(N/32)" in compact(N=65, ldb=2)
    assert b"cap >= 1" in compact(cap=0) and b"ldc must be >= cap" in compact(cap=8, ldc=7)
    assert b"null pointer" in compact(bitmap=None) and b"null pointer" in compact(cnt=None)

    def ids(B=1, C=1, N=1, Lq=1, Ld=1, K=1, ldt=None, ldc=None, lds=None, table=p, codes=p, cand=p, score=p):
        return msg(lib.polus_centroid_scores_ids(table, B * Lq if ldt is None else ldt, None, codes, cand, C if ldc is None else ldc,
                                                 score, C if lds is None else lds, B, C, N, Lq, Ld, K, None),
                   b"polus_centroid_scores_ids")
    assert b"Lq <= 512" in ids(Lq=513) and b"Lq <= 512" in ids(Lq=0) and b"Ld <= 512" in ids(Ld=513) and b"Ld <= 512" in ids(Ld=0)
    assert b"K <= 65535" in ids(K=65536) and b"K <= 65535" in ids(K=0)
    assert b"B <= 65535" in ids(B=65536) and b"B <= 65535" in ids(B=0)
    assert b"C <= 65535" in ids(C=65536) and b"C <= 65535" in ids(C=0) and b"N >= 1" in ids(N=0)
    assert b"ldt must be >= B*Lq" in ids(B=3, Lq=5, ldt=14) and b"ldc must be >= C" in ids(C=4, ldc=3)
    assert b"lds must be >= C" in ids(C=4, lds=3)
    for kw in (dict(table=None), dict(codes=None), dict(cand=None), dict(score=None)):
        assert b"null pointer" in ids(**kw)


def test_surface_without_a_device():
    import inspect

    import polus.ir.search as asr
    import polus_amd.ir.search as s
    from polus_amd import _lib, ops
    assert asr.CorpusIndex is s.CorpusIndex and asr.RetrievalValidationCallback is s.RetrievalValidationCallback
    for name in ("CorpusIndex", "ResidualCodec", "SparseCorpusIndex", "TwoStageSearch", "RetrievalValidationCallback",
                 "MAX_K", "MAX_CENTROIDS"):
        assert getattr(asr, name) is getattr(s, name), name              # the re-exports are what they were
    for name in ("probe", "refresh_lists", "search_pruned"):
        assert callable(getattr(asr.CorpusIndex, name))
    assert isinstance(s.CorpusIndex.lists, property)
    assert inspect.signature(s.CorpusIndex.search_pruned).parameters["nprobe"].default is None
    assert inspect.signature(s.RetrievalValidationCallback.__init__).parameters["nprobe"].default is None
    for name in ("polus_ivf_count", "polus_ivf_offsets", "polus_ivf_fill", "polus_ivf_mark", "polus_ivf_compact",
                 "polus_centroid_scores_ids"):
        assert name in _lib.SIGNATURES
    for name in ("ivf_count", "ivf_offsets", "ivf_fill", "ivf_mark", "ivf_compact", "centroid_scores_ids"):
        assert callable(getattr(ops, name))
    ix = s.CorpusIndex(None, object())
    assert ix.lists is None and ix.nbytes == 0
    for call in (lambda: ix.probe({}, 1), lambda: ix.refresh_lists(), lambda: ix.search_pruned({}, 3, 10, nprobe=1)):
        with pytest.raises(ValueError, match="empty"):
            call()
    ix._n, ix.tokens = 5, True
    for call in (lambda: ix.probe({}, 1), lambda: ix.refresh_lists(), lambda: ix.search_pruned({}, 3, 10, nprobe=1)):
        with pytest.raises(ValueError, match="needs centroids"):
            call()
    assert ix.lists is None
    ix._centroids = np.zeros((6, 32), np.float32)                      # only its shape is looked at before the refusal
    for bad in (0, 7, 2000):
        for call in (lambda: ix.probe({}, bad), lambda: ix.search_pruned({}, 3, 10, nprobe=bad)):
            with pytest.raises(ValueError, match=r"1 <= nprobe <= min\(K, 1024\) = 6"):
                call()
    with pytest.raises(ValueError, match="nprobe needs centroids"):
        s.RetrievalValidationCallback([], [], 5, nprobe=2)
