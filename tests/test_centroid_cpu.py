"""CPU: the centroid reference against the definition, host-side refusals of polus_centroid_scores / _codes / _update
and the route query (one violating call per limit, no device needed), and the route boundary."""
import ctypes

import numpy as np
import pytest

from tests import centroid_ref as cr
from tests.centroid_cases import CODE_SHAPES, LDS_BYTES, NONE, code_case, planted_corpus, score_case, update_case


@pytest.fixture(scope="module")
def lib():
    from polus_amd import build
    build.build(verbose=False)
    from polus_amd import _lib
    return _lib.load()


def test_reference_scores_equal_the_definition():
    for shape in [(1, 1, 1, 1, 1), (3, 6, 5, 17, 64), (2, 4, 31, 65, 30)]:
        B, N, Lq, Ld, K = shape
        for integer in (True, False):
            table, qmask, codes = score_case(*shape, integer=integer)
            want = cr.centroid_scores_loop(table, qmask, codes, B, Lq)
            got, mag = cr.centroid_scores(table, qmask, codes, B, Lq)
            assert np.allclose(got, want, rtol=0, atol=1e-12), shape
            assert (mag >= np.abs(got) - 1e-12).all()
            assert np.allclose(cr.centroid_scores(table, None, codes, B, Lq)[0],
                               cr.centroid_scores_loop(table, None, codes, B, Lq), rtol=0, atol=1e-12)
            if N > 1:
                assert (got[:, 1] == 0).all()                          # the empty document
            if B > 1:
                assert (got[1] == 0).all()                             # the empty query


def test_reference_codes_and_update():
    for rows, K in CODE_SHAPES[:4]:
        sim, mask = code_case(rows, K)
        got = cr.centroid_codes(sim[:, :K], mask)
        for i in range(rows):
            row = sim[i, :K]
            if mask[i] == 0:
                assert got[i] == NONE
            elif np.isnan(row).all():
                assert got[i] == 0
            else:
                best = np.nanmax(row)
                assert got[i] == min(c for c in range(K) if row[c] == best)
    x, codes, prev = update_case(70, 5, 128)
    out, counts, sums, _ = cr.centroid_update(x, codes, prev)
    assert counts.sum() == (codes < 5).sum() and counts[4] == 0 and counts[1] == 8
    assert np.array_equal(out[4], prev[4].astype(np.float64)) and np.array_equal(out[1], prev[1].astype(np.float64))
    assert (sums[1] == 0).all() and abs(np.linalg.norm(out[0]) - 1) < 1e-12
    # the planted corpus of the fit test: three rounds raise the mean best similarity by more than 0.1
    x = planted_corpus()
    gain = cr.mean_best_similarity(x, cr.spherical_kmeans(x, 16, 3)) - cr.mean_best_similarity(x, cr.spherical_kmeans(x, 16, 0))
    assert gain > 0.1, gain


def test_centroid_scores_refuses_on_the_host(lib):
    p = ctypes.c_void_p(256)                                           # never dereferenced: every call below is refused

    def cs(B=1, N=1, Lq=1, Ld=1, K=1, ldt=None, lds=None, table=p, codes=p, score=p):
        rc = lib.polus_centroid_scores(table, B * Lq if ldt is None else ldt, None, codes, score, N if lds is None else lds,
                                       B, N, Lq, Ld, K, None)
        assert rc != 0
        msg = lib.polus_last_error()
        assert b"polus_centroid_scores" in msg
        return msg
    assert b"Lq <= 512" in cs(Lq=513) and b"Lq <= 512" in cs(Lq=0)
    assert b"Ld <= 512" in cs(Ld=513) and b"Ld <= 512" in cs(Ld=0)
    assert b"K <= 65535" in cs(K=65536) and b"K <= 65535" in cs(K=0)
    assert b"B <= 65535" in cs(B=65536) and b"B <= 65535" in cs(B=0)
    assert b"N <= 65535" in cs(N=65536) and b"N <= 65535" in cs(N=0)
    assert b"ldt must be >= B*Lq" in cs(B=3, Lq=5, ldt=14)
    assert b"lds must be >= N" in cs(N=4, lds=3)
    for kw in (dict(table=None), dict(codes=None), dict(score=None)):
        assert b"null pointer" in cs(**kw)


def test_centroid_route_codes_and_update_refuse_on_the_host(lib):
    p = ctypes.c_void_p(256)
    out = (ctypes.c_int * 2)()

    def route(B=1, N=1, Lq=1, Ld=1, K=1, o=out):
        rc = lib.polus_centroid_scores_route(B, N, Lq, Ld, K, o)
        assert rc != 0
        return lib.polus_last_error()
    assert b"Lq <= 512" in route(Lq=513) and b"Ld <= 512" in route(Ld=0) and b"K <= 65535" in route(K=65536)
    assert b"B <= 65535" in route(B=0) and b"N <= 65535" in route(N=65536) and b"null pointer" in route(o=None)
    assert all(b"polus_centroid_scores_route" in m for m in (route(Lq=0), route(o=None)))

    def cc(rows=1, K=1, lds=None, sim=p, codes=p):
        rc = lib.polus_centroid_codes(sim, K if lds is None else lds, None, codes, rows, K, None)
        assert rc != 0
        msg = lib.polus_last_error()
        assert b"polus_centroid_codes" in msg
        return msg
    assert b"rows >= 1" in cc(rows=0) and b"K <= 65535" in cc(K=65536) and b"K <= 65535" in cc(K=0, lds=1)
    assert b"lds must be >= K" in cc(K=8, lds=7)
    assert b"null pointer" in cc(sim=None) and b"null pointer" in cc(codes=None)

    def cu(dtype=0, T=1, K=1, E=32, x=p, codes=p, prev=p, o=p, counts=p):
        rc = lib.polus_centroid_update(dtype, x, codes, prev, o, counts, T, K, E, 1e-12, None)
        assert rc != 0
        msg = lib.polus_last_error()
        assert b"polus_centroid_update" in msg
        return msg
    assert b"unknown dtype" in cu(dtype=2)
    assert b"multiple of 32" in cu(E=48) and b"multiple of 32" in cu(E=288) and b"multiple of 32" in cu(E=0)
    assert b"T >= 1" in cu(T=0) and b"K <= 65535" in cu(K=0) and b"K <= 65535" in cu(K=65536)
    for kw in (dict(x=None), dict(codes=None), dict(prev=None), dict(o=None), dict(counts=None)):
        assert b"null pointer" in cu(**kw)


def test_route_boundary_is_monotone_and_states_the_lds_bytes(lib):
    from polus_amd import ops
    out = (ctypes.c_int * 2)()
    for Lq in (1, 5, 16, 17, 32, 33, 64, 65, 200, 512):
        routes = []
        for K in (1, 2, 40, 79, 80, 318, 319, 1279, 1280, 2559, 2560, 40959, 40960, 65535):
            assert lib.polus_centroid_scores_route(2, 40, Lq, 17, K, out) == 0
            lds_bytes = (K + 1) * Lq * 4
            assert out[0] == (1 if lds_bytes <= LDS_BYTES else 2), (Lq, K)
            assert out[1] == (lds_bytes if out[0] == 1 else 0)
            routes.append(out[0])
        assert routes == sorted(routes), (Lq, routes)                  # LDS first, global from some K on: monotone in K
    for K in (1, 79, 1279, 65535):
        routes = [ops.centroid_scores_route(2, 40, Lq, 17, K).route for Lq in range(1, 513)]
        assert routes == sorted(routes, key=("lds", "global").index), K       # and in Lq
    # the shapes of the launch do not move it: the route is a function of Lq and K
    assert ops.centroid_scores_route(65535, 65535, 32, 512, 1279) == ("lds", 1280 * 32 * 4)
    assert ops.centroid_scores_route(1, 1, 32, 1, 1280) == ("global", 0)


def test_aliases_and_refusals_without_a_device():
    import polus.ir.search as asr
    import polus_amd.ir.search as s
    from polus_amd import _lib
    assert asr.CorpusIndex is s.CorpusIndex and callable(asr.CorpusIndex.search_pruned)
    assert callable(asr.CorpusIndex.fit_centroids) and callable(asr.CorpusIndex.set_centroids)
    for name in ("polus_centroid_scores", "polus_centroid_scores_route", "polus_centroid_codes", "polus_centroid_update"):
        assert name in _lib.SIGNATURES
    ix = s.CorpusIndex(None, object())
    assert ix.centroids is None and ix.centroid_codes is None and ix.nbytes == 0
    for call in (lambda: ix.search_pruned({}, 3, 10), lambda: ix.fit_centroids(4), lambda: ix.set_centroids(np.zeros((2, 32)))):
        with pytest.raises(ValueError, match="empty"):
            call()
    ix._n, ix.tokens = 5, False
    with pytest.raises(ValueError, match=r"\[CLS\]"):
        ix.fit_centroids(4)
    with pytest.raises(ValueError, match="needs centroids"):
        ix.search_pruned({}, 3, 10)
    ix.tokens = True
    with pytest.raises(ValueError, match="normalize=True"):
        ix.set_centroids(np.zeros((2, 32)))
    ix._centroids = object()
    for c in (0, 1025):
        with pytest.raises(ValueError, match="limit of ops.topk_merge"):
            ix.search_pruned({}, 3, c)
