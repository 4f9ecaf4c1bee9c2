"""CPU: the postings reference (tests/postings_ref.py) against an independent dictionary-based float64 brute force, and
the host logic of the postings route: constructors, block_docs, chunking by whole blocks, nbytes, the refusals of the
entry points.  Runs without a device."""
import ctypes

import numpy as np
import pytest

from polus_amd.ir.postings import Postings, block_chunks, check_block_docs
from tests import postings_cases as pc
from tests import postings_ref as pr


def _reference_scores(ids, w, lists4, N, V, bd):
    q_terms, q_w, q_count = lists4
    _, _, _, lists = pr.build(ids, w, V, bd)
    return pr.scores(q_terms, q_w, q_count, lists, bd, N, V)


def test_reference_build_is_consistent():
    V, bd = pc.BUILD["V"], pc.BUILD["block_docs"]
    ids, w = pc.forward_case(300)
    counts, offsets, base, lists = pr.build(ids, w, V, bd)
    assert counts.shape == (5, V) and (offsets[:, 0] == 0).all() and base[0] == 0
    assert int(base[-1]) == int(counts.sum()) == sum(len(v) for v in lists.values())
    assert counts[pc.EMPTY_BLOCK].sum() == 0, "the case must hold a block without a posting"
    assert [int(counts[b, pc.HOT]) for b in range(5)] == [64, 64, 0, 64, 44], "the hot term is in every other document"
    nan = sum(1 for v in lists.values() for _, x in v if np.isnan(np.int32(x).view(np.float32)))
    assert nan == 1, "exactly one NaN weight is a posting"
    brute = sum(pr.is_posting(t, x, V) for t, x in zip(ids.ravel(), w.ravel()))
    assert brute == int(base[-1]) and brute < ids.size
    # a pack / unpack round trip, shuffled or not, gives the same sets
    for rng in (None, np.random.Generator(np.random.PCG64(1))):
        post_doc, post_w = pr.pack(offsets, base, lists, rng)
        assert pr.unpack(offsets, base, post_doc, post_w, V) == lists
    assert int(pr.build(*pc.empty_case(), V, bd)[2][-1]) == 0


@pytest.mark.parametrize("N", pc.BUILD_N)
def test_reference_scores_against_a_float64_brute_force(N):
    V, bd = pc.BUILD["V"], pc.BUILD["block_docs"]
    ids, w = pc.forward_case(N)
    w = np.where(np.isnan(w), np.float32(0.75), w)          # the bound is about finite sums
    for lists4 in (pc.query_lists(), pc.odd_query_list()):
        got = _reference_scores(ids, w, lists4, N, V, bd).astype(np.float64)
        want, mass, used = pr.scores_float64(*lists4, ids, w, V)
        bound = pc.score_bound(used[:, None], mass)
        err = np.abs(got - want)
        worst = float((err[bound > 0] / bound[bound > 0]).max())
        print(f"[postings] reference vs float64, N {N}: worst error / bound {worst:.3f}; {int((want != 0).sum())} of "
              f"{want.size} scores non-zero; entries per query {used.tolist()}")
        assert (err <= bound).all() and (got[mass == 0] == 0).all() and (want != 0).sum() >= N // 2


def test_reference_scores_are_exact_on_the_dyadic_case():
    V, bd, N = pc.BUILD["V"], pc.BUILD["block_docs"], 300
    ids, w = pc.forward_case(N, dyadic=True)
    lists4 = pc.query_lists(dyadic=True)
    got = _reference_scores(ids, w, lists4, N, V, bd)
    want, _, _ = pr.scores_float64(*lists4, ids, w, V)
    assert np.array_equal(got.astype(np.float64), want) and (want != 0).sum() > N
    # the repeated term of the odd list counts twice, the entries behind the count and outside [0, V) not at all
    odd = pc.odd_query_list()
    ids2 = np.array([[10, 20, pc.HOT]], np.int32)
    w2 = np.array([[2.0, 4.0, 1.0]], np.float32)
    s = _reference_scores(ids2, w2, odd, 1, V, bd)
    assert s[0, 0] == 0.5 * 1.0 + 1.25 * 2.0 + 0.75 * 2.0


def test_reference_query_lists():
    q = pc.compact_rows_case(97)
    terms, w, count = pr.compact_rows(q, 12)
    assert count.tolist() == [0, 97, 9, 3, 2, 40]
    assert (terms[0] == -1).all() and terms[1].tolist() == list(range(12)) and terms[4, :3].tolist() == [0, 96, -1]
    assert np.isnan(w[3, 0]) and np.isinf(w[3, 1]) and w[3, 2] > 0 and (np.diff(terms[5]) > 0).all()
    t, tf = pc.counted_queries(8, 97)
    idf = np.linspace(0.5, 2.0, 97).astype(np.float32)
    q_terms, q_w, q_count = pr.bm25_query_lists(t, tf, idf, 97)
    assert q_count.tolist() == [8, 4, 0, 6]
    for r in range(4):
        n = q_count[r]
        assert (np.diff(q_terms[r, :n]) > 0).all() and (q_terms[r, n:] == -1).all() and (q_w[r, n:] == 0).all()
        for j in range(n):
            m = int(np.nonzero(t[r] == q_terms[r, j])[0][0])
            assert q_w[r, j] == np.float32(tf[r, m]) * idf[q_terms[r, j]]


def test_constructors_and_block_docs():
    from polus_amd.ir.lexical import BM25Index
    from polus_amd.ir.search import SparseCorpusIndex
    wide = BM25Index(50000, postings=True)
    assert wide.vocab_size == 50000 and wide.block_docs == 8192 and len(wide) == 0 and wide.nbytes == 0
    assert wide.postings is None
    with pytest.raises(ValueError, match="40960"):
        BM25Index(50000)
    with pytest.raises(ValueError, match="40960"):
        BM25Index(50000, postings=False, block_docs=64)
    for bad in (0, 32, 63, 96, 100, 65536, 1 << 20):
        with pytest.raises(ValueError, match="block_docs"):
            check_block_docs(bad)
        with pytest.raises(ValueError, match="block_docs"):
            BM25Index(100, postings=True, block_docs=bad)
        with pytest.raises(ValueError, match="block_docs"):
            SparseCorpusIndex(None, postings=True, block_docs=bad)
    for good in (64, 128, 8192, 32768):
        assert check_block_docs(good) == good and BM25Index(100, postings=True, block_docs=good).block_docs == good
    with pytest.raises(ValueError, match="empty"):
        wide.search({"input_ids": np.zeros((1, 4), np.int32)}, 5)
    with pytest.raises(ValueError, match="empty"):
        wide.refresh_postings()
    with pytest.raises(ValueError, match="postings=False"):
        BM25Index(100).refresh_postings()
    sparse = SparseCorpusIndex(None, postings=True, block_docs=128, query_terms=64)
    assert (sparse.block_docs, sparse.query_terms, len(sparse), sparse.nbytes, sparse.postings) == (128, 64, 0, 0, None)
    with pytest.raises(ValueError, match="query_terms"):
        SparseCorpusIndex(None, postings=True, query_terms=0)
    with pytest.raises(ValueError, match="postings=False"):
        SparseCorpusIndex(None).refresh_postings()
    # the defaults are today's objects
    plain = SparseCorpusIndex(None)
    assert plain._postings is None and BM25Index(100)._postings is None and plain.postings is None


def test_chunks_are_whole_blocks():
    # 300 documents in blocks of 64: five blocks, two per launch when the scratch holds two blocks of 8 queries
    assert block_chunks(300, 8, 64, 4 * 8 * 64 * 2) == [(0, 2), (2, 2), (4, 1)]
    assert block_chunks(300, 8, 64, 4 * 8 * 64 * 2 + 4 * 8 * 63) == [(0, 2), (2, 2), (4, 1)], "a part of a block does not count"
    assert block_chunks(300, 8, 64, 256 << 20) == [(0, 5)]
    assert block_chunks(64, 1, 64, 256) == [(0, 1)] and block_chunks(40, 1, 64, 256) == [(0, 1)]
    assert block_chunks(33000, 3, 32768, 4 * 3 * 32768) == [(0, 1), (1, 1)]
    with pytest.raises(ValueError, match="one block of 64 documents"):
        block_chunks(300, 8, 64, 4 * 8 * 64 - 1)
    for spans in (block_chunks(1000, 5, 128, 4 * 5 * 128 * 3),):
        assert [b for b, _ in spans] == [0, 3, 6] and sum(n for _, n in spans) == 8


def test_nbytes_without_built_postings_is_the_forward_formula():
    p = Postings(64)
    assert not p.built and p.nbytes == 0 and p.arrays() == (None, None, None, None)

    class Held:
        """Stands in for device tensors: nbytes only asks for sizes."""

        def __init__(self, n, size=4):
            self.n, self.size = n, size

        def numel(self):
            return self.n

        def element_size(self):
            return self.size

    from polus_amd.ir.lexical import BM25Index
    from polus_amd.ir.search import SparseCorpusIndex
    for flag in (False, True):
        ix = BM25Index(500, terms=16, postings=flag, block_docs=64)
        ix._terms, ix._n = Held(200 * 16), 200
        assert ix.nbytes == 200 * (12 * 16 + 4) + 4 * 500 + 24
        sp = SparseCorpusIndex(None, terms=32, postings=flag, block_docs=64)
        sp._ids, sp._w, sp._n = Held(300 * 32), Held(300 * 32), 300
        assert sp.nbytes == 300 * 32 * 8
    # built postings count: offsets, base, and six bytes per posting
    p.offsets, p.base, p.count = Held(5 * 98), Held(6, 8), 1000
    assert p.nbytes == 4 * 5 * 98 + 8 * 6 + 6 * 1000


@pytest.fixture(scope="module")
def lib():
    from polus_amd import build
    build.build(verbose=False)
    from polus_amd import _lib
    return _lib.load()


def test_entry_points_refuse_bad_arguments_on_the_host(lib):
    p = ctypes.c_void_p(16)
    err = lib.polus_last_error
    count = lambda ids=p, ldi=8, ldw=8, N=300, M=8, V=97, bd=64, counts=p: \
        lib.polus_postings_count(ids, ldi, p, ldw, N, M, V, bd, counts, None)
    for kw, msg in ((dict(bd=63), b"power of two"), (dict(bd=32), b"power of two"), (dict(bd=65536), b"power of two"),
                    (dict(bd=96), b"power of two"), (dict(N=0), b"N >= 1"), (dict(V=0), b"1 <= V"), (dict(M=0), b"1 <= M"),
                    (dict(M=1025), b"M <= 1024"), (dict(ldi=7), b"ldi"), (dict(ldw=7), b"ldi, ldw"), (dict(ids=None), b"null pointer"),
                    (dict(counts=None), b"null pointer")):
        assert count(**kw) != 0 and msg in err(), (kw, err())
    off = lambda counts=p, nblk=5, V=97, base=p: lib.polus_postings_offsets(counts, nblk, V, p, base, None)
    for kw, msg in ((dict(nblk=0), b"nblk >= 1"), (dict(V=0), b"1 <= V"), (dict(base=None), b"null pointer")):
        assert off(**kw) != 0 and msg in err(), (kw, err())
    fill = lambda bd=64, P=10, cursor=p, post=p, M=8: \
        lib.polus_postings_fill(p, 8, p, 8, 300, M, 97, bd, p, p, P, cursor, post, p, None)
    for kw, msg in ((dict(bd=100), b"power of two"), (dict(P=-1), b"P >= 0"), (dict(cursor=None), b"null pointer"),
                    (dict(post=None), b"null pointer"), (dict(M=2000), b"M <= 1024")):
        assert fill(**kw) != 0 and msg in err(), (kw, err())
    comp = lambda q=p, ldq=100, Q=2, V=97, cap=12, ldt=12, cnt=p: \
        lib.polus_sparse_compact_rows(q, ldq, Q, V, cap, p, ldt, p, 12, cnt, None)
    for kw, msg in ((dict(Q=0), b"Q >= 1"), (dict(cap=0), b"cap >= 1"), (dict(ldq=96), b"ldq"), (dict(ldt=11), b"ldt"),
                    (dict(q=None), b"null pointer"), (dict(cnt=None), b"null pointer")):
        assert comp(**kw) != 0 and msg in err(), (kw, err())
    ql = lambda terms=p, Q=2, M=8, V=97, ldt2=8, idf=p: \
        lib.polus_bm25_query_lists(terms, 8, p, 8, idf, Q, M, V, p, ldt2, p, 8, p, None)
    for kw, msg in ((dict(M=1025), b"M <= 1024"), (dict(M=0), b"1 <= M"), (dict(Q=0), b"Q >= 1"), (dict(ldt2=7), b"ldt2"),
                    (dict(idf=None), b"null pointer")):
        assert ql(**kw) != 0 and msg in err(), (kw, err())
    sc = lambda cap=12, ldt=12, P=10, bd=64, blk0=0, nb=5, N=300, lds=300, Q=5, post=p, score=p: \
        lib.polus_postings_scores(p, ldt, p, 12, p, cap, p, p, post, p, P, 97, bd, blk0, nb, N, score, lds, Q, None)
    for kw, msg in ((dict(bd=48), b"power of two"), (dict(nb=6), b"blocks"), (dict(blk0=-1), b"blocks"), (dict(nb=0), b"blocks"),
                    (dict(blk0=4, nb=2), b"blocks"), (dict(lds=299), b"lds"), (dict(blk0=4, nb=1, lds=43), b"lds"),
                    (dict(ldt=11), b"ldt"), (dict(P=-5), b"P >= 0"), (dict(Q=0), b"Q >= 1"), (dict(cap=0, ldt=0), b"cap >= 1"),
                    (dict(post=None), b"null pointer"), (dict(score=None), b"null pointer"), (dict(N=0), b"N >= 1")):
        assert sc(**kw) != 0 and msg in err(), (kw, err())
    # the launch geometry checks come before any launch, so none of the calls above touched a device
