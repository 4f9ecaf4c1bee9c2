"""CPU: the NumPy reference of the BM25 and mining rules against independent statements of them (collections.Counter,
a hand-worked corpus, the sampling properties), the host-side argument checks of the four entry points, and the
polus.ir re-exports."""
import collections
import ctypes
import math

import numpy as np
import pytest

from tests import bm25_cases as bc
from tests import bm25_ref as br


def test_reference_term_counts_against_counter():
    ids, mask = bc.main_case()
    V, M, head, tail = (bc.MAIN[k] for k in ("V", "M", "head", "tail"))
    trunc, multi, empty, rejected = bc.main_conditions(ids, mask, V, M, head, tail)
    print(f"[bm25] main case: {trunc} truncated, {multi} with a count above 1, {empty} empty, {rejected} rejected tokens")
    assert trunc >= 1 and empty >= 1 and rejected >= 1 and 2 * multi >= len(ids)
    terms, tf, doc_len, df, stats = br.term_counts(ids, mask, V, M, head, tail)
    want_df = collections.Counter()
    for r in range(len(ids)):
        valid = [int(t) for t, m in zip(ids[r], mask[r]) if m]
        rest = valid[head:len(valid) - tail] if len(valid) > head + tail else []
        bag = collections.Counter(t for t in rest if 0 <= t < V)
        want = sorted(bag.items(), key=lambda kv: (-kv[1], kv[0]))[:M]
        got = [(int(t), int(f)) for t, f in zip(terms[r], tf[r]) if t >= 0]
        assert got == want, r
        assert (tf[r][terms[r] < 0] == 0).all() and doc_len[r] == sum(bag.values())
        want_df.update(bag.keys())
    assert all(df[t] == want_df.get(t, 0) for t in range(V))
    assert stats.tolist() == [trunc, rejected, int(doc_len.sum())]
    # accumulation: two halves into one df / stats give the whole
    h = len(ids) // 2
    _, _, _, df1, st1 = br.term_counts(ids[:h], mask[:h], V, M, head, tail)
    _, _, _, df2, st2 = br.term_counts(ids[h:], mask[h:], V, M, head, tail, df=df1, stats=st1)
    assert np.array_equal(df2, df) and np.array_equal(st2, stats)


def test_hand_worked_three_document_corpus():
    # documents over the terms {0: a, 1: b, 2: c}:  d0 = a a b,  d1 = b c,  d2 = c c c c;  query = a c
    ids = np.array([[0, 0, 1, 9], [1, 2, 9, 9], [2, 2, 2, 2]], np.int32)
    mask = np.array([[1, 1, 1, 0], [1, 1, 0, 0], [1, 1, 1, 1]], np.int32)
    k1, b = 1.2, 0.75
    terms, tf, doc_len, df, stats = br.term_counts(ids, mask, 3, 2, 0, 0)
    assert terms.tolist() == [[0, 1], [1, 2], [2, -1]] and tf.tolist() == [[2, 1], [1, 1], [4, 0]]
    assert doc_len.tolist() == [3, 2, 4] and df.tolist() == [1, 2, 2] and stats.tolist() == [0, 0, 9]
    # avgdl = 3; idf(a) = ln(1 + 2.5 / 1.5), idf(b) = idf(c) = ln(1 + 1.5 / 2.5)
    idf_a, idf_c = math.log(1 + 2.5 / 1.5), math.log(1 + 1.5 / 2.5)
    K = [k1 * (1 - b + b * n / 3.0) for n in (3, 2, 4)]                 # 1.2, 0.9, 1.5
    assert np.allclose(K, [1.2, 0.9, 1.5])
    want = [idf_a * 2 * 2.2 / (2 + 1.2),                                 # d0: a twice
            idf_c * 1 * 2.2 / (1 + 0.9),                                 # d1: c once
            idf_c * 4 * 2.2 / (4 + 1.5)]                                 # d2: c four times
    # ln(8 / 3) = 0.98082925 times 1.375;  ln(1.6) = 0.47000363 times 2.2 / 1.9 and times 1.6
    assert np.allclose(want, [1.3486402, 0.5442147, 0.7520058], rtol=0, atol=1e-7)
    q_ids, q_mask = np.array([[0, 2]], np.int32), np.ones((1, 2), np.int32)
    s64 = br.bm25_float64(ids, mask, q_ids, q_mask, 3, 0, 0, k1, b)
    assert np.allclose(s64[0], want, rtol=1e-12)
    # the f32 pipeline of the index: constants, weights, query row, dot product
    c0, c1, k1p1 = br.constants(k1, b, 3, 9)
    w = br.weights(tf, doc_len, c0, c1, k1p1)
    qt, qf, _, _, _ = br.term_counts(q_ids, q_mask, 3, 2, 0, 0)
    q = br.query(qt, qf, br.idf(df, 3), 3)
    got = [sum(float(w[d, m]) * float(q[0, terms[d, m]]) for m in range(2) if terms[d, m] >= 0) for d in range(3)]
    assert np.allclose(got, want, rtol=bc.score_bound(2)) and w[2, 1] == 0.0 and not np.signbit(w[2, 1])


@pytest.mark.parametrize("C,k,P", [(c, k, p) for c in bc.MINE_C for k in bc.MINE_K for p in (0, 3, 40)])
def test_mining_reference_properties(C, k, P):
    cand, score, exclude, skip_top, min_score = bc.mine_case(C, k, P)
    for seed in (0, 7):
        neg, col, n_pool = br.mine_negatives(cand, score, exclude, skip_top, min_score, k, seed)
        for r in range(cand.shape[0]):
            cols = br.pool(cand[r], score[r], None if exclude is None else exclude[r], skip_top, min_score)
            R = len(cols)
            assert n_pool[r] == R
            used = col[r][col[r] >= 0]
            assert (neg[r][col[r] < 0] == -1).all() and np.array_equal(neg[r][:len(used)], cand[r, used])
            banned = set() if exclude is None else set(exclude[r][exclude[r] >= 0].tolist())
            for c in used:
                assert c >= skip_top and cand[r, c] >= 0 and int(cand[r, c]) not in banned and score[r, c] > min_score
            if R <= k:
                assert used.tolist() == cols                 # the pool, in order
            else:
                assert len(used) == k and len(set(used.tolist())) == k
                pos = [cols.index(c) for c in used]
                assert all(j * R // k <= p < (j + 1) * R // k for j, p in enumerate(pos))


def test_mining_reference_hash_matches_the_dropout_hash():
    # tests/util.py restates polus_keep from the same hash: field 0 of element 4 n is the low half of hash32(seed, n)
    from tests.util import dropout_keep_np
    seed, n = 12345, 64
    keep = dropout_keep_np(seed, 0.5, 0, 4 * n)
    low = (br.hash32(seed, np.arange(n)) & np.uint64(0xFFFF)) >= 32768
    assert np.array_equal(np.asarray(keep[::4], bool), low)


@pytest.fixture(scope="module")
def lib():
    from polus_amd import build
    build.build(verbose=False)
    from polus_amd import _lib
    return _lib.load()


def test_entry_points_refuse_bad_arguments_on_the_host(lib):
    p = ctypes.c_void_p(16)
    tc = lambda **kw: lib.polus_bm25_term_counts(*[dict(dict(
        ids=p, ldi=4096, mask=p, ldm=4096, n=2, L=8, V=100, head=1, tail=1, terms=p, ldt=2048, tf=p, ldf=2048, M=4,
        doc_len=p, df=p, stats=p, stream=None), **kw)[a] for a in (
        "ids", "ldi", "mask", "ldm", "n", "L", "V", "head", "tail", "terms", "ldt", "tf", "ldf", "M", "doc_len", "df",
        "stats", "stream")])
    for kw, msg in ((dict(L=2049), b"L <= 2048"), (dict(L=0), b"1 <= L"), (dict(M=1025), b"M <= 1024"), (dict(M=0), b"1 <= M"),
                    (dict(ids=None), b"null pointer"), (dict(doc_len=None), b"null pointer"), (dict(n=0), b"n >= 1"),
                    (dict(V=0), b"V >= 1"), (dict(head=9), b"strip"), (dict(tail=-1), b"strip"), (dict(ldi=7), b"ldi"),
                    (dict(ldm=7), b"ldm"), (dict(ldt=3), b"ldt")):
        assert tc(**kw) != 0 and msg in lib.polus_last_error(), (kw, lib.polus_last_error())
    w = lambda tf=p, ldf=8, dl=p, out=p, ldw=8, n=2, M=8: lib.polus_bm25_weights(tf, ldf, dl, out, ldw, n, M, 0.5, 0.1, 1.9, None)
    for kw, msg in ((dict(M=1025), b"M <= 1024"), (dict(out=None), b"null pointer"), (dict(n=0), b"n >= 1"), (dict(ldw=7), b"ldw")):
        assert w(**kw) != 0 and msg in lib.polus_last_error(), (kw, lib.polus_last_error())
    q = lambda terms=p, idf=p, ldq=50000, B=1, M=4, V=30522: lib.polus_bm25_query(terms, 8, p, 8, idf, p, ldq, B, M, V, None)
    for kw, msg in ((dict(V=40961), b"V * 4 <= 163840"), (dict(idf=None), b"null pointer"), (dict(B=0), b"B >= 1"),
                    (dict(M=0), b"1 <= M"), (dict(ldq=30521), b"ldq")):
        assert q(**kw) != 0 and msg in lib.polus_last_error(), (kw, lib.polus_last_error())
    mine = lambda cand=p, ldc=100, score=p, lds=100, ex=p, lde=4, Q=2, C=100, P=4, skip=0, k=8, neg=p, pool=p: \
        lib.polus_mine_negatives(cand, ldc, score, lds, ex, lde, Q, C, P, skip, 0.0, k, 7, neg, p, pool, None)
    for kw, msg in ((dict(k=0), b"1 <= k"), (dict(k=1025), b"k <= 1024"), (dict(cand=None), b"null pointer"),
                    (dict(pool=None), b"null pointer"), (dict(ex=None), b"exclude"), (dict(P=1025, lde=2000), b"P <= 1024"),
                    (dict(skip=-1), b"skip_top"), (dict(C=0), b"C >= 1"), (dict(Q=1 << 30, k=8), b"2^32"), (dict(ldc=99), b"ldc"),
                    (dict(lds=99), b"lds"), (dict(lde=3), b"lde")):
        assert mine(**kw) != 0 and msg in lib.polus_last_error(), (kw, lib.polus_last_error())


def test_index_and_mining_refuse_bad_settings_before_touching_a_device():
    from polus_amd.ir.lexical import BM25Index, bm25_constants, bm25_idf
    from polus_amd.ir import mining
    for kw in (dict(vocab_size=0), dict(vocab_size=40961), dict(terms=0), dict(terms=1025), dict(strip=(9, 0)), dict(k1=-1.0),
               dict(b=1.5)):
        with pytest.raises(ValueError):
            BM25Index(**dict(dict(vocab_size=100), **kw))
    ix = BM25Index(30522)
    assert len(ix) == 0 and ix.nbytes == 0 and ix.truncated == 0 and ix.rejected == 0 and ix.term_ids is None
    with pytest.raises(ValueError, match="empty"):
        ix.search({"input_ids": np.zeros((1, 4), np.int32)}, 5)
    with pytest.raises(ValueError):
        ix.set_params(1.2, -0.1)
    # the host arithmetic of a refresh is the reference's
    assert bm25_constants(0.9, 0.4, 7, 123) == br.constants(0.9, 0.4, 7, 123) and bm25_constants(1.2, 0.75, 3, 0)[1] == np.float32(0.9)
    df = np.array([0, 1, 5, 7])
    assert np.array_equal(bm25_idf(df, 7), br.idf(df, 7))

    class Never:
        def search(self, queries, k):
            raise AssertionError("searched before the arguments were checked")
    for kw in (dict(k=0), dict(k=1025), dict(depth=0), dict(skip_top=-1)):
        with pytest.raises(ValueError):
            mining.mine_negatives(Never(), None, np.zeros((1, 1), np.int64), **dict(dict(k=4, depth=10), **kw))
    import torch
    for bad in (np.zeros((2, 1)), np.zeros((3, 1), np.int64), np.zeros((2, 0), np.int64), np.full((2, 1), -2)):
        with pytest.raises(ValueError):
            mining._positives(bad, 2, torch.device("cpu"))
    pos, first = mining._positives(np.array([4, -1]), 2, torch.device("cpu"))
    assert pos.dtype == torch.int32 and pos.tolist() == [[4], [-1]] and first.tolist() == [4, -1]
    # take_rows and tuple_batch are plain indexing: they run on host tensors too
    store = (torch.arange(12, dtype=torch.int32).reshape(4, 3), torch.ones((4, 3), dtype=torch.int32))
    queries = {"input_ids": np.arange(10).reshape(5, 2), "attention_mask": np.ones((5, 2), np.int32)}
    kept = mining.take_rows(queries, [0, 3])
    assert kept["input_ids"].tolist() == [[0, 1], [6, 7]]
    tuples = torch.tensor([[0, 1, 2], [3, 0, 1]], dtype=torch.int32)
    q, pd, nd, t = mining.tuple_batch(store, kept, tuples, np.zeros((2, 3), np.float32))
    assert pd["input_ids"].tolist() == [[0, 1, 2], [9, 10, 11]] and tuple(nd["input_ids"].shape) == (2, 2, 3)
    assert nd["input_ids"][1].tolist() == [[0, 1, 2], [3, 4, 5]] and tuple(nd["attention_mask"].shape) == (2, 2, 3)
    with pytest.raises(ValueError, match="take_rows"):
        mining.tuple_batch(store, queries, tuples)


def test_reexports():
    import polus.ir.lexical as lx
    import polus.ir.mining as mn
    from polus_amd.ir import lexical, mining
    assert lx.BM25Index is lexical.BM25Index
    assert mn.mine_negatives is mining.mine_negatives and mn.mine_tuples is mining.mine_tuples and mn.tuple_batch is mining.tuple_batch
