"""GPU: polus_bm25_term_counts / polus_bm25_weights / polus_bm25_query / polus_mine_negatives bit for bit against
tests/bm25_ref.py, BM25Index against the same kernels run on the reference's arrays and against the textbook formula
in float64, and mining end to end with a cross-encoder teacher.  Outputs are pre-filled with a sentinel, every 2-d
tensor is a view of a wider buffer whose surplus must come back untouched, and every check prints its figure."""
import numpy as np
import pytest
import torch

from tests import bm25_cases as bc
from tests import bm25_ref as br

pytestmark = pytest.mark.gpu
SENTINEL = -77
FSENT = -9.25


def _wide(a, extra_cols, fill):
    """(buffer, view): the 2-d host array `a` in the top-left corner of a device buffer with `extra_cols` more columns
    and one more row, the rest `fill`."""
    t = torch.as_tensor(np.ascontiguousarray(a))
    buf = torch.full((a.shape[0] + 1, a.shape[1] + extra_cols), fill, dtype=t.dtype).cuda()
    view = buf[:a.shape[0], :a.shape[1]]
    view.copy_(t)
    return buf, view


def _out(rows, cols, extra_cols, dtype=torch.int32, fill=SENTINEL):
    buf = torch.full((rows + 1, cols + extra_cols), fill, dtype=dtype, device="cuda")
    return buf, buf[:rows, :cols]


def _untouched(buf, rows, cols, fill=SENTINEL):
    h = buf.cpu().numpy()
    return bool((h[rows:] == fill).all() and (h[:rows, cols:] == fill).all())


def _bits(a):
    a = a.cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    return np.ascontiguousarray(a.astype(np.float32, copy=False)).view(np.int32)


def _dev(a):
    return torch.as_tensor(np.ascontiguousarray(a)).cuda()


# ---------------------------------------------------------------- polus_bm25_term_counts
def _run_term_counts(ids, mask, V, M, head, tail, state=None, use_df=True):
    """One launch on strided views with poisoned outputs; returns host (terms, tf, doc_len, df, stats) and checks that
    nothing outside the outputs changed.  `state` = (df buffer, stats buffer) of an earlier call to accumulate into."""
    from polus_amd import ops
    n = ids.shape[0]
    _, d_ids = _wide(ids, 3, 7)
    d_mask = None if mask is None else _wide(mask, 5, 1)[1]
    (bt, terms), (bf, tf) = _out(n, M, 4), _out(n, M, 2)
    doc_len = torch.full((n + 2,), SENTINEL, dtype=torch.int32, device="cuda")
    if state is None:
        df = torch.full((V + 2,), SENTINEL, dtype=torch.int32, device="cuda")
        if use_df:                                   # without one the buffer stays poisoned: nothing may write it
            df[:V] = 0
        stats = torch.full((4,), SENTINEL, dtype=torch.int64, device="cuda")
        stats[:3] = 0
    else:
        df, stats = state
    ops.bm25_term_counts(d_ids, d_mask, terms, tf, doc_len, V, (head, tail), df=df if use_df else None, stats=stats)
    torch.cuda.synchronize()
    assert _untouched(bt, n, M) and _untouched(bf, n, M), "wrote outside the M columns"
    hl, hd, hs = doc_len.cpu().numpy(), df.cpu().numpy(), stats.cpu().numpy()
    assert (hl[n:] == SENTINEL).all() and (hd[V:] == SENTINEL).all() and hs[3] == SENTINEL
    return (terms.cpu().numpy(), tf.cpu().numpy(), hl[:n], hd[:V], hs[:3]), (df, stats)


def _check_term_counts(ids, mask, V, M, head, tail, what):
    got, _ = _run_term_counts(ids, mask, V, M, head, tail)
    ref = br.term_counts(ids, mask, V, M, head, tail)
    for name, g, r in zip(("terms", "tf", "doc_len", "df", "stats"), got, ref):
        assert np.array_equal(g, r), (what, name)
    print(f"[bm25] term_counts {what}: n {ids.shape[0]} L {ids.shape[1]} M {M}: stats {ref[4].tolist()}, "
          f"largest count {int(ref[1].max())}: exact")
    return ref


def test_term_counts_main_case_and_without_truncation():
    ids, mask = bc.main_case()
    V, M, head, tail = (bc.MAIN[k] for k in ("V", "M", "head", "tail"))
    trunc, multi, empty, rejected = bc.main_conditions(ids, mask, V, M, head, tail)
    print(f"[bm25] main case: {trunc} truncated, {multi} with a count above 1, {empty} empty, {rejected} rejected tokens")
    assert trunc >= 1 and empty >= 1 and rejected >= 1 and 2 * multi >= len(ids)
    ref = _check_term_counts(ids, mask, V, M, head, tail, "main")
    assert ref[4][0] == trunc
    ref = _check_term_counts(ids, mask, V, ids.shape[1], head, tail, "M = L")
    assert ref[4][0] == 0
    _check_term_counts(ids, None, V, M, head, tail, "mask = NULL")


@pytest.mark.parametrize("L", bc.TERM_L)
def test_term_counts_row_lengths(L):
    rng = np.random.Generator(np.random.PCG64(L))
    n, M, V = (2, 1024, 3000) if L == 2048 else (5, max(1, L // 2), 500)
    ids = rng.integers(0, V, size=(n, L)).astype(np.int32) if L == 2048 else bc.zipf_ids(rng, (n, L), V)
    mask = (rng.random((n, L)) < 0.9).astype(np.int32)
    mask[0] = 1
    for head, tail in ((0, 0), (1, 1)):
        ref = _check_term_counts(ids, mask, V, M, head, tail, f"L = {L}, strip {head}/{tail}")
        if L == 2048:
            assert ref[4][0] == n, "the long rows must be truncated at M = 1024"


def test_term_counts_special_rows_and_long_strips():
    L, V = 130, 500
    ids = np.stack([np.full(L, 7), np.arange(L), np.arange(L)[::-1] % 3]).astype(np.int32)
    ref = _check_term_counts(ids, np.ones((3, L), np.int32), V, L, 0, 0, "one repeated id / all distinct")
    assert ref[0][0, 0] == 7 and ref[1][0, 0] == L and (ref[0][0, 1:] == -1).all() and (ref[1][1] == 1).all()
    # strips longer than the row: rows of 0, 5, 16 and 17 valid tokens under head = tail = 8
    lens = np.array([0, 5, 16, 17, 20])
    mask = (np.arange(20)[None] < lens[:, None]).astype(np.int32)
    ids = bc.zipf_ids(np.random.Generator(np.random.PCG64(2)), (5, 20), V)
    ref = _check_term_counts(ids, mask, V, 8, 8, 8, "strips 8/8")
    assert ref[2].tolist() == [0, 0, 0, 1, 4]


def test_term_counts_accumulate_and_leave_df_alone_without_one():
    ids, mask = bc.main_case()
    V, M, head, tail = (bc.MAIN[k] for k in ("V", "M", "head", "tail"))
    h = len(ids) // 2
    _, state = _run_term_counts(ids[:h], mask[:h], V, M, head, tail)
    got, _ = _run_term_counts(ids[h:], mask[h:], V, M, head, tail, state=state)
    ref = br.term_counts(ids, mask, V, M, head, tail)
    assert np.array_equal(got[3], ref[3]) and np.array_equal(got[4], ref[4])
    print(f"[bm25] two calls into one df / stats: df sum {int(ref[3].sum())}, stats {ref[4].tolist()}: exact")
    # df = NULL: a poisoned df is not touched, everything else is as before
    got, _ = _run_term_counts(ids, mask, V, M, head, tail, use_df=False)
    assert (got[3] == SENTINEL).all(), "df = NULL: the poisoned df was written"
    assert all(np.array_equal(got[i], ref[i]) for i in (0, 1, 2, 4))


# ---------------------------------------------------------------- polus_bm25_weights, polus_bm25_query
def _corpus(V):
    if V == bc.MAIN["V"]:
        ids, mask = bc.main_case()
    else:
        rng = np.random.Generator(np.random.PCG64(V))
        ids = rng.integers(0, V, size=(50, 40)).astype(np.int32)
        ids[:, 5] = ids[:, 6]                                   # a count of 2 in every document
        mask = (np.arange(40)[None] < rng.integers(0, 41, size=50)[:, None]).astype(np.int32)
    return ids, mask


@pytest.mark.parametrize("V", [500, 30522])
def test_weights_and_query_bit_exact(V):
    from polus_amd import ops
    ids, mask = _corpus(V)
    n, M = ids.shape[0], 16
    terms, tf, doc_len, df, stats = br.term_counts(ids, mask, V, M, 1, 1)
    assert (tf == 0).any() and (tf > 1).any()
    _, d_tf = _wide(tf, 3, 5)
    d_len = _dev(doc_len)
    q_ids, q_mask = bc.query_case(1, 8, 12, V)
    qt, qf, _, _, _ = br.term_counts(q_ids, q_mask, V, 12, 1, 1)
    for k1, b in bc.PARAMS:
        c0, c1, k1p1 = br.constants(k1, b, n, int(stats[2]))
        want = br.weights(tf, doc_len, c0, c1, k1p1)
        bw, w = _out(n, M, 5, torch.float32, FSENT)
        ops.bm25_weights(d_tf, d_len, w, c0, c1, k1p1)
        got = w.cpu().numpy()
        diff = int((_bits(got) != _bits(want)).sum())
        print(f"[bm25] weights V {V} k1 {k1} b {b}: {diff} of {want.size} entries differ in bits; max w {want.max():.6f}")
        assert diff == 0 and _untouched(bw, n, M, FSENT)
        assert (_bits(got)[tf == 0] == 0).all(), "tf = 0 slots must be +0.0"
    idf = br.idf(df, n)
    want_q = br.query(qt, qf, idf, V)
    bq, q = _out(8, V, 3, torch.float32, FSENT)
    _, d_qt = _wide(qt, 2, 3)
    _, d_qf = _wide(qf, 1, 3)
    ops.bm25_query(d_qt, d_qf, _dev(idf), q)
    diff = int((_bits(q) != _bits(want_q)).sum())
    print(f"[bm25] query V {V}: {diff} of {want_q.size} entries differ in bits; {int((want_q != 0).sum())} non-zero")
    assert diff == 0 and _untouched(bq, 8, V, FSENT) and (want_q != 0).sum() >= 8


# ---------------------------------------------------------------- polus_mine_negatives
def _run_mine(cand, score, exclude, skip_top, min_score, k, seed, with_col=True):
    from polus_amd import ops
    Q, C = cand.shape
    bc_, d_cand = _wide(cand, 1, 0)
    d_score = None if score is None else _wide(score, 2, 9.0)[1]
    d_ex = None if exclude is None else _wide(exclude, 1, int(cand[0, 0]) if cand[0, 0] >= 0 else 0)[1]
    neg = torch.full((Q, k), SENTINEL, dtype=torch.int32, device="cuda")
    col = torch.full((Q, k), SENTINEL, dtype=torch.int32, device="cuda") if with_col else None
    n_pool = torch.full((Q + 2,), SENTINEL, dtype=torch.int32, device="cuda")
    ops.mine_negatives(d_cand, neg, n_pool, score=d_score, exclude=d_ex, skip_top=skip_top, min_score=float(min_score),
                       seed=seed, neg_col=col)
    torch.cuda.synchronize()
    hp = n_pool.cpu().numpy()
    assert (hp[Q:] == SENTINEL).all()
    return neg.cpu().numpy(), None if col is None else col.cpu().numpy(), hp[:Q]


def test_mine_negatives_matches_the_reference():
    seen = dict(zero=0, below=0, equal=0, one_more=0, many=0)
    launches = 0
    for C in bc.MINE_C:
        for k in bc.MINE_K:
            for P in bc.MINE_P:
                cand, score, exclude, skip_top, min_score = bc.mine_case(C, k, P)
                seed = 17 * C + k
                want = br.mine_negatives(cand, score, exclude, skip_top, min_score, k, seed)
                got = _run_mine(cand, score, exclude, skip_top, min_score, k, seed)
                for name, g, w in zip(("neg", "neg_col", "n_pool"), got, want):
                    assert np.array_equal(g, w), (name, C, k, P)
                R = want[2]
                seen["zero"] += int((R == 0).sum()); seen["below"] += int(((R > 0) & (R < k)).sum())
                seen["equal"] += int((R == k).sum()); seen["one_more"] += int((R == k + 1).sum())
                seen["many"] += int((R >= 4 * k).sum())
                launches += 1
    print(f"[mine] {launches} launches exact; pool sizes seen: {seen}")
    assert all(v >= 10 for v in seen.values()), seen
    # without scores and without neg_col
    cand, score, exclude, skip_top, _ = bc.mine_case(200, 8, 3)
    want = br.mine_negatives(cand, None, exclude, skip_top, 0.0, 8, 5)
    got = _run_mine(cand, None, exclude, skip_top, 0.0, 8, 5, with_col=False)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[2], want[2])


def test_mine_negatives_special_rows_and_seeds():
    C, k = 65, 4
    rng = np.random.Generator(np.random.PCG64(9))
    cand = np.stack([rng.permutation(500)[:C] for _ in range(5)]).astype(np.int32)
    score = (1.0 + rng.random((5, C))).astype(np.float32)
    exclude = np.full((5, 3), -1, np.int32)
    exclude[0, 1] = cand[0, 0]                # an excluded id in the first column
    exclude[1, 0] = cand[1, C - 1]            # ... in the last column
    exclude[2, 2] = 777                       # ... absent from the row
    exclude[3] = cand[3, 10]                  # repeated entries
    score[4, ::2], score[4, 1::4] = np.nan, 0.5                 # NaN and values equal to min_score
    want = br.mine_negatives(cand, score, exclude, 0, 0.5, k, 3)
    got = _run_mine(cand, score, exclude, 0, 0.5, k, 3)
    for name, g, w in zip(("neg", "neg_col", "n_pool"), got, want):
        assert np.array_equal(g, w), name
    assert want[2].tolist() == [C - 1, C - 1, C, C - 1, C - 33 - 16]
    assert cand[0, 0] not in got[0][0] and cand[1, C - 1] not in got[0][1] and cand[3, 10] not in got[0][3]
    print(f"[mine] special rows: pools {want[2].tolist()}, picks of row 4 at columns {got[1][4].tolist()}: exact")
    for skip_top in (C, C + 1000):
        neg, col, n_pool = _run_mine(cand, score, exclude, skip_top, 0.5, k, 3)
        assert (neg == -1).all() and (col == -1).all() and (n_pool == 0).all()
    again = _run_mine(cand, score, exclude, 0, 0.5, k, 3)
    other = _run_mine(cand, score, exclude, 0, 0.5, k, 4)
    assert all(np.array_equal(a, b) for a, b in zip(got, again)), "the same seed must give the same bits"
    assert not np.array_equal(other[0], got[0]) and np.array_equal(other[0], br.mine_negatives(cand, score, exclude, 0, 0.5, k, 4)[0])


# ---------------------------------------------------------------- BM25Index
def _batch(ids, mask, a, b):
    return {"input_ids": ids[a:b], "attention_mask": mask[a:b]}


def _reference_search(doc_ids, doc_mask, q_ids, q_mask, V, M, strip, k1, b, k):
    """What the index must return, bit for bit: the search kernels on (q, terms, w) built by the reference and uploaded."""
    from polus_amd import ops
    n = doc_ids.shape[0]
    terms, tf, doc_len, df, stats = br.term_counts(doc_ids, doc_mask, V, M, *strip)
    w = br.weights(tf, doc_len, *br.constants(k1, b, n, int(stats[2])))
    qt, qf, _, _, _ = br.term_counts(q_ids, q_mask, V, q_ids.shape[1], *strip)
    q = br.query(qt, qf, br.idf(df, n), V)
    s = torch.empty((q.shape[0], n), dtype=torch.float32, device="cuda")
    ops.sparse_scores(_dev(q), _dev(terms), _dev(w), s)
    val = torch.empty((q.shape[0], k), dtype=torch.float32, device="cuda")
    idx = torch.empty((q.shape[0], k), dtype=torch.int32, device="cuda")
    ops.topk_merge(s, val, idx, init=True)
    return val, idx, (terms, tf, doc_len, w)


def _same(got, want, what):
    assert torch.equal(got[1], want[1]), f"{what}: ids"
    assert np.array_equal(_bits(got[0]), _bits(want[0])), f"{what}: score bits"


def test_index_search_is_the_search_kernels_on_the_reference_arrays():
    from polus_amd.ir.lexical import BM25Index
    ids, mask = bc.main_case()
    V, M = bc.MAIN["V"], bc.MAIN["M"]
    N, h, k = len(ids), 90, 25
    q_ids, q_mask = bc.query_case(2, 8, 10, V)
    queries = {"input_ids": q_ids, "attention_mask": q_mask}
    index = BM25Index(V, terms=M)
    assert index.add(_batch(ids, mask, 0, h)).cpu().tolist() == list(range(h))
    first = index.search(queries, k)
    _same(first, _reference_search(ids[:h], mask[:h], q_ids, q_mask, V, M, (1, 1), 0.9, 0.4, k), "after the first batch")
    assert index.add(_batch(ids, mask, h, N)).cpu().tolist() == list(range(h, N)) and len(index) == N
    want = _reference_search(ids, mask, q_ids, q_mask, V, M, (1, 1), 0.9, 0.4, k)
    got = index.search(queries, k)                 # stale weights of the first 90 documents would fail here
    _same(got, want, "after the second batch")
    fresh = BM25Index(V, terms=M)
    fresh.add(_batch(ids, mask, 0, N))
    _same(got, fresh.search(queries, k), "two batches against one")
    terms, tf, doc_len, w = want[2]
    assert np.array_equal(index.term_ids.cpu().numpy(), terms) and np.array_equal(index.counts.cpu().numpy(), tf)
    assert np.array_equal(index.doc_lengths.cpu().numpy(), doc_len) and np.array_equal(_bits(index.weights), _bits(w))
    trunc, _, _, rejected = bc.main_conditions(ids, mask, V, M, 1, 1)
    assert index.truncated == trunc and index.rejected == rejected
    index.set_params(1.2, 0.75)
    _same(index.search(queries, k), _reference_search(ids, mask, q_ids, q_mask, V, M, (1, 1), 1.2, 0.75, k), "after set_params")
    index.set_params(0.9, 0.4)
    # three chunks give the bits of one
    small = BM25Index(V, terms=M, scratch_bytes=4 * 8 * 67)
    small.add(_batch(ids, mask, 0, N))
    assert len(small.chunks(8)) == 3 and len(index.chunks(8)) == 1
    _same(small.search(queries, k), got, "three chunks")
    moved = int((got[1] != first[1]).sum())
    print(f"[bm25] index: searches after 90 and {N} documents, set_params and three chunks equal the reference bit for bit; "
          f"{moved} of {first[1].numel()} result ids moved with the second batch")
    assert moved > 0
    # (e) clear, the empty index, nbytes
    assert index.nbytes == N * (12 * M + 4) + 4 * V + 24
    index.clear()
    assert len(index) == 0 and index.nbytes == 0 and index.truncated == 0
    with pytest.raises(ValueError, match="empty"):
        index.search(queries, 5)


def test_index_scores_against_the_textbook_formula_in_float64():
    from polus_amd.ir.lexical import BM25Index
    ids, mask = bc.main_case()
    V, L = bc.MAIN["V"], bc.MAIN["L"]
    N = len(ids)
    q_ids, q_mask = bc.query_case(3, 8, 10, V)
    index = BM25Index(V)                           # terms = L: nothing is truncated
    index.add(_batch(ids, mask, 0, N))
    assert index.terms == L and index.truncated == 0
    val, idx = index.search({"input_ids": q_ids, "attention_mask": q_mask}, N)
    val, idx = val.cpu().numpy().astype(np.float64), idx.cpu().numpy()
    ref = br.bm25_float64(ids, mask, q_ids, q_mask, V, 1, 1, 0.9, 0.4)
    assert (np.sort(idx, axis=1) == np.arange(N)[None]).all(), "k = N returns every document once"
    bound = bc.score_bound(L)
    at = np.take_along_axis(ref, idx, axis=1)      # the float64 score of each returned document
    # (b) every score within the derived bound of the textbook value
    err = np.abs(val - at)
    pos = at > 0
    ratio = float((err[pos] / (bound * at[pos])).max())
    print(f"[bm25] float64: bound {bound:.3e} relative; worst error / bound {ratio:.3f}; "
          f"{int(pos.sum())} of {pos.size} scores positive, largest {at.max():.4f}")
    assert pos.sum() > N and (val[~pos] == 0.0).all() and ratio <= 1.0
    # (c) ranking: position i holds a document at most twice the largest absolute bound below the i-th best
    slack = 2.0 * bound * float(ref.max())
    best = -np.sort(-ref, axis=1)
    gap = float((best - at).max())
    print(f"[bm25] ranking: largest shortfall against the float64 order {gap:.3e}, allowed {slack:.3e}")
    assert (at >= best - slack).all()


def test_two_stage_search_with_a_bm25_first_stage():
    from polus_amd.ir.lexical import BM25Index
    from polus_amd.ir.search import CorpusIndex, TwoStageSearch
    from polus_amd.ir.training import MaxSimScores
    from tests.search_cases import TableModel, batches, token_case
    case = dict(seed=3, Q=16, N=300, Lq=8, Ld=24, E=64, V=4096)
    c = token_case(**case)
    N = case["N"]
    docs = batches(c["d_ids"], c["d_mask"], [N // 2, N - N // 2])
    first = BM25Index(case["V"], strip=(0, 0))
    second = CorpusIndex(TableModel(c["table"], torch.float32, True), MaxSimScores(normalize=False))
    two = TwoStageSearch(first, second, candidates=50)
    assert torch.cat([two.add(b) for b in docs]).cpu().tolist() == list(range(N))
    queries = {"input_ids": c["q_ids"], "attention_mask": c["q_mask"]}
    val, idx = two.search(queries, 10)
    want_val, want_idx = second.rerank(queries, first.search(queries, 50)[1], 10)
    assert torch.equal(idx, want_idx) and np.array_equal(_bits(val), _bits(want_val))
    print(f"[bm25] two-stage: BM25 -> MaxSim equals rerank(search) on {case['Q']} queries")


# ---------------------------------------------------------------- mining end to end
def test_mine_tuples_with_a_cross_encoder_teacher_and_one_training_step():
    from polus_amd.ir.cross import CrossEncoderIndex
    from polus_amd.ir.lexical import BM25Index
    from polus_amd.ir.mining import mine_negatives, mine_tuples, take_rows, tuple_batch
    from polus_amd.ir.training import CrossEncoderTrainer, DistillKLLoss
    from polus_amd.optimizers import Adam
    from tests.test_cross_gpu import CLS, PAD, SEP, _model, _texts
    m, ocfg, _ = _model("bert_small_b3_s48", "f32")
    V = ocfg.vocab_size
    r = np.random.Generator(np.random.PCG64(23))
    N, Q, k, depth, seed = 30, 6, 3, 20, 11
    docs = _texts(ocfg, (N,), 24, r, lo=8)
    docs["input_ids"] = np.where(docs["input_ids"] == V - 1, 3, docs["input_ids"]).astype(np.int32)
    q_ids = np.full((Q, 6), PAD, np.int32)
    q_ids[:, 0], q_ids[:, 4] = CLS, SEP
    for i in range(Q):
        q_ids[i, 1:4] = docs["input_ids"][i, 1:4]               # three words of the query's positive
    q_ids[Q - 1, 1:4] = V - 1                                   # a word no document holds: an empty pool
    queries = {"input_ids": q_ids, "attention_mask": (q_ids != PAD).astype(np.int32)}
    positives = np.full((Q, 2), -1, np.int64)
    positives[:, 0] = np.arange(Q)
    positives[0, 1] = 7
    index = BM25Index(V)
    teacher = CrossEncoderIndex(m, strip=(1, 1), max_query_tokens=8, max_length=64, cls_token_id=CLS, sep_token_id=SEP,
                                pad_token_id=PAD, tokens_per_batch=256, round_to=16)
    index.add(docs)
    teacher.add(docs)
    mined = mine_tuples(index, queries, positives, k, depth, min_score=0.0, seed=seed, teacher=teacher)
    # the reference's tuples, given the index's own search result
    s, ids = index.search(queries, depth)
    want_neg, _, want_pool = br.mine_negatives(ids.cpu().numpy(), s.cpu().numpy(), positives, 0, 0.0, k, seed)
    rows = np.nonzero(want_pool >= k)[0]
    print(f"[mine] end to end: pools {want_pool.tolist()}, kept queries {rows.tolist()}, dropped {mined.dropped}")
    assert 0 < rows.size < Q and want_pool[Q - 1] == 0
    assert np.array_equal(mined.rows, rows) and mined.dropped == Q - rows.size
    assert np.array_equal(mined.n_pool.cpu().numpy(), want_pool)
    tuples = mined.tuples.cpu().numpy()
    assert np.array_equal(tuples[:, 0], positives[rows, 0]) and np.array_equal(tuples[:, 1:], want_neg[rows])
    for t, row in zip(tuples, rows):
        assert not set(t[1:].tolist()) & set(positives[row][positives[row] >= 0].tolist()) and (t >= 0).all()
    neg, n_pool, neg_col = mine_negatives(index, queries, positives, k, depth, min_score=0.0, seed=seed)
    assert np.array_equal(neg.cpu().numpy(), want_neg) and np.array_equal(n_pool.cpu().numpy(), want_pool)
    hc, hn = neg_col.cpu().numpy(), neg.cpu().numpy()
    assert all(ids.cpu().numpy()[i, hc[i, j]] == hn[i, j] for i in rows for j in range(k))
    kept = take_rows(queries, mined.rows)
    assert np.array_equal(_bits(mined.teacher_scores), _bits(teacher.score(kept, mined.tuples)))
    assert tuple(mined.teacher_scores.shape) == (rows.size, 1 + k) and bool(torch.isfinite(mined.teacher_scores).all())
    # the student IS the teacher here, so its own scores would give a loss of exactly 0: train against a softened copy
    batch = tuple_batch(teacher, kept, mined.tuples, mined.teacher_scores * 0.5)
    assert tuple(batch[1]["input_ids"].shape) == (rows.size, 24) and tuple(batch[2]["input_ids"].shape) == (rows.size, k, 24)
    assert np.array_equal(batch[2]["input_ids"].cpu().numpy(), docs["input_ids"][tuples[:, 1:]])
    trainer = CrossEncoderTrainer(m, Adam(1e-3), DistillKLLoss(), strip=(1, 1), max_query_tokens=8, max_length=64,
                                  cls_token_id=CLS, sep_token_id=SEP, pad_token_id=PAD)
    loss = float(trainer.train_step(*batch))
    print(f"[mine] one CrossEncoderTrainer step under DistillKLLoss on the mined batch: loss {loss:.6f}")
    assert np.isfinite(loss) and loss > 0.0 and tuple(trainer.scores.shape) == (rows.size, 1 + k)
