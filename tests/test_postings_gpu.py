"""GPU: the postings kernels (postings.hip) bit for bit against tests/postings_ref.py, and the postings route of
BM25Index and SparseCorpusIndex end to end.  Outputs are pre-filled with a sentinel, every 2-d tensor is a view of a
wider buffer whose surplus must come back untouched, and every check prints its figure (pytest -s shows them)."""
import functools

import numpy as np
import pytest
import torch

from polus_amd.ir.postings import block_chunks
from tests import bm25_cases as bc
from tests import bm25_ref as br
from tests import postings_cases as pc
from tests import postings_ref as pr

pytestmark = pytest.mark.gpu
SENTINEL = -77
FSENT = -9.25
V, BD, M = pc.BUILD["V"], pc.BUILD["block_docs"], pc.BUILD["M"]


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


def _flat(n, extra, dtype, fill=SENTINEL):
    """(buffer, its first n elements): a 1-d output with `extra` poisoned elements behind it."""
    buf = torch.full((n + extra,), fill, dtype=dtype, device="cuda")
    return buf, buf[:n]


def _bits(a):
    a = a.cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    return np.ascontiguousarray(a.astype(np.float32, copy=False)).view(np.int32)


def _dev(a):
    return torch.as_tensor(np.ascontiguousarray(a)).cuda()


def _u16(t):
    return t.cpu().numpy().view(np.uint16)


# ---------------------------------------------------------------- build: count, offsets, fill
def _device_build(ids, w, V, bd):
    """count -> offsets -> fill on strided forward views with poisoned outputs; returns host (counts, offsets, base,
    post_doc uint16, post_w) and checks that nothing outside the outputs changed."""
    from polus_amd import ops
    N = ids.shape[0]
    nblk = (N + bd - 1) // bd
    _, d_ids = _wide(ids, 3, 5)                      # the surplus columns hold a valid id with a non-zero weight
    _, d_w = _wide(w, 1, 1.5)
    cbuf, counts = _flat(nblk * V, 3, torch.int32)
    obuf, offsets = _flat(nblk * (V + 1), 3, torch.int32)
    bbuf, base = _flat(nblk + 1, 2, torch.int64)
    counts, offsets = counts.view(nblk, V), offsets.view(nblk, V + 1)
    ops.postings_count(d_ids, d_w, V, bd, counts)
    ops.postings_offsets(counts, offsets, base)
    h_counts = counts.cpu().numpy().copy()
    P = int(base.cpu()[nblk])
    dbuf, post_doc = _flat(P, 4, torch.int16)
    wbuf, post_w = _flat(P, 4, torch.float32, FSENT)
    ops.postings_fill(d_ids, d_w, bd, offsets, base, counts, post_doc, post_w)          # counts serve as the cursor
    torch.cuda.synchronize()
    for buf, n, fill in ((cbuf, nblk * V, SENTINEL), (obuf, nblk * (V + 1), SENTINEL), (bbuf, nblk + 1, SENTINEL),
                         (dbuf, P, SENTINEL), (wbuf, P, FSENT)):
        assert (buf.cpu().numpy()[n:] == fill).all(), "wrote behind an output"
    assert np.array_equal(counts.cpu().numpy(), h_counts), "fill's cursors must end at the counts"
    return h_counts, offsets.cpu().numpy(), base.cpu().numpy(), _u16(post_doc), post_w.cpu().numpy()


def _check_build(ids, w, V, bd, what):
    counts, offsets, base, post_doc, post_w = _device_build(ids, w, V, bd)
    r_counts, r_offsets, r_base, lists = pr.build(ids, w, V, bd)
    assert np.array_equal(counts, r_counts), (what, "counts")
    assert np.array_equal(offsets, r_offsets), (what, "offsets")
    assert np.array_equal(base, r_base), (what, "base")
    assert pr.unpack(offsets, base, post_doc, post_w, V) == lists, (what, "lists as sorted sets with weight bits")
    print(f"[postings] build {what}: N {ids.shape[0]} blocks {len(base) - 1} P {int(base[-1])}, longest list "
          f"{int(r_counts.max())}, {int((r_counts.sum(axis=1) == 0).sum())} empty blocks: exact")
    return r_counts, r_offsets, r_base, lists


@pytest.mark.parametrize("N", pc.BUILD_N)
def test_build_matches_the_reference(N):
    ids, w = pc.forward_case(N)
    counts, _, base, lists = _check_build(ids, w, V, BD, f"N = {N}")
    assert int(counts[:, pc.HOT].max()) == min(N, BD), "the hot counter takes one add per document of a block"
    assert int(base[-1]) < ids.size, "the case must hold slots that are no postings"
    if N == 300:
        assert counts[pc.EMPTY_BLOCK].sum() == 0 and base[pc.EMPTY_BLOCK] == base[pc.EMPTY_BLOCK + 1]
        assert any(np.isnan(np.int32(x).view(np.float32)) for v in lists.values() for _, x in v), "the NaN weight is a posting"


def test_build_of_a_corpus_without_postings():
    ids, w = pc.empty_case()
    counts, offsets, base, _ = _check_build(ids, w, V, BD, "no posting at all")
    assert base.tolist() == [0, 0, 0] and not counts.any() and not offsets.any()
    none = np.zeros(0, np.uint16), np.zeros(0, np.float32)
    got = _run_scores(pc.query_lists(), offsets, base, *none, BD, len(ids))
    assert (_bits(got) == 0).all(), "P = 0: every document scores +0.0"


# ---------------------------------------------------------------- polus_sparse_compact_rows
@pytest.mark.parametrize("V_", pc.COMPACT_V)
def test_compact_rows(V_):
    from polus_amd import ops
    q = pc.compact_rows_case(V_)
    Q = q.shape[0]
    for cap in (12, 64):
        _, d_q = _wide(q, 2 if V_ % 2 else 3, 4.0)            # an odd row stride: rows are not 16-byte aligned
        assert (d_q.stride(0) * 4) % 16 != 0
        (bt, terms), (bw, w) = _out(Q, cap, 3), _out(Q, cap, 5, torch.float32, FSENT)
        count = torch.full((Q + 2,), SENTINEL, dtype=torch.int32, device="cuda")
        ops.sparse_compact_rows(d_q, terms, w, count)
        r_terms, r_w, r_count = pr.compact_rows(q, cap)
        hc = count.cpu().numpy()
        assert np.array_equal(hc[:Q], r_count) and (hc[Q:] == SENTINEL).all()
        assert np.array_equal(terms.cpu().numpy(), r_terms) and np.array_equal(_bits(w), _bits(r_w))
        assert _untouched(bt, Q, cap) and _untouched(bw, Q, cap, FSENT), "wrote past column cap - 1"
        assert r_count[1] == V_ > cap and r_count[0] == 0 and np.isnan(r_w[3, 0])
        print(f"[postings] compact V {V_} cap {cap}: counts {r_count.tolist()}: exact")


# ---------------------------------------------------------------- polus_bm25_query_lists
@pytest.mark.parametrize("Mq", [1, 8, 65, 1024])
def test_bm25_query_lists(Mq):
    from polus_amd import ops
    Vq = 3000
    terms, tf = pc.counted_queries(Mq, Vq)
    idf = (0.25 + np.random.Generator(np.random.PCG64(Mq)).random(Vq)).astype(np.float32)
    _, d_terms = _wide(terms, 3, 7)
    _, d_tf = _wide(tf, 1, 2)
    (bt, q_terms), (bw, q_w) = _out(4, Mq, 2), _out(4, Mq, 3, torch.float32, FSENT)
    count = torch.full((6,), SENTINEL, dtype=torch.int32, device="cuda")
    ops.bm25_query_lists(d_terms, d_tf, _dev(idf), q_terms, q_w, count)
    r_terms, r_w, r_count = pr.bm25_query_lists(terms, tf, idf, Vq)
    hc = count.cpu().numpy()
    assert np.array_equal(hc[:4], r_count) and (hc[4:] == SENTINEL).all()
    assert np.array_equal(q_terms.cpu().numpy(), r_terms) and np.array_equal(_bits(q_w), _bits(r_w))
    assert _untouched(bt, 4, Mq) and _untouched(bw, 4, Mq, FSENT)
    assert r_count[0] == Mq and r_count[2] == 0 and r_count[3] < Mq, "a full row, an empty row and a row with dropped ids"
    print(f"[postings] bm25_query_lists M {Mq}: counts {r_count.tolist()}: terms and weight bits exact")


# ---------------------------------------------------------------- polus_postings_scores
def _run_scores(lists3, offsets, base, post_doc, post_w, bd, N, blk0=0, nb=None):
    """One launch over the blocks [blk0, blk0 + nb) with strided query lists and a poisoned, wider score buffer."""
    from polus_amd import ops
    q_terms, q_w, q_count = lists3
    Q = q_terms.shape[0]
    nblk = (N + bd - 1) // bd
    nb = nblk - blk0 if nb is None else nb
    cols = min(nb * bd, N - blk0 * bd)
    _, d_terms = _wide(q_terms, 3, 3)
    _, d_w = _wide(q_w, 1, 2.0)
    bs, score = _out(Q, cols, 5, torch.float32, FSENT)
    ops.postings_scores(d_terms, d_w, _dev(q_count), _dev(offsets), _dev(base), _dev(post_doc.view(np.int16)), _dev(post_w),
                        bd, blk0, nb, N, score)
    torch.cuda.synchronize()
    assert _untouched(bs, Q, cols, FSENT), "wrote outside the launch's columns of score"
    return score.cpu().numpy()


@functools.lru_cache(maxsize=None)
def _built(N):
    ids, w = pc.forward_case(N)
    counts, offsets, base, lists = pr.build(ids, w, V, BD)
    return ids, w, offsets, base, lists


@pytest.mark.parametrize("N", pc.BUILD_N)
def test_scores_bit_for_bit_and_independent_of_the_list_order(N):
    ids, w, offsets, base, lists = _built(N)
    queries = pc.query_lists()
    want = pr.scores(*queries, lists, BD, N, V)
    sorted_arrays = pr.pack(offsets, base, lists)
    got = _run_scores(queries, offsets, base, *sorted_arrays, BD, N)
    diff = int((_bits(got) != _bits(want)).sum())
    print(f"[postings] scores N {N}: {diff} of {want.size} differ in bits; {int((want != 0).sum())} non-zero, "
          f"{int(np.isnan(want).sum())} NaN")
    assert diff == 0 and (want != 0).sum() > N // 2
    shuffled = pr.pack(offsets, base, lists, np.random.Generator(np.random.PCG64(N)))
    assert not np.array_equal(shuffled[0], sorted_arrays[0]), "the shuffle must move something"
    again = _run_scores(queries, offsets, base, *shuffled, BD, N)
    assert np.array_equal(_bits(again), _bits(want)), "shuffled lists must give the same bits"
    # the device's own postings give them too
    d_offsets, d_base, d_doc, d_w = _device_build(ids, w, V, BD)[1:]
    assert np.array_equal(_bits(_run_scores(queries, d_offsets, d_base, d_doc, d_w, BD, N)), _bits(want))
    if N == 300:
        assert np.isnan(want).any(), "the NaN weight must reach a score"
        assert (_bits(want[:, pc.EMPTY_BLOCK * BD:(pc.EMPTY_BLOCK + 1) * BD]) == 0).all(), "the empty block scores +0.0"
        # a launch over a part of the blocks writes that part, starting at column 0
        part = _run_scores(queries, offsets, base, *sorted_arrays, BD, N, blk0=3, nb=2)
        assert np.array_equal(_bits(part), _bits(want[:, 3 * BD:]))
        mid = _run_scores(queries, offsets, base, *sorted_arrays, BD, N, blk0=1, nb=2)
        assert np.array_equal(_bits(mid), _bits(want[:, BD:3 * BD]))


def test_scores_of_a_list_that_breaks_its_promises():
    N = 300
    _, _, offsets, base, lists = _built(N)
    odd = pc.odd_query_list()
    want = pr.scores(*odd, lists, BD, N, V)
    got = _run_scores(odd, offsets, base, *pr.pack(offsets, base, lists), BD, N)
    assert np.array_equal(_bits(got), _bits(want)) and (want != 0).sum() > N // 2
    # the repeated term counts twice: dropping its second entry changes scores
    once = (odd[0].copy(), odd[1].copy(), odd[2])
    once[0][0, 4] = -1
    assert not np.array_equal(_bits(pr.scores(*once, lists, BD, N, V)), _bits(want))
    print(f"[postings] odd list (-1 inside, ids >= V, a repeat, entries behind the count): {int((want != 0).sum())} scores exact")


def test_foreign_postings_cannot_fault_or_write_outside_the_row():
    N = 300
    _, _, offsets, base, lists = _built(N)
    queries = pc.query_lists()
    post_doc, post_w = pr.pack(offsets, base, lists)
    P = int(base[-1])
    want = pr.scores(*queries, lists, BD, N, V)
    # (a) a base pointing past P: the block's lists are refused whole and it scores +0.0; the others are unchanged
    bad_base = base.copy()
    bad_base[1] = P + 1000
    got = _run_scores(queries, offsets, bad_base, post_doc, post_w, BD, N)
    assert (_bits(got[:, BD:2 * BD]) == 0).all()
    keep = np.r_[0:BD, 2 * BD:N]
    assert np.array_equal(_bits(got[:, keep]), _bits(want[:, keep]))
    # (b) a negative base: the list positions below 0 are not read
    bad_base = base.copy()
    bad_base[0] = -50
    got = _run_scores(queries, offsets, bad_base, post_doc, post_w, BD, N)
    assert np.array_equal(_bits(got[:, BD:]), _bits(want[:, BD:]))
    # (c) local ids that are no document of their block: the last block holds 44 documents
    last = N // BD
    a, e = int(base[last]), int(base[last + 1])
    bad_doc = post_doc.copy()
    hit = np.arange(a, e)[::3]
    bad_doc[hit] = np.array([44, 50, 63, 64, 30000, 0xFFFF], np.uint16)[np.arange(len(hit)) % 6]
    pruned = {k: [x for i, x in enumerate(v) if k[0] != last or (a + int(offsets[last, k[1]]) + i) not in set(hit.tolist())]
              for k, v in lists.items()}
    want_c = pr.scores(*queries, {k: v for k, v in pruned.items() if v}, BD, N, V)
    got = _run_scores(queries, offsets, base, bad_doc, post_w, BD, N)
    assert np.array_equal(_bits(got), _bits(want_c)) and not np.array_equal(_bits(want_c), _bits(want))
    # (d) offsets of another corpus (descending, negative, huge): any scores, but no fault and the surplus untouched
    rng = np.random.Generator(np.random.PCG64(4))
    wild = rng.integers(-2 ** 31, 2 ** 31 - 1, size=offsets.shape, dtype=np.int64).astype(np.int32)
    _run_scores(queries, wild, base, post_doc, post_w, BD, N)
    print(f"[postings] foreign postings: base past P, negative base, {len(hit)} local ids out of range, wild offsets: "
          f"refused entries contribute nothing, nothing outside the row is written")


def test_scores_with_the_largest_block():
    from polus_amd import ops
    N, bd, Ms = 33000, 32768, 4
    ids, w = pc.forward_case(N, M=Ms, block_docs=bd, special=False)
    ids[::9, 2] = -1
    d_ids, d_w = _dev(ids), _dev(w)
    counts = torch.empty((2, V), dtype=torch.int32, device="cuda")
    offsets = torch.empty((2, V + 1), dtype=torch.int32, device="cuda")
    base = torch.empty((3,), dtype=torch.int64, device="cuda")
    ops.postings_count(d_ids, d_w, V, bd, counts)
    ops.postings_offsets(counts, offsets, base)
    h_counts = counts.cpu().numpy()
    P = int(base.cpu()[2])
    post_doc = torch.empty((P,), dtype=torch.int16, device="cuda")
    post_w = torch.empty((P,), dtype=torch.float32, device="cuda")
    ops.postings_fill(d_ids, d_w, bd, offsets, base, counts, post_doc, post_w)
    # counts by a histogram, scores by the reference over vectorised lists
    valid = ids >= 0
    want_counts = np.stack([np.bincount(ids[a:b][valid[a:b]], minlength=V) for a, b in ((0, bd), (bd, N))])
    assert np.array_equal(h_counts, want_counts) and P == int(valid.sum()) and h_counts.max() > 30000
    lists = {}
    for t in range(V):
        d, m = np.nonzero(ids == t)
        for b in (0, 1):
            sel = (d // bd) == b
            if sel.any():
                lists[(b, t)] = list(zip((d[sel] - b * bd).tolist(), _bits(w[d[sel], m[sel]]).tolist()))
    queries = pc.query_lists()
    want = pr.scores(*queries, lists, bd, N, V)
    got = _run_scores(queries, offsets.cpu().numpy(), base.cpu().numpy(), _u16(post_doc), post_w.cpu().numpy(), bd, N)
    diff = int((_bits(got) != _bits(want)).sum())
    print(f"[postings] block_docs 32768, N {N}: P {P}, longest list {int(h_counts.max())}; {diff} of {want.size} scores differ")
    assert diff == 0 and (want[:, bd:] != 0).any()


# ---------------------------------------------------------------- SparseCorpusIndex end to end
class _Given:
    """An encoder that hands the index ready-made representations."""

    def encode_query(self, x, training=False):
        return x

    encode_document = query_projection = document_projection = encode_query


def _same(got, want, what):
    assert torch.equal(got[1], want[1]), f"{what}: ids"
    assert np.array_equal(_bits(got[0]), _bits(want[0])), f"{what}: score bits"


def test_sparse_index_postings_equal_the_forward_route_on_dyadic_representations():
    from polus_amd.ir.search import SparseCorpusIndex
    Vs, N, Q, terms = 200, 300, 8, 32
    docs = _dev(pc.dyadic_reps(N, Vs, terms, seed=1))
    queries = _dev(pc.dyadic_reps(Q, Vs, terms, seed=2))
    one = 256 << 20
    three = 4 * Q * BD * 2                                # two blocks of 64 per launch: three launches over five blocks
    assert len(block_chunks(N, Q, BD, three)) == 3
    forward = SparseCorpusIndex(_Given(), terms=terms)
    inverted = {s: SparseCorpusIndex(_Given(), terms=terms, scratch_bytes=s, postings=True, block_docs=BD, query_terms=terms)
                for s in (one, three)}
    h = 130                                               # the first batch ends inside the third block
    for ix in (forward, *inverted.values()):
        assert ix.add(docs[:h]).cpu().tolist() == list(range(h))
    assert inverted[one].nbytes == forward.nbytes, "an index never searched builds nothing"
    for k in (10, 350):
        want = forward.search(queries, k)
        for s, ix in inverted.items():
            _same(ix.search(queries, k), want, f"{h} documents, k {k}, scratch {s}")
    built = inverted[one].nbytes - forward.nbytes
    offsets, base, post_doc, post_w = inverted[one].postings
    P = int(base[-1])
    assert built == 4 * offsets.numel() + 8 * base.numel() + 6 * P and tuple(offsets.shape) == (3, Vs + 1)
    assert post_doc.dtype == torch.int16 and post_doc.numel() == P == post_w.numel() == int((docs[:h] != 0).sum())
    for ix in (forward, *inverted.values()):
        ix.add(docs[h:])
    assert inverted[one]._postings_stale and inverted[one].postings[0].shape[0] == 5, "add marks stale, the next use rebuilds"
    ties = 0
    for k in (10, 350):
        want = forward.search(queries, k)
        v = want[0].cpu().numpy()
        ties += int(((v[:, 1:] == v[:, :-1]) & np.isfinite(v[:, 1:])).sum())
        for s, ix in inverted.items():
            _same(ix.search(queries, k), want, f"{N} documents, k {k}, scratch {s}")
        if k > N:
            assert (want[1][:, N:] == -1).all() and torch.isinf(want[0][:, N:]).all()
    print(f"[postings] sparse index: postings route equals the forward route on {Q} queries at k = 10 and 350, one and "
          f"three launches, before and after a second add; {ties} tied neighbours among the results; P {P} after the first batch")
    assert ties > 10, "the case must hold ties"
    # query_terms overflow names the count
    tight = SparseCorpusIndex(_Given(), terms=terms, postings=True, block_docs=BD, query_terms=8)
    tight.add(docs)
    most = int((queries != 0).sum(dim=1).max())
    with pytest.raises(ValueError, match=str(most)):
        tight.search(queries, 5)
    # clear, then a smaller corpus
    ix = inverted[one]
    ix.clear()
    forward.clear()
    assert len(ix) == 0 and ix.nbytes == 0 and ix.postings is None
    with pytest.raises(ValueError, match="empty"):
        ix.search(queries, 5)
    ix.add(docs[200:240])
    forward.add(docs[200:240])
    _same(ix.search(queries, 50), forward.search(queries, 50), "after clear: 40 documents, less than a block")
    assert ix.postings[0].shape[0] == 1


def test_sparse_index_postings_take_a_wide_vocabulary():
    from polus_amd._lib import PolusHipError
    from polus_amd.ir.search import SparseCorpusIndex
    Vw, N, Q = 50000, 100, 4
    rng = np.random.Generator(np.random.PCG64(8))
    docs, queries = np.zeros((N, Vw), np.float32), np.zeros((Q, Vw), np.float32)
    pool = np.concatenate([[0, Vw - 1, 40960, 40961], rng.permutation(Vw)[:40]])
    for r in range(N):
        docs[r, rng.permutation(pool)[:10]] = rng.integers(1, 33, size=10) / 8.0
    for r in range(Q):
        queries[r, rng.permutation(pool)[:12]] = rng.integers(1, 33, size=12) / 8.0
    queries[0, Vw - 1], docs[7, Vw - 1] = 2.0, 4.0
    ix = SparseCorpusIndex(_Given(), terms=16, postings=True, block_docs=BD, query_terms=16)
    ix.add(_dev(docs))
    val, idx = ix.search(_dev(queries), 20)
    want = pr.rank((queries.astype(np.float64) @ docs.astype(np.float64).T).astype(np.float32), 20)    # exact: dyadic
    assert np.array_equal(idx.cpu().numpy(), want[1]) and np.array_equal(_bits(val), _bits(want[0]))
    plain = SparseCorpusIndex(_Given(), terms=16)
    plain.add(_dev(docs))
    with pytest.raises(PolusHipError, match="163840"):
        plain.search(_dev(queries), 20)
    print(f"[postings] sparse index over V = {Vw}: exact; the forward route refuses as before")


# ---------------------------------------------------------------- BM25Index end to end
def _batch(ids, mask, a, b):
    return {"input_ids": ids[a:b], "attention_mask": mask[a:b]}


def _bm25_reference(index, q_ids, q_mask, Vb, strip, k):
    """The reference applied to the index's own (term_ids, weights, idf)."""
    ids, w = index.term_ids.cpu().numpy(), index.weights.cpu().numpy()
    idf = index.idf.cpu().numpy()
    qt, qf, _, _, _ = br.term_counts(q_ids, q_mask, Vb, q_ids.shape[1], *strip)
    lists3 = pr.bm25_query_lists(qt, qf, idf, Vb)
    _, _, _, lists = pr.build(ids, w, Vb, index.block_docs)
    s = pr.scores(*lists3, lists, index.block_docs, len(ids), Vb)
    return pr.rank(s, k), s


def _equal_to_reference(got, want, what):
    assert np.array_equal(got[1].cpu().numpy(), want[1]), f"{what}: ids"
    assert np.array_equal(_bits(got[0]), _bits(want[0])), f"{what}: score bits"


def test_bm25_index_postings_bit_for_bit_and_against_float64():
    from polus_amd.ir.lexical import BM25Index
    ids, mask = bc.main_case()
    Vb, L = bc.MAIN["V"], bc.MAIN["L"]
    N, h, k = len(ids), 90, 25
    q_ids, q_mask = bc.query_case(2, 8, 10, Vb)
    queries = {"input_ids": q_ids, "attention_mask": q_mask}
    index = BM25Index(Vb, postings=True, block_docs=BD)
    index.add(_batch(ids, mask, 0, h))
    forward_bytes = h * (12 * L + 4) + 4 * Vb + 24
    assert index.nbytes == forward_bytes
    first = index.search(queries, k)
    _equal_to_reference(first, _bm25_reference(index, q_ids, q_mask, Vb, (1, 1), k)[0], "after the first batch")
    assert index.nbytes > forward_bytes
    index.add(_batch(ids, mask, h, N))
    got = index.search(queries, k)                         # stale weights or stale postings would fail here
    _equal_to_reference(got, _bm25_reference(index, q_ids, q_mask, Vb, (1, 1), k)[0], "after the second batch")
    assert int((got[1] != first[1]).sum()) > 0
    index.set_params(1.2, 0.75)
    assert index._postings_stale
    moved = index.search(queries, k)
    _equal_to_reference(moved, _bm25_reference(index, q_ids, q_mask, Vb, (1, 1), k)[0], "after set_params")
    assert not np.array_equal(_bits(moved[0]), _bits(got[0]))
    index.set_params(0.9, 0.4)
    small = BM25Index(Vb, postings=True, block_docs=BD, scratch_bytes=4 * 8 * BD)
    small.add(_batch(ids, mask, 0, N))
    assert len(block_chunks(N, 8, BD, small.scratch_bytes)) == 4
    _equal_to_reference(small.search(queries, k), (got[0].cpu().numpy(), got[1].cpu().numpy()), "four launches")
    small.scratch_bytes -= 1
    with pytest.raises(ValueError, match="one block"):
        small.search(queries, k)
    # the textbook formula in float64, with the forward route's bound and ranking slack.  The bound allows for
    # gamma(L + 1) + 10 u with L = 40; this route spends at most 8 sums and one more rounded product per summand.
    val, idx = index.search({"input_ids": q_ids, "attention_mask": q_mask}, N)
    val, idx = val.cpu().numpy().astype(np.float64), idx.cpu().numpy()
    ref = br.bm25_float64(ids, mask, q_ids, q_mask, Vb, 1, 1, 0.9, 0.4)
    assert (np.sort(idx, axis=1) == np.arange(N)[None]).all(), "k = N returns every document once"
    bound = bc.score_bound(L)
    at = np.take_along_axis(ref, idx, axis=1)
    err, pos = np.abs(val - at), at > 0
    ratio = float((err[pos] / (bound * at[pos])).max())
    slack = 2.0 * bound * float(ref.max())
    best = -np.sort(-ref, axis=1)
    print(f"[postings] bm25 float64: bound {bound:.3e} relative, worst error / bound {ratio:.3f}; {int(pos.sum())} of "
          f"{pos.size} scores positive; largest ranking shortfall {float((best - at).max()):.3e}, allowed {slack:.3e}")
    assert pos.sum() > N and (val[~pos] == 0.0).all() and ratio <= 1.0
    assert (at >= best - slack).all()


def test_bm25_index_postings_with_a_vocabulary_past_the_forward_limit():
    from polus_amd.ir.lexical import BM25Index
    Vb, N, L = 50000, 100, 12
    rng = np.random.Generator(np.random.PCG64(31))
    pool = np.concatenate([[0, 49999, 40960, 45000], rng.integers(0, Vb, size=60)])
    d_ids = rng.choice(pool, size=(N, L)).astype(np.int32)
    d_ids[3, 4], d_ids[9, 0] = 49999, 49999
    q_ids = rng.choice(pool, size=(6, 5)).astype(np.int32)
    q_ids[0, 0] = 49999
    ones = lambda a: np.ones_like(a)
    index = BM25Index(Vb, strip=(0, 0), postings=True, block_docs=BD)
    index.add({"input_ids": d_ids, "attention_mask": ones(d_ids)})
    got = index.search({"input_ids": q_ids, "attention_mask": ones(q_ids)}, 30)
    want, s = _bm25_reference(index, q_ids, ones(q_ids), Vb, (0, 0), 30)
    _equal_to_reference(got, want, "V = 50000")
    holders = np.nonzero((d_ids == 49999).any(axis=1))[0]
    assert (s[0, holders] > 0).all() and index.rejected == 0 and tuple(index.postings[0].shape) == (2, Vb + 1)
    with pytest.raises(ValueError, match="encode_query_lists"):
        index.encode_queries({"input_ids": q_ids})
    print(f"[postings] bm25 over V = {Vb}: {len(holders)} documents hold term 49999 and score for it; exact")


def test_two_stage_and_hybrid_search_over_a_postings_first_stage():
    from polus_amd.ir.fusion import HybridSearch
    from polus_amd.ir.lexical import BM25Index
    from polus_amd.ir.search import CorpusIndex, TwoStageSearch
    from polus_amd.ir.training import MaxSimScores
    from tests.search_cases import TableModel, batches, token_case
    case = dict(seed=3, Q=16, N=300, Lq=8, Ld=24, E=64, V=4096)
    c = token_case(**case)
    N = case["N"]
    docs = batches(c["d_ids"], c["d_mask"], [N // 2, N - N // 2])
    queries = {"input_ids": c["q_ids"], "attention_mask": c["q_mask"]}
    first = BM25Index(case["V"], strip=(0, 0), postings=True, block_docs=BD)
    second = CorpusIndex(TableModel(c["table"], torch.float32, True), MaxSimScores(normalize=False))
    two = TwoStageSearch(first, second, candidates=50)
    assert torch.cat([two.add(b) for b in docs]).cpu().tolist() == list(range(N))
    val, idx = two.search(queries, 10)
    cand = first.search(queries, 50)
    want_val, want_idx = second.rerank(queries, cand[1], 10)
    assert torch.equal(idx, want_idx) and np.array_equal(_bits(val), _bits(want_val))
    _equal_to_reference(cand, _bm25_reference(first, c["q_ids"], c["q_mask"], case["V"], (0, 0), 50)[0], "first stage")

    class Frozen:
        """A stage that returns a stored result."""

        def __init__(self, result):
            self.result = result

        def __len__(self):
            return N

        def search(self, queries, k):
            return self.result

    stages = [BM25Index(case["V"], strip=(0, 0), k1=k1, b=b, postings=True, block_docs=BD) for k1, b in ((0.9, 0.4), (2.0, 1.0))]
    hybrid = HybridSearch(stages, 40)
    for b in docs:
        hybrid.add(b)
    own = [s.search(queries, 40) for s in stages]
    assert int((own[0][1] != own[1][1]).sum()) > 0
    got = hybrid.search(queries, 10)
    want = HybridSearch([Frozen(r) for r in own], 40).search(queries, 10)
    assert torch.equal(got[1], want[1]) and np.array_equal(_bits(got[0]), _bits(want[0]))
    print(f"[postings] two-stage and hybrid search over postings first stages: equal to rerank(search) and fuse(searches)")
