"""CPU: the launch plan of the index layer (polus_amd/ir): which entry points `add`, `search` and `rerank` of every index
reach, in which order, with which extents, strides, `id0`, `k` and `init`, and what the growing buffers hold where nothing
was written.

The indexes run on CPU tensors against tests.fakes.RecordingLib with the device check of the wrappers disabled, so nothing
is computed: the stub model hands back whatever batch it is given, and a buffer a kernel would have filled keeps what torch
allocated.  The expected lists are written out from the documented rules (a span holds min(65535, scratch_bytes // (4 Q))
columns; one scoring launch and one merge per span; `init` on the first span only), not captured from a run.  The routes that
copy a count from the device before sizing a buffer (the postings build, probing, SparseCorpusIndex.query_lists) cannot run
here, because the count is never written; the GPU tests cover them."""
import types

import numpy as np
import pytest
import torch

from tests import ops_contract_cases as oc
from tests.fakes import disable_device_check, recording_lib


@pytest.fixture(scope="module")
def real_lib():
    from polus_amd import build
    build.build(verbose=False)
    from polus_amd import _lib
    return _lib.load()


@pytest.fixture
def rec(real_lib, monkeypatch):
    disable_device_check(monkeypatch)
    yield from recording_lib(real_lib, monkeypatch, oc.STREAM)


class PassThrough:
    """A model whose encoders and projections return the batch itself: a test passes the representations it wants stored."""

    def encode_document(self, batch, training=False):
        return batch

    encode_query = document_projection = query_projection = encode_document


def reps(n, L, E=32):
    from polus_amd.ir.models import TokenReps
    return TokenReps(torch.zeros((n, L, E)), torch.ones((n, L), dtype=torch.int32))


def take(rec):
    """The calls recorded since the last take."""
    calls, rec.calls[:] = list(rec.calls), []
    return calls


def picked(call, *at):
    return tuple(call[1][i] for i in at)


# polus_topk_merge(scores, ld, rows, n, id0, top_val, top_id, k, init, stream)
MERGE = (1, 2, 3, 4, 7, 8)
# polus_topk_merge_ids(scores, ld, ids, ld_ids, rows, n, top_val, top_id, k, init, stream)
MERGE_IDS = (1, 3, 4, 5, 8, 9)
SPANS = [(0, 2), (2, 4), (4, 5)]


def check_scan(calls, score_name, score_at, score_want, Q, ld, k, spans=SPANS):
    """One scoring launch and one polus_topk_merge per span: id0 the span's start, init on the first span only."""
    assert [n for n, _ in calls] == [score_name, "polus_topk_merge"] * len(spans)
    for i, (a, b) in enumerate(spans):
        assert picked(calls[2 * i], *score_at) == score_want(b - a), (score_name, a, b)
        assert picked(calls[2 * i + 1], *MERGE) == (ld, Q, b - a, a, k, 1 if i == 0 else 0), ("polus_topk_merge", a, b)


# ------------------------------------------------------------------------------------------------- [CLS]
def test_cls_index_regrows_and_scans_in_three_spans(rec):
    from polus_amd.ir.search import CorpusIndex
    ix = CorpusIndex(PassThrough(), object(), scratch_bytes=3200)
    pattern = torch.arange(250 * 32, dtype=torch.float32).view(250, 32)
    assert ix.add(pattern[:100]).tolist() == list(range(100))
    assert ix.add(pattern[100:]).tolist() == list(range(100, 250))              # 250 > 2 * 100: the buffer is replaced
    assert len(ix) == 250 and ix.tokens is False and take(rec) == []
    assert torch.equal(ix.representations[:100], pattern[:100]) and torch.equal(ix.representations, pattern)
    assert ix.nbytes == 250 * 32 * 4
    assert ix.chunks(8) == [(0, 100), (100, 200), (200, 250)]                   # 3200 // (4 * 8) = 100 columns
    val, ids = ix.search(torch.zeros((8, 32)), 7)
    assert (val.shape, val.dtype, ids.shape, ids.dtype) == ((8, 7), torch.float32, (8, 7), torch.int32)
    # polus_gemm(dt, a_layout, b_layout, out_dt, a, lda, b, ldb, out, ldo, M, N, K, ...): queries x documents of the span
    check_scan(take(rec), "polus_gemm", (5, 7, 9, 10, 11, 12), lambda n: (32, 32, 100, 8, n, 32), Q=8, ld=100, k=7,
               spans=[(0, 100), (100, 200), (200, 250)])


# ------------------------------------------------------------------------------------------------- tokens, plain and FP8
@pytest.mark.parametrize("storage", [None, "fp8"])
def test_token_index_pads_a_short_batch_and_scans_in_three_spans(storage, rec):
    from polus_amd.ir.search import CorpusIndex
    ix = CorpusIndex(PassThrough(), object(), scratch_bytes=16, storage=storage)
    ix.add(reps(3, 4))
    ix.add(reps(2, 3))                                                          # shorter than the index's 4: padded
    # polus_fp8_quantize_rows(dt, x, codes, scale, rows, E, stream): one per add, over the batch as it came
    quantised = [picked(c, 4, 5) for c in take(rec)]
    assert quantised == ([] if storage is None else [(12, 32), (6, 32)])
    assert len(ix) == 5 and ix.tokens is True
    assert ix.mask.tolist() == [[1, 1, 1, 1]] * 3 + [[1, 1, 1, 0]] * 2
    if storage == "fp8":
        assert ix.codes.shape == (5, 4, 32) and ix.codes.dtype == torch.uint8 and ix.scales.shape == (5, 4)
        assert ix.scales[3:, 3].tolist() == [0.0, 0.0] and not ix.codes[3:, 3].any()
        assert ix.nbytes == 5 * 4 * (32 + 4 + 4)
    else:
        assert ix.codes is None and ix.scales is None and ix.representations.shape == (5, 4, 32)
        assert ix.nbytes == 5 * 4 * (32 * 4 + 4)
    take(rec)                                                                   # (an FP8 `representations` dequantises)
    with pytest.raises(ValueError, match="does not fit the index's document length 4"):
        ix.add(reps(1, 5))
    assert ix.chunks(2) == SPANS                                                # 16 // (4 * 2) = 2 columns
    q = reps(2, 2)
    ix.search(q, 3)
    if storage is None:
        # polus_maxsim_scores(dt, q, d, qmask, dmask, score, ld, B, N, Lq, Ld, E, stream)
        check_scan(take(rec), "polus_maxsim_scores", (6, 7, 8, 9, 10, 11), lambda n: (2, 2, n, 2, 4, 32), Q=2, ld=2, k=3)
    else:
        # polus_maxsim_scores_fp8(dt, q, codes, scale, qmask, dmask, score, ld, B, N, Lq, Ld, E, stream)
        check_scan(take(rec), "polus_maxsim_scores_fp8", (7, 8, 9, 10, 11, 12), lambda n: (2, 2, n, 2, 4, 32), Q=2, ld=2, k=3)


# ------------------------------------------------------------------------------------------------- rerank
def token_index():
    from polus_amd.ir.search import CorpusIndex
    ix = CorpusIndex(PassThrough(), object(), scratch_bytes=16)
    ix.add(reps(3, 4))
    ix.add(reps(2, 3))
    return ix


BAD_CANDIDATES = [
    (np.zeros((2, 5), np.float32), r"candidates must be integers \(got float32\)"),
    (np.array([[0, 1, 2, 3, 5]] * 2), r"candidates must lie in \[-1, 5\) \(got 0 \.\. 5\)"),
    (np.zeros((3, 5), np.int64), r"candidates must be \[2, C\] with C >= 1 \(got \(3, 5\)\)"),
]


def test_rerank_scores_candidate_columns_in_three_spans(rec):
    ix = token_index()
    take(rec)
    cand = np.array([[4, 0, -1, 2, 1], [3, -1, 1, 0, 2]], np.int64)             # on the host: checked, then copied as int32
    assert ix.rerank_chunks(2, 5) == SPANS
    val, ids = ix.rerank(reps(2, 2), cand, 3)
    assert (val.shape, val.dtype, ids.shape, ids.dtype) == ((2, 3), torch.float32, (2, 3), torch.int32)
    calls = take(rec)
    assert [n for n, _ in calls] == ["polus_maxsim_rerank", "polus_topk_merge_ids"] * 3
    for i, (a, b) in enumerate(SPANS):
        # polus_maxsim_rerank(dt, q, d, qmask, dmask, cand, ld_cand, score, ld_score, B, C, N, Lq, Ld, E, stream)
        assert picked(calls[2 * i], 6, 8, 9, 10, 11, 12, 13, 14) == (5, 2, 2, b - a, 5, 2, 4, 32)
        assert picked(calls[2 * i + 1], *MERGE_IDS) == (2, 5, 2, b - a, 3, 1 if i == 0 else 0)
    for bad, message in BAD_CANDIDATES:
        with pytest.raises(ValueError, match=message):
            ix.rerank(reps(2, 2), bad, 3)
    assert take(rec) == []


def test_cross_encoder_index_refuses_the_same_candidates(rec):
    from polus_amd.ir.cross import CrossEncoderIndex
    model = types.SimpleNamespace(arena=types.SimpleNamespace(device=torch.device("cpu")))
    cross = CrossEncoderIndex(model)
    cross.add({"input_ids": np.ones((3, 6), np.int32)})
    cross.add({"input_ids": np.ones((2, 4), np.int32)})                          # narrower: padded with masked tokens
    assert len(cross) == 5 and cross.nbytes == 5 * 6 * 8
    assert cross.mask.tolist() == [[1] * 6] * 3 + [[1, 1, 1, 1, 0, 0]] * 2 and not cross.token_ids[3:, 4:].any()
    queries = {"input_ids": np.ones((2, 4), np.int32)}
    for bad, message in BAD_CANDIDATES:
        with pytest.raises(ValueError, match=message):
            cross.score(queries, bad)
        with pytest.raises(ValueError, match=message):
            cross.rerank(queries, bad, 3)
    assert take(rec) == []


# ------------------------------------------------------------------------------------------------- residual
def test_residual_index_assigns_compresses_and_decodes_a_span_at_a_time(rec):
    from polus_amd.ir.search import CorpusIndex, ResidualCodec
    scorer = types.SimpleNamespace(normalize=True, eps=1e-12)
    codec = ResidualCodec(torch.zeros((4, 32)), np.array([-0.1, 0.0, 0.1]), np.array([-0.2, -0.05, 0.05, 0.2]), 2)
    # 512 bytes: one decoded document (4 tokens x 32 f32), and 32 rows of similarities to 4 centroids per assignment GEMM
    ix = CorpusIndex(PassThrough(), scorer, scratch_bytes=512, storage="residual", codec=codec)
    ix.add(reps(3, 4))
    calls = take(rec)
    assert [n for n, _ in calls] == ["polus_l2norm_fwd", "polus_gemm", "polus_centroid_codes", "polus_residual_compress"]
    assert picked(calls[1], 10, 11, 12) == (32, 4, 32)                          # [rows, E] x [K, E]^T at the fixed shape
    # polus_centroid_codes(sim, ld, mask, codes, rows, K, stream)
    assert picked(calls[2], 1, 4, 5) == (4, 12, 4)
    # polus_residual_compress(dt, x, codes, centroids, K, cutoffs, nbits, packed, rows, E, stream)
    assert picked(calls[3], 4, 6, 8, 9) == (4, 2, 12, 32)
    assert ix.residuals.shape == (3, 4, 8) and ix.residuals.dtype == torch.uint8 and not ix.residuals.any()
    # nothing ran, so every code slot is as it was allocated: 0xFFFF, "no token"
    assert ix.centroid_codes.dtype == torch.int16 and ix.centroid_codes.tolist() == [[-1] * 4] * 3
    assert ix.nbytes == 3 * 4 * (8 + 4 + 2) and ix.codes is None and ix.scales is None
    spans = [(0, 1), (1, 2), (2, 3)]
    assert ix.chunks(2, decode=True) == spans and ix.chunks(2) == [(0, 3)]
    ix.search(reps(2, 2), 2)
    calls = take(rec)
    assert [n for n, _ in calls] == ["polus_l2norm_fwd"] + ["polus_residual_decompress", "polus_maxsim_scores", "polus_topk_merge"] * 3
    for i, (a, b) in enumerate(spans):
        # polus_residual_decompress(dt, codes, packed, centroids, K, weights, nbits, y, rows, E, stream)
        assert picked(calls[1 + 3 * i], 4, 6, 8, 9) == (4, 2, 4, 32)
        assert picked(calls[2 + 3 * i], 6, 7, 8, 9, 10, 11) == (1, 2, 1, 2, 4, 32)
        assert picked(calls[3 + 3 * i], *MERGE) == (1, 2, 1, a, 2, 1 if i == 0 else 0)
    ix.scratch_bytes = 511
    with pytest.raises(ValueError, match=r"scratch_bytes = 511 does not hold one decoded document \(512 bytes\)"):
        ix.chunks(2, decode=True)


# ------------------------------------------------------------------------------------------------- sparse and BM25, forward route
# polus_sparse_scores(q, ldq, ids, ld_ids, w, ldw, score, ld_score, B, N, M, V, stream)
SPARSE_AT = (1, 3, 5, 7, 8, 9, 10, 11)


def test_sparse_index_keeps_terms_and_scans_in_three_spans(rec):
    from polus_amd.ir.search import SparseCorpusIndex
    sp = SparseCorpusIndex(PassThrough(), terms=4, scratch_bytes=16)
    sp.add(torch.zeros((3, 64)))
    sp.add(torch.zeros((2, 64)))                                                # 5 > 3: room for 6
    calls = take(rec)
    assert [n for n, _ in calls] == ["polus_topk_merge"] * 2                    # a document's terms: one row of the merge each
    assert [picked(c, *MERGE) for c in calls] == [(64, 3, 64, 0, 4, 1), (64, 2, 64, 0, 4, 1)]
    assert len(sp) == 5 and sp.term_ids.shape == (5, 4) and sp.weights.shape == (5, 4) and sp.nbytes == 5 * 4 * 8
    assert sp._ids.shape == (6, 4) and sp._ids[5].tolist() == [-1] * 4 and sp._w[5].tolist() == [0.0] * 4
    assert sp.chunks(2) == SPANS
    sp.search(torch.zeros((2, 64)), 3)
    check_scan(take(rec), "polus_sparse_scores", SPARSE_AT, lambda n: (64, 4, 4, 2, 2, n, 4, 64), Q=2, ld=2, k=3)


def test_bm25_index_counts_refreshes_and_scans_in_three_spans(rec, monkeypatch):
    from polus_amd.ir import lexical
    monkeypatch.setattr(lexical, "device", lambda: torch.device("cpu"))
    bm = lexical.BM25Index(64, terms=4, strip=(0, 0), scratch_bytes=16)
    bm.add({"input_ids": np.ones((3, 6), np.int32)})
    bm.add({"input_ids": np.ones((2, 6), np.int32)})
    calls = take(rec)
    # polus_bm25_term_counts(ids, ld, mask, ldm, n, L, V, head, tail, terms, ldt, tf, ldf, M, doc_len, df, stats, stream)
    assert [n for n, _ in calls] == ["polus_bm25_term_counts"] * 2
    assert [picked(c, 1, 4, 5, 6, 7, 8, 10, 12, 13) for c in calls] == [(6, 3, 6, 64, 0, 0, 4, 4, 4), (6, 2, 6, 64, 0, 0, 4, 4, 4)]
    assert len(bm) == 5 and bm.nbytes == 5 * (12 * 4 + 4) + 4 * 64 + 24
    # the kernel writes the slots in place, so here every stored slot is as allocated: (-1, 0), and so is the spare row
    assert bm.term_ids.tolist() == [[-1] * 4] * 5 and bm.counts.tolist() == [[0] * 4] * 5 and bm.doc_lengths.tolist() == [0] * 5
    assert bm._terms.shape == (6, 4) and bm._terms[5].tolist() == [-1] * 4 and bm._w[5].tolist() == [0.0] * 4
    assert bm.chunks(2) == SPANS
    bm.search({"input_ids": np.ones((2, 3), np.int32)}, 3)
    calls = take(rec)
    # stale after the adds: one refresh of the weights, then the queries are counted and made dense rows
    assert [n for n, _ in calls[:3]] == ["polus_bm25_weights", "polus_bm25_term_counts", "polus_bm25_query"]
    # polus_bm25_weights(tf, ldf, doc_len, w, ldw, n, M, c0, c1, k1p1, stream)
    assert picked(calls[0], 1, 4, 5, 6) == (4, 4, 5, 4)
    assert picked(calls[1], 1, 4, 5, 6, 13) == (3, 2, 3, 64, 3) and calls[1][1][15] is None and calls[1][1][16] is None
    # polus_bm25_query(terms, ldt, tf, ldf, idf, q, ldq, B, M, V, stream)
    assert picked(calls[2], 1, 3, 6, 7, 8, 9) == (3, 3, 64, 2, 3, 64)
    check_scan(calls[3:], "polus_sparse_scores", SPARSE_AT, lambda n: (64, 4, 4, 2, 2, n, 4, 64), Q=2, ld=2, k=3)
    bm.search({"input_ids": np.ones((2, 3), np.int32)}, 3)
    assert [n for n, _ in take(rec)][:2] == ["polus_bm25_term_counts", "polus_bm25_query"], "fresh weights are not recomputed"


# ------------------------------------------------------------------------------------------------- the chunk rule
def chunkers():
    from polus_amd.ir.lexical import BM25Index
    from polus_amd.ir.search import CorpusIndex, SparseCorpusIndex

    def index(make):
        def spans(total, Q, scratch_bytes):
            ix = make(scratch_bytes)
            ix._n = total
            return ix.chunks(Q)
        return spans

    return {
        "CorpusIndex.chunks": index(lambda sb: CorpusIndex(None, object(), scratch_bytes=sb)),
        "CorpusIndex.chunks[fp8]": index(lambda sb: CorpusIndex(None, object(), scratch_bytes=sb, storage="fp8")),
        "SparseCorpusIndex.chunks": index(lambda sb: SparseCorpusIndex(None, scratch_bytes=sb)),
        "BM25Index.chunks": index(lambda sb: BM25Index(100, scratch_bytes=sb)),
        "CorpusIndex.rerank_chunks": lambda total, Q, sb: CorpusIndex(None, object(), scratch_bytes=sb).rerank_chunks(Q, total),
    }


@pytest.mark.parametrize("name", ["CorpusIndex.chunks", "CorpusIndex.chunks[fp8]", "SparseCorpusIndex.chunks", "BM25Index.chunks",
                                  "CorpusIndex.rerank_chunks"])
def test_every_chunk_method_follows_the_one_rule(name):
    spans = chunkers()[name]
    assert spans(250, 8, 3200) == [(0, 100), (100, 200), (200, 250)]
    assert spans(250, 8, 3231) == [(0, 100), (100, 200), (200, 250)], "a part of a column does not count"
    assert spans(5, 2, 16) == SPANS
    assert spans(100, 8, 3200) == [(0, 100)] and spans(0, 8, 3200) == []
    assert spans(140000, 1, 1 << 40) == [(0, 65535), (65535, 131070), (131070, 140000)], "at most 65535 columns per launch"
    what = "candidate" if name.endswith("rerank_chunks") else "document"
    with pytest.raises(ValueError, match=rf"scratch_bytes = 31 does not hold the scores of one {what} for 8 queries \(32 bytes\)"):
        spans(250, 8, 31)
