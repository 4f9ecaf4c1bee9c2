"""Corpus search for the dual encoders of polus_amd/ir: encode and store a corpus, score queries against it in chunks
with the kernels the trainer uses, keep an exact running top-k on the device, and drive a validation loop with it.

    index = CorpusIndex(model, compute_scores)          # the trainer's model and scorer
    for docs in corpus_batches: index.add(docs)         # {"input_ids", "attention_mask"}
    scores, ids = index.search(queries, k=100)          # f32 / int32 [Q, k] on the device

A token (late-interaction) index scores every document for every query, so its search is linear in the corpus.  Its
other mode is re-ranking: a cheap first stage proposes candidates per query and MaxSim scores only those.

    scores, ids = index.rerank(queries, candidates, k=100)           # candidates [Q, C], padded with -1
    two = TwoStageSearch(cls_index, token_index, candidates=1000)    # first.search, then second.rerank
    scores, ids = two.search(queries, k=100)

A token index can be stored compressed, `CorpusIndex(..., storage="fp8")`: per document token E bytes of OCP e4m3fn
codes and one f32 power-of-two scale beside the int32 mask, E + 8 bytes against 2 E + 4 in bf16 (0.52 at E = 128).
`add` projects, normalises and then quantises (ops.fp8_quantize); `search` and `rerank` score the codes directly
(ops.maxsim_scores_fp8 / ops.maxsim_rerank_fp8), bit for bit what a plain index holding the dequantised vectors
returns, so the quantiser's rounding (about 3 % relative L2 per unit vector) is the only difference from a plain index.

A token index whose scorer normalises (MaxSimScores(normalize=True)) can also prune its own search, without a second
model (ColBERTv2 / PLAID candidate generation): every stored token carries the 16-bit id of its nearest centroid, a
query token's similarity to all K centroids is one GEMM, and MaxSim is approximated by table look-ups
(ops.centroid_scores), one gathered load and one max per token pair where the exact score spends E multiply-adds.

    index.fit_centroids(1024)                           # spherical k-means on the device, or index.set_centroids(c)
    scores, ids = index.search_pruned(queries, k=100, candidates=1000)

The best `candidates` documents under the approximation go through `rerank`.  What is exact: every returned score is
the MaxSim score of its document with the bits `search` gives it, and the returned documents are in `search`'s order.
What is approximate: WHICH documents get scored; a document the look-up score ranks below `candidates` is never
seen, however good its exact score.  How often that happens (recall against `search`) depends on K, `candidates`
and the data; it has not been measured on a real collection.  With candidates >= len(index) the result is `search`'s.

That search still computes the look-up score of every stored document.  With `nprobe` it does not: inverted lists
(centroid -> the documents holding a token of it; built on first use, rebuilt after `add` or new centroids) name the
documents worth scoring, those sharing a centroid with the `nprobe` nearest centroids of some query token, and the
look-up scores are computed for them alone (ops.ivf_* and ops.centroid_scores_ids), with the bits the scan gives them.

    scores, ids = index.search_pruned(queries, k=100, candidates=1000, nprobe=4)
    probes, cand, count = index.probe(queries, nprobe=4)          # the candidates alone, e.g. for a cross-encoder

A document without a present token is in no list, so `nprobe` never returns it (the scan ranks it with score 0.0); with
nprobe = K and no such document the result is the scan's, bit for bit.  Not measured: probed search beyond the
benchmark's 40 000 documents, and recall on a real collection.

With centroids a token index can drop the full vectors altogether (ColBERTv2's residual compression): a token is stored
as its centroid's 16-bit id plus nbits = 1, 2 or 4 bits per dimension naming a bucket of its residual, 2 + E * nbits / 8
bytes beside the int32 mask: 38 at E = 128 and nbits = 2, against 260 in bf16 and 136 in FP8.

    codec = index.fit_codec(2)                          # on a plain or FP8 "training" index that has centroids
    small = CorpusIndex(model, compute_scores, storage="residual", codec=codec)
    for docs in corpus_batches: small.add(docs)         # project, normalise, nearest centroid, compress

`rerank`, `search_pruned` and TwoStageSearch score the compressed tokens directly (ops.maxsim_rerank_res decodes
centroid + bucket weight in registers), bit for bit what a plain index holding the decoded vectors returns; `search`
decodes a chunk at a time into scratch and runs ops.maxsim_scores (a pruned search never touches the residual bits of
a document it does not rerank, and with `nprobe` not even its codes, so there is no exhaustive kernel over residual
bits).  All of the error is the quantiser's.  Recall and score error of 1-, 2- and 4-bit
residuals have not been measured on any real collection here.

A [CLS] index can be stored product-quantised (Jegou et al.): a vector of E = m * dsub features becomes m bytes, each
naming one of ksub <= 256 codewords of its sub-space, 96 bytes against 1536 at E = 768 in bf16 with dsub = 8.

    codec = index.fit_pq(96)                            # Lloyd rounds on the device, on a plain [CLS] "training" index
    small = CorpusIndex(model, compute_scores, post_process_logits, storage="pq", codec=codec)
    for docs in corpus_batches: small.add(docs)         # project, post-process, nearest codeword per sub-space

`search` computes every query's dot products with all m * ksub codewords once (ops.pq_lut) and scores a document by m
table look-ups (ops.pq_scores, the asymmetric-distance scan): the score is the dot product of the query with the
DECODED vector, summed per sub-space first, so all of the error against a plain index is the quantiser's.  Order, ties
and padding are `search`'s own.  Recall against the exact search has not been measured on any real collection.

A PQ index still scans every document.  An IVF-PQ index (Jegou et al., "IVFADC", FAISS' IVFPQ layout, here for inner
products) does not have to: a coarse quantiser of K centroids splits the corpus into K lists, a document is stored as
the 16-bit id of its L2-nearest centroid plus the m PQ bytes of its RESIDUAL against it (m + 2 bytes), and a search
scores only the lists of the `nprobe` centroids with the largest dot product with the query.

    codec = index.fit_ivfpq(1024, 96)                   # coarse Lloyd rounds, then PQ Lloyd rounds on the residuals
    small = CorpusIndex(model, compute_scores, post_process_logits, storage="ivfpq", codec=codec, nprobe=16)
    for docs in corpus_batches: small.add(docs)         # project, post-process, nearest centroid, residual, encode
    scores, ids = small.search(queries, k=100)          # or search(queries, 100, nprobe=4); nprobe unset: every document

The score of a document is <q, centroid> + the look-up sum over its residual codes (ops.ivfpq_scores_ids): the dot
product with centroid + decoded residual, the same bits whether it is reached by a probe or by the exhaustive scan, so
with nprobe = K the result is the exhaustive one, bit for bit.  What is approximate under `nprobe`: WHICH documents are
scored.  Because `search(queries, k)` falls back to the index's own `nprobe`, TwoStageSearch, HybridSearch and
mine_negatives get a probed first stage unchanged.  Recall on a real collection has not been measured.

A [CLS] index can keep a refine store, the vectors an exact second look scores (FAISS' IndexRefine, ScaNN's reordering):

    plain = CorpusIndex(model, compute_scores, post_process_logits, refine="full")     # its own vectors, nothing copied
    scores, ids = plain.rerank(queries, candidates, k=100)                             # e.g. TwoStageSearch(bm25, plain, 1000)
    small = CorpusIndex(model, compute_scores, post_process_logits, storage="ivfpq", codec=codec, nprobe=16, refine="fp8")
    scores, ids = small.search(queries, k=100, candidates=400)                         # first stage for 400, re-scored, best 100

`rerank` scores each query against its own candidate ids with ops.cls_rerank (refine="full": the projected, post-processed
vectors in the model's dtype, beside PQ or IVF-PQ codes a second field of 2 E bytes in bf16) or ops.cls_rerank_fp8 ("fp8":
e4m3fn codes and one power-of-two scale per document, E + 4 bytes, quantised in `add` by ops.cls_fp8_quantize).  The sum's
order is a function of E alone (include/polus_hip.h "refine"), so a score's bits depend on its (query, document) pair only,
and the fp8 score is bit for bit the full score over the dequantised vectors.  The contract of `search` on a PQ or IVF-PQ
index with a refine store: every returned score is the refine rule's score of its document, with the bits `rerank` gives
that pair, in `rerank`'s order (score descending, ties to the lower id); WHICH documents are considered is approximate, the
first stage's best R = `candidates` under its look-up scores; under "fp8" all remaining score error is the quantiser's.
`search(..., candidates=...)` on an index without a refine store is an error, and an index built without `refine` behaves
bit for bit as before.  Recall against the exact search has not been measured on any real collection.

A learned sparse (SPLADE) first stage is a SparseCorpusIndex: per document its best (term id, weight) pairs, dense
queries, every document scored for every query (ops.sparse_scores).  With `postings=True` it searches block-inverted
postings instead (polus_amd/ir/postings.py has the format and the score rule): the dense queries become lists of their
non-zeros (ops.sparse_compact_rows), only the lists of a query's terms are read (ops.postings_scores), and
representations wider than 40 960 columns are accepted.

    sparse = SparseCorpusIndex(splade, terms=128, postings=True, query_terms=1024)
    scores, ids = sparse.search(queries, k=1000)        # the same contract; postings rebuilt when an add made them stale

As in ir/training.py, arithmetic is hand-written HIP (ops.gemm / ops.maxsim_scores / ops.maxsim_rerank,
ops.l2norm_fwd, ops.topk_merge, ops.centroid_scores / centroid_scores_ids / centroid_codes / centroid_update,
ops.ivf_count / ivf_offsets / ivf_fill / ivf_mark / ivf_compact, ops.residual_compress /
residual_decompress / maxsim_rerank_res, ops.pq_encode / pq_update / pq_decode / pq_lut / pq_scores,
ops.ivfpq_residual / ivfpq_coarse_update / ivfpq_scores_ids, ops.cls_rerank / cls_rerank_fp8 / cls_fp8_quantize /
cls_fp8_dequantize); torch allocates, views and copies.  Data parallelism: every rank holds the whole
index and searches its own shard of the queries; ValidationDataCallback gathers the predictions."""
import numpy as np
import torch

from .. import ops
from ..callbacks import ValidationDataCallback
from .models import TokenReps
from .postings import Postings, check_block_docs
from .store import RowStore, check_candidates, score_chunks, stored, stored_rows, topk_scan

MAX_K = 1024                  # results per query: the limit of ops.topk_merge
MAX_CENTROIDS = 65535         # codes are 16 bits and 0xFFFF is "no token"
ASSIGN_ROWS = 16384           # tokens per nearest-centroid GEMM, at most (see CorpusIndex._assign_rows)
PQ_MAX_M = 160                # bytes per product-quantised vector: one query's table of 160 sub-spaces fills a CU's LDS


class ResidualCodec:
    """What turns a token vector into its centroid id plus `nbits` bits per dimension and back (ColBERTv2; the rules
    are include/polus_hip.h polus_residual_compress): `centroids` [K, E] (a tensor, 1 <= K <= 65535), `nbits` 1, 2 or
    4, `cutoffs` f32 [2^nbits - 1], non-decreasing: a residual element's bucket is the number of cutoffs below it, and
    `weights` f32 [2^nbits], what a bucket decodes to.  CorpusIndex.fit_codec makes one from a sample of a corpus."""

    def __init__(self, centroids, cutoffs, weights, nbits):
        if nbits not in (1, 2, 4):
            raise ValueError(f"nbits must be 1, 2 or 4 (got {nbits!r})")
        c = centroids if isinstance(centroids, torch.Tensor) else torch.as_tensor(np.ascontiguousarray(centroids))
        if c.dim() != 2 or not 1 <= c.shape[0] <= MAX_CENTROIDS or c.shape[1] % 32 or not 32 <= c.shape[1] <= 256:
            raise ValueError(f"centroids must be [K, E] with 1 <= K <= {MAX_CENTROIDS} and E a multiple of 32 in "
                             f"[32, 256] (got {tuple(c.shape)})")
        cut = torch.as_tensor(np.ascontiguousarray(np.asarray(cutoffs.cpu() if isinstance(cutoffs, torch.Tensor) else cutoffs,
                                                              dtype=np.float32)))
        w = torch.as_tensor(np.ascontiguousarray(np.asarray(weights.cpu() if isinstance(weights, torch.Tensor) else weights,
                                                            dtype=np.float32)))
        if tuple(cut.shape) != ((1 << nbits) - 1,):
            raise ValueError(f"cutoffs must be [{(1 << nbits) - 1}] for nbits = {nbits} (got {tuple(cut.shape)})")
        if tuple(w.shape) != (1 << nbits,):
            raise ValueError(f"weights must be [{1 << nbits}] for nbits = {nbits} (got {tuple(w.shape)})")
        if not bool((cut[1:] >= cut[:-1]).all()) or bool(torch.isnan(cut).any()):
            raise ValueError("cutoffs must be non-decreasing (and not NaN)")
        self.centroids, self.cutoffs, self.weights, self.nbits = c, cut, w, int(nbits)


class PQCodec:
    """What turns a single ([CLS]) vector of E = m * dsub elements into m bytes and back (product quantisation; the
    format and rules are include/polus_hip.h polus_pq_encode): `codebooks` f32 [m, ksub, dsub], an array or a tensor,
    codeword c of sub-space j in codebooks[j, c]; m a multiple of 4 in [4, 160], 1 <= ksub <= 256, 1 <= dsub <= 32.
    CorpusIndex.fit_pq makes one from a sample of a corpus."""

    def __init__(self, codebooks):
        c = codebooks if isinstance(codebooks, torch.Tensor) else torch.as_tensor(np.ascontiguousarray(codebooks))
        if c.dim() != 3 or c.dtype != torch.float32:
            raise ValueError(f"codebooks must be f32 [m, ksub, dsub] (got {c.dtype} {tuple(c.shape)})")
        m, ksub, dsub = c.shape
        if not 4 <= m <= PQ_MAX_M or m % 4 or not 1 <= ksub <= 256 or not 1 <= dsub <= 32:
            raise ValueError(f"codebooks [m, ksub, dsub] need m a multiple of 4 in [4, {PQ_MAX_M}], 1 <= ksub <= 256 and "
                             f"1 <= dsub <= 32 (got {tuple(c.shape)})")
        self.codebooks = c.contiguous()
        self.m, self.ksub, self.dsub, self.E = int(m), int(ksub), int(dsub), int(m * dsub)


def _half_norms(centroids):
    """f32 [K] on the host: -|c|^2 / 2 per row of `centroids` (a tensor), summed in float64 and rounded once.  As the bias of
    the similarity GEMM it turns the arg-max over centroids into the L2-nearest one: |x - c|^2 = |x|^2 - 2 (x.c - |c|^2 / 2)."""
    c = centroids.detach().float().cpu().numpy().astype(np.float64)
    return torch.as_tensor((-0.5 * (c * c).sum(axis=1)).astype(np.float32))


class IVFPQCodec:
    """What turns a single ([CLS]) vector into the 16-bit id of its L2-nearest coarse centroid plus the m PQ bytes of its
    residual against that centroid, and back (the format and rules are include/polus_hip.h "IVF-PQ"): `centroids` [K, E],
    an array or a tensor, 1 <= K <= 65535, cast to the index's dtype when the index stores them; `codebooks` f32
    [m, ksub, dsub] with PQCodec's limits and m * dsub == E.  `half_norms` f32 [K] = -|c|^2 / 2, computed once on the
    host in float64.  CorpusIndex.fit_ivfpq makes one from a sample of a corpus."""

    def __init__(self, centroids, codebooks):
        pq = PQCodec(codebooks)
        c = centroids if isinstance(centroids, torch.Tensor) else torch.as_tensor(np.ascontiguousarray(centroids))
        if c.dim() != 2 or not 1 <= c.shape[0] <= MAX_CENTROIDS or not c.dtype.is_floating_point:
            raise ValueError(f"centroids must be a floating-point [K, E] with 1 <= K <= {MAX_CENTROIDS} (got {c.dtype} "
                             f"{tuple(c.shape)})")
        if c.shape[1] != pq.E:
            raise ValueError(f"centroids have {c.shape[1]} features, the codebooks quantise {pq.E} ({pq.m} x {pq.dsub})")
        self.centroids, self.codebooks = c.contiguous(), pq.codebooks
        self.m, self.ksub, self.dsub, self.E, self.K = pq.m, pq.ksub, pq.dsub, pq.E, int(c.shape[0])
        self.half_norms = _half_norms(self.centroids)


class _ClsVectors:
    """What a CorpusIndex stores, chosen once (from `storage`, or at the first `add`).  A kind declares its fields of the
    index's RowStore, writes a projected batch, gives `search` the callback that scores a span of documents
    (store.topk_scan) and, for tokens, `rerank` the one that scores a span of candidate columns, returns
    `representations`, reads stored tokens back as vectors for the centroid code, and states the bytes of one document
    `search` decodes into scratch.  This one: [CLS] vectors [N, E] in the model's dtype, a span scored by one GEMM."""
    decoded_bytes = 0

    def __init__(self, ix):
        self.ix, self.store = ix, ix._store

    def fields(self, v):
        return dict(reps=(v.shape[1:], v.dtype, 0))

    def _room(self, v):
        """Rows a .. b for the batch v: the fields are declared by the first batch, the buffers hold b rows."""
        st = self.store
        if not st.fields:
            st.declare(**self.fields(v))       # fill 0: the padding of documents shorter than the index's length is never written
            if self.ix._refine is not None:
                st.declare(**self.ix._refine.fields(v))
        st.reserve(st.n + v.shape[0], v.device)
        self.dtype = v.dtype
        return st.n, st.n + v.shape[0]

    def write(self, v, m):
        a, b = self._room(v)
        self.store.bufs["reps"][a:b].copy_(v)

    def scorer(self, q):
        reps = self.store.bufs["reps"]
        return lambda a, b, s: ops.gemm(q, reps[a:b], s)

    def representations(self):
        return self.store.view("reps")


class _PqVectors(_ClsVectors):
    """The codec's codes uint8 [N, m] of [CLS] vectors.  `search` builds the queries' table once (ops.pq_lut) and a span is
    one look-up scan (ops.pq_scores); `representations` decodes."""

    def fields(self, v):
        return dict(reps=((self.ix.codec.m,), torch.uint8, 0))

    def write(self, v, m):
        codec = self.ix.codec
        if v.dim() != 2 or v.shape[1] != codec.E:
            raise ValueError(f"the codec quantises vectors of {codec.E} features ({codec.m} x {codec.dsub}), the model's "
                             f"have {tuple(v.shape[1:])}")
        a, b = self._room(v)
        self.cb = codec.codebooks.to(v.device)
        ops.pq_encode(v if v.stride(1) == 1 else v.contiguous(), self.cb, self.store.bufs["reps"][a:b])

    def scorer(self, q):
        codec, codes = self.ix.codec, self.store.bufs["reps"]
        lut = torch.empty((q.shape[0], codec.m, codec.ksub), dtype=torch.float32, device=q.device)
        ops.pq_lut(q, self.cb, lut)
        return lambda a, b, s: ops.pq_scores(lut, codes[a:b], s)

    def representations(self):
        codes = self.store.view("reps")
        y = torch.empty((codes.shape[0], self.ix.codec.E), dtype=self.dtype, device=codes.device)
        if codes.shape[0]:
            ops.pq_decode(codes, self.cb, y)
        return y


class _IvfPqVectors(_PqVectors):
    """The codec's coarse codes int16 [N] (fill -1 = 0xFFFF, "no list") and the PQ codes uint8 [N, m] of the residuals.  A
    span, or a list of candidate ids, is one look-up scan (ops.ivfpq_scores_ids) over the queries' table and their dot
    products with the centroids; `representations` decodes centroid + residual."""

    def fields(self, v):
        return dict(reps=((self.ix.codec.m,), torch.uint8, 0), coarse=((), torch.int16, -1))

    def write(self, v, m):
        ix, codec = self.ix, self.ix.codec
        if v.dim() != 2 or v.shape[1] != codec.E:
            raise ValueError(f"the codec quantises vectors of {codec.E} features ({codec.m} x {codec.dsub}), the model's "
                             f"have {tuple(v.shape[1:])}")
        a, b = self._room(v)
        if ix._centroids is None:
            ix._centroids = codec.centroids.to(device=v.device, dtype=v.dtype).contiguous().clone()
            self.cb, self.half_norms = codec.codebooks.to(v.device), codec.half_norms.to(v.device)
        v = v if v.stride(1) == 1 else v.contiguous()
        coarse = self.store.bufs["coarse"][a:b]
        ix._assign_rows(lambda s, e, dst: dst.copy_(v[s:e]), b - a, None, coarse, ix._centroids, bias=self.half_norms)
        r = torch.empty((b - a, codec.E), dtype=torch.float32, device=v.device)
        ops.ivfpq_residual(v, ix._centroids, coarse, r)
        ops.pq_encode(r, self.cb, self.store.bufs["reps"][a:b])

    def tables(self, q):
        """(lut f32 [Q, m, ksub], cdot f32 [Q, K]) of one search: the queries against the residual codewords and the centroids."""
        codec, cent = self.ix.codec, self.ix._centroids
        lut = torch.empty((q.shape[0], codec.m, codec.ksub), dtype=torch.float32, device=q.device)
        ops.pq_lut(q, self.cb, lut)
        cdot = torch.empty((q.shape[0], cent.shape[0]), dtype=torch.float32, device=q.device)
        ops.gemm(q, cent, cdot)
        return lut, cdot

    def scorer(self, q):
        lut, cdot = self.tables(q)
        coarse, codes = self.store.bufs["coarse"], self.store.bufs["reps"]
        return lambda a, b, s: ops.ivfpq_scores_ids(lut, cdot, coarse[a:b], codes[a:b], None, s)

    def list_codes(self):
        return self.store.view("coarse").view(-1, 1)             # the lists' CSR with one "token" per document

    def representations(self):
        """centroid + decoded residual, added in f32 and rounded once to the index's dtype (torch: an accessor, not a
        search path)."""
        codes, coarse = self.store.view("reps"), self.store.view("coarse")
        res = torch.empty((codes.shape[0], self.ix.codec.E), dtype=torch.float32, device=codes.device)
        if not codes.shape[0]:
            return res.to(self.dtype)
        ops.pq_decode(codes, self.cb, res)
        return (self.ix._centroids[coarse.to(torch.int64) & 0xFFFF].float() + res).to(self.dtype)


class _FullRefine:
    """The refine store of a [CLS] index in the model's dtype: the vectors `add` projected and post-processed, [N, E], which
    `rerank` scores with ops.cls_rerank.  On a plain index they ARE the stored vectors (field "reps": no second copy); beside
    PQ or IVF-PQ codes they are a field of their own, "rvec"."""

    def __init__(self, ix):
        self.ix, self.store, self.field = ix, ix._store, "reps" if ix.storage is None else "rvec"

    @staticmethod
    def check_width(E):
        if E % 16 or not 16 <= E <= 5120:
            raise ValueError(f"a refine store holds vectors of a multiple of 16 features in [16, 5120], the rows ops.cls_rerank "
                             f"reads in 16-byte pieces (got E = {E})")

    def fields(self, v):
        self.check_width(v.shape[1])
        return {} if self.field == "reps" else dict(rvec=((v.shape[1],), v.dtype, 0))

    def write(self, a, b, v):
        if self.field != "reps":
            self.store.bufs["rvec"][a:b].copy_(v)

    def reranker(self, q, cand):
        d = self.store.view(self.field)
        return lambda a, b, s: ops.cls_rerank(q, d, cand[:, a:b], s)

    def vectors(self, dtype):
        return self.store.view(self.field)

    codes = scales = property(lambda self: None)


class _Fp8Refine(_FullRefine):
    """The refine store as e4m3fn codes uint8 [N, E] ("rcodes") and one power-of-two scale f32 [N] ("rscale") per document,
    quantised by ops.cls_fp8_quantize in `add` and scored as they are by ops.cls_rerank_fp8."""

    def fields(self, v):
        self.check_width(v.shape[1])
        return dict(rcodes=((v.shape[1],), torch.uint8, 0), rscale=((), torch.float32, 0))

    def write(self, a, b, v):
        ops.cls_fp8_quantize(v.contiguous(), self.store.bufs["rcodes"][a:b], self.store.bufs["rscale"][a:b])

    def reranker(self, q, cand):
        codes, scale = self.store.view("rcodes"), self.store.view("rscale")
        return lambda a, b, s: ops.cls_rerank_fp8(q, codes, scale, cand[:, a:b], s)

    def vectors(self, dtype):
        codes = self.store.view("rcodes")
        if codes is None:
            return None
        y = torch.empty(codes.shape, dtype=dtype, device=codes.device)
        if codes.shape[0]:
            ops.cls_fp8_dequantize(codes, self.store.view("rscale"), y)
        return y

    codes = property(lambda self: self.store.view("rcodes"))
    scales = property(lambda self: self.store.view("rscale"))


class _Tokens(_ClsVectors):
    """Token vectors [N, Ld, E] in the model's dtype with their int32 mask [N, Ld]."""

    def fields(self, v):
        return dict(reps=((self.ix._ld, v.shape[2]), v.dtype, 0), mask=((self.ix._ld,), torch.int32, 0))

    def write(self, v, m):
        a, b = self._room(v)
        self.store.bufs["mask"][a:b, :v.shape[1]].copy_(m)
        self.put(a, b, v)
        if self.ix._centroids is not None:
            self.ix._assign(a, b)

    def put(self, a, b, v):
        self.store.bufs["reps"][a:b, :v.shape[1]].copy_(v)

    def list_codes(self):
        return self.store.view("codes")

    def scorer(self, q):
        reps, mask = self.store.bufs["reps"], self.store.bufs["mask"]
        return lambda a, b, s: ops.maxsim_scores(q.values, reps[a:b], q.mask, mask[a:b], s)

    def reranker(self, q, cand):
        reps, mask = self.store.view("reps"), self.store.view("mask")
        return lambda a, b, s: ops.maxsim_rerank(q.values, reps, q.mask, mask, cand[:, a:b], s)

    def loader(self, a, b):
        """load(s, e, dst) of CorpusIndex._assign_rows over the tokens of documents a .. b."""
        flat = self.store.bufs["reps"][a:b].view(-1, self.store.bufs["reps"].shape[2])
        return lambda s, e, dst: dst.copy_(flat[s:e])

    def gather(self, at):
        """The stored token slots `at` (int64 on the device; slot = document * Ld + position) as vectors [len(at), E]."""
        reps = self.store.view("reps")
        return reps.view(-1, reps.shape[2])[at].contiguous()


class _Fp8Tokens(_Tokens):
    """e4m3fn codes uint8 [N, Ld, E] and power-of-two scales f32 [N, Ld]; scored as they are, read back dequantised."""

    def fields(self, v):
        Ld = self.ix._ld
        return dict(reps=((Ld, v.shape[2]), torch.uint8, 0), mask=((Ld,), torch.int32, 0), scale=((Ld,), torch.float32, 0))

    def put(self, a, b, v):
        v = v.contiguous()
        codes = torch.empty(v.shape, dtype=torch.uint8, device=v.device)
        scale = torch.empty(v.shape[:-1], dtype=torch.float32, device=v.device)
        ops.fp8_quantize(v, codes, scale)
        self.store.bufs["scale"][a:b, :v.shape[1]].copy_(scale)
        self.store.bufs["reps"][a:b, :v.shape[1]].copy_(codes)

    def scorer(self, q):
        reps, scale, mask = (self.store.bufs[f] for f in ("reps", "scale", "mask"))
        return lambda a, b, s: ops.maxsim_scores_fp8(q.values, reps[a:b], scale[a:b], q.mask, mask[a:b], s)

    def reranker(self, q, cand):
        reps, scale, mask = (self.store.view(f) for f in ("reps", "scale", "mask"))
        return lambda a, b, s: ops.maxsim_rerank_fp8(q.values, reps, scale, q.mask, mask, cand[:, a:b], s)

    def _dequantized(self, codes, scale):
        y = torch.empty(codes.shape, dtype=self.dtype, device=codes.device)
        if codes.shape[0]:
            ops.fp8_dequantize(codes, scale, y)
        return y

    def representations(self):
        return self._dequantized(self.store.view("reps"), self.store.view("scale"))

    def loader(self, a, b):
        reps = self.store.bufs["reps"][a:b].view(-1, self.store.bufs["reps"].shape[2])
        scale = self.store.bufs["scale"][a:b].view(-1)
        return lambda s, e, dst: ops.fp8_dequantize(reps[s:e], scale[s:e], dst)

    def gather(self, at):
        reps = self.store.view("reps")
        return self._dequantized(reps.view(-1, reps.shape[2])[at].contiguous(), self.store.view("scale").view(-1)[at].contiguous())


class _ResidualTokens(_Tokens):
    """The codec's centroid codes int16 [N, Ld] and residual bits uint8 [N, Ld, E * nbits / 8]; reranked as they are.
    `search` has no kernel over residual bits (search_pruned never reads them in bulk): it decodes a span into scratch
    and runs the plain kernel.  Centroids cannot be set again, so nothing reads the tokens back (no loader, no gather)."""

    def fields(self, v):
        Ld = self.ix._ld
        return dict(reps=((Ld, v.shape[2] * self.ix.codec.nbits // 8), torch.uint8, 0), mask=((Ld,), torch.int32, 0),
                    codes=((Ld,), torch.int16, -1))                              # 0xFFFF: no token

    def write(self, v, m):
        """v [n, L, E] projected and normalised, m its mask.  The batch is padded to the index's length, its tokens get
        their codes by _assign_rows (the rule a plain index with these centroids follows in `add`) and
        ops.residual_compress writes the bits into the storage."""
        ix, codec = self.ix, self.ix.codec
        n, L, E = v.shape
        if codec.centroids.shape[1] != E:
            raise ValueError(f"the codec's centroids have {codec.centroids.shape[1]} features, the model's tokens {E}")
        if ix._centroids is None:
            ix._centroids = codec.centroids.to(device=v.device, dtype=v.dtype).contiguous().clone()
            ix._cutoffs, ix._weights = codec.cutoffs.to(v.device), codec.weights.to(v.device)
        a, b = self._room(v)
        mask = self.store.bufs["mask"][a:b]
        mask[:, :L].copy_(m)
        if L < ix._ld:
            x = torch.zeros((n, ix._ld, E), dtype=v.dtype, device=v.device)
            x[:, :L].copy_(v)
        else:
            x = v.contiguous()
        flat = x.view(-1, E)
        codes = self.store.bufs["codes"][a:b].view(-1)
        ix._assign_rows(lambda s, e, dst: dst.copy_(flat[s:e]), n * ix._ld, mask.view(-1), codes, ix._centroids)
        ops.residual_compress(x, codes, ix._centroids, ix._cutoffs, codec.nbits, self.store.bufs["reps"][a:b])

    @property
    def decoded_bytes(self):
        return self.ix._ld * self.ix._centroids.shape[1] * self.ix._centroids.element_size()

    def decoded(self, a, b, out=None):
        """Documents a .. b decoded into `out` (or a new tensor) [b - a, Ld, E]."""
        ix, bufs = self.ix, self.store.bufs
        y = out if out is not None else torch.empty((b - a, ix._ld, ix._centroids.shape[1]), dtype=self.dtype,
                                                    device=ix._centroids.device)
        if b > a:
            ops.residual_decompress(bufs["codes"][a:b], bufs["reps"][a:b], ix._centroids, ix._weights, ix.codec.nbits, y)
        return y

    def representations(self):
        return self.decoded(0, self.store.n)

    def scorer(self, q):
        mask = self.store.bufs["mask"]
        width = max(b - a for a, b in self.ix.chunks(q.values.shape[0], decode=True))
        dec = torch.empty((width, self.ix._ld, q.values.shape[2]), dtype=self.dtype, device=q.values.device)
        return lambda a, b, s: ops.maxsim_scores(q.values, self.decoded(a, b, dec[:b - a]), q.mask, mask[a:b], s)

    def reranker(self, q, cand):
        ix, codes, reps, mask = self.ix, self.store.view("codes"), self.store.view("reps"), self.store.view("mask")
        return lambda a, b, s: ops.maxsim_rerank_res(q.values, codes, reps, ix._centroids, ix._weights, ix.codec.nbits,
                                                     q.mask, mask, cand[:, a:b], s)


class CorpusIndex:
    """Projected document representations in one contiguous device buffer, [N, E] ([CLS], DualEncoder) or [N, Ld, E]
    with an int32 mask [N, Ld] (tokens, LateInteractionDualEncoder), in the model's compute dtype.

    `compute_scores` is the trainer's InBatchDotScores or MaxSimScores; `normalize` and `eps` are taken from it.
    `post_process_logits` is the trainer's hook for [CLS] vectors, applied to queries and documents as the trainer
    applies it; token representations refuse it, as the trainer does.  `scratch_bytes` bounds the [Q, n] f32 score
    buffer of one chunk.  `storage` is None (the model's compute dtype) or "fp8" (token representations only: e4m3fn
    codes uint8 [N, Ld, E] and power-of-two scales f32 [N, Ld], include/polus_hip.h polus_fp8_quantize_rows) or
    "residual" (token representations under a scorer that normalises: the centroid codes int16 [N, Ld] of `codec`, a
    ResidualCodec, and uint8 [N, Ld, E * nbits / 8] residual bits, polus_residual_compress; on it `scratch_bytes` also
    bounds the decoded vectors of one chunk of `search`) or "pq" ([CLS] representations only: the m bytes uint8 [N, m] of
    `codec`, a PQCodec, polus_pq_encode; `search` scores them by table look-ups, at most 65535 queries a call) or "ivfpq"
    ([CLS] representations only: per document the coarse code int16 and the m bytes of its residual under `codec`, an
    IVFPQCodec; `nprobe`, which only this storage takes, is the number of lists `search` probes when the call names
    none: None scores every document).

    `refine` gives a [CLS] index a refine store, the vectors `rerank` scores exactly (ops.cls_rerank): "full" keeps the
    projected, post-processed vectors in the model's dtype (on storage=None they are the stored vectors themselves, nothing
    is copied; beside PQ or IVF-PQ codes 2 E or 4 E more bytes per document), "fp8" keeps them as e4m3fn codes with one
    power-of-two scale per document (E + 4 bytes; PQ and IVF-PQ only: a plain index searches exactly already).  On a PQ or
    IVF-PQ index `search` then asks its first stage for `candidates` documents per query (1 .. 1024; None: min(4 k, 1024)),
    re-scores them and returns the best k.  E must be a multiple of 16."""

    def __init__(self, model, compute_scores, post_process_logits=None, scratch_bytes=256 << 20, storage=None, codec=None,
                 nprobe=None, refine=None, candidates=None):
        if storage not in (None, "fp8", "residual", "pq", "ivfpq"):
            raise ValueError(f"storage must be None or 'fp8' or 'residual' or 'pq' or 'ivfpq' (got {storage!r})")
        want = {"residual": ResidualCodec, "pq": PQCodec, "ivfpq": IVFPQCodec}.get(storage)
        if (want is None) != (codec is None):
            raise ValueError("storage='residual' needs a codec (ResidualCodec, see CorpusIndex.fit_codec), storage='pq' "
                             "one (PQCodec, see CorpusIndex.fit_pq) and storage='ivfpq' one (IVFPQCodec, see "
                             "CorpusIndex.fit_ivfpq), and only those storages take one")
        if codec is not None and not isinstance(codec, want):
            raise ValueError(f"storage={storage!r}: codec must be a {want.__name__} (got {type(codec).__name__})")
        if storage == "residual" and not bool(getattr(compute_scores, "normalize", False)):
            raise ValueError("storage='residual' needs a scorer that normalises (MaxSimScores(normalize=True)): the "
                             "nearest centroid by dot product means something on unit vectors only")
        if nprobe is not None and storage != "ivfpq":
            raise ValueError(f"nprobe belongs to storage='ivfpq', whose search probes lists (got storage={storage!r}); a "
                             "token index takes it per call, search_pruned(..., nprobe)")
        if refine not in (None, "full", "fp8"):
            raise ValueError(f"refine must be None or 'full' or 'fp8' (got {refine!r})")
        if refine is not None and storage in ("fp8", "residual"):
            raise ValueError(f"refine belongs to a [CLS] index (storage=None, 'pq' or 'ivfpq'); storage={storage!r} holds token "
                             "representations, which rerank scores by MaxSim as they are")
        if refine == "fp8" and storage is None:
            raise ValueError("refine='fp8' belongs to storage='pq' or 'ivfpq': a plain [CLS] index searches its own vectors "
                             "exactly, and refine='full' lets it rerank them without a second copy")
        if refine is not None and codec is not None:
            _FullRefine.check_width(codec.E)
        if candidates is not None:
            if refine is None or storage is None:
                raise ValueError("candidates belongs to a storage='pq' or 'ivfpq' index with a refine store (refine='full' or "
                                 f"'fp8'), whose search re-scores that many first-stage results (got refine={refine!r}, "
                                 f"storage={storage!r})")
            self._check_candidates(candidates)
        self.storage, self.codec, self.refine = storage, codec, refine
        self.candidates = None if candidates is None else int(candidates)
        self.nprobe = None if nprobe is None else self._check_nprobe(nprobe, codec.K)
        self.model, self.compute_scores = model, compute_scores
        self.post_process_logits = post_process_logits
        self.scratch_bytes = int(scratch_bytes)
        self.normalize = bool(getattr(compute_scores, "normalize", False))
        self.eps = float(getattr(compute_scores, "eps", 1e-12))
        self.clear()

    def clear(self):
        """Empty the index (the storage is released; the next `add` fixes the document length again).  A residual
        index keeps its codec."""
        self._store = RowStore()
        self._refine = {"full": _FullRefine, "fp8": _Fp8Refine}[self.refine](self) if self.refine else None
        self._kind = {"fp8": _Fp8Tokens, "residual": _ResidualTokens, "pq": _PqVectors, "ivfpq": _IvfPqVectors}[self.storage](self) if self.storage else None
        self._centroids = None                        # [K, E]; the codes are the store's int16 [cap, Ld] field
        self._cutoffs = self._weights = None          # a residual index: the codec's tables on the device
        self._lists, self._lists_stale = None, False  # inverted lists (offsets, docs) of refresh_lists
        self.tokens = None            # True: token representations; fixed by the first add

    _n, _reps, _mask, _scale, _codes = stored_rows, stored("reps"), stored("mask"), stored("scale"), stored("codes")

    def __len__(self):
        return self._n

    @property
    def representations(self):
        """[N, E] or [N, Ld, E]: a view of the stored documents.  On an FP8 index a COPY: the codes dequantised into
        a new tensor of the model's dtype (exactly codes * scales); writing to it does not change the index.  On a
        PQ index a COPY as well: every vector decoded from its codes (ops.pq_decode), the vectors `search` scores up to
        the rounding of its sums, not the ones that were added; an IVF-PQ index adds the document's centroid to its decoded
        residual in f32 and rounds once to the index's dtype."""
        return None if self._reps is None else self._kind.representations()

    @property
    def pq_codes(self):
        """uint8 [N, m]: a view of the stored product-quantisation codes (a PQ index, or an IVF-PQ index: the codes of the
        residuals; None otherwise)."""
        return None if self.storage not in ("pq", "ivfpq") else self._store.view("reps")

    @property
    def coarse_codes(self):
        """int16 [N]: a view of the stored coarse codes, the bits of the unsigned centroid id (an IVF-PQ index; None
        otherwise)."""
        return self._store.view("coarse")

    @property
    def refine_vectors(self):
        """[N, E] in the index's dtype: the vectors `rerank` scores (an index with a refine store; None otherwise, and before
        the first add).  Under refine="full" a view (on a plain index the stored vectors themselves); under "fp8" a COPY,
        the codes dequantised (exactly codes * scales), as `representations` is on an FP8 token index."""
        return None if self._refine is None or self._reps is None else self._refine.vectors(self._kind.dtype)

    @property
    def refine_codes(self):
        """uint8 [N, E]: a view of the refine store's e4m3fn codes (refine="fp8"; None otherwise)."""
        return None if self._refine is None else self._refine.codes

    @property
    def refine_scales(self):
        """f32 [N]: a view of the refine store's per-document scales, exact powers of two (refine="fp8"; None otherwise)."""
        return None if self._refine is None else self._refine.scales

    @property
    def residuals(self):
        """uint8 [N, Ld, E * nbits / 8]: a view of the stored residual bits (a residual index; None otherwise)."""
        return None if self.storage != "residual" else self._store.view("reps")

    @property
    def codes(self):
        """uint8 [N, Ld, E]: a view of the stored e4m3fn codes (an FP8 index; None otherwise)."""
        return None if self.storage != "fp8" else self._store.view("reps")

    @property
    def scales(self):
        """f32 [N, Ld]: a view of the stored per-token scales, exact powers of two (an FP8 index; None otherwise)."""
        return self._store.view("scale")

    @property
    def centroids(self):
        """[K, E] in the index's dtype: the centroids of set_centroids / fit_centroids (None before).  A residual
        index: its codec's (as the codec holds them until the first `add` moves them to the device)."""
        if self._centroids is None and self.storage in ("residual", "ivfpq"):
            return self.codec.centroids
        return self._centroids

    @property
    def centroid_codes(self):
        """int16 [N, Ld]: a view of the stored tokens' nearest-centroid ids; the 16 bits are the unsigned code, so -1
        is 0xFFFF, "no token" (None before centroids exist)."""
        return self._store.view("codes")

    @property
    def nbytes(self):
        """Bytes of the stored representations, scales, mask and centroid codes of the len(index) documents, and of
        the inverted lists once a probed search has built them (4 (K + 1) + 4 P; an IVF-PQ index: N (m + 2), and P = N).  A
        refine store beside PQ or IVF-PQ codes counts: N E element sizes under "full", N (E + 4) under "fp8"."""
        return sum(t[:self._n].numel() * t.element_size() for t in self._store.bufs.values()) + sum(
            t.numel() * t.element_size() for t in self._lists or ())

    @property
    def mask(self):
        return self._store.view("mask")

    def _l2norm(self, x):
        y = torch.empty_like(x)
        r = torch.empty(x.shape[:-1], dtype=torch.float32, device=x.device)
        ops.l2norm_fwd(x, y, r, self.eps)
        return y

    def _check_kind(self, rep):
        tokens = isinstance(rep, TokenReps)
        if tokens and self.post_process_logits is not None:
            raise ValueError("post_process_logits does not apply to token representations: normalisation belongs "
                             "to the scorer (MaxSimScores(normalize=True))")
        if self.tokens is not None and tokens != self.tokens:
            raise ValueError("the index holds " + ("token" if self.tokens else "[CLS]") + " representations")
        if tokens and self.refine is not None:
            raise ValueError("refine belongs to a [CLS] index: token representations are what rerank scores by MaxSim, they "
                             "need no refine store")
        if self.storage in ("pq", "ivfpq"):
            if tokens:
                raise ValueError(f"storage={self.storage!r} holds single ([CLS]) vectors only: product quantisation is for "
                                 "one vector per document, a token index has storage='fp8' and 'residual'")
        elif self.storage is not None and not tokens:
            raise ValueError(f"storage={self.storage!r} holds token representations only; a [CLS] index stays in the "
                             "model's dtype or takes storage='pq' or 'ivfpq'")
        return tokens

    def add(self, documents):
        """Encode, project (and normalise) a batch of documents and append it; returns its ids, the consecutive int32
        positions in the index.  Token documents are padded with masked tokens to the length of the first batch;
        a longer batch raises ValueError.  An FP8 index quantises the projected (and normalised) vectors here; a
        residual index gives them their nearest centroid of the codec and compresses them; a PQ index stores the codes
        of the projected (and post-processed) vectors; an IVF-PQ index gives them their L2-nearest coarse centroid
        (ops.gemm with the bias -|c|^2 / 2, then ops.centroid_codes), takes the residual (ops.ivfpq_residual) and stores
        its codes (ops.pq_encode).  A PQ or IVF-PQ index with a refine store also keeps the projected (and post-processed)
        vector itself, as it is ("full") or quantised by ops.cls_fp8_quantize ("fp8")."""
        model = self.model
        rep = model.document_projection(model.encode_document(documents, training=False), training=False)
        if self._check_kind(rep):
            v, m = rep.values, rep.mask
            if self.normalize:
                v = self._l2norm(v.contiguous())
            L = v.shape[1]
            if self.tokens is None:
                self.tokens, self._ld = True, L
            if L > self._ld:
                raise ValueError(f"a document batch of {L} tokens does not fit the index's document length {self._ld} "
                                 "(fixed by the first add)")
        else:
            v, m = rep if self.post_process_logits is None else self.post_process_logits(rep), None
            self.tokens = False
        if self._kind is None:
            self._kind = (_Tokens if self.tokens else _ClsVectors)(self)
        self._kind.write(v, m)
        if self._refine is not None:
            self._refine.write(self._n, self._n + v.shape[0], v)
        ids = torch.arange(self._n, self._n + v.shape[0], dtype=torch.int32, device=v.device)
        self._n += v.shape[0]
        self._lists_stale = True
        return ids

    def chunks(self, Q, decode=False):
        """[(start, stop), ...]: the document ranges a search with Q queries scores, one launch each: at most 65535
        documents, and at most as many as keep the [Q, n] f32 scores within scratch_bytes (store.score_chunks).
        decode=True (what `search` asks for): on a residual index the chunk's decoded vectors [n, Ld, E] stay within
        scratch_bytes as well."""
        return score_chunks(self._n, Q, self.scratch_bytes, "document", self._kind.decoded_bytes if decode and self._n else 0)

    def encode_queries(self, queries):
        """The query side of the trainer: encode_query, query_projection, then the normalisation (tokens) or
        post_process_logits ([CLS])."""
        q = self.model.query_projection(self.model.encode_query(queries, training=False), training=False)
        if self._check_kind(q):
            v = q.values.contiguous()
            return TokenReps(self._l2norm(v) if self.normalize else v, q.mask.contiguous())
        return (q if self.post_process_logits is None else self.post_process_logits(q)).contiguous()

    def _check_candidates(self, candidates, k=1):
        if not int(k) <= int(candidates) <= MAX_K:
            raise ValueError(f"need {'1' if k == 1 else f'k = {k}'} <= candidates <= {MAX_K}, the limit of ops.topk_merge, which keeps "
                             f"the first stage's results (got {candidates})")
        return int(candidates)

    def search(self, queries, k, nprobe=None, candidates=None):
        """(scores f32 [Q, k], ids int32 [Q, k]) on the device: per query the k best documents, score descending, ties
        to the lower id; when the corpus holds fewer than k, the tail is (-inf, -1).

        `nprobe` (an IVF-PQ index only; None: the index's own `nprobe`): 1 <= nprobe <= min(K, 1024) scores only the
        documents in the lists of each query's nprobe best centroids by dot product (ties to the lower centroid), with the
        bits the exhaustive scan gives them; with fewer than k such documents the tail is (-inf, -1).  Both unset: every
        document is scored.

        A PQ or IVF-PQ index with a refine store runs that search, exhaustive or probed, for R = `candidates` (None: the
        index's own `candidates`, else min(4 k, 1024); k <= R <= 1024) results per query, re-scores those R documents
        against the refine store (`rerank`'s path, the queries encoded once) and returns the best k: every score is the
        refine rule's, with the bits `rerank` gives that pair; which documents were considered is the first stage's choice.
        `candidates` on any other index raises."""
        if nprobe is not None and self.storage != "ivfpq":
            raise ValueError(f"nprobe belongs to storage='ivfpq' (got storage={self.storage!r}); a token index takes it "
                             "in search_pruned(..., nprobe)")
        refined = self._refine is not None and self.storage is not None
        if candidates is not None and not refined:
            raise ValueError("candidates belongs to the search of a storage='pq' or 'ivfpq' index with a refine store "
                             f"(got refine={self.refine!r}, storage={self.storage!r}); a token index takes it in search_pruned")
        if self._n == 0:
            raise ValueError("the index is empty: add documents before searching")
        first = k
        if refined:
            R = candidates if candidates is not None else self.candidates
            first = self._check_candidates(min(4 * int(k), MAX_K) if R is None else R, int(k))
        nprobe = self.nprobe if nprobe is None else nprobe
        if nprobe is not None:
            nprobe = self._check_nprobe(nprobe)
        q = self.encode_queries(queries)
        if nprobe is not None:
            top = self._search_probed(q, first, nprobe)
        else:
            qv = q.values if self.tokens else q
            top = topk_scan(qv.shape[0], first, self.chunks(qv.shape[0], decode=True), qv.device, self._kind.scorer(q))
        return self._rerank_encoded(q, top[1], k) if refined else top

    def rerank_chunks(self, Q, C):
        """[(start, stop), ...]: the candidate columns one rerank launch scores: at most 65535, and at most as many as
        keep the [Q, c] f32 scores within scratch_bytes (store.score_chunks)."""
        return score_chunks(C, Q, self.scratch_bytes, "candidate")

    def rerank(self, queries, candidates, k):
        """Score every query against its own candidates only (a token index: MaxSim; a [CLS] index with a refine store:
        the dot product with the refine vectors, ops.cls_rerank / cls_rerank_fp8): (scores f32 [Q, k], ids int32 [Q, k]) on
        the device, the contract of `search` over the documents named in the query's row of `candidates`.

        `candidates` is an integer [Q, C] array of document ids, padded with -1 anywhere in a row.  A host array is
        checked: an id outside [-1, len(index)) raises ValueError.  A device tensor must be int32 (a wider id could
        not be narrowed without a look at it) and is taken as it is, values unseen: an id outside [0, len(index)) is
        absent.  The ids of a row should be distinct: the result is exact and independent of the chunking for
        distinct ids only.  A repeated id is scored once per copy and may come back more than once; how many of its
        copies return is not defined (ops.topk_merge).  A row without a candidate returns (-inf, -1)."""
        if self._n == 0:
            raise ValueError("the index is empty: add documents before re-ranking")
        if not self.tokens and self._refine is None:
            raise ValueError("rerank scores token representations (MaxSim) or the refine store of a [CLS] index; the index "
                             "holds [CLS] representations without one, whose search is already one GEMM: build it with "
                             "refine='full' (or, on storage='pq' / 'ivfpq', refine='fp8') to rerank candidates")
        return self._rerank_encoded(self.encode_queries(queries), candidates, k)

    def _rerank_encoded(self, q, candidates, k):
        """`rerank` behind the query encoder: q is what encode_queries returns, TokenReps or [CLS] vectors [Q, E]."""
        qv = q.values if self.tokens else q
        Q, dev = qv.shape[0], qv.device
        cand = check_candidates(candidates, Q, self._n, dev)
        rr = (self._kind if self.tokens else self._refine).reranker(q, cand)
        return topk_scan(Q, k, self.rerank_chunks(Q, cand.shape[1]), dev, rr, ids=cand)

    # ------------------------------------------------------------ centroid-pruned search
    def _check_centroid_support(self):
        if self.storage == "residual":
            raise ValueError("a residual index takes its centroids from its codec: the stored residuals belong to "
                             "them, so they cannot be set or fitted again")
        if self._n == 0:
            raise ValueError("the index is empty: add documents before setting or fitting centroids")
        if not self.tokens:
            raise ValueError("centroids prune a token (MaxSim) index; the index holds [CLS] representations, whose "
                             "search is already one GEMM")
        if not self.normalize:
            raise ValueError("centroids need a scorer that normalises (MaxSimScores(normalize=True)): the nearest "
                             "centroid by dot product means something on unit vectors only")

    def _assign_rows(self, load, T, mask, codes, centroids, bias=None):
        """codes[t] (int16 [T]) = the nearest row of `centroids` to token t, 0xFFFF where mask[t] == 0 (mask int32 [T]
        or None); load(a, b, dst) writes tokens a .. b into dst [b - a, E].  Nearest by dot product, or, with `bias`
        (f32 [K] = -|c|^2 / 2, added by the GEMM's epilogue), by L2 distance: the IVF-PQ assignment of whole vectors.  Every GEMM of a call runs at the same
        shape [rows, E] x [K, E]^T, rows = the largest power of two with rows * K * 4 <= scratch_bytes, at most
        ASSIGN_ROWS, the last chunk's tail being zero rows: ops.gemm picks its kernel from the shape, and kernels may
        sum in different orders, so a token's similarities, and with them its code at a near tie, depend on nothing
        but the token, the centroids and (through rows) K and scratch_bytes."""
        K, E = centroids.shape
        rows = ASSIGN_ROWS
        while rows > 1 and rows * K * 4 > self.scratch_bytes:
            rows >>= 1
        if rows * K * 4 > self.scratch_bytes:
            raise ValueError(f"scratch_bytes = {self.scratch_bytes} does not hold one token's similarities to "
                             f"{K} centroids ({4 * K} bytes)")
        x = torch.zeros((rows, E), dtype=centroids.dtype, device=centroids.device)
        sim = torch.empty((rows, K), dtype=torch.float32, device=centroids.device)
        for a in range(0, T, rows):
            b = min(a + rows, T)
            load(a, b, x[:b - a])
            ops.gemm(x, centroids, sim, bias=bias)
            ops.centroid_codes(sim, None if mask is None else mask[a:b], codes[a:b], rows=b - a)

    def _assign(self, a, b):
        """Codes of the stored documents a .. b from their stored representation (an FP8 index: the dequantised
        vectors) and the centroids: the same function in `add` and in `set_centroids`."""
        self._assign_rows(self._kind.loader(a, b), (b - a) * self._ld, self._mask[a:b].view(-1), self._codes[a:b].view(-1),
                          self._centroids)

    def set_centroids(self, centroids):
        """Take `centroids` ([K, E] array or tensor, 1 <= K <= 65535, as given: cast to the index's dtype, not
        normalised) and give every stored token the id of its nearest one by dot product (ops.gemm +
        ops.centroid_codes; ties to the lower id; masked and padding slots get 0xFFFF).  Documents added later are
        assigned in `add`.  Codes are a function of the stored representation and the centroids (and of the GEMM
        shape _assign_rows fixes from K and scratch_bytes), so assigning again never changes a code."""
        self._check_centroid_support()
        c = centroids if isinstance(centroids, torch.Tensor) else torch.as_tensor(np.ascontiguousarray(centroids))
        E = self._reps.shape[2]
        if c.dim() != 2 or c.shape[1] != E or not 1 <= c.shape[0] <= MAX_CENTROIDS:
            raise ValueError(f"centroids must be [K, {E}] with 1 <= K <= {MAX_CENTROIDS} (got {tuple(c.shape)})")
        self._centroids = c.to(device=self._reps.device, dtype=self._kind.dtype).contiguous().clone()
        self._store.declare(codes=((self._ld,), torch.int16, -1))              # a fresh buffer, all 0xFFFF
        self._assign(0, self._n)
        self._lists_stale = True

    def _sample_slots(self, sample, seed):
        """The sampled token slots of fit_centroids and fit_codec (the rule is in fit_centroids' docstring)."""
        S = self._n * self._ld
        r = np.random.Generator(np.random.PCG64(int(seed)))
        slots = r.permutation(S) if S <= int(sample) else r.choice(S, size=int(sample), replace=False)
        return slots[self._mask[:self._n].reshape(-1).cpu().numpy()[slots] != 0]

    def fit_centroids(self, K, iters=4, sample=1 << 18, seed=0):
        """Spherical k-means on the device over a sample of the stored tokens, then set_centroids.

        Sample: with r = numpy.random.Generator(PCG64(seed)) and S = N * Ld token slots (slot = document * Ld +
        position), the slots are r.permutation(S) when S <= sample and r.choice(S, size=sample, replace=False)
        otherwise, in the order drawn; slots whose mask is 0 are dropped.  It depends on seed, N, Ld and the masks
        only.  The sampled rows are gathered by a torch index copy (an FP8 index: codes and scales, then
        ops.fp8_dequantize).  The first K of them are the initial centroids; fewer than K raises ValueError.
        Each of `iters` rounds assigns every sampled token to its nearest centroid (ops.gemm + ops.centroid_codes)
        and replaces a centroid by the normalised sum of its tokens (ops.centroid_update; a centroid without tokens
        stays).  All sums run in a fixed order: the same index and seed give the same bits, so data-parallel ranks
        holding the same corpus agree without communication."""
        self._check_centroid_support()
        K = int(K)
        if not 1 <= K <= MAX_CENTROIDS:
            raise ValueError(f"need 1 <= K <= {MAX_CENTROIDS} centroids (got {K})")
        slots = self._sample_slots(sample, seed)
        if len(slots) < K:
            raise ValueError(f"{K} centroids need at least as many valid sampled tokens (got {len(slots)})")
        dev = self._reps.device
        x = self._kind.gather(torch.as_tensor(slots.astype(np.int64)).to(dev))
        (T, E) = x.shape
        cent, nxt = x[:K].clone(), torch.empty((K, E), dtype=x.dtype, device=dev)
        codes = torch.empty((T,), dtype=torch.int16, device=dev)
        counts = torch.empty((K,), dtype=torch.int32, device=dev)
        for _ in range(int(iters)):
            self._assign_rows(lambda a, b, dst: dst.copy_(x[a:b]), T, None, codes, cent)
            ops.centroid_update(x, codes, cent, nxt, counts, self.eps)
            cent, nxt = nxt, cent
        self.set_centroids(cent)

    def fit_codec(self, nbits, sample=1 << 16, seed=0):
        """A ResidualCodec for this index's centroids from a sample of its stored tokens (a plain or FP8 token index
        that has centroids: the "training" index over a sample of the corpus, as in ColBERTv2).

        The sampled slots are fit_centroids' (seed, N, Ld and the masks only; masked slots dropped).  Every sampled
        token's residual against the centroid of its stored code is r = f32(x) - f32(centroid), one f32 subtraction
        (an FP8 index: x is the dequantised vector).  Over all elements of all these residuals, cutoffs[j] is the
        (j + 1) / 2^nbits quantile and weights[b] the (b + 1/2) / 2^nbits quantile: numpy.quantile in float64 with
        method="linear", cast to f32.  Host work at build time, deterministic: data-parallel ranks holding the same
        corpus agree without communication."""
        if nbits not in (1, 2, 4):
            raise ValueError(f"nbits must be 1, 2 or 4 (got {nbits!r})")
        self._check_centroid_support()
        if self._centroids is None:
            raise ValueError("fit_codec needs centroids: call fit_centroids or set_centroids first")
        slots = self._sample_slots(sample, seed)
        if len(slots) == 0:
            raise ValueError("the sample holds no valid token")
        at = torch.as_tensor(slots.astype(np.int64)).to(self._reps.device)
        x = self._kind.gather(at)
        codes = self._codes[:self._n].view(-1)[at].cpu().numpy().view(np.uint16).astype(np.int64)
        cent = self._centroids.float().cpu().numpy()
        res = x.float().cpu().numpy() - cent[codes]
        n = 1 << nbits
        flat64 = res.astype(np.float64).ravel()
        cutoffs = np.quantile(flat64, np.arange(1, n) / n, method="linear").astype(np.float32)
        weights = np.quantile(flat64, (np.arange(n) + 0.5) / n, method="linear").astype(np.float32)
        return ResidualCodec(self._centroids.clone(), cutoffs, weights, nbits)

    def _sample_rows(self, sample, seed):
        """The sampled documents of fit_pq, in the order drawn (the rule is in fit_pq's docstring)."""
        r = np.random.Generator(np.random.PCG64(int(seed)))
        return r.permutation(self._n) if self._n <= int(sample) else r.choice(self._n, size=int(sample), replace=False)

    def fit_pq(self, m, ksub=256, iters=8, sample=1 << 16, seed=0):
        """A PQCodec of m sub-spaces with ksub codewords each from a sample of this index's stored vectors (a plain [CLS]
        index: the "training" index over a sample of the corpus, as fit_codec's is for residuals).

        Sample: with r = numpy.random.Generator(PCG64(seed)) the documents are r.permutation(N) when N <= sample and
        r.choice(N, size=sample, replace=False) otherwise, in the order drawn; it depends on seed and N only.  Their
        rows are gathered by a torch index copy.  The first ksub of them, widened to f32, are the initial codewords of
        every sub-space; fewer than ksub raises ValueError.  Each of `iters` Lloyd rounds gives every sampled sub-vector
        its nearest codeword (ops.pq_encode) and replaces a codeword by the mean of its sub-vectors (ops.pq_update; one
        without any stays).  All sums run in a fixed order: the same index and seed give the same bits, so data-parallel
        ranks holding the same corpus agree without communication."""
        m, ksub = self._check_pq_fit("fit_pq", m, ksub)
        rows = self._sample_rows(sample, seed)
        if len(rows) < ksub:
            raise ValueError(f"{ksub} codewords need at least as many sampled documents (got {len(rows)})")
        x = self._reps[:self._n][torch.as_tensor(rows.astype(np.int64)).to(self._reps.device)].contiguous()
        return PQCodec(self._pq_lloyd(x, m, ksub, iters))

    def _check_pq_fit(self, what, m, ksub):
        """(m, ksub) as ints once the index can train a product quantiser of that format: the refusals fit_pq and fit_ivfpq
        share."""
        if self._n == 0:
            raise ValueError("the index is empty: add documents before fitting a codec")
        if self.tokens or self.storage is not None:
            raise ValueError(f"{what} trains on a plain [CLS] index (storage=None): product quantisation is for one vector "
                             "per document, and a compressed index no longer holds the vectors to learn from")
        m, ksub, E = int(m), int(ksub), self._reps.shape[1]
        if not 4 <= m <= PQ_MAX_M or m % 4 or not 1 <= ksub <= 256:
            raise ValueError(f"need m a multiple of 4 in [4, {PQ_MAX_M}] and 1 <= ksub <= 256 (got m = {m}, ksub = {ksub})")
        if E % m or E // m > 32:
            raise ValueError(f"the index holds vectors of {E} features: m = {m} must divide that into sub-vectors of at "
                             "most 32")
        return m, ksub

    @staticmethod
    def _pq_lloyd(x, m, ksub, iters):
        """The codebook f32 [m, ksub, dsub] after `iters` Lloyd rounds over the rows of x [T >= ksub, m * dsub] (f32 or
        bf16, contiguous): the first ksub rows, widened to f32, are the initial codewords of every sub-space; a round is
        ops.pq_encode then ops.pq_update."""
        T, dsub, dev = x.shape[0], x.shape[1] // m, x.device
        cb = x[:ksub].float().view(ksub, m, dsub).permute(1, 0, 2).contiguous()
        nxt = torch.empty_like(cb)
        codes = torch.empty((T, m), dtype=torch.uint8, device=dev)
        counts = torch.empty((m, ksub), dtype=torch.int32, device=dev)
        for _ in range(int(iters)):
            ops.pq_encode(x, cb, codes)
            ops.pq_update(x, codes, cb, nxt, counts)
            cb, nxt = nxt, cb
        return cb

    def fit_ivfpq(self, K, m, ksub=256, iters=8, pq_iters=8, sample=1 << 16, seed=0):
        """An IVFPQCodec of K coarse centroids and m residual sub-spaces with ksub codewords each from a sample of this
        index's stored vectors (a plain [CLS] index, as for fit_pq).

        The sample is fit_pq's (seed and N only), gathered by a torch index copy; fewer than max(K, ksub) rows raise
        ValueError.  The first K rows are the initial centroids, in the index's dtype.  Each of `iters` rounds gives every
        sampled vector its L2-nearest centroid exactly as `add` does (ops.gemm with the bias -|c|^2 / 2, computed on the
        host in float64, then ops.centroid_codes: ties to the lower id) and replaces a centroid by the mean of its vectors
        (ops.ivfpq_coarse_update; one without any stays).  After a final assignment the f32 residuals
        (ops.ivfpq_residual) go through `pq_iters` rounds of fit_pq's Lloyd loop, the first ksub residuals being the
        initial codewords.  All sums run in a fixed order: the same index and seed give the same bits."""
        m, ksub = self._check_pq_fit("fit_ivfpq", m, ksub)
        K = int(K)
        if not 1 <= K <= MAX_CENTROIDS:
            raise ValueError(f"need 1 <= K <= {MAX_CENTROIDS} centroids (got {K})")
        rows = self._sample_rows(sample, seed)
        if len(rows) < max(K, ksub):
            raise ValueError(f"{K} centroids and {ksub} codewords need at least max(K, ksub) = {max(K, ksub)} sampled "
                             f"documents (got {len(rows)})")
        dev = self._reps.device
        x = self._reps[:self._n][torch.as_tensor(rows.astype(np.int64)).to(dev)].contiguous()
        T, E = x.shape
        cent, nxt = x[:K].clone(), torch.empty((K, E), dtype=x.dtype, device=dev)
        coarse = torch.empty((T,), dtype=torch.int16, device=dev)
        counts = torch.empty((K,), dtype=torch.int32, device=dev)

        def assign():
            self._assign_rows(lambda a, b, dst: dst.copy_(x[a:b]), T, None, coarse, cent, bias=_half_norms(cent).to(dev))

        for _ in range(int(iters)):
            assign()
            ops.ivfpq_coarse_update(x, coarse, cent, nxt, counts)
            cent, nxt = nxt, cent
        assign()
        res = torch.empty((T, E), dtype=torch.float32, device=dev)
        ops.ivfpq_residual(x, cent, coarse, res)
        return IVFPQCodec(cent, self._pq_lloyd(res, m, ksub, pq_iters))

    def search_pruned(self, queries, k, candidates, nprobe=None):
        """`search` over the `candidates` documents per query that score best under the centroid approximation:
        (scores f32 [Q, k], ids int32 [Q, k]) with exactly the contract of `search`.  The returned scores are exact
        MaxSim scores, bit for bit what `search` gives those documents; which documents are scored is approximate
        (see the module docstring).  One GEMM builds the table <centroid, query token>, ops.centroid_scores and
        ops.topk_merge keep the best `candidates` per chunk of documents, and the rerank path scores them.

        nprobe=None: the look-up score of every stored document is computed (a scan, linear in the corpus).
        1 <= nprobe <= min(K, 1024): only the documents holding at least one token whose centroid is among the
        `nprobe` nearest of at least one valid query token are considered (PLAID's candidate generation: the inverted
        lists of `refresh_lists`, ops.ivf_mark / ivf_compact, then ops.centroid_scores_ids, which gives a pair the
        look-up score bits of the scan).  A document without any present token is in no list and never a candidate
        here, while under the scan it scores 0.0 and is ranked.  With nprobe = K every non-empty document is
        considered: on a corpus whose documents all have a present token the result is the scan's, bit for bit."""
        if self._n == 0:
            raise ValueError("the index is empty: add documents before searching")
        self._check_token_lists("search_pruned")
        if self._centroids is None:
            raise ValueError("search_pruned needs centroids: call fit_centroids or set_centroids first")
        if not 1 <= int(candidates) <= MAX_K:
            raise ValueError(f"need 1 <= candidates <= {MAX_K}, the limit of ops.topk_merge, which keeps the candidates "
                             f"(got {candidates})")
        if nprobe is not None:
            self._check_nprobe(nprobe)
            self._fresh_lists()
        q = self.encode_queries(queries)
        qv = q.values
        Q, Lq, E = qv.shape
        table = torch.empty((self._centroids.shape[0], Q * Lq), dtype=torch.float32, device=qv.device)
        ops.gemm(self._centroids, qv.view(Q * Lq, E), table)
        cand_val = torch.empty((Q, int(candidates)), dtype=torch.float32, device=qv.device)
        cand_id = torch.empty((Q, int(candidates)), dtype=torch.int32, device=qv.device)
        if nprobe is not None:
            self._score_probed(q, table, int(nprobe), cand_val, cand_id)
            return self._rerank_encoded(q, cand_id, k)
        codes = self._codes
        topk_scan(Q, None, self.chunks(Q), qv.device,
                  lambda a, b, s: ops.centroid_scores(table, q.mask, codes[a:b], s, Q, Lq), top=(cand_val, cand_id))
        return self._rerank_encoded(q, cand_id, k)

    # ------------------------------------------------------------ inverted lists and probed candidates
    def _check_token_lists(self, what):
        if self.storage == "ivfpq":
            raise ValueError(f"{what} prunes a token (MaxSim) index; this index holds [CLS] representations in lists of "
                             "their own: search(queries, k, nprobe) probes them")

    def refresh_lists(self):
        """Build the inverted lists from the codes of all stored documents (ops.ivf_count / ivf_offsets / ivf_fill):
        offsets int32 [K + 1] and docs int32 [P], docs[offsets[c] : offsets[c + 1]] the documents holding a present
        token of centroid c, each once, in no specified order.  One int (P) is copied to the host to size `docs`.
        `add`, `set_centroids` and `fit_centroids` only mark the lists stale; a search with `nprobe`, `probe` and
        `lists` call this when they are.  An IVF-PQ index: the same CSR over its coarse codes as [N, 1], every document in
        exactly one list, P = N."""
        if self._n == 0:
            raise ValueError("the index is empty: add documents before building the lists")
        if self._centroids is None:
            raise ValueError("refresh_lists needs centroids: call fit_centroids or set_centroids first")
        codes = self._kind.list_codes()
        K, dev = self._centroids.shape[0], codes.device
        counts = torch.empty((K,), dtype=torch.int32, device=dev)
        offsets = torch.empty((K + 1,), dtype=torch.int32, device=dev)
        ops.ivf_count(codes, K, counts)
        ops.ivf_offsets(counts, offsets)
        P = int(offsets[K:].cpu()[0])
        if P < 0:
            raise ValueError("the lists would hold 2^31 or more (centroid, document) pairs, more than an int32 offset "
                             "addresses: shard the corpus")
        docs = torch.empty((P,), dtype=torch.int32, device=dev)
        ops.ivf_fill(codes, offsets, counts, docs)            # counts serves as the cursors
        self._lists, self._lists_stale = (offsets, docs), False

    def _fresh_lists(self):
        if self._lists is None or self._lists_stale:
            self.refresh_lists()

    @property
    def lists(self):
        """(offsets int32 [K + 1], docs int32 [P]) on the device, brought up to date first (refresh_lists); None on
        an index without documents or centroids."""
        if self._n == 0 or self._centroids is None:
            return None
        self._fresh_lists()
        return self._lists

    def _check_nprobe(self, nprobe, K=None):
        most = min(self._centroids.shape[0] if K is None else K, MAX_K)
        if not 1 <= int(nprobe) <= most:
            raise ValueError(f"need 1 <= nprobe <= min(K, {MAX_K}) = {most}, the centroids there are and the limit of "
                             f"ops.topk_merge, which keeps the probes (got {nprobe})")
        return int(nprobe)

    def _mark_probed(self, q, nprobe):
        """(probes int32 [Q * Lq, nprobe], bitmap int32 [Q, ceil(N / 32)], count int32 [Q]) on the device for
        encode_queries' TokenReps: each query token's nprobe nearest centroids (ops.gemm + ops.topk_merge: similarity
        descending, ties to the lower centroid; the queries in chunks whose [rows, K] f32 similarities stay within
        scratch_bytes), the union of their lists as one bitmap row per query (ops.ivf_mark; masked query tokens probe
        nothing) and its number of set bits (ops.ivf_compact)."""
        qv = q.values
        Q, Lq, E = qv.shape
        K, dev = self._centroids.shape[0], qv.device
        per = min(Q, self.scratch_bytes // (4 * Lq * K))
        if per < 1:
            raise ValueError(f"scratch_bytes = {self.scratch_bytes} does not hold one query's similarities to {K} "
                             f"centroids ({4 * Lq * K} bytes)")
        flat = qv.view(Q * Lq, E)
        probes = torch.empty((Q * Lq, nprobe), dtype=torch.int32, device=dev)
        val = torch.empty((per * Lq, nprobe), dtype=torch.float32, device=dev)
        sim = torch.empty((per * Lq, K), dtype=torch.float32, device=dev)
        for a in range(0, Q * Lq, per * Lq):
            b = min(a + per * Lq, Q * Lq)
            ops.gemm(flat[a:b], self._centroids, sim[:b - a])
            ops.topk_merge(sim[:b - a], val[:b - a], probes[a:b], init=True)
        return (probes,) + self._mark(probes, q.mask, Q, Lq)

    def _mark(self, probes, qmask, Q, Lq):
        """(bitmap int32 [Q, ceil(N / 32)], count int32 [Q]) on the device: the union of the lists of probes int32
        [Q * Lq, nprobe] as one bitmap row per query (ops.ivf_mark; qmask int32 [Q, Lq] or None) and its number of set bits
        (ops.ivf_compact)."""
        offsets, docs = self._lists
        bitmap = torch.empty((Q, (self._n + 31) // 32), dtype=torch.int32, device=probes.device)
        count = torch.empty((Q,), dtype=torch.int32, device=probes.device)
        ops.ivf_mark(probes, qmask, offsets, docs, self._n, bitmap, Q, Lq)
        ops.ivf_compact(bitmap, self._n, count)
        return bitmap, count

    def probe(self, queries, nprobe):
        """The candidate generation of `search_pruned(..., nprobe)` on its own: (probes int32 [Q, Lq, nprobe], cand
        int32 [Q, M], count int32 [Q]) on the device.  probes[q, i] are the nprobe centroids nearest to query token
        i (computed for masked tokens too, which then probe nothing); cand[q, :count[q]] are, in ascending order, the
        documents holding a token of a centroid probed by a valid token of query q, the rest of the row is -1;
        M = max(1, max count).  `cand` can go to `rerank`, or to another index holding the same documents."""
        if self._n == 0:
            raise ValueError("the index is empty: add documents before probing")
        self._check_token_lists("probe")
        if self._centroids is None:
            raise ValueError("probe needs centroids: call fit_centroids or set_centroids first")
        self._check_nprobe(nprobe)
        self._fresh_lists()
        q = self.encode_queries(queries)
        Q, Lq = q.values.shape[:2]
        probes, bitmap, count = self._mark_probed(q, int(nprobe))
        cand = torch.empty((Q, max(1, int(count.cpu().max()))), dtype=torch.int32, device=count.device)
        ops.ivf_compact(bitmap, self._n, count, cand)
        return probes.view(Q, Lq, int(nprobe)), cand, count

    def _score_probed(self, q, table, nprobe, cand_val, cand_id):
        """The candidate stage of search_pruned under `nprobe`: the look-up scores of each query's probed documents
        only (ops.centroid_scores_ids: the bits the scan gives those pairs) merged into cand_val / cand_id
        (_scan_probed)."""
        Lq = q.values.shape[1]
        _, bitmap, count = self._mark_probed(q, nprobe)
        codes = self._codes[:self._n]
        self._scan_probed(bitmap, count, (cand_val, cand_id), lambda a, b, cand: lambda s, e, sc: ops.centroid_scores_ids(
            table[:, a * Lq:], q.mask[a:b], codes, cand[:, s:e], sc, b - a, Lq))

    def _scan_probed(self, bitmap, count, top, scorer):
        """The exact top-k (top = (top_val f32 [Q, k], top_id int32 [Q, k]), overwritten) over each query's own candidates,
        the set bits of its row of `bitmap` (count int32 [Q] their numbers).  The counts come to the host in one copy; the
        queries are taken in consecutive groups a .. b whose [group, largest count] int32 candidate buffer stays within
        scratch_bytes; a group's candidates are written in ascending order (ops.ivf_compact) and scorer(a, b, cand) gives
        the score(s, e, out) of store.topk_scan over its candidate columns."""
        Q = count.shape[0]
        counts = np.maximum(count.cpu().numpy(), 1)           # a query without a candidate: one column of -1
        if 4 * int(counts.max()) > self.scratch_bytes:
            raise ValueError(f"scratch_bytes = {self.scratch_bytes} does not hold the {int(counts.max())} candidates "
                             f"of one query ({4 * int(counts.max())} bytes)")
        a = 0
        while a < Q:
            b, C = a + 1, int(counts[a])
            while b < Q and 4 * (b + 1 - a) * max(C, int(counts[b])) <= self.scratch_bytes:
                C, b = max(C, int(counts[b])), b + 1
            cand = torch.empty((b - a, C), dtype=torch.int32, device=count.device)
            ops.ivf_compact(bitmap[a:b], self._n, count[a:b], cand)
            topk_scan(b - a, None, self.rerank_chunks(b - a, C), count.device, scorer(a, b, cand), ids=cand,
                      top=(top[0][a:b], top[1][a:b]))
            a = b

    def _search_probed(self, q, k, nprobe):
        """`search` of an IVF-PQ index under `nprobe` for encoded queries q [Q, E]: one GEMM gives every query's dot products with the centroids, which
        are both the probe ranking (ops.topk_merge: descending, ties to the lower centroid) and the centroid term of the
        scores; the probed lists become a bitmap and ascending candidate ids (_mark, _scan_probed), scored by
        ops.ivfpq_scores_ids."""
        if not 1 <= int(k) <= MAX_K:
            raise ValueError(f"need 1 <= k <= {MAX_K}, the limit of ops.topk_merge (got {k})")
        self._fresh_lists()
        Q, dev = q.shape[0], q.device
        lut, cdot = self._kind.tables(q)
        probes = torch.empty((Q, nprobe), dtype=torch.int32, device=dev)
        ops.topk_merge(cdot, torch.empty((Q, nprobe), dtype=torch.float32, device=dev), probes, init=True)
        bitmap, count = self._mark(probes, None, Q, 1)
        coarse, codes = self._store.view("coarse"), self._store.view("reps")
        top = (torch.empty((Q, int(k)), dtype=torch.float32, device=dev), torch.empty((Q, int(k)), dtype=torch.int32, device=dev))
        self._scan_probed(bitmap, count, top, lambda a, b, cand: lambda s, e, sc: ops.ivfpq_scores_ids(
            lut[a:b], cdot[a:b], coarse, codes, cand[:, s:e], sc))
        return top


class SparseCorpusIndex:
    """A learned sparse (SPLADE) first stage: per document the `terms` best (term id, weight) pairs of its vocabulary
    representation, int32 ids [N, terms] and f32 weights [N, terms] in growing device buffers; queries stay dense.

    `model` is a SpladeEncoder (anything whose encode_document / encode_query give f32 [n, V]).  The contracts of
    `add(documents) -> ids` and `search(queries, k) -> (scores, ids)` are CorpusIndex's, so it serves as the first
    stage of TwoStageSearch and under a validation callback.  `add` keeps a document's terms with ops.topk_merge, each
    row of the representations one "query" of that kernel: weight descending, ties to the lower term id, and a
    document with fewer than `terms` entries (V < terms) is padded with (-inf, -1), slots ops.sparse_scores skips by
    their id.  Zero weights are kept when nothing better is left: they add nothing.
    `search` scores chunks of documents with ops.sparse_scores and merges them with ops.topk_merge, the scan every index
    shares (store.topk_scan).  `scratch_bytes` bounds the [Q, n] f32 score buffer of one chunk.
    `postings=True` searches block-inverted postings of `block_docs` documents per block instead (polus_amd/ir/postings.py):
    `add` marks them stale, `refresh_postings` (or the next search) rebuilds them from the stored slots, the dense
    queries become lists of at most `query_terms` non-zeros (ops.sparse_compact_rows; their counts are copied to the
    host, the route's one synchronisation, and a query with more raises), and representations wider than the 40 960
    columns ops.sparse_scores holds in LDS are accepted.  The default is the forward route, unchanged.
    Not measured: retrieval quality and how sparse the representations of a trained model are on a real collection."""

    def __init__(self, model, terms=128, scratch_bytes=256 << 20, postings=False, block_docs=8192, query_terms=1024):
        if not 1 <= int(terms) <= MAX_K:
            raise ValueError(f"need 1 <= terms <= {MAX_K}, the limit of ops.topk_merge, which keeps them (got {terms})")
        if int(query_terms) < 1:
            raise ValueError(f"need query_terms >= 1 (got {query_terms})")
        self.model, self.terms, self.scratch_bytes = model, int(terms), int(scratch_bytes)
        self.block_docs, self.query_terms = check_block_docs(block_docs), int(query_terms)
        self._postings = Postings(block_docs) if postings else None
        self.clear()

    def clear(self):
        """Empty the index (the storage is released)."""
        self._store = RowStore()
        self._store.declare(ids=((self.terms,), torch.int32, -1), w=((self.terms,), torch.float32, 0))
        if self._postings is not None:
            self._postings.clear()

    _n, _ids, _w = stored_rows, stored("ids"), stored("w")
    _postings_stale = property(lambda self: self._postings is not None and self._postings.stale)

    def refresh_postings(self):
        """Rebuild the postings from the stored (term id, weight) slots (polus_amd/ir/postings.py: count, offsets, one
        8-byte copy to the host, fill).  Needs postings=True."""
        if self._postings is None:
            raise ValueError("this index was made with postings=False")
        if self._n == 0:
            raise ValueError("the index is empty: add documents before refreshing")
        self._postings.build(*self._forward())

    def _forward(self):
        """What the postings are built from: the stored (term id, weight) slots."""
        return self.term_ids, self.weights, self._V

    @property
    def postings(self):
        """(offsets int32 [nblk, V + 1], base int64 [nblk + 1], post_doc int16 [P], post_w f32 [P]), rebuilt first when
        stale; None without postings=True or on an empty index."""
        if self._postings is None or self._n == 0:
            return None
        return self._postings.update(self._forward).arrays()

    def __len__(self):
        return self._n

    @property
    def term_ids(self):
        """int32 [N, terms]: a view of the stored term ids, -1 in unused slots."""
        return self._store.view("ids")

    @property
    def weights(self):
        """f32 [N, terms]: a view of the stored weights, -inf in unused slots."""
        return self._store.view("w")

    @property
    def nbytes(self):
        """Bytes of the stored ids and weights of the len(index) documents, plus the postings that are built."""
        if self._ids is None:
            return 0
        extra = 0 if self._postings is None else self._postings.nbytes
        return self._n * self.terms * (self._ids.element_size() + self._w.element_size()) + extra

    def add(self, documents):
        """Encode a batch of documents, keep each one's `terms` best entries and append them; returns the batch's ids,
        the consecutive int32 positions in the index."""
        model = self.model
        rep = model.document_projection(model.encode_document(documents, training=False), training=False)
        if rep.dim() != 2 or rep.dtype != torch.float32:
            raise ValueError(f"a sparse index holds f32 [n, V] vocabulary representations (got {rep.dtype} {tuple(rep.shape)})")
        n, V = rep.shape
        if getattr(self, "_V", V) != V and self._n:
            raise ValueError(f"the index holds representations over {self._V} terms, the batch has {V}")
        self._V = V
        self._store.reserve(self._n + n, rep.device)
        vals = torch.empty((n, self.terms), dtype=torch.float32, device=rep.device)
        ids = torch.empty((n, self.terms), dtype=torch.int32, device=rep.device)
        ops.topk_merge(rep, vals, ids, init=True)
        self._ids[self._n:self._n + n].copy_(ids)
        self._w[self._n:self._n + n].copy_(vals)
        out = torch.arange(self._n, self._n + n, dtype=torch.int32, device=rep.device)
        self._n += n
        if self._postings is not None:
            self._postings.stale = True
        return out

    def query_lists(self, q):
        """Dense f32 [Q, V] query representations as lists (q_terms int32, q_w f32 [Q, query_terms], q_count int32 [Q]) of
        their non-zeros in ascending term id; copies the Q counts to the host and raises when one exceeds query_terms."""
        Q, cap = q.shape[0], self.query_terms
        q_terms = torch.empty((Q, cap), dtype=torch.int32, device=q.device)
        q_w = torch.empty((Q, cap), dtype=torch.float32, device=q.device)
        q_count = torch.empty((Q,), dtype=torch.int32, device=q.device)
        ops.sparse_compact_rows(q, q_terms, q_w, q_count)
        most = int(q_count.cpu().max())                                   # the route's one synchronisation
        if most > cap:
            raise ValueError(f"a query has {most} non-zero terms, more than query_terms = {cap}: raise query_terms")
        return q_terms, q_w, q_count

    def chunks(self, Q):
        """[(start, stop), ...]: the document ranges a search with Q queries scores, one launch each (store.score_chunks)."""
        return score_chunks(self._n, Q, self.scratch_bytes, "document")

    def encode_queries(self, queries):
        """The queries' dense f32 [Q, V] representations."""
        model = self.model
        return model.query_projection(model.encode_query(queries, training=False), training=False).contiguous()

    def search(self, queries, k):
        """(scores f32 [Q, k], ids int32 [Q, k]) on the device: per query the k best documents, score descending, ties
        to the lower id; when the corpus holds fewer than k, the tail is (-inf, -1)."""
        if self._n == 0:
            raise ValueError("the index is empty: add documents before searching")
        q = self.encode_queries(queries)
        if self._postings is not None:
            if q.dim() != 2 or q.shape[1] != self._V:
                raise ValueError(f"the index holds representations over {self._V} terms, the queries have {tuple(q.shape)}")
            lists = self.query_lists(q)
            return self._postings.update(self._forward).search(*lists, k, self.scratch_bytes)
        return self.search_forward(q, k)

    def search_forward(self, q, k):
        """`search` on the forward route for dense f32 [Q, V] query representations, whatever `postings` says
        (tools/postings_bench.py compares the two routes of one index with it)."""
        ids, w = self._ids, self._w
        return topk_scan(q.shape[0], k, self.chunks(q.shape[0]), q.device,
                         lambda a, b, s: ops.sparse_scores(q, ids[a:b], w[a:b], s))


class TwoStageSearch:
    """Retrieve with a cheap index, re-rank with a better one: `first` is anything with search(queries, k) ->
    (scores, ids) and add(documents), in practice a [CLS] CorpusIndex over a DualEncoder, a BM25Index, a SparseCorpusIndex
    or a HybridSearch; `second` is anything with rerank(queries, candidates, k) holding the same documents under the same
    ids: a token CorpusIndex (MaxSim), or a [CLS] CorpusIndex with a refine store (refine="full" on a plain index: the
    lexical -> bi-encoder pipeline); `candidates` is how many documents the first stage proposes per query.  A CorpusIndex returns at most 1024 results per query (the limit of ops.topk_merge), so with
    one as the first stage `candidates` is at most 1024; another first stage sets its own limit."""

    def __init__(self, first, second, candidates):
        if int(candidates) < 1:
            raise ValueError(f"candidates must be >= 1 (got {candidates})")
        if isinstance(first, CorpusIndex) and int(candidates) > MAX_K:
            raise ValueError(f"a CorpusIndex as the first stage proposes at most {MAX_K} candidates per query "
                             f"(got {candidates})")
        self.first, self.second, self.candidates = first, second, int(candidates)

    def __len__(self):
        return len(self.second)

    def add(self, documents):
        """Add a batch to both stages; returns its ids.  The two stages must number it alike."""
        a, b = self.first.add(documents), self.second.add(documents)
        if tuple(a.shape) != tuple(b.shape) or not bool((torch.as_tensor(a).to(b.device) == b).all()):
            raise ValueError("the two stages gave a document batch different ids: they must hold the same documents "
                             "in the same order")
        return b

    def search(self, queries, k):
        """(scores f32 [Q, k], ids int32 [Q, k]): the second stage's ranking of the first stage's candidates."""
        return self.second.rerank(queries, self.first.search(queries, self.candidates)[1], k)


class RetrievalValidationCallback(ValidationDataCallback):
    """Validation of a retrieval run: on each validated epoch the corpus (an iterable of document batches) is encoded
    again with the trainer's current model, compute_scores and post_process_logits, every validation sample
    `(queries, relevant)` becomes `(ids [Q, k], relevant)`, and the trainer's metrics (polus_amd/ir/metrics.py) land in
    shared_dict["validation"][name], where SaveModelCallback(strategy="best") reads them.  `storage` is the
    CorpusIndex's (None or "fp8", token representations only).  With `centroids` (a number K) the index fits that many
    centroids once the corpus is added (CorpusIndex.fit_centroids) and ranks with search_pruned over `candidates`
    documents per query (None: 1024, the most it takes), with `nprobe` passed on to it (None: the scan; a number: the
    probed candidate generation, which needs `centroids`); the defaults rank with the exhaustive `search`."""

    def __init__(self, corpus, tf_validation, k, name=None, validation_interval=1, show_progress=False,
                 scratch_bytes=256 << 20, storage=None, centroids=None, candidates=None, nprobe=None):
        if nprobe is not None and centroids is None:
            raise ValueError("nprobe needs centroids: it probes the lists of search_pruned's centroids")
        if nprobe is not None and int(nprobe) < 1:
            raise ValueError(f"need nprobe >= 1 (got {nprobe})")
        self.nprobe = None if nprobe is None else int(nprobe)
        super().__init__(tf_validation, custom_inference_f=self._rank, name=name, show_progress=show_progress,
                         validation_interval=validation_interval)
        self.corpus, self.k, self.scratch_bytes, self.storage = corpus, int(k), scratch_bytes, storage
        self.centroids = centroids
        self.candidates = MAX_K if candidates is None else int(candidates)
        self.index = None

    def _rank(self, model, sample):
        queries, relevant = sample
        if self.centroids is not None:
            return self.index.search_pruned(queries, self.k, self.candidates, self.nprobe)[1], relevant
        return self.index.search(queries, self.k)[1], relevant

    def on_epoch_end(self, epoch):
        if epoch % self.validation_interval:
            return
        trainer = self.coordinator.trainer
        self.index = CorpusIndex(trainer.model, trainer.compute_scores, trainer.post_process_logits, self.scratch_bytes,
                                 storage=self.storage)
        for documents in self.corpus:
            self.index.add(documents)
        if self.centroids is not None:
            self.index.fit_centroids(int(self.centroids))
        super().on_epoch_end(epoch)
        self.index.clear()
