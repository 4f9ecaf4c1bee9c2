"""Lexical retrieval: a BM25 index over token ids, built and searched on the device.

    index = BM25Index(vocab_size=30522)                   # no model: the "terms" are the tokeniser's ids
    for docs in corpus_batches: index.add(docs)           # {"input_ids", "attention_mask"}; returns the batch's ids
    scores, ids = index.search(queries, k=1000)           # f32 / int32 [Q, k] on the device
    two = TwoStageSearch(index, token_index, 1000)        # a first stage like any other

BM25 needs no trained model; it is the baseline every retrieval result is quoted against and the cheapest first stage
of the hard-negative loop (polus_amd/ir/mining.py).  The score of document d for query q is

    sum over the terms t of q of  tf_q(t) * idf(t) * tf_d(t) (k1 + 1) / (tf_d(t) + k1 (1 - b + b len_d / avgdl)),
    idf(t) = log(1 + (N - df(t) + 0.5) / (df(t) + 0.5))       (Lucene's non-negative form)

with the defaults k1 = 0.9, b = 0.4 of the Anserini MS MARCO baseline.

Format.  Per document `terms` slots of (term id int32, count int32, weight f32), the distinct token ids of the document
ordered by (count descending, id ascending) with (-1, 0, 0.0) in unused slots, plus its length int32; per index the
document frequencies df int32 [V] and three int64 counters (truncated documents, rejected tokens, tokens), all on the
device (ops.bm25_term_counts).  A document with more than `terms` distinct ids loses its rarest-in-document ones and is
counted in `truncated`; the default `terms` is the width of the first batch, so nothing is truncated.  The weight is
the document-side factor tf (k1 + 1) / (tf + K) of the formula.

Refresh.  The weights depend on N and the average length, so they go stale with every `add` (and `set_params`).  The
counts are kept, which makes `refresh` cheap: one copy of df and the counters to the host (4 V + 24 bytes, the one
synchronisation), idf and three constants in float64 rounded once to f32, one upload of idf, one launch of
ops.bm25_weights over all rows.  `search` refreshes a stale index first.

Queries are counted by the same kernel (without df), turned into dense f32 [Q, V] rows tf_q idf (ops.bm25_query), and
`search` is the chunked scan every index shares (store.topk_scan) over ops.sparse_scores: its scores are the bits
polus_sparse_scores gives for (q, terms, w), in slot order.

Postings.  That search reads every slot of every document for every query.  `BM25Index(vocab_size, postings=True,
block_docs=...)` searches block-inverted postings instead (polus_amd/ir/postings.py has the format and the score rule):

    index = BM25Index(vocab_size=119547, postings=True)   # no dense query row: the vocabulary is bounded by int32 only
    scores, ids = index.search(queries, k=1000)           # refresh, then refresh_postings, when stale

`add` and `set_params` only mark the postings stale; `refresh_postings` rebuilds them from the stored (term id, weight)
slots after a `refresh` (the weights change with N); queries are counted as before and become lists of (term, tf_q idf)
in ascending id (ops.bm25_query_lists; no dense row, no synchronisation), and `search` is the same scan over
ops.postings_scores, whole blocks per launch.  The contract of `search` is the same; the scores are
the bits of the postings score rule (products and sums in ascending term id, each rounded once), which differ from the
forward route's fma chain in slot order by rounding.  The forward route is the default and keeps its bits.

Tokens are the wordpieces of whatever tokeniser made the ids, which is known to cost some quality against word-level
BM25 with stemming and stop words.  Not measured: retrieval quality on any real collection.

Arithmetic is hand-written HIP (ops.bm25_term_counts / bm25_weights / bm25_query / sparse_scores / topk_merge, and on
the postings route ops.postings_count / postings_offsets / postings_fill / bm25_query_lists / postings_scores) except
the V idf values of a refresh, which are NumPy float64 on the host; torch allocates, views and copies."""
import numpy as np
import torch

from .. import ops
from ..tensor import device, to_device
from .postings import MAX_POSTINGS_VOCAB, Postings, check_block_docs
from .store import RowStore, score_chunks, stored, stored_rows, topk_scan

MAX_TERMS = 1024              # slots per document: what ops.sparse_scores accepts
MAX_TOKENS = 2048             # tokens per row: the limit of ops.bm25_term_counts
MAX_VOCAB = 163840 // 4       # the dense query row ops.sparse_scores holds in LDS


def bm25_constants(k1, b, n_docs, n_tokens):
    """(c0, c1, k1p1) as np.float32: K = c1 len + c0 and the numerator's k1 + 1.  avgdl = n_tokens / n_docs in float64,
    1 when the corpus has no token; each constant is computed in float64 and rounded once."""
    avgdl = float(n_tokens) / float(n_docs) if n_tokens > 0 else 1.0
    k1, b = float(k1), float(b)
    return np.float32(k1 * (1.0 - b)), np.float32(k1 * b / avgdl), np.float32(k1 + 1.0)


def bm25_idf(df, n_docs):
    """f32 [V]: log1p((N - df + 0.5) / (df + 0.5)) in float64, rounded once."""
    df = np.asarray(df, np.float64)
    return np.log1p((float(n_docs) - df + 0.5) / (df + 0.5)).astype(np.float32)


class BM25Index:
    """BM25 over token ids with the contract of SparseCorpusIndex: `add(documents) -> ids`, `search(queries, k) ->
    (scores, ids)`, so it serves as `first` of TwoStageSearch and of polus_amd.ir.mining (see the module docstring).

    `vocab_size` bounds the ids (a token outside [0, vocab_size) is dropped and counted in `rejected`); `terms` is the
    number of slots per document (None: min(width of the first batch, 1024)); `strip` = (head, tail) valid tokens taken
    off every document and query row, (1, 1) for the [CLS] and [SEP] of HF-tokenised inputs, (0, 0) for raw ids;
    `scratch_bytes` bounds the [Q, n] f32 score buffer of one chunk of a search.  `postings=True` searches block-inverted
    postings of `block_docs` documents per block instead of the forward slots (polus_amd/ir/postings.py) and lifts the
    limit on `vocab_size`; the default is the forward route, unchanged."""

    def __init__(self, vocab_size, terms=None, k1=0.9, b=0.4, strip=(1, 1), scratch_bytes=256 << 20, postings=False,
                 block_docs=8192):
        V = int(vocab_size)
        self._postings = Postings(block_docs) if postings else None
        self.block_docs = check_block_docs(block_docs)
        if postings:
            if not 1 <= V <= MAX_POSTINGS_VOCAB:
                raise ValueError(f"need 1 <= vocab_size <= {MAX_POSTINGS_VOCAB} (got {vocab_size})")
        elif not 1 <= V <= MAX_VOCAB:
            raise ValueError(f"need 1 <= vocab_size <= {MAX_VOCAB}, the query row ops.sparse_scores holds in LDS (got {vocab_size})")
        if terms is not None and not 1 <= int(terms) <= MAX_TERMS:
            raise ValueError(f"need 1 <= terms <= {MAX_TERMS}, what ops.sparse_scores accepts (got {terms})")
        self.strip = (int(strip[0]), int(strip[1]))
        if not all(0 <= s <= 8 for s in self.strip):
            raise ValueError(f"strip counts must be in 0..8, got {strip}")
        self.vocab_size, self.terms, self.scratch_bytes = V, None if terms is None else int(terms), int(scratch_bytes)
        self._auto_terms = terms is None
        self._check_params(k1, b)
        self.k1, self.b = float(k1), float(b)
        self.clear()

    @staticmethod
    def _check_params(k1, b):
        if not (np.isfinite(k1) and float(k1) >= 0.0 and 0.0 <= float(b) <= 1.0):
            raise ValueError(f"need k1 >= 0 and 0 <= b <= 1 (got k1 = {k1}, b = {b})")

    def clear(self):
        """Empty the index (the storage and the statistics are released)."""
        self._store, self._stat, self._idf, self._stale = RowStore(), None, None, False
        if self._postings is not None:
            self._postings.clear()
        if self._auto_terms:
            self.terms = None

    def __len__(self):
        return self._n

    def set_params(self, k1, b):
        """New k1 and b for the documents already stored: only marks the index stale, the counts are kept."""
        self._check_params(k1, b)
        self.k1, self.b = float(k1), float(b)
        if self._n:
            self._mark_stale()

    def _mark_stale(self):
        self._stale = True
        if self._postings is not None:
            self._postings.stale = True

    # ------------------------------------------------------------ storage
    _n, _terms, _tf, _w, _len = stored_rows, stored("terms"), stored("tf"), stored("w"), stored("len")
    _postings_stale = property(lambda self: self._postings is not None and self._postings.stale)

    @property
    def _df(self):
        return self._stat[6:]

    @property
    def _counters(self):
        return self._stat[:6].view(torch.int64)

    @staticmethod
    def _rows(batch, what):
        dev = device()
        ids = to_device(batch["input_ids"], torch.int32, dev)
        if ids.dim() != 2 or ids.shape[0] < 1:
            raise ValueError(f"{what} input_ids must be [n, L] with n >= 1 (got {list(ids.shape)})")
        if not 1 <= ids.shape[1] <= MAX_TOKENS:
            raise ValueError(f"{what} rows of {ids.shape[1]} tokens: ops.bm25_term_counts takes 1 .. {MAX_TOKENS}")
        m = batch.get("attention_mask")
        return ids, (None if m is None else to_device(m, torch.int32, dev).reshape(ids.shape))

    def add(self, documents):
        """Count a batch {"input_ids" [n, L][, "attention_mask"]} and append it; returns its ids, the consecutive int32
        positions in the index (CorpusIndex.add's numbering).  Marks the index stale."""
        ids, mask = self._rows(documents, "document")
        n, L = ids.shape
        dev = ids.device
        if self.terms is None:
            self.terms = min(L, MAX_TERMS)
        if self._stat is None:
            # one buffer, so that a refresh is one copy: the three int64 counters, then df
            self._stat = torch.zeros(6 + self.vocab_size, dtype=torch.int32, device=dev)
            slots = (self.terms,)
            self._store.declare(terms=(slots, torch.int32, -1), tf=(slots, torch.int32, 0), w=(slots, torch.float32, 0),
                                len=((), torch.int32, 0))
        a, b = self._n, self._n + n
        self._store.reserve(b, dev)
        ops.bm25_term_counts(ids, mask, self._terms[a:b], self._tf[a:b], self._len[a:b], self.vocab_size, self.strip,
                             df=self._df, stats=self._counters)
        self._n = b
        self._mark_stale()
        return torch.arange(a, b, dtype=torch.int32, device=dev)

    def _host_stats(self):
        h = self._stat.cpu().numpy()
        return h[:6].view(np.int64), h[6:]

    def refresh(self):
        """Recompute idf and the weights of every stored document from the counts (see the module docstring)."""
        if self._n == 0:
            raise ValueError("the index is empty: add documents before refreshing")
        counters, df = self._host_stats()                            # the one synchronisation
        c0, c1, k1p1 = bm25_constants(self.k1, self.b, self._n, int(counters[2]))
        self._idf = torch.as_tensor(bm25_idf(df, self._n)).to(self._stat.device)
        ops.bm25_weights(self._tf[:self._n], self._len[:self._n], self._w[:self._n], c0, c1, k1p1)
        self._stale = False

    def _fresh(self):
        if self._stale:
            self.refresh()

    def refresh_postings(self):
        """Rebuild the postings from the stored (term id, weight) slots, after a `refresh` when the weights are stale
        (polus_amd/ir/postings.py: count, offsets, one 8-byte copy to the host, fill).  Needs postings=True."""
        if self._postings is None:
            raise ValueError("this index was made with postings=False")
        if self._n == 0:
            raise ValueError("the index is empty: add documents before refreshing")
        self._postings.build(*self._forward())

    def _forward(self):
        """What the postings are built from: the stored (term id, weight) slots, the weights refreshed first."""
        self._fresh()
        return self._terms[:self._n], self._w[:self._n], self.vocab_size

    @property
    def postings(self):
        """(offsets int32 [nblk, V + 1], base int64 [nblk + 1], post_doc int16 [P], post_w f32 [P]), rebuilt first when
        stale; None without postings=True or on an empty index."""
        if self._postings is None or self._n == 0:
            return None
        return self._postings.update(self._forward).arrays()

    # ------------------------------------------------------------ views
    @property
    def truncated(self):
        """Documents that had more than `terms` distinct ids (copies the counters to the host)."""
        return 0 if self._stat is None else int(self._host_stats()[0][0])

    @property
    def rejected(self):
        """Document tokens dropped because their id lay outside [0, vocab_size) (copies the counters to the host)."""
        return 0 if self._stat is None else int(self._host_stats()[0][1])

    @property
    def nbytes(self):
        """Bytes of the stored documents (12 * terms + 4 each: ids, counts, weights, length) plus df and the counters,
        plus the postings that are built."""
        if self._terms is None:
            return 0
        extra = 0 if self._postings is None else self._postings.nbytes
        return self._n * (12 * self.terms + 4) + 4 * self.vocab_size + 24 + extra

    @property
    def term_ids(self):
        """int32 [N, terms]: a view of the stored term ids, -1 in unused slots."""
        return None if self._terms is None else self._terms[:self._n]

    @property
    def counts(self):
        """int32 [N, terms]: a view of the stored term counts, 0 in unused slots."""
        return None if self._tf is None else self._tf[:self._n]

    @property
    def weights(self):
        """f32 [N, terms]: a view of the weights, refreshed first when stale; 0.0 in unused slots."""
        if self._w is None:
            return None
        self._fresh()
        return self._w[:self._n]

    @property
    def doc_lengths(self):
        """int32 [N]: the tokens of each document after the strip and the rejection."""
        return None if self._len is None else self._len[:self._n]

    @property
    def idf(self):
        """f32 [V] on the device, refreshed first when stale."""
        if self._n:
            self._fresh()
        return self._idf

    # ------------------------------------------------------------ search
    def chunks(self, Q):
        """[(start, stop), ...]: the document ranges a search with Q queries scores, one launch each (store.score_chunks)."""
        return score_chunks(self._n, Q, self.scratch_bytes, "document")

    def encode_queries(self, queries):
        """The queries' dense f32 [Q, V] rows: tf_q(t) * idf(t) at the query's terms, 0 elsewhere.  A query row holds at
        most 1024 tokens; its tokens are stripped and rejected like a document's."""
        terms, tf = self._query_counts(queries)
        if self.vocab_size > MAX_VOCAB:
            raise ValueError(f"dense query rows need vocab_size <= {MAX_VOCAB}, the row ops.sparse_scores holds in LDS "
                             f"(got {self.vocab_size}): use encode_query_lists")
        q = torch.empty((terms.shape[0], self.vocab_size), dtype=torch.float32, device=terms.device)
        return ops.bm25_query(terms, tf, self._idf, q)

    def encode_query_lists(self, queries):
        """The queries as lists (q_terms int32 [Q, Lq], q_w f32 [Q, Lq], q_count int32 [Q]): the query's distinct terms
        in ascending id with weight tf_q(t) * idf(t), then (-1, 0.0).  What the postings route searches with; no dense
        row is made, so the vocabulary is not limited."""
        terms, tf = self._query_counts(queries)
        Q, Lq = terms.shape
        q_terms = torch.empty((Q, Lq), dtype=torch.int32, device=terms.device)
        q_w = torch.empty((Q, Lq), dtype=torch.float32, device=terms.device)
        q_count = torch.empty((Q,), dtype=torch.int32, device=terms.device)
        ops.bm25_query_lists(terms, tf, self._idf, q_terms, q_w, q_count)
        return q_terms, q_w, q_count

    def _query_counts(self, queries):
        if self._n == 0:
            raise ValueError("the index is empty: idf needs documents")
        self._fresh()
        ids, mask = self._rows(queries, "query")
        Q, Lq = ids.shape
        if Lq > MAX_TERMS:
            raise ValueError(f"query rows of {Lq} tokens: at most {MAX_TERMS}")
        dev = ids.device
        terms = torch.empty((Q, Lq), dtype=torch.int32, device=dev)
        tf = torch.empty((Q, Lq), dtype=torch.int32, device=dev)
        ln = torch.empty((Q,), dtype=torch.int32, device=dev)
        ops.bm25_term_counts(ids, mask, terms, tf, ln, self.vocab_size, self.strip)
        return terms, tf

    def search(self, queries, k):
        """(scores f32 [Q, k], ids int32 [Q, k]) on the device: per query the k best documents, score descending, ties
        to the lower id; when the corpus holds fewer than k, the tail is (-inf, -1).  A document that shares no term with
        the query scores 0.0 and is still ranked (behind every matching one, in id order): polus_amd.ir.mining drops
        such results with min_score = 0."""
        if self._n == 0:
            raise ValueError("the index is empty: add documents before searching")
        if self._postings is not None:
            lists = self.encode_query_lists(queries)
            return self._postings.update(self._forward).search(*lists, k, self.scratch_bytes)
        return self.search_forward(queries, k)

    def search_forward(self, queries, k):
        """`search` on the forward route, whatever `postings` says (tools/postings_bench.py compares the two routes of
        one index with it); needs vocab_size <= 40960."""
        q = self.encode_queries(queries)
        terms, w = self._terms, self._w
        return topk_scan(q.shape[0], k, self.chunks(q.shape[0]), q.device,
                         lambda a, b, s: ops.sparse_scores(q, terms[a:b], w[a:b], s))
