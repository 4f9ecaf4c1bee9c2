"""Block-inverted postings: the inverted route of the two lexical first stages, BM25Index(postings=True) and
SparseCorpusIndex(postings=True).  The forward route scores every stored document for every query from its (term,
weight) slots, Q * N * terms * 8 bytes per search; this route turns the slots into per-block inverted lists once and a
search reads only the lists of the query's terms (term-at-a-time, as every text search engine does).

Format (include/polus_hip.h has it to the bit).  The N documents are cut into blocks of `block_docs` consecutive ids, a
power of two in [64, 32768].  A forward slot (id, w) is a posting iff 0 <= id < V and w != 0.  Per block the postings
are in CSR form over the terms: offsets int32 [nblk, V + 1], base int64 [nblk + 1] (the exclusive scan of the block
totals, base[nblk] = P), post_doc int16 [P] (the bits of the unsigned id local to the block) and post_w f32 [P].  The
order inside a list is unspecified; lists as sets, offsets and base are exact.

Score rule.  acc = +0.0; the query's entries (ascending term id) are taken in order and a document holding the term
gets acc = f32(acc + f32(q_w * w)): one rounding each, no fma, so NumPy float32 arithmetic gives the same bits and the
bits do not depend on the order inside a list, the chunking or the grid.  A document without a matching term scores
0.0 and is still ranked.  On the forward route the same sum runs in slot order through an fma chain and a shuffle tree,
so the two routes agree bit for bit only where every sum is exact; otherwise they differ by rounding.

Build: ops.postings_count -> ops.postings_offsets -> one 8-byte copy of base[nblk] to the host, which sizes the arrays
-> ops.postings_fill.  A full rebuild per refresh; counts and cursor are one scratch buffer of nblk * V int32, released
afterwards.  Search: the chunked scan of the other indexes (store.topk_scan) over ops.postings_scores; a chunk is as many
whole blocks as fit `scratch_bytes`.  The owning index marks the postings `stale` when its forward arrays change, and
`update` rebuilds them before the next use.

Arithmetic is hand-written HIP (ops.postings_* / sparse_compact_rows / bm25_query_lists / topk_merge); torch
allocates, views and copies."""
import torch

from .. import ops
from .store import topk_scan

MIN_BLOCK_DOCS, MAX_BLOCK_DOCS = 64, 32768
MAX_POSTINGS_VOCAB = (1 << 31) - 2


def check_block_docs(block_docs):
    bd = int(block_docs)
    if not (MIN_BLOCK_DOCS <= bd <= MAX_BLOCK_DOCS and bd & (bd - 1) == 0):
        raise ValueError(f"block_docs must be a power of two in [{MIN_BLOCK_DOCS}, {MAX_BLOCK_DOCS}] (got {block_docs})")
    return bd


def block_chunks(n_docs, Q, block_docs, scratch_bytes):
    """[(first block, blocks), ...]: the launches of a search with Q queries over n_docs documents: as many whole blocks
    as `scratch_bytes` holds f32 scores of, at least one."""
    nblk = (int(n_docs) + block_docs - 1) // block_docs
    per = int(scratch_bytes) // (4 * int(Q) * block_docs)
    if per < 1:
        raise ValueError(f"scratch_bytes = {scratch_bytes} does not hold the scores of one block of {block_docs} documents "
                         f"for {Q} queries ({4 * int(Q) * block_docs} bytes): raise it or lower block_docs")
    return [(b, min(per, nblk - b)) for b in range(0, nblk, per)]


class Postings:
    """The built postings of one index and the search over them (see the module docstring)."""

    def __init__(self, block_docs):
        self.block_docs = check_block_docs(block_docs)
        self.clear()

    def clear(self):
        self.offsets = self.base = self.post_doc = self.post_w = None
        self.n_docs = self.vocab = self.count = 0
        self.stale = False

    @property
    def built(self):
        return self.offsets is not None

    @property
    def nbytes(self):
        if not self.built:
            return 0
        return 4 * self.offsets.numel() + 8 * self.base.numel() + 6 * self.count

    def arrays(self):
        return self.offsets, self.base, self.post_doc, self.post_w

    def update(self, forward):
        """Bring the postings up to date: `build` from forward() = (ids, w, V) when they are stale or were never built."""
        if self.stale or not self.built:
            self.build(*forward())
        return self

    def build(self, ids, w, V):
        """Rebuild from the forward arrays ids int32 / w f32 [N, M] (views of the index's storage)."""
        N, bd, dev = ids.shape[0], self.block_docs, ids.device
        nblk = (N + bd - 1) // bd
        if nblk * int(V) >= 1 << 31:
            raise ValueError(f"{nblk} blocks x {V} terms do not fit the int32 index of the offsets: raise block_docs")
        scratch = torch.empty((nblk, V), dtype=torch.int32, device=dev)           # counts, then fill's cursor
        offsets = torch.empty((nblk, V + 1), dtype=torch.int32, device=dev)
        base = torch.empty((nblk + 1,), dtype=torch.int64, device=dev)
        ops.postings_count(ids, w, V, bd, scratch)
        ops.postings_offsets(scratch, offsets, base)
        P = int(base[nblk:].cpu()[0])                                             # 8 bytes: the build's one synchronisation
        post_doc = torch.empty((P,), dtype=torch.int16, device=dev)
        post_w = torch.empty((P,), dtype=torch.float32, device=dev)
        ops.postings_fill(ids, w, bd, offsets, base, scratch, post_doc, post_w)
        self.offsets, self.base, self.post_doc, self.post_w = offsets, base, post_doc, post_w
        self.n_docs, self.vocab, self.count, self.stale = N, int(V), P, False

    def search(self, q_terms, q_w, q_count, k, scratch_bytes):
        """(scores f32 [Q, k], ids int32 [Q, k]) of the query lists over the built postings."""
        Q, bd, N = q_terms.shape[0], self.block_docs, self.n_docs
        spans = [(b0 * bd, min((b0 + nb) * bd, N)) for b0, nb in block_chunks(N, Q, bd, scratch_bytes)]

        def score(a, b, s):
            ops.postings_scores(q_terms, q_w, q_count, self.offsets, self.base, self.post_doc, self.post_w, bd, a // bd,
                                (b - a + bd - 1) // bd, N, s)
        return topk_scan(Q, k, spans, q_terms.device, score)
