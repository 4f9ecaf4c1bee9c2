"""Hybrid retrieval: the ranked lists of several first stages fused into one, on the device.

    hybrid = HybridSearch([bm25_index, cls_index], depth=1000)      # any stages with search(queries, k) and add(documents)
    for docs in corpus_batches: hybrid.add(docs)                    # every stage gets the batch and must number it alike
    scores, ids = hybrid.search(queries, k=100)                     # f32 / int32 [Q, k] on the device
    cand, count = hybrid.candidates(queries)                        # the union alone, ascending, padded with -1
    two = TwoStageSearch(hybrid, token_index, 1000)                 # a first stage like any other
    neg, n_pool, col = mine_negatives(hybrid, queries, positives, k=7, depth=200)

Lexical + dense is the combination tried first, and the union of two top-1000 lists is the usual candidate set of a
ColBERT or cross-encoder stage.  `search` asks every stage for its `depth` best documents, joins the lists by document
id and fuses their scores in one launch (ops.fuse_lists), and ranks the fused scores with ops.topk_merge: the contract
of every other `search` here (score descending, ties to the lower id, the tail (-inf, -1)).

Methods.  With rank the 1-based position of a document in a stage's list, counting only entries with a valid id and a
finite score, and w the stage's weight:

    "rrf"     sum over the stages that returned it of  w / (rrf_k + rank)       (Cormack et al. 2009; rrf_k = 60)
    "sum"     sum of  w * score                                                 (CombSUM)
    "minmax"  sum of  w * (score - lo) / (hi - lo),  lo and hi over the stage's own list for that query

A stage that did not return a document adds nothing for it; under "minmax" the worst document a stage returned also
gets 0 from it.  Every operation is one f32 rounding and a document's terms are added in stage order, so the fused
scores are specified to the bit (include/polus_hip.h polus_fuse_lists) and two documents that tie do so exactly.

The union comes out with ascending ids because that is the candidate row CorpusIndex.probe hands out and
CorpusIndex.rerank, CrossEncoderIndex.score and ops.topk_merge already read, negative ids meaning "missing".

Not measured: the retrieval quality of any method, weight or rrf_k on a real collection.

Arithmetic is hand-written HIP (the stages' searches, ops.fuse_lists, ops.topk_merge); torch allocates, views and
copies."""
import math

import torch

from .. import ops
from .search import MAX_K, CorpusIndex

METHODS = tuple(ops.FUSE_MODES)
MAX_LISTS = 8                 # lists per launch of ops.fuse_lists
MAX_ENTRIES = 4096            # entries per query over all lists


def _check_method(method, n_lists, weights, rrf_k):
    if method not in METHODS:
        raise ValueError(f"method must be one of {METHODS} (got {method!r})")
    if not 1 <= n_lists <= MAX_LISTS:
        raise ValueError(f"need between 1 and {MAX_LISTS} ranked lists (got {n_lists})")
    if weights is not None:
        weights = [float(w) for w in weights]
        if len(weights) != n_lists or not all(math.isfinite(w) for w in weights):
            raise ValueError(f"weights must be {n_lists} finite numbers, one per list (got {weights})")
    if not (math.isfinite(float(rrf_k)) and float(rrf_k) >= 0.0):
        raise ValueError(f"rrf_k must be finite and >= 0 (got {rrf_k})")
    return weights


def fuse(results, n_docs, method="rrf", weights=None, rrf_k=60.0):
    """(ids int32 [Q, L * C], values f32 [Q, L * C], count int32 [Q]) on the device from `results`, a sequence of L
    (scores, ids) pairs as `search` returns them (f32 / int32 [Q, C_l] device tensors): per query the distinct document
    ids of the L lists in ascending order with their fused scores, then (-1, -inf); count is how many.  C is the widest
    list; a narrower one is padded with (-inf, -1).  Ids outside [0, n_docs) and entries with a non-finite score take
    no part and no rank.  The rule is the module docstring's."""
    results = list(results)
    weights = _check_method(method, len(results), weights, rrf_k)
    Q, dev = results[0][1].shape[0], results[0][1].device
    for s, i in results:
        if i.dim() != 2 or tuple(s.shape) != tuple(i.shape) or i.shape[0] != Q or i.shape[1] < 1:
            raise ValueError(f"every result is a pair of [{Q}, C] tensors (got scores {tuple(s.shape)}, ids {tuple(i.shape)})")
    L, C = len(results), max(i.shape[1] for _, i in results)
    if L * C > MAX_ENTRIES:
        raise ValueError(f"{L} lists of up to {C} entries: ops.fuse_lists joins at most {MAX_ENTRIES} entries per query")
    ragged = any(i.shape[1] != C for _, i in results)
    ids = torch.full((L, Q, C), -1, dtype=torch.int32, device=dev) if ragged else torch.empty((L, Q, C), dtype=torch.int32, device=dev)
    scores = (torch.full((L, Q, C), -math.inf, dtype=torch.float32, device=dev) if ragged
              else torch.empty((L, Q, C), dtype=torch.float32, device=dev))
    for l, (s, i) in enumerate(results):
        ids[l, :, :i.shape[1]].copy_(i)
        scores[l, :, :i.shape[1]].copy_(s)
    out_id = torch.empty((Q, L * C), dtype=torch.int32, device=dev)
    out_val = torch.empty((Q, L * C), dtype=torch.float32, device=dev)
    count = torch.empty((Q,), dtype=torch.int32, device=dev)
    ops.fuse_lists(ids, scores, out_id, out_val, count, n_docs, method, weights=weights, rrf_k=rrf_k)
    return out_id, out_val, count


class HybridSearch:
    """Several first stages searched side by side and fused: `stages` is a sequence of 1 to 8 indexes with
    search(queries, k) -> (scores, ids) and add(documents) -> ids that hold the same documents under the same ids (a
    BM25Index, a SparseCorpusIndex, a CorpusIndex ...); `depth` is how many documents each stage contributes per query;
    `method`, `weights` (one per stage, None: all 1) and `rrf_k` are `fuse`'s.  len(stages) * depth is at most 4096, the
    entries ops.fuse_lists joins per query, and a CorpusIndex returns at most 1024 results per query, so with one among
    the stages `depth` is at most 1024."""

    def __init__(self, stages, depth, method="rrf", weights=None, rrf_k=60.0):
        self.stages = list(stages)
        self.weights = _check_method(method, len(self.stages), weights, rrf_k)
        if int(depth) < 1:
            raise ValueError(f"depth must be >= 1 (got {depth})")
        if len(self.stages) * int(depth) > MAX_ENTRIES:
            raise ValueError(f"{len(self.stages)} stages at depth {depth}: len(stages) * depth must be <= {MAX_ENTRIES}, "
                             "the entries ops.fuse_lists joins per query")
        if int(depth) > MAX_K and any(isinstance(s, CorpusIndex) for s in self.stages):
            raise ValueError(f"a CorpusIndex among the stages returns at most {MAX_K} results per query (got depth {depth})")
        self.depth, self.method, self.rrf_k = int(depth), method, float(rrf_k)

    def __len__(self):
        return len(self.stages[0])

    def add(self, documents):
        """Add a batch to every stage; returns its ids.  The stages must number it alike."""
        first = self.stages[0].add(documents)
        for stage in self.stages[1:]:
            ids = stage.add(documents)
            if tuple(ids.shape) != tuple(first.shape) or not bool((torch.as_tensor(ids).to(first.device) == first).all()):
                raise ValueError("the stages gave a document batch different ids: they must hold the same documents in "
                                 "the same order")
        return first

    def _fused(self, queries):
        return fuse([stage.search(queries, self.depth) for stage in self.stages], len(self), self.method, self.weights,
                    self.rrf_k)

    def candidates(self, queries):
        """(ids int32 [Q, len(stages) * depth], count int32 [Q]) on the device: per query the union of the stages' top
        `depth`, ascending, the rest of the row -1: ready for CorpusIndex.rerank or CrossEncoderIndex.score."""
        ids, _, count = self._fused(queries)
        return ids, count

    def search(self, queries, k):
        """(scores f32 [Q, k], ids int32 [Q, k]) on the device: per query the k best documents by fused score, score
        descending, ties to the lower id; when the union holds fewer than k, the tail is (-inf, -1)."""
        if not 1 <= int(k) <= MAX_K:
            raise ValueError(f"need 1 <= k <= {MAX_K}, the limit of ops.topk_merge (got {k})")
        ids, values, _ = self._fused(queries)
        top_val = torch.empty((ids.shape[0], int(k)), dtype=torch.float32, device=ids.device)
        top_id = torch.empty((ids.shape[0], int(k)), dtype=torch.int32, device=ids.device)
        ops.topk_merge(values, top_val, top_id, init=True, ids=ids)
        return top_val, top_id
