"""Hard-negative mining: from a first-stage search to the (question, positive, negatives[, teacher_scores]) batches of
the trainers, without the candidate ids leaving the device.

    index = BM25Index(30522); ...add the corpus...        # or any index with search(queries, k) -> (scores, ids)
    mined = mine_tuples(index, queries, positives, k=7, depth=200, min_score=0.0, teacher=cross_index)
    batch = tuple_batch(cross_index, take_rows(queries, mined.rows), mined.tuples, mined.teacher_scores)
    trainer.train_step(*batch)

The recipe of ColBERTv2, the SPLADE distillation runs and monoBERT: retrieve the top `depth` passages per training
query with a cheap first stage, drop the known positives, sample k negatives from what is left, optionally score the
tuples with a cross-encoder teacher.

Sampling rule (ops.mine_negatives; include/polus_hip.h polus_mine_negatives).  The pool of a query is its candidates
from rank `skip_top` on that are not among its positives and, with `min_score`, score above it (min_score = 0 drops the
documents a BM25 search ranks although they share no term with the query).  A pool of at most k goes out whole.  A
larger pool of R is cut into k rank strata [floor(j R / k), floor((j + 1) R / k)) and each stratum gives one draw,
position lo + hash32(seed, row * k + j) mod (hi - lo): the negatives come out in rank order, are distinct, span the
whole depth, and are the same for the same seed.

Arithmetic is hand-written HIP (the first stage's search, ops.mine_negatives, the teacher); torch allocates, views,
copies and gathers rows by index."""
import collections

import numpy as np
import torch

from .. import ops
from ..tensor import to_device

MinedTuples = collections.namedtuple("MinedTuples", "tuples rows teacher_scores n_pool dropped")


def _positives(positives, Q, dev):
    """An integer [Q, P] array padded with -1 (or [Q]: one positive each), host or device -> (int32 device [Q, P], the
    host copy of its first column or None when the input lives on the device)."""
    if isinstance(positives, torch.Tensor) and positives.is_cuda:
        pos, first = positives, None
        if pos.dtype != torch.int32:
            raise ValueError(f"positives on the device must be int32 (got {pos.dtype})")
        if pos.dim() == 1:
            pos = pos[:, None]
    else:
        h = positives.numpy() if isinstance(positives, torch.Tensor) else np.asarray(positives)
        if h.dtype.kind not in "iu":
            raise ValueError(f"positives must be integers (got {h.dtype})")
        if h.ndim == 1:
            h = h[:, None]
        if h.size and (int(h.min()) < -1 or int(h.max()) > 2 ** 31 - 1):
            raise ValueError("positives must be document ids, padded with -1")
        pos, first = h, (h[:, 0].copy() if h.ndim == 2 and h.shape[1] else None)
    if pos.ndim != 2 or pos.shape[0] != Q or pos.shape[1] < 1:
        raise ValueError(f"positives must be [{Q}, P] with P >= 1 (got {tuple(pos.shape)})")
    if pos.shape[1] > 1024:
        raise ValueError(f"at most 1024 positives per query (got {pos.shape[1]})")
    if first is not None:
        return torch.as_tensor(np.ascontiguousarray(pos.astype(np.int32))).to(dev), first
    return pos.contiguous(), None


def _mine(first, queries, positives, k, depth, skip_top, min_score, seed):
    k, depth = int(k), int(depth)
    if k < 1 or k > 1024 or depth < 1:
        raise ValueError(f"need 1 <= k <= 1024 and depth >= 1 (got k = {k}, depth = {depth})")
    if int(skip_top) < 0:
        raise ValueError(f"skip_top must be >= 0 (got {skip_top})")
    scores, ids = first.search(queries, depth)
    Q, dev = ids.shape[0], ids.device
    pos, pos_first = _positives(positives, Q, dev)
    neg = torch.empty((Q, k), dtype=torch.int32, device=dev)
    neg_col = torch.empty((Q, k), dtype=torch.int32, device=dev)
    n_pool = torch.empty((Q,), dtype=torch.int32, device=dev)
    ops.mine_negatives(ids, neg, n_pool, score=None if min_score is None else scores, exclude=pos, skip_top=int(skip_top),
                       min_score=0.0 if min_score is None else float(min_score), seed=int(seed), neg_col=neg_col)
    return neg, n_pool, neg_col, pos, pos_first


def mine_negatives(first, queries, positives, k, depth, skip_top=0, min_score=None, seed=0):
    """(neg int32 [Q, k], n_pool int32 [Q], neg_col int32 [Q, k]), all on the device: k negatives per query sampled from
    `first.search(queries, depth)` by the rule of the module docstring, the size of each query's pool, and the rank
    (column of the search result) each negative came from.  `positives` is an integer [Q, P] array of document ids padded
    with -1, host or device.  A query whose pool holds fewer than k gets them all, then -1.  `min_score` = None ignores
    the scores."""
    return _mine(first, queries, positives, k, depth, skip_top, min_score, seed)[:3]


def take_rows(batch, rows):
    """The rows `rows` (a host integer array) of every array of a {"input_ids", "attention_mask", ...} dict: host arrays
    are indexed on the host, device tensors on the device."""
    rows = np.asarray(rows, np.int64)
    out = {}
    for key, v in batch.items():
        if isinstance(v, torch.Tensor):
            out[key] = v[torch.as_tensor(rows).to(v.device)]
        else:
            out[key] = np.asarray(v)[rows]
    return out


def mine_tuples(first, queries, positives, k, depth, skip_top=0, min_score=None, seed=0, teacher=None):
    """MinedTuples(tuples, rows, teacher_scores, n_pool, dropped).  tuples int32 [Q', 1 + k] on the device: positives[:, 0]
    then the k mined negatives, for the queries that have a positive and a pool of at least k; rows (host int64 [Q']) are
    those queries' positions, dropped = Q - Q'.  Finding them is one copy of the Q pool sizes to the host (and of the Q
    first positives when `positives` lives on the device).  With a `teacher` (anything with CrossEncoderIndex.score's
    contract) teacher_scores = teacher.score(the kept queries, tuples), f32 [Q', 1 + k]: a ready last element of a
    distillation batch.  n_pool is mine_negatives' (device int32 [Q])."""
    neg, n_pool, _, pos, pos_first = _mine(first, queries, positives, k, depth, skip_top, min_score, seed)
    if pos_first is None:
        pos_first = pos[:, 0].cpu().numpy()
    rows = np.nonzero((n_pool.cpu().numpy() >= int(k)) & (pos_first >= 0))[0].astype(np.int64)
    dev = neg.device
    sel = torch.as_tensor(rows).to(dev)
    tuples = torch.empty((rows.size, 1 + int(k)), dtype=torch.int32, device=dev)
    tuples[:, 0].copy_(pos[:, 0][sel])
    tuples[:, 1:].copy_(neg[sel])
    scores = None
    if teacher is not None:
        scores = (teacher.score(take_rows(queries, rows), tuples) if rows.size
                  else torch.empty((0, 1 + int(k)), dtype=torch.float32, device=dev))
    return MinedTuples(tuples, rows, scores, n_pool, int(n_pool.numel() - rows.size))


def tuple_batch(store, queries, tuples, teacher_scores=None):
    """The trainers' batch (question, positive_doc, negative_doc[, teacher_scores]) of n-way tuples.  `store` is a token
    store: a CrossEncoderIndex (its token_ids / mask) or a pair (ids, mask) of int32 [N, L] device tensors; `queries`
    holds one row per tuple (take_rows(queries, mined.rows)); `tuples` is int32 [B, 1 + k] document ids, positive first,
    every id in [0, N) (values on the device are not checked).  positive_doc is [B, L], negative_doc [B, k, L], both
    gathered by torch row indexing (a copy).  CrossEncoderTrainer, EfficientDenseRetrievalTrainer and
    SparseRetrievalTrainer take the result as it is."""
    ids, mask = (store.token_ids, store.mask) if hasattr(store, "token_ids") else store
    if ids is None:
        raise ValueError("the token store is empty")
    if ids.dim() != 2 or tuple(mask.shape) != tuple(ids.shape):
        raise ValueError(f"a token store is two [N, L] tensors (got {list(ids.shape)} and {list(mask.shape)})")
    t = to_device(tuples, torch.int32, ids.device) if not (isinstance(tuples, torch.Tensor) and tuples.is_cuda) else tuples
    if t.dim() != 2 or t.shape[1] < 1:
        raise ValueError(f"tuples must be [B, 1 + k] (got {list(t.shape)})")
    B = t.shape[0]
    nq = np.shape(queries["input_ids"])[0]
    if nq != B:
        raise ValueError(f"{nq} queries for {B} tuples: select the kept queries with take_rows(queries, mined.rows)")
    idx = t.long()
    pos = {"input_ids": ids[idx[:, 0]], "attention_mask": mask[idx[:, 0]]}
    out = (queries, pos)
    if t.shape[1] > 1:
        out += ({"input_ids": ids[idx[:, 1:]], "attention_mask": mask[idx[:, 1:]]},)
    elif teacher_scores is not None:
        raise ValueError("teacher_scores need negatives: a one-column tuple has nothing to contrast")
    return out if teacher_scores is None else out + (teacher_scores,)
