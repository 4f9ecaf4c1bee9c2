"""Cross-encoder reranking: the last stage of a retrieval pipeline, and the teacher of the distillation losses.

    cross = CrossEncoderIndex(model)                      # a CrossEncoder (polus_amd/ir/models.py)
    for docs in corpus_batches: cross.add(docs)           # {"input_ids", "attention_mask"}: token ids stay on the device
    teacher = cross.score(queries, candidates)            # f32 [Q, C] in candidate order, -inf for a missing candidate
    scores, ids = cross.rerank(queries, candidates, k)    # the contract of CorpusIndex.rerank
    three = TwoStageSearch(TwoStageSearch(splade, colbert, 1000), cross, 100)

Nothing is encoded ahead of time: a cross-encoder reads query and document as ONE sequence, so the index stores token
ids (8 * doc_tokens bytes per document: int32 ids and int32 mask) and every call pays the whole encoder per pair.  The
pair rows `cls q sep d sep` are built on the device from the candidate ids (ops.pair_pack); the candidate ids of a
search never visit the host.

Bucketing.  Passages are far shorter than `max_length`, and the encoder's GEMMs and row-wise kernels run on every
padded token.  `score` therefore asks ops.pair_lengths for the real length of each of the Q C pairs, copies those Q C
integers to the host (the one synchronisation of a call), sorts the pairs by length (plan_buckets) and runs them in
buckets whose S is the bucket's longest pair rounded up to `round_to`.  ops.pair_scatter_scores puts every bucket's
scores back into candidate order.  `bucket=False` runs the pairs in candidate order at S = max_length in chunks of the
same token budget, without the copy.

Arithmetic is hand-written HIP (ops.pair_lengths / pair_pack / pair_scatter_scores, the encoder's kernels,
ops.topk_merge); torch allocates, views and copies."""
import numpy as np
import torch

from .. import ops
from ..callbacks import ValidationDataCallback
from ..tensor import to_device
from .store import RowStore, check_candidates, stored, stored_rows

MAX_K = 1024                  # results per query: the limit of ops.topk_merge


def plan_buckets(lengths, tokens_per_batch, round_to=64, max_length=None):
    """Pure host function: [(S, rows), ...] for the pairs whose real lengths are `lengths` (1-d integers).  The pairs go
    in descending length, ties by pair index; a bucket's S is its first (longest) length rounded up to a multiple of
    `round_to` and capped at `max_length`; a bucket takes max(1, tokens_per_batch // S) rows.  `rows` is the int32
    array of the bucket's pair indices.  Every pair appears exactly once."""
    lengths = np.asarray(lengths).reshape(-1)
    if lengths.dtype.kind not in "iu":
        raise ValueError(f"lengths must be integers (got {lengths.dtype})")
    tokens_per_batch, round_to = int(tokens_per_batch), int(round_to)
    if tokens_per_batch < 1 or round_to < 1:
        raise ValueError(f"tokens_per_batch and round_to must be >= 1 (got {tokens_per_batch}, {round_to})")
    if lengths.size and int(lengths.min()) < 1:
        raise ValueError("a pair row has at least its three special tokens: lengths must be >= 1")
    if max_length is not None and lengths.size and int(lengths.max()) > int(max_length):
        raise ValueError(f"a length of {int(lengths.max())} exceeds max_length = {max_length}")
    order = np.argsort(-lengths.astype(np.int64), kind="stable").astype(np.int32)
    out, at = [], 0
    while at < order.size:
        S = (int(lengths[order[at]]) + round_to - 1) // round_to * round_to
        if max_length is not None:
            S = min(S, int(max_length))
        n = max(1, tokens_per_batch // S)
        out.append((S, order[at:at + n]))
        at += n
    return out


class CrossEncoderIndex:
    """A token store + a CrossEncoder: `score` and `rerank` over candidate ids (see the module docstring).

    `doc_tokens` is the stored length per document (None: the width of the first batch added); narrower batches are
    padded with masked tokens, wider ones raise.  `strip` = (head, tail) tokens taken off every valid query and document
    row before the pair is built: (1, 1) removes the [CLS] and [SEP] of HF-tokenised inputs, (0, 0) takes raw ids.  A query
    keeps at most `max_query_tokens`, the document gets the rest of the `max_length` row.  `tokens_per_batch` is the
    budget rows x S of one pass through the encoder."""

    def __init__(self, model, doc_tokens=None, strip=(1, 1), max_query_tokens=64, max_length=256, cls_token_id=101,
                 sep_token_id=102, pad_token_id=0, tokens_per_batch=32768, bucket=True, round_to=64):
        self.model = model
        self.strip = (int(strip[0]), int(strip[1]))
        self.max_query_tokens, self.max_length = int(max_query_tokens), int(max_length)
        self.special = (int(cls_token_id), int(sep_token_id), int(pad_token_id))
        self.tokens_per_batch, self.bucket, self.round_to = int(tokens_per_batch), bool(bucket), int(round_to)
        if not all(0 <= s <= 8 for s in self.strip):
            raise ValueError(f"strip counts must be in 0..8, got {strip}")
        if self.max_query_tokens < 0 or self.max_length < self.max_query_tokens + 3:
            raise ValueError(f"max_length ({max_length}) must be at least max_query_tokens ({max_query_tokens}) + 3")
        if self.tokens_per_batch < 1 or self.round_to < 1:
            raise ValueError("tokens_per_batch and round_to must be >= 1")
        if doc_tokens is not None and int(doc_tokens) < 1:
            raise ValueError(f"doc_tokens must be >= 1 (got {doc_tokens})")
        cfg = getattr(model, "config", None)
        if cfg is not None:
            if self.max_length > cfg.max_position_embeddings:
                raise ValueError(f"max_length {max_length} exceeds the model's {cfg.max_position_embeddings} positions")
            if not all(0 <= t < cfg.vocab_size for t in self.special):
                raise ValueError(f"special token ids {self.special} must lie in the vocabulary [0, {cfg.vocab_size})")
        self.doc_tokens = None if doc_tokens is None else int(doc_tokens)
        self.last_plan = None         # [(S, rows in the bucket), ...] of the last `score`
        self.clear()

    def clear(self):
        self._store = RowStore()

    _n, _ids, _mask = stored_rows, stored("ids"), stored("mask")

    def __len__(self):
        return self._n

    @property
    def nbytes(self):
        """Bytes the stored documents take: int32 ids and int32 mask, 8 * doc_tokens per document."""
        return 8 * (self.doc_tokens or 0) * self._n

    @property
    def token_ids(self):
        return None if self._ids is None else self._ids[:self._n]

    @property
    def mask(self):
        return None if self._mask is None else self._mask[:self._n]

    def _device(self):
        return self.model.arena.device

    def add(self, documents):
        """Append a batch {"input_ids" [n, L][, "attention_mask"]}; returns its ids, the consecutive int32 positions in
        the index (the numbering of CorpusIndex.add).  A batch wider than doc_tokens raises ValueError."""
        dev = self._device()
        ids = to_device(documents["input_ids"], torch.int32, dev)
        if ids.dim() != 2:
            raise ValueError(f"document input_ids must be [n, L] (got {list(ids.shape)})")
        n, L = ids.shape
        m = documents.get("attention_mask")
        if self.doc_tokens is None:
            self.doc_tokens = L
        if L > self.doc_tokens:
            raise ValueError(f"a document batch of {L} tokens does not fit the index's document length {self.doc_tokens}")
        if not self._store.fields:
            # zeros: the padding of documents shorter than doc_tokens is never written, and its mask is 0
            self._store.declare(ids=((self.doc_tokens,), torch.int32, 0), mask=((self.doc_tokens,), torch.int32, 0))
        a, b = self._n, self._n + n
        self._store.reserve(b, dev)
        self._ids[a:b, :L].copy_(ids)
        if m is None:
            self._mask[a:b, :L].fill_(1)
        else:
            self._mask[a:b, :L].copy_(to_device(m, torch.int32, dev).reshape(n, L))
        self._n = b
        return torch.arange(a, b, dtype=torch.int32, device=dev)

    def _queries(self, queries):
        dev = self._device()
        q = to_device(queries["input_ids"], torch.int32, dev)
        if q.dim() != 2:
            raise ValueError(f"query input_ids must be [Q, L] (got {list(q.shape)})")
        m = queries.get("attention_mask")
        return q, (None if m is None else to_device(m, torch.int32, dev).reshape(q.shape))

    def _run(self, q, qm, cand, rows, S, out):
        """One pass through the encoder: the pairs `rows` (int32 on the device) at row length S, scattered into out."""
        R = rows.numel()
        buf = torch.empty((3, R, S), dtype=torch.int32, device=q.device)
        d_ids, d_mask = self._ids[:self._n], self._mask[:self._n]
        ops.pair_pack(q, qm, d_ids, d_mask, cand, buf[0], buf[1], buf[2], self.strip + self.strip, self.max_query_tokens,
                      self.special, rows=rows)
        s = self.model(input_ids=buf[0], attention_mask=buf[2], token_type_ids=buf[1], training=False)
        ops.pair_scatter_scores(s, cand, self._n, out, rows=rows)

    def score(self, queries, candidates, bucket=None):
        """f32 [Q, C] on the device: the model's score of every query against each of its own candidates, in candidate
        order, -inf where the candidate id lies outside [0, len(index)): a ready `teacher_scores`.  `candidates` follows
        CorpusIndex.rerank's contract.  `bucket` overrides the index's setting for this call."""
        if self._n == 0:
            raise ValueError("the index is empty: add documents before scoring")
        q, qm = self._queries(queries)
        Q, Lq = q.shape
        cand = check_candidates(candidates, Q, self._n, q.device)
        C = cand.shape[1]
        if Q * C > 2 ** 31 - 1:
            raise ValueError(f"{Q} x {C} pairs exceed 2^31 - 1")
        out = torch.empty((Q, C), dtype=torch.float32, device=q.device)
        P, S = Q * C, self.max_length
        if self.bucket if bucket is None else bucket:
            length = torch.empty(P, dtype=torch.int32, device=q.device)
            ops.pair_lengths((Q, Lq), qm, (self._n, self.doc_tokens), self._mask[:self._n], cand, length,
                             self.strip + self.strip, self.max_query_tokens, S)
            plan = plan_buckets(length.cpu().numpy(), self.tokens_per_batch, self.round_to, S)      # the one D2H copy
            order = torch.as_tensor(np.concatenate([rows for _, rows in plan])).to(q.device)
            at = 0
            for s_b, rows in plan:
                self._run(q, qm, cand, order[at:at + rows.size], s_b, out)
                at += rows.size
            self.last_plan = [(s_b, rows.size) for s_b, rows in plan]
        else:
            per = max(1, self.tokens_per_batch // S)
            order = torch.arange(P, dtype=torch.int32, device=q.device)
            for at in range(0, P, per):
                self._run(q, qm, cand, order[at:at + per], S, out)
            self.last_plan = [(S, min(per, P - at)) for at in range(0, P, per)]
        return out

    def rerank(self, queries, candidates, k):
        """(scores f32 [Q, k], ids int32 [Q, k]) on the device: per query its k best candidates, score descending, ties
        to the lower id, (-inf, -1) behind the last one: the contract of CorpusIndex.rerank, so the index is a second
        stage of TwoStageSearch."""
        k = int(k)
        if not 1 <= k <= MAX_K:
            raise ValueError(f"k must be in 1..{MAX_K} (got {k})")
        q, _ = self._queries(queries)
        cand = check_candidates(candidates, q.shape[0], self._n, q.device)
        s = self.score(queries, cand)
        top_val = torch.empty((q.shape[0], k), dtype=torch.float32, device=s.device)
        top_id = torch.empty((q.shape[0], k), dtype=torch.int32, device=s.device)
        ops.topk_merge(s, top_val, top_id, init=True, ids=cand)
        return top_val, top_id


class RerankValidationCallback(ValidationDataCallback):
    """Validation of a reranker: every validation sample `(queries, candidates, relevant)` becomes `(ids [Q, k],
    relevant)` through CrossEncoderIndex.rerank with the trainer's current model, and the trainer's ranking metrics
    (polus_amd/ir/metrics.py) land in shared_dict["validation"][name].  The token store is filled once, from `corpus`
    (an iterable of document batches), at the first validated epoch: token ids do not change with the model.
    `index_kwargs` go to CrossEncoderIndex; by default the trainer's strip, lengths and special ids are used."""

    def __init__(self, corpus, tf_validation, k, name=None, validation_interval=1, show_progress=False, **index_kwargs):
        super().__init__(tf_validation, custom_inference_f=self._rank, name=name, show_progress=show_progress,
                         validation_interval=validation_interval)
        self.corpus, self.k, self.index_kwargs = corpus, int(k), index_kwargs
        self.index = None

    def _rank(self, model, sample):
        queries, candidates, relevant = sample
        return self.index.rerank(queries, candidates, self.k)[1], relevant

    def on_epoch_end(self, epoch):
        if epoch % self.validation_interval:
            return
        trainer = self.coordinator.trainer
        if self.index is None:
            kw = {}
            if hasattr(trainer, "special"):
                kw = dict(strip=trainer.strip, max_query_tokens=trainer.max_query_tokens, max_length=trainer.max_length,
                          cls_token_id=trainer.special[0], sep_token_id=trainer.special[1], pad_token_id=trainer.special[2])
            kw.update(self.index_kwargs)
            self.index = CrossEncoderIndex(trainer.model, **kw)
            for documents in self.corpus:
                self.index.add(documents)
        self.index.model = trainer.model
        super().on_epoch_end(epoch)
