"""What the indexes of polus_amd/ir share: the chunk rule of a search (score_chunks), the chunked top-k scan (topk_scan),
the candidate contract of a rerank (check_candidates) and the growing device buffers documents are stored in (RowStore).
torch allocates, views and copies; the arithmetic is the callers' (ops.*) and ops.topk_merge."""
import operator

import numpy as np
import torch

from .. import ops

MAX_CHUNK = 65535             # columns per launch: the MaxSim grid's limit, kept on every other path too


def score_chunks(total, Q, scratch_bytes, what, item_bytes=0):
    """[(start, stop), ...]: the ranges of `total` columns (`what`: "document" or "candidate") a search with Q queries scores,
    one launch each: at most 65535 columns, and at most as many as keep the [Q, n] f32 scores within scratch_bytes.  With
    item_bytes (a residual index's `search`: the bytes of one decoded document) the n items of a chunk stay within
    scratch_bytes as well."""
    per = min(MAX_CHUNK, scratch_bytes // (4 * int(Q)))
    if per < 1:
        raise ValueError(f"scratch_bytes = {scratch_bytes} does not hold the scores of one {what} for "
                         f"{Q} queries ({4 * int(Q)} bytes)")
    if item_bytes and total:
        if scratch_bytes < item_bytes:
            raise ValueError(f"scratch_bytes = {scratch_bytes} does not hold one decoded {what} ({item_bytes} bytes)")
        per = min(per, scratch_bytes // item_bytes)
    return [(s, min(s + per, int(total))) for s in range(0, int(total), per)]


def topk_scan(Q, k, spans, device, score, ids=None, top=None):
    """(top_val f32 [Q, k], top_id int32 [Q, k]) on `device`: the exact top-k over the columns of `spans`, a span at a time
    through one [Q, widest span] f32 scratch: score(a, b, s) writes the scores of columns a .. b into s [Q, b - a], and
    ops.topk_merge folds them in, starting a new state on the first span.  Column c is document c, or ids[:, c] with `ids`
    (int32 [Q, columns]: the candidates of a rerank).  `top` = (top_val, top_id) merges into the caller's buffers."""
    scratch = torch.empty((Q, max(b - a for a, b in spans)), dtype=torch.float32, device=device)
    top_val, top_id = top or (torch.empty((Q, int(k)), dtype=torch.float32, device=device),
                              torch.empty((Q, int(k)), dtype=torch.int32, device=device))
    for i, (a, b) in enumerate(spans):
        s = scratch[:, :b - a]
        score(a, b, s)
        if ids is None:
            ops.topk_merge(s, top_val, top_id, id0=a, init=(i == 0))
        else:
            ops.topk_merge(s, top_val, top_id, init=(i == 0), ids=ids[:, a:b])
    return top_val, top_id


def check_candidates(candidates, Q, n_docs, dev):
    """The candidate contract of CorpusIndex.rerank: an integer [Q, C] array of document ids padded with -1.  A host
    array is checked (an id outside [-1, n_docs) raises ValueError) and copied over; a device tensor must be int32 and
    is taken as it is, values unseen."""
    if isinstance(candidates, torch.Tensor) and candidates.is_cuda:
        cand = candidates
        if cand.dtype != torch.int32:
            raise ValueError(f"candidates on the device must be int32, the ids a search returns (got {cand.dtype})")
        host = None
    else:
        host = candidates.numpy() if isinstance(candidates, torch.Tensor) else np.asarray(candidates)
        if host.dtype.kind not in "iu":
            raise ValueError(f"candidates must be integers (got {host.dtype})")
        if host.size and (int(host.min()) < -1 or int(host.max()) >= n_docs):
            raise ValueError(f"candidates must lie in [-1, {n_docs}) (got {int(host.min())} .. {int(host.max())})")
        cand = host
    if cand.ndim != 2 or cand.shape[0] != Q or cand.shape[1] < 1:
        raise ValueError(f"candidates must be [{Q}, C] with C >= 1 (got {tuple(cand.shape)})")
    if host is not None:
        return torch.as_tensor(np.ascontiguousarray(host.astype(np.int32))).to(dev)
    return cand if cand.stride(1) == 1 else cand.contiguous()


class RowStore:
    """The stored rows of an index: `n` rows in named device buffers [capacity, *tail] that grow together.  A field is
    declared by tail shape, dtype and fill value; the fill is part of the contract, because what `add` does not write
    (the padding of a short document, the rows beyond n) is never written afterwards: -1 for term ids and centroid
    codes, 0 everywhere else."""

    def __init__(self):
        self.n, self.fields, self.bufs = 0, {}, {}

    @property
    def capacity(self):
        return next((b.shape[0] for b in self.bufs.values()), 0)

    def declare(self, **fields):
        """name=(tail shape, dtype, fill): new fields, or old ones again.  Once the store has buffers a declared field's
        buffer is made at once, all fill (CorpusIndex gains its centroid codes on a filled index)."""
        for name, (tail, dtype, fill) in fields.items():
            self.fields[name] = (tuple(tail), dtype, fill)
            if self.bufs:
                self.bufs[name] = self._new(name, self.capacity, next(iter(self.bufs.values())).device)

    def _new(self, name, cap, device):
        tail, dtype, fill = self.fields[name]
        if fill == 0:
            return torch.zeros((cap,) + tail, dtype=dtype, device=device)
        return torch.full((cap,) + tail, fill, dtype=dtype, device=device)

    def reserve(self, need, device):
        """Room for `need` rows: the capacity doubles, the first n rows are copied over."""
        cap = self.capacity
        if need <= cap:
            return
        cap = max(need, 2 * cap)
        for name in self.fields:
            new = self._new(name, cap, device)
            if self.n:
                new[:self.n].copy_(self.bufs[name][:self.n])
            self.bufs[name] = new

    def view(self, name):
        """buf[:n], None before the first reserve (or for a field the index does not have)."""
        buf = self.bufs.get(name)
        return None if buf is None else buf[:self.n]


def stored(name):
    """A property of an index over its `_store`: the whole buffer of a field, None while there is none (settable: tests
    put stand-ins there)."""
    return property(lambda self: self._store.bufs.get(name), lambda self, buf: self._store.bufs.__setitem__(name, buf))


stored_rows = property(operator.attrgetter("_store.n"), lambda self, n: setattr(self._store, "n", n),
                       doc="A property of an index over its `_store`: the number of stored rows.")
