"""BIO span decoding and strict entity matching over tag tensors (polus/ner/bio.py decode_bio, polus/ner/utils.py
eval_list_of_entity_sets), without the corpus object model.

The rule (DESIGN.md "NER entity metrics"; the kernels of csrc/bio.hip and this host path implement the same one):

* a tag scheme is an int32 table scheme[C]: -1 for an outside tag (O, PAD, anything that is not B-x / I-x), else
  2 * type + (1 for I-, 0 for B-);
* an optional mask [B, S] selects the tokens that take part; masked-out tokens are removed before decoding, so the kept
  tokens on either side of a hole are neighbours, and values at masked-out positions are never interpreted;
* a kept token is in an entity iff its tag is not outside; it starts one iff it is B-x, or I-x whose previous kept token
  is absent, outside or of another type (the lenient decoding of allow_errors=True); it ends one iff it is in one and
  the next kept token is absent, outside or a start;
* an entity is (row, start, end_exclusive = last kept column + 1, type); positions are original column indices;
* a kept tag id outside [0, C) decodes as outside and is counted as rejected.

The reference's decode_bio resets (s, e, t) inside its loop (polus/ner/bio.py:139-141), so every entity it decodes is
(-1, -1, "None"); that bug is not reproduced: this is the decoder its comments describe.

Host arrays are decoded here in NumPy, without a Python loop over tokens; device tensors by ops.bio_spans."""
import numpy as np

STAT_KEYS = ("tags", "rejected", "inside_tag_after_other_tag", "inside_tag_with_different_entity_type")


def parse_scheme(tag_names):
    """(scheme int32 [C], type_names): ["PAD", "O", "B-Chemical", "I-Chemical"] -> ([-1, -1, 0, 1], ["Chemical"]).
    Types are numbered in order of first appearance; an I-x without a B-x still defines type x."""
    names = list(tag_names)
    if not names:
        raise ValueError("parse_scheme: the list of tag names is empty")
    seen, types, scheme = set(), {}, []
    for name in names:
        if not isinstance(name, str):
            raise TypeError(f"parse_scheme: tag names are strings (got {name!r})")
        if name in seen:
            raise ValueError(f"parse_scheme: tag name {name!r} appears twice")
        seen.add(name)
        if len(name) > 2 and name[0] in "BI" and name[1] == "-":
            t = types.setdefault(name[2:], len(types))
            scheme.append(2 * t + (name[0] == "I"))
        else:
            scheme.append(-1)
    return np.asarray(scheme, np.int32), list(types)


def check_scheme(scheme, num_types=None):
    """The scheme as an int32 array and its number of types T; raises unless every entry is -1 or in [0, 2 T)."""
    s = np.asarray(scheme)
    if s.ndim != 1 or s.size == 0 or not np.issubdtype(s.dtype, np.integer):
        raise ValueError("scheme must be a non-empty one-dimensional integer table")
    if (s < -1).any():
        raise ValueError("scheme entries are -1 (outside) or 2 * type + (1 for I-)")
    T = max(int(s.max()) // 2 + 1, 1) if num_types is None else int(num_types)
    if T < 1 or int(s.max()) >= 2 * T:
        raise ValueError(f"scheme names type {int(s.max()) // 2} but there are only {T} type(s)")
    return s.astype(np.int32), T


def _np(x):
    if hasattr(x, "detach"):
        x = x.detach().cpu().numpy()
    return np.asarray(x)


def _rows(tags, mask):
    tags = _np(tags)
    if tags.ndim == 1:
        tags = tags[None]
    if tags.ndim != 2 or not np.issubdtype(tags.dtype, np.integer):
        raise ValueError(f"tags must be integer [B, S] or [S] (got {tags.dtype} {tags.shape})")
    if mask is None:
        keep = np.ones(tags.shape, bool)
    else:
        keep = _np(mask) != 0
        if keep.ndim == 1:
            keep = keep[None]
        if keep.shape != tags.shape:
            raise ValueError(f"mask {keep.shape} does not match tags {tags.shape}")
    return tags, keep


def device_rows(tags, mask):
    """A device tag tensor as int32 [B, S] with unit inner stride, and the mask (host or device, any dtype, nonzero =
    kept) as an int32 device tensor of the same shape; tensors that already have that form are passed through."""
    import torch
    t = tags if tags.dim() == 2 else tags.reshape(1, -1)
    t = t.to(torch.int32)
    if t.stride(1) != 1 and t.shape[1] != 1:
        t = t.contiguous()
    if mask is None:
        return t, None
    m = mask if hasattr(mask, "is_cuda") else torch.as_tensor(_np(mask))
    m = m.to(t.device).reshape(t.shape)
    if m.dtype != torch.int32:                     # the kernels keep a token whose int32 mask is nonzero
        m = (m != 0).to(torch.int32)
    if m.stride(1) != 1 and m.shape[1] != 1:
        m = m.contiguous()
    return t, m


class _Decoded:
    """The kept tokens of all rows, flattened in row-major order, with the rule's flags per token."""

    def __init__(self, tags, keep, scheme):
        C = scheme.size
        self.rows, self.cols = np.nonzero(keep)
        t = tags[self.rows, self.cols].astype(np.int64)
        bad = (t < 0) | (t >= C)
        code = np.where(bad, -1, scheme[np.clip(t, 0, C - 1)]).astype(np.int64)
        n = code.size
        first = np.ones(n, bool)                   # no previous kept token in the row
        first[1:] = self.rows[1:] != self.rows[:-1]
        prev = np.full(n, -1, np.int64)
        prev[1:] = code[:-1]
        prev[first] = -1
        inside = code >= 0
        inside_tag = inside & ((code & 1) == 1)
        after_other = inside_tag & (prev < 0)
        other_type = inside_tag & (prev >= 0) & ((prev >> 1) != (code >> 1))
        start = inside & (~inside_tag | after_other | other_type)
        last = np.ones(n, bool)                    # no next kept token in the row
        last[:-1] = first[1:]
        nxt_open = np.zeros(n, bool)               # the next kept token goes on with this entity
        nxt_open[:-1] = inside[1:] & ~start[1:]
        end = inside & (last | ~nxt_open)
        self.type = code >> 1
        self.start_at, self.end_at = np.nonzero(start)[0], np.nonzero(end)[0]     # pair up in order: one of each per entity
        self.stats = np.array([n, int(bad.sum()), int(after_other.sum()), int(other_type.sum())], np.int64)


def decode_bio(tags, scheme, mask=None, max_spans=None):
    """Entities of integer tags [B, S] (or [S]) under the rule above.

    Host arrays: (entities, stats) with entities[b] the list of (start, end_exclusive, type) of row b in order of
    start, and stats a dict with the reference's keys (tags, inside_tag_after_other_tag,
    inside_tag_with_different_entity_type) plus rejected.
    Device tensors: (spans, count) on the device, spans int32 [B, max_spans, 3] filled with -1 behind a row's
    entities and count int32 [B] the row's true number (ops.bio_spans); max_spans defaults to S, which always
    suffices.  Out-of-range ids decode as outside there too; pass a `rejected` tensor to ops.bio_spans to count them."""
    scheme, _ = check_scheme(scheme)
    if getattr(tags, "is_cuda", False):
        import torch
        from .. import ops
        t, m = device_rows(tags, mask)
        B, S = t.shape
        M = S if max_spans is None else int(max_spans)
        spans = torch.full((B, M, 3), -1, dtype=torch.int32, device=t.device)
        count = torch.zeros(B, dtype=torch.int32, device=t.device)
        ops.bio_spans(t, torch.as_tensor(scheme, device=t.device), spans, count, mask=m)
        return spans, count
    tags, keep = _rows(tags, mask)
    d = _Decoded(tags, keep, scheme)
    entities = [[] for _ in range(tags.shape[0])]
    for r, s, e, t in zip(d.rows[d.start_at].tolist(), d.cols[d.start_at].tolist(), (d.cols[d.end_at] + 1).tolist(),
                          d.type[d.start_at].tolist()):
        if max_spans is None or len(entities[r]) < max_spans:
            entities[r].append((s, e, t))
    return entities, dict(zip(STAT_KEYS, d.stats.tolist()))


def entity_counts(tags_a, tags_b, scheme, mask=None, num_types=None):
    """Host counterpart of ops.bio_entity_counts: (counts int64 [T, 3], stats int64 [6]) for two integer [B, S] arrays
    decoded under one mask.  counts[t] = (entities of type t in both with the same row, start and end; entities of a;
    entities of b); stats = kept tokens, rejected values of both arrays, then inside_tag_after_other_tag and
    inside_tag_with_different_entity_type of a, then of b."""
    scheme, T = check_scheme(scheme, num_types)
    a, keep = _rows(tags_a, mask)
    b, keep_b = _rows(tags_b, mask)
    if a.shape != b.shape:
        raise ValueError(f"the two tag arrays differ in shape: {a.shape} and {b.shape}")
    da, db = _Decoded(a, keep, scheme), _Decoded(b, keep_b, scheme)
    # both sides index the same list of kept tokens, so an entity is the pair of its first and last token there
    _, ia, ib = np.intersect1d(da.start_at, db.start_at, assume_unique=True, return_indices=True)
    ta = da.type[da.start_at]
    same = (da.end_at[ia] == db.end_at[ib]) & (ta[ia] == db.type[db.start_at][ib])
    counts = np.stack([np.bincount(ta[ia][same], minlength=T), np.bincount(ta, minlength=T),
                       np.bincount(db.type[db.start_at], minlength=T)], axis=1).astype(np.int64)
    stats = np.array([da.stats[0], da.stats[1] + db.stats[1], da.stats[2], da.stats[3], db.stats[2], db.stats[3]], np.int64)
    return counts, stats
