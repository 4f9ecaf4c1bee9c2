"""NumPy restatement of the pair-packing rule of include/polus_hip.h (pairs.hip), written row by row with Python lists
so that it shares nothing with the kernel's ballot / popcount arithmetic."""
import numpy as np


def kept_tokens(ids, mask, head, tail):
    """The valid tokens of one row (mask non-zero, in order; None: all), minus the first `head` and the last `tail`."""
    ids = [int(t) for t in ids]
    valid = ids if mask is None else [t for t, m in zip(ids, mask) if int(m) != 0]
    end = len(valid) - tail
    return valid[head:end] if end > head else []


def pair_row(q, d, max_q, S, special):
    """(input_ids, token_type_ids, attention_mask, length) of one pair from the stripped query tokens `q` and document
    tokens `d` (None: the empty document of a missing candidate)."""
    cls, sep, pad = special
    assert S >= max_q + 3
    q = q[:max_q]
    d = [] if d is None else d[:S - 3 - len(q)]
    row = [cls] + q + [sep] + d + [sep]
    types = [0] * (len(q) + 2) + [1] * (len(d) + 1)
    n = len(row)
    assert 3 <= n <= S
    fill = S - n
    return row + [pad] * fill, types + [0] * fill, [1] * n + [0] * fill, n


def pair_pack(q_ids, qmask, d_ids, dmask, cand, strips, max_q, S, special, rows=None):
    """input_ids, token_type_ids, attention_mask int32 [R, S] and length int32 [R] for the pairs `rows` (None: all the
    B n pairs in order) of cand int [B, n]; strips = (q_head, q_tail, d_head, d_tail)."""
    q_ids, d_ids, cand = np.asarray(q_ids), np.asarray(d_ids), np.asarray(cand)
    B, n = cand.shape
    N = d_ids.shape[0]
    qh, qt, dh, dt = strips
    rows = list(range(B * n)) if rows is None else [int(p) for p in rows]
    ids, types, att, length = [], [], [], []
    for p in rows:
        assert 0 <= p < B * n
        b, j = divmod(p, n)
        c = int(cand[b, j])
        q = kept_tokens(q_ids[b], None if qmask is None else qmask[b], qh, qt)
        d = kept_tokens(d_ids[c], None if dmask is None else dmask[c], dh, dt) if 0 <= c < N else None
        r = pair_row(q, d, max_q, S, special)
        ids.append(r[0]); types.append(r[1]); att.append(r[2]); length.append(r[3])
    i32 = lambda a, shape: np.asarray(a, np.int32).reshape(shape)
    R = len(rows)
    return i32(ids, (R, S)), i32(types, (R, S)), i32(att, (R, S)), i32(length, (R,))


def pair_lengths(qmask, q_shape, dmask, d_shape, cand, strips, max_q, S, rows=None):
    """length int32 [R] alone, from the masks (None: all ones over q_shape = (B, Lq) / d_shape = (N, Ld))."""
    zq, zd = np.zeros(q_shape, np.int32), np.zeros(d_shape, np.int32)
    return pair_pack(zq, qmask, zd, dmask, cand, strips, max_q, S, (0, 0, 0), rows)[3]


def scatter_scores(s, cand, N, out, rows=None):
    """out[b, j] = s[r] for pair rows[r] = b n + j when cand[b, j] lies in [0, N), -inf when not; the rest of `out`
    is left alone.  Returns the new array."""
    cand = np.asarray(cand)
    B, n = cand.shape
    out = np.array(out, dtype=np.float32, copy=True)
    rows = list(range(B * n)) if rows is None else [int(p) for p in rows]
    assert len(set(rows)) == len(rows), "scatter needs distinct rows"
    for r, p in enumerate(rows):
        b, j = divmod(p, n)
        out[b, j] = np.float32(s[r]) if 0 <= int(cand[b, j]) < N else np.float32(-np.inf)
    return out
