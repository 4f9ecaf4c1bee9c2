"""NumPy reference of the block-inverted postings and the term-at-a-time score rule (include/polus_hip.h, the block of
polus_postings_*), for tests/test_postings_cpu.py and tests/test_postings_gpu.py.  NumPy only."""
import numpy as np


def bits(a):
    return np.ascontiguousarray(np.asarray(a, np.float32)).view(np.int32)


def is_posting(t, w, V):
    """0 <= id < V and w != 0: NaN counts, +0.0 and -0.0 do not."""
    return 0 <= int(t) < V and bool(np.float32(w) != 0)


def build(ids, w, V, block_docs):
    """(counts int32 [nblk, V], offsets int32 [nblk, V + 1], base int64 [nblk + 1], lists): lists[(b, t)] is the sorted
    list of (local document id, weight bits) of the postings of term t in block b; empty lists are absent."""
    ids, w = np.asarray(ids), np.asarray(w, np.float32)
    N, M = ids.shape
    nblk = (N + block_docs - 1) // block_docs
    counts = np.zeros((nblk, V), np.int32)
    lists = {}
    for d in range(N):
        b = d // block_docs
        for m in range(M):
            if is_posting(ids[d, m], w[d, m], V):
                t = int(ids[d, m])
                counts[b, t] += 1
                lists.setdefault((b, t), []).append((d - b * block_docs, int(np.float32(w[d, m]).view(np.int32))))
    for key in lists:
        lists[key].sort()
    offsets = np.zeros((nblk, V + 1), np.int32)
    offsets[:, 1:] = np.cumsum(counts, axis=1, dtype=np.int64)
    base = np.zeros(nblk + 1, np.int64)
    base[1:] = np.cumsum(offsets[:, V].astype(np.int64))
    return counts, offsets, base, lists


def pack(offsets, base, lists, rng=None):
    """(post_doc uint16 [P], post_w f32 [P]) holding `lists` at their positions, each list in sorted order or, with a
    generator, shuffled."""
    P = int(base[-1])
    post_doc, post_bits = np.zeros(P, np.uint16), np.zeros(P, np.int32)
    for (b, t), entries in lists.items():
        order = np.arange(len(entries)) if rng is None else rng.permutation(len(entries))
        at = int(base[b]) + int(offsets[b, t])
        assert len(entries) == int(offsets[b, t + 1]) - int(offsets[b, t])
        for i, e in enumerate(order):
            post_doc[at + i], post_bits[at + i] = entries[e]
    return post_doc, post_bits.view(np.float32)


def unpack(offsets, base, post_doc, post_w, V):
    """The lists of device-built arrays in build()'s form, for a comparison as sorted sets."""
    lists = {}
    wb = bits(post_w)
    for b in range(offsets.shape[0]):
        for t in range(V):
            a, e = int(base[b]) + int(offsets[b, t]), int(base[b]) + int(offsets[b, t + 1])
            if e > a:
                lists[(b, t)] = sorted((int(post_doc[p]), int(wb[p])) for p in range(a, e))
    return lists


def compact_rows(q, cap):
    """(q_terms int32 [Q, cap], q_w f32 [Q, cap], q_count int32 [Q]): the entries with q != 0 (NaN kept, -0.0 dropped)
    in ascending column, the first cap of them, then (-1, 0.0); the count is the full number."""
    q = np.asarray(q, np.float32)
    Q = q.shape[0]
    terms, w, count = np.full((Q, cap), -1, np.int32), np.zeros((Q, cap), np.float32), np.zeros(Q, np.int32)
    for r in range(Q):
        keep = np.nonzero(q[r] != 0)[0]
        count[r] = len(keep)
        keep = keep[:cap]
        terms[r, :len(keep)], w[r, :len(keep)] = keep, q[r, keep]
    return terms, w, count


def bm25_query_lists(terms, tf, idf_f32, V):
    """The used slots of a counted query, ids outside [0, V) dropped, in ascending id with weight fl(f32(tf) * idf[t]);
    the output is as wide as the input."""
    Q, M = terms.shape
    q_terms, q_w, count = np.full((Q, M), -1, np.int32), np.zeros((Q, M), np.float32), np.zeros(Q, np.int32)
    for r in range(Q):
        kept = sorted((int(t), m) for m, t in enumerate(terms[r]) if 0 <= t < V)
        count[r] = len(kept)
        for j, (t, m) in enumerate(kept):
            q_terms[r, j] = t
            q_w[r, j] = np.float32(tf[r, m]) * np.float32(idf_f32[t])
    return q_terms, q_w, count


def term_lists(lists, block_docs):
    """{t: (global document ids, weights f32)} from build()'s lists."""
    out = {}
    for (b, t), entries in lists.items():
        docs = np.array([b * block_docs + d for d, _ in entries], np.int64)
        ws = np.array([x for _, x in entries], np.int32).view(np.float32)
        if t in out:
            out[t] = (np.concatenate([out[t][0], docs]), np.concatenate([out[t][1], ws]))
        else:
            out[t] = (docs, ws)
    return out


def scores(q_terms, q_w, q_count, lists, block_docs, N, V):
    """f32 [Q, N] by the score rule: acc = +0.0; the entries j < min(q_count, cap) in order, ids outside [0, V) skipped;
    acc = f32(acc + f32(q_w * w)) for the documents holding the term.  A Python loop over the entries, np.float32
    products and sums over a term's documents (which are distinct)."""
    by_term = term_lists(lists, block_docs)
    Q, cap = q_terms.shape
    out = np.zeros((Q, N), np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        for r in range(Q):
            for j in range(min(max(int(q_count[r]), 0), cap)):
                t = int(q_terms[r, j])
                if not 0 <= t < V or t not in by_term:
                    continue
                docs, ws = by_term[t]
                prod = (np.float32(q_w[r, j]) * ws).astype(np.float32)
                out[r, docs] = (out[r, docs] + prod).astype(np.float32)
    return out


def scores_float64(q_terms, q_w, q_count, ids, w, V):
    """An independent brute force: per document a dictionary term -> weight from the forward slots, float64 sums.
    Returns (scores [Q, N], sum of |products| [Q, N], entries that took part [Q])."""
    ids, w = np.asarray(ids), np.asarray(w, np.float32)
    N = ids.shape[0]
    docs = [{int(t): float(x) for t, x in zip(ids[d], w[d]) if is_posting(t, x, V)} for d in range(N)]
    Q, cap = q_terms.shape
    out, mass, used = np.zeros((Q, N)), np.zeros((Q, N)), np.zeros(Q, np.int64)
    for r in range(Q):
        entries = [(int(q_terms[r, j]), float(q_w[r, j])) for j in range(min(max(int(q_count[r]), 0), cap))]
        entries = [(t, x) for t, x in entries if 0 <= t < V]
        used[r] = len(entries)
        for d in range(N):
            for t, x in entries:
                if t in docs[d]:
                    out[r, d] += x * docs[d][t]
                    mass[r, d] += abs(x * docs[d][t])
    return out, mass, used


def rank(s, k):
    """(values f32 [Q, k], ids int32 [Q, k]): score descending, ties to the lower id, NaN dropped; (-inf, -1) behind."""
    Q, N = s.shape
    val, idx = np.full((Q, k), -np.inf, np.float32), np.full((Q, k), -1, np.int32)
    for r in range(Q):
        keep = np.nonzero(~np.isnan(s[r]) & (s[r] != -np.inf))[0]
        order = keep[np.lexsort((keep, -s[r, keep].astype(np.float64)))][:k]
        val[r, :len(order)], idx[r, :len(order)] = s[r, order], order
    return val, idx
