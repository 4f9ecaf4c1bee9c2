"""NumPy restatement of the BM25 and mining rules of include/polus_hip.h (polus_bm25_term_counts, polus_bm25_weights,
polus_bm25_query, polus_mine_negatives) and of BM25Index.refresh, written from the rules and not from the kernels, plus
the textbook BM25 score in float64.  Host only."""
import numpy as np


def hash32(seed, idx):
    """polus_hash32 of polus_amd/csrc/common.h: the murmur3 finaliser of idx * 0x9E3779B1 + seed in uint32 arithmetic
    (tests/util.py restates the same hash for the dropout mask).  Scalars or arrays."""
    U, M = np.uint64, np.uint64(0xFFFFFFFF)
    x = ((np.asarray(idx, np.uint64) & M) * U(0x9E3779B1) + U(int(seed) & 0xFFFFFFFF)) & M
    x ^= x >> U(16); x = (x * U(0x85EBCA6B)) & M
    x ^= x >> U(13); x = (x * U(0xC2B2AE35)) & M
    x ^= x >> U(16)
    return x


def remaining_tokens(row, mask_row, V, head, tail):
    """(the tokens of one row that are counted, how many were rejected): valid = non-zero mask, in order; at most head +
    tail valid tokens leave nothing, otherwise the first head and last tail go; ids outside [0, V) are rejected."""
    valid = [int(t) for t, m in zip(row, mask_row if mask_row is not None else np.ones(len(row), np.int32)) if m != 0]
    if len(valid) <= head + tail:
        return [], 0
    rest = valid[head:len(valid) - tail]
    kept = [t for t in rest if 0 <= t < V]
    return kept, len(rest) - len(kept)


def term_counts(ids, mask, V, M, head, tail, df=None, stats=None):
    """(terms int32 [n, M], tf int32 [n, M], doc_len int32 [n], df int32 [V], stats int64 [3]); df and stats continue
    from the arrays given (accumulation) or from zero.  stats = (truncated documents, rejected tokens, tokens)."""
    ids = np.asarray(ids)
    n = ids.shape[0]
    terms, tf = np.full((n, M), -1, np.int32), np.zeros((n, M), np.int32)
    doc_len = np.zeros(n, np.int32)
    df = np.zeros(V, np.int32) if df is None else np.array(df, np.int32)
    stats = np.zeros(3, np.int64) if stats is None else np.array(stats, np.int64)
    for r in range(n):
        kept, rejected = remaining_tokens(ids[r], None if mask is None else mask[r], V, head, tail)
        doc_len[r] = len(kept)
        stats[1] += rejected
        stats[2] += len(kept)
        distinct = sorted(set(kept))
        count = {t: 0 for t in distinct}
        for t in kept:
            count[t] += 1
        order = sorted(distinct, key=lambda t: (-count[t], t))
        for s, t in enumerate(order[:M]):
            terms[r, s], tf[r, s] = t, count[t]
        stats[0] += len(order) > M
        for t in distinct:
            df[t] += 1
    return terms, tf, doc_len, df, stats


def constants(k1, b, n_docs, n_tokens):
    """(c0, c1, k1p1) as np.float32, each computed in float64 and rounded once; avgdl = 1 for a corpus without tokens."""
    avgdl = n_tokens / n_docs if n_tokens > 0 else 1.0
    return np.float32(k1 * (1.0 - b)), np.float32(k1 * b / avgdl), np.float32(k1 + 1.0)


def idf(df, n_docs):
    """f32 [V]: Lucene's non-negative idf, float64 then one rounding."""
    df = np.asarray(df, np.float64)
    return np.log1p((n_docs - df + 0.5) / (df + 0.5)).astype(np.float32)


def weights(tf, doc_len, c0, c1, k1p1):
    """f32 [n, M]: every operation one float32 rounding (NumPy float32 arithmetic); +0.0 where tf == 0."""
    c0, c1, k1p1 = np.float32(c0), np.float32(c1), np.float32(k1p1)
    x = np.asarray(tf).astype(np.float32)
    K = (c1 * np.asarray(doc_len).astype(np.float32) + c0).astype(np.float32)[:, None]
    with np.errstate(divide="ignore", invalid="ignore"):
        w = ((x * k1p1).astype(np.float32) / (x + K).astype(np.float32)).astype(np.float32)
    return np.where(np.asarray(tf) > 0, w, np.float32(0.0)).astype(np.float32)


def query(terms, tf, idf_f32, V):
    """f32 [B, V]: fl(f32(tf) * idf) at the used slots, +0.0 elsewhere."""
    B, M = terms.shape
    q = np.zeros((B, V), np.float32)
    for b in range(B):
        for m in range(M):
            t = int(terms[b, m])
            if 0 <= t < V:
                q[b, t] = np.float32(tf[b, m]) * np.float32(idf_f32[t])
    return q


def pool(cand_row, score_row, exclude_row, skip_top, min_score):
    """The pool columns of one row, in column order."""
    banned = set(int(e) for e in (exclude_row if exclude_row is not None else []) if e >= 0)
    out = []
    for c in range(skip_top, len(cand_row)):
        if cand_row[c] < 0 or int(cand_row[c]) in banned:
            continue
        if score_row is not None and not (score_row[c] > min_score):        # a NaN fails
            continue
        out.append(c)
    return out


def mine_negatives(cand, score, exclude, skip_top, min_score, k, seed):
    """(neg int32 [Q, k], neg_col int32 [Q, k], n_pool int32 [Q])."""
    Q = cand.shape[0]
    neg, col = np.full((Q, k), -1, np.int32), np.full((Q, k), -1, np.int32)
    n_pool = np.zeros(Q, np.int32)
    for r in range(Q):
        cols = pool(cand[r], None if score is None else score[r], None if exclude is None else exclude[r], skip_top,
                    np.float32(min_score))
        R = n_pool[r] = len(cols)
        if R <= k:
            picks = list(range(R))
        else:
            picks = []
            for j in range(k):
                lo, hi = j * R // k, (j + 1) * R // k                       # Python integers: no overflow
                picks.append(lo + int(hash32(seed, (r * k + j) & 0xFFFFFFFF)) % (hi - lo))
        for j, p in enumerate(picks):
            neg[r, j], col[r, j] = cand[r, cols[p]], cols[p]
    return neg, col, n_pool


def bm25_float64(doc_ids, doc_mask, q_ids, q_mask, V, head, tail, k1, b):
    """The textbook BM25 score in float64 with untruncated counts, [Q, N]:
    sum over the query's distinct terms t of tf_q(t) idf(t) tf_d(t) (k1 + 1) / (tf_d(t) + k1 (1 - b + b len_d / avgdl))."""
    N, Q = len(doc_ids), len(q_ids)
    bags, lens, df = [], np.zeros(N), np.zeros(V)
    for r in range(N):
        kept, _ = remaining_tokens(doc_ids[r], None if doc_mask is None else doc_mask[r], V, head, tail)
        bag = {}
        for t in kept:
            bag[t] = bag.get(t, 0) + 1
        bags.append(bag)
        lens[r] = len(kept)
        for t in bag:
            df[t] += 1
    avgdl = lens.sum() / N if lens.sum() > 0 else 1.0
    idf64 = np.log1p((N - df + 0.5) / (df + 0.5))
    out = np.zeros((Q, N))
    for i in range(Q):
        kept, _ = remaining_tokens(q_ids[i], None if q_mask is None else q_mask[i], V, head, tail)
        qbag = {}
        for t in kept:
            qbag[t] = qbag.get(t, 0) + 1
        for r in range(N):
            K = k1 * (1.0 - b + b * lens[r] / avgdl)
            s = 0.0
            for t, qt in qbag.items():
                f = bags[r].get(t, 0)
                if f:
                    s += qt * idf64[t] * f * (k1 + 1.0) / (f + K)
            out[i, r] = s
    return out


def rank(scores, k):
    """(values, ids) [Q, k]: score descending, ties to the lower id; (-inf, -1) behind the corpus."""
    Q, N = scores.shape
    val, idx = np.full((Q, k), -np.inf), np.full((Q, k), -1, np.int64)
    for i in range(Q):
        order = np.lexsort((np.arange(N), -scores[i]))[:k]
        val[i, :len(order)], idx[i, :len(order)] = scores[i, order], order
    return val, idx
