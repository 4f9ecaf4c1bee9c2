"""float64 / NumPy reference of the centroid kernels (test infrastructure; the product never imports it):
polus_centroid_scores, polus_centroid_codes, polus_centroid_update and the spherical k-means they make up."""
import numpy as np

NONE = 0xFFFF


def centroid_scores(table, qmask, codes, B, Lq):
    """table [K, >= B*Lq], qmask [B, Lq] or None, codes uint16 [N, Ld] -> (score [B, N] float64, abs [B, N] float64 =
    the sum of |term| over the query tokens, what the f32 summation error scales with)."""
    table = np.asarray(table, np.float64)
    codes = np.asarray(codes).astype(np.int64) & 0xFFFF
    K = table.shape[0]
    idx = np.where(codes < K, codes, K)
    score, mag = np.zeros((B, codes.shape[0])), np.zeros((B, codes.shape[0]))
    for b in range(B):
        t = np.concatenate([table[:, b * Lq:(b + 1) * Lq], np.full((1, Lq), -np.inf)], 0)
        m = t[idx].max(axis=1)                                         # [N, Lq]
        m = np.where(np.isneginf(m), 0.0, m)
        if qmask is not None:
            m = m * (np.asarray(qmask)[b] != 0)
        score[b], mag[b] = m.sum(axis=1), np.abs(m).sum(axis=1)
    return score, mag


def centroid_scores_loop(table, qmask, codes, B, Lq):
    """The definition, one pair at a time."""
    K, (N, Ld) = len(table), np.shape(codes)
    out = np.zeros((B, N))
    for b in range(B):
        for n in range(N):
            for i in range(Lq):
                if qmask is not None and not qmask[b][i]:
                    continue
                best = None
                for j in range(Ld):
                    c = int(codes[n][j]) & 0xFFFF
                    if c < K:
                        v = float(table[c][b * Lq + i])
                        best = v if best is None or v > best else best
                out[b, n] += 0.0 if best is None else best
    return out


def centroid_codes(sim, mask=None):
    """sim [rows, K] -> uint16 [rows]: the first column of the maximum, NaN never winning (a row of NaN: 0), 0xFFFF
    where mask == 0."""
    s = np.asarray(sim, np.float64)
    out = np.argmax(np.where(np.isnan(s), -np.inf, s), axis=1).astype(np.uint16)
    if mask is not None:
        out[np.asarray(mask) == 0] = NONE
    return out


def centroid_update(x, codes, prev, eps=1e-12):
    """x [T, E], codes uint16 [T], prev [K, E] -> (out [K, E] float64, counts int32 [K], sums [K, E], abs sums [K, E])."""
    x, prev = np.asarray(x, np.float64), np.asarray(prev, np.float64)
    codes = np.asarray(codes).astype(np.int64) & 0xFFFF
    K = prev.shape[0]
    out, counts = prev.copy(), np.zeros(K, np.int32)
    sums, mags = np.zeros_like(prev), np.zeros_like(prev)
    for k in range(K):
        rows = x[codes == k]
        counts[k] = len(rows)
        sums[k], mags[k] = rows.sum(0), np.abs(rows).sum(0)
        nrm = np.sqrt((sums[k] ** 2).sum())
        if counts[k] > 0 and nrm > eps:
            out[k] = sums[k] / nrm
    return out, counts, sums, mags


def spherical_kmeans(x, K, iters):
    """The algorithm of CorpusIndex.fit_centroids on unit rows x [T, E] in float64: the first K rows, then `iters`
    rounds of (nearest by dot product, normalised sum; an empty centroid stays)."""
    x = np.asarray(x, np.float64)
    c = x[:K].copy()
    for _ in range(iters):
        c = centroid_update(x, centroid_codes(x @ c.T), c)[0]
    return c


def mean_best_similarity(x, c):
    return float((np.asarray(x, np.float64) @ np.asarray(c, np.float64).T).max(axis=1).mean())
