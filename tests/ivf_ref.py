"""NumPy restatement of the inverted lists and the probed candidate set (polus_amd/csrc/ivf.hip): plain loops and
sets, nothing shared with the kernels."""
import numpy as np


def lists(codes, K):
    """codes uint16 [N, Ld] -> (counts int64 [K], offsets int64 [K + 1], per centroid the sorted list of its documents).
    A code >= K is no token; a document enters a centroid's list once."""
    members = [set() for _ in range(K)]
    for n, row in enumerate(np.asarray(codes)):
        for c in row.tolist():
            if c < K:
                members[c].add(n)
    counts = np.array([len(m) for m in members], np.int64)
    offsets = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    return counts, offsets, [sorted(m) for m in members]


def split(offsets, docs):
    """The per-centroid lists, each sorted, of a CSR pair as the device leaves it."""
    offsets, docs = np.asarray(offsets).astype(np.int64), np.asarray(docs)
    return [sorted(docs[offsets[c]:offsets[c + 1]].tolist()) for c in range(len(offsets) - 1)]


def candidates(probes, qmask, per_centroid, N):
    """probes int [B, Lq, nprobe], qmask [B, Lq] or None, per_centroid: K lists of document ids -> per query the set of
    documents in the list of a probe in [0, K) of a token whose mask is non-zero; ids outside [0, N) never enter."""
    K = len(per_centroid)
    out = []
    for b in range(probes.shape[0]):
        s = set()
        for i in range(probes.shape[1]):
            if qmask is not None and qmask[b, i] == 0:
                continue
            for c in probes[b, i].tolist():
                if 0 <= c < K:
                    s.update(d for d in per_centroid[c] if 0 <= d < N)
        out.append(s)
    return out


def bitmap(sets, N):
    """uint32 [B, ceil(N / 32)]: bit d & 31 of word d >> 5 of row b set for d in sets[b]."""
    out = np.zeros((len(sets), (N + 31) // 32), np.uint32)
    for b, s in enumerate(sets):
        for d in s:
            out[b, d >> 5] |= np.uint32(1 << (d & 31))
    return out


def compact(bits, N, cap):
    """uint32 [B, >= ceil(N / 32)] -> (count int32 [B], cand int32 [B, cap]): the set positions below N ascending, the
    first cap of them, then -1; count is the full number."""
    B = bits.shape[0]
    count, cand = np.zeros(B, np.int32), np.full((B, cap), -1, np.int32)
    for b in range(B):
        ids = [d for d in range(N) if (int(bits[b, d >> 5]) >> (d & 31)) & 1]
        count[b] = len(ids)
        cand[b, :min(cap, len(ids))] = ids[:cap]
    return count, cand
