"""The lexical path at a passage-collection shape: 40 000 documents x 180 tokens, V = 30522, ids drawn with probability
proportional to rank^-1 (so that a few terms occur in almost every document and the df atomics see the contention a
real collection gives them).  HIP events around each call after a warm-up; variants that are compared run interleaved,
round by round, in this one process; medians.  Prints one JSON line and writes it as the first line of --out
(profiles/bm25.txt; whatever stands below the first line of an existing file, the commentary, is kept):
  - term_counts[M]: ops.bm25_term_counts at M = 180 and 128 with and without df (the difference is what the df atomics
    cost), tokens/s, the compulsory bytes (ids and mask read, terms and tf written) and bound_us = those bytes at
    6.3 TB/s (the achievable HBM rate); df_adds = the int32 atomics of one call, df_max = the most on one address;
    torch_us: torch.sort + torch.unique_consecutive over (row, id) keys of the same inputs, for orientation (it
    produces the counts, not the per-document ordered slots)
  - refresh: BM25Index.refresh() over that corpus, wall time around a synchronise (it contains the one device-to-host
    copy), and the weights kernel alone against its bytes
  - query: ops.bm25_query for 64 queries against its bytes
  - search: BM25Index.search (k = 100) for 64 queries of 4..16 tokens beside SparseCorpusIndex.search over a synthetic
    index of the same N with terms = 128
  - mine: ops.mine_negatives at Q = 64 and 4096, C = 1000, k = 7 and 63, against cand + score read once and the
    outputs written
These are records, not thresholds.

    python tools/bm25_bench.py [--rounds 15] [--warmup 3] [--out profiles/bm25.txt]
"""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from polus_amd import ops  # noqa: E402
from polus_amd.ir.lexical import BM25Index  # noqa: E402
from polus_amd.ir.search import SparseCorpusIndex  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=15)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--docs", type=int, default=40000)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bm25.txt"))
args = ap.parse_args()
N, L, V, Q = args.docs, 180, 30522, 64
HBM = 6.3e12
g = torch.Generator(device="cuda").manual_seed(11)


def interleaved(fns):
    """{name: median us}: every variant once per round, `rounds` rounds after `warmup` rounds."""
    for _ in range(args.warmup):
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    ts = {name: [] for name in fns}
    for _ in range(args.rounds):
        for name, fn in fns.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            ts[name].append(e0.elapsed_time(e1) * 1e3)
    return {name: sorted(v)[len(v) // 2] for name, v in ts.items()}


def record(us, nbytes):
    bound = nbytes / HBM * 1e6
    return {"us": round(us, 2), "bytes": int(nbytes), "bound_us": round(bound, 2), "fraction_of_bound": round(bound / us, 4)}


def zipf(shape, s=1.0):
    """ids with probability proportional to rank^-s; which id has which rank is a seeded permutation."""
    p = torch.arange(1, V + 1, device="cuda", dtype=torch.float64) ** -s
    n = 1
    for d in shape:
        n *= d
    ranks = torch.cat([torch.multinomial(p, min(1 << 23, n - a), replacement=True, generator=g) for a in range(0, n, 1 << 23)])
    return torch.randperm(V, device="cuda", generator=g)[ranks].to(torch.int32).reshape(shape).contiguous()


out = {"shape": {"N": N, "L": L, "V": V, "Q": Q}, "rounds": args.rounds, "hbm_tb_s": HBM / 1e12, "term_counts": {}, "mine": {}}
ids = zipf((N, L))
lens = torch.randint(L // 2, L + 1, (N, 1), device="cuda", generator=g)
mask = (torch.arange(L, device="cuda")[None] < lens).to(torch.int32).contiguous()
tokens = int(mask.sum()) - 2 * N                                    # the strip takes two per document
doc_len = torch.empty(N, dtype=torch.int32, device="cuda")
df = torch.zeros(V, dtype=torch.int32, device="cuda")
stats = torch.zeros(3, dtype=torch.int64, device="cuda")


def torch_counts():
    keys = torch.where(mask != 0, torch.arange(N, device="cuda")[:, None] * V + ids.long(), N * V).reshape(-1)
    return torch.unique_consecutive(torch.sort(keys).values, return_counts=True)


for M in (180, 128):
    terms = torch.empty((N, M), dtype=torch.int32, device="cuda")
    tf = torch.empty((N, M), dtype=torch.int32, device="cuda")
    df.zero_()
    ops.bm25_term_counts(ids, mask, terms, tf, doc_len, V, (1, 1), df=df, stats=stats)
    adds, hottest = int(df.sum()), int(df.max())
    t = interleaved({"with_df": lambda: ops.bm25_term_counts(ids, mask, terms, tf, doc_len, V, (1, 1), df=df, stats=stats),
                     "without_df": lambda: ops.bm25_term_counts(ids, mask, terms, tf, doc_len, V, (1, 1)),
                     "torch": torch_counts})
    rec = record(t["with_df"], 2 * N * L * 4 + 2 * N * M * 4 + N * 4)
    rec.update(us_without_df=round(t["without_df"], 2), torch_us=round(t["torch"], 2), tokens=tokens,
               tokens_per_s=round(tokens / (t["with_df"] * 1e-6)), df_adds=adds, df_max=hottest)
    out["term_counts"][str(M)] = rec
    del terms, tf

# the index: adds in batches, then refresh / query / search
index = BM25Index(V, terms=L)
for a in range(0, N, 8192):
    index.add({"input_ids": ids[a:a + 8192], "attention_mask": mask[a:a + 8192]})
walls = []
for _ in range(args.warmup + args.rounds):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    index.refresh()
    torch.cuda.synchronize()
    walls.append((time.perf_counter() - t0) * 1e6)
walls = sorted(walls[args.warmup:])
w_us = interleaved({"w": lambda: ops.bm25_weights(index.counts, index.doc_lengths, index._w[:N], 0.54, 0.003, 1.9)})["w"]
out["refresh"] = {"wall_us": round(walls[len(walls) // 2], 1), "d2h_bytes": 4 * V + 24,
                  "weights": record(w_us, 2 * N * L * 4 + N * 4)}
index.refresh()

qlen = torch.randint(4, 17, (Q, 1), device="cuda", generator=g) + 2  # [CLS] + 4..16 tokens + [SEP]
q_ids = zipf((Q, 18), s=0.7)
q_mask = (torch.arange(18, device="cuda")[None] < qlen).to(torch.int32).contiguous()
queries = {"input_ids": q_ids, "attention_mask": q_mask}
qt = torch.empty((Q, 18), dtype=torch.int32, device="cuda")
qf = torch.empty((Q, 18), dtype=torch.int32, device="cuda")
ql = torch.empty((Q,), dtype=torch.int32, device="cuda")
ops.bm25_term_counts(q_ids, q_mask, qt, qf, ql, V, (1, 1))
qrow = torch.empty((Q, V), dtype=torch.float32, device="cuda")
out["query"] = record(interleaved({"q": lambda: ops.bm25_query(qt, qf, index.idf, qrow)})["q"], Q * V * 4 + 2 * Q * 18 * 4)


class _Given:
    """Hands the sparse index ready-made representations."""

    def encode_query(self, x, training=False):
        return x

    encode_document = query_projection = document_projection = encode_query


sparse = SparseCorpusIndex(_Given(), terms=128)
for a in range(0, N, 2048):
    n = min(2048, N - a)
    d = torch.zeros(n, V, device="cuda")
    d.scatter_(1, torch.randint(0, V, (n, 256), device="cuda", generator=g), torch.rand(n, 256, device="cuda", generator=g) + 0.01)
    sparse.add(d)
dense_q = index.encode_queries(queries)
score = torch.empty(Q, N, device="cuda")
t = interleaved({"bm25_search": lambda: index.search(queries, 100), "sparse_search": lambda: sparse.search(dense_q, 100),
                 "bm25_scores": lambda: ops.sparse_scores(dense_q, index.term_ids, index.weights, score),
                 "sparse_scores": lambda: ops.sparse_scores(dense_q, sparse.term_ids, sparse.weights, score)})
out["search"] = {"k": 100, "bm25_search_us": round(t["bm25_search"], 2), "sparse128_search_us": round(t["sparse_search"], 2),
                 "bm25_scores": record(t["bm25_scores"], N * L * 8 + Q * N * 4 + Q * V * 4),
                 "sparse128_scores": record(t["sparse_scores"], N * 128 * 8 + Q * N * 4 + Q * V * 4)}
del sparse, score, index

C = 1000
for Qm in (64, 4096):
    start = torch.randint(0, N, (Qm, 1), device="cuda", generator=g)
    cand = ((start + torch.arange(C, device="cuda")[None] * 7) % N).to(torch.int32).contiguous()       # distinct per row
    sc = torch.sort(torch.rand(Qm, C, device="cuda", generator=g) * 20, dim=1, descending=True).values.contiguous()
    excl = cand[:, [3, 40]].contiguous()
    n_pool = torch.empty(Qm, dtype=torch.int32, device="cuda")
    for k in (7, 63):
        neg = torch.empty((Qm, k), dtype=torch.int32, device="cuda")
        col = torch.empty((Qm, k), dtype=torch.int32, device="cuda")
        us = interleaved({"m": lambda: ops.mine_negatives(cand, neg, n_pool, score=sc, exclude=excl, min_score=0.0, seed=1, neg_col=col)})["m"]
        out["mine"][f"Q{Qm}_k{k}"] = record(us, Qm * C * 8 + Qm * 8 + 2 * Qm * k * 4 + Qm * 4)

line = json.dumps(out)
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
notes = open(args.out).read().split("\n", 1)[1:] if os.path.exists(args.out) else []     # the commentary under the line stays
with open(args.out, "w") as f:
    f.write(line + "\n" + "".join(notes))
print(line, flush=True)
