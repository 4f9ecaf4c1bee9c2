"""Centroid-pruned search (polus_amd/ir/search.py fit_centroids, search_pruned) at a ColBERT retrieval shape: 64 queries
of Lq 32 tokens, E 128, bf16, over --docs token documents of Ld 180 with ragged masks generated from a seed (the corpus
of tools/search_bench.py, here under MaxSimScores(normalize=True): centroids need unit vectors).  HIP events around each
call after a warm-up; every timing is [median, p10, p90] of its calls.  Prints one JSON line:
  - fit_s: one fit_centroids(K) call, wall clock (sample, k-means rounds and the assignment of every stored token)
  - index_bytes / index_bytes_with_codes: CorpusIndex.nbytes before and after
  - route / lds_bytes, table_gemm_us, scan_us: at K = --k (LDS route) the <centroid, query token> GEMM and the
    ops.centroid_scores launch over the first chunk (chunk_docs documents); scan_lookups_per_ns: Q n Ld Lq table entries
    over scan_us (masked tails are skipped, so the launch reads fewer)
  - global_scan_us: the same launch at K = 4096 (global route), after fit_centroids(4096, iters=1)
  - pruned_ms / search_ms: search_pruned(k = 100, candidates = --cands) and the exhaustive search on the same index,
    called alternately; search_over_pruned: the ratio of the medians; pruned_p90_below_search_p10: the acceptance
  - overlap_at_100: the share of the exhaustive top 100 that the pruned top 100 holds, mean over the queries.
    Informational only: the synthetic corpus is unclustered noise, so this says nothing about recall on real text.

    python tools/centroid_bench.py [--docs 100000] [--k 1024] [--cands 1000] [--calls 10] [--warmup 3] [--rounds 3]
"""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from polus_amd import ops  # noqa: E402
from polus_amd.ir.models import TokenReps  # noqa: E402
from polus_amd.ir.search import CorpusIndex  # noqa: E402
from polus_amd.ir.training import MaxSimScores  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--docs", type=int, default=100000)
ap.add_argument("--k", type=int, default=1024)
ap.add_argument("--cands", type=int, default=1000)
ap.add_argument("--calls", type=int, default=10)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--rounds", type=int, default=3)
args = ap.parse_args()
Q, Lq, Ld, E, TOP = 64, 32, 180, 128, 100
DT = torch.bfloat16


class GivenReps:
    """A dual encoder whose encoders and projections are the identity: the batch is the representation."""

    def encode_query(self, x, training=False):
        return x

    encode_document = query_projection = document_projection = encode_query


def samples(fn, calls, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(calls):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1) * 1e3)
    return ts


def stats(ts, scale=1.0):
    ts = sorted(ts)
    pick = lambda p: round(ts[min(len(ts) - 1, int(p * len(ts)))] / scale, 3)
    return [pick(0.5), pick(0.1), pick(0.9)]


def timed(fn):
    return stats(samples(fn, args.calls, args.warmup))


def scan(index, out, prefix):
    K = index.centroids.shape[0]
    a, b = index.chunks(Q)[0]
    q = index.encode_queries(queries)
    table = torch.empty((K, Q * Lq), dtype=torch.float32, device="cuda")
    s = torch.empty((Q, b - a), dtype=torch.float32, device="cuda")
    gemm = lambda: ops.gemm(index.centroids, q.values.view(Q * Lq, E), table)
    out[prefix + "table_gemm_us"] = timed(gemm)
    out[prefix + "scan_us"] = timed(lambda: ops.centroid_scores(table, q.mask, index.centroid_codes[a:b], s, Q, Lq))
    out[prefix + "scan_lookups_per_ns"] = round(Q * (b - a) * Ld * Lq / (out[prefix + "scan_us"][0] * 1e3), 2)
    return b - a


g = torch.Generator(device="cuda").manual_seed(11)
STEP = 10000                                          # documents per add, as a loader would feed them
index = CorpusIndex(GivenReps(), MaxSimScores(normalize=True))
for a in range(0, args.docs, STEP):
    n = min(STEP, args.docs - a)
    d = torch.randn(n, Ld, E, device="cuda", generator=g).to(DT)
    dm = (torch.arange(Ld, device="cuda")[None] < torch.randint(Ld // 2, Ld + 1, (n, 1), device="cuda", generator=g)).to(torch.int32)
    index.add(TokenReps(d, dm))
    del d
queries = TokenReps(torch.randn(Q, Lq, E, device="cuda", generator=g).to(DT), torch.ones(Q, Lq, dtype=torch.int32, device="cuda"))

out = {"Q": Q, "docs": len(index), "Lq": Lq, "Ld": Ld, "E": E, "K": args.k, "cands": args.cands, "k": TOP, "calls": args.calls,
       "index_bytes": index.nbytes}
torch.cuda.synchronize()
t0 = time.perf_counter()
index.fit_centroids(args.k)
torch.cuda.synchronize()
out["fit_s"] = round(time.perf_counter() - t0, 3)
out["index_bytes_with_codes"] = index.nbytes
route = ops.centroid_scores_route(Q, min(len(index), 65535), Lq, Ld, args.k)
out["route"], out["lds_bytes"] = route.route, route.lds_bytes
out["chunk_docs"] = scan(index, out, "")

pruned, full = [], []
for _ in range(args.rounds):
    pruned += samples(lambda: index.search_pruned(queries, TOP, args.cands), args.calls, args.warmup)
    full += samples(lambda: index.search(queries, TOP), args.calls, args.warmup)
out["pruned_ms"], out["search_ms"] = stats(pruned, 1e3), stats(full, 1e3)
out["search_over_pruned"] = round(out["search_ms"][0] / out["pruned_ms"][0], 2)
out["pruned_p90_below_search_p10"] = out["pruned_ms"][2] < out["search_ms"][1]
pi, fi = index.search_pruned(queries, TOP, args.cands)[1].cpu().numpy(), index.search(queries, TOP)[1].cpu().numpy()
out["overlap_at_100"] = round(float(sum(len(set(a.tolist()) & set(b.tolist())) for a, b in zip(pi, fi))) / fi.size, 4)
out["overlap_note"] = "unclustered synthetic corpus: says nothing about recall on real text"

t0 = time.perf_counter()
index.fit_centroids(4096, iters=1)
torch.cuda.synchronize()
out["global_fit_s"] = round(time.perf_counter() - t0, 3)
out["global_route"] = ops.centroid_scores_route(Q, min(len(index), 65535), Lq, Ld, 4096).route
scan(index, out, "global_")
out["global_pruned_ms"] = stats(samples(lambda: index.search_pruned(queries, TOP, args.cands), args.calls, args.warmup), 1e3)
print(json.dumps(out), flush=True)
