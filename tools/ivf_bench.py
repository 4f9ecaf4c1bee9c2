"""Probed candidate generation (polus_amd/ir/search.py refresh_lists, probe, search_pruned(nprobe=...)) against the
scan of the same index: 64 queries of Lq 32 tokens, E 128, bf16, over --docs token documents of Ld 180 with ragged
masks, under MaxSimScores(normalize=True).

The corpus is PLANTED, so that centroids have something to find (tools/centroid_bench.py's unclustered noise would make
every list a random sample of the corpus): --directions unit directions; a document draws --topic of them and each of
its tokens is one of those plus noise * N(0, I) / sqrt(E); a query's tokens are drawn the same way from the directions of
one document.  All from a seed.  The structure is by construction: the overlaps below say how the probed search behaves
on it, nothing about recall on real text.

For K in --ks (fit_centroids) and nprobe in --nprobes, same process, HIP events around each call after a warm-up, the
probed search and the scan called alternately, every timing [median, p10, p90].  One JSON line per (K, nprobe):
  - refresh_ms / pairs: one refresh_lists() call and P, the (centroid, document) pairs; fit_s: fit_centroids(K), wall clock
  - cand_mean / cand_median / cand_max: candidates per query; cand_fraction: cand_mean / docs
  - probe_us (ops.gemm + ops.topk_merge), mark_us (ops.ivf_mark), compact_us (ops.ivf_compact twice: count, then ids),
    score_us (ops.centroid_scores_ids + ops.topk_merge over the candidates), rerank_us (the exact MaxSim of the best
    --cands): the stages of one probed search, each timed alone
  - probed_ms / scan_ms: search_pruned(k = 100, candidates = --cands) with and without nprobe; scan_over_probed: the
    ratio of the medians (> 1: probing is faster)
  - overlap_scan_at_100 / overlap_exhaustive_at_100: the share of the scan's (search_pruned without nprobe) and of the
    exhaustive search's top 100 that the probed top 100 holds, mean over the queries
Not measured: probed search beyond this corpus size; recall on a real collection.

    python tools/ivf_bench.py [--docs 40000] [--ks 1024,16384] [--nprobes 1,2,4,8] [--cands 1000] [--out profiles/ivf.txt]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from polus_amd import ops  # noqa: E402
from polus_amd.ir.models import TokenReps  # noqa: E402
from polus_amd.ir.search import CorpusIndex  # noqa: E402
from polus_amd.ir.training import MaxSimScores  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--docs", type=int, default=40000)
ap.add_argument("--ks", default="1024,16384")
ap.add_argument("--nprobes", default="1,2,4,8")
ap.add_argument("--cands", type=int, default=1000)
ap.add_argument("--directions", type=int, default=8192)
ap.add_argument("--topic", type=int, default=24)
ap.add_argument("--noise", type=float, default=0.35)
ap.add_argument("--calls", type=int, default=10)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--rounds", type=int, default=2)
ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "ivf.txt"))
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


g = torch.Generator(device="cuda").manual_seed(11)
dirs = torch.randn(args.directions, E, device="cuda", generator=g)
dirs /= dirs.norm(dim=1, keepdim=True)


def planted(topics, L):
    """topics int64 [n, topic] -> [n, L, E]: each token one of its row's directions plus noise."""
    n = topics.shape[0]
    pick = torch.randint(0, topics.shape[1], (n, L), device="cuda", generator=g)
    x = dirs[torch.gather(topics, 1, pick)] + args.noise * torch.randn(n, L, E, device="cuda", generator=g) / E ** 0.5
    return x.to(DT)


STEP = 10000                                          # documents per add, as a loader would feed them
index = CorpusIndex(GivenReps(), MaxSimScores(normalize=True))
doc_topics = torch.randint(0, args.directions, (args.docs, args.topic), device="cuda", generator=g)
for a in range(0, args.docs, STEP):
    n = min(STEP, args.docs - a)
    dm = (torch.arange(Ld, device="cuda")[None] < torch.randint(Ld // 2, Ld + 1, (n, 1), device="cuda", generator=g)).to(torch.int32)
    index.add(TokenReps(planted(doc_topics[a:a + n], Ld), dm))
source = torch.randint(0, args.docs, (Q,), device="cuda", generator=g)
queries = TokenReps(planted(doc_topics[source], Lq), torch.ones(Q, Lq, dtype=torch.int32, device="cuda"))
N = len(index)


def overlap(a, b):
    return round(float(sum(len(set(x.tolist()) & set(y.tolist())) for x, y in zip(a, b))) / b.size, 4)


lines = [f"# python tools/ivf_bench.py   (one MI355X; {N} planted documents of Ld {Ld} ragged, {args.directions} directions, "
         f"{args.topic} per document, noise {args.noise}; {Q} queries x {Lq} tokens, E {E}, bf16; k {TOP}, candidates {args.cands}; "
         "timings [median, p10, p90])",
         "# not measured: probed search beyond this corpus size; recall on a real collection (the centroid structure here is planted)"]
exhaustive = index.search(queries, TOP)[1].cpu().numpy()
for K in [int(x) for x in args.ks.split(",")]:
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    index.fit_centroids(K)
    torch.cuda.synchronize()
    fit_s = round(time.perf_counter() - t0, 3)
    refresh = samples(index.refresh_lists, 5, 1)
    offsets, docs = index.lists
    scan_ids = index.search_pruned(queries, TOP, args.cands)[1].cpu().numpy()
    q = index.encode_queries(queries)
    flat = q.values.view(Q * Lq, E)
    table = torch.empty((K, Q * Lq), dtype=torch.float32, device="cuda")
    ops.gemm(index.centroids, flat, table)
    for nprobe in [int(x) for x in args.nprobes.split(",")]:
        out = {"K": K, "nprobe": nprobe, "Q": Q, "docs": N, "cands": args.cands, "fit_s": fit_s,
               "refresh_ms": stats(refresh, 1e3), "pairs": int(offsets[-1]), "index_bytes": index.nbytes}
        probes, cand, count = index.probe(queries, nprobe)
        cn = count.cpu().numpy()
        out.update(cand_mean=round(float(cn.mean()), 1), cand_median=float(np.median(cn)), cand_max=int(cn.max()),
                   cand_fraction=round(float(cn.mean()) / N, 4))
        # the stages, each alone, on the buffers of one search
        sim = torch.empty((Q * Lq, K), dtype=torch.float32, device="cuda")
        pv = torch.empty((Q * Lq, nprobe), dtype=torch.float32, device="cuda")
        pi = torch.empty((Q * Lq, nprobe), dtype=torch.int32, device="cuda")
        bitmap = torch.empty((Q, (N + 31) // 32), dtype=torch.int32, device="cuda")
        cnt = torch.empty((Q,), dtype=torch.int32, device="cuda")
        C = cand.shape[1]
        score = torch.empty((Q, min(C, 65535)), dtype=torch.float32, device="cuda")
        cv = torch.empty((Q, args.cands), dtype=torch.float32, device="cuda")
        ci = torch.empty((Q, args.cands), dtype=torch.int32, device="cuda")

        def probe_stage():
            ops.gemm(flat, index.centroids, sim)
            ops.topk_merge(sim, pv, pi, init=True)

        def compact_stage():
            ops.ivf_compact(bitmap, N, cnt)
            ops.ivf_compact(bitmap, N, cnt, cand)

        def score_stage():
            for s in range(0, C, 65535):
                e = min(s + 65535, C)
                ops.centroid_scores_ids(table, q.mask, index.centroid_codes, cand[:, s:e], score[:, :e - s], Q, Lq)
                ops.topk_merge(score[:, :e - s], cv, ci, init=(s == 0), ids=cand[:, s:e])
        out["probe_us"] = timed(probe_stage)
        out["mark_us"] = timed(lambda: ops.ivf_mark(pi, q.mask, offsets, docs, N, bitmap, Q, Lq))
        out["compact_us"] = timed(compact_stage)
        out["score_us"] = timed(score_stage)
        out["rerank_us"] = timed(lambda: index._rerank_encoded(q, ci, TOP))
        probed, scan = [], []
        for _ in range(args.rounds):
            probed += samples(lambda: index.search_pruned(queries, TOP, args.cands, nprobe=nprobe), args.calls, args.warmup)
            scan += samples(lambda: index.search_pruned(queries, TOP, args.cands), args.calls, args.warmup)
        out["probed_ms"], out["scan_ms"] = stats(probed, 1e3), stats(scan, 1e3)
        out["scan_over_probed"] = round(out["scan_ms"][0] / out["probed_ms"][0], 2)
        got = index.search_pruned(queries, TOP, args.cands, nprobe=nprobe)[1].cpu().numpy()
        out["overlap_scan_at_100"], out["overlap_exhaustive_at_100"] = overlap(got, scan_ids), overlap(got, exhaustive)
        lines.append(json.dumps(out))
        print(lines[-1], flush=True)
    out = {"K": K, "nprobe": None, "overlap_exhaustive_at_100": overlap(scan_ids, exhaustive)}
    lines.append(json.dumps(out))
    print(lines[-1], flush=True)
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    f.write("\n".join(lines) + "\n")
