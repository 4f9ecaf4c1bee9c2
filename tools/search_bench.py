"""Corpus search (polus_amd/ir/search.py) at a ColBERT retrieval shape: 64 queries of Lq 32 tokens, E 128, bf16,
k = 100, over --docs documents generated from a seed: token documents of Ld 180 with ragged masks (about 4.6 GB of
representations at 100 000 documents) through ops.maxsim_scores, and the same number of [CLS] vectors through ops.gemm;
both merged by ops.topk_merge.  HIP events around each call after a warm-up; medians of --calls calls.  Prints one
JSON line per path:
  - search_ms: one CorpusIndex.search call (query side included: here the identity)
  - score_us / merge_us: the scoring launch and the merge launch of the first chunk alone (chunk_docs documents)
  - score_tflops: 2 Q n Lq Ld E (dot: 2 Q n E) over score_us; merge_gbs: 4 Q n bytes over merge_us
  - merge_over_score: merge_us / score_us (the MaxSim path must stay <= 0.10)
  - torch_topk_us / merge_us_alt: torch.topk on the same chunk's scores and ops.topk_merge, timed alternately in this
    process; topk_values_equal: both return the same values

    python tools/search_bench.py [--docs 100000] [--calls 20] [--warmup 5]
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from polus_amd import ops  # noqa: E402
from polus_amd.ir.models import TokenReps  # noqa: E402
from polus_amd.ir.search import CorpusIndex  # noqa: E402
from polus_amd.ir.training import InBatchDotScores, MaxSimScores  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--docs", type=int, default=100000)
ap.add_argument("--calls", type=int, default=20)
ap.add_argument("--warmup", type=int, default=5)
args = ap.parse_args()
Q, Lq, Ld, E, K = 64, 32, 180, 128, 100
DT = torch.bfloat16


class GivenReps:
    """A dual encoder whose encoders and projections are the identity: the batch is the representation."""

    def encode_query(self, x, training=False):
        return x

    encode_document = query_projection = document_projection = encode_query


def timed(fn):
    for _ in range(args.warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(args.calls):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1) * 1e3)
    ts.sort()
    return ts[len(ts) // 2]


def alternate(fa, fb, rounds=5):
    a, b = [], []
    for _ in range(rounds):
        a.append(timed(fa))
        b.append(timed(fb))
    a.sort(); b.sort()
    return a[len(a) // 2], b[len(b) // 2]


def run(name, index, queries, flop_per_pair):
    out = {"path": name, "Q": Q, "docs": len(index), "k": K, "E": E, "calls": args.calls}
    spans = index.chunks(Q)
    out["chunks"] = len(spans)
    out["search_ms"] = timed(lambda: index.search(queries, K)) / 1e3
    a, b = spans[0]
    n = b - a
    out["chunk_docs"] = n
    q = index.encode_queries(queries)
    s = torch.empty((Q, n), dtype=torch.float32, device="cuda")
    if index.tokens:
        score = lambda: ops.maxsim_scores(q.values, index.representations[a:b], q.mask, index.mask[a:b], s)
    else:
        score = lambda: ops.gemm(q, index.representations[a:b], s)
    tv = torch.empty((Q, K), dtype=torch.float32, device="cuda")
    ti = torch.empty((Q, K), dtype=torch.int32, device="cuda")
    merge = lambda: ops.topk_merge(s, tv, ti, id0=a, init=True)
    out["score_us"], out["merge_us"] = timed(score), timed(merge)
    out["score_tflops"] = flop_per_pair * Q * n / (out["score_us"] * 1e-6) / 1e12
    out["merge_gbs"] = 4.0 * Q * n / (out["merge_us"] * 1e-6) / 1e9
    out["merge_over_score"] = out["merge_us"] / out["score_us"]
    ref = [None]

    def topk():
        ref[0] = torch.topk(s, K, dim=1)
    out["merge_us_alt"], out["torch_topk_us"] = alternate(merge, topk)
    torch.cuda.synchronize()
    out["topk_values_equal"] = bool(torch.equal(ref[0].values, tv))
    print(json.dumps({k: (round(v, 4) if isinstance(v, float) else v) for k, v in out.items()}), flush=True)


g = torch.Generator(device="cuda").manual_seed(11)
STEP = 10000                                          # documents per add, as a loader would feed them

index = CorpusIndex(GivenReps(), MaxSimScores(normalize=False))
for a in range(0, args.docs, STEP):
    n = min(STEP, args.docs - a)
    d = torch.randn(n, Ld, E, device="cuda", generator=g).to(DT)
    dm = (torch.arange(Ld, device="cuda")[None] < torch.randint(Ld // 2, Ld + 1, (n, 1), device="cuda", generator=g)).to(torch.int32)
    index.add(TokenReps(d, dm))
queries = TokenReps(torch.randn(Q, Lq, E, device="cuda", generator=g).to(DT), torch.ones(Q, Lq, dtype=torch.int32, device="cuda"))
run("maxsim", index, queries, 2.0 * Lq * Ld * E)
index.clear()
del index
torch.cuda.empty_cache()

index = CorpusIndex(GivenReps(), InBatchDotScores())
for a in range(0, args.docs, STEP):
    index.add(torch.randn(min(STEP, args.docs - a), E, device="cuda", generator=g).to(DT))
run("dot", index, torch.randn(Q, E, device="cuda", generator=g).to(DT), 2.0 * E)
