"""Two-stage search (polus_amd/ir/search.py rerank, TwoStageSearch) at a ColBERT retrieval shape: 64 queries of Lq 32
tokens, E 128, bf16, k = 100, over --docs token documents of Ld 180 with ragged masks generated from a seed (the
corpus of tools/search_bench.py), C = --cands candidates per query drawn without replacement, and as many [CLS]
vectors as a first stage.  HIP events around each call after a warm-up; medians of --calls calls.  Prints one JSON line:
  - rerank_us / merge_us: the polus_maxsim_rerank launch and the polus_topk_merge_ids launch over all C columns
  - doc_bytes: document bytes the rerank launch fetches: per candidate the 16-token tiles up to its last valid token
    (tiles behind it are skipped), each row once; rerank_tbs: doc_bytes over rerank_us
  - rerank_ms: one CorpusIndex.rerank call; search_ms: one exhaustive CorpusIndex.search call on the same index
  - first_ms: the [CLS] index's search for C candidates; two_stage_ms: one TwoStageSearch.search call
  - rerank_equals_search_scores: the rerank scores of the exhaustive search's own top k have the search's bits

    python tools/rerank_bench.py [--docs 100000] [--cands 1000] [--calls 20] [--warmup 5]
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from polus_amd import ops  # noqa: E402
from polus_amd.ir.models import TokenReps  # noqa: E402
from polus_amd.ir.search import CorpusIndex, TwoStageSearch  # noqa: E402
from polus_amd.ir.training import InBatchDotScores, MaxSimScores  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--docs", type=int, default=100000)
ap.add_argument("--cands", type=int, default=1000)
ap.add_argument("--calls", type=int, default=20)
ap.add_argument("--warmup", type=int, default=5)
args = ap.parse_args()
Q, Lq, Ld, E, K = 64, 32, 180, 128, 100
C = args.cands
DT = torch.bfloat16


class GivenReps:
    """A dual encoder whose encoders and projections are the identity: the batch is the representation."""

    def encode_query(self, x, training=False):
        return x

    encode_document = query_projection = document_projection = encode_query


class Pair:
    """Queries of a two-stage search over GivenReps: each stage's index takes its own representation of them."""

    def __init__(self, cls, tokens):
        self.cls, self.tokens = cls, tokens


class PairReps(GivenReps):
    def __init__(self, tokens):
        self.tokens = tokens

    def encode_query(self, x, training=False):
        return (x.tokens if self.tokens else x.cls) if isinstance(x, Pair) else x


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


g = torch.Generator(device="cuda").manual_seed(11)
STEP = 10000                                          # documents per add, as a loader would feed them
second = CorpusIndex(PairReps(True), MaxSimScores(normalize=False))
first = CorpusIndex(PairReps(False), InBatchDotScores())
for a in range(0, args.docs, STEP):
    n = min(STEP, args.docs - a)
    d = torch.randn(n, Ld, E, device="cuda", generator=g).to(DT)
    dm = (torch.arange(Ld, device="cuda")[None] < torch.randint(Ld // 2, Ld + 1, (n, 1), device="cuda", generator=g)).to(torch.int32)
    second.add(TokenReps(d, dm))
    first.add(d[:, 0].contiguous())                   # a stand-in first stage: the first token's vector
    del d
qt = TokenReps(torch.randn(Q, Lq, E, device="cuda", generator=g).to(DT), torch.ones(Q, Lq, dtype=torch.int32, device="cuda"))
queries = Pair(qt.values[:, 0].contiguous(), qt)
N = len(second)
# C candidates per query without replacement: the first C of a random order of the corpus
cand = torch.stack([torch.randperm(N, device="cuda", generator=g)[:C] for _ in range(Q)]).to(torch.int32)

out = {"Q": Q, "docs": N, "cands": C, "k": K, "Lq": Lq, "Ld": Ld, "E": E, "calls": args.calls}
s = torch.empty((Q, C), dtype=torch.float32, device="cuda")
tv = torch.empty((Q, K), dtype=torch.float32, device="cuda")
ti = torch.empty((Q, K), dtype=torch.int32, device="cuda")
out["rerank_us"] = timed(lambda: ops.maxsim_rerank(qt.values, second.representations, qt.mask, second.mask, cand, s))
out["merge_us"] = timed(lambda: ops.topk_merge(s, tv, ti, init=True, ids=cand))
mask = second.mask
last = (mask * torch.arange(1, Ld + 1, device="cuda", dtype=torch.int32)[None]).amax(1)     # tokens up to the last valid one
rows = torch.clamp((last + 15) // 16 * 16, max=Ld).to(torch.int64)
out["doc_bytes"] = int(rows[cand.long()].sum().item()) * E * 2
out["doc_bytes_unskipped"] = Q * C * Ld * E * 2
out["rerank_tbs"] = out["doc_bytes"] / (out["rerank_us"] * 1e-6) / 1e12
out["rerank_ms"] = timed(lambda: second.rerank(queries, cand, K)) / 1e3
out["search_ms"] = timed(lambda: second.search(queries, K)) / 1e3
out["first_ms"] = timed(lambda: first.search(queries, C)) / 1e3
two = TwoStageSearch(first, second, C)
out["two_stage_ms"] = timed(lambda: two.search(queries, K)) / 1e3
out["search_over_two_stage"] = out["search_ms"] / out["two_stage_ms"]
sv, si = second.search(queries, K)
rv, ri = second.rerank(queries, si, K)
torch.cuda.synchronize()
out["rerank_equals_search_scores"] = bool(torch.equal(sv.view(torch.int32), rv.view(torch.int32)) and torch.equal(si, ri))
print(json.dumps({k: (round(v, 4) if isinstance(v, float) else v) for k, v in out.items()}), flush=True)
