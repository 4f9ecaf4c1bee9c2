"""Rank fusion at hybrid-retrieval shapes: Q = 64 queries, L ranked lists of C entries each drawn from a corpus of 40 000
documents (ids distinct within a list row, scores descending), fused and ranked to k = 100.  HIP events around each
call after a warm-up; the variants of a comparison run interleaved, round by round, in this one process; medians.
Prints one JSON line and writes it as the first line of --out (profiles/fusion.txt; whatever stands below the first line
of an existing file, the commentary, is kept):
  - fuse[L x C][method]: `hip_us` = ops.fuse_lists + ops.topk_merge (two launches) beside `torch_us` = the torch
    composition cat -> sort -> unique_consecutive -> scatter_add -> topk on the same inputs (rrf: the reciprocal ranks
    are computed inside the timed call, as the kernel computes them; sum: the scores are added as they are; the float
    sums of scatter_add have no defined order), `fuse_us` the fusion launch alone, and `same_ids`: the fraction of
    the k result ids on which the two agree (the torch sums may differ in the last bits, and with them the order of
    near-ties)
  - many_queries: ops.fuse_lists alone at Q = 4096, L = 2, C = 1000 (a mining run: more queries than the grid has
    workgroups), with the bytes it reads and writes (ids and scores in, ids and values out)
  - hybrid: HybridSearch.search (k = 100, depth = 1000, rrf) over two BM25Index of tools/bm25_bench.py's corpus
    (40 000 documents x 180 tokens, k1 / b = 0.9 / 0.4 and 1.6 / 0.75), split into the two stage searches and the fusion
    (fuse + topk over their results)
These are records, not thresholds.

    python tools/fusion_bench.py [--rounds 15] [--warmup 3] [--out profiles/fusion.txt]
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from polus_amd import ops  # noqa: E402
from polus_amd.ir.fusion import HybridSearch, fuse  # noqa: E402
from polus_amd.ir.lexical import BM25Index  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=15)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--docs", type=int, default=40000)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fusion.txt"))
args = ap.parse_args()
N, Q, K, RRF_K = args.docs, 64, 100, 60.0
g = torch.Generator(device="cuda").manual_seed(17)


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


def torch_fusion(ids, scores, method):
    """The composition a user writes today: (values [Q, K], ids [Q, K]).  Every id is in [0, N)."""
    L, Q_, C = ids.shape
    if method == "rrf":
        contrib = (1.0 / (RRF_K + torch.arange(1, C + 1, device=ids.device, dtype=torch.float32))).expand(L, Q_, C)
    else:
        contrib = scores
    flat_id = torch.cat(list(ids.long()), dim=1)                         # cat: [Q, L C]
    flat_v = torch.cat(list(contrib), dim=1)
    key = flat_id + torch.arange(Q_, device=ids.device)[:, None] * N     # one sort for all rows
    order = torch.sort(key.reshape(-1)).indices
    uniq, inverse = torch.unique_consecutive(key.reshape(-1)[order], return_inverse=True)
    fused = torch.zeros(uniq.numel(), dtype=torch.float32, device=ids.device).scatter_add_(0, inverse, flat_v.reshape(-1)[order])
    row = uniq // N
    dense = torch.full((Q_, L * C), -float("inf"), device=ids.device)
    start = torch.searchsorted(row, torch.arange(Q_, device=ids.device))
    col = torch.arange(uniq.numel(), device=ids.device) - start[row]
    dense[row, col] = fused
    dense_id = torch.full((Q_, L * C), -1, dtype=torch.long, device=ids.device)
    dense_id[row, col] = uniq % N
    top = torch.topk(dense, K, dim=1)
    return top.values, torch.gather(dense_id, 1, top.indices)


out = {"shape": {"N": N, "Q": Q, "k": K, "rrf_k": RRF_K}, "rounds": args.rounds, "fuse": {}}
for L, C in ((2, 1000), (3, 1000), (4, 1024)):
    ids = torch.stack([torch.stack([torch.randperm(N, device="cuda", generator=g)[:C] for _ in range(Q)]) for _ in range(L)])
    ids = ids.to(torch.int32).contiguous()
    scores = torch.sort(torch.rand((L, Q, C), device="cuda", generator=g) * 20, dim=2, descending=True).values.contiguous()
    out_id = torch.empty((Q, L * C), dtype=torch.int32, device="cuda")
    out_val = torch.empty((Q, L * C), dtype=torch.float32, device="cuda")
    count = torch.empty((Q,), dtype=torch.int32, device="cuda")
    top_val = torch.empty((Q, K), dtype=torch.float32, device="cuda")
    top_id = torch.empty((Q, K), dtype=torch.int32, device="cuda")
    rec = {}
    for method in ("rrf", "sum"):
        def hip_fuse():
            ops.fuse_lists(ids, scores, out_id, out_val, count, N, method, rrf_k=RRF_K)

        def hip():
            hip_fuse()
            ops.topk_merge(out_val, top_val, top_id, init=True, ids=out_id)

        t = interleaved({"hip": hip, "torch": lambda: torch_fusion(ids, scores, method), "fuse": hip_fuse})
        hip()
        want = torch_fusion(ids, scores, method)[1]
        same = float((top_id.long() == want).float().mean())
        rec[method] = {"hip_us": round(t["hip"], 2), "torch_us": round(t["torch"], 2), "fuse_us": round(t["fuse"], 2),
                       "torch_over_hip": round(t["torch"] / t["hip"], 2), "same_ids": round(same, 4),
                       "union_mean": round(float(count.float().mean()), 1)}
    out["fuse"][f"{L}x{C}"] = rec

# many queries per call (a mining run): the fusion launch alone, more workgroups than the grid holds
Qm, L, C = 4096, 2, 1000
start = torch.randint(0, N, (L, Qm, 1), device="cuda", generator=g)
ids = ((start + torch.arange(C, device="cuda")[None, None] * 7) % N).to(torch.int32).contiguous()        # distinct per row
scores = torch.sort(torch.rand((L, Qm, C), device="cuda", generator=g) * 20, dim=2, descending=True).values.contiguous()
out_id = torch.empty((Qm, L * C), dtype=torch.int32, device="cuda")
out_val = torch.empty((Qm, L * C), dtype=torch.float32, device="cuda")
count = torch.empty((Qm,), dtype=torch.int32, device="cuda")
t = interleaved({"fuse": lambda: ops.fuse_lists(ids, scores, out_id, out_val, count, N, "rrf", rrf_k=RRF_K)})
out["many_queries"] = {"Q": Qm, "L": L, "C": C, "fuse_us": round(t["fuse"], 2), "us_per_query": round(t["fuse"] / Qm, 4),
                       "bytes": Qm * L * C * 16, "union_mean": round(float(count.float().mean()), 1)}
del ids, scores, out_id, out_val, count

# HybridSearch over two BM25 indexes of tools/bm25_bench.py's corpus
Ld, V = 180, 30522
p = torch.arange(1, V + 1, device="cuda", dtype=torch.float64) ** -1.0


def zipf(shape, probs):
    n = shape[0] * shape[1]
    ranks = torch.cat([torch.multinomial(probs, min(1 << 23, n - a), replacement=True, generator=g) for a in range(0, n, 1 << 23)])
    return torch.randperm(V, device="cuda", generator=g)[ranks].to(torch.int32).reshape(shape).contiguous()


d_ids = zipf((N, Ld), p)
lens = torch.randint(Ld // 2, Ld + 1, (N, 1), device="cuda", generator=g)
d_mask = (torch.arange(Ld, device="cuda")[None] < lens).to(torch.int32).contiguous()
stages = [BM25Index(V, terms=Ld, k1=0.9, b=0.4), BM25Index(V, terms=Ld, k1=1.6, b=0.75)]
hybrid = HybridSearch(stages, depth=1000)
for a in range(0, N, 8192):
    hybrid.add({"input_ids": d_ids[a:a + 8192], "attention_mask": d_mask[a:a + 8192]})
qlen = torch.randint(4, 17, (Q, 1), device="cuda", generator=g) + 2
queries = {"input_ids": zipf((Q, 18), torch.arange(1, V + 1, device="cuda", dtype=torch.float64) ** -0.7),
           "attention_mask": (torch.arange(18, device="cuda")[None] < qlen).to(torch.int32).contiguous()}
results = [s.search(queries, 1000) for s in stages]
top_val = torch.empty((Q, K), dtype=torch.float32, device="cuda")
top_id = torch.empty((Q, K), dtype=torch.int32, device="cuda")


def fusion_only():
    fid, fval, _ = fuse(results, N, "rrf")
    ops.topk_merge(fval, top_val, top_id, init=True, ids=fid)


t = interleaved({"hybrid": lambda: hybrid.search(queries, K), "stage0": lambda: stages[0].search(queries, 1000),
                 "stage1": lambda: stages[1].search(queries, 1000), "fusion": fusion_only})
out["hybrid"] = {"docs": N, "tokens": Ld, "depth": 1000, "k": K, "search_us": round(t["hybrid"], 2),
                 "stage_search_us": [round(t["stage0"], 2), round(t["stage1"], 2)], "fusion_us": round(t["fusion"], 2),
                 "fusion_share": round(t["fusion"] / t["hybrid"], 4)}

line = json.dumps(out)
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
notes = open(args.out).read().split("\n", 1)[1:] if os.path.exists(args.out) else []     # the commentary under the line stays
with open(args.out, "w") as f:
    f.write(line + "\n" + "".join(notes))
print(line, flush=True)
