"""The refine stage on tools/pq_bench.py's corpus: N = 1 000 000 vectors of E = 768 in bf16 drawn around 4096 random centres
(SYNTHETIC: centre + 0.7 N(0, 1) noise; queries drawn the same way, same seed and order as pq_bench), k = 100.  HIP events
around each call after a warm-up; the variants of a comparison run interleaved, round by round, in this one process; medians.
Prints one JSON line and writes it as the first line of --out (profiles/refine.txt; the commentary below the first line of an
existing file is kept):
  - kernel[shape][route]: ops.cls_rerank ("full") / ops.cls_rerank_fp8 ("fp8") alone over B x 1000 random distinct ids, and
    the torch foil on the same inputs (`torch_us`: the rows gathered by index_select, then torch.bmm in bf16 and a cast of
    the result to f32; it has no FP8 form, so the fp8 row has no foil).  `bytes` is what the algorithm needs (B C rows of E
    elements, the ids, the scores, the queries once), `gbytes_per_s` = bytes / time, `hbm_bound_us` = bytes over the 6.29 TB/s
    a copy kernel reaches on this part (8.0 TB/s spec)
  - search[index][Q]: `bare_us` and `bare_overlap` of the index WITHOUT refine (the route that exists without this stage),
    `plain_us` of the plain index's exact search in the same rounds, and per refine store and R `us` and `overlap`: the mean
    share of the plain index's k ids the search returns (synthetic data: no statement about a real collection).  Indexes:
    PQ at m = 96 and 24, IVF-PQ at K = 4096, m = 96, nprobe = 16
  - bytes_per_document[index][refine]: nbytes / N once the lists are built
These are records, not thresholds.

    python tools/refine_bench.py [--rounds 15] [--warmup 3] [--docs 1000000] [--out profiles/refine.txt]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from polus_amd import ops  # noqa: E402
from polus_amd.ir.search import CorpusIndex  # noqa: E402
from polus_amd.ir.training import InBatchDotScores  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=15)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--docs", type=int, default=1000000)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "refine.txt"))
args = ap.parse_args()
N, E, K_TOP, KSUB, CENTRES, BATCH = args.docs, 768, 100, 256, 4096, 65536
QS, RS, LISTS, NPROBE, C_KERNEL = (1, 8, 64), (200, 400, 1000), 4096, 16, 1000
HBM_COPY_BYTES_PER_S = 6.29e12
g = torch.Generator(device="cuda").manual_seed(23)


class Given:
    """A dual encoder whose inputs are the vectors themselves."""

    def encode_query(self, x, training=False):
        return x

    encode_document = query_projection = document_projection = encode_query


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


def draw(n):
    centres_of = torch.randint(0, CENTRES, (n,), device="cuda", generator=g)
    return (centres[centres_of] + 0.7 * torch.randn((n, E), device="cuda", generator=g)).to(torch.bfloat16)


def overlap(got, want):
    return round(float(np.mean([len(set(a.tolist()) & set(b.tolist())) / K_TOP for a, b in zip(got.cpu(), want.cpu())])), 3)


def filled(**kw):
    index = CorpusIndex(Given(), InBatchDotScores(), **kw)
    reps = plain.representations
    for a in range(0, N, BATCH):
        index.add(reps[a:a + BATCH])
    return index


centres = torch.randn((CENTRES, E), device="cuda", generator=g)
plain = CorpusIndex(Given(), InBatchDotScores())
for a in range(0, N, BATCH):
    plain.add(draw(min(BATCH, N - a)))
queries = {Q: draw(Q) for Q in QS}

out = {"shape": {"N": N, "E": E, "k": K_TOP, "ksub": KSUB, "dtype": "bf16", "corpus": f"synthetic: {CENTRES} centres + 0.7 noise"},
       "rounds": args.rounds, "hbm_copy_bytes_per_s": HBM_COPY_BYTES_PER_S, "kernel": {}, "search": {}, "bytes_per_document": {}}

# ---------------------------------------------------------------- (a) the kernel alone
docs = plain.representations
codes = torch.empty((N, E), dtype=torch.uint8, device="cuda")
scale = torch.empty((N,), dtype=torch.float32, device="cuda")
ops.cls_fp8_quantize(docs, codes, scale)
for B in (64, 1):
    q = queries[64][:B].contiguous()
    cand = torch.stack([torch.randperm(N, device="cuda", generator=g)[:C_KERNEL] for _ in range(B)]).to(torch.int32)
    flat_ids = cand.long().view(-1)
    score = torch.empty((B, C_KERNEL), dtype=torch.float32, device="cuda")

    def foil():
        rows = docs.index_select(0, flat_ids).view(B, C_KERNEL, E)       # the gather, materialised
        return torch.bmm(rows, q.unsqueeze(2)).squeeze(2).float()

    t = interleaved({"full": lambda: ops.cls_rerank(q, docs, cand, score),
                     "fp8": lambda: ops.cls_rerank_fp8(q, codes, scale, cand, score), "torch": foil})
    ops.cls_rerank(q, docs, cand, score)
    worst = float((score - foil()).abs().max() / score.abs().max())      # the foil rounds its sums to bf16
    rec = {}
    for route, row_bytes in (("full", 2 * E), ("fp8", E + 4)):
        nbytes = B * C_KERNEL * (row_bytes + 4 + 4) + B * E * 2
        rec[route] = {"us": round(t[route], 1), "bytes": nbytes, "gbytes_per_s": round(nbytes / t[route] * 1e-3, 1),
                      "hbm_bound_us": round(nbytes / HBM_COPY_BYTES_PER_S * 1e6, 2)}
    rec["full"]["torch_us"] = round(t["torch"], 1)
    rec["full"]["torch_over_hip"] = round(t["torch"] / t["full"], 2)
    rec["full"]["foil_max_rel_diff"] = round(worst, 5)
    out["kernel"][f"{B}x{C_KERNEL}"] = rec
    print(f"[refine_bench] kernel {B} x {C_KERNEL}: {rec}", file=sys.stderr, flush=True)
del codes, scale

# ---------------------------------------------------------------- (b) search through the refine stage, (c) bytes per document
out["bytes_per_document"]["plain"] = {"none": round(plain.nbytes / N, 2)}
exact = {Q: plain.search(queries[Q], K_TOP)[1] for Q in QS}


def configurations():
    for m in (96, 24):
        yield f"pq_m{m}", dict(storage="pq", codec=plain.fit_pq(m, KSUB))
    yield f"ivfpq_K{LISTS}_m96_nprobe{NPROBE}", dict(storage="ivfpq", codec=plain.fit_ivfpq(LISTS, 96, KSUB), nprobe=NPROBE)


for name, kw in configurations():
    bare = filled(**kw)
    stores = {r: filled(refine=r, **kw) for r in ("full", "fp8")}
    for ix in (bare, *stores.values()):
        if ix.storage == "ivfpq":
            ix.refresh_lists()
    out["bytes_per_document"][name] = {"none": round(bare.nbytes / N, 2), **{r: round(ix.nbytes / N, 2) for r, ix in stores.items()}}
    out["search"][name] = {}
    for Q in QS:
        q = queries[Q]
        fns = {"plain": lambda: plain.search(q, K_TOP), "bare": lambda: bare.search(q, K_TOP)}
        for r, ix in stores.items():
            for R in RS:
                fns[f"{r}{R}"] = lambda ix=ix, R=R: ix.search(q, K_TOP, candidates=R)
        t = interleaved(fns)
        row = {"plain_us": round(t["plain"], 1), "bare_us": round(t["bare"], 1), "bare_overlap": overlap(bare.search(q, K_TOP)[1], exact[Q])}
        for r, ix in stores.items():
            row[r] = {str(R): {"us": round(t[f"{r}{R}"], 1), "over_bare": round(t[f"{r}{R}"] / t["bare"], 2),
                               "plain_over_this": round(t["plain"] / t[f"{r}{R}"], 2),
                               "overlap": overlap(ix.search(q, K_TOP, candidates=R)[1], exact[Q])} for R in RS}
        out["search"][name][str(Q)] = row
        print(f"[refine_bench] {name} Q {Q}: {row}", file=sys.stderr, flush=True)
    del bare, stores

line = json.dumps(out)
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
notes = open(args.out).read().split("\n", 1)[1:] if os.path.exists(args.out) else []     # the commentary under the line stays
with open(args.out, "w") as f:
    f.write(line + "\n" + "".join(notes))
print(line, flush=True)
