"""Residual-compressed token index (polus_amd/csrc/residual.hip) beside the bf16 and FP8 index kernels at a ColBERT
retrieval shape: 64 queries of Lq 32 tokens, E 128, bf16, C = 1000 distinct random candidates per query over --docs
documents of Ld 180 (a corpus far larger than L2), K = 1024 and 65535 centroids, codes uniform over the centroids (the
widest spread of centroid rows a corpus can ask for), random residual bits.

One process.  Per round, in turn on the same queries and candidates: polus_maxsim_rerank (bf16), polus_maxsim_rerank_fp8,
polus_maxsim_rerank_res at nbits 1 / 2 / 4 for each K, bf16 again; --warmup rounds, then --rounds timed; HIP events, us;
4 candidate sets taken in turn.  "full" = no document mask, "ragged" = document lengths uniform in [Ld / 2, Ld].
polus_residual_compress is timed the same way over the whole corpus, in tokens/s.  Before timing, each residual
format's rerank scores are compared bit for bit with polus_maxsim_rerank over the decoded corpus (K = 1024).

    python tools/residual_bench.py [--docs 40000] [--rounds 30] [--warmup 5] [--out profiles/residual.txt]
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from polus_amd import ops  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--docs", type=int, default=40000)
ap.add_argument("--rounds", type=int, default=30)
ap.add_argument("--warmup", type=int, default=5)
ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "residual.txt"))
args = ap.parse_args()
Q, Lq, Ld, E, C, SETS = 64, 32, 180, 128, 1000, 4
N, DT = args.docs, torch.bfloat16
KS, NBITS = (1024, 65535), (1, 2, 4)
assert torch.cuda.is_available(), "a measurement needs the GPU"
g = torch.Generator(device="cuda").manual_seed(23)


def unit(*shape):
    x = torch.randn(*shape, device="cuda", generator=g)
    return (x / x.norm(dim=-1, keepdim=True)).to(DT)


def stats(ts):
    ts = sorted(ts)
    n = len(ts)
    return {"median": round(ts[n // 2], 1), "min": round(ts[0], 1), "p10": round(ts[n // 10], 1), "p90": round(ts[(9 * n) // 10], 1),
            "max": round(ts[-1], 1)}


def run_rounds(variants, rounds, warmup):
    """variants: [(name, fn(round))]; every round runs each once, in order; returns {name: [us]}."""
    ts = {name: [] for name, _ in variants}
    for r in range(warmup + rounds):
        for name, fn in variants:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn(r)
            e1.record()
            e1.synchronize()
            if r >= warmup:
                ts[name].append(e0.elapsed_time(e1) * 1e3)
    return ts


q = unit(Q, Lq, E)
qm = torch.ones(Q, Lq, dtype=torch.int32, device="cuda")
cands = [torch.stack([torch.randperm(N, device="cuda", generator=g)[:C] for _ in range(Q)]).to(torch.int32) for _ in range(SETS)]
ragged = (torch.arange(Ld, device="cuda")[None] < torch.randint(Ld // 2, Ld + 1, (N, 1), device="cuda", generator=g)).to(torch.int32)
score = torch.empty((Q, C), dtype=torch.float32, device="cuda")

# the three corpora: bf16 vectors, their FP8 codes, and residual codes + bits per (K, nbits)
d = torch.empty((N, Ld, E), dtype=DT, device="cuda")
for a in range(0, N, 5000):
    d[a:a + 5000] = unit(min(5000, N - a), Ld, E)
f8 = torch.empty((N, Ld, E), dtype=torch.uint8, device="cuda")
f8s = torch.empty((N, Ld), dtype=torch.float32, device="cuda")
ops.fp8_quantize(d, f8, f8s)
cent = {K: unit(K, E) for K in KS}
codes = {K: torch.randint(0, K, (N, Ld), device="cuda", generator=g).to(torch.int32).to(torch.int16) for K in KS}   # the bits of the unsigned code
packed = {nb: torch.randint(0, 256, (N, Ld, E * nb // 8), device="cuda", generator=g, dtype=torch.int32).to(torch.uint8) for nb in NBITS}
weights = {nb: ((torch.arange(1 << nb, device="cuda", dtype=torch.float32) + 0.5) / (1 << nb) - 0.5) * 0.12 for nb in NBITS}
cutoffs = {nb: ((torch.arange(1, 1 << nb, device="cuda", dtype=torch.float32)) / (1 << nb) - 0.5) * 0.12 for nb in NBITS}

lines = []
equal = {}
dec = torch.empty((N, Ld, E), dtype=DT, device="cuda")
ref = torch.empty_like(score)
for nb in NBITS:
    ops.residual_decompress(codes[1024], packed[nb], cent[1024], weights[nb], nb, dec)
    ops.maxsim_rerank(q, dec, qm, ragged, cands[0], ref)
    ops.maxsim_rerank_res(q, codes[1024], packed[nb], cent[1024], weights[nb], nb, qm, ragged, cands[0], score)
    torch.cuda.synchronize()
    equal[nb] = bool(torch.equal(ref.view(torch.int32), score.view(torch.int32)))
del dec

result = {}
for name, dm in (("full", None), ("ragged", ragged)):
    variants = [("bf16", lambda r, dm=dm: ops.maxsim_rerank(q, d, qm, dm, cands[r % SETS], score)),
                ("fp8", lambda r, dm=dm: ops.maxsim_rerank_fp8(q, f8, f8s, qm, dm, cands[r % SETS], score))]
    for K in KS:
        for nb in NBITS:
            variants.append((f"res{nb}_K{K}", lambda r, dm=dm, K=K, nb=nb: ops.maxsim_rerank_res(
                q, codes[K], packed[nb], cent[K], weights[nb], nb, qm, dm, cands[r % SETS], score)))
    variants.append(("bf16_again", variants[0][1]))
    ts = run_rounds(variants, args.rounds, args.warmup)
    result[name] = {k: stats(v) for k, v in ts.items()}
    lines.append(f"rerank_{name} " + json.dumps(result[name]))

tokens = N * Ld
comp = {}
variants = []
for K in KS:
    for nb in NBITS:
        out = torch.empty_like(packed[nb])
        variants.append((f"compress{nb}_K{K}", lambda r, K=K, nb=nb, out=out: ops.residual_compress(d, codes[K], cent[K], cutoffs[nb], nb, out)))
ts = run_rounds(variants, max(5, args.rounds // 3), 2)
for k, v in ts.items():
    s = stats(v)
    comp[k] = {"median_us": s["median"], "min_us": s["min"], "max_us": s["max"], "tokens_per_s": round(tokens / (s["median"] * 1e-6) / 1e9, 2)}
lines.append("compress (tokens_per_s in 1e9) " + json.dumps(comp))

bpt = {"bf16": 2 * E + 4, "fp8": E + 8, **{f"res{nb}": 2 + E * nb // 8 + 4 for nb in NBITS}}
head = [
    "Residual-compressed token index kernels (polus_amd/csrc/residual.hip) against the bf16 and FP8 index kernels, one MI355X (gfx950).",
    f"One process; per round every variant once in turn on the same inputs, bf16 again at the end; {args.warmup} warm-up rounds, {args.rounds} timed; HIP events, us.",
    f"Corpus {N} documents x Ld {Ld} x E {E}, unit-norm rows: {d.numel() * 2 >> 20} MiB bf16, {(f8.numel() + f8s.numel() * 4) >> 20} MiB FP8 codes + scales; "
    + ", ".join(f"{(packed[nb].numel() + codes[1024].numel() * 2) >> 20} MiB at {nb} bits" for nb in NBITS) + " (codes + residual bits).",
    f"Queries {Q} x Lq {Lq}, bf16.  rerank: C = {C} distinct random candidates per query, {SETS} sets in turn.  Codes uniform over K centroids, K = 1024 "
    f"({1024 * E * 2 >> 10} KiB of centroid rows) and 65535 ({65535 * E * 2 >> 20} MiB).",
    "Bytes per token with the int32 mask: " + ", ".join(f"{k} {v}" for k, v in bpt.items()) + ".",
    "full = no document mask; ragged = document lengths uniform in [90, 180].  Residual rerank scores against polus_maxsim_rerank over the decoded corpus "
    "(K = 1024, ragged, bit for bit): " + ", ".join(f"{nb} bits {'equal' if equal[nb] else 'DIFFERENT'}" for nb in NBITS) + ".",
    f"compress: polus_residual_compress over the whole corpus, {tokens} tokens a call.",
    "",
]
text = "\n".join(head + lines) + "\n"
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    f.write(text)
print(text, flush=True)
