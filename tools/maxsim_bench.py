"""Token-level late interaction (MaxSim) at the ColBERT batch shape: B 64 queries, k 1 explicit negative per query
(N = 128 documents), Lq 32, Ld 256, E 128, both engines.  HIP events around each call after a warm-up; the median
of --calls calls.  Prints one JSON line:
  - fwd_us / bwd_us / norm_us: the fused forward, the backward (dQ + dD), and the row L2 normalisation of Q and D
    (forward + backward)
  - fwd_tflops: 2 B N Lq Ld E over the forward time
  - gemm_sim_us (bf16): polus_gemm writing the same [B Lq, N Ld] similarity matrix in bf16, timed alternately with
    the fused forward in this process (fused_fwd_us_alt)
  - bwd_bound_us: the backward's compulsory HBM bytes (argmax, Q, D, dQ, dD) at 5 TB/s, beside its 4 B N Lq E FLOP

    python tools/maxsim_bench.py [--calls 50] [--warmup 10]
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from polus_amd import ops  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--calls", type=int, default=50)
ap.add_argument("--warmup", type=int, default=10)
args = ap.parse_args()
B, K, Lq, Ld, E = 64, 1, 32, 256, 128
N = (1 + K) * B


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
    """Medians of fa and fb, each timed in `rounds` alternating blocks of --calls calls."""
    a, b = [], []
    for _ in range(rounds):
        a.append(timed(fa))
        b.append(timed(fb))
    a.sort(); b.sort()
    return a[len(a) // 2], b[len(b) // 2]


out = {"shape": {"B": B, "k": K, "N": N, "Lq": Lq, "Ld": Ld, "E": E}, "calls": args.calls}
flop = 2.0 * B * N * Lq * Ld * E
for name, dt in (("bf16", torch.bfloat16), ("f32", torch.float32)):
    g = torch.Generator(device="cuda").manual_seed(7)
    q = torch.randn(B, Lq, E, device="cuda", generator=g).to(dt)
    d = torch.randn(N, Ld, E, device="cuda", generator=g).to(dt)
    qm = torch.ones(B, Lq, dtype=torch.int32, device="cuda")
    dm = (torch.arange(Ld, device="cuda")[None] < torch.randint(Ld // 2, Ld + 1, (N, 1), device="cuda", generator=g)).to(torch.int32)
    score = torch.empty(B, N, dtype=torch.float32, device="cuda")
    am = torch.empty(B, N, Lq, dtype=torch.int32, device="cuda")
    ds = torch.randn(B, N, device="cuda", generator=g)
    dq, dd = torch.empty_like(q), torch.empty_like(d)
    fwd = lambda: ops.maxsim_fwd(q, d, qm, dm, score, am)
    fwd()
    bwd = lambda: ops.maxsim_bwd(q, d, ds, am, dq, dd)
    qn, dn = torch.empty_like(q), torch.empty_like(d)
    rq, rd = torch.empty(B * Lq, device="cuda"), torch.empty(N * Ld, device="cuda")
    gq, gd = torch.empty_like(q), torch.empty_like(d)

    def norm():
        ops.l2norm_fwd(q, qn, rq)
        ops.l2norm_fwd(d, dn, rd)
        ops.l2norm_bwd(qn, rq, dq, gq)
        ops.l2norm_bwd(dn, rd, dd, gd)
    r = {"fwd_us": timed(fwd), "bwd_us": timed(bwd), "norm_us": timed(norm)}
    r["fwd_tflops"] = flop / (r["fwd_us"] * 1e-6) / 1e12
    es = q.element_size()
    nbytes = B * N * Lq * 4 + 2 * (B * Lq * E + N * Ld * E) * es + B * N * 4
    r["bwd_bytes"] = nbytes
    r["bwd_flop"] = 4.0 * B * N * Lq * E
    r["bwd_bound_us"] = nbytes / 5e12 * 1e6
    if name == "bf16":
        sim = torch.empty(B * Lq, N * Ld, dtype=dt, device="cuda")
        q2, d2 = q.view(B * Lq, E), d.view(N * Ld, E)
        gemm = lambda: ops.gemm(q2, d2, sim)
        r["fused_fwd_us_alt"], r["gemm_sim_us"] = alternate(fwd, gemm)
        r["gemm_sim_bytes"] = sim.numel() * sim.element_size()
        r["fused_over_gemm"] = r["fused_fwd_us_alt"] / r["gemm_sim_us"]
        del sim
    out[name] = {k: (round(v, 3) if isinstance(v, float) else v) for k, v in r.items()}
print(json.dumps(out), flush=True)
