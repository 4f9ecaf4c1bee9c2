"""Tuple scoring against all-pairs scoring at the ColBERTv2 distillation shape: B 32 queries with n 64 passages each
(N = 2048 documents), Lq 32, Ld 180, E 128, bf16; full-length and ragged documents (lengths Ld/2..Ld).

  - tuple_us / allpairs_us: TupleMaxSimScores forward + backward (2 048 pairs) and MaxSimScores forward + backward over the
    same 2 048 documents (65 536 pairs), normalisation included in both, timed in this process in alternating blocks
    after a warm-up, HIP events around each forward + backward; medians.  ratio = allpairs_us / tuple_us.
  - dot: ops.dot_tuples_fwd / dot_tuples_bwd at W = 30522 in f32 over the same (B, n), with the bytes they must move
    (forward: q and d once; backward: q, d, dq, dd once) at 5 TB/s beside them.
  - kl_us / mse_us: ops.distill_kl and ops.margin_mse over the [32, 64] score matrix (two and three launches).
Prints one JSON line and writes the report to --out (default profiles/tuples.txt).  Nothing here says anything about
retrieval quality.  The per-kernel split comes from a separate run:
    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/tuples_bench.py --calls 20 --out <dir>/run.txt

    python tools/tuples_bench.py [--calls 50] [--warmup 10] [--rounds 5] [--out profiles/tuples.txt]
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from polus_amd import ops  # noqa: E402
from polus_amd.ir.models import TokenReps  # noqa: E402
from polus_amd.ir.training import MaxSimScores, TupleMaxSimScores  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--calls", type=int, default=50)
ap.add_argument("--warmup", type=int, default=10)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tuples.txt"))
args = ap.parse_args()
B, n, Lq, Ld, E, W = 32, 64, 32, 180, 128, 30522
N = B * n


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


def alternate(fa, fb):
    """Medians of fa and fb, each timed in --rounds alternating blocks of --calls calls."""
    a, b = [], []
    for _ in range(args.rounds):
        a.append(timed(fa))
        b.append(timed(fb))
    a.sort(); b.sort()
    return a[len(a) // 2], b[len(b) // 2]


def rnd(r):
    return {k: (round(v, 3) if isinstance(v, float) else v) for k, v in r.items()}


out = {"shape": {"B": B, "n": n, "N": N, "Lq": Lq, "Ld": Ld, "E": E, "W": W}, "calls": args.calls, "rounds": args.rounds}
g = torch.Generator(device="cuda").manual_seed(7)
dt = torch.bfloat16
q = TokenReps(torch.randn(B, Lq, E, device="cuda", generator=g).to(dt), torch.ones(B, Lq, dtype=torch.int32, device="cuda"))
docs = torch.randn(N, Ld, E, device="cuda", generator=g).to(dt)                 # slot-major: positives, then 63 negative blocks
lens = {"full": torch.full((N, 1), Ld, device="cuda"), "ragged": torch.randint(Ld // 2, Ld + 1, (N, 1), device="cuda", generator=g)}
for docs_kind, ln in lens.items():
    dm = (torch.arange(Ld, device="cuda")[None] < ln).to(torch.int32)
    parts = [TokenReps(docs[i * B:(i + 1) * B], dm[i * B:(i + 1) * B]) for i in range(n)]
    tup, allp = TupleMaxSimScores(), MaxSimScores()
    ds_t = torch.randn(B, n, device="cuda", generator=g)
    ds_a = torch.randn(B, N, device="cuda", generator=g)

    def run_tuple():
        tup(q, *parts)
        tup.backward(ds_t[:, :1], ds_t[:, 1:])

    def run_all():
        allp(q, *parts)
        allp.backward(ds_a[:, :B], ds_a[:, B:])
    run_tuple(); run_all()
    idx = torch.arange(B, device="cuda")
    rows = torch.arange(n, device="cuda")[None] * B + idx[:, None]
    torch.cuda.synchronize()
    same = bool(torch.equal(tup.scores, allp.scores[idx[:, None], rows]))
    t_us, a_us = alternate(run_tuple, run_all)
    out["maxsim_" + docs_kind] = rnd({"tuple_us": t_us, "allpairs_us": a_us, "ratio": a_us / t_us,
                                      "tuple_scores_equal_allpairs_bits": same})
    del tup, allp, parts

del docs
qv = torch.randn(B, W, device="cuda", generator=g)
dv = torch.randn(N, W, device="cuda", generator=g)
score, dsc = torch.empty(B, n, device="cuda"), torch.randn(B, n, device="cuda", generator=g)
dq, dd = torch.empty_like(qv), torch.empty_like(dv)
r = {"fwd_us": timed(lambda: ops.dot_tuples_fwd(qv, dv, score)), "bwd_us": timed(lambda: ops.dot_tuples_bwd(qv, dv, dsc, dq, dd))}
r["fwd_bytes"], r["bwd_bytes"] = 4 * W * (B + N), 4 * W * 2 * (B + N)
r["fwd_bound_us"], r["bwd_bound_us"] = r["fwd_bytes"] / 5e12 * 1e6, r["bwd_bytes"] / 5e12 * 1e6
out["dot_f32"] = rnd(r)
del dv, dd

s = torch.randn(B, n, device="cuda", generator=g) * 8
t = s + torch.randn(B, n, device="cuda", generator=g)
loss, grad = torch.empty(1, device="cuda"), torch.empty_like(s)
out["losses"] = rnd({"kl_us": timed(lambda: ops.distill_kl(s, t, loss, grad)), "mse_us": timed(lambda: ops.margin_mse(s, t, loss, grad))})

line = json.dumps(out)
print(line, flush=True)
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    f.write("Tuple scoring and distillation losses, polus_amd/csrc/tuples.hip, on one MI355X (gfx950): tools/tuples_bench.py.\n"
            f"B {B} queries x n {n} passages (N = {N} documents), Lq {Lq}, Ld {Ld}, E {E}, bf16; dot tuples at W = {W} in f32.\n"
            f"Medians of {args.rounds} alternating blocks of {args.calls} calls after {args.warmup} warm-up calls, HIP events, us.\n"
            "Retrieval quality: not measured.\n\n" + line + "\n\n")
    for kind in lens:
        m = out["maxsim_" + kind]
        verdict = "faster" if m["ratio"] > 1 else "NOT faster"
        f.write(f"{kind} documents: TupleMaxSimScores forward + backward {m['tuple_us']} us, MaxSimScores forward + backward over the "
                f"same {N} documents {m['allpairs_us']} us: the tuple path is {verdict}, all-pairs / tuple = {m['ratio']}.\n")
