"""CRF NLL (forward + backward) and Viterbi per call at B = 64, S = 256: the one-thread-per-sequence kernels
(C <= 16, loss.hip) and the workgroup-per-sequence kernels (17 <= C <= 128, crf.hip).  HIP events around each
call after a warm-up; the median (and min) of --calls calls.

    python tools/crf_bench.py [--batch 64] [--seq 256] [--calls 25] [--tags 4,9,16,17,32,64,128]
"""
import argparse, os, sys
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from polus_amd import ops

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=64)
ap.add_argument("--seq", type=int, default=256)
ap.add_argument("--calls", type=int, default=25)
ap.add_argument("--warmup", type=int, default=5)
ap.add_argument("--tags", default="4,9,16,17,32,64,128")
args = ap.parse_args()
assert args.calls >= 20
B, S = args.batch, args.seq


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
    return ts[len(ts) // 2], ts[0]


print(f"# B={B} S={S}: median (min) of {args.calls} calls after {args.warmup} warm-up calls, us per call", flush=True)
for C in [int(c) for c in args.tags.split(",")]:
    g = torch.Generator(device="cuda").manual_seed(C)
    pot = torch.randn(B, S, C, device="cuda", generator=g) * 2
    tags = torch.randint(0, C, (B, S), device="cuda", generator=g, dtype=torch.int32)
    lengths = torch.full((B,), S, dtype=torch.int32, device="cuda")
    trans = torch.randn(C, C, device="cuda", generator=g) * 0.5
    loss = torch.empty(1, device="cuda")
    dpot = torch.empty(B, S, C, device="cuda")
    dtrans = torch.empty(C, C, device="cuda")
    out = torch.empty(B, S, dtype=torch.int32, device="cuda")
    nll = timed(lambda: ops.crf_nll(pot, tags, lengths, trans, None, loss, dpot, dtrans))
    vit = timed(lambda: ops.crf_viterbi(pot, lengths, trans, out))
    kind = "thread/seq" if C <= 16 else "workgroup/seq"
    print(f"C={C:4d} ({kind:13s})  nll {nll[0]:9.1f} ({nll[1]:9.1f})   viterbi {vit[0]:9.1f} ({vit[1]:9.1f})", flush=True)
