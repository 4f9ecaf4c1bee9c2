"""The masked-LM path at the BERT-base pre-training shape: B 64, S 256, P 40 masked positions per sequence
(R = 2560 rows), V 30522.  HIP events around each call after a warm-up; the median of --calls calls.  Prints one JSON line:
  - xent[dtype]: the wide loss kernel (count + row kernel + finalize) in place on a [R, V] matrix with a 16-byte row
    stride: us, the compulsory bytes (R V elements read + written), bound_us = those bytes at 6.3 TB/s (the achievable
    HBM rate the fused AdamW reaches), fraction = bound_us / us, the route taken; plus us_unpadded, the same matrix with
    ldl = V (scalar accesses)
  - gather[dtype]: gather_rows of the R masked rows out of [B S, 768], and the scatter back (inverse map + gather)
  - step: a full MLM training step of BERT-base (bf16 engine, dropout 0.1, AdamW) next to the token-classification
    step (4 labels) of the same B x S, each timed in alternating blocks in this process; head_ms = the difference

    python tools/mlm_bench.py [--calls 30] [--warmup 5] [--steps 10] [--no-step]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from polus_amd import ops  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--calls", type=int, default=30)
ap.add_argument("--warmup", type=int, default=5)
ap.add_argument("--steps", type=int, default=10)
ap.add_argument("--no-step", action="store_true")
args = ap.parse_args()
B, S, P, V, H = 64, 256, 40, 30522, 768
R = B * P
HBM = 6.3e12


def timed(fn, calls=None, warmup=None):
    for _ in range(args.warmup if warmup is None else warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(args.calls if calls is None else calls):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1) * 1e3)
    ts.sort()
    return ts[len(ts) // 2]


out = {"shape": {"B": B, "S": S, "P": P, "R": R, "V": V, "H": H}, "calls": args.calls, "hbm_tb_s": HBM / 1e12}
g = torch.Generator(device="cuda").manual_seed(7)
labels = torch.randint(0, V, (R,), device="cuda", generator=g).to(torch.int32)
labels[::9] = -1
loss, stats = torch.empty(1, device="cuda"), torch.empty(2, dtype=torch.int32, device="cuda")
out["xent"], out["gather"] = {}, {}
for name, dt in (("bf16", torch.bfloat16), ("f32", torch.float32)):
    es = 2 if dt == torch.bfloat16 else 4
    ld = (V * es + 15) // 16 * 16 // es
    src = (torch.randn(R, ld, device="cuda", generator=g) * 4).to(dt)
    work = torch.empty_like(src)
    r = {}
    for key, stride in (("us", ld), ("us_unpadded", V)):
        view = work.view(-1)[:R * stride].view(R, stride)[:, :V]

        def call():
            ops.softmax_xent_wide(view, labels, loss, stats=stats)       # in place; the values drift to a gradient's, the traffic does not
        view.copy_(src[:, :V])
        r[key] = timed(call)
        route = ops.softmax_xent_wide_route(view)
        r["route" if key == "us" else "route_unpadded"] = [route.path, "16B" if route.vec16 else "scalar", route.lds_bytes]
    r["bytes"] = 2 * R * V * es
    r["bound_us"] = r["bytes"] / HBM * 1e6
    r["fraction_of_bound"] = r["bound_us"] / r["us"]
    out["xent"][name] = {k: (round(v, 3) if isinstance(v, float) else v) for k, v in r.items()}
    del src, work
    x = torch.randn(B * S, H, device="cuda", generator=g).to(dt)
    idx = (torch.arange(B, device="cuda")[:, None] * S + torch.argsort(torch.rand(B, S, device="cuda", generator=g), 1)[:, :P]).to(torch.int32).reshape(-1).contiguous()
    y, inv, back = torch.empty(R, H, dtype=dt, device="cuda"), torch.empty(B * S, dtype=torch.int32, device="cuda"), torch.empty_like(x)

    def scatter():
        ops.inverse_map(idx, inv)
        ops.gather_rows(y, inv, back)
    gr = {"gather_us": timed(lambda: ops.gather_rows(x, idx, y)), "scatter_us": timed(scatter)}
    gr["scatter_bound_us"] = (B * S * H + R * H) * es / HBM * 1e6
    out["gather"][name] = {k: round(v, 3) for k, v in gr.items()}

if not args.no_step:
    from polus_amd.data import mask_tokens
    from polus_amd.losses import MaskedSparseCategoricalCrossentropy, SparseCategoricalCrossentropy
    from polus_amd.models import BertConfig, BertForMaskedLM, BertModel
    from polus_amd.optimizers import AdamWeightDecay
    from polus_amd.training import ClassifierTrainer
    rng = np.random.Generator(np.random.PCG64(3))
    ids = rng.integers(1000, V, size=(B, S)).astype(np.int32)
    att = np.ones((B, S), np.int32)
    mids, pos, mlab = mask_tokens(ids, att, mask_id=103, vocab_size=V, special_ids=(0, 100, 101, 102, 103), max_predictions=P, rng=rng)
    dev = lambda a: torch.as_tensor(a).cuda()
    cfg = dict(hidden_dropout_prob=0.1, attention_probs_dropout_prob=0.1)
    mlm = BertForMaskedLM(BertConfig(**cfg), compute_dtype="bf16")
    mlm_tr = ClassifierTrainer(mlm, AdamWeightDecay(1e-4, weight_decay_rate=0.01), MaskedSparseCategoricalCrossentropy())
    xm, ym = {"input_ids": dev(mids), "attention_mask": dev(att), "masked_positions": dev(pos)}, dev(mlab)
    cls = BertModel(BertConfig(**cfg), compute_dtype="bf16", num_labels=4)
    cls_tr = ClassifierTrainer(cls, AdamWeightDecay(1e-4, weight_decay_rate=0.01), SparseCategoricalCrossentropy(grad_dtype=cls.compute_dtype))
    xc, yc = {"input_ids": dev(ids), "attention_mask": dev(att)}, dev(rng.integers(0, 4, size=(B, S)).astype(np.int32))
    a, b = [], []
    for _ in range(3):                                   # alternating blocks: both see the same clocks
        a.append(timed(lambda: mlm_tr.train_step(xm, ym), calls=args.steps, warmup=3))
        b.append(timed(lambda: cls_tr.train_step(xc, yc), calls=args.steps, warmup=3))
    a.sort(); b.sort()
    out["step"] = {"mlm_ms": round(a[1] / 1e3, 3), "token_classification_ms": round(b[1] / 1e3, 3),
                   "head_ms": round((a[1] - b[1]) / 1e3, 3), "mlm_over_classification": round(a[1] / b[1], 4),
                   "counted": int(mlm_tr.loss.counted), "steps": args.steps}
print(json.dumps(out), flush=True)
