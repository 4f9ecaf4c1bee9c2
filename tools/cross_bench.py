"""Cross-encoder reranking at the BERT-base shape: 64 queries x 100 candidates, max_length 256, bf16 engine.  HIP events
around each call after a warm-up, same process, the two legs of a comparison alternating; the median, minimum and
maximum of --calls calls.  Prints one JSON line (profiles/cross.txt keeps it):
  - ragged: CrossEncoderIndex.score with bucketing against bucket=False on passages whose lengths come from the seeded
    distribution below; pairs/s of both, their ratio, the bucket plan, and the largest difference between the two
    score matrices (the same pairs at another padded length and batch composition: bf16 rounding, not bits)
  - full: the same on documents that fill the row, where bucketing can only cost (its length pass, the copy of the Q C
    lengths to the host, the sort)
  - overhead: ops.pair_lengths + the copy + plan_buckets + every bucket's ops.pair_pack and ops.pair_scatter_scores
    without the encoder, as a share of a bucketed call
  - step: one CrossEncoderTrainer step at B 32, k 7 (256 pairs x 256 tokens, dropout 0.1, AdamW)
Length distribution (seed 11): query tokens uniform in 4..16; passage tokens round(lognormal(log 60, 0.45)) clipped to
8..250; both plus [CLS] and [SEP], which strip (1, 1) takes off again.  These are records, not thresholds.

    python tools/cross_bench.py [--calls 5] [--warmup 1] [--steps 5] [--tokens-per-batch 32768] [--no-step]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from polus_amd import ops  # noqa: E402
from polus_amd.ir.cross import CrossEncoderIndex, plan_buckets  # noqa: E402
from polus_amd.ir.models import CrossEncoder  # noqa: E402
from polus_amd.models import BertConfig  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--calls", type=int, default=5)
ap.add_argument("--warmup", type=int, default=1)
ap.add_argument("--steps", type=int, default=5)
ap.add_argument("--tokens-per-batch", type=int, default=32768)
ap.add_argument("--no-step", action="store_true")
args = ap.parse_args()
assert torch.cuda.is_available(), "cross_bench.py measures on the GPU: there is nothing to report without one"
Q, C, N, S, LQ, MAXQ, V = 64, 100, 4096, 256, 20, 32, 30522
CLS, SEP, PAD = 101, 102, 0
rng = np.random.Generator(np.random.PCG64(11))


def texts(lens, L):
    """HF-shaped rows cls w.. sep pad..; lens counts the ordinary tokens."""
    n = len(lens)
    ids = rng.integers(1000, V, size=(n, L)).astype(np.int32)
    col = np.arange(L)
    ids[:, 0] = CLS
    ids = np.where(col == lens[:, None] + 1, SEP, ids)
    mask = (col < lens[:, None] + 2).astype(np.int32)
    return {"input_ids": torch.as_tensor(np.where(mask > 0, ids, PAD).astype(np.int32)).cuda(),
            "attention_mask": torch.as_tensor(mask).cuda()}


def interleaved(legs, calls, warmup):
    """{name: [us, ...]}: the legs run in turn, `calls` rounds after `warmup` rounds."""
    for _ in range(warmup):
        for fn in legs.values():
            fn()
    torch.cuda.synchronize()
    ts = {k: [] for k in legs}
    for _ in range(calls):
        for k, fn in legs.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            ts[k].append(e0.elapsed_time(e1) * 1e3)
    return ts


def stats(us, pairs):
    us = sorted(us)
    med = us[len(us) // 2]
    return {"ms": round(med / 1e3, 3), "ms_min": round(us[0] / 1e3, 3), "ms_max": round(us[-1] / 1e3, 3),
            "pairs_per_s": round(pairs / (med * 1e-6), 1)}


model = CrossEncoder(BertConfig(hidden_dropout_prob=0.1, attention_probs_dropout_prob=0.1), compute_dtype="bf16")
queries = texts(rng.integers(4, 17, size=Q), LQ)
cand = torch.as_tensor(np.stack([rng.choice(N, size=C, replace=False) for _ in range(Q)]).astype(np.int32)).cuda()
out = {"shape": {"Q": Q, "C": C, "max_length": S, "max_query_tokens": MAXQ, "documents": N, "model": "BERT-base bf16"},
       "calls": args.calls, "tokens_per_batch": args.tokens_per_batch}


def prep_only(index):
    """A bucketed call without the encoder: lengths, the copy, the plan, every bucket's pack and scatter."""
    q, qm = index._queries(queries)
    P = Q * C
    length = torch.empty(P, dtype=torch.int32, device="cuda")
    ops.pair_lengths((Q, LQ), qm, (len(index), index.doc_tokens), index.mask, cand, length, index.strip + index.strip, MAXQ, S)
    plan = plan_buckets(length.cpu().numpy(), index.tokens_per_batch, index.round_to, S)
    order = torch.as_tensor(np.concatenate([rows for _, rows in plan])).cuda()
    res = torch.empty((Q, C), dtype=torch.float32, device="cuda")
    fake = torch.zeros(P, dtype=torch.float32, device="cuda")
    at = 0
    for s_b, rows in plan:
        buf = torch.empty((3, rows.size, s_b), dtype=torch.int32, device="cuda")
        ops.pair_pack(q, qm, index.token_ids, index.mask, cand, buf[0], buf[1], buf[2], index.strip + index.strip, MAXQ,
                      index.special, rows=order[at:at + rows.size])
        ops.pair_scatter_scores(fake, cand, len(index), res, rows=order[at:at + rows.size])
        at += rows.size


for name, lens in (("ragged", np.clip(np.rint(rng.lognormal(np.log(60.0), 0.45, size=N)), 8, 250).astype(np.int64)),
                   ("full", np.full(N, S - 2, np.int64))):
    index = CrossEncoderIndex(model, doc_tokens=S, strip=(1, 1), max_query_tokens=MAXQ, max_length=S, cls_token_id=CLS,
                              sep_token_id=SEP, pad_token_id=PAD, tokens_per_batch=args.tokens_per_batch)
    index.add(texts(lens, S))
    keep = {}
    legs = {"bucketed": lambda: keep.__setitem__("b", index.score(queries, cand, bucket=True)),
            "flat": lambda: keep.__setitem__("f", index.score(queries, cand, bucket=False)),
            "prep": lambda: prep_only(index)}
    ts = interleaved(legs, args.calls, args.warmup)
    index.score(queries, cand, bucket=True)
    plan = index.last_plan
    b, f = stats(ts["bucketed"], Q * C), stats(ts["flat"], Q * C)
    prep = sorted(ts["prep"])[len(ts["prep"]) // 2]
    hist = {}
    for s_b, n in plan:
        hist[s_b] = hist.get(s_b, 0) + n
    out[name] = {"doc_tokens_mean": round(float(lens.mean()), 1), "bucketed": b, "flat": f,
                 "bucketed_over_flat_pairs_per_s": round(b["pairs_per_s"] / f["pairs_per_s"], 3),
                 "padded_tokens": {"bucketed": int(sum(s_b * n for s_b, n in plan)), "flat": Q * C * S},
                 "rows_per_bucket_S": hist, "passes": len(plan),
                 "max_abs_score_difference": round(float((keep["b"] - keep["f"]).abs().max()), 5),
                 "max_abs_score": round(float(keep["f"].abs().max()), 5),
                 "overhead": {"prep_ms": round(prep / 1e3, 3), "share_of_bucketed_call": round(prep / (b["ms"] * 1e3), 4)}}
    del index, keep
    torch.cuda.empty_cache()

if not args.no_step:
    from polus_amd.ir.training import CrossEncoderTrainer
    from polus_amd.optimizers import AdamWeightDecay
    B, k = 32, 7
    plens = np.clip(np.rint(rng.lognormal(np.log(60.0), 0.45, size=B * (1 + k))), 8, 250).astype(np.int64)
    pos, neg = texts(plens[:B], S), texts(plens[B:], S)
    neg = {key: v.view(B, k, S) for key, v in neg.items()}
    q = texts(rng.integers(4, 17, size=B), LQ)
    tr = CrossEncoderTrainer(model, AdamWeightDecay(1e-5, weight_decay_rate=0.01), max_query_tokens=MAXQ, max_length=S,
                             cls_token_id=CLS, sep_token_id=SEP, pad_token_id=PAD)
    ts = interleaved({"step": lambda: tr.train_step(q, pos, neg)}, args.steps, 2)["step"]
    ts.sort()
    out["step"] = {"ms": round(ts[len(ts) // 2] / 1e3, 3), "ms_min": round(ts[0] / 1e3, 3), "ms_max": round(ts[-1] / 1e3, 3),
                   "pairs": B * (1 + k), "tokens": B * (1 + k) * S, "loss": round(float(tr.loss.loss), 4), "steps": args.steps}
print(json.dumps(out), flush=True)
