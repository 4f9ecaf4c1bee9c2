"""The SPLADE path at the BERT-base shape: 64 sequences x 256 tokens x V 30522.  HIP events around each call after a
warm-up; the median of --calls calls.  Prints one JSON line (profiles/splade.txt keeps it):
  - pool_fwd[dtype] / pool_bwd[dtype]: the two pooling kernels on a [B S, V] matrix with a 16-byte row stride: us, the
    compulsory bytes (forward: B S V elements read + three [B, V] arrays written, a quarter of the tokens masked and
    not read; backward: B S V elements written + three [B, V] arrays read), bound_us = those bytes at 6.3 TB/s (the
    achievable HBM rate), fraction = bound_us / us
  - flops_reg: the regulariser with its gradient on [64, V]
  - step: one SparseRetrievalTrainer step of BERT-base (bf16 engine, dropout 0.1, AdamW): 16 questions, 16 positives and
    2 x 16 negatives of 256 tokens, 64 sequences in one pass
  - search: 64 dense queries against 100 000 documents of 128 terms (ops.sparse_scores + ops.topk_merge, k = 100),
    against the bytes of the index read once per query block
These are records, not thresholds.

    python tools/splade_bench.py [--calls 20] [--warmup 3] [--steps 5] [--no-step]
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
ap.add_argument("--calls", type=int, default=20)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--steps", type=int, default=5)
ap.add_argument("--no-step", action="store_true")
args = ap.parse_args()
B, S, V = 64, 256, 30522
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


def record(us, nbytes):
    bound = nbytes / HBM * 1e6
    return {"us": round(us, 2), "bytes": int(nbytes), "bound_us": round(bound, 2), "fraction_of_bound": round(bound / us, 4)}


out = {"shape": {"B": B, "S": S, "V": V}, "calls": args.calls, "hbm_tb_s": HBM / 1e12, "pool_fwd": {}, "pool_bwd": {}}
g = torch.Generator(device="cuda").manual_seed(7)
mask = (torch.arange(S, device="cuda")[None] < torch.randint(S // 2, S + 1, (B, 1), device="cuda", generator=g)).to(torch.int32).contiguous()
valid = int(mask.sum())
rep, xmax = torch.empty(B, V, device="cuda"), torch.empty(B, V, device="cuda")
arg = torch.empty(B, V, dtype=torch.int32, device="cuda")
drep = torch.randn(B, V, device="cuda", generator=g)
for name, dt in (("bf16", torch.bfloat16), ("f32", torch.float32)):
    es = 2 if dt == torch.bfloat16 else 4
    ld = (V * es + 15) // 16 * 16 // es
    buf = torch.empty(B * S, ld, dtype=dt, device="cuda")
    for a in range(0, B * S, 1024):                                  # in slices: no f32 copy of the whole matrix
        buf[a:a + 1024].copy_(torch.randn(1024, ld, device="cuda", generator=g))
    logits = buf[:, :V]
    out["pool_fwd"][name] = dict(record(timed(lambda: ops.splade_pool_fwd(logits, mask, rep, xmax, arg, B, S)), valid * V * es + 3 * B * V * 4),
                                 valid_tokens=valid)
    out["pool_fwd"][name]["us_no_mask"] = round(timed(lambda: ops.splade_pool_fwd(logits, None, rep, xmax, arg, B, S)), 2)
    ops.splade_pool_fwd(logits, mask, rep, xmax, arg, B, S)
    out["pool_bwd"][name] = record(timed(lambda: ops.splade_pool_bwd(drep, xmax, arg, logits, B, S)), B * S * V * es + 3 * B * V * 4)
    del buf, logits

loss = torch.zeros(1, device="cuda")
rep.copy_(torch.relu(torch.randn(B, V, device="cuda", generator=g)))
out["flops_reg"] = record(timed(lambda: ops.flops_reg(rep, 1e-3, loss, drep=drep)), 3 * B * V * 4)

# search: a synthetic index of 100 000 documents x 128 terms
from polus_amd.ir.search import SparseCorpusIndex  # noqa: E402
N, M, Q, K = 100_000, 128, 64, 100


class _Given:
    """Hands the index ready-made representations."""

    def encode_query(self, x, training=False):
        return x

    encode_document = query_projection = document_projection = encode_query


index = SparseCorpusIndex(_Given(), terms=M)
for a in range(0, N, 2048):
    n = min(2048, N - a)
    d = torch.zeros(n, V, device="cuda")
    cols = torch.randint(0, V, (n, 2 * M), device="cuda", generator=g)
    d.scatter_(1, cols, torch.rand(n, 2 * M, device="cuda", generator=g) + 0.01)
    index.add(d)
queries = torch.relu(torch.randn(Q, V, device="cuda", generator=g))
ids, w = index.term_ids, index.weights
score = torch.empty(Q, N, device="cuda")
out["search"] = {"queries": Q, "documents": N, "terms": M, "k": K, "index_bytes": index.nbytes,
                 "scores": record(timed(lambda: ops.sparse_scores(queries, ids, w, score)), index.nbytes + Q * N * 4 + Q * V * 4),
                 "search_us": round(timed(lambda: index.search(queries, K)), 2)}

if not args.no_step:
    from polus_amd.ir.models import SpladeEncoder
    from polus_amd.ir.training import SparseRetrievalTrainer
    from polus_amd.models import BertConfig, BertForMaskedLM
    from polus_amd.optimizers import AdamWeightDecay
    del index, score, drep
    torch.cuda.empty_cache()
    rng = np.random.Generator(np.random.PCG64(3))
    Bq, k = 16, 2
    tok = lambda *shape: torch.as_tensor(rng.integers(1000, V, size=shape).astype(np.int32)).cuda()
    ones = lambda *shape: torch.ones(shape, dtype=torch.int32, device="cuda")
    batch = ({"input_ids": tok(Bq, S), "attention_mask": ones(Bq, S)}, {"input_ids": tok(Bq, S), "attention_mask": ones(Bq, S)},
             {"input_ids": tok(Bq, k, S), "attention_mask": ones(Bq, k, S)})
    model = SpladeEncoder(BertForMaskedLM(BertConfig(hidden_dropout_prob=0.1, attention_probs_dropout_prob=0.1), compute_dtype="bf16"))
    tr = SparseRetrievalTrainer(model, AdamWeightDecay(1e-5, weight_decay_rate=0.01), lambda_q=1e-3, lambda_d=1e-3)
    ms = timed(lambda: tr.train_step(*batch), calls=args.steps, warmup=2) / 1e3
    out["step"] = {"ms": round(ms, 3), "sequences": (2 + k) * Bq, "tokens": (2 + k) * Bq * S, "loss": round(float(tr.loss.loss), 4),
                   "logits_bytes": int(model.mlm._bufs["logits"].numel() * 2), "steps": args.steps}
print(json.dumps(out), flush=True)
