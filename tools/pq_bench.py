"""Product-quantised [CLS] search beside the plain one at collection shapes: N = 1 000 000 vectors of E = 768 in bf16, drawn
around 4096 random centres (a SYNTHETIC clustered corpus: centre + 0.7 N(0, 1) noise; queries are drawn the same way), a plain
CorpusIndex and PQ indexes with m = 96, 48 and 24 bytes per vector (ksub = 256, codec from fit_pq on the plain index), Q = 1, 8
and 64 queries, k = 100.  HIP events around each call after a warm-up; the variants of a comparison run interleaved, round by
round, in this one process; medians.  Prints one JSON line and writes it as the first line of --out (profiles/pq.txt; whatever
stands below the first line of an existing file, the commentary, is kept):
  - search[m][Q]: `pq_us` = CorpusIndex.search on the PQ index (pq_lut, then pq_scores + topk_merge per chunk of 65535
    documents) beside `plain_us` = the same call on the plain bf16 index (gemm + topk_merge per chunk), with the bytes per
    vector of both and `overlap`: the mean share of the plain index's k ids that the PQ index returns too (synthetic data:
    no statement about a real collection)
  - scan[m][Q]: ops.pq_scores alone over all chunks, with the route's qt and LDS bytes and the look-ups per second
    (Q * N * m / time), and `lut_us`: ops.pq_lut alone
  - encode[m]: ops.pq_encode of 65536 vectors, in vectors per second; fit_pq_s: one CorpusIndex.fit_pq(96) (8 rounds over
    65536 sampled vectors), host clock around a synchronise
These are records, not thresholds.

    python tools/pq_bench.py [--rounds 15] [--warmup 3] [--docs 1000000] [--out profiles/pq.txt]
"""
import argparse
import json
import os
import sys
import time

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
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pq.txt"))
args = ap.parse_args()
N, E, K, KSUB, CENTRES, BATCH = args.docs, 768, 100, 256, 4096, 65536
MS, QS = (96, 48, 24), (1, 8, 64)
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


centres = torch.randn((CENTRES, E), device="cuda", generator=g)
plain = CorpusIndex(Given(), InBatchDotScores())
for a in range(0, N, BATCH):
    plain.add(draw(min(BATCH, N - a)))
queries = {Q: draw(Q) for Q in QS}

out = {"shape": {"N": N, "E": E, "k": K, "ksub": KSUB, "dtype": "bf16", "corpus": f"synthetic: {CENTRES} centres + 0.7 noise"},
       "rounds": args.rounds, "plain_bytes_per_vector": plain.nbytes // N, "search": {}, "scan": {}, "encode": {}}

torch.cuda.synchronize()
t0 = time.perf_counter()
codecs = {96: plain.fit_pq(96, KSUB)}
torch.cuda.synchronize()
out["fit_pq_s"] = round(time.perf_counter() - t0, 3)
for m in MS[1:]:
    codecs[m] = plain.fit_pq(m, KSUB)

for m in MS:
    index = CorpusIndex(Given(), InBatchDotScores(), storage="pq", codec=codecs[m])
    reps = plain.representations
    for a in range(0, N, BATCH):
        index.add(reps[a:a + BATCH])
    cb = codecs[m].codebooks.cuda()
    codes = index.pq_codes
    batch, batch_codes = reps[:BATCH], torch.empty((min(BATCH, N), m), dtype=torch.uint8, device="cuda")
    t = interleaved({"encode": lambda: ops.pq_encode(batch, cb, batch_codes)})
    out["encode"][str(m)] = {"us": round(t["encode"], 1), "vectors_per_s": round(batch.shape[0] / t["encode"] * 1e6)}
    out["search"][str(m)], out["scan"][str(m)] = {}, {}
    for Q in QS:
        q = queries[Q]
        spans = index.chunks(Q)
        lut = torch.empty((Q, m, KSUB), dtype=torch.float32, device="cuda")
        scratch = torch.empty((Q, max(b - a for a, b in spans)), dtype=torch.float32, device="cuda")

        def scan():
            for a, b in spans:
                ops.pq_scores(lut, codes[a:b], scratch[:, :b - a])

        t = interleaved({"pq": lambda: index.search(q, K), "plain": lambda: plain.search(q, K), "scan": scan,
                         "lut": lambda: ops.pq_lut(q, cb, lut)})
        same = [len(set(a.tolist()) & set(b.tolist())) / K for a, b in zip(index.search(q, K)[1].cpu(), plain.search(q, K)[1].cpu())]
        route = ops.pq_scores_route(Q, min(N, 65535), m, KSUB)
        out["search"][str(m)][str(Q)] = {"pq_us": round(t["pq"], 1), "plain_us": round(t["plain"], 1),
                                         "plain_over_pq": round(t["plain"] / t["pq"], 2), "bytes_per_vector": index.nbytes // N,
                                         "overlap": round(sum(same) / len(same), 3)}
        out["scan"][str(m)][str(Q)] = {"scan_us": round(t["scan"], 1), "launches": len(spans), "qt": route.qt,
                                       "lds_bytes": route.lds_bytes, "lookups_per_s": round(Q * N * m / t["scan"] * 1e6),
                                       "code_bytes_per_s": round(-(-Q // route.qt) * N * m / t["scan"] * 1e6), "lut_us": round(t["lut"], 1)}
    del index, codes

line = json.dumps(out)
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
notes = open(args.out).read().split("\n", 1)[1:] if os.path.exists(args.out) else []     # the commentary under the line stays
with open(args.out, "w") as f:
    f.write(line + "\n" + "".join(notes))
print(line, flush=True)
