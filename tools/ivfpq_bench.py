"""IVF-PQ [CLS] search beside the exhaustive PQ search and the plain one on tools/pq_bench.py's corpus: N = 1 000 000 vectors of
E = 768 in bf16 drawn around 4096 random centres (SYNTHETIC: centre + 0.7 N(0, 1) noise; queries drawn the same way, same seed
and order as pq_bench), m = 96 and 24 bytes per residual (ksub = 256), K = 1024 and 4096 lists (codec from fit_ivfpq on the
plain index), nprobe = 1, 4, 16, 64, Q = 1, 8 and 64 queries, k = 100.  HIP events around each call after a warm-up; the
variants of a comparison run interleaved, round by round, in this one process; medians.  Prints one JSON line and writes it as
the first line of --out (profiles/ivfpq.txt; the commentary below the first line of an existing file is kept):
  - search[m][K][Q]: `plain_us`, `pq_us` (storage="pq" at the same m), `exhaustive_us` (the IVF-PQ index with nprobe unset) and
    per nprobe `us`, the mean candidates per query, `overlap_pq` / `overlap_exact`: the mean share of the exhaustive PQ
    search's / the plain index's k ids that the probed search returns too (synthetic data: no statement about a real collection)
  - split[m][K][Q][nprobe]: `tables_us` (pq_lut + the centroid GEMM), `probe_us` (topk_merge of the probes, ivf_mark, the
    counting ivf_compact and the copy of Q counts to the host) and `score_us` (ivf_compact of the ids, ivfpq_scores_ids and
    topk_merge per group and chunk)
  - scan[m][K][nprobe] at Q = 64: ops.ivfpq_scores_ids alone over the prepared candidate ids, in look-ups per second
    (candidates * m / time; the -1 padding of shorter rows is not counted)
  - build[m][K]: fit_ivfpq_s (8 + 8 rounds over 65536 sampled vectors) and add in vectors per second, host clock around a
    synchronise; bytes per vector with the lists
These are records, not thresholds.

    python tools/ivfpq_bench.py [--rounds 15] [--warmup 3] [--docs 1000000] [--out profiles/ivfpq.txt]
"""
import argparse
import json
import os
import sys
import time

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
ap.add_argument("--lists", type=int, nargs="+", default=[1024, 4096])
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ivfpq.txt"))
args = ap.parse_args()
N, E, K_TOP, KSUB, CENTRES, BATCH = args.docs, 768, 100, 256, 4096, 65536
MS, QS, NPROBES = (96, 24), (1, 8, 64), (1, 4, 16, 64)
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


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = fn()
    torch.cuda.synchronize()
    return r, time.perf_counter() - t0


def overlap(got, want):
    return round(float(np.mean([len(set(a.tolist()) & set(b.tolist())) / K_TOP for a, b in zip(got.cpu(), want.cpu())])), 3)


def filled(**kw):
    index = CorpusIndex(Given(), InBatchDotScores(), **kw)
    reps = plain.representations
    _, s = wall(lambda: [index.add(reps[a:a + BATCH]) for a in range(0, N, BATCH)])
    return index, s


centres = torch.randn((CENTRES, E), device="cuda", generator=g)
plain = CorpusIndex(Given(), InBatchDotScores())
for a in range(0, N, BATCH):
    plain.add(draw(min(BATCH, N - a)))
queries = {Q: draw(Q) for Q in QS}

out = {"shape": {"N": N, "E": E, "k": K_TOP, "ksub": KSUB, "dtype": "bf16", "corpus": f"synthetic: {CENTRES} centres + 0.7 noise"},
       "rounds": args.rounds, "plain_bytes_per_vector": plain.nbytes // N, "search": {}, "split": {}, "scan": {}, "build": {}}

for m in MS:
    pq, _ = filled(storage="pq", codec=plain.fit_pq(m, KSUB))
    for key in ("search", "split", "scan", "build"):
        out[key][str(m)] = {}
    for K in args.lists:
        codec, fit_s = wall(lambda: plain.fit_ivfpq(K, m, KSUB))
        index, add_s = filled(storage="ivfpq", codec=codec)
        index.refresh_lists()
        sizes = np.diff(index.lists[0].cpu().numpy())
        out["build"][str(m)][str(K)] = {"fit_ivfpq_s": round(fit_s, 3), "add_vectors_per_s": round(N / add_s),
                                        "bytes_per_vector": round(index.nbytes / N, 2), "empty_lists": int((sizes == 0).sum()),
                                        "largest_list": int(sizes.max())}
        print(f"[ivfpq_bench] m {m} K {K}: {out['build'][str(m)][str(K)]}", file=sys.stderr, flush=True)
        search, split, scan = {}, {}, {}
        coarse, codes = index.coarse_codes, index.pq_codes
        for Q in QS:
            q = queries[Q]
            fns = {"plain": lambda: plain.search(q, K_TOP), "pq": lambda: pq.search(q, K_TOP), "exhaustive": lambda: index.search(q, K_TOP)}
            for p in NPROBES:
                fns[f"nprobe{p}"] = lambda p=p: index.search(q, K_TOP, nprobe=p)
            t = interleaved(fns)
            exact_ids, pq_ids = plain.search(q, K_TOP)[1], pq.search(q, K_TOP)[1]
            row = {"plain_us": round(t["plain"], 1), "pq_us": round(t["pq"], 1), "exhaustive_us": round(t["exhaustive"], 1),
                   "exhaustive_overlap_pq": overlap(index.search(q, K_TOP)[1], pq_ids),
                   "exhaustive_overlap_exact": overlap(index.search(q, K_TOP)[1], exact_ids), "nprobe": {}}
            split[str(Q)] = {}
            for p in NPROBES:
                ids = index.search(q, K_TOP, nprobe=p)[1]
                # the stages of _search_probed, one at a time
                state = {}

                def tables():
                    state["lut"], state["cdot"] = index._kind.tables(q)

                def probe():
                    probes = torch.empty((Q, p), dtype=torch.int32, device="cuda")
                    ops.topk_merge(state["cdot"], torch.empty((Q, p), dtype=torch.float32, device="cuda"), probes, init=True)
                    state["bitmap"], state["count"] = index._mark(probes, None, Q, 1)
                    state["counts"] = state["count"].cpu()

                def score():
                    top = (torch.empty((Q, K_TOP), dtype=torch.float32, device="cuda"), torch.empty((Q, K_TOP), dtype=torch.int32, device="cuda"))
                    lut, cdot = state["lut"], state["cdot"]
                    index._scan_probed(state["bitmap"], state["count"], top, lambda a, b, cand: lambda s, e, sc: ops.ivfpq_scores_ids(
                        lut[a:b], cdot[a:b], coarse, codes, cand[:, s:e], sc))

                tables(), probe()
                ts = interleaved({"tables": tables, "probe": probe, "score": score})
                cands = float(state["counts"].float().mean())
                row["nprobe"][str(p)] = {"us": round(t[f"nprobe{p}"], 1), "candidates_per_query": round(cands),
                                         "pq_over_ivfpq": round(t["pq"] / t[f"nprobe{p}"], 2),
                                         "plain_over_ivfpq": round(t["plain"] / t[f"nprobe{p}"], 2),
                                         "overlap_pq": overlap(ids, pq_ids), "overlap_exact": overlap(ids, exact_ids)}
                split[str(Q)][str(p)] = {k: round(v, 1) for k, v in (("tables_us", ts["tables"]), ("probe_us", ts["probe"]),
                                                                     ("score_us", ts["score"]))}
                if Q == 64:                                   # the kernel alone over the prepared ids of all 64 queries
                    C = max(1, int(state["counts"].max()))
                    cand = torch.empty((Q, C), dtype=torch.int32, device="cuda")
                    ops.ivf_compact(state["bitmap"], N, state["count"], cand)
                    spans = index.rerank_chunks(Q, C)
                    scratch = torch.empty((Q, max(b - a for a, b in spans)), dtype=torch.float32, device="cuda")
                    lut, cdot = state["lut"], state["cdot"]

                    def kernel():
                        for a, b in spans:
                            ops.ivfpq_scores_ids(lut, cdot, coarse, codes, cand[:, a:b], scratch[:, :b - a])

                    tk = interleaved({"kernel": kernel})["kernel"]
                    route = ops.ivfpq_scores_ids_route(Q, min(C, 65535), m, KSUB)
                    total = int(state["counts"].sum())
                    scan[str(p)] = {"us": round(tk, 1), "launches": len(spans), "columns": C, "candidates": total,
                                    "lds_bytes": route.lds_bytes, "cols_per_block": route.cols_per_block,
                                    "lookups_per_s": round(total * m / tk * 1e6)}
            search[str(Q)] = row
            print(f"[ivfpq_bench] m {m} K {K} Q {Q}: {row}", file=sys.stderr, flush=True)
        out["search"][str(m)][str(K)], out["split"][str(m)][str(K)], out["scan"][str(m)][str(K)] = search, split, scan
        del index, coarse, codes
    del pq

line = json.dumps(out)
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
notes = open(args.out).read().split("\n", 1)[1:] if os.path.exists(args.out) else []     # the commentary under the line stays
with open(args.out, "w") as f:
    f.write(line + "\n" + "".join(notes))
print(line, flush=True)
