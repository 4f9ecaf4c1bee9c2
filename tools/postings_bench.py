"""The inverted route of the lexical first stages beside the forward route, on the Zipf corpus of tools/bm25_bench.py:
40 000 documents x 180 tokens, V = 30522, ids drawn with probability proportional to rank^-1, 64 queries of 18 tokens.
HIP events around each call after a warm-up; variants that are compared run interleaved, round by round, in this one
process; medians.  Prints one JSON line and writes it as the first line of --out (profiles/postings.txt; whatever
stands below the first line of an existing file, the commentary, is kept):
  - build[block_docs]: BM25Index.refresh_postings() as wall time around a synchronise (it contains the 8-byte copy), and
    its three steps alone, ops.postings_count / postings_offsets / postings_fill; P, the bytes of the postings and of
    the forward arrays; hot = the most postings one (block, term) counter takes
  - search[block_docs]: BM25Index.search (k = 100) on the inverted route and BM25Index.search_forward on the same index,
    and the two score kernels alone; agree = the share of result ids the two routes have in common per query (their
    scores differ by rounding: the forward route sums through an fma chain in slot order)
  - big: the same at --big-docs documents of --big-len tokens
  - splade[block_docs]: a SparseCorpusIndex of 128-term documents, dense queries of 40 non-zeros, both routes
These are records, not thresholds.

    python tools/postings_bench.py [--rounds 15] [--warmup 3] [--out profiles/postings.txt]
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
from polus_amd.ir.lexical import BM25Index  # noqa: E402
from polus_amd.ir.search import SparseCorpusIndex  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=15)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--docs", type=int, default=40000)
ap.add_argument("--big-docs", type=int, default=1000000)
ap.add_argument("--big-len", type=int, default=60)
ap.add_argument("--big-rounds", type=int, default=5)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "postings.txt"))
args = ap.parse_args()
V, Q, K = 30522, 64, 100
BLOCK_DOCS = (4096, 8192, 16384, 32768)
g = torch.Generator(device="cuda").manual_seed(11)


def interleaved(fns, rounds=None, warmup=None):
    """{name: median us}: every variant once per round, `rounds` rounds after `warmup` rounds."""
    for _ in range(args.warmup if warmup is None else warmup):
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    ts = {name: [] for name in fns}
    for _ in range(args.rounds if rounds is None else rounds):
        for name, fn in fns.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            ts[name].append(e0.elapsed_time(e1) * 1e3)
    return {name: round(sorted(v)[len(v) // 2], 2) for name, v in ts.items()}


def zipf(shape, s=1.0):
    """ids with probability proportional to rank^-s; which id has which rank is a seeded permutation."""
    p = torch.arange(1, V + 1, device="cuda", dtype=torch.float64) ** -s
    n = 1
    for d in shape:
        n *= d
    ranks = torch.cat([torch.multinomial(p, min(1 << 23, n - a), replacement=True, generator=g) for a in range(0, n, 1 << 23)])
    return torch.randperm(V, device="cuda", generator=g)[ranks].to(torch.int32).reshape(shape).contiguous()


def agreement(a, b):
    """The mean share of a query's result ids that the other result holds too."""
    a, b = a.cpu().tolist(), b.cpu().tolist()
    return round(sum(len(set(x) & set(y)) / len(x) for x, y in zip(a, b)) / len(a), 4)


def corpus(N, L):
    ids = zipf((N, L))
    lens = torch.randint(L // 2, L + 1, (N, 1), device="cuda", generator=g)
    mask = (torch.arange(L, device="cuda")[None] < lens).to(torch.int32).contiguous()
    return ids, mask


def bm25_records(N, L, queries, rounds, warmup):
    """The build and search records of BM25 indexes over one corpus, one index per block_docs."""
    ids, mask = corpus(N, L)
    indexes = {}
    for bd in BLOCK_DOCS:
        ix = BM25Index(V, terms=L, postings=True, block_docs=bd)
        for a in range(0, N, 8192):
            ix.add({"input_ids": ids[a:a + 8192], "attention_mask": mask[a:a + 8192]})
        ix.refresh()
        indexes[bd] = ix
    del ids, mask
    build, search = {}, {}
    for bd, ix in indexes.items():
        walls = []
        for _ in range(warmup + rounds):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            ix.refresh_postings()
            torch.cuda.synchronize()
            walls.append((time.perf_counter() - t0) * 1e6)
        walls = sorted(walls[warmup:])
        offsets, base, post_doc, post_w = ix.postings
        nblk = offsets.shape[0]
        scratch = torch.empty((nblk, V), dtype=torch.int32, device="cuda")
        fwd = (ix.term_ids, ix.weights)
        ops.postings_count(*fwd, V, bd, scratch)
        hot = int(scratch.max())
        t = interleaved({"count": lambda: ops.postings_count(*fwd, V, bd, scratch),
                         "offsets": lambda: ops.postings_offsets(scratch, offsets, base),
                         "fill": lambda: ops.postings_fill(*fwd, bd, offsets, base, scratch, post_doc, post_w)}, rounds, warmup)
        ix.refresh_postings()                                   # the timed fills ran on cursors, not counts: build again
        P = int(ix.postings[1][-1])
        build[str(bd)] = {"wall_us": round(walls[len(walls) // 2], 1), "count_us": t["count"], "offsets_us": t["offsets"],
                          "fill_us": t["fill"], "P": P, "hot": hot, "blocks": nblk,
                          "postings_bytes": ix._postings.nbytes, "forward_bytes": ix.nbytes - ix._postings.nbytes,
                          "scratch_bytes": 4 * nblk * V}
        del scratch
    fns = {"forward": lambda: indexes[BLOCK_DOCS[1]].search_forward(queries, K)}
    for bd, ix in indexes.items():
        fns[f"inverted_{bd}"] = (lambda ix=ix: ix.search(queries, K))
    t = interleaved(fns, rounds, warmup)
    want = indexes[BLOCK_DOCS[1]].search_forward(queries, K)
    for bd, ix in indexes.items():
        got = ix.search(queries, K)
        search[str(bd)] = {"inverted_us": t[f"inverted_{bd}"], "forward_us": t["forward"],
                           "forward_over_inverted": round(t["forward"] / t[f"inverted_{bd}"], 3),
                           "agree": agreement(got[1], want[1]),
                           "max_score_diff": float((got[0] - want[0]).abs().max()) if agreement(got[1], want[1]) == 1.0 else None}
    # the score kernels alone, one launch over the first chunk of the forward route (at most 65535 documents)
    ix = indexes[BLOCK_DOCS[1]]
    n = min(N, 65535 // BLOCK_DOCS[1] * BLOCK_DOCS[1])
    dense = ix.encode_queries(queries)
    lists = ix.encode_query_lists(queries)
    score = torch.empty((Q, n), dtype=torch.float32, device="cuda")
    kern = {"forward_scores": lambda: ops.sparse_scores(dense, ix.term_ids[:n], ix.weights[:n], score)}
    for bd, jx in indexes.items():
        nb = n // bd
        if nb:
            kern[f"inverted_scores_{bd}"] = (lambda jx=jx, bd=bd, nb=nb: ops.postings_scores(
                *lists, *jx.postings, bd, 0, nb, N, score[:, :min(nb * bd, N)]))
    t = interleaved(kern, rounds, warmup)
    t["documents"] = n
    t["topk_merge_us"] = interleaved({"m": lambda: ops.topk_merge(score, torch.empty((Q, K), device="cuda"),
                                                                  torch.empty((Q, K), dtype=torch.int32, device="cuda"),
                                                                  init=True)}, rounds, warmup)["m"]
    return {"N": N, "L": L, "build": build, "search": search, "kernels": t}


out = {"shape": {"V": V, "Q": Q, "k": K}, "rounds": args.rounds}
qlen = torch.randint(4, 17, (Q, 1), device="cuda", generator=g) + 2  # [CLS] + 4..16 tokens + [SEP]
q_ids = zipf((Q, 18), s=0.7)
q_mask = (torch.arange(18, device="cuda")[None] < qlen).to(torch.int32).contiguous()
queries = {"input_ids": q_ids, "attention_mask": q_mask}
out["bm25"] = bm25_records(args.docs, 180, queries, args.rounds, args.warmup)
torch.cuda.empty_cache()
if args.big_docs:
    out["big"] = bm25_records(args.big_docs, args.big_len, queries, args.big_rounds, 2)
    torch.cuda.empty_cache()


class _Given:
    """Hands the sparse index ready-made representations."""

    def encode_query(self, x, training=False):
        return x

    encode_document = query_projection = document_projection = encode_query


N = args.docs
sparse = {bd: SparseCorpusIndex(_Given(), terms=128, postings=True, block_docs=bd) for bd in BLOCK_DOCS}
for a in range(0, N, 2048):
    n = min(2048, N - a)
    d = torch.zeros(n, V, device="cuda")
    d.scatter_(1, torch.randint(0, V, (n, 256), device="cuda", generator=g), torch.rand(n, 256, device="cuda", generator=g) + 0.01)
    for ix in sparse.values():
        ix.add(d)
dense_q = torch.zeros(Q, V, device="cuda")
dense_q.scatter_(1, torch.randint(0, V, (Q, 40), device="cuda", generator=g), torch.rand(Q, 40, device="cuda", generator=g) + 0.01)
fns = {"forward": lambda: sparse[BLOCK_DOCS[1]].search_forward(dense_q, K)}
for bd, ix in sparse.items():
    ix.refresh_postings()
    fns[f"inverted_{bd}"] = (lambda ix=ix: ix.search(dense_q, K))
t = interleaved(fns)
want = sparse[BLOCK_DOCS[1]].search_forward(dense_q, K)
out["splade"] = {"N": N, "terms": 128, "query_nonzeros": 40}
for bd, ix in sparse.items():
    out["splade"][str(bd)] = {"inverted_us": t[f"inverted_{bd}"], "forward_us": t["forward"],
                              "forward_over_inverted": round(t["forward"] / t[f"inverted_{bd}"], 3),
                              "P": int(ix.postings[1][-1]), "postings_bytes": ix._postings.nbytes,
                              "agree": agreement(ix.search(dense_q, K)[1], want[1])}

line = json.dumps(out)
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
notes = open(args.out).read().split("\n", 1)[1:] if os.path.exists(args.out) else []     # the commentary under the line stays
with open(args.out, "w") as f:
    f.write(line + "\n" + "".join(notes))
print(line, flush=True)
