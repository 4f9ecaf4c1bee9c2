"""GPU: polus_fuse_lists bit for bit against tests/fusion_ref.py on the cases of tests/fusion_cases.py, then fuse and
HybridSearch over stub stages and over two BM25 indexes, and mining from a hybrid first stage.  Outputs are pre-filled
with a sentinel, every 2-d or 3-d tensor is a view of a wider poisoned buffer whose surplus must come back untouched,
and every check prints its figure."""
import numpy as np
import pytest
import torch

from tests import fusion_cases as fc
from tests import fusion_ref as fr

pytestmark = pytest.mark.gpu
SENTINEL = -77
FSENT = -9.25
POISON_ID = 1                  # a valid id: reading the surplus of the id buffer would change the result
POISON_SCORE = 1e6             # finite and larger than every score: reading it would change ranks and hi


def _bits(a):
    a = a.cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    return np.ascontiguousarray(a.astype(np.float32, copy=False)).view(np.int32)


def _wide3(a, extra_rows, extra_cols, fill):
    """(buffer, view): the host array a [L, Q, C] inside a device buffer [L, Q + extra_rows, C + extra_cols] of `fill`."""
    t = torch.as_tensor(np.ascontiguousarray(a))
    L, Q, C = a.shape
    buf = torch.full((L, Q + extra_rows, C + extra_cols), fill, dtype=t.dtype).cuda()
    view = buf[:, :Q, :C]
    view.copy_(t)
    return buf, view


def _out(rows, cols, extra_cols, dtype, fill):
    buf = torch.full((rows + 1, cols + extra_cols), fill, dtype=dtype, device="cuda")
    return buf, buf[:rows, :cols]


def _untouched(buf, rows, cols, fill):
    h = buf.cpu().numpy()
    return bool((h[rows:] == fill).all() and (h[:rows, cols:] == fill).all())


def _run(c, mode, with_scores=True):
    """One launch on strided views with poisoned surroundings; returns host (out_id, out_val, count)."""
    from polus_amd import ops
    L, Q, C = c["ids"].shape
    bi, ids = _wide3(c["ids"], 1, 3, POISON_ID)
    bs, scores = _wide3(c["scores"], 2, 5, POISON_SCORE) if with_scores else (None, None)
    before = (bi.clone(), None if bs is None else bs.clone())
    (boi, out_id), (bov, out_val) = _out(Q, L * C, 4, torch.int32, SENTINEL), _out(Q, L * C, 2, torch.float32, FSENT)
    count = torch.full((Q + 2,), SENTINEL, dtype=torch.int32, device="cuda")
    ops.fuse_lists(ids, scores, out_id, out_val, count, c["n_docs"], mode, weights=c["weights"], rrf_k=c["rrf_k"])
    torch.cuda.synchronize()
    assert _untouched(boi, Q, L * C, SENTINEL) and _untouched(bov, Q, L * C, FSENT), "wrote outside the L*C columns"
    hc = count.cpu().numpy()
    assert (hc[Q:] == SENTINEL).all(), "wrote behind count[Q - 1]"
    assert torch.equal(bi, before[0]) and (bs is None or torch.equal(bs.view(torch.int32), before[1].view(torch.int32))), "an input changed"
    return out_id.cpu().numpy(), out_val.cpu().numpy(), hc[:Q]


def _compare(got, want, what):
    assert np.array_equal(got[2], want[2]), f"{what}: count"
    assert np.array_equal(got[0], want[0]), f"{what}: ids"
    diff = int((_bits(got[1]) != _bits(want[1])).sum())
    assert diff == 0, f"{what}: {diff} fused scores differ in bits"


@pytest.mark.parametrize("name", fc.NAMES)
def test_fuse_lists_matches_the_reference_bit_for_bit(name):
    c = fc.case(name)
    L, Q, C = c["ids"].shape
    for mode in fc.MODE_NAMES:
        want = fc.reference(name, mode)
        _compare(_run(c, mode), want, f"{name}, {mode}")
        n = want[2]
        print(f"[fusion] {name}, {mode}: L {L} Q {Q} C {C}, weights {c['weights']}: {int(n.sum())} fused scores, "
              f"counts {int(n.min())}..{int(n.max())} of {L * C}: ids, counts and value bits equal")
    _compare(_run(c, "rrf", with_scores=False), fc.reference(name, "rrf", False), f"{name}, rrf without scores")


def test_special_rows_come_out_as_the_contract_says():
    got = _run(fc.case("disjoint"), "minmax")
    L, Q, C = fc.case("disjoint")["ids"].shape
    assert (got[2] == L * C).all() and (got[0] == np.arange(L * C)[None]).all()
    for mode in fc.MODE_NAMES:
        out_id, out_val, count = _run(fc.case("holes"), mode)
        assert count[3] == 0 and (out_id[3] == -1).all() and (out_val[3] == -np.inf).all()
    # scores = None under rrf is the launch with scores given when all of them are finite
    for name in ("C = 65", "partial", "repeats"):
        a, b = _run(fc.case(name), "rrf"), _run(fc.case(name), "rrf", with_scores=False)
        assert np.array_equal(a[0], b[0]) and np.array_equal(_bits(a[1]), _bits(b[1])) and np.array_equal(a[2], b[2])
    # the same launch twice gives the same bits
    a, b = _run(fc.case("4095 slots"), "minmax"), _run(fc.case("4095 slots"), "minmax")
    assert all(np.array_equal(_bits(x), _bits(y)) for x, y in zip(a, b))
    print(f"[fusion] disjoint lists: count {L * C} in every row; an all-dropped row: count 0 and (-1, -inf); "
          "rrf without scores equals rrf with finite scores; two launches equal")


class _Fixed:
    """A stage that returns list l of a case whatever the queries are."""

    def __init__(self, c, l):
        self.scores, self.ids, self.n = torch.as_tensor(c["scores"][l]).cuda(), torch.as_tensor(c["ids"][l]).cuda(), c["n_docs"]

    def __len__(self):
        return self.n

    def search(self, queries, k):
        return self.scores[:, :k].contiguous(), self.ids[:, :k].contiguous()


def test_hybrid_search_breaks_the_symmetric_tie_by_id_and_fuse_pads_narrow_lists():
    from polus_amd.ir import HybridSearch, fuse
    c = fc.case("symmetric")
    hybrid = HybridSearch([_Fixed(c, 0), _Fixed(c, 1)], depth=2)
    val, idx = hybrid.search(None, 3)
    assert idx.cpu().tolist() == [[3, 7, -1]]
    b = _bits(val)
    assert b[0, 0] == b[0, 1] and val[0, 2].item() == -np.inf
    print(f"[fusion] symmetric rrf lists: both fused scores have bits {int(b[0, 0]):#x}; ids come back as {idx.cpu().tolist()[0]}")
    # lists of different widths: the narrow ones are padded with (-inf, -1)
    c = fc.case("partial")
    widths = (70, 33, 1)
    results = [(torch.as_tensor(c["scores"][l][:, :w]).cuda(), torch.as_tensor(c["ids"][l][:, :w]).cuda()) for l, w in enumerate(widths)]
    ids = np.full(c["ids"].shape, -1, np.int32)
    scores = np.full(c["scores"].shape, -np.inf, np.float32)
    for l, w in enumerate(widths):
        ids[l, :, :w], scores[l, :, :w] = c["ids"][l][:, :w], c["scores"][l][:, :w]
    for mode in fc.MODE_NAMES:
        got = fuse(results, c["n_docs"], mode, weights=c["weights"], rrf_k=c["rrf_k"])
        want = fr.fuse_lists(ids, scores, c["n_docs"], mode, c["weights"], c["rrf_k"])
        _compare((got[0].cpu().numpy(), got[1].cpu().numpy(), got[2].cpu().numpy()), want, f"ragged, {mode}")
    print(f"[fusion] fuse over lists of widths {widths}: equal to the reference over the padded stack in all modes")


def test_hybrid_search_over_two_bm25_indexes_and_mining_from_it():
    from polus_amd.ir.fusion import HybridSearch
    from polus_amd.ir.lexical import BM25Index
    from polus_amd.ir.mining import mine_negatives
    from tests import bm25_ref as br
    d_ids, d_mask, q_ids, q_mask = fc.corpus()
    N, V, depth, k = fc.E2E["N"], fc.E2E["V"], fc.E2E["depth"], fc.E2E["k"]
    docs = {"input_ids": d_ids, "attention_mask": d_mask}
    queries = {"input_ids": q_ids, "attention_mask": q_mask}
    stages = [BM25Index(V, k1=k1, b=b) for k1, b in fc.E2E["params"]]
    hybrid = HybridSearch(stages, depth, weights=[1.0, 0.3])
    assert hybrid.add(docs).cpu().tolist() == list(range(N)) and len(hybrid) == N
    own = [s.search(queries, depth) for s in stages]
    ids = np.stack([i.cpu().numpy() for _, i in own])
    scores = np.stack([s.cpu().numpy() for s, _ in own])
    differ = int((ids[0] != ids[1]).sum())
    assert differ > 0, "the two stages must rank differently for the fusion to mean anything"
    for method in fc.MODE_NAMES:
        hybrid.method = method
        want_id, want_val, want_count = fr.fuse_lists(ids, scores, N, method, [1.0, 0.3], 60.0)
        want = fr.topk(want_id, want_val, k)
        val, idx = hybrid.search(queries, k)
        assert np.array_equal(idx.cpu().numpy(), want[1]), method
        assert np.array_equal(_bits(val), _bits(want[0])), method
        cand, count = hybrid.candidates(queries)
        cand, count = cand.cpu().numpy(), count.cpu().numpy()
        for r in range(len(q_ids)):
            union = np.union1d(ids[0, r][ids[0, r] >= 0], ids[1, r][ids[1, r] >= 0])
            assert count[r] == len(union) and np.array_equal(cand[r, :count[r]], union) and (cand[r, count[r]:] == -1).all()
        print(f"[fusion] two BM25 stages, {method}: top {k} of {len(q_ids)} queries equal the reference in ids and score bits; "
              f"unions of {int(count.min())}..{int(count.max())} documents from 2 x {depth}; {differ} list positions differ between the stages")
    hybrid.method = "rrf"
    positives = np.arange(len(q_ids), dtype=np.int64)[:, None]
    neg, n_pool, neg_col = mine_negatives(hybrid, queries, positives, k=4, depth=depth, seed=5)
    s, ranked = hybrid.search(queries, depth)
    want = br.mine_negatives(ranked.cpu().numpy(), None, positives, 0, 0.0, 4, 5)
    for name, g, w in zip(("neg", "neg_col", "n_pool"), (neg, neg_col, n_pool), want):
        assert np.array_equal(g.cpu().numpy(), w), name
    hn, hr = neg.cpu().numpy(), ranked.cpu().numpy()
    assert all(set(hn[r][hn[r] >= 0].tolist()) <= set(hr[r].tolist()) - {r} for r in range(len(q_ids))) and (hn >= 0).any()
    print(f"[fusion] mine_negatives over the hybrid stage: pools {n_pool.cpu().tolist()}, every negative from the fused ranking")
