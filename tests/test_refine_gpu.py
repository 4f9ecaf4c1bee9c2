"""MI355X: the refine kernels against the NumPy float32 reference bit for bit (tests/refine_ref.py), the quantiser against
tests/fp8_ref.py, and CorpusIndex with a refine store: rerank on a plain [CLS] index, search of PQ / IVF-PQ indexes through
the refine stage, TwoStageSearch behind a lexical first stage, and no change without `refine`."""
import functools

import numpy as np
import pytest
import torch

from tests import fp8_ref
from tests import ivfpq_cases as ic
from tests import pq_cases as pc
from tests import refine_cases as rc
from tests import refine_ref as rr
from tests import search_ref as sr
from tests.search_cases import TableModel, batches, token_case

pytestmark = pytest.mark.gpu
DT = {"f32": torch.float32, "bf16": torch.bfloat16}
FSENT = -9.25                  # outputs are pre-filled with it
POISON_X = 1e6                 # the surplus columns of a wide document matrix
POISON_ID = 0                  # a valid id: reading the surplus of a candidate row would score document 0


def _bits(a):
    a = a.cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    return np.ascontiguousarray(a.astype(np.float32, copy=False)).view(np.int32)


def _np(pair):
    torch.cuda.synchronize()
    return pair[0].cpu().numpy(), pair[1].cpu().numpy()


def _same(got, want, what):
    assert np.array_equal(got[1], want[1]), f"{what}: ids differ in {int((got[1] != want[1]).sum())} places"
    assert np.array_equal(_bits(got[0]), _bits(want[0])), f"{what}: values differ"


def _rounded(a, mode):
    """The f32 values the device sees for an input of the mode's dtype."""
    return torch.as_tensor(np.ascontiguousarray(a)).to(DT[mode]).float().numpy()


def _wide(a, extra_cols, fill, dtype=None):
    """(buffer, view): the host array a [R, C] inside a device buffer [R + 1, C + extra_cols] of `fill`."""
    t = torch.as_tensor(np.ascontiguousarray(a))
    t = t if dtype is None else t.to(dtype)
    buf = torch.full((a.shape[0] + 1, a.shape[1] + extra_cols), fill, dtype=t.dtype).cuda()
    view = buf[:a.shape[0], :a.shape[1]]
    view.copy_(t)
    return buf, view


def _launch(q, d, cand, mode, scale=None, wide=True):
    """One launch of ops.cls_rerank (or, with `scale`, ops.cls_rerank_fp8 over the codes d) on strided views with poisoned
    surroundings: ldd > E through a column view (16 more columns: rows stay 16-byte aligned in every dtype), ldcand = C + 3,
    lds = C + 5.  Returns the host scores [B, C]."""
    from polus_amd import ops
    Bq, C = cand.shape
    dq = torch.as_tensor(q).to(DT[mode]).cuda()
    if scale is None:
        bd, dv = _wide(d, 16 if wide else 0, POISON_X, DT[mode])
    else:
        bd, dv = _wide(d, 16 if wide else 0, 0x7E)                    # 448: the largest code
        ds = torch.as_tensor(scale).cuda()
    bn, nv = _wide(cand, 3 if wide else 0, POISON_ID)
    bs = torch.full((Bq + 1, C + (5 if wide else 0)), FSENT, dtype=torch.float32, device="cuda")
    score = bs[:Bq, :C]
    before = [t.clone() for t in (bd, bn)]
    if scale is None:
        ops.cls_rerank(dq, dv, nv, score)
    else:
        ops.cls_rerank_fp8(dq, dv, ds, nv, score)
    torch.cuda.synchronize()
    h = bs.cpu().numpy()
    assert (h[Bq:] == FSENT).all() and (h[:Bq, C:] == FSENT).all(), "wrote outside the [B, C] scores"
    assert all(torch.equal(a, b) for a, b in zip((bd, bn), before)), "an input changed"
    return score.cpu().numpy()


@functools.lru_cache(maxsize=None)
def _kernel_case(E, mode):
    """(q, d) as the device sees them (f32 values) and the reference scores of every pair, computed once per (E, mode)."""
    q, d = rc.gaussian(E)
    q, d = _rounded(q, mode), _rounded(d, mode)
    whole = rr.scores(q, d)
    whole.setflags(write=False)
    return q, d, whole


def _expected(whole, cand, n):
    ok = (cand >= 0) & (cand < n)
    return np.where(ok, np.take_along_axis(whole, np.where(ok, cand, 0).astype(np.int64), 1), np.float32(-np.inf)).astype(np.float32)


# ---------------------------------------------------------------- the kernel
@pytest.mark.parametrize("mode", ["f32", "bf16"])
@pytest.mark.parametrize("E", rc.ES)
def test_kernel_matches_the_reference_bit_for_bit(E, mode):
    q, d, whole = _kernel_case(E, mode)
    absent = 0
    for C in rc.CS:
        cand = rc.candidates(rc.B, C, rc.N)
        got = _launch(q, d, cand, mode)
        want = _expected(whole, cand, rc.N)
        ok = (cand >= 0) & (cand < rc.N)
        assert np.isneginf(got[~ok]).all(), f"E={E} {mode} C={C}: an absent candidate must score -inf"
        assert np.array_equal(_bits(got), _bits(want)), \
            f"E={E} {mode} C={C}: {int((_bits(got) != _bits(want)).sum())} of {got.size} scores differ in bits"
        absent += int((~ok).sum())
    assert absent == 4 * rc.B * 2 + 2, "the cases hold -1, N, INT_MAX, INT_MIN"
    err = np.abs(whole.astype(np.float64) - rr.exact(q, d))
    room = rc.err_bound(E) * 2.0 ** -24 * (np.abs(q.astype(np.float64)) @ np.abs(d.astype(np.float64)).T)
    assert (err <= room).all()
    print(f"[refine] kernel E={E} {mode}: C {rc.CS} on strided views equal the reference in bits ({absent} absent candidates "
          f"score -inf, poisoned surroundings untouched); worst |err| / bound against float64 {float((err / room).max()):.3f}")


@pytest.mark.parametrize("mode", ["f32", "bf16"])
@pytest.mark.parametrize("E", rc.WIDE_ES)
def test_wide_rows_match_the_reference_bit_for_bit(E, mode):
    """Rows of more than 2048 features, up to the limit, as vectors and as codes."""
    q, d = rc.gaussian(E, n=40)
    q, d = _rounded(q, mode), _rounded(d, mode)
    codes, scale = rr.quantize(d)
    for C in (7, 257):
        cand = rc.candidates(rc.B, C, 40)
        got = _launch(q, d, cand, mode)
        assert np.array_equal(_bits(got), _bits(rr.rerank(q, d, cand))), f"E={E} {mode} C={C}"
        got = _launch(q, codes, cand, mode, scale=scale)
        assert np.array_equal(_bits(got), _bits(rr.rerank_fp8(q, codes, scale, cand))), f"E={E} {mode} C={C} fp8"


@pytest.mark.parametrize("mode", ["f32", "bf16"])
def test_kernel_is_exact_on_the_summable_inputs(mode):
    for E in rc.ES:
        q, d = rc.summable(E)
        cand = rc.candidates(rc.B, 257, rc.N)
        got = _launch(q, d, cand, mode)
        ok = (cand >= 0) & (cand < rc.N)
        want = np.take_along_axis(rr.exact(q, d), np.where(ok, cand, 0).astype(np.int64), 1)
        assert np.array_equal(got[ok].astype(np.float64), want[ok]), f"E={E} {mode}"


@pytest.mark.parametrize("mode", ["f32", "bf16"])
def test_bits_depend_on_the_pair_only(mode):
    """The same (query, document) pair at B = 1 and B = 5, in another column, in another chunk of the columns, alone (C = 1),
    on contiguous and on strided operands, and with so many columns that a wave takes several."""
    E = 768
    q, d, whole = _kernel_case(E, mode)
    cand = rc.candidates(rc.B, 257, rc.N)
    want = _expected(whole, cand, rc.N)
    for b in (0, 3):
        alone = _launch(q[b:b + 1], d, cand[b:b + 1], mode)
        assert np.array_equal(_bits(alone), _bits(want[b:b + 1])), f"query {b} at B = 1"
    moved = np.ascontiguousarray(cand[:, ::-1])
    assert np.array_equal(_bits(_launch(q, d, moved, mode)), _bits(want[:, ::-1])), "the columns reversed"
    for a, b in ((0, 100), (100, 103), (103, 257)):
        part = _launch(q, d, np.ascontiguousarray(cand[:, a:b]), mode, wide=False)
        assert np.array_equal(_bits(part), _bits(want[:, a:b])), f"columns {a} .. {b} as a launch of their own"
    for c in (0, 6, 200):
        one = _launch(q, d, np.ascontiguousarray(cand[:, c:c + 1]), mode)
        assert np.array_equal(_bits(one), _bits(want[:, c:c + 1])), f"column {c} with C = 1"
    # many columns: a wave takes more than one batch of candidates
    big = np.ascontiguousarray(np.tile(cand, (1, 40))[:, :10000])
    got = _launch(np.tile(q, (4, 1)), d, np.tile(big, (4, 1)), mode)
    assert np.array_equal(_bits(got), _bits(np.tile(np.tile(want, (1, 40))[:, :10000], (4, 1)))), "B = 20, C = 10000"


# ---------------------------------------------------------------- FP8
@pytest.mark.parametrize("mode", ["f32", "bf16"])
@pytest.mark.parametrize("E", rc.FP8_ES)
def test_fp8_quantiser_and_rerank(E, mode):
    from polus_amd import ops
    _, d = rc.gaussian(E)
    d = d * np.float32(0.05)
    d[3] = 0                                                             # a zero row: e = 0
    d[5, 1] = np.float32(2.0 ** -120)                                    # beside normal entries: quantises to zero
    d[7] = np.float32(2.0 ** -100) * d[7]                                # the clamp at e = -100
    d = _rounded(d, mode)
    x = torch.as_tensor(d).to(DT[mode]).cuda()
    codes = torch.full((rc.N + 1, E), 0xAA, dtype=torch.uint8, device="cuda")
    scale = torch.full((rc.N + 1,), FSENT, dtype=torch.float32, device="cuda")
    ops.cls_fp8_quantize(x, codes[:rc.N], scale[:rc.N])
    torch.cuda.synchronize()
    want_codes, want_scale = rr.quantize(d)
    assert np.array_equal(codes[:rc.N].cpu().numpy(), want_codes), f"E={E} {mode}: codes"
    assert np.array_equal(_bits(scale[:rc.N]), _bits(want_scale)), f"E={E} {mode}: scales"
    assert bool((codes[rc.N] == 0xAA).all()) and float(scale[rc.N]) == FSENT, "wrote past the rows"
    y = torch.full((rc.N + 1, E), 7.0, dtype=DT[mode], device="cuda")
    ops.cls_fp8_dequantize(codes[:rc.N], scale[:rc.N], y[:rc.N])
    torch.cuda.synchronize()
    deq = fp8_ref.dequantize(want_codes, want_scale)
    assert np.array_equal(_bits(y[:rc.N].float()), _bits(deq)) and bool((y[rc.N] == 7.0).all())
    # the rerank over the codes is the rerank over the dequantised matrix, and the reference's FP8 route, in bits
    q = _rounded(rc.gaussian(E)[0], mode)
    for C in rc.CS:
        cand = rc.candidates(rc.B, C, rc.N)
        got = _launch(q, want_codes, cand, mode, scale=want_scale)
        over = _launch(q, deq, cand, mode)
        assert np.array_equal(_bits(got), _bits(over)), f"E={E} {mode} C={C}: fp8 against the dequantised matrix"
        assert np.array_equal(_bits(got), _bits(rr.rerank_fp8(q, want_codes, want_scale, cand))), f"E={E} {mode} C={C}: reference"
    rel = np.linalg.norm(deq - d, axis=1)[8:] / np.linalg.norm(d, axis=1)[8:]
    print(f"[refine] fp8 E={E} {mode}: codes, scales and dequantised rows equal fp8_ref; rerank_fp8 equals rerank over the "
          f"dequantised matrix in bits for C {rc.CS}; relative L2 error of a row {float(rel.mean()):.4f} (mean)")


# ---------------------------------------------------------------- the index
def _queries(c):
    return {"input_ids": c["q_ids"], "attention_mask": c["q_mask"]}


def _index(c, mode, sizes=None, **kw):
    from polus_amd.ir.search import CorpusIndex
    from polus_amd.ir.training import InBatchDotScores
    index = CorpusIndex(TableModel(c["table"], DT[mode], False), InBatchDotScores(), **kw)
    n = len(c["d_ids"])
    for b in batches(c["d_ids"], c["d_mask"], sizes or [n // 2, n - n // 2]):
        index.add(b)
    return index


@pytest.mark.parametrize("mode", ["f32", "bf16"])
def test_rerank_on_a_plain_cls_index(mode):
    q, d = rc.gaussian(rc.INDEX_E, Bq=5, n=700, seed=3)
    q, d = _rounded(q, mode), _rounded(d, mode)
    c = pc.as_search_case(q, d)
    Q, N, C, k = 5, 700, 100, 10
    r = rc.rng(31)
    cand = np.stack([r.permutation(N)[:C] for _ in range(Q)]).astype(np.int32)
    cand[:, 5], cand[1, 40:] = -1, -1
    cand[2] = -1                                                         # a row without a candidate
    want = sr.topk_merge(rr.rerank(q, d, cand), cand, k)
    assert (want[1][2] == -1).all() and np.isneginf(want[0][2]).all()
    plain = _index(c, mode)
    with pytest.raises(ValueError, match=r"\[CLS\].*refine="):
        plain.rerank(_queries(c), cand, k)
    for scratch, chunks in ((256 << 20, 1), (4 * Q * 34, 3)):
        index = _index(c, mode, refine="full", scratch_bytes=scratch)
        assert len(index.rerank_chunks(Q, C)) == chunks and index.nbytes == plain.nbytes
        assert index.refine_vectors.data_ptr() == index.representations.data_ptr(), "no second copy"
        _same(_np(index.rerank(_queries(c), cand, k)), want, f"{mode} host candidates, {chunks} chunk(s)")
        _same(_np(index.rerank(_queries(c), torch.as_tensor(cand).cuda(), k)), want, f"{mode} device candidates, {chunks} chunk(s)")
        _same(_np(index.search(_queries(c), k)), _np(plain.search(_queries(c), k)), "search is unchanged")
    with pytest.raises(ValueError, match=r"candidates must lie in \[-1, 700\)"):
        index.rerank(_queries(c), np.full((Q, 2), N), k)
    far = torch.as_tensor(np.full((Q, 2), N, np.int32)).cuda()           # device ids are taken as they are: absent
    got = _np(index.rerank(_queries(c), far, 2))
    assert (got[1] == -1).all() and np.isneginf(got[0]).all()


def _first_stage(kind):
    """(search case, codec kwargs, docs) of the exactly-summable corpus under the planted codecs: its documents are no
    codewords, so the first stage is lossy and the refine stage has something to repair."""
    from polus_amd.ir.search import IVFPQCodec, PQCodec
    q, d = rc.index_corpus()
    c = pc.as_search_case(q, d)
    if kind == "pq":
        return c, dict(storage="pq", codec=PQCodec(pc.planted()["cb"])), q, d
    p = ic.planted()
    return c, dict(storage="ivfpq", codec=IVFPQCodec(p["cent"] / 16, p["cb"])), q, d


@pytest.mark.parametrize("refine", ["full", "fp8"])
@pytest.mark.parametrize("kind", ["pq", "ivfpq"])
def test_search_through_the_refine_stage(kind, refine):
    """search(q, k, candidates=R) = rerank(q, the first R ids of an identically built index without refine, k); with R >= N
    it is the float64 ranking of the exactly-summable corpus, planted ties to the lower id."""
    c, kw, q, d = _first_stage(kind)
    Q, N, k, R = len(q), len(d), 10, 64
    queries = _queries(c)
    for mode in ("f32", "bf16"):
        bare = _index(c, mode, **kw)
        index = _index(c, mode, refine=refine, **kw)
        E, size = d.shape[1], {"f32": 4, "bf16": 2}[mode]
        assert index.nbytes - bare.nbytes == N * (E * size if refine == "full" else E + 4)
        assert torch.equal(index.pq_codes, bare.pq_codes) and index.representations.dtype == DT[mode]
        assert np.array_equal(index.refine_vectors.float().cpu().numpy(), d), "the corpus survives both refine stores exactly"
        if refine == "fp8":
            codes, scale = rr.quantize(d)
            assert np.array_equal(index.refine_codes.cpu().numpy(), codes) and np.array_equal(_bits(index.refine_scales), _bits(scale))
        else:
            assert index.refine_codes is None and index.refine_scales is None
        probes = (None,) if kind == "pq" else (None, 3, 12)
        lossy = 0
        for nprobe in probes:
            pk = {} if nprobe is None else dict(nprobe=nprobe)
            first = bare.search(queries, R, **pk)
            got = _np(index.search(queries, k, candidates=R, **pk))
            _same(got, _np(index.rerank(queries, first[1], k)), f"{kind} {refine} {mode} nprobe={nprobe}: search against rerank by hand")
            want = sr.topk_merge(rr.rerank(q, d, first[1].cpu().numpy()), first[1].cpu().numpy(), k)
            _same(got, want, f"{kind} {refine} {mode} nprobe={nprobe}: against the reference over the first stage's ids")
            lossy += int((_np(bare.search(queries, k, **pk))[1] != got[1]).sum())
        assert lossy > 0, "the first stage alone already agrees with the refine stage: the case shows nothing"
        # the default R = min(4 k, 1024), and the index's own `candidates`
        own = _index(c, mode, refine=refine, candidates=40, **kw)
        _same(_np(index.search(queries, k)), _np(own.search(queries, k)), "R defaults to 4 k")
        # R >= N: every document is re-scored, the result is float64's
        exact = rr.exact(q, d)
        every = _np(index.search(queries, N, candidates=1024))
        _same(every, sr.topk(exact.astype(np.float32), N), f"{kind} {refine} {mode}: R >= N against float64")
        for lo, hi in ((11, 400), (3, 650)):
            for b in range(Q):
                at = {int(i): n for n, i in enumerate(every[1][b])}
                assert every[0][b][at[lo]] == every[0][b][at[hi]] and at[lo] < at[hi], \
                    f"query {b}: the tie ({lo}, {hi}) must come back lower id first"
        with pytest.raises(ValueError, match="<= candidates <= 1024"):
            index.search(queries, k, candidates=k - 1)
        with pytest.raises(ValueError, match="candidates belongs to the search"):
            bare.search(queries, k, candidates=R)


@pytest.mark.parametrize("mode", ["f32", "bf16"])
def test_no_change_without_refine(mode):
    """An index built without `refine` on the planted corpora: the references the PQ and IVF-PQ tests hold it to."""
    from polus_amd.ir.search import IVFPQCodec, PQCodec
    p = pc.planted()
    c = pc.as_search_case(p["q"], p["docs"])
    exact = rr.exact(p["q"], p["docs"]).astype(np.float32)
    index = _index(c, mode, storage="pq", codec=PQCodec(p["cb"]))
    assert index.refine is None and index._refine is None and index.nbytes == len(p["docs"]) * p["cb"].shape[0]
    assert set(index._store.bufs) == {"reps"}
    for k in pc.KS:
        _same(_np(index.search(_queries(c), k)), sr.topk(exact, k), f"PQ {mode} k={k}")
    p = ic.planted()
    c = pc.as_search_case(p["q"], p["docs"])
    exact = rr.exact(p["q"], p["docs"]).astype(np.float32)
    index = _index(c, mode, storage="ivfpq", codec=IVFPQCodec(p["cent"], p["cb"]))
    assert set(index._store.bufs) == {"reps", "coarse"}
    for k in ic.KS:
        got = _np(index.search(_queries(c), k))
        _same(got, sr.topk(exact, k), f"IVF-PQ {mode} k={k}")
        _same(_np(index.search(_queries(c), k, nprobe=len(p["cent"]))), got, f"IVF-PQ {mode} k={k} nprobe = K")
    with pytest.raises(ValueError, match=r"\[CLS\]"):
        index.rerank(_queries(c), [[0]] * len(p["q"]), 1)


def test_two_stage_search_behind_a_lexical_first_stage():
    from polus_amd.ir.lexical import BM25Index
    from polus_amd.ir.search import CorpusIndex, TwoStageSearch
    from polus_amd.ir.training import InBatchDotScores
    case = dict(seed=3, Q=16, N=300, Lq=8, Ld=24, E=32, V=4096)
    c = token_case(**case)
    N = case["N"]
    docs = batches(c["d_ids"], c["d_mask"], [N // 2, N - N // 2])
    first = BM25Index(case["V"], strip=(0, 0))
    second = CorpusIndex(TableModel(c["table"], torch.bfloat16, False), InBatchDotScores(), refine="full")
    two = TwoStageSearch(first, second, candidates=50)
    assert torch.cat([two.add(b) for b in docs]).cpu().tolist() == list(range(N)) and len(two) == N
    queries = _queries(c)
    got = _np(two.search(queries, 10))
    proposed = first.search(queries, 50)[1]
    _same(got, _np(second.rerank(queries, proposed, 10)), "two stages by hand")
    table = _rounded(c["table"], "bf16")
    q, d = table[c["q_ids"][:, 0]], table[c["d_ids"][:, 0]]              # a [CLS] vector is its first token's row
    host = proposed.cpu().numpy()
    _same(got, sr.topk_merge(rr.rerank(q, d, host), host, 10), "against the reference over BM25's candidates")
    assert (host >= 0).sum() > 10 * case["Q"], "BM25 proposed candidates"
    bare = CorpusIndex(TableModel(c["table"], torch.bfloat16, False), InBatchDotScores())
    for b in docs:
        bare.add(b)
    with pytest.raises(ValueError, match=r"\[CLS\]"):
        TwoStageSearch(first, bare, candidates=50).search(queries, 10)
