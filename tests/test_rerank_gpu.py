"""Two-stage search on the device: polus_maxsim_rerank (bit for bit the scores polus_maxsim_scores gives each pair, -inf
for absent candidates, strides respected; within the MaxSim tolerance of float64), polus_topk_merge_ids (exact against
tests/search_ref.topk_merge over ties, special values, dropped ids, strides, misaligned rows and chunkings),
CorpusIndex.rerank (a permutation of the whole corpus reproduces search) and TwoStageSearch."""
import numpy as np
import pytest
import torch

from tests import maxsim_ref, search_ref as sr
from tests.maxsim_cases import TOL
from tests.rerank_cases import (CS, INT_MAX, MASKS, SHAPES, WAVE_SHAPES, candidates, docs_per_wave, make_case, present,
                                wave_candidates, wave_transitions)
from tests.search_cases import TableModel, batches, maxsim_tol, token_case
from tests.util import assert_close, dev, rounded

pytestmark = pytest.mark.gpu
DT = {"f32": torch.float32, "bf16": torch.bfloat16}
GUARD = 64
_CASES = {}


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _case(shape, masks, mode):
    """Device tensors of a case and the exhaustive scores of polus_maxsim_scores over its whole corpus, computed once
    and shared by the tests below (nothing writes to them)."""
    key = (shape, masks, mode)
    if key not in _CASES:
        from polus_amd import ops
        q, d, qm, dm = make_case(shape, masks)
        t = dict(q=dev(q, DT[mode]), d=dev(d, DT[mode]), qm=None if qm is None else dev(qm),
                 dm=None if dm is None else dev(dm), host=(q, d, qm, dm))
        full = torch.full((q.shape[0], d.shape[0]), float("nan"), dtype=torch.float32, device="cuda")
        ops.maxsim_scores(t["q"], t["d"], t["qm"], t["dm"], full)
        torch.cuda.synchronize()
        t["full"] = full.cpu().numpy()
        _CASES[key] = t
    return _CASES[key]


def _rerank(t, cand, ldc=None, lds=None):
    """One polus_maxsim_rerank call; cand and score sit in the leading C columns of [Q, ldc] / [Q, lds] buffers.
    Returns the whole score buffer (columns past C hold -7.25)."""
    from polus_amd import ops
    Q, C = cand.shape
    cbuf = torch.full((Q, ldc or C), 0, dtype=torch.int32, device="cuda")       # id 0 behind C: read = scored = seen
    cbuf[:, :C] = torch.as_tensor(cand)
    sbuf = torch.full((Q, lds or C), -7.25, dtype=torch.float32, device="cuda")
    ops.maxsim_rerank(t["q"], t["d"], t["qm"], t["dm"], cbuf[:, :C], sbuf[:, :C])
    torch.cuda.synchronize()
    return sbuf.cpu().numpy()


@pytest.mark.parametrize("mode", ["f32", "bf16"])
@pytest.mark.parametrize("si", range(len(SHAPES)), ids=[str(s) for s in SHAPES])
def test_rerank_equals_exhaustive_scores_bitwise(si, mode):
    Q, N = SHAPES[si][:2]
    for masks in MASKS:
        t = _case(SHAPES[si], masks, mode)
        full = t["full"]
        if masks == "ragged" and N > 1:
            assert (full[:, N - 1] == 0.0).all()                           # the empty document is in every list below
        for C in CS:
            cand = candidates(Q, N, C)
            ok = present(cand, N)
            if C >= 7:
                assert (cand == N).any() and (cand == INT_MAX).any() and (cand[:, 2] == -1).all() and (cand[:, -1] == -1).all()
                assert (cand[:, 0] == N - 1).all() and len(set(cand[:, 1].tolist())) == 1
            want = np.where(ok, full[np.arange(Q)[:, None], np.where(ok, cand, 0)], -np.inf).astype(np.float32)
            got = _rerank(t, cand, lds=C + 5)
            what = f"{SHAPES[si]} {masks} {mode} C={C}"
            assert np.array_equal(_bits(got[:, :C]), _bits(want)), f"{what}: {int((_bits(got[:, :C]) != _bits(want)).sum())} entries differ"
            assert (got[:, C:] == -7.25).all(), f"{what}: columns past C were written"
            strided = _rerank(t, cand, ldc=C + 3)
            assert np.array_equal(_bits(strided), _bits(want)), f"{what}: strided candidates"


@pytest.mark.parametrize("mode", ["f32", "bf16"])
@pytest.mark.parametrize("wi", range(len(WAVE_SHAPES)), ids=[str(w[0]) for w in WAVE_SHAPES])
def test_rerank_several_documents_per_wave_bitwise(wi, mode):
    """The document loop with a wave taking 2, 4 and 8 documents in turn: the next candidate's id and mask read a
    document ahead, the first tile of the next document loaded behind the current one's last, absent and empty
    documents between present ones, a last block whose waves hold fewer documents than the others, on both routes
    (query in registers, rounds over the query).  Every entry has the bits of the exhaustive scores."""
    shape, cs = WAVE_SHAPES[wi]
    Q, N = shape[:2]
    for masks in MASKS:
        t = _case(shape, masks, mode)
        full = t["full"]
        for C, dpw in cs:
            assert docs_per_wave(Q, C) == dpw and C % (4 * dpw)
            cand = wave_candidates(Q, N, C)
            if masks == "ragged":
                assert (full[:, N - 1] == 0.0).all()
                kinds = ("present", "empty", "absent")
                assert wave_transitions(cand, N, dpw, N - 1) == {(a, b) for a in kinds for b in kinds}
            ok = present(cand, N)
            want = np.where(ok, full[np.arange(Q)[:, None], np.where(ok, cand, 0)], -np.inf).astype(np.float32)
            got = _rerank(t, cand, lds=C + 5)
            what = f"{shape} {masks} {mode} C={C} ({dpw} documents per wave)"
            bad = np.argwhere(_bits(got[:, :C]) != _bits(want))
            assert len(bad) == 0, f"{what}: {len(bad)} entries differ, the first at (row, column) {bad[0].tolist()}"
            assert (got[:, C:] == -7.25).all(), f"{what}: columns past C were written"


@pytest.mark.parametrize("mode", ["f32", "bf16"])
@pytest.mark.parametrize("si", range(len(SHAPES)), ids=[str(s) for s in SHAPES])
def test_rerank_against_float64(si, mode):
    """The reference runs on the inputs as the device sees them; the tolerance is the MaxSim kernels' own
    (tests/maxsim_cases.TOL, which tests/test_maxsim_cpu.py holds 5x below one wrong decision)."""
    Q, N = SHAPES[si][:2]
    for masks in MASKS:
        t = _case(SHAPES[si], masks, mode)
        q, d, qm, dm = t["host"]
        ref = maxsim_ref.maxsim_fwd(rounded(q, DT[mode]), rounded(d, DT[mode]), qm, dm)[0]
        cand = candidates(Q, N, 70)
        ok = present(cand, N)
        got = _rerank(t, cand)
        want = ref[np.arange(Q)[:, None], np.where(ok, cand, 0)]
        assert np.isneginf(got[~ok]).all()
        assert_close(got[ok], want[ok], TOL[mode]["score"], f"{SHAPES[si]} {masks} {mode}")


# ---------------------------------------------------------------- polus_topk_merge_ids
def _strided(a, ld, col0, fill, dtype):
    rows, n = a.shape
    buf = torch.full((rows * ld + 8,), fill, dtype=dtype, device="cuda")
    view = buf[col0:col0 + rows * ld].view(rows, ld)[:, :n]
    view.copy_(torch.as_tensor(a))
    return view


def _merge_ids(scores, ids, k, state=None):
    """One merge over host arrays.  Scores and ids sit in buffers of different odd row strides and column offsets, so
    their rows start at different 4-byte phases of a 16-byte line; the state carries GUARD elements that must stay."""
    from polus_amd import ops
    rows, n = scores.shape
    s = _strided(scores, n + 7, 1, 3e38, torch.float32)
    i = _strided(ids, n + 5, 3, 5, torch.int32)
    assert s.data_ptr() % 16 and i.data_ptr() % 16 and (s.data_ptr() - i.data_ptr()) % 16
    tv = torch.full((rows * k + GUARD,), 777.0, dtype=torch.float32, device="cuda")
    ti = torch.full((rows * k + GUARD,), 424242, dtype=torch.int32, device="cuda")
    if state is not None:
        tv[:rows * k] = torch.as_tensor(state[0]).reshape(-1)
        ti[:rows * k] = torch.as_tensor(state[1]).reshape(-1)
    ops.topk_merge(s, tv[:rows * k].view(rows, k), ti[:rows * k].view(rows, k), init=state is None, ids=i)
    torch.cuda.synchronize()
    assert (tv[rows * k:] == 777.0).all() and (ti[rows * k:] == 424242).all(), "guard elements were written"
    return tv[:rows * k].view(rows, k).cpu().numpy(), ti[:rows * k].view(rows, k).cpu().numpy()


def _same(got, want, what):
    assert np.array_equal(got[1], want[1]), f"{what}: ids differ in {int((got[1] != want[1]).sum())} places"
    assert np.array_equal(_bits(got[0]), _bits(want[0])), f"{what}: values differ"


def _chunkings(n):
    cuts = [[0, n], [0, 1, n], sorted({0, n // 3, 2 * n // 3, n})]
    return [[(a, b) for a, b in zip(c[:-1], c[1:]) if b > a] for c in cuts]


@pytest.mark.parametrize("n", [1, 5, 1023, 1024, 1025, 5000])
def test_topk_merge_ids_matches_reference_exactly(n):
    from polus_amd import ops
    r = np.random.Generator(np.random.PCG64(50 + n))
    rows = 3
    s = r.integers(0, 6, size=(rows, n)).astype(np.float32)                # integer-valued: heavy ties
    u = r.random((rows, n))
    for lo, hi, v in ((0.00, 0.04, np.nan), (0.04, 0.08, -np.inf), (0.08, 0.10, np.inf), (0.10, 0.14, -0.0)):
        s[(u >= lo) & (u < hi)] = v
    ids = np.stack([r.permutation(n) * 3 + row for row in range(rows)]).astype(np.int64)
    ids[0, r.integers(0, n)] = INT_MAX                                     # the largest id there is
    ids[r.random((rows, n)) < 0.1] = -1                                    # dropped whatever their score
    if n > 1:
        ids[1, 0], s[1, 0] = -1, np.inf
    ids = ids.astype(np.int32)
    live = np.where(ids < 0, -np.inf, s).astype(np.float32)                # the reference does not know negative ids
    for k in (1, 10, 100, 1000):
        want = sr.topk_merge(live, ids, k)
        if n <= 5 and k >= 10:
            assert (want[1][:, n:] == -1).all()                            # k above the number of live columns
        for spans in _chunkings(n):
            for order in (spans, spans[::-1]):
                state = None
                for a, b in order:
                    state = _merge_ids(s[:, a:b], ids[:, a:b], k, state)
                _same(state, want, f"n={n} k={k} chunks={order}")
    # ids = id0 + column: the bits of polus_topk_merge
    id0 = 1000
    for k in (10, 1000):
        got = _merge_ids(s, np.tile(id0 + np.arange(n, dtype=np.int32), (rows, 1)), k)
        tv = torch.empty((rows, k), dtype=torch.float32, device="cuda")
        ti = torch.empty((rows, k), dtype=torch.int32, device="cuda")
        ops.topk_merge(dev(s), tv, ti, id0=id0, init=True)
        _same(got, (tv.cpu().numpy(), ti.cpu().numpy()), f"n={n} k={k} against id0")
    with pytest.raises(AssertionError):
        ops.topk_merge(dev(s), tv, ti, id0=1, init=True, ids=dev(ids))


# ---------------------------------------------------------------- CorpusIndex.rerank, TwoStageSearch
CASE = dict(seed=3, Q=16, N=300, Lq=8, Ld=24, E=64, V=4096)                 # tests/search_cases.TOKEN_CASE, N scaled down


def _index(case, mode, tokens, **kw):
    from polus_amd.ir.search import CorpusIndex
    from polus_amd.ir.training import InBatchDotScores, MaxSimScores
    index = CorpusIndex(TableModel(case["table"], DT[mode], tokens), MaxSimScores(normalize=False) if tokens else InBatchDotScores(), **kw)
    n = len(case["d_ids"])
    for b in batches(case["d_ids"], case["d_mask"], [n // 2, n - n // 2]):
        index.add(b)
    return index


def _np(pair):
    torch.cuda.synchronize()
    return pair[0].cpu().numpy(), pair[1].cpu().numpy()


@pytest.mark.parametrize("mode", ["f32", "bf16"])
def test_corpus_index_rerank_of_every_document_is_search(mode):
    c = token_case(**CASE)
    Q, N = CASE["Q"], CASE["N"]
    queries = {"input_ids": c["q_ids"], "attention_mask": c["q_mask"]}
    r = np.random.Generator(np.random.PCG64(77))
    cand = np.stack([r.permutation(N) for _ in range(Q)])
    index = _index(c, mode, True)
    for k in (10, 100):
        want = _np(index.search(queries, k))
        for scratch in (4 * Q * 100, 256 << 20):
            index.scratch_bytes = scratch
            assert len(index.rerank_chunks(Q, N)) == (3 if scratch < 1 << 20 else 1)
            _same(_np(index.rerank(queries, cand, k)), want, f"{mode} k={k} scratch={scratch} host candidates")
            _same(_np(index.rerank(queries, torch.as_tensor(cand.astype(np.int32)).cuda(), k)), want, f"{mode} k={k} device candidates")
        index.scratch_bytes = 256 << 20
    val, idx = _np(index.rerank(queries, np.full((Q, 9), -1), 10))
    assert (idx == -1).all() and np.isneginf(val).all()
    # a device tensor is not checked: ids past the corpus are absent
    wild = torch.as_tensor(np.concatenate([cand[:, :20], np.full((Q, 2), N), np.full((Q, 1), INT_MAX)], 1).astype(np.int32)).cuda()
    _same(_np(index.rerank(queries, wild, 10)), _np(index.rerank(queries, cand[:, :20], 10)), "ids past the corpus")
    # a wider device id is not narrowed (2^32 + 5 would become document 5)
    with pytest.raises(ValueError, match="must be int32"):
        index.rerank(queries, torch.as_tensor(cand).cuda(), 10)
    for bad in (N, -2):
        with pytest.raises(ValueError, match="candidates must lie in"):
            index.rerank(queries, np.array([[0, bad]] * Q), 10)
    with pytest.raises(ValueError, match=r"\[CLS\]"):
        _index(c, mode, False).rerank(queries, cand, 10)


@pytest.mark.parametrize("mode", ["f32", "bf16"])
def test_two_stage_search(mode):
    from polus_amd.ir.search import TwoStageSearch
    c = token_case(**CASE)
    Q, N = CASE["Q"], CASE["N"]
    queries = {"input_ids": c["q_ids"], "attention_mask": c["q_mask"]}
    first, second = _index(c, mode, False), _index(c, mode, True)
    two = TwoStageSearch(first, second, candidates=50)
    assert len(two) == N
    got = _np(two.search(queries, 10))
    _same(got, _np(second.rerank(queries, first.search(queries, 50)[1], 10)), f"{mode} two stages by hand")
    tab = rounded(c["table"], DT[mode])
    s64 = sr.maxsim_scores(tab[c["q_ids"]], tab[c["d_ids"]], c["q_mask"], c["d_mask"])
    t = maxsim_tol(mode) * np.abs(s64).max()
    val, idx = got
    assert (idx >= 0).all() and all(len(set(row.tolist())) == 10 for row in idx)
    first_ids = first.search(queries, 50)[1].cpu().numpy()
    assert all(set(row.tolist()) <= set(f.tolist()) for row, f in zip(idx, first_ids))
    worst = np.abs(val.astype(np.float64) - s64[np.arange(Q)[:, None], idx]).max()
    print(f"{mode}: worst |score - float64| = {worst:.3e}, t = {t:.3e}")
    assert worst <= t
    assert (np.diff(val, axis=1) <= 0).all()
    _same(_np(TwoStageSearch(first, second, candidates=N).search(queries, 10)), _np(second.search(queries, 10)),
          f"{mode} candidates = N")
    # the stages must number a batch alike
    docs = {"input_ids": c["d_ids"][:4], "attention_mask": c["d_mask"][:4]}
    assert two.add(docs).cpu().tolist() == list(range(N, N + 4)) and len(first) == len(second) == N + 4
    first.add(docs)
    with pytest.raises(ValueError, match="different ids"):
        two.add(docs)
