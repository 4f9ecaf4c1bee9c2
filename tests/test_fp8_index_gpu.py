"""The FP8 token index on the device: polus_fp8_quantize_rows / polus_fp8_dequantize_rows byte for byte against
tests/fp8_ref.py; polus_maxsim_scores_fp8 bit for bit polus_maxsim_scores over the dequantised corpus, and
polus_maxsim_rerank_fp8 bit for bit those scores; exact integers against float64 (independent of the bf16 kernels);
the MaxSim tolerance against float64; CorpusIndex(storage="fp8"), TwoStageSearch and RetrievalValidationCallback."""
import types

import numpy as np
import pytest
import torch

from tests import fp8_ref, maxsim_ref, search_ref as sr
from tests.fp8_cases import INT_SHAPES, PLANTS, QUANT_SHAPES, integer_case, quant_rows
from tests.maxsim_cases import TOL
from tests.rerank_cases import (CS, INT_MAX, MASKS, SHAPES, WAVE_SHAPES, candidates, docs_per_wave, make_case, present,
                                wave_candidates, wave_transitions)
from tests.search_cases import TableModel, batches, token_case
from tests.util import assert_close, dev, rounded

pytestmark = pytest.mark.gpu
DT = {"f32": torch.float32, "bf16": torch.bfloat16}
GUARD = 64
_CASES = {}


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _f32(t):
    torch.cuda.synchronize()
    return t.float().cpu().numpy()


# ---------------------------------------------------------------- quantiser
@pytest.mark.parametrize("mode", ["f32", "bf16"])
@pytest.mark.parametrize("rows,E", QUANT_SHAPES)
def test_quantiser_is_the_reference_byte_for_byte(rows, E, mode):
    from polus_amd import ops
    x, where = quant_rows(rows, E, mode)
    assert sorted(where) == sorted(PLANTS[:min(rows, len(PLANTS))])
    xd = dev(x, DT[mode])
    assert np.array_equal(_f32(xd), x)                                       # the planted values reach the device as they are
    cbuf = torch.full((rows * E + GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
    sbuf = torch.full((rows + GUARD,), 777.0, dtype=torch.float32, device="cuda")
    codes, scale = cbuf[:rows * E].view(rows, E), sbuf[:rows]
    ops.fp8_quantize(xd, codes, scale)
    torch.cuda.synchronize()
    want_c, want_s, _ = fp8_ref.quantize(x)
    got_c, got_s = codes.cpu().numpy(), scale.cpu().numpy()
    bad = np.argwhere(got_c != want_c)
    assert len(bad) == 0, f"{len(bad)} codes differ, the first at {bad[0].tolist()}: {got_c[tuple(bad[0])]:#x} for {want_c[tuple(bad[0])]:#x}"
    assert np.array_equal(_bits(got_s), _bits(want_s)), np.argwhere(got_s != want_s)[:4].tolist()
    assert (cbuf[rows * E:] == 0xA5).all() and (sbuf[rows:] == 777.0).all(), "guard elements were written"
    # the inverse map is exact, into either dtype
    for out in DT.values():
        ybuf = torch.full((rows * E + GUARD,), 3.0, dtype=out, device="cuda")
        ops.fp8_dequantize(codes, scale, ybuf[:rows * E].view(rows, E))
        y = _f32(ybuf)
        assert np.array_equal(_bits(y[:rows * E].reshape(rows, E)), _bits(fp8_ref.dequantize(want_c, want_s))), out
        assert (y[rows * E:] == 3.0).all(), "guard elements were written"


# ---------------------------------------------------------------- scores and rerank, bitwise
def _case(shape, masks, mode):
    """Device tensors of a case, its corpus quantised on the device, and the exhaustive scores of both kernels over
    the whole corpus (polus_maxsim_scores_fp8 on the codes, polus_maxsim_scores on the dequantised corpus), each in a
    buffer of row stride N + 5.  Computed once and shared by the tests below (nothing writes to them)."""
    key = (shape, masks, mode)
    if key not in _CASES:
        from polus_amd import ops
        q, d, qm, dm = make_case(shape, masks)
        Q, N = shape[:2]
        t = dict(q=dev(q, DT[mode]), qm=None if qm is None else dev(qm), dm=None if dm is None else dev(dm))
        dd = dev(d, DT[mode])
        t["codes"] = torch.empty(dd.shape, dtype=torch.uint8, device="cuda")
        t["scale"] = torch.empty(dd.shape[:2], dtype=torch.float32, device="cuda")
        ops.fp8_quantize(dd, t["codes"], t["scale"])
        deq = torch.empty_like(dd)
        ops.fp8_dequantize(t["codes"], t["scale"], deq)
        fp8 = torch.full((Q, N + 5), -7.25, dtype=torch.float32, device="cuda")
        plain = torch.full((Q, N + 5), -7.25, dtype=torch.float32, device="cuda")
        ops.maxsim_scores_fp8(t["q"], t["codes"], t["scale"], t["qm"], t["dm"], fp8[:, :N])
        ops.maxsim_scores(t["q"], deq, t["qm"], t["dm"], plain[:, :N])
        torch.cuda.synchronize()
        t["fp8"], t["plain"] = fp8.cpu().numpy(), plain.cpu().numpy()
        t["full"] = t["fp8"][:, :N]
        t["host"] = (rounded(q, DT[mode]), _f32(deq).astype(np.float64), qm, dm)
        t["host_codes"] = (t["codes"].cpu().numpy(), t["scale"].cpu().numpy(), rounded(d, DT[mode]))
        _CASES[key] = t
    return _CASES[key]


@pytest.mark.parametrize("mode", ["f32", "bf16"])
@pytest.mark.parametrize("si", range(len(SHAPES)), ids=[str(s) for s in SHAPES])
def test_scores_equal_the_scores_of_the_dequantised_corpus_bitwise(si, mode):
    Q, N = SHAPES[si][:2]
    for masks in MASKS:
        t = _case(SHAPES[si], masks, mode)
        what = f"{SHAPES[si]} {masks} {mode}"
        codes, scale, d = t["host_codes"]
        want_c, want_s, _ = fp8_ref.quantize(d.astype(np.float32))
        assert np.array_equal(codes, want_c) and np.array_equal(scale, want_s), f"{what}: the quantised corpus"
        bad = np.argwhere(_bits(t["fp8"][:, :N]) != _bits(t["plain"][:, :N]))
        assert len(bad) == 0, f"{what}: {len(bad)} of {Q * N} scores differ, the first at (query, document) {bad[0].tolist()}"
        assert np.isfinite(t["fp8"][:, :N]).all() and (N == 1 or np.abs(t["fp8"][:, :N]).max() > 0)
        assert (t["fp8"][:, N:] == -7.25).all(), f"{what}: columns past N were written"
        if masks == "ragged" and N > 1:
            assert (t["fp8"][:, N - 1] == 0.0).all() and (t["fp8"][Q - 1, :N] == 0.0).all()


def _rerank(t, cand, ldc=None, lds=None):
    """One polus_maxsim_rerank_fp8 call; cand and score sit in the leading C columns of [Q, ldc] / [Q, lds] buffers.
    Returns the whole score buffer (columns past C hold -7.25)."""
    from polus_amd import ops
    Q, C = cand.shape
    cbuf = torch.full((Q, ldc or C), 0, dtype=torch.int32, device="cuda")
    cbuf[:, :C] = torch.as_tensor(cand)
    sbuf = torch.full((Q, lds or C), -7.25, dtype=torch.float32, device="cuda")
    ops.maxsim_rerank_fp8(t["q"], t["codes"], t["scale"], t["qm"], t["dm"], cbuf[:, :C], sbuf[:, :C])
    torch.cuda.synchronize()
    return sbuf.cpu().numpy()


def _wanted(full, cand, N):
    ok = present(cand, N)
    return np.where(ok, full[np.arange(len(cand))[:, None], np.where(ok, cand, 0)], -np.inf).astype(np.float32)


@pytest.mark.parametrize("mode", ["f32", "bf16"])
@pytest.mark.parametrize("si", range(len(SHAPES)), ids=[str(s) for s in SHAPES])
def test_rerank_equals_exhaustive_fp8_scores_bitwise(si, mode):
    Q, N = SHAPES[si][:2]
    for masks in MASKS:
        t = _case(SHAPES[si], masks, mode)
        full = t["full"]
        for C in CS:
            cand = candidates(Q, N, C)
            if C >= 7:
                assert (cand == N).any() and (cand == INT_MAX).any() and (cand[:, 2] == -1).all() and (cand[:, -1] == -1).all()
            want = _wanted(full, cand, N)
            assert np.isneginf(want[~present(cand, N)]).all()
            got = _rerank(t, cand, lds=C + 5)
            what = f"{SHAPES[si]} {masks} {mode} C={C}"
            assert np.array_equal(_bits(got[:, :C]), _bits(want)), f"{what}: {int((_bits(got[:, :C]) != _bits(want)).sum())} entries differ"
            assert (got[:, C:] == -7.25).all(), f"{what}: columns past C were written"
            strided = _rerank(t, cand, ldc=C + 3)
            assert np.array_equal(_bits(strided), _bits(want)), f"{what}: strided candidates"


@pytest.mark.parametrize("mode", ["f32", "bf16"])
@pytest.mark.parametrize("wi", range(len(WAVE_SHAPES)), ids=[str(w[0]) for w in WAVE_SHAPES])
def test_rerank_several_documents_per_wave_bitwise(wi, mode):
    """2, 4 and 8 documents per wave on both query routes, with every transition between present, empty and absent
    documents inside a wave: the next document's tile AND scale are loaded behind the current one's last."""
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
            want = _wanted(full, cand, N)
            got = _rerank(t, cand, lds=C + 5)
            what = f"{shape} {masks} {mode} C={C} ({dpw} documents per wave)"
            bad = np.argwhere(_bits(got[:, :C]) != _bits(want))
            assert len(bad) == 0, f"{what}: {len(bad)} entries differ, the first at (row, column) {bad[0].tolist()}"
            assert (got[:, C:] == -7.25).all(), f"{what}: columns past C were written"


# ---------------------------------------------------------------- exact integers, against float64
@pytest.mark.parametrize("mode", ["f32", "bf16"])
@pytest.mark.parametrize("shape", INT_SHAPES, ids=[str(s) for s in INT_SHAPES])
def test_integer_scores_are_exact(shape, mode):
    """Independent of the bf16 / f32 MaxSim kernels: small integers, power-of-two scales, asymmetric documents.  A
    code byte taken in another order, or a token's accumulator row multiplied by another token's scale, changes a score
    (tests/test_fp8_index_cpu.py shows that for this data)."""
    from polus_amd import ops
    Q, N, Lq, Ld, E = shape
    q, v, s, qm, dm = integer_case(shape)
    codes = fp8_ref.encode(v)
    assert np.array_equal(fp8_ref.decode(codes), v)
    want = maxsim_ref.maxsim_fwd(q, v * s[..., None], qm, dm)[0].astype(np.float32)
    assert np.abs(want).max() > 100 and (want[:, N - 1] == 0).all()
    qd, cd, sd, qmd, dmd = dev(q, DT[mode]), dev(codes), dev(s), dev(qm), dev(dm)
    got = torch.full((Q, N), np.nan, dtype=torch.float32, device="cuda")
    ops.maxsim_scores_fp8(qd, cd, sd, qmd, dmd, got)
    torch.cuda.synchronize()
    assert np.array_equal(got.cpu().numpy(), want), f"scores: {int((got.cpu().numpy() != want).sum())} of {Q * N} differ"
    r = np.random.Generator(np.random.PCG64(91))
    cand = np.stack([r.permutation(N) for _ in range(Q)]).astype(np.int32)
    out = torch.full((Q, N), np.nan, dtype=torch.float32, device="cuda")
    ops.maxsim_rerank_fp8(qd, cd, sd, qmd, dmd, dev(cand), out)
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy(), want[np.arange(Q)[:, None], cand]), "rerank"


@pytest.mark.parametrize("mode", ["f32", "bf16"])
@pytest.mark.parametrize("si", range(len(SHAPES)), ids=[str(s) for s in SHAPES])
def test_scores_against_float64(si, mode):
    """The reference runs on the inputs as the device sees them (the dequantised corpus); the tolerance is the MaxSim
    kernels' own (tests/maxsim_cases.TOL), no new one."""
    Q, N = SHAPES[si][:2]
    for masks in MASKS:
        t = _case(SHAPES[si], masks, mode)
        q, deq, qm, dm = t["host"]
        ref = maxsim_ref.maxsim_fwd(q, deq, qm, dm)[0]
        assert_close(t["fp8"][:, :N], ref, TOL[mode]["score"], f"{SHAPES[si]} {masks} {mode} scores")
        cand = candidates(Q, N, 70)
        ok = present(cand, N)
        got = _rerank(t, cand)
        assert np.isneginf(got[~ok]).all()
        assert_close(got[ok], ref[np.arange(Q)[:, None], np.where(ok, cand, 0)][ok], TOL[mode]["score"], f"{SHAPES[si]} {masks} {mode} rerank")


# ---------------------------------------------------------------- CorpusIndex(storage="fp8")
CASE = dict(seed=3, Q=16, N=300, Lq=8, Ld=24, E=64, V=4096)                 # the case of tests/test_rerank_gpu.py


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


def _same(got, want, what):
    assert np.array_equal(got[1], want[1]), f"{what}: ids differ in {int((got[1] != want[1]).sum())} places"
    assert np.array_equal(_bits(got[0]), _bits(want[0])), f"{what}: values differ"


@pytest.mark.parametrize("mode", ["f32", "bf16"])
def test_fp8_corpus_index_is_a_plain_index_of_the_dequantised_corpus(mode):
    c = token_case(**CASE)
    Q, N, Ld, E = CASE["Q"], CASE["N"], CASE["Ld"], CASE["E"]
    queries = {"input_ids": c["q_ids"], "attention_mask": c["q_mask"]}
    fp8, plain = _index(c, mode, True, storage="fp8"), _index(c, mode, True)
    assert len(fp8) == N and fp8.codes.dtype == torch.uint8 and tuple(fp8.codes.shape) == (N, Ld, E)
    assert fp8.scales.dtype == torch.float32 and tuple(fp8.scales.shape) == (N, Ld) and plain.codes is None and plain.scales is None
    assert fp8.nbytes == N * Ld * (E + 8) and plain.nbytes == N * Ld * (DT[mode].itemsize * E + 4)
    assert torch.equal(fp8.mask, plain.mask)
    # the stored codes are the reference quantiser's of the table rows, across the two adds and the growth between them
    tab = rounded(c["table"], DT[mode]).astype(np.float32)
    want_c, want_s, _ = fp8_ref.quantize(tab[c["d_ids"]])
    assert np.array_equal(fp8.codes.cpu().numpy(), want_c) and np.array_equal(fp8.scales.cpu().numpy(), want_s)
    reps = fp8.representations
    assert reps.dtype == DT[mode] and reps.data_ptr() != fp8.representations.data_ptr()           # a copy, each time
    assert np.array_equal(_f32(reps), fp8_ref.dequantize(want_c, want_s))
    plain.representations.copy_(reps)
    r = np.random.Generator(np.random.PCG64(77))
    cand = np.stack([r.permutation(N) for _ in range(Q)])
    for k in (10, 100):
        want = _np(plain.search(queries, k))
        assert (want[1] >= 0).all()
        for scratch in (4 * Q * 100, 256 << 20):
            fp8.scratch_bytes = scratch
            assert len(fp8.chunks(Q)) == len(fp8.rerank_chunks(Q, N)) == (3 if scratch < 1 << 20 else 1)
            _same(_np(fp8.search(queries, k)), want, f"{mode} k={k} scratch={scratch} search")
            _same(_np(fp8.rerank(queries, cand, k)), want, f"{mode} k={k} scratch={scratch} host candidates")
            _same(_np(fp8.rerank(queries, torch.as_tensor(cand.astype(np.int32)).cuda(), k)), want, f"{mode} k={k} device candidates")
        fp8.scratch_bytes = 256 << 20
    with pytest.raises(ValueError, match="candidates must lie in"):
        fp8.rerank(queries, np.array([[0, N]] * Q), 10)
    fp8.clear()
    assert len(fp8) == 0 and fp8.nbytes == 0 and fp8.codes is None and fp8.representations is None


def test_fp8_storage_refusals():
    from polus_amd.ir.search import CorpusIndex
    from polus_amd.ir.training import InBatchDotScores, MaxSimScores
    c = token_case(**CASE)
    docs = {"input_ids": c["d_ids"][:8], "attention_mask": c["d_mask"][:8]}
    index = CorpusIndex(TableModel(c["table"], torch.float32, False), InBatchDotScores(), storage="fp8")
    with pytest.raises(ValueError, match="token representations only"):
        index.add(docs)
    assert len(index) == 0
    with pytest.raises(ValueError, match="storage must be None or 'fp8'"):
        CorpusIndex(TableModel(c["table"], torch.float32, True), MaxSimScores(), storage="int4")


@pytest.mark.parametrize("mode", ["f32", "bf16"])
def test_two_stage_search_with_an_fp8_second_stage(mode):
    from polus_amd.ir.search import TwoStageSearch
    c = token_case(**CASE)
    N = CASE["N"]
    queries = {"input_ids": c["q_ids"], "attention_mask": c["q_mask"]}
    first, second = _index(c, mode, False), _index(c, mode, True, storage="fp8")
    two = TwoStageSearch(first, second, 50)
    assert len(two) == N
    got = _np(two.search(queries, 10))
    _same(got, _np(second.rerank(queries, first.search(queries, 50)[1], 10)), f"{mode} two stages by hand")
    assert (got[1] >= 0).all() and (np.diff(got[0], axis=1) <= 0).all()
    _same(_np(TwoStageSearch(first, second, N).search(queries, 10)), _np(second.search(queries, 10)), f"{mode} candidates = N")
    docs = {"input_ids": c["d_ids"][:4], "attention_mask": c["d_mask"][:4]}
    assert two.add(docs).cpu().tolist() == list(range(N, N + 4)) and len(second) == N + 4


def test_retrieval_validation_callback_with_fp8_storage():
    """One validated epoch through the callback protocol, the trainer stood in for by its four attributes the callback
    reads: the metrics equal those of ranking with an FP8 index by hand, and the callback's index was an FP8 one."""
    from polus_amd.callbacks import CallbackCoordinator
    from polus_amd.ir.metrics import MRRAtK, NDCGAtK, RecallAtK
    from polus_amd.ir.search import RetrievalValidationCallback
    from polus_amd.ir.training import MaxSimScores
    c = token_case(**CASE)
    N, K = CASE["N"], 5
    model, scorer = TableModel(c["table"], torch.bfloat16, True), MaxSimScores(normalize=True)
    corpus = batches(c["d_ids"], c["d_mask"], [N // 2, N - N // 2])
    r = np.random.Generator(np.random.PCG64(12))
    relevant = [set(r.integers(0, N, size=100).tolist()) for _ in range(CASE["Q"])]
    val = [({"input_ids": c["q_ids"][a:a + 8], "attention_mask": c["q_mask"][a:a + 8]}, relevant[a:a + 8]) for a in (0, 8)]
    metrics = [RecallAtK(K), MRRAtK(K), NDCGAtK(K)]
    trainer = types.SimpleNamespace(model=model, compute_scores=scorer, post_process_logits=None, metrics=metrics)
    cb = RetrievalValidationCallback(corpus, val, K, name="val", storage="fp8")
    seen = []
    rank = cb.custom_inference_f
    cb.custom_inference_f = lambda m, sample: (seen.append((cb.index.storage, cb.index.codes.dtype, len(cb.index))), rank(m, sample))[1]
    coordinator = CallbackCoordinator([cb], trainer, 1, 1)
    coordinator.on_train_begin()
    coordinator.on_epoch_end(0)
    torch.cuda.synchronize()
    assert seen == [("fp8", torch.uint8, N)] * 2 and len(cb.index) == 0
    res = coordinator.shared_dict["validation"]["val"]
    from polus_amd.ir.search import CorpusIndex
    index = CorpusIndex(model, scorer, storage="fp8")
    for b in corpus:
        index.add(b)
    ranked = np.concatenate([index.search(q, K)[1].cpu().numpy() for q, _ in val], 0)
    want = {f"Recall@{K}": sr.recall_at_k(ranked, relevant, K), f"MRR@{K}": sr.mrr_at_k(ranked, relevant, K),
            f"nDCG@{K}": sr.ndcg_at_k(ranked, relevant, K)}
    assert sorted(res) == sorted(want)
    for name, v in want.items():
        assert len(res[name]) == 1 and abs(res[name][0] - v) < 1e-12, (name, res[name], v)
    assert res[f"Recall@{K}"][0] > 0
