"""The residual-compressed token index on the device: polus_residual_compress / polus_residual_decompress byte for byte
and bit for bit against tests/residual_ref.py; polus_maxsim_rerank_res bit for bit polus_maxsim_rerank over the
device-decoded corpus; exact integers against float64 (independent of the bf16 kernels); the MaxSim tolerance against
float64; CorpusIndex(storage="residual"), fit_codec and TwoStageSearch."""
import numpy as np
import pytest
import torch

from tests import maxsim_ref, residual_ref as ref
from tests.maxsim_cases import TOL
from tests.rerank_cases import CS, INT_MAX, MASKS, SHAPES, WAVE_SHAPES, candidates, docs_per_wave, make_case, present, wave_candidates
from tests.residual_cases import (CODEC_SHAPES, INT_SHAPES, K_EDGES, MODES, NBITS, codec_case, corpus_codes, gaussian_case,
                                  gaussian_codec, integer_case)
from tests.search_cases import TableModel, batches, token_case
from tests.util import assert_close, dev, rounded

pytestmark = pytest.mark.gpu
DT = {"f32": torch.float32, "bf16": torch.bfloat16}
GUARD = 64
K_RERANK = 16
_CASES = {}


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _f32(t):
    torch.cuda.synchronize()
    return t.float().cpu().numpy()


# ---------------------------------------------------------------- codec
def _compress(c, nbits, mode):
    """Device compress of a codec_case into a guarded buffer; returns (packed bytes, guard intact)."""
    from polus_amd import ops
    rows, E = c["x"].shape
    nb = E * nbits // 8
    xd = dev(c["x"], DT[mode])
    assert np.array_equal(_f32(xd), c["x"], equal_nan=True)                  # the planted values reach the device as they are
    buf = torch.full((rows * nb + GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
    ops.residual_compress(xd, dev(c["codes"]), dev(c["centroids"], DT[mode]), dev(c["cutoffs"]), nbits, buf[:rows * nb].view(rows, nb))
    torch.cuda.synchronize()
    got = buf.cpu().numpy()
    return got[:rows * nb].reshape(rows, nb), bool((got[rows * nb:] == 0xA5).all())


def _decompress(codes, packed, centroids, weights, nbits, mode):
    from polus_amd import ops
    rows, E = len(codes), centroids.shape[1]
    buf = torch.full((rows * E + GUARD,), 3.0, dtype=DT[mode], device="cuda")
    ops.residual_decompress(dev(codes), dev(packed), dev(centroids, DT[mode]), dev(weights), nbits, buf[:rows * E].view(rows, E))
    y = _f32(buf)
    return y[:rows * E].reshape(rows, E), bool((y[rows * E:] == 3.0).all())


def _check_codec(c, nbits, mode, what):
    with np.errstate(invalid="ignore"):
        want = ref.compress(c["x"], c["codes"], c["centroids"], c["cutoffs"], nbits)
    got, guard = _compress(c, nbits, mode)
    bad = np.argwhere(got != want)
    assert len(bad) == 0, f"{what}: {len(bad)} bytes differ, the first at {bad[0].tolist()}: {got[tuple(bad[0])]:#x} for {want[tuple(bad[0])]:#x}"
    assert guard, f"{what}: compress wrote guard bytes"
    absent = (c["codes"].view(np.uint16) >= c["K"])
    assert (got[absent] == 0).all() and (len(c["x"]) < 3 or absent.sum() == 2)
    # decode: the reference's bytes and bytes of every value
    r = np.random.Generator(np.random.PCG64(len(c["x"]) + nbits))
    for packed in (want, r.integers(0, 256, size=want.shape).astype(np.uint8)):
        y, guard = _decompress(c["codes"], packed, c["centroids"], c["weights"], nbits, mode)
        wanted = ref.decompress(c["codes"], packed, c["centroids"], c["weights"], nbits, mode)
        bad = np.argwhere(_bits(y) != _bits(wanted))
        assert len(bad) == 0, f"{what}: {len(bad)} decoded elements differ, the first at {bad[0].tolist()}"
        assert guard, f"{what}: decompress wrote guard elements"
        assert (_bits(y[absent]) == 0).all()


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("nbits", NBITS)
@pytest.mark.parametrize("rows,E", CODEC_SHAPES)
def test_codec_is_the_reference_byte_for_byte(rows, E, nbits, mode):
    c = codec_case(rows, E, nbits, mode)
    valid = rows - 2 if rows >= 3 else rows
    assert len(c["planted"]) == min(3 * ((1 << nbits) - 1) + 3, valid * E)
    _check_codec(c, nbits, mode, f"({rows}, {E}) nbits={nbits} {mode}")


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("K", K_EDGES)
def test_codec_at_the_limits_of_K(K, mode):
    for nbits in NBITS:
        c = codec_case(5, 32, nbits, mode, K=K)
        assert c["codes"].view(np.uint16)[0] == K - 1 and len(c["centroids"]) == K
        _check_codec(c, nbits, mode, f"K={K} nbits={nbits} {mode}")


# ---------------------------------------------------------------- rerank, bitwise
def _case(shape, masks, mode, nbits):
    """Device tensors of a case (tests/residual_cases.gaussian_case: the Gaussian queries and corpus of
    tests/rerank_cases.make_case, codes given by the test, >= K exactly where the mask is 0) and the corpus as the
    device decodes it.  Built once and shared (nothing writes to them)."""
    key = (shape, masks, mode, nbits)
    if key not in _CASES:
        from polus_amd import ops
        Q, N, Lq, Ld, E = shape
        q, qm, dm, codes, packed, cent, w = gaussian_case(shape, masks, K_RERANK, nbits, mode)
        if dm is not None:
            assert ((codes.view(np.uint16) >= K_RERANK) == (dm == 0)).all() and (packed[dm == 0] == 0).all()
        assert len(np.unique(packed)) > 1 or N * Ld * E <= 32
        t = dict(q=dev(q, DT[mode]), qm=None if qm is None else dev(qm), dm=None if dm is None else dev(dm), codes=dev(codes),
                 packed=dev(packed), cent=dev(cent, DT[mode]), w=dev(w), nbits=nbits, N=N)
        t["deq"] = torch.empty((N, Ld, E), dtype=DT[mode], device="cuda")
        ops.residual_decompress(t["codes"], t["packed"], t["cent"], t["w"], nbits, t["deq"])
        t["host"] = (rounded(q, DT[mode]), qm, dm)
        _CASES[key] = t
    return _CASES[key]


def _rerank(t, cand, ldc=None, lds=None, plain=False):
    """One polus_maxsim_rerank_res call (plain: polus_maxsim_rerank over the decoded corpus); cand and score sit in the
    leading C columns of [Q, ldc] / [Q, lds] buffers.  Returns the whole score buffer (columns past C hold -7.25)."""
    from polus_amd import ops
    Q, C = cand.shape
    cbuf = torch.full((Q, ldc or C), 0, dtype=torch.int32, device="cuda")
    cbuf[:, :C] = torch.as_tensor(cand)
    sbuf = torch.full((Q, lds or C), -7.25, dtype=torch.float32, device="cuda")
    if plain:
        ops.maxsim_rerank(t["q"], t["deq"], t["qm"], t["dm"], cbuf[:, :C], sbuf[:, :C])
    else:
        ops.maxsim_rerank_res(t["q"], t["codes"], t["packed"], t["cent"], t["w"], t["nbits"], t["qm"], t["dm"], cbuf[:, :C], sbuf[:, :C])
    torch.cuda.synchronize()
    return sbuf.cpu().numpy()


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("nbits", NBITS)
@pytest.mark.parametrize("si", range(len(SHAPES)), ids=[str(s) for s in SHAPES])
def test_rerank_equals_rerank_of_the_decoded_corpus_bitwise(si, nbits, mode):
    Q, N = SHAPES[si][:2]
    for masks in MASKS:
        t = _case(SHAPES[si], masks, mode, nbits)
        for C in CS:
            cand = candidates(Q, N, C)
            if C >= 7:
                assert (cand == N).any() and (cand == INT_MAX).any() and (cand[:, 2] == -1).all() and (cand[:, -1] == -1).all()
            ok = present(cand, N)
            want = _rerank(t, cand, plain=True)
            got = _rerank(t, cand, lds=C + 5)
            what = f"{SHAPES[si]} {masks} nbits={nbits} {mode} C={C}"
            assert np.isneginf(got[:, :C][~ok]).all() and np.isfinite(got[:, :C][ok]).all(), f"{what}: absent entries"
            bad = np.argwhere(_bits(got[:, :C]) != _bits(want))
            assert len(bad) == 0, f"{what}: {len(bad)} entries differ, the first at (row, column) {bad[0].tolist()}"
            assert C < 7 or np.abs(got[:, :C][ok]).max() > 0
            assert (got[:, C:] == -7.25).all(), f"{what}: columns past C were written"
            strided = _rerank(t, cand, ldc=C + 3)
            assert np.array_equal(_bits(strided), _bits(want)), f"{what}: strided candidates"
        if masks == "ragged" and N > 1:
            cand = np.full((Q, 1), N - 1, np.int32)
            assert (_rerank(t, cand) == 0.0).all(), "the empty document scores 0"


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("nbits", NBITS)
@pytest.mark.parametrize("wi", (0, len(WAVE_SHAPES) - 1), ids=[str(WAVE_SHAPES[w][0]) for w in (0, len(WAVE_SHAPES) - 1)])
def test_rerank_several_documents_per_wave_bitwise(wi, nbits, mode):
    """2, 4 and 8 documents per wave with partial last blocks: the next document's codes, bits and centroid rows are
    loaded behind the current document's last tile."""
    shape, cs = WAVE_SHAPES[wi]
    Q, N = shape[:2]
    for masks in MASKS:
        t = _case(shape, masks, mode, nbits)
        for C, dpw in cs:
            assert docs_per_wave(Q, C) == dpw and C % (4 * dpw)
            cand = wave_candidates(Q, N, C)
            want = _rerank(t, cand, plain=True)
            got = _rerank(t, cand, lds=C + 5)
            what = f"{shape} {masks} nbits={nbits} {mode} C={C} ({dpw} documents per wave)"
            assert np.isneginf(got[:, :C][~present(cand, N)]).all()
            bad = np.argwhere(_bits(got[:, :C]) != _bits(want))
            assert len(bad) == 0, f"{what}: {len(bad)} entries differ, the first at (row, column) {bad[0].tolist()}"
            assert (got[:, C:] == -7.25).all(), f"{what}: columns past C were written"


@pytest.mark.parametrize("mode", MODES)
def test_a_valid_token_without_a_centroid_counts_as_a_row_of_zeros(mode):
    """No mask, and codes >= K among the tokens: the decoder writes zeros for them and the rerank kernel scores them as
    zeros, reading nothing of the centroids for them."""
    from polus_amd import ops
    shape = (3, 40, 5, 17, 32)
    Q, N, Lq, Ld, E = shape
    q, _, _, _ = make_case(shape, "none")
    _, _, _, holes = make_case(shape, "ragged")
    for nbits in NBITS:
        codes, packed = corpus_codes(shape, holes, K_RERANK, nbits)
        cent, w = gaussian_codec(K_RERANK, E, nbits, mode)
        t = dict(q=dev(q, DT[mode]), qm=None, dm=None, codes=dev(codes), packed=dev(packed), cent=dev(cent, DT[mode]), w=dev(w), nbits=nbits)
        t["deq"] = torch.empty((N, Ld, E), dtype=DT[mode], device="cuda")
        ops.residual_decompress(t["codes"], t["packed"], t["cent"], t["w"], nbits, t["deq"])
        assert (_f32(t["deq"])[holes == 0] == 0).all() and (_f32(t["deq"])[N - 1] == 0).all()
        cand = candidates(Q, N, 70)
        assert np.array_equal(_bits(_rerank(t, cand)), _bits(_rerank(t, cand, plain=True))), nbits


# ---------------------------------------------------------------- exact integers, against float64
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("nbits", NBITS)
@pytest.mark.parametrize("shape", INT_SHAPES, ids=[str(s) for s in INT_SHAPES])
def test_integer_scores_are_exact(shape, nbits, mode):
    """Independent of the bf16 / f32 MaxSim kernels: small integers, so every product and sum is exact and float64 on
    the reference's decoded corpus must be met with equality.  A bucket taken from another bit position, a weight of
    another bucket or a centroid row of another token changes a score."""
    from polus_amd import ops
    Q, N, Lq, Ld, E = shape
    q, cent, w, codes, packed, qm, dm = integer_case(shape, nbits)
    d = ref.decompress(codes.reshape(-1), packed.reshape(N * Ld, -1), cent, w, nbits, mode).reshape(N, Ld, E)
    want = maxsim_ref.maxsim_fwd(q, d, qm, dm)[0].astype(np.float32)
    assert np.abs(want).max() > 100 and (want[:, N - 1] == 0).all()
    r = np.random.Generator(np.random.PCG64(91))
    cand = np.stack([r.permutation(N) for _ in range(Q)]).astype(np.int32)
    out = torch.full((Q, N), np.nan, dtype=torch.float32, device="cuda")
    ops.maxsim_rerank_res(dev(q, DT[mode]), dev(codes), dev(packed), dev(cent, DT[mode]), dev(w), nbits, dev(qm), dev(dm), dev(cand), out)
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert np.array_equal(got, want[np.arange(Q)[:, None], cand]), f"{int((got != want[np.arange(Q)[:, None], cand]).sum())} of {Q * N} differ"


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("si", range(len(SHAPES)), ids=[str(s) for s in SHAPES])
def test_scores_against_float64(si, mode):
    """The reference runs on the corpus as the device decodes it; the tolerance is the MaxSim kernels' own
    (tests/maxsim_cases.TOL), no new one."""
    Q, N = SHAPES[si][:2]
    for masks in MASKS:
        for nbits in NBITS:
            t = _case(SHAPES[si], masks, mode, nbits)
            q, qm, dm = t["host"]
            full = maxsim_ref.maxsim_fwd(q, _f32(t["deq"]).astype(np.float64), qm, dm)[0]
            cand = candidates(Q, N, 70)
            ok = present(cand, N)
            got = _rerank(t, cand)
            assert np.isneginf(got[~ok]).all()
            assert_close(got[ok], full[np.arange(Q)[:, None], np.where(ok, cand, 0)][ok], TOL[mode]["score"],
                         f"{SHAPES[si]} {masks} nbits={nbits} {mode} rerank")


# ---------------------------------------------------------------- CorpusIndex(storage="residual")
CASE = dict(seed=3, Q=16, N=300, Lq=8, Ld=24, E=64, V=4096)                 # the case of tests/test_fp8_index_gpu.py
K_INDEX = 64


def _index(case, mode, tokens, **kw):
    from polus_amd.ir.search import CorpusIndex
    from polus_amd.ir.training import InBatchDotScores, MaxSimScores
    index = CorpusIndex(TableModel(case["table"], DT[mode], tokens), MaxSimScores(normalize=True) if tokens else InBatchDotScores(), **kw)
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


def _plain_with_codec(c, mode, nbits=2):
    """A plain index with K_INDEX centroids (rows of the table, normalised on the host) and its fit_codec(nbits)."""
    plain = _index(c, mode, True)
    rows = c["table"][:K_INDEX].astype(np.float64)
    plain.set_centroids((rows / np.linalg.norm(rows, axis=1, keepdims=True)).astype(np.float32))
    return plain, plain.fit_codec(nbits)


@pytest.mark.parametrize("mode", MODES)
def test_residual_corpus_index_is_a_plain_index_of_the_decoded_corpus(mode):
    from polus_amd.ir.search import CorpusIndex
    c = token_case(**CASE)
    Q, N, Ld, E, nbits = CASE["Q"], CASE["N"], CASE["Ld"], CASE["E"], 2
    queries = {"input_ids": c["q_ids"], "attention_mask": c["q_mask"]}
    plain, codec = _plain_with_codec(c, mode)
    # the codec's tables are the reference's quantiles of the sampled residuals, bit for bit
    x = _f32(plain.representations).reshape(N * Ld, E)
    codes = plain.centroid_codes.cpu().numpy().reshape(-1)
    cent = _f32(plain.centroids)
    slots = ref.sample_slots(0, N, Ld, c["d_mask"], 1 << 16)
    assert 0 < len(slots) < N * Ld and (codes.view(np.uint16)[slots] < K_INDEX).all()
    want_cut, want_w = ref.fit_tables(x[slots] - cent[codes.view(np.uint16)[slots].astype(np.int64)], nbits)
    assert np.array_equal(_bits(codec.cutoffs.numpy()), _bits(want_cut)) and np.array_equal(_bits(codec.weights.numpy()), _bits(want_w))
    assert codec.nbits == nbits and torch.equal(codec.centroids, plain.centroids) and (np.diff(want_cut) > 0).all()

    res = _index(c, mode, True, storage="residual", codec=codec)
    assert len(res) == N and res.residuals.dtype == torch.uint8 and tuple(res.residuals.shape) == (N, Ld, E * nbits // 8)
    assert res.codes is None and res.scales is None and plain.residuals is None
    assert res.nbytes == N * Ld * (E * nbits // 8 + 2 + 4)
    assert torch.equal(res.mask, plain.mask) and torch.equal(res.centroids, plain.centroids)
    # the same codes as the plain index, across the two adds and the growth between them; the reference's bytes
    assert torch.equal(res.centroid_codes, plain.centroid_codes)
    want_p = ref.compress(x, codes, cent, want_cut, nbits)
    assert np.array_equal(res.residuals.cpu().numpy().reshape(N * Ld, -1), want_p)
    assert (want_p[c["d_mask"].reshape(-1) == 0] == 0).all() and want_p.any()
    reps = res.representations
    assert reps.dtype == DT[mode] and reps.data_ptr() != res.representations.data_ptr()           # a copy, each time
    assert np.array_equal(_bits(_f32(reps).reshape(N * Ld, E)), _bits(ref.decompress(codes, want_p, cent, want_w, nbits, mode)))
    plain.representations.copy_(reps)
    r = np.random.Generator(np.random.PCG64(77))
    cand = np.stack([r.permutation(N) for _ in range(Q)])
    big = 256 << 20
    for k in (10, 100):
        want = _np(plain.search(queries, k))
        assert (want[1] >= 0).all()
        for scratch in (100 * Ld * E * DT[mode].itemsize, big):              # 100 decoded documents per chunk, or all
            res.scratch_bytes = scratch
            assert len(res.chunks(Q, decode=True)) == (3 if scratch < big else 1)
            _same(_np(res.search(queries, k)), want, f"{mode} k={k} scratch={scratch} search")
        for scratch in (4 * Q * 100, big):                                    # 100 candidate columns per chunk, or all
            res.scratch_bytes = scratch
            assert len(res.rerank_chunks(Q, N)) == len(res.chunks(Q)) == (3 if scratch < big else 1)
            _same(_np(res.rerank(queries, cand, k)), want, f"{mode} k={k} scratch={scratch} host candidates")
            _same(_np(res.rerank(queries, torch.as_tensor(cand.astype(np.int32)).cuda(), k)), want, f"{mode} k={k} device candidates")
            _same(_np(res.search_pruned(queries, k, 120)), _np(plain.search_pruned(queries, k, 120)), f"{mode} k={k} scratch={scratch} pruned")
        _same(_np(res.search_pruned(queries, k, 1024)), want, f"{mode} k={k} pruned with candidates >= N")
    with pytest.raises(ValueError, match="candidates must lie in"):
        res.rerank(queries, np.array([[0, N]] * Q), 10)
    with pytest.raises(ValueError, match="takes its centroids from its codec"):
        res.set_centroids(cent)
    with pytest.raises(ValueError, match="takes its centroids from its codec"):
        res.fit_centroids(K_INDEX)
    res.clear()
    assert len(res) == 0 and res.nbytes == 0 and res.residuals is None and res.representations is None and res.codec is codec
    docs = {"input_ids": c["d_ids"][:4], "attention_mask": c["d_mask"][:4]}
    assert res.add(docs).cpu().tolist() == [0, 1, 2, 3] and np.array_equal(res.residuals.cpu().numpy().reshape(4 * Ld, -1), want_p[:4 * Ld])


def test_codec_from_an_fp8_index_and_refusals():
    from polus_amd.ir.search import CorpusIndex
    from polus_amd.ir.training import InBatchDotScores, MaxSimScores
    c = token_case(**CASE)
    N, Ld, E = CASE["N"], CASE["Ld"], CASE["E"]
    docs = {"input_ids": c["d_ids"][:8], "attention_mask": c["d_mask"][:8]}
    fp8 = _index(c, "bf16", True, storage="fp8")
    with pytest.raises(ValueError, match="fit_codec needs centroids"):
        fp8.fit_codec(2)
    fp8.fit_centroids(K_INDEX)
    with pytest.raises(ValueError, match="nbits must be 1, 2 or 4"):
        fp8.fit_codec(3)
    for nbits in (1, 4):
        codec = fp8.fit_codec(nbits, sample=2000, seed=5)
        x = _f32(fp8.representations).reshape(N * Ld, E)
        codes = fp8.centroid_codes.cpu().numpy().reshape(-1).view(np.uint16).astype(np.int64)
        slots = ref.sample_slots(5, N, Ld, c["d_mask"], 2000)
        cut, w = ref.fit_tables(x[slots] - _f32(fp8.centroids)[codes[slots]], nbits)
        assert np.array_equal(_bits(codec.cutoffs.numpy()), _bits(cut)) and np.array_equal(_bits(codec.weights.numpy()), _bits(w))
    with pytest.raises(ValueError, match="needs a codec"):
        CorpusIndex(TableModel(c["table"], torch.float32, True), MaxSimScores(normalize=True), storage="residual")
    with pytest.raises(ValueError, match="scorer that normalises"):
        CorpusIndex(TableModel(c["table"], torch.float32, True), MaxSimScores(normalize=False), storage="residual", codec=codec)
    index = CorpusIndex(TableModel(c["table"], torch.float32, False), MaxSimScores(normalize=True), storage="residual", codec=codec)
    with pytest.raises(ValueError, match="token representations only"):
        index.add(docs)
    assert len(index) == 0
    with pytest.raises(ValueError, match="^storage must be None or 'fp8'"):
        CorpusIndex(TableModel(c["table"], torch.float32, True), MaxSimScores(), storage="int4")


@pytest.mark.parametrize("mode", MODES)
def test_two_stage_search_with_a_residual_second_stage(mode):
    from polus_amd.ir.search import TwoStageSearch
    c = token_case(**CASE)
    N = CASE["N"]
    queries = {"input_ids": c["q_ids"], "attention_mask": c["q_mask"]}
    plain, codec = _plain_with_codec(c, mode, nbits=4)
    first, second = _index(c, mode, False), _index(c, mode, True, storage="residual", codec=codec)
    plain.representations.copy_(second.representations)
    two = TwoStageSearch(first, second, 50)
    assert len(two) == N
    got = _np(two.search(queries, 10))
    _same(got, _np(second.rerank(queries, first.search(queries, 50)[1], 10)), f"{mode} two stages by hand")
    _same(got, _np(TwoStageSearch(first, plain, 50).search(queries, 10)), f"{mode} a plain second stage of the decoded corpus")
    assert (got[1] >= 0).all() and (np.diff(got[0], axis=1) <= 0).all()
    _same(_np(TwoStageSearch(first, second, N).search(queries, 10)), _np(second.search(queries, 10)), f"{mode} candidates = N")
    docs = {"input_ids": c["d_ids"][:4], "attention_mask": c["d_mask"][:4]}
    assert two.add(docs).cpu().tolist() == list(range(N, N + 4)) and len(second) == N + 4
