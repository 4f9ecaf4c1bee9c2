"""CPU: the FP8 token index's quantiser rule (tests/fp8_ref.py) has the properties the device kernels rely on, the
bitwise comparisons of tests/test_fp8_index_gpu.py see each of the mistakes a quantiser or an FP8 scoring kernel can
make, the new entry points validate on the host, and what quantisation does to a ranking (reported)."""
import ctypes

import numpy as np
import pytest
import torch

from tests import fp8_ref, maxsim_ref, search_ref as sr
from tests.fp8_cases import INT_SHAPES, MIDPOINTS_RNE, PLANTS, QUANT_SHAPES, integer_case, quant_rows
from tests.rerank_cases import make_case
from tests.search_cases import TOKEN_CASE, token_case


def _bf16(a):
    return torch.as_tensor(np.ascontiguousarray(a, np.float32)).to(torch.bfloat16).float().numpy()


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.mark.parametrize("mode", ["f32", "bf16"])
@pytest.mark.parametrize("rows,E", QUANT_SHAPES)
def test_reference_quantiser_properties(rows, E, mode):
    x, where = quant_rows(rows, E, mode)
    assert np.array_equal(_bf16(x), x) or mode == "f32"
    codes, scale, e = fp8_ref.quantize(x)
    amax = np.abs(x).max(-1)
    top = np.abs(fp8_ref.decode(codes)).max(-1)
    nz = amax > 0
    # nothing saturates and nothing is wasted: the scaled maximum of a non-zero row lies in (224, 448]
    scaled = amax[nz].astype(np.float64) / scale[nz]
    assert (scaled > 224).all() and (scaled <= 448).all(), (scaled.min(), scaled.max())
    assert (top[nz] >= 224).all() and (top <= 448).all()
    assert np.array_equal(scale, np.ldexp(np.float32(1), e)) and (np.frexp(scale)[0] == 0.5).all()       # powers of two
    if "zero" in where:
        z = where["zero"]
        assert e[z] == 0 and scale[z] == 1.0 and not (codes[z] & 0x7f).any()
    if "m>0.875" in where:
        a, b = where["m=0.875"], where["m>0.875"]
        assert e[b] == e[a] + 1 and top[a] == 448 and 224 <= top[b] <= 240
    if "ties" in where:
        t = where["ties"]
        want = np.resize(MIDPOINTS_RNE, E)
        want[E - 1] = -448
        assert e[t] == 0 and np.array_equal(_bits(fp8_ref.decode(codes[t])), _bits(want))
    # a dequantised value has at most 4 significant bits: bf16 holds it, and quantising it again changes nothing
    y = fp8_ref.dequantize(codes, scale)
    assert np.array_equal(_bits(_bf16(y)), _bits(y))
    c2, s2, _ = fp8_ref.quantize(y)
    assert np.array_equal(fp8_ref.dequantize(c2, s2), y)
    # scaling a row by a power of two moves the exponent and nothing else
    for sh in (-20, 20):
        c3, s3, e3 = fp8_ref.quantize(np.ldexp(x, sh))
        assert np.array_equal(c3, codes) and np.array_equal(e3[nz], e[nz] + sh) and (e3[~nz] == 0).all()
    assert sorted(where) == sorted(PLANTS[:min(rows, len(PLANTS))])


def test_values_that_are_codes_times_a_power_of_two_round_trip():
    r = np.random.Generator(np.random.PCG64(9100))
    codes = r.integers(0, 256, size=(200, 64)).astype(np.uint8)
    codes[(codes & 0x7f) == 0x7f] = 0x38                       # no NaN
    codes[:, 0] = np.where(r.random(200) < 0.5, 0x7e, 0xfe)    # +-448 in every row: the row's scale is forced
    e = r.integers(-60, 60, size=200)
    x = np.ldexp(fp8_ref.decode(codes), e[:, None])
    c, s, e2 = fp8_ref.quantize(x)
    assert np.array_equal(e2, e) and np.array_equal(fp8_ref.dequantize(c, s), x)
    assert np.array_equal(c & 0x7f, codes & 0x7f) and np.array_equal((c >> 7)[x != 0], (codes >> 7)[x != 0])
    # the clamp: rows below 2^-91 keep e = -100 and lose precision instead of overflowing the scale's inverse
    tiny = np.ldexp(np.float32(1.5), np.array([[-95], [-105], [-120]])).astype(np.float32) * np.ones((1, 8), np.float32)
    ct, st, et = fp8_ref.quantize(tiny)
    assert (et == -100).all() and np.array_equal(fp8_ref.dequantize(ct, st)[:2], tiny[:2])


@pytest.mark.parametrize("mode", ["f32", "bf16"])
def test_quantiser_mistakes_change_the_bytes_the_gpu_test_compares(mode):
    """tests/test_fp8_index_gpu.py compares codes and scales byte for byte with fp8_ref.quantize.  An exponent off by
    one either way and truncation instead of round-to-nearest-even each change those bytes, on every shape."""
    for rows, E in QUANT_SHAPES:
        x, where = quant_rows(rows, E, mode)
        codes, scale, _ = fp8_ref.quantize(x)
        for mutant in ("exponent+1", "exponent-1"):
            c, s, _ = fp8_ref.quantize(x, mutant)
            nz = np.abs(x).max(-1) > 0
            assert (s[nz] != scale[nz]).all() and (c[nz] != codes[nz]).any(-1).all(), (rows, E, mutant)
        c, s, _ = fp8_ref.quantize(x, "truncate")
        assert np.array_equal(s, scale) and (c != codes).any(), (rows, E)
        if "ties" in where:
            assert (c[where["ties"]] != codes[where["ties"]]).sum() >= E // 3


@pytest.mark.parametrize("mode", ["f32", "bf16"])
def test_scoring_mistakes_change_the_scores_the_gpu_test_compares(mode):
    """A dropped scale changes the bits of every non-empty pair's score in the bitwise comparison (scores over the
    dequantised corpus); a scale taken from the neighbouring token or an operand read in another order changes the
    exact-integer scores."""
    q, d, qm, dm = make_case((3, 40, 5, 17, 32), "ragged")
    if mode == "bf16":
        q, d = _bf16(q), _bf16(d)
    codes, scale, _ = fp8_ref.quantize(d)
    good = maxsim_ref.maxsim_fwd(q, fp8_ref.dequantize(codes, scale), qm, dm)[0].astype(np.float32)
    bad = maxsim_ref.maxsim_fwd(q, fp8_ref.decode(codes), qm, dm)[0].astype(np.float32)
    live = good != 0
    assert live.sum() >= good.size // 2 and (_bits(bad)[live] != _bits(good)[live]).all()
    for shape in INT_SHAPES:
        q, v, s, qm, dm = integer_case(shape)
        want = maxsim_ref.maxsim_fwd(q, v * s[..., None], qm, dm)[0]
        assert np.array_equal(want, np.round(want)) and np.abs(want).max() < 2 ** 24
        shifted = maxsim_ref.maxsim_fwd(q, v * np.roll(s, 1, axis=1)[..., None], qm, dm)[0]
        swapped = maxsim_ref.maxsim_fwd(q, (v * s[..., None]).reshape(v.shape[:2] + (-1, 2))[..., ::-1].reshape(v.shape), qm, dm)[0]
        for other in (shifted, swapped):
            assert (other != want).mean() > 0.5


def test_argument_validation_happens_on_the_host():
    from polus_amd import build
    build.build(verbose=False)
    from polus_amd import _lib, ops
    lib = _lib.load()
    p, odd = ctypes.c_void_p(4096), ctypes.c_void_p(4096 + 8)

    def refused(rc, text):
        assert rc != 0 and text in lib.polus_last_error(), (rc, lib.polus_last_error())
    for fn in (lib.polus_fp8_quantize_rows, lib.polus_fp8_dequantize_rows):
        refused(fn(7, p, p, p, 4, 32, None), b"unknown dtype")
        refused(fn(0, p, p, p, 0, 32, None), b"rows >= 1")
        refused(fn(0, p, p, p, 4, 30, None), b"multiple of 4")
        refused(fn(0, p, p, p, 4, 260, None), b"multiple of 4")
        refused(fn(1, p, None, p, 4, 32, None), b"null pointer")
    refused(lib.polus_fp8_quantize_rows(0, p, odd, p, 4, 32, None), b"16-byte aligned")
    refused(lib.polus_fp8_dequantize_rows(0, odd, p, p, 4, 32, None), b"16-byte aligned")
    scores = lambda dtype=1, Q=p, codes=p, scale=p, score=p, lds=8, B=2, N=8, Lq=4, Ld=6, E=64: lib.polus_maxsim_scores_fp8(
        dtype, Q, codes, scale, None, None, score, lds, B, N, Lq, Ld, E, None)
    rerank = lambda dtype=1, Q=p, codes=p, scale=p, cand=p, ldc=8, score=p, lds=8, B=2, C=8, N=8, Lq=4, Ld=6, E=64: \
        lib.polus_maxsim_rerank_fp8(dtype, Q, codes, scale, None, None, cand, ldc, score, lds, B, C, N, Lq, Ld, E, None)
    for call in (scores, rerank):
        refused(call(dtype=2), b"unknown dtype")
        refused(call(E=48), b"multiple of 32")
        refused(call(E=288), b"multiple of 32")
        refused(call(Lq=513), b"Lq")
        refused(call(Ld=0), b"Ld")
        refused(call(B=65536), b"B <= 65535")
        refused(call(scale=None), b"null pointer")
        refused(call(codes=odd), b"16-byte aligned")
        refused(call(lds=7), b"lds must be >=")
    refused(scores(N=65536, lds=1 << 20), b"N <= 65535")
    refused(rerank(C=0), b"C <= 65535")
    refused(rerank(N=0), b"N")
    refused(rerank(ldc=7), b"ldc must be >=")
    refused(rerank(cand=None), b"null pointer")
    # the ops refuse host tensors, and the index refuses an unknown storage before it touches anything
    x = torch.zeros(4, 32)
    with pytest.raises(_lib.PolusHipError):
        ops.fp8_quantize(x, torch.zeros(4, 32, dtype=torch.uint8), torch.zeros(4))
    with pytest.raises(_lib.PolusHipError):
        ops.maxsim_scores_fp8(torch.zeros(1, 4, 32), torch.zeros(2, 4, 32, dtype=torch.uint8), torch.zeros(2, 4), None, None,
                              torch.zeros(1, 2))
    from polus_amd.ir.search import CorpusIndex, RetrievalValidationCallback
    with pytest.raises(ValueError, match="storage must be None or 'fp8'"):
        CorpusIndex(None, None, storage="int4")
    index = CorpusIndex(None, None, storage="fp8")
    assert index.storage == "fp8" and len(index) == 0 and index.nbytes == 0 and index.codes is None and index.scales is None
    assert CorpusIndex(None, None).storage is None
    assert RetrievalValidationCallback([], [], 5, storage="fp8").storage == "fp8"
    import polus.ir.search as alias
    assert alias.CorpusIndex is CorpusIndex


def test_ranking_fidelity_reported():
    """How far FP8 storage moves a ranking, on random tables (NOT a trained model): the overlap of the top-10 ids between
    float64 MaxSim over unit-norm token vectors and over their quantised form.  Reported; only positivity is asserted."""
    c = token_case(**TOKEN_CASE)
    tab = maxsim_ref.l2norm_fwd(c["table"])[0].astype(np.float32)
    codes, scale, _ = fp8_ref.quantize(tab)
    deq = fp8_ref.dequantize(codes, scale)
    rel = np.linalg.norm(deq.astype(np.float64) - tab, axis=-1) / np.linalg.norm(tab, axis=-1)
    full = sr.maxsim_scores(tab[c["q_ids"]], tab[c["d_ids"]], c["q_mask"], c["d_mask"])
    quant = sr.maxsim_scores(tab[c["q_ids"]], deq[c["d_ids"]], c["q_mask"], c["d_mask"])
    top = lambda s: np.argsort(-s, axis=1, kind="stable")[:, :10]
    overlap = np.mean([len(set(a.tolist()) & set(b.tolist())) / 10 for a, b in zip(top(full), top(quant))])
    first = np.mean(top(full)[:, 0] == top(quant)[:, 0])
    print(f"FP8 index, random unit-norm tables (Q {TOKEN_CASE['Q']}, N {TOKEN_CASE['N']}, Lq {TOKEN_CASE['Lq']}, "
          f"Ld {TOKEN_CASE['Ld']}, E {TOKEN_CASE['E']}): top-10 overlap {overlap:.3f}, same first document {first:.3f}, "
          f"worst |score change| {np.abs(quant - full).max():.4f} of max|score| {np.abs(full).max():.3f}, "
          f"per-row relative L2 error mean {rel.mean():.4f} worst {rel.max():.4f}")
    assert overlap > 0
