"""The residual codec without a GPU: tests/residual_ref.py against a per-element Python loop, every planted mistake
of the reference visible in the bytes or decoded bits of the planted case (so the comparisons of
tests/test_residual_gpu.py would see it), ResidualCodec's validation, the new symbols, and the host-side refusals of the
three entry points."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from tests import residual_ref as ref
from tests.residual_cases import MODES, NBITS, codec_case, codec_tables, integer_case

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("polus_residual_compress", "polus_residual_decompress", "polus_maxsim_rerank_res")


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _bf16(v):
    return torch.tensor([float(v)], dtype=torch.float32).to(torch.bfloat16).float().item()


def _loop_compress(x, codes, centroids, cutoffs, nbits):
    rows, E = x.shape
    out = np.zeros((rows, E * nbits // 8), np.uint8)
    for row in range(rows):
        code = int(codes[row]) & 0xFFFF
        if code >= len(centroids):
            continue
        for k in range(E):
            r = np.float32(x[row, k]) - np.float32(centroids[code, k])
            b = sum(1 for c in cutoffs if r > c)
            out[row, k * nbits // 8] |= b << (nbits * (k % (8 // nbits)))
    return out


def _loop_decompress(codes, packed, centroids, weights, nbits, mode):
    rows, E = len(codes), packed.shape[1] * 8 // nbits
    out = np.zeros((rows, E), np.float32)
    for row in range(rows):
        code = int(codes[row]) & 0xFFFF
        if code >= len(centroids):
            continue
        for k in range(E):
            b = (int(packed[row, k * nbits // 8]) >> (nbits * (k % (8 // nbits)))) & ((1 << nbits) - 1)
            v = np.float32(centroids[code, k]) + np.float32(weights[b])
            out[row, k] = v if mode == "f32" else _bf16(v)
    return out


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("nbits", NBITS)
def test_reference_equals_a_per_element_loop(nbits, mode):
    with np.errstate(invalid="ignore"):
        c = codec_case(5, 32, nbits, mode)
        want = _loop_compress(c["x"], c["codes"], c["centroids"], c["cutoffs"], nbits)
        got = ref.compress(c["x"], c["codes"], c["centroids"], c["cutoffs"], nbits)
    assert np.array_equal(got, want)
    assert (got[3:] == 0).all() and got[:3].any()                             # rows 3 and 4 have no centroid
    assert np.array_equal(ref.unpack(got, nbits), ref.buckets(c["x"], c["codes"], c["centroids"], c["cutoffs"]))
    r = np.random.Generator(np.random.PCG64(5))
    packed = r.integers(0, 256, size=got.shape).astype(np.uint8)
    y = ref.decompress(c["codes"], packed, c["centroids"], c["weights"], nbits, mode)
    assert np.array_equal(_bits(y), _bits(_loop_decompress(c["codes"], packed, c["centroids"], c["weights"], nbits, mode)))
    assert (_bits(y[3:]) == 0).all()


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("nbits", NBITS)
def test_planted_values_land_where_the_rules_say(nbits, mode):
    with np.errstate(invalid="ignore"):
        c = codec_case(5, 32, nbits, mode)
        b = ref.buckets(c["x"], c["codes"], c["centroids"], c["cutoffs"]).reshape(-1)
    n = 1 << nbits
    assert len(c["planted"]) == 3 * (n - 1) + 3
    at = {name: b[p] for p, name in enumerate(c["planted"])}
    for j in range(n - 1):
        assert (at[f"cut{j}-"], at[f"cut{j}"], at[f"cut{j}+"]) == (j, j, j + 1), j    # ON a cutoff: the lower bucket
    assert (at["nan"], at["+inf"], at["-inf"]) == (0, n - 1, 0)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("nbits", NBITS)
@pytest.mark.parametrize("mutant", ref.MUTANTS)
def test_every_planted_mistake_changes_the_planted_case(mutant, nbits, mode):
    """What the GPU tests compare is the packed bytes (compress) and the decoded bits (decompress of given bytes)."""
    with np.errstate(invalid="ignore"):
        c = codec_case(5, 32, nbits, mode)
        good_p = ref.compress(c["x"], c["codes"], c["centroids"], c["cutoffs"], nbits)
        bad_p = ref.compress(c["x"], c["codes"], c["centroids"], c["cutoffs"], nbits, mutate=mutant)
    good_y = ref.decompress(c["codes"], good_p, c["centroids"], c["weights"], nbits, mode)
    bad_y = ref.decompress(c["codes"], good_p, c["centroids"], c["weights"], nbits, mode, mutate=mutant)
    bytes_differ, bits_differ = not np.array_equal(good_p, bad_p), not np.array_equal(_bits(good_y), _bits(bad_y))
    if mutant == "ge":
        assert bytes_differ
    elif mutant in ("weights", "round"):
        assert bits_differ
    else:
        assert bytes_differ and bits_differ                                   # "msb" at 1, 2 and 4 bits alike


def test_integer_case_is_exact_in_every_format():
    for nbits in NBITS:
        q, cent, w, codes, packed, qm, dm = integer_case((3, 40, 5, 17, 32), nbits)
        flat = ref.decompress(codes.reshape(-1), packed.reshape(-1, packed.shape[-1]), cent, w, nbits, "bf16")
        assert np.array_equal(flat, ref.decompress(codes.reshape(-1), packed.reshape(-1, packed.shape[-1]), cent, w, nbits, "f32"))
        assert np.abs(flat).max() <= 11 and (flat == np.round(flat)).all()
        assert ((codes.view(np.uint16) >= 11) == (dm == 0)).all()


def test_codec_validation():
    from polus_amd.ir.search import ResidualCodec
    cent = torch.zeros((5, 64))
    cut, w = codec_tables(2)
    codec = ResidualCodec(cent, cut, w, 2)
    assert codec.nbits == 2 and codec.cutoffs.dtype == torch.float32 and tuple(codec.weights.shape) == (4,)
    assert np.array_equal(codec.cutoffs.numpy(), cut) and np.array_equal(codec.weights.numpy(), w)
    ResidualCodec(cent.numpy(), [0.0], [-1.0, 1.0], 1)                        # arrays and lists; equal cutoffs are allowed
    ResidualCodec(cent, [0.0, 0.0, 0.5], w, 2)
    for bad in (3, 0, 8, "2", None):
        with pytest.raises(ValueError, match="nbits must be 1, 2 or 4"):
            ResidualCodec(cent, cut, w, bad)
    with pytest.raises(ValueError, match="cutoffs must be \\[3\\]"):
        ResidualCodec(cent, cut[:2], w, 2)
    with pytest.raises(ValueError, match="weights must be \\[4\\]"):
        ResidualCodec(cent, cut, codec_tables(4)[1], 2)
    with pytest.raises(ValueError, match="non-decreasing"):
        ResidualCodec(cent, cut[::-1].copy(), w, 2)
    with pytest.raises(ValueError, match="non-decreasing"):
        ResidualCodec(cent, [0.0, np.nan, 1.0], w, 2)
    for shape in ((5, 48), (0, 64), (65536, 32), (5, 288), (64,)):
        with pytest.raises(ValueError, match="centroids must be"):
            ResidualCodec(torch.zeros(shape, dtype=torch.bfloat16), cut, w, 2)


def test_unknown_storage_message_and_codec_pairing():
    from polus_amd.ir.search import CorpusIndex, ResidualCodec
    from polus_amd.ir.training import MaxSimScores
    with pytest.raises(ValueError, match="^storage must be None or 'fp8'"):
        CorpusIndex(None, MaxSimScores(normalize=True), storage="int4")
    with pytest.raises(ValueError, match="needs a codec"):
        CorpusIndex(None, MaxSimScores(normalize=True), storage="residual")
    codec = ResidualCodec(torch.zeros((5, 64)), [0.0], [-1.0, 1.0], 1)
    with pytest.raises(ValueError, match="needs a codec"):
        CorpusIndex(None, MaxSimScores(normalize=True), storage="fp8", codec=codec)
    with pytest.raises(ValueError, match="scorer that normalises"):
        CorpusIndex(None, MaxSimScores(normalize=False), storage="residual", codec=codec)
    index = CorpusIndex(None, MaxSimScores(normalize=True), storage="residual", codec=codec)
    assert len(index) == 0 and index.nbytes == 0 and index.residuals is None and index.codes is None
    assert index.centroids is codec.centroids and index.centroid_codes is None
    for call in (lambda: index.set_centroids(np.zeros((5, 64), np.float32)), lambda: index.fit_centroids(5)):
        with pytest.raises(ValueError, match="takes its centroids from its codec"):
            call()


# ---------------------------------------------------------------- header, binding, host-side refusals
def test_new_symbols_are_declared_and_bound():
    from polus_amd import _lib
    txt = open(os.path.join(ROOT, "include", "polus_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    for name in NEW:
        assert re.search(r"\bint\s+%s\s*\(" % name, code), name
        assert name in _lib.SIGNATURES, name
    n_args = {name: len(re.search(r"%s\s*\((.*?)\)" % name, code, flags=re.S).group(1).split(",")) for name in NEW}
    assert n_args == {name: len(_lib.SIGNATURES[name][1]) for name in NEW} == dict(zip(NEW, (11, 11, 21)))
    for rule in ("r_k = f32(x_k) - f32(centroids[code][k])", "the number of cutoffs c_j with r_k > c_j", "significant first","bit for bit polus_maxsim_rerank(Q, D)"):
        assert rule in txt, rule


@pytest.fixture(scope="module")
def lib():
    from polus_amd import build
    build.build(verbose=False)
    from polus_amd import _lib
    return _lib.load()


def test_entry_points_refuse_bad_arguments_on_the_host(lib):
    assert lib.polus_abi_version() == 1
    p, z = ctypes.c_void_p(256), None
    comp = lambda dtype=1, x=p, codes=p, cent=p, K=16, cut=p, nbits=2, packed=p, rows=4, E=64: \
        lib.polus_residual_compress(dtype, x, codes, cent, K, cut, nbits, packed, rows, E, None)
    dec = lambda dtype=1, codes=p, packed=p, cent=p, K=16, w=p, nbits=2, y=p, rows=4, E=64: \
        lib.polus_residual_decompress(dtype, codes, packed, cent, K, w, nbits, y, rows, E, None)
    rr = lambda dtype=1, Q=p, codes=p, packed=p, cent=p, K=16, w=p, nbits=2, cand=p, score=p, ldc=8, lds=8, B=2, C=8, N=10, Lq=4, Ld=6, E=64: \
        lib.polus_maxsim_rerank_res(dtype, Q, codes, packed, cent, K, w, nbits, None, None, cand, ldc, score, lds, B, C, N, Lq, Ld, E, None)

    def refused(rc, text):
        msg = lib.polus_last_error()
        assert rc != 0 and text in msg, (rc, msg)

    for call, name in ((comp, b"polus_residual_compress"), (dec, b"polus_residual_decompress"), (rr, b"polus_maxsim_rerank_res")):
        refused(call(nbits=3), name + b": nbits must be 1, 2 or 4 (got 3)")
        refused(call(nbits=0), b"nbits must be 1, 2 or 4")
        refused(call(nbits=8), b"nbits must be 1, 2 or 4")
        refused(call(E=48), name + b": E must be a multiple of 32 in [32, 256] (got 48)")
        refused(call(E=288), b"E must be a multiple of 32")
        refused(call(K=0), name + b": need 1 <= K <= 65535 centroids (got 0)")
        refused(call(K=65536), b"need 1 <= K <= 65535")
        refused(call(dtype=2), b"unknown dtype 2")
        refused(call(cent=z), name + b": null pointer")
        refused(call(codes=z), b"null pointer")
        refused(call(packed=z), b"null pointer")
        refused(call(cent=ctypes.c_void_p(264)), b"16-byte aligned")
        refused(call(packed=ctypes.c_void_p(258)), b"packed must be 4-byte aligned")
    for call in (comp, dec):
        refused(call(rows=0), b"need rows >= 1")
    refused(comp(x=z), b"null pointer")
    refused(comp(cut=z), b"null pointer")
    refused(dec(w=z), b"null pointer")
    refused(dec(y=z), b"null pointer")
    for kw in (dict(Q=z), dict(w=z), dict(cand=z), dict(score=z)):
        refused(rr(**kw), b"null pointer")
    refused(rr(ldc=7), b"ldc must be >= C")
    refused(rr(lds=7), b"lds must be >= C")
    refused(rr(N=0), b"need 1 <= N")
    refused(rr(C=0), b"need 1 <= C <= 65535")
    refused(rr(Lq=513), b"need 1 <= Lq <= 512")
    refused(rr(Ld=0), b"need 1 <= Ld <= 512")
