"""CPU: polus_maxsim_rerank and polus_topk_merge_ids refuse bad arguments on the host, their kernels compile for gfx950
without scratch in the expected instantiations, the polus.ir aliases resolve, and CorpusIndex.rerank cuts its candidate
columns by scratch_bytes."""
import ctypes
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "polus_amd", "csrc")


@pytest.fixture(scope="module")
def lib():
    from polus_amd import build
    build.build(verbose=False)
    from polus_amd import _lib
    return _lib.load()


def test_maxsim_rerank_refuses_on_the_host(lib):
    p = ctypes.c_void_p(256)                                           # never dereferenced: every call below is refused

    def rr(dtype=0, B=1, C=1, N=1, Lq=1, Ld=1, E=32, ldc=None, lds=None, Q=p, D=p, cand=p, S=p):
        rc = lib.polus_maxsim_rerank(dtype, Q, D, None, None, cand, C if ldc is None else ldc, S,
                                     C if lds is None else lds, B, C, N, Lq, Ld, E, None)
        assert rc != 0
        return lib.polus_last_error()
    assert b"unknown dtype" in rr(dtype=2) and b"unknown dtype" in rr(dtype=-1)
    assert b"multiple of 32" in rr(E=48) and b"multiple of 32" in rr(E=288) and b"multiple of 32" in rr(E=0)
    assert b"Lq <= 512" in rr(Lq=513) and b"Lq <= 512" in rr(Lq=0)
    assert b"Ld <= 512" in rr(Ld=513) and b"Ld <= 512" in rr(Ld=0)
    assert b"B <= 65535" in rr(B=65536) and b"B <= 65535" in rr(B=0)
    assert b"C <= 65535" in rr(C=65536) and b"C <= 65535" in rr(C=0, ldc=1, lds=1)
    assert b"N <= 2^31 - 1" in rr(N=0) and b"N <= 2^31 - 1" in rr(N=-5)
    assert b"ldc must be >= C" in rr(C=4, ldc=3, lds=4)
    assert b"lds must be >= C" in rr(C=4, ldc=4, lds=3)
    for kw in (dict(Q=None), dict(D=None), dict(cand=None), dict(S=None)):
        assert b"null pointer" in rr(**kw)
    assert b"16-byte aligned" in rr(Q=ctypes.c_void_p(260)) and b"16-byte aligned" in rr(D=ctypes.c_void_p(264))
    # the corpus may be as large as ids reach: N = 2^31 - 1 is refused for the null pointer alone
    assert b"null pointer" in rr(N=2 ** 31 - 1, S=None)
    assert lib.polus_abi_version() == 1


def test_topk_merge_ids_refuses_on_the_host(lib):
    p = ctypes.c_void_p(256)

    def topk(lds=8, ldi=8, rows=1, n=8, k=4, scores=p, ids=p, tv=p, ti=p):
        rc = lib.polus_topk_merge_ids(scores, lds, ids, ldi, rows, n, tv, ti, k, 1, None)
        assert rc != 0
        return lib.polus_last_error()
    assert b"1 <= k <= 1024" in topk(k=0) and b"1 <= k <= 1024" in topk(k=1025)
    assert b"rows >= 1 and n >= 1" in topk(n=0, lds=0, ldi=0) and b"rows >= 1 and n >= 1" in topk(rows=0)
    assert b"lds must be >= n" in topk(lds=7)
    assert b"ldi must be >= n" in topk(ldi=7)
    for kw in (dict(scores=None), dict(ids=None), dict(tv=None), dict(ti=None)):
        assert b"null pointer" in topk(**kw)
    assert all(b"polus_topk_merge_ids" in m for m in (topk(k=0), topk(ldi=7), topk(ids=None)))


@pytest.fixture(scope="module")
def rerank_asm(tmp_path_factory):
    hipcc = next((c for c in (os.environ.get("HIPCC"), "/opt/rocm/bin/hipcc") if c and os.path.exists(c)), None)
    if hipcc is None:
        pytest.skip("hipcc not found")
    out = {}
    for name in ("rerank", "topk"):
        dst = str(tmp_path_factory.mktemp(name) / (name + ".s"))
        r = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-S", "--cuda-device-only",
                            os.path.join(CSRC, name + ".hip"), "-o", dst], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        out[name] = open(dst).read()
    return out


def _private_segments(asm):
    return dict(re.findall(r"\.amdhsa_kernel\s+(\S+).*?\.amdhsa_private_segment_fixed_size\s+(\d+)", asm, flags=re.S))


def test_rerank_kernels_compile_without_scratch(rerank_asm):
    rr = {n: s for n, s in _private_segments(rerank_asm["rerank"]).items() if "maxsim_rerank_kernel" in n}
    # {f32, bf16} x E / 32 in 1..8 x {the query resident in registers, rounds over the document}
    assert len(rr) == 32
    assert sum("IfLi" in n for n in rr) == 16 and sum("Lb1E" in n for n in rr) == 16
    tk = {n: s for n, s in _private_segments(rerank_asm["topk"]).items() if "topk_merge_ids_kernel" in n}
    assert len(tk) == 2                                                # 2048 and 4096 LDS keys
    for name, size in {**rr, **tk}.items():
        assert int(size) == 0, f"{name}: private segment {size} B"
    # the new file's kernels keep clear of the names other tests count
    for n in _private_segments(rerank_asm["rerank"]):
        assert not any(x in n for x in ("maxsim_fwd_kernel", "maxsim_scores_kernel", "topk_merge_kernel"))


def test_two_stage_aliases():
    import polus.ir.search as asr
    import polus_amd.ir.search as s
    assert asr.TwoStageSearch is s.TwoStageSearch and asr.CorpusIndex is s.CorpusIndex
    assert callable(asr.CorpusIndex.rerank)
    from polus_amd import ops
    assert callable(ops.maxsim_rerank)
    from polus_amd import _lib
    assert "polus_maxsim_rerank" in _lib.SIGNATURES and "polus_topk_merge_ids" in _lib.SIGNATURES


def test_rerank_chunks_follow_scratch_bytes():
    from polus_amd.ir.search import CorpusIndex, TwoStageSearch
    ix = CorpusIndex(None, object(), scratch_bytes=4 * 8 * 100)
    assert ix.rerank_chunks(8, 250) == [(0, 100), (100, 200), (200, 250)]
    assert ix.rerank_chunks(8, 100) == [(0, 100)]
    ix.scratch_bytes = 1 << 40
    assert ix.rerank_chunks(1, 140000) == [(0, 65535), (65535, 131070), (131070, 140000)]
    ix.scratch_bytes = 31
    with pytest.raises(ValueError, match="scratch_bytes"):
        ix.rerank_chunks(8, 10)
    with pytest.raises(ValueError, match="empty"):
        CorpusIndex(None, object()).rerank({}, [[0]], 3)
    ix._n, ix.tokens = 5, False
    with pytest.raises(ValueError, match=r"\[CLS\]"):
        ix.rerank({}, [[0]], 3)
    with pytest.raises(ValueError, match="candidates must be >= 1"):
        TwoStageSearch(ix, ix, 0)
    # a CorpusIndex returns at most 1024 results per query, so it proposes no more candidates than that
    assert TwoStageSearch(ix, ix, 1024).candidates == 1024
    with pytest.raises(ValueError, match="at most 1024 candidates"):
        TwoStageSearch(ix, ix, 1025)
    assert TwoStageSearch(object(), ix, 5000).candidates == 5000           # another first stage sets its own limit
