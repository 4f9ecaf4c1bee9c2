"""CPU: the NumPy reference of corpus search (tests/search_ref.py) obeys the selection rule of polus_topk_merge, the
ranking metrics give hand-worked float64 values, polus_topk_merge and polus_maxsim_scores refuse bad arguments on the
host, their kernels compile for gfx950 without scratch, the polus.ir aliases resolve, and the seeded corpora of the
GPU float64 test leave an f32 evaluation of the reference inside that test's bounds."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from tests import maxsim_ref, search_ref as sr
from tests.search_cases import CLS_CASE, KS, TOKEN_CASE, cls_case, dot_tol, maxsim_tol, token_case

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "polus_amd", "csrc")


# ---------------------------------------------------------------- reference top-k
def test_reference_topk_is_chunk_invariant():
    r = np.random.Generator(np.random.PCG64(1))
    s = r.integers(0, 6, size=(5, 300)).astype(np.float32)            # heavy ties
    s[0, ::7] = np.nan
    s[1, ::5] = -np.inf
    whole = sr.topk(s, 20)
    for cuts in ([0, 300], [0, 1, 300], [0, 100, 200, 300], [0, 17, 18, 250, 300]):
        state = None
        for a, b in zip(cuts[:-1], cuts[1:]):
            state = sr.topk_merge(s[:, a:b], np.arange(a, b), 20, state)
        assert np.array_equal(state[0], whole[0]) and np.array_equal(state[1], whole[1]), cuts
    # chunks merged in reverse order give the same set and order too
    state = None
    for a, b in ((200, 300), (0, 200)):
        state = sr.topk_merge(s[:, a:b], np.arange(a, b), 20, state)
    assert np.array_equal(state[0], whole[0]) and np.array_equal(state[1], whole[1])


def test_reference_topk_ties_padding_and_k_above_n():
    s = np.array([[2.0, 5.0, 2.0, 5.0, np.nan, -np.inf, -0.0, 0.0, np.inf]], np.float32)
    v, i = sr.topk(s, 4, id0=100)
    assert i.tolist() == [[108, 101, 103, 100]] and v.tolist() == [[np.inf, 5.0, 5.0, 2.0]]      # ties: lower id first
    v, i = sr.topk(s, 12)
    assert i.tolist() == [[8, 1, 3, 0, 2, 6, 7, -1, -1, -1, -1, -1]]                            # -0.0 == +0.0: id order
    assert v[0, 7:].tolist() == [-np.inf] * 5 and not np.signbit(v[0, 5])
    v, i = sr.topk(np.full((2, 3), -np.inf, np.float32), 2)
    assert (i == -1).all() and (v == -np.inf).all()
    v, i = sr.topk_merge(np.array([[1.0]], np.float32), [7], 3, state=(np.array([[4.0, -np.inf, 9.0]]), np.array([[2, -1, -1]])))
    assert i.tolist() == [[2, 7, -1]]                                  # state entries with id < 0 are padding, whatever their value


# ---------------------------------------------------------------- metrics
def test_ranking_metrics_hand_worked_values():
    from polus_amd.ir.metrics import MRRAtK, NDCGAtK, RecallAtK
    ranked = np.array([[9, 8, 4, 7, 3],          # query 0: relevant {4, 3, 6}: first hit at rank 3
                       [1, -1, 2, -1, -1]])      # query 1: relevant {2}; padding inside the top k
    rel = [[4, 3, 6], {2}]
    for k, recall, mrr in ((2, (0 + 0) / 2, (0 + 0) / 2), (5, (2 / 3 + 1) / 2, (1 / 3 + 1 / 3) / 2)):
        m1, m2 = RecallAtK(k), MRRAtK(k)
        assert (m1.name, m2.name) == (f"Recall@{k}", f"MRR@{k}")
        m1.samples_from_batch((ranked, rel))
        m2.samples_from_batch((ranked, rel))
        assert m1.evaluate() == recall and m2.evaluate() == mrr
        assert sr.recall_at_k(ranked, rel, k) == recall and sr.mrr_at_k(ranked, rel, k) == mrr
    # graded gains: DCG = 1 / log2(4) + 3 / log2(5) (ranks 3 and 4), ideal = 3 / log2(2) + 2 / log2(3) + 1 / log2(4)
    g = [{4: 1.0, 7: 3.0, 6: 2.0}]
    m = NDCGAtK(4)
    assert m.name == "nDCG@4"
    m.samples_from_batch((ranked[:1], g))
    want = (1 / np.log2(4) + 3 / np.log2(5)) / (3 / np.log2(2) + 2 / np.log2(3) + 1 / np.log2(4))
    got = m.evaluate()
    assert abs(got - want) < 1e-15 and abs(sr.ndcg_at_k(ranked[:1], g, 4) - want) < 1e-15
    # binary relevance given as ids, padding inside k: only rank 3 counts
    m.samples_from_batch((ranked[1:], [[2]]))
    assert abs(m.evaluate() - (1 / np.log2(4)) / 1.0) < 1e-15
    # evaluate() resets; the mean runs over every query since
    m = RecallAtK(5)
    m.samples_from_batch((ranked[:1], rel[:1]))
    m.samples_from_batch((ranked[1:], rel[1:]))
    assert m.evaluate() == (2 / 3 + 1) / 2
    m.samples_from_batch((ranked[1:], rel[1:]))
    assert m.evaluate() == 1.0
    # reduce_f is applied first; a query without a relevant document raises; too few columns raise
    m = MRRAtK(5, reduce_f=lambda s: (s[0][:, ::-1], s[1]))
    m.samples_from_batch((ranked[:1], rel[:1]))
    assert m.evaluate() == 1.0                                       # reversed: document 3 at rank 1
    for cls in (RecallAtK, MRRAtK, NDCGAtK):
        with pytest.raises(ValueError):
            cls(2).samples_from_batch((ranked, [[4], []]))
        with pytest.raises(ValueError):
            cls(6).samples_from_batch((ranked, rel))
        with pytest.raises(ValueError):
            cls(0)


def test_metrics_take_device_like_tensors():
    import torch
    from polus_amd.ir.metrics import RecallAtK
    m = RecallAtK(2)
    m.samples_from_batch((torch.tensor([[5, 1, 0]], dtype=torch.int32), [(1,)]))
    assert m.evaluate() == 1.0


# ---------------------------------------------------------------- host refusals
@pytest.fixture(scope="module")
def lib():
    from polus_amd import build
    build.build(verbose=False)
    from polus_amd import _lib
    return _lib.load()


def test_topk_merge_and_maxsim_scores_refuse_on_the_host(lib):
    p = ctypes.c_void_p(256)                                           # never dereferenced: every call below is refused

    def topk(lds=8, rows=1, n=8, id0=0, k=4, scores=p, tv=p, ti=p):
        rc = lib.polus_topk_merge(scores, lds, rows, n, id0, tv, ti, k, 1, None)
        assert rc != 0
        return lib.polus_last_error()
    assert b"1 <= k <= 1024" in topk(k=0) and b"1 <= k <= 1024" in topk(k=1025)
    assert b"lds must be >= n" in topk(lds=7)
    assert b"2^31 - 1" in topk(id0=2 ** 31 - 8, n=8, lds=8) and b"2^31 - 1" in topk(id0=-1)
    assert b"rows >= 1 and n >= 1" in topk(n=0, lds=0) and b"rows >= 1 and n >= 1" in topk(rows=0)
    for kw in (dict(scores=None), dict(tv=None), dict(ti=None)):
        assert b"null pointer" in topk(**kw)

    def scores(B=1, N=1, Lq=1, Ld=1, E=32, lds=None, Q=p, D=p, S=p):
        rc = lib.polus_maxsim_scores(0, Q, D, None, None, S, N if lds is None else lds, B, N, Lq, Ld, E, None)
        assert rc != 0
        return lib.polus_last_error()
    assert b"multiple of 32" in scores(E=48) and b"multiple of 32" in scores(E=288)
    assert b"Lq <= 512" in scores(Lq=513) and b"Ld <= 512" in scores(Ld=513)
    assert b"B <= 65535" in scores(B=65536) and b"N <= 65535" in scores(N=65536)
    assert b"lds must be >= N" in scores(N=4, lds=3)
    for kw in (dict(Q=None), dict(D=None), dict(S=None)):
        assert b"null pointer" in scores(**kw)
    assert b"16-byte aligned" in scores(Q=ctypes.c_void_p(260))
    # B*N*Lq >= 2^31 is the argmax's limit: polus_maxsim_fwd refuses it, polus_maxsim_scores does not name it
    rc = lib.polus_maxsim_fwd(0, p, p, None, None, p, 2049, p, 2049, 2049, 512, 1, 32, None)
    assert rc != 0 and b"2^31" in lib.polus_last_error()
    assert b"2^31" not in scores(B=2049, N=2049, Lq=512, S=None)       # refused for the null pointer alone
    assert lib.polus_abi_version() == 1


# ---------------------------------------------------------------- compile check
@pytest.fixture(scope="module")
def search_asm(tmp_path_factory):
    hipcc = next((c for c in (os.environ.get("HIPCC"), "/opt/rocm/bin/hipcc") if c and os.path.exists(c)), None)
    if hipcc is None:
        pytest.skip("hipcc not found")
    out = {}
    for name in ("topk", "maxsim"):
        dst = str(tmp_path_factory.mktemp(name) / (name + ".s"))
        r = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-S", "--cuda-device-only",
                            os.path.join(CSRC, name + ".hip"), "-o", dst], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        out[name] = open(dst).read()
    return out


def _kernels(asm):
    segs = dict(re.findall(r"\.amdhsa_kernel\s+(\S+).*?\.amdhsa_private_segment_fixed_size\s+(\d+)", asm, flags=re.S))
    bodies = {m.group(1): m.group(2) for m in re.finditer(r"^(_Z\w+):[^\n]*$(.*?)^\s*\.size\s+\1,", asm, flags=re.M | re.S)}
    return segs, bodies


def test_search_kernels_compile_without_scratch(search_asm):
    segs, bodies = _kernels(search_asm["topk"])
    assert sum("topk_merge_kernel" in n for n in segs) == 2            # 2048 and 4096 LDS keys
    m_segs, m_bodies = _kernels(search_asm["maxsim"])
    new = {n for n in m_segs if "maxsim_scores_kernel" in n}
    assert len(new) == 16                                              # E / 32 in 1..8 x {f32, bf16}
    segs.update({n: m_segs[n] for n in new})
    bodies.update(m_bodies)
    for name, size in segs.items():
        assert int(size) == 0, f"{name}: private segment {size} B"
        assert not re.search(r"^\s*scratch_", bodies[name], flags=re.M), f"{name} uses scratch_ instructions"
    # the scores kernels write no argmax: one global store site fewer than their polus_maxsim_fwd twins
    stores = lambda n: len(re.findall(r"^\s*global_store_", m_bodies[n], flags=re.M))
    for n in new:
        inst = lambda name: re.search(r"kernelI(\w+?Li\d)E", name).group(1)      # element type and E / 32
        twin = next(t for t in m_segs if "maxsim_fwd_kernel" in t and inst(t) == inst(n))
        assert stores(n) < stores(twin), (n, twin)


# ---------------------------------------------------------------- aliases
def test_search_and_metrics_aliases():
    import polus.ir.metrics as am
    import polus.ir.search as asr
    import polus_amd.ir.metrics as m
    import polus_amd.ir.search as s
    for name in ("CorpusIndex", "RetrievalValidationCallback"):
        assert getattr(asr, name) is getattr(s, name)
    for name in ("RecallAtK", "MRRAtK", "NDCGAtK"):
        assert getattr(am, name) is getattr(m, name)
    from polus_amd import ops
    assert callable(ops.topk_merge) and callable(ops.maxsim_scores)


def test_corpus_index_chunks_follow_scratch_bytes():
    from polus_amd.ir.search import CorpusIndex
    ix = CorpusIndex(None, object(), scratch_bytes=4 * 8 * 100)
    ix._n = 250
    assert ix.chunks(8) == [(0, 100), (100, 200), (200, 250)]
    ix.scratch_bytes, ix._n = 1 << 40, 140000
    assert ix.chunks(1) == [(0, 65535), (65535, 131070), (131070, 140000)]
    ix.scratch_bytes = 31
    with pytest.raises(ValueError):
        ix.chunks(8)
    with pytest.raises(ValueError):
        CorpusIndex(None, object()).search({}, 3)                      # empty index


# ---------------------------------------------------------------- the float64 test's seeds
@pytest.mark.parametrize("mode", ["f32", "bf16"])
def test_float64_search_bounds_hold_for_an_f32_evaluation_of_the_reference(mode):
    """The GPU test holds CorpusIndex.search to three bounds against float64 (tests/search_ref.check_against_float64).
    On the same seeded corpora, with the inputs rounded as the device sees them, scores evaluated in f32 by NumPy and
    ranked by the reference stay inside those bounds: the bounds ask nothing f32 arithmetic cannot give."""
    import torch
    from tests.util import rounded
    dt = torch.float32 if mode == "f32" else torch.bfloat16
    c = token_case(**TOKEN_CASE)
    tab = rounded(c["table"], dt)
    q, d = tab[c["q_ids"]], tab[c["d_ids"]]
    s64 = sr.maxsim_scores(q, d, c["q_mask"], c["d_mask"])
    s32 = np.empty_like(s64, dtype=np.float32)
    q32, d32 = q.astype(np.float32), d.astype(np.float32)
    for a in range(0, d.shape[0], 64):
        sim = np.einsum("bie,cje->bcij", q32, d32[a:a + 64]).astype(np.float64)
        s32[:, a:a + 64] = maxsim_ref.maxsim_fwd(q, d[a:a + 64], c["q_mask"], c["d_mask"][a:a + 64], s=sim)[0].astype(np.float32)
    t = maxsim_tol(mode) * np.abs(s64).max()
    for k in KS:
        v, i = sr.topk(s32, k)
        assert sr.check_against_float64(v, i, s64, k, t) == []
    c = cls_case(**CLS_CASE)
    tab = rounded(c["table"], dt)
    q, d = tab[c["q_ids"][:, 0]], tab[c["d_ids"][:, 0]]
    s64 = sr.dot_scores(q, d)
    s32 = q.astype(np.float32) @ d.astype(np.float32).T
    t = dot_tol(CLS_CASE["E"]) * np.abs(s64).max()
    for k in KS:
        v, i = sr.topk(s32, k)
        assert sr.check_against_float64(v, i, s64, k, t) == []
