"""CPU: what of the SPLADE path needs no GPU -- the host-side refusals of the four entry points, the host-only
workspace query, the compile check of splade.hip (no scratch memory, read from the kernel descriptors alone), the cases'
own properties and the references' consistency."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from tests import splade_cases as sc
from tests import splade_ref as sr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    from polus_amd import build
    build.build(verbose=False)
    from polus_amd import _lib
    return _lib.load()


def _err(lib):
    return lib.polus_last_error()


def test_pooling_refusals_happen_on_the_host(lib):
    p = ctypes.c_void_p(4096)
    fwd = lambda dtype=0, logits=p, ldl=64, rep=p, ldr=64, ldx=64, lda=64, B=2, S=5, V=64: lib.polus_splade_pool_fwd(
        dtype, logits, ldl, None, rep, ldr, p, ldx, p, lda, B, S, V, None)
    bwd = lambda dtype=0, drep=p, lddr=64, d=p, lddl=64, B=2, S=5, V=64: lib.polus_splade_pool_bwd(
        dtype, drep, lddr, p, 64, p, 64, d, lddl, B, S, V, None)
    for call, who in ((fwd, b"polus_splade_pool_fwd"), (bwd, b"polus_splade_pool_bwd")):
        assert call(dtype=2) != 0 and b"bad dtype" in _err(lib) and who in _err(lib)
        for kw in (dict(B=0), dict(S=0), dict(V=0), dict(B=65536)):
            assert call(**kw) != 0 and b"bad shape" in _err(lib), kw
    assert fwd(logits=None) != 0 and b"null pointer" in _err(lib)
    assert fwd(rep=None) != 0 and b"null pointer" in _err(lib)
    assert bwd(drep=None) != 0 and b"null pointer" in _err(lib)
    assert bwd(d=None) != 0 and b"null pointer" in _err(lib)
    for kw in (dict(ldl=63), dict(ldr=63), dict(ldx=63), dict(lda=63)):
        assert fwd(**kw) != 0 and b"bad stride" in _err(lib), kw
    for kw in (dict(lddr=63), dict(lddl=63)):
        assert bwd(**kw) != 0 and b"bad stride" in _err(lib), kw
    assert fwd(logits=ctypes.c_void_p(4098)) != 0 and b"not aligned" in _err(lib)          # f32 at an odd 2-byte address
    assert bwd(dtype=1, d=ctypes.c_void_p(4097)) != 0 and b"not aligned" in _err(lib)


def test_flops_reg_refusals_and_host_only_workspace_query(lib):
    p, q = ctypes.c_void_p(4096), ctypes.c_void_p(8192)
    assert lib.polus_flops_reg_workspace_bytes(30522) == 120 * 4                # one f32 per 256 columns
    assert lib.polus_flops_reg_workspace_bytes(256) == 4 and lib.polus_flops_reg_workspace_bytes(257) == 8
    assert lib.polus_flops_reg_workspace_bytes(0) == 0
    call = lambda rep=p, ldr=64, rows=3, V=64, loss=p, drep=q, lddr=64, ws=p, nb=1 << 20: lib.polus_flops_reg(
        rep, ldr, rows, V, 0.1, loss, 0, drep, lddr, ws, nb, None)
    for kw in (dict(rows=0), dict(V=0)):
        assert call(**kw) != 0 and b"bad shape" in _err(lib), kw
    for kw in (dict(rep=None), dict(loss=None)):
        assert call(**kw) != 0 and b"null pointer" in _err(lib), kw
    for kw in (dict(ldr=63), dict(lddr=63)):
        assert call(**kw) != 0 and b"bad stride" in _err(lib), kw
    assert call(drep=p) != 0 and b"must not be rep" in _err(lib)
    assert call(nb=0) != 0 and b"workspace" in _err(lib)
    assert call(ws=None) != 0 and b"workspace" in _err(lib)


def test_sparse_scores_refusals_happen_on_the_host(lib):
    p = ctypes.c_void_p(4096)
    call = lambda q=p, ldq=30522, ids=p, ldi=128, w=p, ldw=128, s=p, lds=1000, B=4, N=1000, M=128, V=30522: lib.polus_sparse_scores(
        q, ldq, ids, ldi, w, ldw, s, lds, B, N, M, V, None)
    for M in (0, 1025):
        assert call(M=M, ldi=2048, ldw=2048) != 0 and b"1 <= M <= 1024" in _err(lib), M
    # a vocabulary whose row does not fit LDS: the message names the limit
    assert call(V=sc.LDS_LIMIT_V + 1, ldq=sc.LDS_LIMIT_V + 1) != 0
    assert b"163840" in _err(lib) and b"V <= 40960" in _err(lib) and b"LDS" in _err(lib)
    for kw in (dict(B=0), dict(N=0), dict(V=0)):
        assert call(**kw) != 0 and b"bad shape" in _err(lib), kw
    for kw in (dict(q=None), dict(ids=None), dict(w=None), dict(s=None)):
        assert call(**kw) != 0 and b"null pointer" in _err(lib), kw
    for kw in (dict(ldq=30521), dict(ldi=127), dict(ldw=127), dict(lds=999)):
        assert call(**kw) != 0 and b"bad stride" in _err(lib), kw


def test_launchers_refuse_host_tensors():
    from polus_amd import build
    build.build(verbose=False)
    from polus_amd import ops
    from polus_amd._lib import PolusHipError
    f, i = torch.zeros(2, 8), torch.zeros(2, 8, dtype=torch.int32)
    with pytest.raises(PolusHipError):
        ops.splade_pool_fwd(torch.zeros(6, 8), None, f, f.clone(), i, 2, 3)
    with pytest.raises(PolusHipError):
        ops.splade_pool_bwd(f, f.clone(), i, torch.zeros(6, 8), 2, 3)
    with pytest.raises(PolusHipError):
        ops.flops_reg(f, 0.1, torch.zeros(1))
    with pytest.raises(PolusHipError):
        ops.sparse_scores(f, i, f.clone(), torch.zeros(2, 2))


def test_index_and_trainer_argument_checks_need_no_gpu():
    from polus_amd.ir.search import SparseCorpusIndex
    for terms in (0, 1025):
        with pytest.raises(ValueError, match="terms"):
            SparseCorpusIndex(None, terms=terms)
    index = SparseCorpusIndex(None, terms=128)
    assert len(index) == 0 and index.nbytes == 0 and index.term_ids is None
    with pytest.raises(ValueError, match="empty"):
        index.search(None, 5)


# ---------------------------------------------------------------- compile check
def test_splade_kernels_compile_for_gfx950_without_scratch(tmp_path):
    hipcc = next((c for c in (os.environ.get("HIPCC"), "/opt/rocm/bin/hipcc") if c and os.path.exists(c)), None)
    if hipcc is None:
        pytest.skip("hipcc not found")
    dst = str(tmp_path / "splade.s")
    r = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-S", "--cuda-device-only",
                        os.path.join(ROOT, "polus_amd", "csrc", "splade.hip"), "-o", dst], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    segs = dict(re.findall(r"\.amdhsa_kernel\s+(\S+).*?\.amdhsa_private_segment_fixed_size\s+(\d+)", open(dst).read(), flags=re.S))
    for stem, n in (("splade_pool_fwd_kernel", 4), ("splade_pool_bwd_kernel", 4), ("flops_reg_cols_kernel", 1),
                    ("flops_reg_finalize_kernel", 1), ("sparse_scores_kernel", 1)):
        assert sum(stem in name for name in segs) == n, (stem, sorted(segs))
    assert len(segs) == 11
    for name, size in segs.items():
        assert int(size) == 0, f"{name}: private segment {size} B"


# ---------------------------------------------------------------- the cases and the references
def test_pool_cases_are_what_the_docstring_says():
    for B, S, V in sc.POOL_SHAPES:
        x, mask = sc.pool_case(B, S, V)
        assert np.array_equal(torch.as_tensor(x.copy()).to(torch.bfloat16).double().numpy(), x), "not exact in bf16"
        rep, xmax, arg = sr.pool_fwd(x, mask)
        assert (x[:, :, 0] < 0).all() and (arg[:, 0] == -1).all()
        assert (x[:, :, 1].max(1) == 0).all() and (arg[:, 1] == -1).all() and (rep[:, 1] == 0).all()
        if B > 1:
            assert not mask[B - 1].any() and (arg[B - 1] == -1).all() and 0 < mask[0].sum() < S      # a masked sequence; holes
        if S >= 17:
            won = arg >= 0
            ties = (np.where(mask[:, :, None] != 0, x, -np.inf) == np.where(won, xmax, np.inf)[:, None, :]).sum(1)
            assert (ties[won] > 1).mean() > 0.1, "ties are rare"
            assert (np.asarray(mask)[np.arange(B)[:, None], np.maximum(arg, 0)][won] != 0).all()
    assert {(sc.padded_ld(V, dt) * sc.ESIZE[dt]) % 16 for _, _, V in sc.POOL_SHAPES for dt in sc.ESIZE} == {0}


def test_pool_references_agree_with_finite_differences():
    rng = np.random.Generator(np.random.PCG64(4))
    x = rng.standard_normal((2, 6, 9))
    mask = np.ones((2, 6), np.int32)
    mask[0, 3:] = 0
    c = rng.standard_normal((2, 9))
    rep, xmax, arg = sr.pool_fwd(x, mask)
    d = sr.pool_bwd(c, xmax, arg, 6)
    f = lambda z: float((c * sr.pool_fwd(z, mask)[0]).sum())
    num = np.zeros_like(x)
    for idx in np.ndindex(*x.shape):
        z = x.copy(); z[idx] += 1e-6
        w = x.copy(); w[idx] -= 1e-6
        num[idx] = (f(z) - f(w)) / 2e-6
    assert np.abs(num - d).max() < 1e-6
    assert (d[0, 3:] == 0).all()
    f32 = sr.pool_bwd_f32(c.astype(np.float32), xmax.astype(np.float32), arg, 6)
    assert f32.dtype == np.float32 and np.abs(f32 - d).max() < 1e-6


def test_flops_and_score_references():
    rep, _ = sc.flops_case(3, 64)
    val, g = sr.flops_reg(rep, 0.5)
    eps = 1e-6
    z = rep.astype(np.float64).copy(); z[1, 7] += eps
    assert abs((sr.flops_reg(z, 0.5)[0] - val) / eps - g[1, 7]) < 1e-5
    for M in sc.SCORE_M:
        q, ids, w = sc.score_case(M, 64, exact=True)
        assert ids.min() == -1 and ids.max() == 64 and (M == 1 or (ids[:, 0] == ids[:, 1]).all())
        s, mag = sr.sparse_scores(q, ids, w)
        n = 7
        want = sum(float(w[n, m]) * float(q[1, ids[n, m]]) for m in range(M) if 0 <= ids[n, m] < 64)
        assert s[1, n] == want and mag[1, n] == want                    # eighths, non-negative: exact
        assert np.array_equal(s.astype(np.float32).astype(np.float64), s), "case (a) is not exact in f32"
    t_ids, t_w = sr.truncate(np.array([[0.0, 2.0, 2.0, 1.0]]), 3)
    assert t_ids.tolist() == [[1, 2, 3]] and t_w.tolist() == [[2.0, 2.0, 1.0]]
    assert sr.rank(np.array([[1.0, 3.0, 3.0]]), 2)[1].tolist() == [[1, 2]]
