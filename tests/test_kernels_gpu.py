"""Per-kernel parity: HIP kernels (through the C ABI) vs the CPU oracle on seeded inputs.

Tolerances: f32 path 2e-5 of max|ref| (exact-f32 MFMA, different summation order only);
bf16 path 1.5e-2 of max|ref| against the oracle evaluated on the bf16-rounded inputs
(bf16 storage of outputs, f32 accumulation)."""
import math

import numpy as np
import pytest
import torch

from oracle import bert as ob
from oracle import losses as ol
from oracle import optim as oo
from tests.util import TOL, assert_close, dev, host, rounded

pytestmark = pytest.mark.gpu

DTYPES = [torch.float32, torch.bfloat16]


@pytest.fixture(scope="module")
def ops():
    from polus_amd import ops as _ops
    return _ops


def rng(seed):
    return np.random.Generator(np.random.PCG64(seed))


# ------------------------------------------------------------------------------- GEMM
def _layout(a, layout):
    return a if layout == 0 else np.ascontiguousarray(a.T)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("al,bl", [(0, 0), (0, 1), (1, 1), (1, 0)])
@pytest.mark.parametrize("M,N,K", [(256, 384, 192), (128, 128, 64), (100, 72, 136), (97, 50, 75), (5, 4, 768)])
def test_gemm_layouts(ops, dtype, al, bl, M, N, K):
    r = rng(M * 7 + N * 3 + K + al * 2 + bl)
    A = r.standard_normal((M, K))
    B = r.standard_normal((N, K))
    a_t, b_t = dev(_layout(A, al), dtype), dev(_layout(B, bl), dtype)
    out = torch.full((M, N), float("nan"), dtype=dtype, device="cuda")
    ops.gemm(a_t, b_t, out, a_layout=al, b_layout=bl)
    ref = rounded(A, dtype) @ rounded(B, dtype).T
    assert_close(host(out), ref, TOL[dtype], f"gemm {al}{bl} {M}x{N}x{K}")


@pytest.mark.parametrize("dtype", DTYPES)
def test_gemm_asymmetric_identity(ops, dtype):
    # A = I with an asymmetric B catches a transposed C write or a swapped fragment map
    n = 128
    A = np.eye(n)
    B = (np.arange(n)[:, None] * 3 + np.arange(n)[None, :] % 7).astype(np.float64) / 64.0
    out = torch.zeros((n, n), dtype=dtype, device="cuda")
    ops.gemm(dev(A, dtype), dev(B, dtype), out)          # out = A @ B^T = B^T
    assert_close(host(out), rounded(B, dtype).T, 1e-6 if dtype == torch.float32 else 4e-3, "identity")
    for al, bl in [(0, 1), (1, 1), (1, 0)]:
        out.zero_()
        ops.gemm(dev(_layout(A, al), dtype), dev(_layout(B, bl), dtype), out, a_layout=al, b_layout=bl)
        assert_close(host(out), rounded(B, dtype).T, 1e-6 if dtype == torch.float32 else 4e-3, f"identity {al}{bl}")


@pytest.mark.parametrize("dtype", DTYPES)
def test_gemm_epilogues(ops, dtype):
    M, N, K = 200, 136, 96
    r = rng(5)
    A, B = r.standard_normal((M, K)), r.standard_normal((N, K)) * 0.2
    bias = r.standard_normal(N)
    R = r.standard_normal((M, N))
    a_t, b_t = dev(A, dtype), dev(B, dtype)
    bias_t, r_t = dev(bias, torch.float32), dev(R, dtype)
    base = rounded(A, dtype) @ rounded(B, dtype).T
    tol = TOL[dtype]
    # bias + residual
    out = torch.empty((M, N), dtype=dtype, device="cuda")
    ops.gemm(a_t, b_t, out, bias=bias_t, resid=r_t)
    assert_close(host(out), base + bias + rounded(R, dtype), tol, "bias+resid")
    # bias + gelu forward with pre-activation saved
    aux = torch.empty((M, N), dtype=dtype, device="cuda")
    ops.gemm(a_t, b_t, out, bias=bias_t, aux=aux, act="gelu", flags=ops.GEMM_ACT_FWD)
    assert_close(host(aux), base + bias, tol, "gelu aux")
    assert_close(host(out), ob.gelu(base + bias), tol, "gelu out")
    # activation backward: C = (A.B) * gelu'(aux)
    u = host(aux)
    ops.gemm(a_t, b_t, out, aux=aux, act="gelu", flags=ops.GEMM_ACT_BWD)
    assert_close(host(out), base * ob.gelu_grad(u), tol, "gelu bwd")
    ops.gemm(a_t, b_t, out, bias=bias_t, aux=aux, act="swish", flags=ops.GEMM_ACT_FWD)
    assert_close(host(out), ob.swish(base + bias), tol, "swish out")
    # alpha + accumulate into an f32 C (gradient accumulation), also with split-K
    c32 = dev(R, torch.float32)
    ops.gemm(a_t, b_t, c32, alpha=0.5, flags=ops.GEMM_ACCUM_C)
    assert_close(host(c32), 0.5 * base + R.astype(np.float32), tol, "accum f32")
    c32 = dev(R, torch.float32)
    ops.gemm(a_t, b_t, c32, alpha=0.5, flags=ops.GEMM_ACCUM_C, split_k=3, bias=bias_t)
    assert_close(host(c32), 0.5 * base + bias + R.astype(np.float32), tol, "accum f32 split-k")


@pytest.mark.parametrize("dtype", DTYPES)
def test_gemm_dw_shape_splitk(ops, dtype):
    # dW = dY^T X with a long contraction, both operands K-strided, f32 output, split-K
    T, N, K = 2048, 192, 160
    r = rng(11)
    dY, X = r.standard_normal((T, N)) * 0.1, r.standard_normal((T, K))
    out = torch.empty((N, K), dtype=torch.float32, device="cuda")
    ref = rounded(dY, dtype).T @ rounded(X, dtype)
    for sk in (1, 4, 7):
        out.fill_(float("nan"))
        ops.gemm(dev(dY, dtype), dev(X, dtype), out, a_layout=1, b_layout=1, split_k=sk)
        assert_close(host(out), ref, 3e-5 if dtype == torch.float32 else 2e-3, f"dW split_k={sk}")
    # bitwise reproducible
    o1 = out.clone()
    ops.gemm(dev(dY, dtype), dev(X, dtype), out, a_layout=1, b_layout=1, split_k=7)
    assert torch.equal(o1, out)


@pytest.mark.parametrize("dtype", DTYPES)
def test_gemm_bert_shapes(ops, dtype):
    T, H, I = 512, 768, 3072
    r = rng(3)
    X, W = r.standard_normal((T, H)), r.standard_normal((I, H)) * 0.02
    out = torch.empty((T, I), dtype=dtype, device="cuda")
    ops.gemm(dev(X, dtype), dev(W, dtype), out)
    assert_close(host(out), rounded(X, dtype) @ rounded(W, dtype).T, TOL[dtype], "ffn1")
    dY = r.standard_normal((T, I)) * 0.1
    dx = torch.empty((T, H), dtype=dtype, device="cuda")
    ops.gemm(dev(dY, dtype), dev(W, dtype), dx, b_layout=1)
    assert_close(host(dx), rounded(dY, dtype) @ rounded(W, dtype), TOL[dtype], "dX")


def test_gemm_rejects_bad_arguments(ops):
    from polus_amd._lib import PolusHipError
    a = torch.zeros((8, 8), device="cuda")
    with pytest.raises(PolusHipError):
        ops.gemm(a, a, torch.zeros((8, 8), device="cuda"), aux=None, act="gelu", flags=ops.GEMM_ACT_BWD)
    with pytest.raises(PolusHipError):
        ops.gemm(a.cpu(), a.cpu(), a.cpu())


@pytest.mark.parametrize("dtype", DTYPES)
def test_attention_rejects_dropout_index_overflow(ops, dtype):
    """The attention dropout index ((b A + h) S + q) S + key is a uint32: both directions refuse B * A * S^2 >= 2^32
    before launching anything."""
    from polus_amd._lib import PolusHipError
    B, S, A = 1, 65536, 1
    qkv = torch.zeros((B * S, 192), dtype=dtype, device="cuda")
    ctx = torch.zeros((B * S, 64), dtype=dtype, device="cuda")
    lse = torch.zeros((B, A, S), device="cuda")
    with pytest.raises(PolusHipError, match="dropout"):
        ops.attention_fwd(qkv, None, ctx, lse, B, S, A, drop_p=0.1, seed=1)
    dqkv = torch.full_like(qkv, 7.0)
    with pytest.raises(PolusHipError, match="dropout"):
        ops.attention_bwd(qkv, None, ctx, torch.zeros_like(ctx), lse, dqkv, B, S, A, drop_p=0.1, seed=1)
    torch.cuda.synchronize()
    assert bool((dqkv == 7.0).all())                    # nothing was launched


# ------------------------------------------------------------------------------- attention
def _attn_case(B, S, A, seed, full_mask=False):
    r = rng(seed)
    H = A * 64
    qkv = r.standard_normal((B, S, 3 * H)) * 0.7
    lens = r.integers(max(1, S // 2), S + 1, size=B)
    mask = (np.arange(S)[None] < lens[:, None]).astype(np.int32)
    if full_mask:
        mask[:] = 1
    dctx = r.standard_normal((B, S, H))
    return qkv, mask, dctx


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("B,S,A", [(2, 64, 2), (3, 48, 2), (1, 200, 3), (2, 256, 12), (1, 512, 2), (2, 17, 1)])
def test_attention_fwd_bwd(ops, dtype, B, S, A):
    qkv, mask, dctx = _attn_case(B, S, A, seed=B * 100 + S + A)
    H = A * 64
    q_r = rounded(qkv, dtype)
    ctx_ref, probs = ob.attention_fwd(q_r, ob.additive_mask(mask, np.float64), A)
    qkv_t = dev(qkv.reshape(B * S, 3 * H), dtype)
    mask_t = dev(mask)
    ctx = torch.full((B * S, H), float("nan"), dtype=dtype, device="cuda")
    lse = torch.empty((B, A, S), dtype=torch.float32, device="cuda")
    ops.attention_fwd(qkv_t, mask_t, ctx, lse, B, S, A)
    tol = 5e-5 if dtype == torch.float32 else 2e-2
    assert_close(host(ctx).reshape(B, S, H), ctx_ref, tol, "ctx")
    # log-sum-exp of the masked scaled scores
    q = q_r[..., :H].reshape(B, S, A, 64).transpose(0, 2, 1, 3)
    k = q_r[..., H:2 * H].reshape(B, S, A, 64).transpose(0, 2, 1, 3)
    sc = q @ k.transpose(0, 1, 3, 2) / 8.0 + ob.additive_mask(mask, np.float64)
    mx = sc.max(-1, keepdims=True)
    lse_ref = (mx + np.log(np.exp(sc - mx).sum(-1, keepdims=True)))[..., 0]
    assert np.abs(host(lse) - lse_ref).max() < (1e-3 if dtype == torch.float32 else 5e-2)
    # backward
    dqkv_ref = ob.attention_bwd(rounded(dctx, dtype), q_r, probs, A)
    dqkv = torch.full((B * S, 3 * H), float("nan"), dtype=dtype, device="cuda")
    ops.attention_bwd(qkv_t, mask_t, ctx, dev(dctx.reshape(B * S, H), dtype), lse, dqkv, B, S, A)
    out = host(dqkv).reshape(B, S, 3 * H)
    for nm, sl in (("dq", slice(0, H)), ("dk", slice(H, 2 * H)), ("dv", slice(2 * H, 3 * H))):
        assert_close(out[..., sl], dqkv_ref[..., sl], 1e-4 if dtype == torch.float32 else 3e-2, nm)


@pytest.mark.parametrize("S,A,drop", [(64, 2, 0.0), (128, 3, 0.2), (256, 12, 0.1)])
def test_attention_backward_one_pass_equals_two_kernel_form(ops, S, A, drop):
    """The one-pass backward (one workgroup per (batch, head), every score evaluated once; bf16, S in {64, 128,
    256}) against the two-kernel form on the same inputs, masks and dropout seed: same dropped probabilities and
    dS in bf16, different summation order only."""
    B, H = 3, A * 64
    qkv, mask, dctx = _attn_case(B, S, A, seed=S + A)
    dt = torch.bfloat16
    qkv_t, mask_t, dctx_t = dev(qkv.reshape(B * S, 3 * H), dt), dev(mask), dev(dctx.reshape(B * S, H), dt)
    ctx = torch.empty((B * S, H), dtype=dt, device="cuda")
    lse = torch.empty((B, A, S), dtype=torch.float32, device="cuda")
    ops.attention_fwd(qkv_t, mask_t, ctx, lse, B, S, A, drop_p=drop, seed=77)
    outs = []
    ops.set_env("POLUS_ATTN_BWD_KRES", 0)            # the query-resident one-pass kernel (S = 256 would otherwise take the key-resident one)
    try:
        for fused in (1, 0):                          # 1: one pass (32-key blocks at S = 64 / 128, 64-key blocks by LDS-DMA at 256), 0: two kernels
            ops.set_env("POLUS_ATTN_FUSED", fused)
            try:
                d = torch.full((B * S, 3 * H), float("nan"), dtype=dt, device="cuda")
                ops.attention_bwd(qkv_t, mask_t, ctx, dctx_t, lse, d, B, S, A, drop_p=drop, seed=77)
                outs.append(host(d).reshape(B, S, 3 * H))
            finally:
                ops.set_env("POLUS_ATTN_FUSED")
        for nm, sl in (("dq", slice(0, H)), ("dk", slice(H, 2 * H)), ("dv", slice(2 * H, 3 * H))):
            assert_close(outs[0][..., sl], outs[1][..., sl], 1.5e-2, nm)
        # run-to-run bitwise identical
        d2 = torch.empty((B * S, 3 * H), dtype=dt, device="cuda")
        ops.attention_bwd(qkv_t, mask_t, ctx, dctx_t, lse, d2, B, S, A, drop_p=drop, seed=77)
        d3 = torch.empty_like(d2)
        ops.attention_bwd(qkv_t, mask_t, ctx, dctx_t, lse, d3, B, S, A, drop_p=drop, seed=77)
        assert torch.equal(d2, d3)
    finally:
        ops.set_env("POLUS_ATTN_BWD_KRES")


@pytest.mark.parametrize("S,A,B,drop", [(256, 12, 3, 0.0), (256, 2, 2, 0.1), (512, 3, 2, 0.1), (768, 1, 1, 0.2)])
def test_attention_backward_key_resident_equals_two_kernel_form(ops, S, A, B, drop):
    """The key-resident one-pass backward (one workgroup per 256-key block; S^T / dP^T with the key on the lane, dK^T and
    dV^T in registers, dQ through LDS -- or through f32 slabs per key block for S > 256) against the two-kernel form on
    the same inputs, masks and dropout seed: the SAME dropout mask (the lanes of a key quad exchange their hashes), the
    same dropped probabilities and dS in bf16, a different summation order only; bitwise reproducible."""
    H = A * 64
    qkv, mask, dctx = _attn_case(B, S, A, seed=S + A)
    dt = torch.bfloat16
    qkv_t, mask_t, dctx_t = dev(qkv.reshape(B * S, 3 * H), dt), dev(mask), dev(dctx.reshape(B * S, H), dt)
    ctx = torch.empty((B * S, H), dtype=dt, device="cuda")
    lse = torch.empty((B, A, S), dtype=torch.float32, device="cuda")
    ops.attention_fwd(qkv_t, mask_t, ctx, lse, B, S, A, drop_p=drop, seed=77)
    outs = []
    for kres in (2, 0):                                   # 2: the key-resident kernel also at S = 256 (it is the default from 512 on)
        ops.set_env("POLUS_ATTN_BWD_KRES", kres)
        ops.set_env("POLUS_ATTN_FUSED", 1 if kres else 0)
        try:
            d = torch.full((B * S, 3 * H), float("nan"), dtype=dt, device="cuda")
            ops.attention_bwd(qkv_t, mask_t, ctx, dctx_t, lse, d, B, S, A, drop_p=drop, seed=77)
            outs.append(host(d).reshape(B, S, 3 * H))
        finally:
            ops.set_env("POLUS_ATTN_BWD_KRES")
            ops.set_env("POLUS_ATTN_FUSED")
    assert not np.isnan(outs[0]).any()
    for nm, sl in (("dq", slice(0, H)), ("dk", slice(H, 2 * H)), ("dv", slice(2 * H, 3 * H))):
        assert_close(outs[0][..., sl], outs[1][..., sl], 1.5e-2, nm)
    ops.set_env("POLUS_ATTN_BWD_KRES", 2)
    try:
        d2 = torch.empty((B * S, 3 * H), dtype=dt, device="cuda")
        ops.attention_bwd(qkv_t, mask_t, ctx, dctx_t, lse, d2, B, S, A, drop_p=drop, seed=77)
        d3 = torch.empty_like(d2)
        ops.attention_bwd(qkv_t, mask_t, ctx, dctx_t, lse, d3, B, S, A, drop_p=drop, seed=77)
        assert torch.equal(d2, d3)
    finally:
        ops.set_env("POLUS_ATTN_BWD_KRES")


def test_attention_no_mask_and_all_masked_row(ops):
    B, S, A = 2, 64, 1
    qkv, mask, _ = _attn_case(B, S, A, 9, full_mask=True)
    ctx_ref, _ = ob.attention_fwd(qkv, ob.additive_mask(mask, np.float64), A)
    ctx = torch.empty((B * S, 64), device="cuda")
    lse = torch.empty((B, A, S), device="cuda")
    ops.attention_fwd(dev(qkv.reshape(B * S, 192), torch.float32), None, ctx, lse, B, S, A)
    assert_close(host(ctx).reshape(B, S, 64), ctx_ref, 5e-5, "no mask")
    # a sample whose mask is all zeros: -10000 on every key is shift-invariant (reference semantics)
    mask[1] = 0
    ctx_ref, _ = ob.attention_fwd(qkv, ob.additive_mask(mask, np.float64), A)
    ops.attention_fwd(dev(qkv.reshape(B * S, 192), torch.float32), dev(mask), ctx, lse, B, S, A)
    # scores sit at -10000 + x: f32 spacing there is ~1e-3, so probabilities carry ~5e-4 relative
    # rounding (the reference's f32 TF path has the same rounding; the oracle is float64)
    assert_close(host(ctx).reshape(B, S, 64), ctx_ref, 2e-3, "all-masked sample")


# ------------------------------------------------------------------------------- LayerNorm / embeddings
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("rows,H", [(37, 128), (1000, 768), (64, 1024), (5, 2048), (3, 64)])
def test_layernorm(ops, dtype, rows, H):
    r = rng(rows + H)
    x = r.standard_normal((rows, H)) * 2 + 0.5
    g, b = 1 + 0.1 * r.standard_normal(H), 0.1 * r.standard_normal(H)
    dy = r.standard_normal((rows, H))
    xr, dyr = rounded(x, dtype), rounded(dy, dtype)
    y_ref, mean_ref, rstd_ref = ob.layer_norm_fwd(xr, g.astype(np.float32).astype(np.float64), b.astype(np.float32).astype(np.float64), 1e-12)
    x_t, g_t, b_t = dev(x, dtype), dev(g, torch.float32), dev(b, torch.float32)
    y = torch.empty_like(x_t)
    mean = torch.empty(rows, device="cuda")
    rstd = torch.empty(rows, device="cuda")
    ops.layernorm_fwd(x_t, g_t, b_t, y, mean, rstd, 1e-12)
    tol = TOL[dtype]
    assert_close(host(y), y_ref, tol, "ln y")
    assert_close(host(mean), mean_ref, 1e-5, "mean")
    assert_close(host(rstd), rstd_ref, 1e-5, "rstd")
    dx_ref, dg_ref, db_ref = ob.layer_norm_bwd(dyr, xr, host(g_t), mean_ref, rstd_ref)
    dx = torch.empty_like(x_t)
    dg = torch.full((H,), float("nan"), device="cuda")
    db = torch.full((H,), float("nan"), device="cuda")
    dbias = torch.full((H,), float("nan"), device="cuda")
    ops.layernorm_bwd(dev(dy, dtype), x_t, g_t, mean, rstd, dx, dg, db, dbias)
    assert_close(host(dx), dx_ref, tol, "ln dx")
    assert_close(host(dg), dg_ref, 1e-4, "dgamma")
    assert_close(host(db), db_ref, 1e-4, "dbeta")
    assert_close(host(dbias), host(dx).sum(0), 1e-4 if dtype == torch.float32 else 2e-2, "dbias")
    # accumulate
    ops.layernorm_bwd(dev(dy, dtype), x_t, g_t, mean, rstd, dx, dg, db, None, accumulate=True)
    assert_close(host(dg), 2 * dg_ref, 1e-4, "dgamma accumulate")


# y = xhat * g + b cancels to ~1e-6 in a few elements; there the two kernels' f32 values (which differ by an f32
# eps of the O(1) terms, 3.7e-8 at most observed) straddle many bf16 ulps of the tiny result.  Two f32 eps of 1.0.
LN_F32_FLOOR = 2.5e-7


@pytest.mark.parametrize("rows,H", [(4096, 1024), (4096, 768), (4098, 512), (16, 256)])
def test_layernorm_halfwave_vs_wave_per_row(ops, rows, H):
    """The half-wave-per-row bf16 kernels (norm.hip, 16-byte accesses) against the wave-per-row ones on the same
    input: forward and backward outputs may differ only where the different summation order moved a value across a
    bf16 rounding boundary (one ulp, a few elements per million), and both sit equally far from the oracle."""
    r = rng(rows * 3 + H)
    x = r.standard_normal((rows, H)) * 2 + 0.5
    g, b = 1 + 0.1 * r.standard_normal(H), 0.1 * r.standard_normal(H)
    dy = r.standard_normal((rows, H))
    dt = torch.bfloat16
    xr, dyr = rounded(x, dt), rounded(dy, dt)
    g64, b64 = g.astype(np.float32).astype(np.float64), b.astype(np.float32).astype(np.float64)
    y_ref, mean_ref, rstd_ref = ob.layer_norm_fwd(xr, g64, b64, 1e-12)
    dx_ref, dg_ref, db_ref = ob.layer_norm_bwd(dyr, xr, g64, mean_ref, rstd_ref)
    x_t, dy_t, g_t, b_t = dev(x, dt), dev(dy, dt), dev(g, torch.float32), dev(b, torch.float32)
    got = {}
    try:
        for hw in (0, 1):
            ops.set_env("POLUS_LN_HALFWAVE", hw)
            y = torch.full_like(x_t, float("nan"))
            mean, rstd = torch.empty(rows, device="cuda"), torch.empty(rows, device="cuda")
            ops.layernorm_fwd(x_t, g_t, b_t, y, mean, rstd, 1e-12)
            dx = torch.full_like(x_t, float("nan"))
            dg, db, dbias = (torch.full((H,), float("nan"), device="cuda") for _ in range(3))
            ops.layernorm_bwd(dy_t, x_t, g_t, mean, rstd, dx, dg, db, dbias)
            assert_close(host(y), y_ref, TOL[dt], f"y (halfwave={hw})")
            assert_close(host(dx), dx_ref, TOL[dt], f"dx (halfwave={hw})")
            assert_close(host(mean), mean_ref, 1e-5, "mean"); assert_close(host(rstd), rstd_ref, 1e-5, "rstd")
            assert_close(host(dg), dg_ref, 1e-4, "dgamma"); assert_close(host(db), db_ref, 1e-4, "dbeta")
            got[hw] = (host(y), host(dx))
    finally:
        ops.set_env("POLUS_LN_HALFWAVE")
    for name, a, c, ref in (("y", got[0][0], got[1][0], y_ref), ("dx", got[0][1], got[1][1], dx_ref)):
        differ = a != c
        assert differ.mean() < 1e-4, (name, differ.mean())
        if differ.any():   # one bf16 ulp = 2^-7 relative at most
            d, mag = np.abs(a - c)[differ], np.abs(a)[differ]
            bad = d > mag * 2.0 ** -7 + LN_F32_FLOOR
            assert not bad.any(), (name, list(zip(a[differ][bad][:8], c[differ][bad][:8], ref[differ][bad][:8])))
        ea, ec = np.sqrt(((a - ref) ** 2).mean()), np.sqrt(((c - ref) ** 2).mean())
        assert abs(ea - ec) < 1e-2 * ea, (name, ea, ec)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("deterministic", [False, True])
def test_embeddings(ops, dtype, deterministic):
    cfg = ob.BertConfig(vocab_size=300, hidden_size=128, max_position_embeddings=64)
    B, S = 5, 40
    r = rng(21)
    p = {k: v.astype(np.float64) for k, v in ob.init_params(cfg, with_embeddings=True).items() if k.startswith("emb")}
    p["emb.ln.g"] = p["emb.ln.g"] + 0.1 * r.standard_normal(128)
    p["emb.ln.b"] = 0.1 * r.standard_normal(128)
    p = {k: v.astype(np.float32).astype(np.float64) for k, v in p.items()}
    ids = r.integers(0, 300, size=(B, S)).astype(np.int32)
    ids[:, 30:] = 0  # heavy duplicates (padding id)
    tt = r.integers(0, 2, size=(B, S)).astype(np.int32)
    y_ref, cache = ob.embeddings_fwd(p, cfg, ids, tt)
    t = {k: dev(v, torch.float32) for k, v in p.items()}
    y = torch.empty((B * S, 128), dtype=dtype, device="cuda")
    mean = torch.empty(B * S, device="cuda")
    rstd = torch.empty(B * S, device="cuda")
    ops.embed_ln_fwd(dev(ids), dev(tt), t["emb.word"], t["emb.pos"], t["emb.type"], t["emb.ln.g"], t["emb.ln.b"],
                     y, mean, rstd, 1e-12)
    assert_close(host(y).reshape(B, S, 128), y_ref, TOL[dtype], "embed y")
    dy = r.standard_normal((B, S, 128))
    g_ref = ob.embeddings_bwd(rounded(dy, dtype), p, cfg, cache)
    gw = torch.full_like(t["emb.word"], float("nan"))
    gp = torch.full_like(t["emb.pos"], float("nan"))
    gt = torch.full_like(t["emb.type"], float("nan"))
    gg = torch.full((128,), float("nan"), device="cuda")
    gb = torch.full((128,), float("nan"), device="cuda")
    args = (dev(dy.reshape(B * S, 128), dtype), dev(ids), dev(tt), t["emb.word"], t["emb.pos"], t["emb.type"],
            t["emb.ln.g"], mean, rstd, gw, gp, gt, gg, gb)
    ops.embed_ln_bwd(*args, deterministic=deterministic)
    for nm, got in (("emb.word", gw), ("emb.pos", gp), ("emb.type", gt), ("emb.ln.g", gg), ("emb.ln.b", gb)):
        assert_close(host(got), g_ref[nm], 1e-4, nm)
    if deterministic:
        first = gw.clone()
        ops.embed_ln_bwd(*args, deterministic=True)
        assert torch.equal(first, gw)
    ops.embed_ln_bwd(*args, accumulate=True, deterministic=deterministic)
    assert_close(host(gw), 2 * g_ref["emb.word"], 1e-4, "word accumulate")
    assert_close(host(gt), 2 * g_ref["emb.type"], 1e-4, "type accumulate")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("rows,cols", [(1000, 768), (33, 10), (4096, 2304)])
def test_colsum(ops, dtype, rows, cols):
    x = rng(rows).standard_normal((rows, cols))
    out = torch.full((cols,), float("nan"), device="cuda")
    ops.colsum(dev(x, dtype), out)
    assert_close(host(out), rounded(x, dtype).sum(0), 1e-4, "colsum")
    ops.colsum(dev(x, dtype), out, accumulate=True)
    assert_close(host(out), 2 * rounded(x, dtype).sum(0), 1e-4, "colsum accumulate")


# ------------------------------------------------------------------------------- losses
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("rows,C", [(64, 4), (1000, 10), (3, 3)])
def test_softmax_xent(ops, dtype, rows, C):
    r = rng(rows + C)
    logits = (r.standard_normal((rows, C)) * 3).astype(np.float32)
    labels = r.integers(0, C, size=rows).astype(np.int32)
    loss_ref, d_ref = ol.sparse_softmax_xent_fwd(logits.astype(np.float64), labels)
    loss = torch.empty(1, device="cuda")
    d = torch.empty((rows, C), dtype=dtype, device="cuda")
    ops.softmax_xent(dev(logits), dev(labels), loss, d)
    assert abs(float(loss) - loss_ref) < 1e-5 * max(1, abs(loss_ref))
    assert_close(host(d), d_ref, 1e-5 if dtype == torch.float32 else 1e-2, "dlogits")
    cw = r.uniform(0.5, 2.0, size=C)
    onehot = np.eye(C)[labels]
    loss_ref, d_ref = ol.weighted_softmax_xent_fwd(cw, onehot, logits.astype(np.float64))
    ops.softmax_xent(dev(logits), dev(labels), loss, d, class_weights=dev(cw, torch.float32))
    assert abs(float(loss) - loss_ref) < 1e-5 * max(1, abs(loss_ref))
    assert_close(host(d), d_ref, 1e-5 if dtype == torch.float32 else 1e-2, "weighted dlogits")


def test_sigmoid_xent(ops):
    rows, C = 200, 5
    r = rng(8)
    logits = (r.standard_normal((rows, C)) * 2).astype(np.float32)
    y = (r.uniform(size=(rows, C)) < 0.3).astype(np.float32)
    y[:20] = 0
    cw = r.uniform(0.5, 2.0, size=C)
    loss_ref, d_ref = ol.weighted_sigmoid_xent_fwd(cw, 0.3, y.astype(np.float64), logits.astype(np.float64))
    loss = torch.empty(1, device="cuda")
    d = torch.empty((rows, C), device="cuda")
    ops.sigmoid_xent(dev(logits), dev(y), dev(cw, torch.float32), 0.3, loss, d)
    assert abs(float(loss) - loss_ref) < 1e-5 * max(1, abs(loss_ref))
    assert_close(host(d), d_ref, 1e-5, "sigmoid dlogits")


@pytest.mark.parametrize("B,S,C", [(4, 12, 3), (7, 50, 4), (2, 1, 5)])
def test_crf(ops, B, S, C):
    r = rng(B + S + C)
    pot = r.standard_normal((B, S, C)).astype(np.float32)
    tags = r.integers(0, C, size=(B, S)).astype(np.int32)
    lengths = r.integers(1, S + 1, size=B).astype(np.int32)
    lengths[0] = S
    trans = (r.standard_normal((C, C)) * 0.5).astype(np.float32)
    onehot = np.eye(C)[tags]
    sw = r.uniform(0.5, 1.5, size=B).astype(np.float32)
    for weights in (None, sw):
        loss_ref, dx_ref, dT_ref = ol.crf_nll_fwd(onehot, pot, lengths, trans, None, weights)
        loss = torch.empty(1, device="cuda")
        dpot = torch.full((B, S, C), float("nan"), device="cuda")
        dT = torch.full((C, C), float("nan"), device="cuda")
        ops.crf_nll(dev(pot), dev(tags), dev(lengths), dev(trans), None if weights is None else dev(weights), loss, dpot, dT)
        assert abs(float(loss) - loss_ref) < 2e-5 * max(1, abs(loss_ref))
        assert_close(host(dpot), dx_ref, 1e-4, "crf dpot")  # f32 alpha/beta scans of length S vs float64 oracle
        assert_close(host(dT), dT_ref, 2e-4, "crf dtrans")
    dec_ref = ol.crf_viterbi(pot, lengths, trans)
    dec = torch.empty((B, S), dtype=torch.int32, device="cuda")
    ops.crf_viterbi(dev(pot), dev(lengths), dev(trans), dec)
    assert np.array_equal(dec.cpu().numpy(), dec_ref)


def test_argmax(ops):
    x = rng(4).standard_normal((300, 7)).astype(np.float32)
    x[5, 2] = x[5, 4] = 9.0  # tie -> first index
    out = torch.empty(300, dtype=torch.int32, device="cuda")
    ops.argmax(dev(x), out)
    assert np.array_equal(out.cpu().numpy(), x.argmax(-1))


# ------------------------------------------------------------------------------- optimizer
def test_adam_matches_oracle(ops):
    r = rng(13)
    sizes = [("a.w", 1000), ("a.b", 37), ("ln.g", 64), ("c.w", 4099)]
    params = {k: r.standard_normal(n).astype(np.float32) for k, n in sizes}
    opt = oo.Adam(lr=lambda t: oo.warmup_linear_lr(t, 10, 1e-2), weight_decay=0.01,
                  no_decay=[k for k, _ in sizes if oo.is_no_decay(k)])
    n = sum(s for _, s in sizes)
    flat = np.concatenate([params[k] for k, _ in sizes])
    p = dev(flat)
    m, v = torch.zeros_like(p), torch.zeros_like(p)
    shadow = torch.zeros(n, dtype=torch.bfloat16, device="cuda")
    seg, off = [], 0
    for k, s in sizes:
        flags = (0 if oo.is_no_decay(k) else 1) | (2 if k.endswith(".w") else 0)
        for b in range(off, off + s, 1 << 14):
            seg.append((b, min(off + s, b + (1 << 14)), flags))
        off += s
    seg_t = dev(np.array(seg, np.int64))
    for step in range(4):
        grads = {k: r.standard_normal(s).astype(np.float32) for k, s in sizes}
        lr = oo.warmup_linear_lr(step, 10, 1e-2)
        t = step + 1
        lr_t = lr * math.sqrt(1 - 0.999 ** t) / (1 - 0.9 ** t)
        g = dev(np.concatenate([grads[k] for k, _ in sizes]))
        ops.adam_step(p, g, m, v, shadow, seg_t, len(seg), lr, lr_t, 0.9, 0.999, 1e-7, 0.01)
        opt.step(params, grads)
    ref = np.concatenate([params[k] for k, _ in sizes])
    assert_close(host(p), ref, 2e-6, "adam params")
    sh = host(shadow)
    assert_close(sh[:1000], rounded(ref[:1000], torch.bfloat16), 1e-6, "bf16 shadow")
    assert np.all(sh[1000:1101] == 0)  # no shadow for biases / LN


def test_sqnorm_clip_cast_scale(ops):
    r = rng(17)
    g = r.standard_normal(100003).astype(np.float32)
    g_t = dev(g)[:100003]
    sq = torch.empty(1, device="cuda")
    ops.sqnorm(g_t, sq)
    assert abs(float(sq) - float((g.astype(np.float64) ** 2).sum())) < 1e-3 * float(sq)
    sc = torch.empty(1, device="cuda")
    ops.clip_scale(sq, 0.5, 1.0, sc)
    norm = math.sqrt(float((g.astype(np.float64) ** 2).sum())) * 0.5
    assert abs(float(sc) - 1.0 / max(norm, 1.0)) < 1e-6
    b = torch.empty(100003, dtype=torch.bfloat16, device="cuda")
    ops.cast(g_t, b)
    assert torch.equal(b, g_t.to(torch.bfloat16))
    ops.scale_(g_t, 0.25)
    assert_close(host(g_t), g * 0.25, 1e-7, "scale")


# ------------------------------------------------------------------------------- direct-to-LDS GEMMs (ring / ping-pong, chosen per shape)
@pytest.mark.parametrize("M,N,K", [(256, 256, 64), (256, 256, 128), (512, 768, 768), (300, 200, 72), (1000, 520, 264),
                                   (257, 193, 8), (2048, 3072, 768), (1024, 768, 3072)])
def test_gemm_lds_dma_matches_reference_and_v1(ops, M, N, K, monkeypatch):
    r = rng(M + N + K)
    A, B = r.standard_normal((M, K)), r.standard_normal((N, K))
    a_t, b_t = dev(A, torch.bfloat16), dev(B, torch.bfloat16)
    ref = rounded(A, torch.bfloat16) @ rounded(B, torch.bfloat16).T
    out = torch.full((M, N), float("nan"), dtype=torch.bfloat16, device="cuda")
    ops.gemm(a_t, b_t, out)
    assert_close(host(out), ref, TOL[torch.bfloat16], f"gemm256 {M}x{N}x{K}")
    o32 = torch.full((M, N), float("nan"), dtype=torch.float32, device="cuda")
    ops.gemm(a_t, b_t, o32)
    assert_close(host(o32), ref, 2e-5 * max(1, K / 64), "gemm256 f32 out")
    ops.set_env("POLUS_GEMM_V1", "1")
    o1 = torch.empty_like(o32)
    ops.gemm(a_t, b_t, o1)
    ops.set_env("POLUS_GEMM_V1")
    assert_close(host(o32), host(o1), 1e-5, "gemm256 vs 128x128 kernel")
    # run-to-run bitwise identical (no atomics, fixed k order)
    o2 = torch.empty_like(o32)
    ops.gemm(a_t, b_t, o2)
    assert torch.equal(o32, o2)


def test_gemm_lds_dma_epilogues_and_identity(ops):
    M, N, K = 384, 256, 192
    r = rng(77)
    A, B = r.standard_normal((M, K)), r.standard_normal((N, K)) * 0.2
    bias, R = r.standard_normal(N), r.standard_normal((M, N))
    dt = torch.bfloat16
    a_t, b_t, bias_t, r_t = dev(A, dt), dev(B, dt), dev(bias, torch.float32), dev(R, dt)
    base = rounded(A, dt) @ rounded(B, dt).T
    out = torch.empty((M, N), dtype=dt, device="cuda")
    aux = torch.empty((M, N), dtype=dt, device="cuda")
    ops.gemm(a_t, b_t, out, bias=bias_t, resid=r_t)
    assert_close(host(out), base + bias + rounded(R, dt), TOL[dt], "bias+resid")
    ops.gemm(a_t, b_t, out, bias=bias_t, aux=aux, act="gelu", flags=ops.GEMM_ACT_FWD)
    assert_close(host(aux), base + bias, TOL[dt], "aux")
    assert_close(host(out), ob.gelu(base + bias), TOL[dt], "gelu")
    ops.gemm(a_t, b_t, out, aux=aux, act="gelu", flags=ops.GEMM_ACT_BWD, resid=r_t)
    assert_close(host(out), base * ob.gelu_grad(host(aux)) + rounded(R, dt), TOL[dt], "act bwd + resid")
    # A = I with an asymmetric B: catches any row/col or swizzle mix-up exactly
    n = 256
    Bm = (np.arange(n)[:, None] * 3 + np.arange(n)[None, :] % 7).astype(np.float64) / 64.0
    o = torch.zeros((n, n), dtype=dt, device="cuda")
    ops.gemm(dev(np.eye(n), dt), dev(Bm, dt), o)
    assert np.array_equal(host(o), rounded(Bm, dt).T)


def test_transposed_shadow_dx(ops):
    """bf16 engine: dX = dY . W reads the transposed weight shadow, refreshed for all matrices by
    one batched launch (ragged 64x64 tiles, several matrices at different arena offsets)."""
    from polus_amd.layers import gemm_dx
    from polus_amd.tensor import ParamArena
    arena = ParamArena(torch.bfloat16)
    r = rng(31)
    W = r.standard_normal((320, 256)) * 0.1
    others = [arena.add("a", (70, 130), r.standard_normal((70, 130)).astype(np.float32), matrix=True),
              arena.add("bias", (130,), np.zeros(130, np.float32))]
    w = arena.add("w", (320, 256), W.astype(np.float32), matrix=True)
    others.append(arena.add("z", (33, 5), r.standard_normal((33, 5)).astype(np.float32), matrix=True))
    arena.finalize()
    for v in [others[0], w, others[2]]:
        assert torch.equal(v.compute_t, v.compute.t().contiguous()), v.name
    assert others[1].compute_t is None
    dY = r.standard_normal((512, 320))
    dx = torch.empty((512, 256), dtype=torch.bfloat16, device="cuda")
    gemm_dx(dev(dY, torch.bfloat16), w, dx)
    assert_close(host(dx), rounded(dY, torch.bfloat16) @ rounded(W.astype(np.float32), torch.bfloat16), TOL[torch.bfloat16], "dx via W^T shadow")
    w.assign(W.astype(np.float32) * 2)
    assert torch.equal(w.compute_t, w.compute.t().contiguous())


@pytest.mark.parametrize("T,N,K,splits", [(4096, 768, 768, (1, 4, 7)), (1000, 304, 136, (1, 3)), (2048, 2304, 768, (5,)),
                                           (8192, 768, 3072, (8,)), (64, 256, 128, (1, 2))])
def test_gemm_ring_dw_k_strided(ops, T, N, K, splits, monkeypatch):
    """dW = dY^T X on the ring kernel: k-major LDS images + transposing LDS reads + split-K slabs."""
    r = rng(T + N + K)
    dY, X = r.standard_normal((T, N)) * 0.1, r.standard_normal((T, K))
    dt = torch.bfloat16
    dy_t, x_t = dev(dY, dt), dev(X, dt)
    ref = rounded(dY, dt).T @ rounded(X, dt)
    for sk in splits:
        out = torch.full((N, K), float("nan"), dtype=torch.float32, device="cuda")
        ops.gemm(dy_t, x_t, out, a_layout=1, b_layout=1, split_k=sk)
        assert_close(host(out), ref, 2e-3, f"ring dW split_k={sk}")
        o2 = torch.empty_like(out)
        ops.gemm(dy_t, x_t, o2, a_layout=1, b_layout=1, split_k=sk)
        assert torch.equal(out, o2), "split-K reduction must be bitwise reproducible"
        ops.set_env("POLUS_GEMM_V1", "1")
        o1 = torch.empty_like(out)
        ops.gemm(dy_t, x_t, o1, a_layout=1, b_layout=1, split_k=sk)
        ops.set_env("POLUS_GEMM_V1")
        assert_close(host(out), host(o1), 2e-5, "ring vs 128x128 kernel")
    # accumulate + alpha through the split-K reduce kernel
    base = r.standard_normal((N, K)).astype(np.float32)
    acc = dev(base)
    ops.gemm(dy_t, x_t, acc, a_layout=1, b_layout=1, split_k=splits[-1], alpha=0.5, flags=ops.GEMM_ACCUM_C)
    assert_close(host(acc), 0.5 * ref + base, 2e-3, "ring dW accumulate")


@pytest.mark.parametrize("M,N,K", [(512, 768, 2304), (300, 136, 72), (2048, 3072, 768), (256, 128, 32)])
def test_gemm_ring_mixed_layouts(ops, M, N, K, monkeypatch):
    """dX = dY . W with W[out=K, in=N] as the K-strided B operand (and the mirrored A-strided form)."""
    r = rng(M * 3 + N + K)
    A, B = r.standard_normal((M, K)), r.standard_normal((N, K)) * 0.1
    dt = torch.bfloat16
    ref = rounded(A, dt) @ rounded(B, dt).T
    for al, bl in ((0, 1), (1, 0)):
        a_t, b_t = dev(_layout(A, al), dt), dev(_layout(B, bl), dt)
        out = torch.full((M, N), float("nan"), dtype=dt, device="cuda")
        ops.gemm(a_t, b_t, out, a_layout=al, b_layout=bl)
        assert_close(host(out), ref, TOL[dt], f"ring mixed {al}{bl}")
        ops.set_env("POLUS_GEMM_V1", "1")
        o1 = torch.empty_like(out)
        ops.gemm(a_t, b_t, o1, a_layout=al, b_layout=bl)
        ops.set_env("POLUS_GEMM_V1")
        assert_close(host(out), host(o1), 1e-2, "ring vs 128x128")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("T,n_out,n_in,sk", [(4096, 768, 768, 7), (2048, 2304, 768, 3), (1000, 304, 136, 2),
                                            (512, 10, 128, 1), (4096, 3072, 768, 1)])
def test_dense_bwd_params(ops, dtype, T, n_out, n_in, sk):
    """dW and db in one pass (bias gradient on the matrix pipe for the bf16 ring kernel)."""
    r = rng(T + n_out + n_in)
    dY, X = r.standard_normal((T, n_out)) * 0.1, r.standard_normal((T, n_in))
    dy_t, x_t = dev(dY, dtype), dev(X, dtype)
    dw = torch.full((n_out, n_in), float("nan"), device="cuda")
    db = torch.full((n_out,), float("nan"), device="cuda")
    ops.dense_bwd_params(dy_t, x_t, dw, db, split_k=sk)
    tol = 3e-5 if dtype == torch.float32 else 2e-3
    assert_close(host(dw), rounded(dY, dtype).T @ rounded(X, dtype), tol, "dW")
    assert_close(host(db), rounded(dY, dtype).sum(0), 1e-4 if dtype == torch.float32 else 2e-3, "db")
    w0, b0 = dw.clone(), db.clone()
    ops.dense_bwd_params(dy_t, x_t, dw, db, accumulate=True, split_k=sk)
    assert_close(host(dw), 2 * host(w0), 1e-6, "dW accumulate")
    assert_close(host(db), 2 * host(b0), 1e-6, "db accumulate")


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("rows,H,C", [(16384, 768, 4), (1000, 1024, 8), (37, 128, 1), (513, 264, 3), (2048, 768, 5)])
def test_dense_thin(ops, dt, rows, H, C):
    """The wave-per-row kernels of a Dense with at most 8 units (a classification head): forward, and the one-pass backward
    (dx, dW, db) against NumPy on the rounded operands; f32 and compute-dtype dy; dx skipped; accumulate; reproducible."""
    if not ops.dense_thin_supported(dt, H, C):
        pytest.skip("shape outside the thin kernels")
    r = rng(rows + H + C)
    X, W, b = r.standard_normal((rows, H)), r.standard_normal((C, H)) * 0.1, r.standard_normal(C)
    dY = r.standard_normal((rows, C)) * 0.1
    x_t, w_t, b_t = dev(X, dt), dev(W, dt), dev(b, torch.float32)
    Xr, Wr = rounded(X, dt), rounded(W, dt)
    for ydt in (torch.float32, dt):
        y = torch.full((rows, C), float("nan"), dtype=ydt, device="cuda")
        ops.dense_thin_fwd(x_t, w_t, b_t, y)
        assert_close(host(y), Xr @ Wr.T + b, 2e-2 if ydt == torch.bfloat16 else 2e-5, "thin forward")
    tol = 2e-2 if dt == torch.bfloat16 else 2e-5
    for dydt in (torch.float32, dt):
        dy_t = dev(dY, dydt)
        dYr = rounded(dY, dydt)
        dx = torch.full((rows, H), float("nan"), dtype=dt, device="cuda")
        dw, db = torch.full((C, H), float("nan"), device="cuda"), torch.full((C,), float("nan"), device="cuda")
        ops.dense_thin_bwd(x_t, dy_t, w_t, dx, dw, db)
        assert_close(host(dx), dYr @ Wr, tol, "thin dx")
        assert_close(host(dw), dYr.T @ Xr, 2e-5, "thin dW")
        assert_close(host(db), dYr.sum(0), 2e-5, "thin db")
        dw2, db2 = torch.full_like(dw, float("nan")), torch.full_like(db, float("nan"))
        ops.dense_thin_bwd(x_t, dy_t, w_t, None, dw2, db2)
        assert torch.equal(dw, dw2) and torch.equal(db, db2), "thin backward is not reproducible / depends on dx"
        ops.dense_thin_bwd(x_t, dy_t, w_t, None, dw2, None, accumulate=True)
        assert_close(host(dw2), 2 * host(dw), 1e-6, "thin dW accumulate")


@pytest.mark.parametrize("T,shapes", [
    (16384, [(768, 3072), (3072, 768), (768, 768), (2304, 768)]),      # BERT-base layer: 108 tiles, 2 slices + 40 remainder workgroups
    (4096, [(768, 3072), (3072, 768), (768, 768), (2304, 768)]),       # 64 K-tiles: short slices, parts of one or two K-tiles
    (8192, [(1024, 4096), (4096, 1024), (1024, 1024), (3072, 1024)]),  # BERT-large layer: 192 tiles, 1 slice + 64 remainder workgroups
    (2048, [(640, 768), (768, 328), (256, 256)]),                      # ragged edge tiles
])
def test_dense_bwd_params_grouped_streamk(ops, T, shapes):
    """The grouped dW launch with a stream-K remainder (POLUS_DW_STREAMK=1: the CUs the even K split leaves idle take
    equal runs of the K-tiles the regular slices are shortened by): against dY^T X, against the even split, bitwise
    reproducible, accumulate, null db."""
    r = rng(T + len(shapes))
    dt = torch.bfloat16
    probs, refs = [], []
    for k, (n_out, n_in) in enumerate(shapes):
        dY, X = r.standard_normal((T, n_out)) * 0.1, r.standard_normal((T, n_in))
        dw = torch.full((n_out, n_in), float("nan"), device="cuda")
        db = torch.full((n_out,), float("nan"), device="cuda") if k % 2 else None
        probs.append((dev(dY, dt), dev(X, dt), dw, db))
        refs.append((rounded(dY, dt).T @ rounded(X, dt), rounded(dY, dt).sum(0)))
    even = [(torch.full_like(p[2], float("nan")), None if p[3] is None else torch.full_like(p[3], float("nan"))) for p in probs]
    ops.dense_bwd_params_grouped([(p[0], p[1], a[0], a[1]) for p, a in zip(probs, even)], False, 0)
    ops.set_env("POLUS_DW_STREAMK", 1)
    try:
        ops.dense_bwd_params_grouped(probs, False, 0)
        for (dy, x, dw, db), (rw, rb), (ew, eb) in zip(probs, refs, even):
            assert_close(host(dw), rw, 2e-3, "stream-K dW")
            assert_close(host(dw), host(ew), 1e-5, "stream-K vs even split")
            if db is not None:
                assert_close(host(db), rb, 2e-3, "stream-K db")
                assert_close(host(db), host(eb), 1e-5, "stream-K vs even split db")
        first = [(p[2].clone(), None if p[3] is None else p[3].clone()) for p in probs]
        for p in probs:
            p[2].fill_(float("nan"))
        ops.dense_bwd_params_grouped(probs, False, 0)
        for (dy, x, dw, db), (w0, b0) in zip(probs, first):
            assert torch.equal(dw, w0) and (db is None or torch.equal(db, b0)), "stream-K split is not reproducible"
        ops.dense_bwd_params_grouped(probs, True, 0)
        for (dy, x, dw, db), (w0, b0) in zip(probs, first):
            assert_close(host(dw), 2 * host(w0), 1e-6, "stream-K dW accumulate")
            if db is not None:
                assert_close(host(db), 2 * host(b0), 1e-6, "stream-K db accumulate")
    finally:
        ops.set_env("POLUS_DW_STREAMK")


@pytest.mark.parametrize("tn", [256, 192])
@pytest.mark.parametrize("M,N,K", [(1024, 3072, 768), (1280, 2304, 320), (1032, 2200, 64), (2048, 3072, 768), (2000, 3072, 320)])
def test_gemm_pingpong_persistent_equals_per_tile(ops, tn, M, N, K):
    """gemm_ppp_kernel (one workgroup per CU walks several tiles, the next tile's operand prologue issued before the current
    epilogue) against the one-workgroup-per-tile launch: same MFMA order, same epilogue arithmetic -- bit-identical, for
    every epilogue mode, odd and even K-tile counts, ragged edges.  POLUS_GEMM_RESERVE_CUS shrinks the grid to 32
    workgroups so that these small problems take 2-3 tiles each; POLUS_GEMM_PERSIST=2 selects the form for every mode."""
    r = rng(M + N + K)
    dt = torch.bfloat16
    a_t, b_t = dev(r.standard_normal((M, K)), dt), dev(r.standard_normal((N, K)) * 0.1, dt)
    bias_t, r_t, u_t = dev(r.standard_normal(N), torch.float32), dev(r.standard_normal((M, N)), dt), dev(r.standard_normal((M, N)), dt)
    # ACT_FWD without an aux buffer (inference, the frozen dual-encoder towers) issues half the epilogue stores of the
    # training forward; with no bias either nothing else waits for the next tile's operand prologue but the counted
    # vmcnt at the head of its K loop (round-3 advisor finding: that count must not exceed the stores really issued)
    cases = [dict(bias=bias_t), dict(bias=bias_t, aux="new", act="gelu", flags=ops.GEMM_ACT_FWD), dict(resid=r_t),
             dict(bias=bias_t, resid=r_t, drop_p=0.1, seed=11), dict(aux=u_t, act="gelu", flags=ops.GEMM_ACT_BWD),
             dict(bias=bias_t, act="gelu", flags=ops.GEMM_ACT_FWD), dict(act="gelu", flags=ops.GEMM_ACT_FWD)]
    ops.set_env("POLUS_GEMM_PP", tn)
    ops.set_env("POLUS_GEMM_RESERVE_CUS", 224)
    try:
        for kw in cases:
            outs = []
            for pers in (2, 0):
                ops.set_env("POLUS_GEMM_PERSIST", pers)
                out = torch.full((M, N), float("nan"), dtype=dt, device="cuda")
                kw2 = dict(kw)
                if kw2.get("aux") == "new":
                    kw2["aux"] = torch.full((M, N), float("nan"), dtype=dt, device="cuda")
                route = ops.gemm_route(a_t, b_t, out, **kw2)
                assert (route.kernel, route.tn) == ("pp_persist" if pers else "pp", tn), (sorted(kw), route)
                ops.gemm(a_t, b_t, out, **kw2)
                outs.append((out, kw2.get("aux")))
            assert not torch.isnan(outs[0][0].float()).any()
            for o in outs[1:]:
                assert torch.equal(outs[0][0], o[0]), sorted(kw)
                if kw.get("aux") == "new":
                    assert torch.equal(outs[0][1], o[1])
    finally:
        ops.set_env("POLUS_GEMM_PP"); ops.set_env("POLUS_GEMM_RESERVE_CUS"); ops.set_env("POLUS_GEMM_PERSIST")


@pytest.mark.parametrize("tn", [256, 192])
@pytest.mark.parametrize("M,N,K", [(512, 768, 768), (256, 256, 64), (256, 192, 128), (520, 456, 192), (1024, 2304, 320),
                                   (768, 3072, 3072)])
def test_gemm_pingpong_256wide(ops, tn, M, N, K):
    """gemm_pp.hip (256 x 256 / 256 x 192 tile, two staggered wave groups): every epilogue mode, one /
    two / three / many K-tiles (the three tail variants of the load schedule), interior and ragged
    tiles, against the oracle arithmetic and bit-for-bit against the ring kernel (same MFMA k-order,
    same epilogue)."""
    r = rng(M + 7 * N + K + tn)
    A, B = r.standard_normal((M, K)), r.standard_normal((N, K)) * 0.1
    bias, R, U = r.standard_normal(N), r.standard_normal((M, N)), r.standard_normal((M, N))
    dt = torch.bfloat16
    a_t, b_t, bias_t, r_t, u_t = dev(A, dt), dev(B, dt), dev(bias, torch.float32), dev(R, dt), dev(U, dt)
    base = rounded(A, dt) @ rounded(B, dt).T
    tol = TOL[dt]

    def both(**kw):
        outs = []
        try:
            for sel in (tn, -1):
                ops.set_env("POLUS_GEMM_PP", sel)
                out = torch.full((M, N), float("nan"), dtype=dt, device="cuda")
                kw2 = dict(kw)
                if kw2.get("aux") == "new":
                    kw2["aux"] = torch.full((M, N), float("nan"), dtype=dt, device="cuda")
                ops.gemm(a_t, b_t, out, **kw2)
                outs.append((out, kw2.get("aux")))
        finally:
            ops.set_env("POLUS_GEMM_PP")
        assert torch.equal(outs[0][0], outs[1][0]), "ping-pong kernel differs from the ring kernel"
        if outs[0][1] is not None and kw.get("aux") == "new":
            assert torch.equal(outs[0][1], outs[1][1]), "ping-pong kernel: aux differs from the ring kernel"
        return outs[0]

    out, _ = both(bias=bias_t)
    assert_close(host(out), base + bias, tol, "bias")
    out, aux = both(bias=bias_t, aux="new", act="gelu", flags=ops.GEMM_ACT_FWD)
    assert_close(host(aux), base + bias, tol, "aux")
    assert_close(host(out), ob.gelu(base + bias), tol, "gelu")
    out, _ = both(bias=bias_t, resid=r_t)
    assert_close(host(out), base + bias + rounded(R, dt), tol, "bias+resid")
    out, _ = both(aux=u_t, act="gelu", flags=ops.GEMM_ACT_BWD)
    assert_close(host(out), base * ob.gelu_grad(rounded(U, dt)), tol, "gelu bwd")
    out, _ = both(bias=bias_t, resid=r_t, drop_p=0.25, seed=123)
    keep = host(ops.dropout_mask(123, 0.25, M * N)).astype(np.float64).reshape(M, N)
    assert_close(host(out), (base + bias) * keep / 0.75 + rounded(R, dt), tol, "dropout+resid")
    # run-to-run bitwise identical
    ops.set_env("POLUS_GEMM_PP", tn)
    try:
        o1, o2 = torch.empty((M, N), dtype=dt, device="cuda"), torch.empty((M, N), dtype=dt, device="cuda")
        ops.gemm(a_t, b_t, o1, bias=bias_t)
        ops.gemm(a_t, b_t, o2, bias=bias_t)
        assert torch.equal(o1, o2)
    finally:
        ops.set_env("POLUS_GEMM_PP")


@pytest.mark.parametrize("M,N,K,split", [(4096, 768, 3072, 4), (1024, 768, 2304, 3), (512, 1000, 1024, 2)])
def test_split_k_with_full_epilogue(ops, M, N, K, split):
    """bf16 Dense GEMMs that 256-row tiles cannot fill the chip with run their K range in slices (f32 slabs) and a
    reduce kernel applies the WHOLE epilogue (pgemm::epilogue_tile) to the sum: bias, GELU + pre-activation store,
    GELU', dropout, residual.  Against the unsplit kernel (same arithmetic except the f32 summation order of the
    slices: a bf16 ulp at most, on a few elements), against the oracle, and bitwise run to run."""
    r = rng(M + N + K)
    A, B = r.standard_normal((M, K)), r.standard_normal((N, K)) * 0.05
    bias, R, U = r.standard_normal(N), r.standard_normal((M, N)), r.standard_normal((M, N))
    dt = torch.bfloat16
    a_t, b_t, bias_t, r_t, u_t = dev(A, dt), dev(B, dt), dev(bias, torch.float32), dev(R, dt), dev(U, dt)
    base = rounded(A, dt) @ rounded(B, dt).T
    tol = TOL[dt]

    def run(sk, **kw):
        out = torch.full((M, N), float("nan"), dtype=dt, device="cuda")
        kw2 = dict(kw)
        if kw2.get("aux") == "new":
            kw2["aux"] = torch.full((M, N), float("nan"), dtype=dt, device="cuda")
        ops.gemm(a_t, b_t, out, split_k=sk, **kw2)
        return out, kw2.get("aux")

    def both(what, ref, **kw):
        (o1, x1), (os_, xs), (os2, _) = run(1, **kw), run(split, **kw), run(split, **kw)
        assert torch.equal(os_, os2), f"{what}: split path is not reproducible"
        assert_close(host(os_), ref, tol, f"{what} (split) vs oracle")
        d = (os_.float() - o1.float()).abs()
        scale = o1.float().abs().clamp_min(2.0 ** -6)
        assert float((d / scale).max()) <= 2.0 ** -6, f"{what}: split differs from unsplit by more than two bf16 ulps"
        assert float((d > 0).float().mean()) < 0.2, f"{what}: too many elements differ"
        return os_, xs

    both("bias", base + bias, bias=bias_t)
    out, aux = both("gelu", ob.gelu(base + bias), bias=bias_t, aux="new", act="gelu", flags=ops.GEMM_ACT_FWD)
    assert_close(host(aux), base + bias, tol, "pre-activation (split)")
    both("bias+resid", base + bias + rounded(R, dt), bias=bias_t, resid=r_t)
    both("gelu bwd", base * ob.gelu_grad(rounded(U, dt)), aux=u_t, act="gelu", flags=ops.GEMM_ACT_BWD)
    keep = host(ops.dropout_mask(77, 0.25, M * N)).astype(np.float64).reshape(M, N)
    both("dropout+resid", (base + bias) * keep / 0.75 + rounded(R, dt), bias=bias_t, resid=r_t, drop_p=0.25, seed=77)


def test_gemm_auto_split_heuristic(ops):
    """polus_gemm_auto_split: 1 where a 256-wide ping-pong tile fills the chip (the headline shapes), where K < 2048, and
    wherever the 128 x 128 ring tile fills more than an eighth of its slots (it beats slicing there and writes no
    slabs); slices, each at least 768 deep, only for about two thousand tokens and fewer."""
    from polus_amd import _lib
    f = _lib.load().polus_gemm_auto_split
    assert [f(16384, n, k) for n, k in ((768, 3072), (3072, 768), (2304, 768), (768, 768))] == [1, 1, 1, 1]
    assert f(4096, 768, 3072) == 1 and f(4096, 768, 2304) == 1 and f(8192, 768, 3072) == 1 and f(4096, 1024, 4096) == 1
    assert f(2048, 768, 3072) == 4 and f(2048, 768, 2304) == 3 and f(1024, 1024, 4096) == 5
    assert f(2048, 768, 768) == 1 and f(2048, 768, 1000) == 1 and f(128, 768, 3072) == 1 and f(4096, 64, 3072) == 1
    try:
        ops.set_env("POLUS_GEMM_RING128", -1)        # without the 128-row tile: the rule measured in the step before it existed
        assert f(4096, 768, 3072) == 4 and f(4096, 768, 2304) == 3 and f(4096, 1024, 4096) == 3
        assert f(6144, 768, 3072) == 1 and f(8192, 768, 3072) == 1
    finally:
        ops.set_env("POLUS_GEMM_RING128")


@pytest.mark.parametrize("M,N,K", [(4096, 768, 2304), (1000, 1000, 1056), (384, 256, 96), (8192, 768, 768)])
def test_gemm_ring128_equals_ring256(ops, M, N, K):
    """The 128 x 128 ring tile (three workgroups per CU; chosen where 256-row tiles would leave most of the chip idle)
    against the 256 x 128 ring tile: same MFMA k order, same epilogue arithmetic -> bit-identical C (and pre-activation)
    in every epilogue mode, ragged edges included; and against the oracle."""
    r = rng(M + 3 * N + K)
    A, B = r.standard_normal((M, K)), r.standard_normal((N, K)) * 0.05
    bias, R, U = r.standard_normal(N), r.standard_normal((M, N)), r.standard_normal((M, N))
    dt = torch.bfloat16
    a_t, b_t, bias_t, r_t, u_t = dev(A, dt), dev(B, dt), dev(bias, torch.float32), dev(R, dt), dev(U, dt)
    base = rounded(A, dt) @ rounded(B, dt).T
    tol = TOL[dt]

    def both(**kw):
        outs = []
        try:
            ops.set_env("POLUS_GEMM_PP", -1)
            for sel in (1, -1):
                ops.set_env("POLUS_GEMM_RING128", sel)
                out = torch.full((M, N), float("nan"), dtype=dt, device="cuda")
                kw2 = dict(kw)
                if kw2.get("aux") == "new":
                    kw2["aux"] = torch.full((M, N), float("nan"), dtype=dt, device="cuda")
                ops.gemm(a_t, b_t, out, split_k=1, **kw2)
                outs.append((out, kw2.get("aux")))
        finally:
            ops.set_env("POLUS_GEMM_RING128"); ops.set_env("POLUS_GEMM_PP")
        assert torch.equal(outs[0][0], outs[1][0]), "128-row ring tile differs from the 256-row one"
        if kw.get("aux") == "new":
            assert torch.equal(outs[0][1], outs[1][1]), "128-row ring tile: pre-activation differs"
        return outs[0]

    out, _ = both(bias=bias_t)
    assert_close(host(out), base + bias, tol, "bias")
    out, aux = both(bias=bias_t, aux="new", act="gelu", flags=ops.GEMM_ACT_FWD)
    assert_close(host(aux), base + bias, tol, "aux"); assert_close(host(out), ob.gelu(base + bias), tol, "gelu")
    out, _ = both(bias=bias_t, resid=r_t)
    assert_close(host(out), base + bias + rounded(R, dt), tol, "bias+resid")
    out, _ = both(aux=u_t, act="gelu", flags=ops.GEMM_ACT_BWD)
    assert_close(host(out), base * ob.gelu_grad(rounded(U, dt)), tol, "gelu bwd")
    out, _ = both(bias=bias_t, resid=r_t, drop_p=0.25, seed=321)
    keep = host(ops.dropout_mask(321, 0.25, M * N)).astype(np.float64).reshape(M, N)
    assert_close(host(out), (base + bias) * keep / 0.75 + rounded(R, dt), tol, "dropout+resid")


def test_dropout_mask_definition_and_statistics(ops):
    """The dropout mask is the engine's own counter-based generator (one murmur3-finaliser hash per FOUR elements,
    polus_amd/csrc/common.h).  Pinned here against a numpy restatement at several offsets (aligned and not, and
    across the 32-bit wrap), and held to the statistics a mask needs -- fixed seeds, so this either passes or not:
    keep rate, serial correlation at the strides tensors have (neighbouring keys, next query row at S = 256 / 257,
    next token row at H = 768, next head), and the six pairings of the fields that share one hash."""
    from tests.util import dropout_keep_np
    for seed, p, idx0, n in ((123, 0.1, 0, 4099), (0xDEADBEEF, 0.25, 5, 1001), (7, 0.5, 2, 64), (99, 0.1, 0xFFFFFFF0 - 100, 90), (1, 0.9, 1 << 30, 513)):
        got = host(ops.dropout_mask(seed, p, n, idx0=idx0)).astype(np.uint8)
        assert np.array_equal(got, dropout_keep_np(seed, p, idx0, n)), (seed, p, idx0)
    N = 1 << 24
    for seed in (0x12345678, 0x5BD1E995):
        k = host(ops.dropout_mask(seed, 0.1, N)).astype(np.float64)
        q = 1.0 - round(0.1 * 65536) / 65536.0
        assert abs(k.mean() - q) / np.sqrt(q * (1 - q) / N) < 4.5, ("keep rate", seed, k.mean())
        kd = k - k.mean()
        var = float((kd * kd).mean())
        for lag in (1, 2, 3, 4, 8, 64, 256, 257, 768, 65536, 65536 * 12):
            z = float(np.dot(kd[:-lag], kd[lag:])) / (N - lag) / var * np.sqrt(N - lag)
            assert abs(z) < 4.5, ("serial correlation", seed, lag, z)
        quad = kd.reshape(-1, 4)
        for a in range(4):
            for b in range(a + 1, 4):
                z = float(np.dot(quad[:, a], quad[:, b])) / (N / 4) / var * np.sqrt(N / 4)
                assert abs(z) < 4.5, ("fields of one hash", seed, a, b, z)
    # two seeds as the host derives them for neighbouring sites / steps give unrelated masks
    a = host(ops.dropout_mask(0x3C6EF372, 0.1, 1 << 22)).astype(np.float64)
    for other in (0x3C6EF373, 0x3C6EF372 ^ 0x9E3779B1, (0x3C6EF372 + 0x85EBCA6B) & 0xFFFFFFFF, (0x3C6EF372 + 9 * 0xC2B2AE35) & 0xFFFFFFFF):
        b = host(ops.dropout_mask(other, 0.1, 1 << 22)).astype(np.float64)
        z = float(np.corrcoef(a, b)[0, 1]) * np.sqrt(1 << 22)
        assert abs(z) < 4.5, ("cross-seed correlation", hex(other), z)


def test_gelu_polynomial_epilogue_precision(ops):
    """The bf16 GEMM epilogues evaluate GELU / GELU' by a degree-10 polynomial in x^2 (no erf, no
    exp): through an identity product the error against the exact erf form must stay below a
    bf16 ulp of the result over the whole range, including the clamped tails."""
    n = 512
    x = np.linspace(-9.0, 9.0, 256 * n).reshape(256, n)
    dt = torch.bfloat16
    eye = dev(np.eye(n), dt)
    x_t = dev(x, dt)
    xr = rounded(x, dt)
    out = torch.empty((256, n), dtype=dt, device="cuda")
    ops.gemm(x_t, eye, out, act="gelu", flags=ops.GEMM_ACT_FWD)
    ref = ob.gelu(xr)
    assert np.abs(host(out) - ref).max() <= 2.0 ** -8 * np.maximum(np.abs(ref), 2.0 ** -4).max()
    assert np.all(np.abs(host(out) - ref) <= 2.0 ** -8 * np.maximum(np.abs(ref), 2.0 ** -5))
    ones = dev(np.ones((256, n)), dt)
    ops.gemm(ones, eye, out, aux=x_t, act="gelu", flags=ops.GEMM_ACT_BWD)
    refg = ob.gelu_grad(xr)
    assert np.all(np.abs(host(out) - refg) <= 2.0 ** -8 * np.maximum(np.abs(refg), 2.0 ** -5))


@pytest.mark.parametrize("T,split_k", [(4096, 1), (4096, 2), (1000, 3), (16384, 0)])
def test_dense_bwd_params_grouped(ops, T, split_k):
    """All four weight gradients of an encoder layer in one launch: against dY^T X per matrix,
    bitwise against the one-matrix entry point (same split), accumulate, and a null db."""
    r = rng(T + split_k)
    dt = torch.bfloat16
    shapes = [(768, 3072), (3072, 768), (768, 768), (2304, 768)]
    want_db = [False, True, False, True]
    probs, refs = [], []
    for (n_out, n_in), wb in zip(shapes, want_db):
        dY, X = r.standard_normal((T, n_out)) * 0.1, r.standard_normal((T, n_in))
        dw = torch.full((n_out, n_in), float("nan"), device="cuda")
        db = torch.full((n_out,), float("nan"), device="cuda") if wb else None
        probs.append((dev(dY, dt), dev(X, dt), dw, db))
        refs.append((rounded(dY, dt).T @ rounded(X, dt), rounded(dY, dt).sum(0)))
    ops.dense_bwd_params_grouped(probs, False, split_k)
    for (dy, x, dw, db), (rw, rb) in zip(probs, refs):
        assert_close(host(dw), rw, 2e-3, "grouped dW")
        if db is not None:
            assert_close(host(db), rb, 2e-3, "grouped db")
            if split_k > 0:      # 0 = per-problem splits chosen by the library
                dw1, db1 = torch.empty_like(dw), torch.empty_like(db)
                ops.dense_bwd_params(dy, x, dw1, db1, split_k=split_k)
                assert torch.equal(dw, dw1) and torch.equal(db, db1), "grouped launch differs from the single-matrix one"
    # the ping-pong 256 x 256 kernel (default where T is whole K-tiles) and the ring kernel agree bit for bit
    # (same k order inside a slice, same slice-ordered reduction), fused or per-matrix reduce launches alike
    for env, val in (("POLUS_GEMM_PP", -1), ("POLUS_DW_FUSED_REDUCE", 0)):
        ops.set_env(env, val)
        try:
            alt = [(torch.full_like(p[2], float("nan")), None if p[3] is None else torch.full_like(p[3], float("nan"))) for p in probs]
            ops.dense_bwd_params_grouped([(p[0], p[1], a[0], a[1]) for p, a in zip(probs, alt)], False, split_k)
        finally:
            ops.set_env(env)
        if env == "POLUS_DW_FUSED_REDUCE" or split_k > 0:      # with library-chosen splits the two kernels cut K differently
            for (dy, x, dw, db), (aw, ab) in zip(probs, alt):
                assert torch.equal(dw, aw) and (db is None or torch.equal(db, ab)), env
        else:
            for (dy, x, dw, db), (aw, ab) in zip(probs, alt):
                assert_close(host(aw), host(dw), 1e-5, "ring vs ping-pong dW")
    first = [(p[2].clone(), None if p[3] is None else p[3].clone()) for p in probs]
    ops.dense_bwd_params_grouped(probs, True, split_k)
    for (dy, x, dw, db), (w0, b0) in zip(probs, first):
        assert_close(host(dw), 2 * host(w0), 1e-6, "grouped dW accumulate")
        if db is not None:
            assert_close(host(db), 2 * host(b0), 1e-6, "grouped db accumulate")
