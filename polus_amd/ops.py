"""Host-side launchers: torch tensors in, raw pointers through the C ABI, nothing computed here.

torch is the allocator and the stream owner only.  Every function launches on torch's
current stream and returns without synchronising.
"""
import collections
import ctypes

import torch

from . import _lib
from ._lib import (F32, BF16, K_CONTIG, K_STRIDED, ACT_NONE, ACT_GELU, ACT_SWISH, ACT_RELU, ACT_TANH,
                   GEMM_ACCUM_C, GEMM_ACT_FWD, GEMM_ACT_BWD, check, ptr, dtype_code)
# the product-quantisation wrappers (csrc/pq.hip) live in a module of their own and are part of this namespace
from .pq_ops import (IvfPqRoute, PqRoute, ivfpq_coarse_update, ivfpq_residual, ivfpq_scores_ids, ivfpq_scores_ids_route,
                     pq_decode, pq_encode, pq_lut, pq_scores, pq_scores_route, pq_update)
# so do the refine wrappers (csrc/refine.hip)
from .refine_ops import cls_fp8_dequantize, cls_fp8_quantize, cls_rerank, cls_rerank_fp8

# bench.py instrumentation: when a list, every gemm launch appends (kind, flops, ev0, ev1)
GEMM_PROFILE = None

ACT_CODES = {None: ACT_NONE, "linear": ACT_NONE, "gelu": ACT_GELU, "swish": ACT_SWISH,
             "relu": ACT_RELU, "tanh": ACT_TANH}


class Workspace:
    """Grow-only device scratch. Kernels on one stream run in order, so one buffer per
    stream is enough; it is sized during the first step and never reallocated after."""

    def __init__(self, device):
        self.device = device
        self.buf = None

    def get(self, nbytes):
        nbytes = int(nbytes)
        if self.buf is None or self.buf.numel() < nbytes:
            # drop the old buffer only after queued kernels are done with it
            if self.buf is not None:
                torch.cuda.current_stream().synchronize()
            self.buf = torch.empty(max(nbytes, 1 << 20), dtype=torch.uint8, device=self.device)
        return self.buf


_WS = {}
WORKSPACE_OVERRIDE = None      # polus_amd/graph.py: the scratch a captured step uses (same buffer in every replay)


_HAS_GPU = None


def workspace(device):
    global _HAS_GPU
    if WORKSPACE_OVERRIDE is not None:
        return WORKSPACE_OVERRIDE
    if _HAS_GPU is None:
        _HAS_GPU = torch.cuda.is_available()      # ~20 us per call otherwise, once per launch
    key = (device, _lib.current_stream() if _HAS_GPU else 0)
    ws = _WS.get(key)
    if ws is None:
        ws = _WS[key] = Workspace(device)
    return ws


def _st():
    return _lib.current_stream()


def set_dynamic_params(block):
    """Register (None: unregister) the 16-byte device block {uint32 salt, f32 lr, f32 lr_t, 0} that dropout
    kernels and the fused optimizer read per-step scalars from (include/polus_hip.h)."""
    if block is not None:
        _req_cuda(block)
        assert block.numel() * block.element_size() >= 16 and block.is_contiguous(), \
            f"set_dynamic_params: block must be contiguous and hold at least 16 bytes {_got(block)}"
    check(_lib.load().polus_set_dynamic_params(ptr(block)), "polus_set_dynamic_params")


def set_env(name, value=None):
    """Set (or, with None, unset) one of the library's POLUS_* tuning switches and make the library
    re-read them: they are cached at load time (include/polus_hip.h polus_reload_env)."""
    import os
    if value is None:
        os.environ.pop(name, None)
    else:
        os.environ[name] = str(value)
    check(_lib.load().polus_reload_env(), "polus_reload_env")
    _AUTO_SPLIT.clear()


def reserve_cus(active):
    """Switch the CU reserve of the GEMM launches (POLUS_GEMM_RESERVE_CUS) on or off: on while RCCL's channel kernels
    share the chip (backward of a data-parallel step), off otherwise (include/polus_hip.h polus_set_reserve_active)."""
    check(_lib.load().polus_set_reserve_active(1 if active else 0), "polus_set_reserve_active")


def _req_cuda(*ts):
    for t in ts:
        if t is not None and not t.is_cuda:
            raise _lib.PolusHipError("polus_amd ops need device (HBM) tensors; there is no CPU path")


_F32T, _BF16T, _I32T, _I64T = torch.float32, torch.bfloat16, torch.int32, torch.int64


def _got(t):
    return f"(got {t.dtype} {list(t.shape)}, strides {list(t.stride())})"


def _dt(op, name, t):
    """dtype_code for a tensor whose dtype the entry point takes as an argument; the refusal names the parameter."""
    d = t.dtype
    if d == _F32T:
        return F32
    assert d == _BF16T, f"{op}: {name} must be f32 or bf16 {_got(t)}"
    return BF16


def _vec(op, name, t, dtype, n, optional=False):
    """A flat pointer and a count: a contiguous tensor of `dtype` with at least n elements."""
    if t is None:
        assert optional, f"{op}: {name} is required"
        return
    assert t.dtype == dtype and t.numel() >= n and t.is_contiguous(), \
        f"{op}: {name} must be contiguous {dtype} with at least {n} elements {_got(t)}"


def _mat(op, name, t, dtype, rows, cols, exact=False):
    """A pointer and a row stride: a 2-D tensor of `dtype` with at least (exact: exactly) rows x cols elements whose inner
    stride is one."""
    if exact:
        assert t.dtype == dtype and tuple(t.shape) == (rows, cols) and (t.stride(1) == 1 or cols == 1), \
            f"{op}: {name} must be {dtype} [{rows}, {cols}] with a unit inner stride {_got(t)}"
        return
    assert t.dtype == dtype and t.dim() == 2 and t.shape[0] >= rows and t.shape[1] >= cols and (t.stride(1) == 1 or t.shape[1] == 1), \
        f"{op}: {name} must be {dtype} [>= {rows}, >= {cols}] with a unit inner stride {_got(t)}"


def _ld(t, cols):
    """The row stride of a checked matrix, legal for a single row too (whose stride torch leaves arbitrary)."""
    return t.stride(0) if t.shape[0] > 1 else max(t.stride(0), cols)


def _eng(op, name, t, dims):
    """The dtype code of an f32 or bf16 tensor passed as a flat pointer: `dims`-D and contiguous."""
    code = _dt(op, name, t)
    assert t.dim() == dims and t.is_contiguous(), f"{op}: {name} must be a contiguous {dims}-D tensor {_got(t)}"
    return code


def _flat(op, name, t, dtype, shape):
    """A flat pointer whose extent the call fixes: contiguous, of `dtype`, exactly `shape` (an int: that many elements)."""
    ok = t.numel() == shape if isinstance(shape, int) else tuple(t.shape) == tuple(shape)
    want = f"{shape} elements" if isinstance(shape, int) else f"{list(shape)}"
    assert t.dtype == dtype and ok and t.is_contiguous(), f"{op}: {name} must be contiguous {dtype} with {want} {_got(t)}"


def _disjoint(op, a_name, a, b_name, b):
    """Two contiguous tensors the kernel treats as distinct buffers: their byte ranges must not meet."""
    a0, b0 = a.data_ptr(), b.data_ptr()
    a1, b1 = a0 + a.numel() * a.element_size(), b0 + b.numel() * b.element_size()
    assert a1 <= b0 or b1 <= a0, f"{op}: {a_name} must not overlap {b_name}"


_AUTO_SPLIT = {}


def _gemm_call(a, b, out, a_layout, b_layout, M, N, K, alpha, bias, resid, aux, act, flags, split_k):
    """What `gemm` and `gemm_route` share: (M, N, K, split_k with "auto" settled, the arguments of polus_gemm and
    polus_gemm_route up to split_k)."""
    dt = a.dtype
    assert a.dim() == 2 and a.stride(1) == 1, f"gemm: a must be 2-D with a unit inner stride {_got(a)}"
    assert b.dtype == dt and b.dim() == 2 and b.stride(1) == 1, f"gemm: b must be 2-D {dt} with a unit inner stride {_got(b)}"
    if a_layout == K_CONTIG:
        m_, k_ = a.shape
    else:
        k_, m_ = a.shape
    if b_layout == K_CONTIG:
        n_, kb_ = b.shape
    else:
        kb_, n_ = b.shape
    M = m_ if M is None else M
    N = n_ if N is None else N
    K = k_ if K is None else K
    assert kb_ == k_, f"gemm: b: contraction mismatch with a, {k_} vs {kb_}"
    assert m_ >= M and k_ >= K, f"gemm: a holds fewer than M={M} x K={K} elements {_got(a)}"
    assert n_ >= N, f"gemm: b holds fewer than N={N} rows of the product {_got(b)}"
    assert ((out.dtype == dt or out.dtype == _F32T) and out.dim() == 2 and out.shape[0] >= M and out.shape[1] >= N
            and out.stride(1) == 1), f"gemm: out must be f32 or {dt} [>= {M}, >= {N}] with a unit inner stride {_got(out)}"
    if bias is not None:
        _vec("gemm", "bias", bias, _F32T, N)
    if resid is not None:
        _mat("gemm", "resid", resid, dt, M, N)
    if aux is not None:
        _mat("gemm", "aux", aux, dt, M, N)
    if split_k == "auto":
        # the library's recommendation for a bf16 Dense GEMM (K-contiguous operands, bf16 C); 1 for everything else
        split_k = 1
        if (a.dtype == torch.bfloat16 and out.dtype == a.dtype and a_layout == K_CONTIG and b_layout == K_CONTIG
                and not (flags & GEMM_ACCUM_C)):
            key = (M, N, K)
            split_k = _AUTO_SPLIT.get(key)
            if split_k is None:
                split_k = _AUTO_SPLIT[key] = int(_lib.load().polus_gemm_auto_split(M, N, K))
    return M, N, K, split_k, (dtype_code(a.dtype), a_layout, b_layout, dtype_code(out.dtype),
                              ptr(a), a.stride(0), ptr(b), b.stride(0), ptr(out), out.stride(0),
                              M, N, K, float(alpha), ptr(bias),
                              ptr(resid), resid.stride(0) if resid is not None else 0,
                              ptr(aux), aux.stride(0) if aux is not None else 0,
                              ACT_CODES[act] if not isinstance(act, int) else act, flags, split_k)


def gemm(a, b, out, *, a_layout=K_CONTIG, b_layout=K_CONTIG, M=None, N=None, K=None, alpha=1.0,
         bias=None, resid=None, aux=None, act=None, flags=0, split_k=1, drop_p=0.0, seed=0):
    """out[M,N] = epilogue(alpha * A_op . B_op); see include/polus_hip.h polus_gemm."""
    lib = _lib.load()
    _req_cuda(a, b, out, bias, resid, aux)
    M, N, K, split_k, args = _gemm_call(a, b, out, a_layout, b_layout, M, N, K, alpha, bias, resid, aux, act, flags, split_k)
    ws = None
    ws_bytes = 0
    if split_k > 1:
        ws_bytes = lib.polus_gemm_workspace_bytes(M, N, split_k)
        ws = workspace(a.device).get(ws_bytes)
    prof = GEMM_PROFILE
    if prof is not None:
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
    common = args + (ptr(ws), ws_bytes)
    if drop_p > 0.0:
        check(lib.polus_gemm_dropout(*common, float(drop_p), int(seed) & 0xFFFFFFFF, _st()), "polus_gemm_dropout")
    else:
        check(lib.polus_gemm(*common, _st()), "polus_gemm")
    if prof is not None:
        e1.record()
        kind = "fwd" if (a_layout == K_CONTIG and b_layout == K_CONTIG) else ("dx" if a_layout == K_CONTIG else "dw")
        prof.append((kind, 2.0 * M * N * K, e0, e1))
    return out


# The host-only route reports (include/polus_hip.h): what the call with the same tensors and keywords would run.
GEMM_KERNELS = ("v1", "ring", "ring128", "ring_drop", "pp", "pp_persist")
GEMM_REDUCES = ("none", "plain", "epi")
DW_GROUPED_KERNELS = ("one_by_one", "ring_grouped", "pp_grouped", "pp_streamk")
GemmRoute = collections.namedtuple("GemmRoute", "kernel tn mode drop splits reduce persist_cus a_vec b_vec epi_vec epi_vec16 v1_vec")
DwRoute = collections.namedtuple("DwRoute", "ring splits")
DwGroupedRoute = collections.namedtuple("DwGroupedRoute", "kernel fused_reduce eff")


def gemm_route(a, b, out, *, a_layout=K_CONTIG, b_layout=K_CONTIG, M=None, N=None, K=None, alpha=1.0,
               bias=None, resid=None, aux=None, act=None, flags=0, split_k=1, drop_p=0.0, seed=0):
    """The route `gemm` takes with these arguments under the current switches (polus_gemm_route); launches nothing."""
    args = _gemm_call(a, b, out, a_layout, b_layout, M, N, K, alpha, bias, resid, aux, act, flags, split_k)[4]
    r = (ctypes.c_int * 12)()
    check(_lib.load().polus_gemm_route(*args, float(drop_p), r), "polus_gemm_route")
    v = list(r)
    return GemmRoute(GEMM_KERNELS[v[0]], v[1], v[2], v[3], v[4], GEMM_REDUCES[v[5]], v[6], *map(bool, v[7:]))


def dense_bwd_params_route(dy, x, dw, db, accumulate=False, split_k=1):
    """The form `dense_bwd_params` takes with these arguments (polus_dense_bwd_params_route); launches nothing."""
    r = (ctypes.c_int * 2)()
    check(_lib.load().polus_dense_bwd_params_route(dtype_code(dy.dtype), ptr(dy), dy.stride(0), ptr(x), x.stride(0), ptr(dw), dw.stride(0),
                                                   ptr(db), dy.shape[0], dy.shape[1], x.shape[1], split_k, r),
          "polus_dense_bwd_params_route")
    return DwRoute(bool(r[0]), r[1])


def _dw_problems(problems):
    arr = (_lib.DwProblem * len(problems))()
    for k, (dy, x, dw, db) in enumerate(problems):
        arr[k] = _lib.DwProblem(ptr(dy), dy.stride(0), ptr(x), x.stride(0), ptr(dw), dw.stride(0), ptr(db), dy.shape[1], x.shape[1])
    return arr


def dense_bwd_params_grouped_route(problems, accumulate=False, split_k=1):
    """The kernel `dense_bwd_params_grouped` runs for these problems (polus_dense_bwd_params_grouped_route); launches nothing."""
    n = len(problems)
    r = (ctypes.c_int * (2 + n))()
    check(_lib.load().polus_dense_bwd_params_grouped_route(dtype_code(problems[0][0].dtype), n, _dw_problems(problems),
                                                           problems[0][0].shape[0], int(split_k), r),
          "polus_dense_bwd_params_grouped_route")
    return DwGroupedRoute(DW_GROUPED_KERNELS[r[0]], bool(r[1]), tuple(r[2:2 + n]))


LN_ROUTES = (None, "wave_f32", "wave_bf16", "halfwave")
SCATTER_ROUTES = (None, "atomic1", "atomic2", "atomic3", "atomic4", "atomic_wide", "owner")
RowwiseRoute = collections.namedtuple("RowwiseRoute", "ln ln_fwd_blocks ln_bwd_blocks ln_finalize_stages scatter embed_fwd_blocks embed_bwd_blocks")


def rowwise_route(dtype, rows, H, deterministic=False):
    """What layernorm_fwd / layernorm_bwd / embed_ln_fwd / embed_ln_bwd run for `rows` rows of H features of a torch
    dtype under the current switches (polus_rowwise_route); launches nothing."""
    r = (ctypes.c_int * 7)()
    check(_lib.load().polus_rowwise_route(dtype_code(dtype), rows, H, 1 if deterministic else 0, r), "polus_rowwise_route")
    return RowwiseRoute(LN_ROUTES[r[0]], r[1], r[2], r[3], SCATTER_ROUTES[r[4]], r[5], r[6])


def _dense(op, name, t, dtype, shape):
    """A flat pointer whose extents the other arguments fix: a contiguous tensor of exactly this dtype and shape."""
    assert t.dtype == dtype and t.shape == shape and t.is_contiguous(), \
        f"{op}: {name} must be contiguous {dtype} {list(shape)} {_got(t)}"


def attention_fwd(qkv, mask, ctx, lse, B, S, n_heads, drop_p=0.0, seed=0):
    """ctx [B*S, H] = softmax attention over the fused projections qkv [B*S, 3H] (H = 64 n_heads), both contiguous and of
    one dtype, f32 or bf16; mask int32 with B*S elements or None; lse f32 with at least B*n_heads*S elements, contiguous."""
    lib = _lib.load()
    _req_cuda(qkv, mask, ctx, lse)
    H = n_heads * 64
    dt = qkv.dtype
    _dense("attention_fwd", "qkv", qkv, dt, (B * S, 3 * H))
    _dense("attention_fwd", "ctx", ctx, dt, (B * S, H))
    _vec("attention_fwd", "lse", lse, _F32T, B * n_heads * S)
    if mask is not None:
        assert mask.dtype == _I32T and mask.numel() == B * S and mask.is_contiguous(), \
            f"attention_fwd: mask must be contiguous int32 with {B * S} elements {_got(mask)}"
    check(lib.polus_attention_fwd(_dt("attention_fwd", "qkv", qkv), ptr(qkv), ptr(mask), ptr(ctx), ptr(lse),
                                  B, S, n_heads, 64, float(drop_p), int(seed) & 0xFFFFFFFF, _st()), "polus_attention_fwd")


def attention_bwd(qkv, mask, ctx, dctx, lse, dqkv, B, S, n_heads, drop_p=0.0, seed=0):
    """dqkv [B*S, 3H] from dctx [B*S, H] and the forward's qkv, ctx and lse: the four matrices contiguous and of one dtype,
    mask and lse as in attention_fwd."""
    lib = _lib.load()
    _req_cuda(qkv, mask, ctx, dctx, lse, dqkv)
    H = n_heads * 64
    dt = qkv.dtype
    _dense("attention_bwd", "qkv", qkv, dt, (B * S, 3 * H))
    _dense("attention_bwd", "dqkv", dqkv, dt, (B * S, 3 * H))
    _dense("attention_bwd", "ctx", ctx, dt, (B * S, H))
    _dense("attention_bwd", "dctx", dctx, dt, (B * S, H))
    _vec("attention_bwd", "lse", lse, _F32T, B * n_heads * S)
    if mask is not None:
        assert mask.dtype == _I32T and mask.numel() == B * S and mask.is_contiguous(), \
            f"attention_bwd: mask must be contiguous int32 with {B * S} elements {_got(mask)}"
    nb = lib.polus_attention_bwd_workspace_bytes(B, S, n_heads)
    ws = workspace(qkv.device).get(nb)
    check(lib.polus_attention_bwd(_dt("attention_bwd", "qkv", qkv), ptr(qkv), ptr(mask), ptr(ctx), ptr(dctx), ptr(lse),
                                  ptr(dqkv), B, S, n_heads, 64, float(drop_p), int(seed) & 0xFFFFFFFF, ptr(ws), nb, _st()),
          "polus_attention_bwd")


def layernorm_fwd(x, gamma, beta, y, mean, rstd, eps):
    """y = LayerNorm(x) over the last axis; x and y contiguous [rows, H] of one dtype, f32 or bf16; gamma and beta f32 with
    at least H elements, mean and rstd (saved for backward) f32 with at least rows, all contiguous."""
    lib = _lib.load()
    _req_cuda(x, gamma, beta, y, mean, rstd)
    assert x.dim() == 2 and x.is_contiguous(), f"layernorm_fwd: x must be contiguous [rows, H] {_got(x)}"
    rows, H = x.shape
    _dense("layernorm_fwd", "y", y, x.dtype, x.shape)
    _vec("layernorm_fwd", "gamma", gamma, _F32T, H)
    _vec("layernorm_fwd", "beta", beta, _F32T, H)
    _vec("layernorm_fwd", "mean", mean, _F32T, rows)
    _vec("layernorm_fwd", "rstd", rstd, _F32T, rows)
    check(lib.polus_layernorm_fwd(_dt("layernorm_fwd", "x", x), ptr(x), ptr(gamma), ptr(beta), ptr(y), ptr(mean), ptr(rstd),
                                  rows, H, float(eps), _st()), "polus_layernorm_fwd")


def layernorm_bwd_partial_floats(rows, H):
    """f32 elements of a partial-sum buffer for layernorm_bwd(..., partials=...)."""
    return (_lib.load().polus_layernorm_bwd_workspace_bytes(rows, H) + 3) // 4


def layernorm_bwd(dy, x, gamma, mean, rstd, dx, dgamma, dbeta, dbias=None, accumulate=False, dx_masked=None,
                  drop_p=0.0, seed=0, partials=None):
    """`partials` (f32 tensor of layernorm_bwd_partial_floats elements, owned by the caller): stop after the main kernel and
    leave the per-workgroup sums there; dgamma / dbeta / dbias are then written by layernorm_bwd_finalize, which the caller
    queues on any stream ordered behind this call."""
    lib = _lib.load()
    _req_cuda(dy, x, gamma, mean, rstd, dx, dgamma, dbeta, dbias, dx_masked, partials)
    assert x.dim() == 2 and x.is_contiguous(), f"layernorm_bwd: x must be contiguous [rows, H] {_got(x)}"
    rows, H = x.shape
    dt = x.dtype
    _dense("layernorm_bwd", "dy", dy, dt, x.shape)
    _dense("layernorm_bwd", "dx", dx, dt, x.shape)
    _vec("layernorm_bwd", "gamma", gamma, _F32T, H)
    _vec("layernorm_bwd", "mean", mean, _F32T, rows)
    _vec("layernorm_bwd", "rstd", rstd, _F32T, rows)
    if dbias is not None:
        _vec("layernorm_bwd", "dbias", dbias, _F32T, H)
    if dx_masked is not None:
        _vec("layernorm_bwd", "dx_masked", dx_masked, dt, rows * H)
    nb = lib.polus_layernorm_bwd_workspace_bytes(rows, H)
    if partials is not None:
        _vec("layernorm_bwd", "partials", partials, _F32T, (nb + 3) // 4)
        check(lib.polus_layernorm_bwd(_dt("layernorm_bwd", "x", x), ptr(dy), ptr(x), ptr(gamma), ptr(mean), ptr(rstd), ptr(dx),
                                      None, None, ptr(dbias), int(accumulate), rows, H,
                                      ptr(dx_masked), float(drop_p), int(seed) & 0xFFFFFFFF, ptr(partials), partials.numel() * 4, _st()),
              "polus_layernorm_bwd")
        return
    _vec("layernorm_bwd", "dgamma", dgamma, _F32T, H)
    _vec("layernorm_bwd", "dbeta", dbeta, _F32T, H)
    ws = workspace(x.device).get(nb)
    check(lib.polus_layernorm_bwd(_dt("layernorm_bwd", "x", x), ptr(dy), ptr(x), ptr(gamma), ptr(mean), ptr(rstd), ptr(dx),
                                  ptr(dgamma), ptr(dbeta), ptr(dbias), int(accumulate), rows, H,
                                  ptr(dx_masked), float(drop_p), int(seed) & 0xFFFFFFFF, ptr(ws), nb, _st()), "polus_layernorm_bwd")


def layernorm_bwd_finalize(partials, rows, H, dgamma, dbeta, dbias=None, accumulate=False):
    """Reduce the partial sums that layernorm_bwd(..., partials=...) left for `rows` rows of H features into dgamma, dbeta and
    (if given) dbias, each f32 with at least H elements; partials f32 with at least layernorm_bwd_partial_floats(rows, H)."""
    _req_cuda(partials, dgamma, dbeta, dbias)
    _vec("layernorm_bwd_finalize", "partials", partials, _F32T, layernorm_bwd_partial_floats(rows, H))
    _vec("layernorm_bwd_finalize", "dgamma", dgamma, _F32T, H)
    _vec("layernorm_bwd_finalize", "dbeta", dbeta, _F32T, H)
    if dbias is not None:
        _vec("layernorm_bwd_finalize", "dbias", dbias, _F32T, H)
    check(_lib.load().polus_layernorm_bwd_finalize(ptr(partials), partials.numel() * 4, rows, H, ptr(dgamma), ptr(dbeta), ptr(dbias),
                                                   int(accumulate), _st()), "polus_layernorm_bwd_finalize")


def _embed_args(op, ids, type_ids, word, pos, typ, gamma, mean, rstd):
    """What both embedding calls share; returns (B, S, V, H)."""
    assert ids.dtype == _I32T and ids.dim() == 2 and ids.is_contiguous(), f"{op}: ids must be contiguous int32 [B, S] {_got(ids)}"
    B, S = ids.shape
    if type_ids is not None:
        _vec(op, "type_ids", type_ids, _I32T, B * S)
    assert word.dtype == _F32T and word.dim() == 2 and word.is_contiguous(), f"{op}: word must be contiguous f32 [V, H] {_got(word)}"
    V, H = word.shape
    assert pos.dtype == _F32T and pos.dim() == 2 and pos.shape[0] >= S and pos.shape[1] == H and pos.is_contiguous(), \
        f"{op}: pos must be contiguous f32 [>= {S}, {H}] {_got(pos)}"
    assert typ.dtype == _F32T and typ.dim() == 2 and typ.shape[1] == H and typ.is_contiguous(), \
        f"{op}: typ must be contiguous f32 [T, {H}] {_got(typ)}"
    _vec(op, "gamma", gamma, _F32T, H)
    _vec(op, "mean", mean, _F32T, B * S)
    _vec(op, "rstd", rstd, _F32T, B * S)
    return B, S, V, H


def embed_ln_fwd(ids, type_ids, word, pos, typ, gamma, beta, y, mean, rstd, eps, drop_p=0.0, seed=0):
    """y [B*S, H] (f32 or bf16, contiguous) = LayerNorm(word[ids] + pos[s] + typ[type_ids]); ids int32 [B, S] and type_ids
    (int32, B*S elements, or None) contiguous; the tables word [V, H], pos [>= S, H] and typ [T, H] are contiguous f32 whatever
    y's dtype; gamma and beta f32 with at least H elements, mean and rstd f32 with at least B*S."""
    lib = _lib.load()
    _req_cuda(ids, type_ids, word, pos, typ, gamma, beta, y, mean, rstd)
    B, S, V, H = _embed_args("embed_ln_fwd", ids, type_ids, word, pos, typ, gamma, mean, rstd)
    _vec("embed_ln_fwd", "beta", beta, _F32T, H)
    assert y.numel() >= B * S * H and y.is_contiguous(), \
        f"embed_ln_fwd: y must be contiguous with at least {B * S * H} elements {_got(y)}"
    check(lib.polus_embed_ln_fwd(_dt("embed_ln_fwd", "y", y), ptr(ids), ptr(type_ids), ptr(word), ptr(pos), ptr(typ),
                                 ptr(gamma), ptr(beta), ptr(y), ptr(mean), ptr(rstd),
                                 B, S, H, V, pos.shape[0], typ.shape[0], float(eps), float(drop_p), int(seed) & 0xFFFFFFFF,
                                 _st()), "polus_embed_ln_fwd")


def embed_ln_bwd(dy, ids, type_ids, word, pos, typ, gamma, mean, rstd, gword, gpos, gtyp, ggamma, gbeta,
                 accumulate=False, deterministic=False, drop_p=0.0, seed=0):
    """Gradients of embed_ln_fwd from dy [B*S, H] (f32 or bf16, contiguous): gword, gpos and gtyp are contiguous f32 with at
    least the elements of word, pos and typ, ggamma and gbeta f32 with at least H elements; the inputs are as in embed_ln_fwd."""
    lib = _lib.load()
    _req_cuda(dy, ids, type_ids, word, pos, typ, gamma, mean, rstd, gword, gpos, gtyp, ggamma, gbeta)
    B, S, V, H = _embed_args("embed_ln_bwd", ids, type_ids, word, pos, typ, gamma, mean, rstd)
    assert dy.numel() >= B * S * H and dy.is_contiguous(), \
        f"embed_ln_bwd: dy must be contiguous with at least {B * S * H} elements {_got(dy)}"
    _vec("embed_ln_bwd", "gword", gword, _F32T, V * H)
    _vec("embed_ln_bwd", "gpos", gpos, _F32T, pos.shape[0] * H)
    _vec("embed_ln_bwd", "gtyp", gtyp, _F32T, typ.shape[0] * H)
    _vec("embed_ln_bwd", "ggamma", ggamma, _F32T, H)
    _vec("embed_ln_bwd", "gbeta", gbeta, _F32T, H)
    nb = lib.polus_embed_bwd_workspace_bytes(B, S, H)
    ws = workspace(dy.device).get(nb)
    check(lib.polus_embed_ln_bwd(_dt("embed_ln_bwd", "dy", dy), ptr(dy), ptr(ids), ptr(type_ids), ptr(word), ptr(pos), ptr(typ),
                                 ptr(gamma), ptr(mean), ptr(rstd), ptr(gword), ptr(gpos), ptr(gtyp), ptr(ggamma),
                                 ptr(gbeta), int(accumulate), int(deterministic),
                                 B, S, H, V, pos.shape[0], typ.shape[0], float(drop_p), int(seed) & 0xFFFFFFFF,
                                 ptr(ws), nb, _st()), "polus_embed_ln_bwd")


def colsum(x, out, accumulate=False, rows=None, cols=None):
    """out[c] (+)= sum over r < rows of x[r, c]; x f32 or bf16 [>= rows, >= cols] with any row stride and a unit inner
    stride, out contiguous f32 with at least cols elements."""
    lib = _lib.load()
    _req_cuda(x, out)
    assert x.dim() == 2, f"colsum: x must be 2-D {_got(x)}"
    rows = x.shape[0] if rows is None else rows
    cols = x.shape[1] if cols is None else cols
    _mat("colsum", "x", x, x.dtype, rows, cols)
    _vec("colsum", "out", out, _F32T, cols)
    nb = lib.polus_colsum_workspace_bytes(rows, cols)
    ws = workspace(x.device).get(nb)
    check(lib.polus_colsum(_dt("colsum", "x", x), ptr(x), x.stride(0), rows, cols, ptr(out), int(accumulate),
                           ptr(ws), nb, _st()), "polus_colsum")


def softmax_xent(logits, labels, loss, dlogits, class_weights=None, rows=None, C=None):
    """loss (f32 [1]) = mean sparse softmax cross-entropy of logits f32 [>= rows, >= C] against labels (contiguous int32, at
    least rows), dlogits (f32 or bf16, [>= rows, >= C]) its gradient; both matrices have free row strides and a unit inner
    stride; class_weights None or contiguous f32 with at least C elements."""
    lib = _lib.load()
    _req_cuda(logits, labels, loss, dlogits, class_weights)
    assert logits.dim() == 2, f"softmax_xent: logits must be 2-D {_got(logits)}"
    rows = logits.shape[0] if rows is None else rows
    C = logits.shape[1] if C is None else C
    _mat("softmax_xent", "logits", logits, _F32T, rows, C)
    _vec("softmax_xent", "labels", labels, _I32T, rows)
    _vec("softmax_xent", "loss", loss, _F32T, 1)
    _mat("softmax_xent", "dlogits", dlogits, dlogits.dtype, rows, C)
    if class_weights is not None:
        _vec("softmax_xent", "class_weights", class_weights, _F32T, C)
    nb = lib.polus_loss_workspace_bytes(rows)
    ws = workspace(logits.device).get(nb)
    check(lib.polus_softmax_xent(_dt("softmax_xent", "dlogits", dlogits), ptr(logits), logits.stride(0), ptr(labels),
                                 ptr(class_weights), ptr(loss), ptr(dlogits), dlogits.stride(0), rows, C,
                                 ptr(ws), nb, _st()), "polus_softmax_xent")


def sigmoid_xent(logits, y_true, class_weights, negative_weight, loss, dlogits):
    """loss (f32 [1]) = mean weighted sigmoid cross-entropy of logits f32 [rows, C] against the multi-hot y_true f32
    [rows, C], dlogits (f32 or bf16 [rows, C]) its gradient; the three matrices have free row strides and a unit inner
    stride; class_weights contiguous f32 with at least C elements."""
    lib = _lib.load()
    _req_cuda(logits, y_true, class_weights, loss, dlogits)
    assert logits.dim() == 2, f"sigmoid_xent: logits must be 2-D {_got(logits)}"
    rows, C = logits.shape
    _mat("sigmoid_xent", "logits", logits, _F32T, rows, C)
    _mat("sigmoid_xent", "y_true", y_true, _F32T, rows, C)
    _vec("sigmoid_xent", "class_weights", class_weights, _F32T, C)
    _vec("sigmoid_xent", "loss", loss, _F32T, 1)
    _mat("sigmoid_xent", "dlogits", dlogits, dlogits.dtype, rows, C)
    nb = lib.polus_loss_workspace_bytes(rows)
    ws = workspace(logits.device).get(nb)
    check(lib.polus_sigmoid_xent(_dt("sigmoid_xent", "dlogits", dlogits), ptr(logits), logits.stride(0), ptr(y_true), y_true.stride(0),
                                 ptr(class_weights), float(negative_weight), ptr(loss), ptr(dlogits), dlogits.stride(0),
                                 rows, C, ptr(ws), nb, _st()), "polus_sigmoid_xent")


XentWideRoute = collections.namedtuple("XentWideRoute", "path vec16 lds_bytes")
XENT_WIDE_PATHS = ("staged", "streaming")


def _xent_wide_args(logits, dlogits, rows, V):
    dlogits = logits if dlogits is None else dlogits
    assert logits.dim() == 2 and dlogits.dim() == 2 and dlogits.dtype == logits.dtype
    assert (logits.stride(1) == 1 or logits.shape[1] == 1) and (dlogits.stride(1) == 1 or dlogits.shape[1] == 1), \
        "softmax_xent_wide: the class axis must be contiguous"
    rows = logits.shape[0] if rows is None else rows
    V = logits.shape[1] if V is None else V
    assert dlogits.shape[0] >= rows and dlogits.shape[1] >= V
    # the stride of a single row is never used: report one that is legal
    ldl = logits.stride(0) if logits.shape[0] > 1 else max(logits.stride(0), V)
    lddl = dlogits.stride(0) if dlogits.shape[0] > 1 else max(dlogits.stride(0), V)
    return dlogits, rows, V, ldl, lddl


def softmax_xent_wide_route(logits, dlogits=None, rows=None, V=None):
    """What `softmax_xent_wide` runs for these tensors (polus_softmax_xent_wide_route): path "staged" or "streaming",
    whether it moves 16 bytes per lane, and the dynamic LDS bytes; launches nothing and reads no memory, so host
    tensors do (they count for their address and strides alone)."""
    dlogits, rows, V, ldl, lddl = _xent_wide_args(logits, dlogits, rows, V)
    r = (ctypes.c_int * 3)()
    check(_lib.load().polus_softmax_xent_wide_route(dtype_code(logits.dtype), ptr(logits), ldl, ptr(dlogits), lddl,
                                                    rows, V, r), "polus_softmax_xent_wide_route")
    return XentWideRoute(XENT_WIDE_PATHS[r[0]], bool(r[1]), r[2])


def softmax_xent_wide(logits, labels, loss, dlogits=None, stats=None, rows=None, V=None):
    """loss (f32 [1]) = mean over the counted rows of -log softmax(logits)[label]; dlogits (None: in place, into logits)
    = its gradient.  logits f32 or bf16 [rows, V] with any row stride; labels int32 [rows]: < 0 ignores the row,
    >= V ignores it and counts it in stats[1]; stats int32 [2] = {counted, rejected} (include/polus_hip.h
    polus_softmax_xent_wide)."""
    lib = _lib.load()
    _req_cuda(logits, labels, loss, dlogits, stats)
    dlogits, rows, V, ldl, lddl = _xent_wide_args(logits, dlogits, rows, V)
    assert labels.dtype == torch.int32 and labels.is_contiguous() and labels.numel() >= rows
    assert loss.dtype == torch.float32 and loss.numel() >= 1
    assert stats is None or (stats.dtype == torch.int32 and stats.numel() >= 2 and stats.is_contiguous())
    nb = lib.polus_softmax_xent_wide_workspace_bytes(rows)
    ws = workspace(logits.device).get(nb)
    check(lib.polus_softmax_xent_wide(dtype_code(logits.dtype), ptr(logits), ldl, ptr(labels), ptr(loss), ptr(dlogits), lddl,
                                      ptr(stats), rows, V, ptr(ws), nb, _st()), "polus_softmax_xent_wide")
    return dlogits


def gather_rows(x, idx, y, n=None):
    """y[i] = x[idx[i]] where 0 <= idx[i] < x.shape[0], a zero row otherwise; x [rows, H], y [n, H] f32 or bf16 with free row
    strides, idx int32 [n] (include/polus_hip.h polus_gather_rows).  With idx = inverse_map(...) it is the scatter."""
    _req_cuda(x, idx, y)
    assert x.dim() == 2 and y.dim() == 2 and y.dtype == x.dtype and y.shape[1] == x.shape[1]
    assert (x.stride(1) == 1 or x.shape[1] == 1) and (y.stride(1) == 1 or y.shape[1] == 1)
    n = idx.numel() if n is None else n
    assert idx.dtype == torch.int32 and idx.is_contiguous() and idx.numel() >= n and y.shape[0] >= n
    rows, H = x.shape
    ldx = x.stride(0) if rows > 1 else max(x.stride(0), H)
    ldy = y.stride(0) if y.shape[0] > 1 else max(y.stride(0), H)
    check(_lib.load().polus_gather_rows(dtype_code(x.dtype), ptr(x), ldx, ptr(idx), ptr(y), ldy, n, rows, H, _st()),
          "polus_gather_rows")
    return y


def inverse_map(idx, inv):
    """inv[j] (int32 [rows]) = the last i with idx[i] == j, else -1; entries of idx outside [0, rows) are skipped
    (include/polus_hip.h polus_inverse_map)."""
    _req_cuda(idx, inv)
    assert idx.dtype == torch.int32 and inv.dtype == torch.int32 and idx.is_contiguous() and inv.is_contiguous()
    check(_lib.load().polus_inverse_map(ptr(idx), idx.numel(), ptr(inv), inv.numel(), _st()), "polus_inverse_map")
    return inv


def _crf_arg(name, t, dtype, shape, optional=False):
    """The CRF kernels index their arguments as dense arrays of one element type: anything else is read as garbage."""
    if t is None:
        assert optional, f"crf: {name} is required"
        return
    assert t.dtype == dtype and tuple(t.shape) == tuple(shape) and t.is_contiguous(), \
        f"crf: {name} must be contiguous {dtype} {list(shape)} (got {t.dtype} {list(t.shape)}, strides {list(t.stride())})"


def crf_nll(potentials, tags, lengths, trans, sample_w, loss, dpot, dtrans, accumulate=False):
    lib = _lib.load()
    _req_cuda(potentials, tags, lengths, trans, sample_w, loss, dpot, dtrans)
    B, S, C = potentials.shape
    assert potentials.dtype == torch.float32 and potentials.is_contiguous() and dpot.is_contiguous()
    assert dpot.shape == potentials.shape
    _crf_arg("tags", tags, torch.int32, (B, S))
    _crf_arg("lengths", lengths, torch.int32, (B,), optional=True)
    _crf_arg("trans", trans, torch.float32, (C, C))
    _crf_arg("sample_w", sample_w, torch.float32, (B,), optional=True)
    _crf_arg("dtrans", dtrans, torch.float32, (C, C))
    assert loss.dtype == torch.float32 and loss.numel() >= 1, "crf: loss must be f32"
    nb = lib.polus_crf_workspace_bytes(B, S, C)
    ws = workspace(potentials.device).get(nb)
    check(lib.polus_crf_nll(dtype_code(dpot.dtype), ptr(potentials), ptr(tags), ptr(lengths), ptr(trans), ptr(sample_w),
                            ptr(loss), ptr(dpot), ptr(dtrans), int(accumulate), B, S, C, ptr(ws), nb, _st()),
          "polus_crf_nll")


def crf_viterbi(potentials, lengths, trans, out_tags):
    lib = _lib.load()
    _req_cuda(potentials, lengths, trans, out_tags)
    B, S, C = potentials.shape
    assert potentials.dtype == torch.float32 and potentials.is_contiguous()
    _crf_arg("lengths", lengths, torch.int32, (B,), optional=True)
    _crf_arg("trans", trans, torch.float32, (C, C))
    _crf_arg("out_tags", out_tags, torch.int32, (B, S))
    nb = lib.polus_crf_workspace_bytes(B, S, C)
    ws = workspace(potentials.device).get(nb)
    check(lib.polus_crf_viterbi(ptr(potentials), ptr(lengths), ptr(trans), ptr(out_tags), B, S, C, ptr(ws), nb, _st()),
          "polus_crf_viterbi")


def _maxsim_mask(op, name, m, rows, L):
    if m is None:
        return None
    assert m.dtype == torch.int32 and m.is_contiguous() and m.numel() == rows * L, \
        f"{op}: {name} must be contiguous int32 [{rows}, {L}] {_got(m)}"
    return m


def _maxsim_qd(op, q, d):
    """The query and document token matrices of the MaxSim family: q [B, Lq, E], d [N, Ld, E], contiguous, one dtype."""
    code = _eng(op, "q", q, 3)
    B, Lq, E = q.shape
    assert d.dtype == q.dtype and d.dim() == 3 and d.shape[2] == E and d.is_contiguous(), \
        f"{op}: d must be contiguous [N, Ld, {E}] in q's dtype {q.dtype} {_got(d)}"
    return code, B, Lq, E, d.shape[0], d.shape[1]


def _cand(op, cand, B):
    """A candidate list per query: int32 [B, C] with any row stride; returns C."""
    assert cand.dtype == torch.int32 and cand.dim() == 2 and cand.shape[0] == B and (cand.stride(1) == 1 or cand.shape[1] == 1), \
        f"{op}: cand must be int32 [{B}, C] with a unit inner stride {_got(cand)}"
    return cand.shape[1]


def maxsim_fwd(q, d, qmask, dmask, score, argmax):
    """score[b, c] (f32, any row stride >= N) = sum over valid i of max over valid j of <q[b, i], d[c, j]>, and
    argmax[b, c, i] (int32 [B, N, Lq]) the winning j; q [B, Lq, E], d [N, Ld, E] (include/polus_hip.h)."""
    op = "maxsim_fwd"
    _req_cuda(q, d, qmask, dmask, score, argmax)
    code, B, Lq, E, N, Ld = _maxsim_qd(op, q, d)
    _mat(op, "score", score, _F32T, B, N)
    _flat(op, "argmax", argmax, _I32T, B * N * Lq)
    check(_lib.load().polus_maxsim_fwd(code, ptr(q), ptr(d), ptr(_maxsim_mask(op, "qmask", qmask, B, Lq)),
                                       ptr(_maxsim_mask(op, "dmask", dmask, N, Ld)), ptr(score), _ld(score, N), ptr(argmax),
                                       B, N, Lq, Ld, E, _st()), "polus_maxsim_fwd")


def maxsim_scores(q, d, qmask, dmask, score):
    """maxsim_fwd without the argmax (the same kernel body, bitwise the same scores): for scoring a corpus, where
    nothing runs backward.  No B*N*Lq limit."""
    op = "maxsim_scores"
    _req_cuda(q, d, qmask, dmask, score)
    code, B, Lq, E, N, Ld = _maxsim_qd(op, q, d)
    _mat(op, "score", score, _F32T, B, N)
    check(_lib.load().polus_maxsim_scores(code, ptr(q), ptr(d), ptr(_maxsim_mask(op, "qmask", qmask, B, Lq)),
                                          ptr(_maxsim_mask(op, "dmask", dmask, N, Ld)), ptr(score), _ld(score, N),
                                          B, N, Lq, Ld, E, _st()), "polus_maxsim_scores")


def maxsim_rerank(q, d, qmask, dmask, cand, score):
    """score[b, c] (f32 [B, C], any row stride) = the MaxSim score of query b and document cand[b, c] (int32 [B, C],
    any row stride) of the corpus d [N, Ld, E], bit for bit what maxsim_scores gives that pair; -inf where cand[b, c]
    is outside [0, N) (include/polus_hip.h polus_maxsim_rerank)."""
    op = "maxsim_rerank"
    _req_cuda(q, d, qmask, dmask, cand, score)
    code, B, Lq, E, N, Ld = _maxsim_qd(op, q, d)
    C = _cand(op, cand, B)
    _mat(op, "score", score, _F32T, B, C, exact=True)
    check(_lib.load().polus_maxsim_rerank(code, ptr(q), ptr(d), ptr(_maxsim_mask(op, "qmask", qmask, B, Lq)),
                                          ptr(_maxsim_mask(op, "dmask", dmask, N, Ld)), ptr(cand), cand.stride(0), ptr(score),
                                          score.stride(0), B, C, N, Lq, Ld, E, _st()), "polus_maxsim_rerank")


def _fp8_rows(op, name, t, codes, scale):
    """The three tensors of the row quantiser: t [..., E] f32 or bf16, codes uint8 of t's shape, one f32 scale per row."""
    code = _dt(op, name, t)
    assert t.dim() >= 1 and t.is_contiguous(), f"{op}: {name} must be contiguous [..., E] {_got(t)}"
    E = t.shape[-1]
    rows = t.numel() // E
    _flat(op, "codes", codes, torch.uint8, tuple(t.shape))
    _flat(op, "scale", scale, _F32T, rows)
    return code, rows, E


def fp8_quantize(x, codes, scale):
    """x [..., E] (f32 or bf16) -> codes uint8 [..., E] (OCP e4m3fn) and scale f32 [...], one power of two per row:
    the integer rule of include/polus_hip.h polus_fp8_quantize_rows; x ~ e4m3fn(codes) * scale."""
    _req_cuda(x, codes, scale)
    code, rows, E = _fp8_rows("fp8_quantize", "x", x, codes, scale)
    check(_lib.load().polus_fp8_quantize_rows(code, ptr(x), ptr(codes), ptr(scale), rows, E, _st()),
          "polus_fp8_quantize_rows")


def fp8_dequantize(codes, scale, y):
    """y [..., E] (f32 or bf16) = e4m3fn(codes) * scale, exact (codes uint8 [..., E], scale f32 [...])."""
    _req_cuda(codes, scale, y)
    code, rows, E = _fp8_rows("fp8_dequantize", "y", y, codes, scale)
    check(_lib.load().polus_fp8_dequantize_rows(code, ptr(codes), ptr(scale), ptr(y), rows, E, _st()),
          "polus_fp8_dequantize_rows")


def _fp8_corpus(op, q, codes, scale):
    code = _eng(op, "q", q, 3)
    B, Lq, E = q.shape
    assert codes.dtype == torch.uint8 and codes.dim() == 3 and codes.shape[2] == E and codes.is_contiguous(), \
        f"{op}: codes must be contiguous uint8 [N, Ld, {E}] {_got(codes)}"
    N, Ld = codes.shape[0], codes.shape[1]
    _flat(op, "scale", scale, _F32T, (N, Ld))
    return code, B, Lq, E, N, Ld


def maxsim_scores_fp8(q, codes, scale, qmask, dmask, score):
    """maxsim_scores over an FP8 corpus (codes uint8 [N, Ld, E], scale f32 [N, Ld]; q stays f32 or bf16): bit for bit
    maxsim_scores(q, dequantised corpus) (include/polus_hip.h polus_maxsim_scores_fp8)."""
    op = "maxsim_scores_fp8"
    _req_cuda(q, codes, scale, qmask, dmask, score)
    code, B, Lq, E, N, Ld = _fp8_corpus(op, q, codes, scale)
    _mat(op, "score", score, _F32T, B, N)
    check(_lib.load().polus_maxsim_scores_fp8(code, ptr(q), ptr(codes), ptr(scale),
                                              ptr(_maxsim_mask(op, "qmask", qmask, B, Lq)), ptr(_maxsim_mask(op, "dmask", dmask, N, Ld)),
                                              ptr(score), _ld(score, N), B, N, Lq, Ld, E, _st()), "polus_maxsim_scores_fp8")


def maxsim_rerank_fp8(q, codes, scale, qmask, dmask, cand, score):
    """maxsim_rerank over an FP8 corpus: score[b, c] is bit for bit what maxsim_scores_fp8 gives query b and document
    cand[b, c]; -inf where cand[b, c] is outside [0, N) (include/polus_hip.h polus_maxsim_rerank_fp8)."""
    op = "maxsim_rerank_fp8"
    _req_cuda(q, codes, scale, qmask, dmask, cand, score)
    code, B, Lq, E, N, Ld = _fp8_corpus(op, q, codes, scale)
    C = _cand(op, cand, B)
    _mat(op, "score", score, _F32T, B, C, exact=True)
    check(_lib.load().polus_maxsim_rerank_fp8(code, ptr(q), ptr(codes), ptr(scale),
                                              ptr(_maxsim_mask(op, "qmask", qmask, B, Lq)), ptr(_maxsim_mask(op, "dmask", dmask, N, Ld)),
                                              ptr(cand), cand.stride(0), ptr(score), score.stride(0), B, C, N, Lq, Ld, E, _st()),
          "polus_maxsim_rerank_fp8")


def _residual_codec(op, centroids, dtype, table, nbits, E, name):
    """Checks of a residual codec's device tensors; `table` is the cutoffs (2^nbits - 1) or the weights (2^nbits)."""
    assert nbits in (1, 2, 4), f"{op}: nbits must be 1, 2 or 4 (got {nbits})"
    assert centroids.dtype == dtype and centroids.dim() == 2 and centroids.shape[1] == E and centroids.is_contiguous() \
        and 1 <= centroids.shape[0] <= 65535, f"{op}: centroids must be contiguous {dtype} [1 <= K <= 65535, {E}] {_got(centroids)}"
    _flat(op, name, table, _F32T, (1 << nbits) - (1 if name == "cutoffs" else 0))
    return centroids.shape[0]


def _residual_rows(op, name, t, codes, packed, nbits):
    """t [..., E] f32 or bf16 with one int16 code and E * nbits / 8 packed bytes per row."""
    code = _dt(op, name, t)
    assert t.dim() >= 1 and t.is_contiguous(), f"{op}: {name} must be contiguous [..., E] {_got(t)}"
    E = t.shape[-1]
    rows = t.numel() // E
    _flat(op, "codes", codes, torch.int16, rows)
    _flat(op, "packed", packed, torch.uint8, rows * E * nbits // 8)
    return code, rows, E


def residual_compress(x, codes, centroids, cutoffs, nbits, packed):
    """x [..., E] (f32 or bf16) and its centroid codes int16 [...] (the bits of the unsigned code; >= K: no token) ->
    packed uint8 [..., E * nbits / 8], the bucket of every residual element x - centroids[code] among the cutoffs
    f32 [2^nbits - 1] (include/polus_hip.h polus_residual_compress); centroids [K, E] in x's dtype."""
    op = "residual_compress"
    _req_cuda(x, codes, centroids, cutoffs, packed)
    assert nbits in (1, 2, 4), f"{op}: nbits must be 1, 2 or 4 (got {nbits})"
    code, rows, E = _residual_rows(op, "x", x, codes, packed, nbits)
    K = _residual_codec(op, centroids, x.dtype, cutoffs, nbits, E, "cutoffs")
    check(_lib.load().polus_residual_compress(code, ptr(x), ptr(codes), ptr(centroids), K, ptr(cutoffs),
                                              int(nbits), ptr(packed), rows, E, _st()), "polus_residual_compress")


def residual_decompress(codes, packed, centroids, weights, nbits, y):
    """y [..., E] (f32 or bf16) = centroids[code] + weights[bucket], one f32 addition rounded once to y's dtype; rows
    whose code is >= K are zeros (codes int16 [...], packed uint8 [..., E * nbits / 8], weights f32 [2^nbits];
    include/polus_hip.h polus_residual_decompress)."""
    op = "residual_decompress"
    _req_cuda(codes, packed, centroids, weights, y)
    assert nbits in (1, 2, 4), f"{op}: nbits must be 1, 2 or 4 (got {nbits})"
    code, rows, E = _residual_rows(op, "y", y, codes, packed, nbits)
    K = _residual_codec(op, centroids, y.dtype, weights, nbits, E, "weights")
    check(_lib.load().polus_residual_decompress(code, ptr(codes), ptr(packed), ptr(centroids), K, ptr(weights),
                                                int(nbits), ptr(y), rows, E, _st()), "polus_residual_decompress")


def maxsim_rerank_res(q, codes, packed, centroids, weights, nbits, qmask, dmask, cand, score):
    """maxsim_rerank over a residual-compressed corpus (codes int16 [N, Ld], packed uint8 [N, Ld, E * nbits / 8],
    centroids [K, E] in q's dtype, weights f32 [2^nbits]): score[b, c] is bit for bit what maxsim_rerank gives over the
    corpus residual_decompress writes; -inf where cand[b, c] is outside [0, N) (include/polus_hip.h
    polus_maxsim_rerank_res)."""
    op = "maxsim_rerank_res"
    _req_cuda(q, codes, packed, centroids, weights, qmask, dmask, cand, score)
    code = _eng(op, "q", q, 3)
    B, Lq, E = q.shape
    K = _residual_codec(op, centroids, q.dtype, weights, nbits, E, "weights")
    assert codes.dtype == torch.int16 and codes.dim() == 2 and codes.is_contiguous(), \
        f"{op}: codes must be contiguous int16 [N, Ld] {_got(codes)}"
    N, Ld = codes.shape
    _flat(op, "packed", packed, torch.uint8, (N, Ld, E * nbits // 8))
    C = _cand(op, cand, B)
    _mat(op, "score", score, _F32T, B, C, exact=True)
    check(_lib.load().polus_maxsim_rerank_res(code, ptr(q), ptr(codes), ptr(packed), ptr(centroids), K,
                                              ptr(weights), int(nbits), ptr(_maxsim_mask(op, "qmask", qmask, B, Lq)),
                                              ptr(_maxsim_mask(op, "dmask", dmask, N, Ld)), ptr(cand), cand.stride(0), ptr(score),
                                              score.stride(0), B, C, N, Lq, Ld, E, _st()), "polus_maxsim_rerank_res")


def topk_merge(scores, top_val, top_id, id0=0, init=False, ids=None):
    """Merge scores (f32 [rows, n], any row stride; column c is document id0 + c) into the running top-k state
    top_val f32 / top_id int32 [rows, k]: score descending, ties to the lower id, NaN and -inf dropped, (-inf, -1)
    padding.  init=True starts a new state (the old contents are not read).  Exact and bitwise reproducible
    (include/polus_hip.h polus_topk_merge).  With `ids` (int32 [rows, n], any row stride; not together with an id0)
    column c of row r is document ids[r, c] and a negative id drops the column (polus_topk_merge_ids); exact for distinct
    ids, while of a repeated id an undefined number of copies returns."""
    op = "topk_merge"
    _req_cuda(scores, top_val, top_id, ids)
    assert scores.dim() == 2, f"{op}: scores must be f32 [rows, n] {_got(scores)}"
    rows, n = scores.shape
    _mat(op, "scores", scores, _F32T, rows, n, exact=True)
    assert top_val.dim() == 2, f"{op}: top_val must be f32 [{rows}, k] {_got(top_val)}"
    k = top_val.shape[1]
    _flat(op, "top_val", top_val, _F32T, (rows, k))
    _flat(op, "top_id", top_id, _I32T, (rows, k))
    if ids is not None:
        assert int(id0) == 0, f"{op}: ids and a non-zero id0 exclude each other"
        _mat(op, "ids", ids, _I32T, rows, n, exact=True)
        check(_lib.load().polus_topk_merge_ids(ptr(scores), scores.stride(0), ptr(ids), ids.stride(0), rows, n,
                                               ptr(top_val), ptr(top_id), k, 1 if init else 0, _st()),
              "polus_topk_merge_ids")
        return
    check(_lib.load().polus_topk_merge(ptr(scores), scores.stride(0), rows, n, int(id0), ptr(top_val), ptr(top_id), k,
                                       1 if init else 0, _st()), "polus_topk_merge")


CENTROID_ROUTES = (None, "lds", "global")
CentroidRoute = collections.namedtuple("CentroidRoute", "route lds_bytes")


def _centroid_table(op, table, B, Lq):
    """The look-up table of the centroid scorers: f32 [K, >= B * Lq] with any row stride; returns K."""
    assert table.dim() == 2, f"{op}: table must be f32 [K, >= {B * Lq}] {_got(table)}"
    _mat(op, "table", table, _F32T, table.shape[0], B * Lq)
    return table.shape[0]


def _codes2d(op, codes):
    """The centroid codes of a corpus: contiguous int16 [N, Ld] (the bits of the unsigned code); returns (N, Ld)."""
    assert codes.dtype == torch.int16 and codes.dim() == 2 and codes.is_contiguous(), \
        f"{op}: codes must be contiguous int16 [N, Ld] {_got(codes)}"
    return codes.shape


def centroid_scores_route(B, N, Lq, Ld, K):
    """What `centroid_scores` runs for these shapes (polus_centroid_scores_route): the route, "lds" or "global", and the
    dynamic LDS bytes of the LDS route; launches nothing."""
    r = (ctypes.c_int * 2)()
    check(_lib.load().polus_centroid_scores_route(int(B), int(N), int(Lq), int(Ld), int(K), r), "polus_centroid_scores_route")
    return CentroidRoute(CENTROID_ROUTES[r[0]], r[1])


def centroid_scores(table, qmask, codes, score, B, Lq):
    """score[b, n] (f32, any row stride >= N) = sum over valid i of max over present j of table[codes[n, j], b * Lq + i]:
    MaxSim approximated by look-ups.  table f32 [K, >= B * Lq] (any row stride) holds <centroid c, query token (b, i)>;
    codes int16 [N, Ld] (the bits are the unsigned code; 0xFFFF or any code >= K: no token); qmask int32 [B, Lq] or
    None (include/polus_hip.h polus_centroid_scores)."""
    op = "centroid_scores"
    _req_cuda(table, qmask, codes, score)
    K = _centroid_table(op, table, B, Lq)
    N, Ld = _codes2d(op, codes)
    _mat(op, "score", score, _F32T, B, N)
    check(_lib.load().polus_centroid_scores(ptr(table), table.stride(0), ptr(_maxsim_mask(op, "qmask", qmask, B, Lq)), ptr(codes),
                                            ptr(score), score.stride(0), int(B), N, int(Lq), Ld, K, _st()), "polus_centroid_scores")


def centroid_codes(sim, mask, codes, rows=None, K=None):
    """codes[r] (int16, the bits of the unsigned code) = 0xFFFF where mask[r] == 0, else the first column maximising
    sim[r] (f32 [rows, K], any row stride); NaN never wins (include/polus_hip.h polus_centroid_codes)."""
    op = "centroid_codes"
    _req_cuda(sim, mask, codes)
    assert sim.dim() == 2, f"{op}: sim must be f32 [rows, K] {_got(sim)}"
    rows = sim.shape[0] if rows is None else rows
    K = sim.shape[1] if K is None else K
    _mat(op, "sim", sim, _F32T, rows, K)
    _vec(op, "codes", codes, torch.int16, rows)
    _vec(op, "mask", mask, _I32T, rows, optional=True)
    check(_lib.load().polus_centroid_codes(ptr(sim), sim.stride(0), ptr(mask), ptr(codes), rows, K, _st()), "polus_centroid_codes")


def centroid_update(x, codes, prev, out, counts, eps=1e-12):
    """One spherical k-means update: out[k] = the normalised f32 sum of the rows x[t] with codes[t] == k, rounded once to
    x's dtype, or prev[k] where no row has code k or the sum's norm is <= eps; counts[k] (int32) = how many rows.
    x [T, E], codes int16 [T], prev / out [K, E] (distinct buffers) (include/polus_hip.h polus_centroid_update)."""
    op = "centroid_update"
    _req_cuda(x, codes, prev, out, counts)
    code = _eng(op, "x", x, 2)
    T, E = x.shape
    assert prev.dtype == x.dtype and prev.dim() == 2 and prev.shape[1] == E and prev.is_contiguous(), \
        f"{op}: prev must be contiguous [K, {E}] in x's dtype {x.dtype} {_got(prev)}"
    K = prev.shape[0]
    _flat(op, "out", out, x.dtype, (K, E))
    _disjoint(op, "out", out, "prev", prev)
    _flat(op, "codes", codes, torch.int16, T)
    _flat(op, "counts", counts, _I32T, K)
    check(_lib.load().polus_centroid_update(code, ptr(x), ptr(codes), ptr(prev), ptr(out), ptr(counts), T, K, E,
                                            float(eps), _st()), "polus_centroid_update")


def centroid_scores_ids(table, qmask, codes, cand, score, B, Lq):
    """score[b, c] (f32, any row stride) = the bits `centroid_scores` gives the pair (b, cand[b, c]); cand int32 [B, C]
    (any row stride), an id outside [0, N) gives -inf and reads nothing; table, qmask and codes (int16 [N, Ld]) as for
    `centroid_scores` (include/polus_hip.h polus_centroid_scores_ids)."""
    op = "centroid_scores_ids"
    _req_cuda(table, qmask, codes, cand, score)
    K = _centroid_table(op, table, B, Lq)
    N, Ld = _codes2d(op, codes)
    assert cand.dim() == 2, f"{op}: cand must be int32 [>= {B}, C] {_got(cand)}"
    C = cand.shape[1]
    _mat(op, "cand", cand, _I32T, B, C)
    _mat(op, "score", score, _F32T, B, C)
    check(_lib.load().polus_centroid_scores_ids(ptr(table), table.stride(0), ptr(_maxsim_mask(op, "qmask", qmask, B, Lq)), ptr(codes),
                                                ptr(cand), cand.stride(0), ptr(score), score.stride(0), int(B), C, N, int(Lq), Ld,
                                                K, _st()), "polus_centroid_scores_ids")


def _ivf_codes(op, codes, K, k_name):
    N, Ld = _codes2d(op, codes)
    assert 1 <= int(K) <= 65535, f"{op}: {k_name} must give 1 <= K <= 65535 centroids (got {K})"
    return N, Ld


def _bitmap(op, bitmap, B, N):
    """The candidate bitmap: int32 words [>= B, >= ceil(N / 32)] with any row stride."""
    _mat(op, "bitmap", bitmap, _I32T, B, (int(N) + 31) // 32)


def _docs(op, docs):
    """The document ids of the inverted lists: contiguous int32 [P]; P = offsets[K] lives on the device."""
    assert docs.dtype == torch.int32 and docs.dim() == 1 and docs.is_contiguous(), f"{op}: docs must be contiguous int32 [P] {_got(docs)}"


def ivf_count(codes, K, counts):
    """counts[c] (int32 [K], zeroed here) = the documents of codes (int16 [N, Ld], the bits of the unsigned code; >= K: no
    token) that hold at least one token coded c (include/polus_hip.h polus_ivf_count)."""
    op = "ivf_count"
    _req_cuda(codes, counts)
    N, Ld = _ivf_codes(op, codes, K, "K")
    _flat(op, "counts", counts, _I32T, int(K))
    check(_lib.load().polus_ivf_count(ptr(codes), N, Ld, int(K), ptr(counts), _st()), "polus_ivf_count")


def ivf_offsets(counts, offsets):
    """offsets (int32 [K + 1]) = the exclusive scan of counts (int32 [K]); offsets[K] = P, the number of (centroid,
    document) pairs, or -1 when P >= 2^31 (include/polus_hip.h polus_ivf_offsets)."""
    op = "ivf_offsets"
    _req_cuda(counts, offsets)
    K = counts.numel()
    _flat(op, "counts", counts, _I32T, K)
    _flat(op, "offsets", offsets, _I32T, K + 1)
    check(_lib.load().polus_ivf_offsets(ptr(counts), K, ptr(offsets), _st()), "polus_ivf_offsets")


def ivf_fill(codes, offsets, cursor, docs):
    """docs[offsets[c] .. offsets[c + 1]) (int32 [P]) = the ids of the documents counted for centroid c, each once, in
    no specified order; cursor int32 [K] is scratch (include/polus_hip.h polus_ivf_fill)."""
    op = "ivf_fill"
    _req_cuda(codes, offsets, cursor, docs)
    K = cursor.numel()
    _flat(op, "cursor", cursor, _I32T, K)
    N, Ld = _ivf_codes(op, codes, K, "cursor")
    _flat(op, "offsets", offsets, _I32T, K + 1)
    _docs(op, docs)
    check(_lib.load().polus_ivf_fill(ptr(codes), N, Ld, K, ptr(offsets), docs.numel(), ptr(cursor),
                                     ptr(docs) if docs.numel() else None, _st()), "polus_ivf_fill")


def ivf_mark(probes, qmask, offsets, docs, N, bitmap, B, Lq):
    """bitmap (int32 [B, >= ceil(N / 32)] words, any row stride; the first ceil(N / 32) words of a row are cleared here)
    gets bit d of row b for every document d in the list of every probe of query b: probes int32 [B * Lq, nprobe] (any
    row stride; an id outside [0, K) is skipped), qmask int32 [B, Lq] or None, lists (offsets int32 [K + 1], docs int32
    [P]) (include/polus_hip.h polus_ivf_mark)."""
    op = "ivf_mark"
    _req_cuda(probes, qmask, offsets, docs, bitmap)
    K = offsets.numel() - 1
    assert probes.dim() == 2, f"{op}: probes must be int32 [>= {B * Lq}, nprobe] {_got(probes)}"
    nprobe = probes.shape[1]
    _mat(op, "probes", probes, _I32T, B * Lq, nprobe)
    _flat(op, "offsets", offsets, _I32T, K + 1)
    _docs(op, docs)
    _bitmap(op, bitmap, B, N)
    check(_lib.load().polus_ivf_mark(ptr(probes), probes.stride(0), ptr(_maxsim_mask(op, "qmask", qmask, B, Lq)), ptr(offsets),
                                     ptr(docs) if docs.numel() else None, docs.numel(), K, int(N), ptr(bitmap), bitmap.stride(0),
                                     int(B), int(Lq), nprobe, _st()), "polus_ivf_mark")


def ivf_compact(bitmap, N, count, cand=None):
    """count[b] (int32 [B]) = the set bits of row b of bitmap (int32 [B, >= ceil(N / 32)] words) among bits [0, N); with
    cand (int32 [B, cap], any row stride) its row gets the first cap set positions in ascending order, then -1
    (include/polus_hip.h polus_ivf_compact)."""
    op = "ivf_compact"
    _req_cuda(bitmap, count, cand)
    B = count.numel()
    _flat(op, "count", count, _I32T, B)
    _bitmap(op, bitmap, B, N)
    cap = ldc = 0
    if cand is not None:
        assert cand.dim() == 2, f"{op}: cand must be int32 [>= {B}, cap] {_got(cand)}"
        _mat(op, "cand", cand, _I32T, B, cand.shape[1])
        cap, ldc = cand.shape[1], cand.stride(0)
    check(_lib.load().polus_ivf_compact(ptr(bitmap), bitmap.stride(0), B, int(N), ptr(cand), ldc, cap, ptr(count), _st()),
          "polus_ivf_compact")


def _rows2d(t, dtype, rows, cols, name):
    """t is a [>= rows, >= cols] matrix of `dtype` with contiguous columns; returns a row stride that is legal for one row too."""
    assert t.dtype == dtype and t.dim() == 2 and t.shape[0] >= rows and t.shape[1] >= cols, f"{name}: need {dtype} [>= {rows}, >= {cols}], got {t.dtype} {tuple(t.shape)}"
    assert t.stride(1) == 1 or t.shape[1] == 1, f"{name}: the last axis must be contiguous"
    return t.stride(0) if t.shape[0] > 1 else max(t.stride(0), cols)


def splade_pool_fwd(logits, mask, rep, xmax, arg, B, S):
    """rep[b, v] = log1p(max(0, max over the valid tokens s of logits[b S + s, v])), with xmax (the maximum, 0 where
    none is positive) and arg (the lowest winning s, -1 where none) kept for backward.  logits f32 or bf16 [B S, V], any
    row stride; mask int32 [B, S] or None; rep, xmax f32 and arg int32 [B, V] (include/polus_hip.h
    polus_splade_pool_fwd)."""
    _req_cuda(logits, mask, rep, xmax, arg)
    V = logits.shape[1]
    ldl = _rows2d(logits, logits.dtype, B * S, V, "logits")
    ldr, ldx, lda = _rows2d(rep, torch.float32, B, V, "rep"), _rows2d(xmax, torch.float32, B, V, "xmax"), _rows2d(arg, torch.int32, B, V, "arg")
    assert mask is None or (mask.dtype == torch.int32 and mask.is_contiguous() and mask.numel() == B * S)
    check(_lib.load().polus_splade_pool_fwd(dtype_code(logits.dtype), ptr(logits), ldl, ptr(mask), ptr(rep), ldr, ptr(xmax), ldx,
                                            ptr(arg), lda, int(B), int(S), V, _st()), "polus_splade_pool_fwd")
    return rep


def splade_pool_bwd(drep, xmax, arg, dlogits, B, S):
    """dlogits[b S + s, v] = drep[b, v] / (1 + xmax[b, v]) where s == arg[b, v], 0 elsewhere; every row of dlogits (f32 or
    bf16 [B S, V], any row stride; may be the forward's logits buffer) is written (include/polus_hip.h
    polus_splade_pool_bwd)."""
    _req_cuda(drep, xmax, arg, dlogits)
    V = dlogits.shape[1]
    lddl = _rows2d(dlogits, dlogits.dtype, B * S, V, "dlogits")
    lddr, ldx, lda = _rows2d(drep, torch.float32, B, V, "drep"), _rows2d(xmax, torch.float32, B, V, "xmax"), _rows2d(arg, torch.int32, B, V, "arg")
    check(_lib.load().polus_splade_pool_bwd(dtype_code(dlogits.dtype), ptr(drep), lddr, ptr(xmax), ldx, ptr(arg), lda,
                                            ptr(dlogits), lddl, int(B), int(S), V, _st()), "polus_splade_pool_bwd")
    return dlogits


def flops_reg(rep, lam, loss, accumulate=False, drep=None):
    """loss[0] (=, or += with `accumulate`) lam * sum over v of (mean over the rows of rep[:, v])^2, and with drep
    (f32, rep's shape) drep += its gradient.  rep f32 [rows, V], any row stride (include/polus_hip.h polus_flops_reg)."""
    lib = _lib.load()
    _req_cuda(rep, loss, drep)
    rows, V = rep.shape
    ldr = _rows2d(rep, torch.float32, rows, V, "rep")
    lddr = 0 if drep is None else _rows2d(drep, torch.float32, rows, V, "drep")
    assert loss.dtype == torch.float32 and loss.numel() >= 1
    nb = lib.polus_flops_reg_workspace_bytes(V)
    ws = workspace(rep.device).get(nb)
    check(lib.polus_flops_reg(ptr(rep), ldr, rows, V, float(lam), ptr(loss), 1 if accumulate else 0, ptr(drep), lddr,
                              ptr(ws), nb, _st()), "polus_flops_reg")


def sparse_scores(q, ids, w, score):
    """score[b, n] (f32, any row stride >= N) = sum over m with 0 <= ids[n, m] < V of w[n, m] * q[b, ids[n, m]]: N sparse
    documents of M (term, weight) pairs against B dense queries q f32 [B, V]; ids int32 and w f32 [N, M], any row stride
    (include/polus_hip.h polus_sparse_scores)."""
    _req_cuda(q, ids, w, score)
    B, V = q.shape
    N, M = ids.shape
    ldq = _rows2d(q, torch.float32, B, V, "q")
    ldi, ldw = _rows2d(ids, torch.int32, N, M, "ids"), _rows2d(w, torch.float32, N, M, "w")
    lds = _rows2d(score, torch.float32, B, N, "score")
    check(_lib.load().polus_sparse_scores(ptr(q), ldq, ptr(ids), ldi, ptr(w), ldw, ptr(score), lds, B, N, M, V, _st()),
          "polus_sparse_scores")
    return score


def bm25_term_counts(ids, mask, terms, tf, doc_len, V, strip=(0, 0), df=None, stats=None):
    """Per row of ids (int32 [n, L], any row stride; mask int32 [n, L] or None) the distinct token ids that remain after
    the strip (head, tail) and their counts, ordered by (count descending, id ascending), into terms / tf (int32 [n, M],
    any row stride, unused slots (-1, 0)) and the number of remaining tokens into doc_len (int32 [n]).  df (int32 [V])
    and stats (int64 [3]: truncated documents, rejected tokens, tokens) are accumulated into when given
    (include/polus_hip.h polus_bm25_term_counts)."""
    _req_cuda(ids, mask, terms, tf, doc_len, df, stats)
    assert ids.dim() == 2 and terms.dim() == 2, "ids: need int32 [n, L]; terms: need int32 [n, M]"
    (n, L), M = ids.shape, terms.shape[1]
    ldi = _rows2d(ids, torch.int32, n, L, "ids")
    pm, ldm = _pair_mask(mask, n, L, "mask")
    ldt, ldf = _rows2d(terms, torch.int32, n, M, "terms"), _rows2d(tf, torch.int32, n, M, "tf")
    assert tf.shape[1] == M, f"terms has {M} slots, tf {tf.shape[1]}"
    assert doc_len.dtype == torch.int32 and doc_len.is_contiguous() and doc_len.numel() >= n
    assert df is None or (df.dtype == torch.int32 and df.is_contiguous() and df.numel() >= int(V))
    assert stats is None or (stats.dtype == torch.int64 and stats.is_contiguous() and stats.numel() >= 3)
    check(_lib.load().polus_bm25_term_counts(ptr(ids), ldi, pm, ldm, n, L, int(V), int(strip[0]), int(strip[1]), ptr(terms),
                                             ldt, ptr(tf), ldf, M, ptr(doc_len), ptr(df), ptr(stats), _st()),
          "polus_bm25_term_counts")


def bm25_weights(tf, doc_len, w, c0, c1, k1p1):
    """w[r, m] (f32 [n, M], any row stride) = tf (k1 + 1) / (tf + c1 doc_len[r] + c0) where tf[r, m] > 0, else 0; every
    operation rounded once to f32 (include/polus_hip.h polus_bm25_weights)."""
    _req_cuda(tf, doc_len, w)
    n, M = tf.shape
    ldf, ldw = _rows2d(tf, torch.int32, n, M, "tf"), _rows2d(w, torch.float32, n, M, "w")
    assert w.shape[1] == M, f"tf has {M} slots, w {w.shape[1]}"
    assert doc_len.dtype == torch.int32 and doc_len.is_contiguous() and doc_len.numel() >= n
    check(_lib.load().polus_bm25_weights(ptr(tf), ldf, ptr(doc_len), ptr(w), ldw, n, M, float(c0), float(c1), float(k1p1),
                                         _st()), "polus_bm25_weights")
    return w


def bm25_query(terms, tf, idf, q):
    """q (f32 [B, V], any row stride, every element written) = tf[b, m] * idf[terms[b, m]] at column terms[b, m] for
    the used slots of terms / tf (int32 [B, M]), 0 elsewhere; idf f32 [V] (include/polus_hip.h polus_bm25_query)."""
    _req_cuda(terms, tf, idf, q)
    B, M = terms.shape
    V = q.shape[1]
    ldt, ldf = _rows2d(terms, torch.int32, B, M, "terms"), _rows2d(tf, torch.int32, B, M, "tf")
    ldq = _rows2d(q, torch.float32, B, V, "q")
    assert tf.shape[1] == M and q.shape[0] == B
    assert idf.dtype == torch.float32 and idf.is_contiguous() and idf.numel() >= V
    check(_lib.load().polus_bm25_query(ptr(terms), ldt, ptr(tf), ldf, ptr(idf), ptr(q), ldq, B, M, V, _st()), "polus_bm25_query")
    return q


def _postings_blocks(N, block_docs):
    bd = int(block_docs)
    assert 64 <= bd <= 32768 and bd & (bd - 1) == 0, f"block_docs must be a power of two in [64, 32768] (got {block_docs})"
    return (int(N) + bd - 1) // bd


def _postings_forward(ids, w, name):
    assert ids.dim() == 2 and w.dim() == 2 and ids.shape == w.shape, f"{name}: ids and w must both be [N, M]"
    N, M = ids.shape
    return N, M, _rows2d(ids, torch.int32, N, M, "ids"), _rows2d(w, torch.float32, N, M, "w")


def postings_count(ids, w, V, block_docs, counts):
    """counts[b, t] (int32 [nblk, V] contiguous, zeroed here) = the postings of term t among the documents of block b:
    the slots of ids int32 / w f32 [N, M] (any row stride) with 0 <= id < V and w != 0 (include/polus_hip.h
    polus_postings_count)."""
    _req_cuda(ids, w, counts)
    N, M, ldi, ldw = _postings_forward(ids, w, "postings_count")
    nblk = _postings_blocks(N, block_docs)
    assert counts.dtype == torch.int32 and counts.is_contiguous() and tuple(counts.shape) == (nblk, int(V))
    check(_lib.load().polus_postings_count(ptr(ids), ldi, ptr(w), ldw, N, M, int(V), int(block_docs), ptr(counts), _st()),
          "polus_postings_count")


def postings_offsets(counts, offsets, base):
    """offsets (int32 [nblk, V + 1]) = the exclusive scan of every row of counts (int32 [nblk, V]); base (int64
    [nblk + 1]) = the exclusive scan of the block totals, base[nblk] = P (include/polus_hip.h polus_postings_offsets)."""
    _req_cuda(counts, offsets, base)
    nblk, V = counts.shape
    assert counts.dtype == torch.int32 and counts.is_contiguous()
    assert offsets.dtype == torch.int32 and offsets.is_contiguous() and tuple(offsets.shape) == (nblk, V + 1)
    assert base.dtype == torch.int64 and base.is_contiguous() and base.numel() == nblk + 1
    check(_lib.load().polus_postings_offsets(ptr(counts), nblk, V, ptr(offsets), ptr(base), _st()), "polus_postings_offsets")


def postings_fill(ids, w, block_docs, offsets, base, cursor, post_doc, post_w):
    """post_doc (int16 [P], the bits of the unsigned local id) and post_w (f32 [P]) receive the postings of ids / w
    [N, M], the list of (block b, term t) at base[b] + offsets[b, t] .., in no specified order inside a list; cursor
    int32 [nblk, V] is scratch, zeroed here (include/polus_hip.h polus_postings_fill)."""
    _req_cuda(ids, w, offsets, base, cursor, post_doc, post_w)
    N, M, ldi, ldw = _postings_forward(ids, w, "postings_fill")
    nblk = _postings_blocks(N, block_docs)
    V = offsets.shape[1] - 1
    assert offsets.dtype == torch.int32 and offsets.is_contiguous() and tuple(offsets.shape) == (nblk, V + 1)
    assert base.dtype == torch.int64 and base.is_contiguous() and base.numel() == nblk + 1
    assert cursor.dtype == torch.int32 and cursor.is_contiguous() and tuple(cursor.shape) == (nblk, V)
    P = post_doc.numel()
    assert post_doc.dtype == torch.int16 and post_doc.dim() == 1 and post_doc.is_contiguous()
    assert post_w.dtype == torch.float32 and post_w.dim() == 1 and post_w.is_contiguous() and post_w.numel() == P
    check(_lib.load().polus_postings_fill(ptr(ids), ldi, ptr(w), ldw, N, M, V, int(block_docs), ptr(offsets), ptr(base), P,
                                          ptr(cursor), ptr(post_doc) if P else None, ptr(post_w) if P else None, _st()),
          "polus_postings_fill")


def _query_list(q_terms, q_w, q_count, Q, cap):
    ldt, ldw = _rows2d(q_terms, torch.int32, Q, cap, "q_terms"), _rows2d(q_w, torch.float32, Q, cap, "q_w")
    assert q_count.dtype == torch.int32 and q_count.is_contiguous() and q_count.numel() >= Q
    return ldt, ldw


def sparse_compact_rows(q, q_terms, q_w, q_count):
    """The non-zero entries (NaN included, -0.0 not) of every row of q (f32 [Q, V], any row stride) as a query list:
    q_terms int32 / q_w f32 [Q, cap] (any row stride) in ascending term id, then (-1, 0.0); q_count int32 [Q] = the full
    number of non-zeros, also when it exceeds cap (include/polus_hip.h polus_sparse_compact_rows)."""
    _req_cuda(q, q_terms, q_w, q_count)
    Q, V = q.shape
    cap = q_terms.shape[1]
    ldq = _rows2d(q, torch.float32, Q, V, "q")
    assert q_w.shape[1] == cap
    ldt, ldw = _query_list(q_terms, q_w, q_count, Q, cap)
    check(_lib.load().polus_sparse_compact_rows(ptr(q), ldq, Q, V, cap, ptr(q_terms), ldt, ptr(q_w), ldw, ptr(q_count), _st()),
          "polus_sparse_compact_rows")


def bm25_query_lists(terms, tf, idf, q_terms, q_w, q_count):
    """The used slots of terms / tf (int32 [Q, M], as bm25_term_counts leaves a query) as a query list in ascending id:
    q_terms int32 / q_w f32 [Q, M] (any row stride), weight tf * idf[t], then (-1, 0.0); q_count int32 [Q]; idf f32 [V],
    ids outside [0, V) are dropped (include/polus_hip.h polus_bm25_query_lists)."""
    _req_cuda(terms, tf, idf, q_terms, q_w, q_count)
    Q, M = terms.shape
    ldt, ldf = _rows2d(terms, torch.int32, Q, M, "terms"), _rows2d(tf, torch.int32, Q, M, "tf")
    assert tf.shape[1] == M and q_terms.shape[1] == M and q_w.shape[1] == M
    assert idf.dtype == torch.float32 and idf.is_contiguous()
    ldt2, ldw = _query_list(q_terms, q_w, q_count, Q, M)
    check(_lib.load().polus_bm25_query_lists(ptr(terms), ldt, ptr(tf), ldf, ptr(idf), Q, M, idf.numel(), ptr(q_terms), ldt2,
                                             ptr(q_w), ldw, ptr(q_count), _st()), "polus_bm25_query_lists")


def postings_scores(q_terms, q_w, q_count, offsets, base, post_doc, post_w, block_docs, blk0, nblk_launch, N, score):
    """score[q, (b - blk0) * block_docs + local] (f32, any row stride) = the score of query q and document
    b * block_docs + local under the rule of include/polus_hip.h polus_postings_scores, for the blocks blk0 ..
    blk0 + nblk_launch of an N-document corpus; columns of documents >= N are not written.  The query list is q_terms /
    q_w [Q, cap] and q_count [Q]; the postings are (offsets, base, post_doc, post_w)."""
    _req_cuda(q_terms, q_w, q_count, offsets, base, post_doc, post_w, score)
    Q, cap = q_terms.shape
    assert q_w.shape[1] == cap
    ldt, ldw = _query_list(q_terms, q_w, q_count, Q, cap)
    nblk = _postings_blocks(N, block_docs)
    V = offsets.shape[1] - 1
    assert offsets.dtype == torch.int32 and offsets.is_contiguous() and tuple(offsets.shape) == (nblk, V + 1)
    assert base.dtype == torch.int64 and base.is_contiguous() and base.numel() == nblk + 1
    P = post_doc.numel()
    assert post_doc.dtype == torch.int16 and post_doc.dim() == 1 and post_doc.is_contiguous()
    assert post_w.dtype == torch.float32 and post_w.dim() == 1 and post_w.is_contiguous() and post_w.numel() == P
    cols = min(int(nblk_launch) * int(block_docs), int(N) - int(blk0) * int(block_docs))
    lds = _rows2d(score, torch.float32, Q, cols, "score")
    check(_lib.load().polus_postings_scores(ptr(q_terms), ldt, ptr(q_w), ldw, ptr(q_count), cap, ptr(offsets), ptr(base),
                                            ptr(post_doc) if P else None, ptr(post_w) if P else None, P, V, int(block_docs),
                                            int(blk0), int(nblk_launch), int(N), ptr(score), lds, Q, _st()),
          "polus_postings_scores")
    return score


def mine_negatives(cand, neg, n_pool, score=None, exclude=None, skip_top=0, min_score=0.0, seed=0, neg_col=None):
    """k = neg.shape[1] negatives per row of cand (int32 [Q, C] in rank order, any row stride) into neg (int32 [Q, k]),
    their columns into neg_col (int32 [Q, k] or None) and the pool size into n_pool (int32 [Q]).  The pool of a row:
    columns >= skip_top with a non-negative id that is not in exclude (int32 [Q, P] or None) and, with score (f32
    [Q, C]), a score above min_score.  A pool of at most k goes out whole, padded with -1; a larger one gives one seeded
    draw per rank stratum (include/polus_hip.h polus_mine_negatives)."""
    _req_cuda(cand, neg, n_pool, score, exclude, neg_col)
    Q, C, ldc = _pair_cand(cand)
    assert neg.dim() == 2 and neg.dtype == torch.int32 and neg.is_contiguous() and neg.shape[0] == Q, "neg: need contiguous int32 [Q, k]"
    k = neg.shape[1]
    assert neg_col is None or (neg_col.dtype == torch.int32 and neg_col.is_contiguous() and tuple(neg_col.shape) == (Q, k))
    assert n_pool.dtype == torch.int32 and n_pool.is_contiguous() and n_pool.numel() >= Q
    lds = 0 if score is None else _rows2d(score, torch.float32, Q, C, "score")
    assert score is None or score.shape[1] == C
    P, lde = 0, 0
    if exclude is not None and exclude.shape[1] > 0:
        P = exclude.shape[1]
        lde = _rows2d(exclude, torch.int32, Q, P, "exclude")
        assert exclude.shape[0] == Q
    check(_lib.load().polus_mine_negatives(ptr(cand), ldc, ptr(score), lds, ptr(exclude) if P else None, lde, Q, C, P,
                                           int(skip_top), float(min_score), k, int(seed) & 0xFFFFFFFF, ptr(neg), ptr(neg_col),
                                           ptr(n_pool), _st()), "polus_mine_negatives")


FUSE_MODES = {"rrf": 0, "sum": 1, "minmax": 2}


def _lists3d(t, dtype, name):
    """t is an [L, Q, C] stack of `dtype` with contiguous columns; returns strides that are legal for one list or row too."""
    assert t.dtype == dtype and t.dim() == 3, f"{name}: need {dtype} [L, Q, C], got {t.dtype} {tuple(t.shape)}"
    L, Q, C = t.shape
    assert t.stride(2) == 1 or C == 1, f"{name}: the last axis must be contiguous"
    ldr = t.stride(1) if Q > 1 else max(t.stride(1), C)
    return (t.stride(0) if L > 1 else max(t.stride(0), (Q - 1) * ldr + C)), ldr


def fuse_lists(ids, scores, out_id, out_val, count, n_docs, mode, weights=None, rrf_k=60.0):
    """Join L ranked lists per query by document id and fuse their scores.  ids int32 and scores f32 [L, Q, C] (any list
    and row stride; scores may be None under "rrf") are the stacked results of L searches; an entry counts iff its id is
    in [0, n_docs) and its score is finite, and its rank is its position among the entries of its list row that count.
    mode "rrf" (or 0): w / (rrf_k + rank);  "sum" (1): w * score;  "minmax" (2): w * (score - lo) / (hi - lo) over the
    list row's own scores; `weights` is a host sequence of L floats (None: all 1).  out_id int32 / out_val f32 [Q, L*C]
    (any row stride) get each query's distinct ids ascending with their fused scores, then (-1, -inf); count int32 [Q]
    how many.  Every operation is one f32 rounding and a document's contributions are added in (list, column) order
    (include/polus_hip.h polus_fuse_lists)."""
    _req_cuda(ids, scores, out_id, out_val, count)
    lsi, ldi = _lists3d(ids, torch.int32, "ids")
    L, Q, C = ids.shape
    lss = lds = 0
    if scores is not None:
        assert tuple(scores.shape) == (L, Q, C), f"ids is {tuple(ids.shape)}, scores {tuple(scores.shape)}"
        lss, lds = _lists3d(scores, torch.float32, "scores")
    assert tuple(out_id.shape) == (Q, L * C) and tuple(out_val.shape) == (Q, L * C), "out_id, out_val: need [Q, L*C]"
    ldoi, ldov = _rows2d(out_id, torch.int32, Q, L * C, "out_id"), _rows2d(out_val, torch.float32, Q, L * C, "out_val")
    assert count.dtype == torch.int32 and count.is_contiguous() and count.numel() >= Q
    w = None
    if weights is not None:
        assert len(weights) == L, f"{L} lists, {len(weights)} weights"
        w = (ctypes.c_float * L)(*[float(x) for x in weights])
    check(_lib.load().polus_fuse_lists(ptr(ids), lsi, ldi, ptr(scores), lss, lds, L, Q, C, int(n_docs),
                                       FUSE_MODES[mode] if isinstance(mode, str) else int(mode), w, float(rrf_k), ptr(out_id), ldoi, ptr(out_val), ldov,
                                       ptr(count), _st()), "polus_fuse_lists")


def maxsim_bwd(q, d, dscore, argmax, dq, dd):
    """dq [B, Lq, E] and dd [N, Ld, E] from dscore (f32 [B, N], row stride free) and the forward's argmax; every
    element is written."""
    op = "maxsim_bwd"
    _req_cuda(q, d, dscore, argmax, dq, dd)
    code, B, Lq, E, N, Ld = _maxsim_qd(op, q, d)
    _mat(op, "dscore", dscore, _F32T, B, N)
    _flat(op, "argmax", argmax, _I32T, B * N * Lq)
    _flat(op, "dq", dq, q.dtype, tuple(q.shape))
    _flat(op, "dd", dd, d.dtype, tuple(d.shape))
    check(_lib.load().polus_maxsim_bwd(code, ptr(q), ptr(d), ptr(dscore), _ld(dscore, N), ptr(argmax),
                                       ptr(dq), ptr(dd), B, N, Lq, Ld, E, _st()), "polus_maxsim_bwd")


def _norm_rows(op, name, t, rnorm):
    """The rows of a normalisation: t [..., E] f32 or bf16, contiguous, with one f32 rnorm per row."""
    code = _dt(op, name, t)
    assert t.dim() >= 1 and t.is_contiguous(), f"{op}: {name} must be contiguous [..., E] {_got(t)}"
    E = t.shape[-1]
    rows = t.numel() // E
    _flat(op, "rnorm", rnorm, _F32T, rows)
    return code, rows, E


def l2norm_fwd(x, y, rnorm, eps=1e-12):
    """y = x / max(|x|, eps) over the last axis, rnorm (f32, one per row) = 1 / max(|x|, eps)."""
    op = "l2norm_fwd"
    _req_cuda(x, y, rnorm)
    code, rows, E = _norm_rows(op, "x", x, rnorm)
    _flat(op, "y", y, x.dtype, tuple(x.shape))
    check(_lib.load().polus_l2norm_fwd(code, ptr(x), ptr(y), ptr(rnorm), rows, E, float(eps), _st()),
          "polus_l2norm_fwd")


def l2norm_bwd(y, rnorm, dy, dx, eps=1e-12):
    """dx = (dy - y <y, dy>) * rnorm where |x| > eps, dy / eps otherwise (y, rnorm: the forward's outputs; rnorm
    contiguous f32, one per row)."""
    op = "l2norm_bwd"
    _req_cuda(y, rnorm, dy, dx)
    code, rows, E = _norm_rows(op, "y", y, rnorm)
    _flat(op, "dy", dy, y.dtype, tuple(y.shape))
    _flat(op, "dx", dx, y.dtype, tuple(y.shape))
    check(_lib.load().polus_l2norm_bwd(code, ptr(y), ptr(rnorm), ptr(dy), ptr(dx), rows, E, float(eps), _st()),
          "polus_l2norm_bwd")


SLOT_MAJOR, QUERY_MAJOR = 0, 1          # tuple layouts: document (b, j) at row j*B + b / b*n + j


def _tuple_shapes(op, q, d):
    code, B, Lq, E, docs, Ld = _maxsim_qd(op, q, d)
    assert B >= 1 and docs % B == 0, f"{op}: d holds {docs} documents, which is not n per query for {B} queries"
    return code, B, docs // B, Lq, Ld, E


def maxsim_tuples_fwd(q, d, qmask, dmask, score, argmax, layout=SLOT_MAJOR):
    """score[b, j] (f32, any row stride >= n) = MaxSim(q[b], d[doc(b, j)]) of query b and its own n documents, and
    argmax[b, j, i] (int32 [B, n, Lq]) the winning document token: bit for bit what maxsim_fwd gives that pair.
    q [B, Lq, E], d [B n, Ld, E]; document (b, j) is row j*B + b (layout SLOT_MAJOR) or b*n + j (QUERY_MAJOR)
    (include/polus_hip.h polus_maxsim_tuples_fwd)."""
    op = "maxsim_tuples_fwd"
    _req_cuda(q, d, qmask, dmask, score, argmax)
    code, B, n, Lq, Ld, E = _tuple_shapes(op, q, d)
    _mat(op, "score", score, _F32T, B, n)
    _flat(op, "argmax", argmax, _I32T, B * n * Lq)
    check(_lib.load().polus_maxsim_tuples_fwd(code, ptr(q), ptr(d), ptr(_maxsim_mask(op, "qmask", qmask, B, Lq)),
                                              ptr(_maxsim_mask(op, "dmask", dmask, B * n, Ld)), ptr(score), _ld(score, n), ptr(argmax),
                                              B, n, int(layout), Lq, Ld, E, _st()), "polus_maxsim_tuples_fwd")


def maxsim_tuples_bwd(q, d, dscore, argmax, dq, dd, layout=SLOT_MAJOR):
    """dq [B, Lq, E] and dd [B n, Ld, E] from dscore (f32 [B, n], row stride free) and the forward's argmax; every
    element is written, with the bits maxsim_bwd gives for the dscore scattered into a zero [B, B n] matrix."""
    op = "maxsim_tuples_bwd"
    _req_cuda(q, d, dscore, argmax, dq, dd)
    code, B, n, Lq, Ld, E = _tuple_shapes(op, q, d)
    _mat(op, "dscore", dscore, _F32T, B, n)
    _flat(op, "argmax", argmax, _I32T, B * n * Lq)
    _flat(op, "dq", dq, q.dtype, tuple(q.shape))
    _flat(op, "dd", dd, d.dtype, tuple(d.shape))
    check(_lib.load().polus_maxsim_tuples_bwd(code, ptr(q), ptr(d), ptr(dscore), _ld(dscore, n), ptr(argmax),
                                              ptr(dq), ptr(dd), B, n, int(layout), Lq, Ld, E, _st()),
          "polus_maxsim_tuples_bwd")


def _dot_tuple_shapes(op, q, d):
    """q [B, W] and d [B n, W] of one f32 or bf16 dtype with free row strides; returns (dtype code, B, n, W)."""
    code = _dt(op, "q", q)
    assert q.dim() == 2 and q.shape[0] >= 1, f"{op}: q must be [B, W] {_got(q)}"
    B, W = q.shape
    _mat(op, "q", q, q.dtype, B, W, exact=True)
    assert d.dim() == 2, f"{op}: d must be [B n, {W}] in q's dtype {_got(d)}"
    _mat(op, "d", d, q.dtype, d.shape[0], W, exact=True)
    assert d.shape[0] % B == 0, f"{op}: d holds {d.shape[0]} documents, which is not n per query for {B} queries"
    return code, B, d.shape[0] // B, W


def dot_tuples_fwd(q, d, score, layout=SLOT_MAJOR):
    """score[b, j] (f32, any row stride >= n) = <q[b], d[doc(b, j)]>, accumulated in f32 in a fixed order; q [B, W] and
    d [B n, W] f32 or bf16 with free row strides (include/polus_hip.h polus_dot_tuples_fwd)."""
    op = "dot_tuples_fwd"
    _req_cuda(q, d, score)
    code, B, n, W = _dot_tuple_shapes(op, q, d)
    _mat(op, "score", score, _F32T, B, n)
    check(_lib.load().polus_dot_tuples_fwd(code, ptr(q), _ld(q, W), ptr(d), _ld(d, W), ptr(score), _ld(score, n), B, n, int(layout),
                                           W, _st()), "polus_dot_tuples_fwd")
    return score


def dot_tuples_bwd(q, d, dscore, dq, dd, layout=SLOT_MAJOR):
    """dq[b] = sum over j ascending of dscore[b, j] d[doc(b, j)] and dd[doc(b, j)] = dscore[b, j] q[b], f32 arithmetic
    rounded once; dscore f32 [B, n]; every element of dq and dd (free row strides) is written."""
    op = "dot_tuples_bwd"
    _req_cuda(q, d, dscore, dq, dd)
    code, B, n, W = _dot_tuple_shapes(op, q, d)
    _mat(op, "dq", dq, q.dtype, B, W)
    _mat(op, "dd", dd, q.dtype, B * n, W)
    _mat(op, "dscore", dscore, _F32T, B, n)
    check(_lib.load().polus_dot_tuples_bwd(code, ptr(q), _ld(q, W), ptr(d), _ld(d, W), ptr(dscore), _ld(dscore, n), ptr(dq), _ld(dq, W),
                                           ptr(dd), _ld(dd, W), B, n, int(layout), W, _st()), "polus_dot_tuples_bwd")


def _distill(op, student, teacher, loss, dstudent):
    lib = _lib.load()
    _req_cuda(student, teacher, loss, dstudent)
    assert student.dim() == 2, f"{op}: student must be f32 [rows, n] {_got(student)}"
    rows, n = student.shape
    _mat(op, "student", student, _F32T, rows, n, exact=True)
    _mat(op, "teacher", teacher, _F32T, rows, n, exact=True)
    _mat(op, "dstudent", dstudent, _F32T, rows, n, exact=True)
    assert loss.dtype == torch.float32 and loss.numel() >= 1, f"{op}: loss must be f32 with at least one element {_got(loss)}"
    nb = lib.polus_distill_workspace_bytes(rows)
    ws = workspace(student.device).get(nb)
    fn = "polus_" + op
    check(getattr(lib, fn)(ptr(student), _ld(student, n), ptr(teacher), _ld(teacher, n), ptr(loss), ptr(dstudent), _ld(dstudent, n),
                           rows, n, ptr(ws), nb, _st()), fn)


def distill_kl(student, teacher, loss, dstudent):
    """loss (f32 [1]) = mean over the rows of KL(softmax(teacher) || softmax(student)) over the present columns, and
    dstudent its gradient; student, teacher, dstudent f32 [rows, n] with free row strides; a column whose teacher score
    is -inf is absent (include/polus_hip.h polus_distill_kl)."""
    _distill("distill_kl", student, teacher, loss, dstudent)


def margin_mse(student, teacher, loss, dstudent):
    """loss (f32 [1]) = mean over the present negatives j >= 1 of every row of ((s_0 - s_j) - (t_0 - t_j))^2, column 0
    the positive, and dstudent its gradient; same arguments as distill_kl (include/polus_hip.h polus_margin_mse)."""
    _distill("margin_mse", student, teacher, loss, dstudent)


def _pair_rows(rows, B, n, distinct=False):
    """`rows` (None, a host array or an int32 device tensor [R]) -> (device tensor or None, R).  A host array is checked
    (values in [0, B n), distinct where the caller needs that) and copied over; a device tensor is taken as it is."""
    if rows is None:
        return None, B * n
    if not (isinstance(rows, torch.Tensor) and rows.is_cuda):
        import numpy as np
        h = rows.numpy() if isinstance(rows, torch.Tensor) else np.asarray(rows)
        if h.ndim != 1 or h.size < 1 or not np.issubdtype(h.dtype, np.integer):
            raise ValueError(f"rows must be a non-empty 1-d integer array, got {h.dtype} {h.shape}")
        if h.min() < 0 or h.max() >= B * n:
            raise ValueError(f"rows holds a pair index outside [0, B n) = [0, {B * n})")
        if distinct and np.unique(h).size != h.size:
            raise ValueError("rows repeats a pair index: the scattered scores need distinct rows")
        rows = torch.as_tensor(np.ascontiguousarray(h.astype(np.int32))).cuda()
    assert rows.dtype == torch.int32 and rows.dim() == 1 and rows.is_contiguous() and rows.numel() >= 1
    return rows, rows.numel()


def _pair_mask(mask, rows, L, name):
    if mask is None:
        return None, 0
    return ptr(mask), _rows2d(mask, torch.int32, rows, L, name)


def _pair_cand(cand):
    assert cand.dtype == torch.int32 and cand.dim() == 2 and (cand.stride(1) == 1 or cand.shape[1] == 1), "cand: need int32 [B, n]"
    B, n = cand.shape
    return B, n, cand.stride(0) if B > 1 else max(cand.stride(0), n)


def pair_lengths(q_shape, qmask, d_shape, dmask, cand, length, strips, max_q, S, rows=None):
    """length[r] (int32 [R]) = the real tokens of the pair row `cls q' sep d' sep` that pair_pack would build for pair
    rows[r] (None: pair r) of cand (int32 [B, n]): q_shape = (B, Lq) and d_shape = (N, Ld) with their int32 masks (None:
    all ones), strips = (q_head, q_tail, d_head, d_tail) (include/polus_hip.h polus_pair_lengths)."""
    _req_cuda(qmask, dmask, cand, length)
    B, n, ldc = _pair_cand(cand)
    (Bq, Lq), (N, Ld) = q_shape, d_shape
    assert Bq == B, f"cand has {B} rows for {Bq} queries"
    rows, R = _pair_rows(rows, B, n)
    pq, ldqm = _pair_mask(qmask, B, Lq, "qmask")
    pd, lddm = _pair_mask(dmask, N, Ld, "dmask")
    assert length.dtype == torch.int32 and length.is_contiguous() and length.numel() >= R
    qh, qt, dh, dt = (int(s) for s in strips)
    check(_lib.load().polus_pair_lengths(pq, ldqm, pd, lddm, ptr(cand), ldc, ptr(rows), R, B, n, int(N), int(Lq), int(Ld),
                                         qh, qt, dh, dt, int(max_q), int(S), ptr(length), _st()), "polus_pair_lengths")


def pair_pack(q_ids, qmask, d_ids, dmask, cand, input_ids, token_type_ids, attention_mask, strips, max_q, special,
              rows=None, length=None):
    """The pair rows `cls q' sep d' sep pad..` of pairs rows[r] (None: every pair of cand, in order) into input_ids,
    token_type_ids and attention_mask (int32 [R, S], one common row stride; S is their width) and, when given, their
    real lengths into length (int32 [R]).  q_ids int32 [B, Lq], d_ids int32 [N, Ld], the masks int32 or None, cand int32
    [B, n] (an id outside [0, N) is the empty document), strips = (q_head, q_tail, d_head, d_tail), special = (cls, sep,
    pad) (include/polus_hip.h polus_pair_pack)."""
    _req_cuda(q_ids, qmask, d_ids, dmask, cand, input_ids, token_type_ids, attention_mask, length)
    B, n, ldc = _pair_cand(cand)
    assert q_ids.dim() == 2 and d_ids.dim() == 2 and q_ids.shape[0] == B, f"cand has {B} rows for {tuple(q_ids.shape)} query ids"
    (Lq, (N, Ld)) = q_ids.shape[1], d_ids.shape
    rows, R = _pair_rows(rows, B, n)
    ldq, ldd = _rows2d(q_ids, torch.int32, B, Lq, "q_ids"), _rows2d(d_ids, torch.int32, N, Ld, "d_ids")
    pq, ldqm = _pair_mask(qmask, B, Lq, "qmask")
    pd, lddm = _pair_mask(dmask, N, Ld, "dmask")
    S = input_ids.shape[1]
    ldo = _rows2d(input_ids, torch.int32, R, S, "input_ids")
    for t, name in ((token_type_ids, "token_type_ids"), (attention_mask, "attention_mask")):
        assert tuple(t.shape) == tuple(input_ids.shape) and _rows2d(t, torch.int32, R, S, name) == ldo, \
            f"{name}: the three outputs share one shape and row stride"
    assert input_ids.shape[0] == R, f"the outputs have {input_ids.shape[0]} rows for {R} pairs"
    assert length is None or (length.dtype == torch.int32 and length.is_contiguous() and length.numel() >= R)
    qh, qt, dh, dt = (int(s) for s in strips)
    cls, sep, pad = (int(s) for s in special)
    check(_lib.load().polus_pair_pack(ptr(q_ids), ldq, pq, ldqm, ptr(d_ids), ldd, pd, lddm, ptr(cand), ldc, ptr(rows), R, B, n,
                                      N, Lq, Ld, qh, qt, dh, dt, int(max_q), S, cls, sep, pad, ptr(input_ids),
                                      ptr(token_type_ids), ptr(attention_mask), ldo, ptr(length), _st()), "polus_pair_pack")


def pair_scatter_scores(s, cand, N, out, rows=None):
    """out[b, j] = s[r] for pair rows[r] = b n + j (None: pair r) whose candidate cand[b, j] lies in [0, N), -inf for one
    that does not; s f32 [R], out f32 [B, n] (any row stride), entries that `rows` does not name left alone; `rows` must
    be distinct (include/polus_hip.h polus_pair_scatter_scores)."""
    _req_cuda(s, cand, out)
    B, n, ldc = _pair_cand(cand)
    rows, R = _pair_rows(rows, B, n, distinct=True)
    assert s.dtype == torch.float32 and s.is_contiguous() and s.numel() >= R
    ldo = _rows2d(out, torch.float32, B, n, "out")
    check(_lib.load().polus_pair_scatter_scores(ptr(s), ptr(rows), ptr(cand), ldc, R, B, n, int(N), ptr(out), ldo, _st()),
          "polus_pair_scatter_scores")


def argmax(x, out, rows=None, C=None):
    """out[r] (contiguous int32, at least rows) = argmax over c < C of x[r, c]; x f32 [>= rows, >= C] with any row stride and
    a unit inner stride."""
    lib = _lib.load()
    _req_cuda(x, out)
    assert x.dim() == 2, f"argmax: x must be 2-D {_got(x)}"
    rows = x.shape[0] if rows is None else rows
    C = x.shape[1] if C is None else C
    _mat("argmax", "x", x, _F32T, rows, C)
    _vec("argmax", "out", out, _I32T, rows)
    check(lib.polus_argmax(ptr(x), x.stride(0), ptr(out), rows, C, _st()), "polus_argmax")


def confusion_matrix(row_idx, col_idx, cm, rejected=None):
    """cm[row_idx[i], col_idx[i]] += 1 (int32 [C, C] on the device); pairs with an index outside [0, C) are counted in
    `rejected` (int32 [1] on the device) instead."""
    _req_cuda(row_idx, col_idx, cm, rejected)
    n = row_idx.numel()
    assert row_idx.dtype == _I32T and row_idx.is_contiguous(), f"confusion_matrix: row_idx must be contiguous int32 {_got(row_idx)}"
    _vec("confusion_matrix", "col_idx", col_idx, _I32T, n)
    assert col_idx.numel() == n, f"confusion_matrix: col_idx must pair up with the {n} elements of row_idx {_got(col_idx)}"
    assert cm.dtype == _I32T and cm.dim() == 2 and cm.shape[0] == cm.shape[1] and cm.is_contiguous(), \
        f"confusion_matrix: cm must be contiguous int32 [C, C] {_got(cm)}"
    if rejected is not None:
        _vec("confusion_matrix", "rejected", rejected, _I32T, 1)
    check(_lib.load().polus_confusion_matrix(ptr(row_idx), ptr(col_idx), row_idx.numel(), cm.shape[0], ptr(cm),
                                             ptr(rejected) if rejected is not None else None, _st()),
          "polus_confusion_matrix")


def _bio_rows(t, B, S, what):
    assert t.dtype == torch.int32 and tuple(t.shape) == (B, S) and (t.stride(1) == 1 or S == 1), what
    return ptr(t), t.stride(0) if B > 1 else S          # the stride of a single row is never used and may be anything


def bio_entity_counts(tags_a, tags_b, scheme, counts, stats, mask=None):
    """Decode both int32 [B, S] tag tensors (any row stride) by the BIO rule under one optional int32 [B, S] mask and add
    per type (common, n_a, n_b) to counts (int32 [T, 3]) and the decode statistics to stats (int32 [6]); scheme is the
    int32 [C] table of polus_amd.ner.bio.parse_scheme, on the device (include/polus_hip.h polus_bio_entity_counts)."""
    _req_cuda(tags_a, tags_b, scheme, counts, stats, mask)
    assert tags_a.dim() == 2
    B, S = tags_a.shape
    pa, lda = _bio_rows(tags_a, B, S, "tags_a")
    pb, ldb = _bio_rows(tags_b, B, S, "tags_b")
    pm, ldm = _bio_rows(mask, B, S, "mask") if mask is not None else (None, 0)
    assert scheme.dtype == torch.int32 and scheme.dim() == 1 and scheme.is_contiguous()
    assert counts.dtype == torch.int32 and counts.dim() == 2 and counts.shape[1] == 3 and counts.is_contiguous()
    assert stats.dtype == torch.int32 and stats.numel() == 6 and stats.is_contiguous()
    check(_lib.load().polus_bio_entity_counts(pa, lda, pb, ldb, pm, ldm, ptr(scheme), scheme.numel(), counts.shape[0],
                                              B, S, ptr(counts), ptr(stats), _st()), "polus_bio_entity_counts")


def bio_spans(tags, scheme, spans, count, mask=None, rejected=None):
    """A row's entities of the int32 [B, S] tag tensor (any row stride) as (start, end_exclusive, type) in order of
    start into spans (int32 [B, M, 3]); count (int32 [B]) gets the row's true number of entities, of which the first M
    are written and the slots behind them left alone; out-of-range tag ids are added to rejected (int32 [1])
    (include/polus_hip.h polus_bio_spans)."""
    _req_cuda(tags, scheme, spans, count, mask, rejected)
    assert tags.dim() == 2
    B, S = tags.shape
    pt, ldt = _bio_rows(tags, B, S, "tags")
    pm, ldm = _bio_rows(mask, B, S, "mask") if mask is not None else (None, 0)
    assert scheme.dtype == torch.int32 and scheme.dim() == 1 and scheme.is_contiguous()
    assert spans.dtype == torch.int32 and spans.dim() == 3 and spans.shape[0] == B and spans.shape[2] == 3 and spans.is_contiguous()
    assert count.dtype == torch.int32 and count.numel() == B and count.is_contiguous()
    assert rejected is None or (rejected.dtype == torch.int32 and rejected.numel() == 1)
    check(_lib.load().polus_bio_spans(pt, ldt, pm, ldm, ptr(scheme), scheme.numel(), B, S, ptr(spans), spans.shape[1],
                                      ptr(count), ptr(rejected), _st()), "polus_bio_spans")


def adam_step(p, g, m, v, shadow, seg, n_seg, lr, lr_t, beta1, beta2, eps, weight_decay, grad_scale=1.0,
              clip_scale=None):
    """One Adam / AdamW update of the flat arena p from g, with the moments m and v: contiguous f32, g, m and v with at least
    p's elements; shadow None or contiguous bf16 of at least as many; seg contiguous int64 with at least 3 n_seg elements
    (begin, end, flags per window); clip_scale None or f32 [1] on the device."""
    lib = _lib.load()
    _req_cuda(p, g, m, v, shadow, seg, clip_scale)
    n = p.numel()
    _vec("adam_step", "p", p, _F32T, 1)
    _vec("adam_step", "g", g, _F32T, n)
    _vec("adam_step", "m", m, _F32T, n)
    _vec("adam_step", "v", v, _F32T, n)
    if shadow is not None:
        _vec("adam_step", "shadow", shadow, _BF16T, n)
    _vec("adam_step", "seg", seg, _I64T, 3 * n_seg)
    if clip_scale is not None:
        _vec("adam_step", "clip_scale", clip_scale, _F32T, 1)
    check(lib.polus_adam_step(ptr(p), ptr(g), ptr(m), ptr(v), ptr(shadow), ptr(seg), n_seg, p.numel(),
                              float(lr), float(lr_t), float(beta1), float(beta2), float(eps), float(weight_decay),
                              float(grad_scale), ptr(clip_scale), _st()), "polus_adam_step")


def sqnorm(g, out):
    """out[0] (f32) = the sum of squares of g, contiguous f32 of any shape."""
    lib = _lib.load()
    _req_cuda(g, out)
    _vec("sqnorm", "g", g, _F32T, 1)
    _vec("sqnorm", "out", out, _F32T, 1)
    nb = lib.polus_sqnorm_workspace_bytes(g.numel())
    ws = workspace(g.device).get(nb)
    check(lib.polus_sqnorm(ptr(g), g.numel(), ptr(out), ptr(ws), nb, _st()), "polus_sqnorm")


def sqnorm_segments(g, seg, n_seg, out):
    """sum of g^2 over the windows of the Adam segment table `seg` (int64 [n_seg, 3]) -> out[0]; g contiguous f32 that
    covers every window, seg contiguous with at least 3 n_seg elements, out f32."""
    lib = _lib.load()
    _req_cuda(g, seg, out)
    _vec("sqnorm_segments", "g", g, _F32T, 1)
    _vec("sqnorm_segments", "seg", seg, _I64T, 3 * n_seg)
    _vec("sqnorm_segments", "out", out, _F32T, 1)
    ws =workspace(g.device).get(4096)
    check(lib.polus_sqnorm_segments(ptr(g), ptr(seg), int(n_seg), ptr(out), ptr(ws), 4096, _st()), "polus_sqnorm_segments")


def clip_scale(sq, grad_scale, clip_norm, out):
    """out = clip_norm / max(sqrt(sum(sq)) * |grad_scale|, clip_norm); sq holds one partial sum per arena (contiguous f32,
    every element is read), out f32 [1]."""
    _req_cuda(sq, out)
    _vec("clip_scale", "sq", sq, _F32T, 1)
    _vec("clip_scale", "out", out, _F32T, 1)
    check(_lib.load().polus_clip_scale(ptr(sq), sq.numel(), float(grad_scale), float(clip_norm), ptr(out), _st()), "polus_clip_scale")


def cast(src, dst):
    """dst = src converted, element by element: both contiguous, f32 or bf16 each, with the same number of elements."""
    _req_cuda(src, dst)
    n = src.numel()
    assert src.is_contiguous(), f"cast: src must be contiguous {_got(src)}"
    assert dst.numel() == n and dst.is_contiguous(), f"cast: dst must be contiguous with the {n} elements of src {_got(dst)}"
    check(_lib.load().polus_cast(_dt("cast", "src", src), ptr(src), _dt("cast", "dst", dst), ptr(dst), n, _st()),
          "polus_cast")


def scale_(x, a):
    """x *= a in place; x contiguous f32 of any shape."""
    _req_cuda(x)
    assert x.dtype == _F32T and x.is_contiguous(), f"scale_: x must be contiguous f32 {_got(x)}"
    check(_lib.load().polus_scale(ptr(x), float(a), x.numel(), _st()), "polus_scale")


def act_bwd(dy, u, du, act):
    """du = dy * act'(u) element by element: three contiguous tensors of one dtype, f32 or bf16, and one size."""
    _req_cuda(dy, u, du)
    n = dy.numel()
    dt = dy.dtype
    assert dy.is_contiguous(), f"act_bwd: dy must be contiguous {_got(dy)}"
    assert u.dtype == dt and u.numel() == n and u.is_contiguous(), f"act_bwd: u must be contiguous {dt} with {n} elements {_got(u)}"
    assert du.dtype == dt and du.numel() == n and du.is_contiguous(), f"act_bwd: du must be contiguous {dt} with {n} elements {_got(du)}"
    check(_lib.load().polus_act_bwd(_dt("act_bwd", "dy", dy), ptr(dy), ptr(u), ptr(du), n,
                                    ACT_CODES[act] if not isinstance(act, int) else act, _st()), "polus_act_bwd")


def transpose_bf16(src, dst):
    """dst [C, R] = the transpose of src [R, C]; both contiguous bf16, dst with src's number of elements."""
    _req_cuda(src, dst)
    assert src.dtype == _BF16T and src.dim() == 2 and src.is_contiguous(), f"transpose_bf16: src must be contiguous bf16 [R, C] {_got(src)}"
    R, C = src.shape
    assert dst.dtype == _BF16T and dst.numel() == R * C and dst.is_contiguous(), \
        f"transpose_bf16: dst must be contiguous bf16 with {R * C} elements {_got(dst)}"
    check(_lib.load().polus_transpose_bf16(ptr(src), ptr(dst), R, C, _st()), "polus_transpose_bf16")


def dense_bwd_params_grouped(problems, accumulate=False, split_k=1):
    """dW (+ db) of several Dense layers in one launch.  problems: [(dy [T,n_out], x [T,n_in], dw f32 [n_out,n_in],
    db f32 [n_out] or None), ...] with one common T."""
    lib = _lib.load()
    T = problems[0][0].shape[0]
    dt0 = problems[0][0].dtype
    for k, (dy, x, dw, db) in enumerate(problems):
        _req_cuda(dy, x, dw, db)
        assert dy.dtype == dt0 and dy.dim() == 2 and dy.shape[0] == T and dy.stride(1) == 1, \
            f"dense_bwd_params_grouped: problems[{k}]: dy must be {dt0} [{T}, n_out] with a unit inner stride {_got(dy)}"
        assert x.dtype == dt0 and x.dim() == 2 and x.shape[0] == T and x.stride(1) == 1, \
            f"dense_bwd_params_grouped: problems[{k}]: x must be {dt0} [{T}, n_in] with a unit inner stride {_got(x)}"
        n_out, n_in = dy.shape[1], x.shape[1]
        assert dw.dtype == _F32T and dw.shape == (n_out, n_in) and dw.stride(1) == 1, \
            f"dense_bwd_params_grouped: problems[{k}]: dw must be f32 [{n_out}, {n_in}] with a unit inner stride {_got(dw)}"
        if db is not None:
            _vec("dense_bwd_params_grouped", f"problems[{k}]: db", db, _F32T, n_out)
    arr = _dw_problems(problems)
    dt = _dt("dense_bwd_params_grouped", "problems[0]: dy", problems[0][0])
    nb = lib.polus_dense_bwd_params_grouped_workspace_bytes(len(problems), arr, T, int(split_k))
    ws = workspace(problems[0][0].device).get(nb)
    prof = GEMM_PROFILE
    if prof is not None:
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
    check(lib.polus_dense_bwd_params_grouped(dt, len(problems), arr, T, 1 if accumulate else 0, int(split_k),
                                             ptr(ws), ws.numel(), _st()), "polus_dense_bwd_params_grouped")
    if prof is not None:
        e1.record()
        prof.append(("dw", sum(2.0 * T * p[0].shape[1] * p[1].shape[1] for p in problems), e0, e1))


def dense_thin_supported(dtype, H, C):
    """A Dense with at most 8 units takes the HBM-bound wave-per-row kernels instead of MFMA tiles (include/polus_hip.h)."""
    return bool(_lib.load().polus_dense_thin_supported(dtype_code(dtype), int(H), int(C)))


def dense_thin_fwd(x, w, bias, y):
    """y [rows, C] = x [rows, H] . w [C, H]^T + bias; y in f32 or x's dtype."""
    _req_cuda(x, w, bias, y)
    assert x.dim() == 2 and x.stride(1) == 1, f"dense_thin_fwd: x must be [rows, H] with a unit inner stride {_got(x)}"
    rows, H = x.shape
    dt = x.dtype
    assert w.dtype == dt and w.dim() == 2 and w.shape[1] == H and w.stride(1) == 1, \
        f"dense_thin_fwd: w must be {dt} [C, {H}] with a unit inner stride {_got(w)}"
    C = w.shape[0]
    if bias is not None:
        _vec("dense_thin_fwd", "bias", bias, _F32T, C)
    assert (y.dtype == dt or y.dtype == _F32T) and y.shape == (rows, C) and (y.stride(1) == 1 or C == 1), \
        f"dense_thin_fwd: y must be f32 or {dt} [{rows}, {C}] with a unit inner stride {_got(y)}"
    check(_lib.load().polus_dense_thin_fwd(_dt("dense_thin_fwd", "x", x), ptr(x), x.stride(0), ptr(w), w.stride(0), ptr(bias),
                                           dtype_code(y.dtype), ptr(y), y.stride(0), rows, H, C, _st()), "polus_dense_thin_fwd")


def dense_thin_bwd(x, dy, w, dx, dw, db, accumulate=False):
    """dx [rows, H] = dy . w (dx None: skipped), dw [C, H] (+)= dy^T x, db [C] (+)= colsum(dy): one pass over x."""
    lib = _lib.load()
    _req_cuda(x, dy, w, dx, dw, db)
    assert x.dim() == 2 and x.stride(1) == 1, f"dense_thin_bwd: x must be [rows, H] with a unit inner stride {_got(x)}"
    rows, H = x.shape
    dt = x.dtype
    assert w.dtype == dt and w.dim() == 2 and w.shape[1] == H and w.stride(1) == 1, \
        f"dense_thin_bwd: w must be {dt} [C, {H}] with a unit inner stride {_got(w)}"
    C = w.shape[0]
    assert (dy.dtype == dt or dy.dtype == _F32T) and dy.shape == (rows, C) and dy.stride(1) == 1, \
        f"dense_thin_bwd: dy must be f32 or {dt} [{rows}, {C}] with a unit inner stride {_got(dy)}"
    assert dw.dtype == _F32T and dw.shape == (C, H) and dw.stride(1) == 1, \
        f"dense_thin_bwd: dw must be f32 [{C}, {H}] with a unit inner stride {_got(dw)}"
    if dx is not None:
        assert dx.dtype == dt and dx.shape == x.shape and dx.stride(1) == 1, \
            f"dense_thin_bwd: dx must be {dt} {list(x.shape)} with a unit inner stride {_got(dx)}"
    if db is not None:
        _vec("dense_thin_bwd", "db", db, _F32T, C)
    code = _dt("dense_thin_bwd", "x", x)
    nb = lib.polus_dense_thin_bwd_workspace_bytes(code, rows, H, C)
    ws = workspace(x.device).get(nb)
    check(lib.polus_dense_thin_bwd(code, ptr(x), x.stride(0), dtype_code(dy.dtype), ptr(dy), dy.stride(0),
                                   ptr(w), w.stride(0), ptr(dx), dx.stride(0) if dx is not None else 0, ptr(dw), dw.stride(0), ptr(db),
                                   rows, H, C, 1 if accumulate else 0, ptr(ws), ws.numel(), _st()), "polus_dense_thin_bwd")


def transpose_bf16_batched(src_base, dst_base, segs_dev, nseg, total_tiles):
    """All matrices of a flat bf16 arena into its transposed twin in one launch (segs: int64 [nseg, 4]); both arenas
    contiguous bf16 of one size, segs_dev contiguous with at least 4 nseg elements."""
    _req_cuda(src_base, dst_base, segs_dev)
    assert src_base.dtype == _BF16T and src_base.is_contiguous(), f"transpose_bf16_batched: src_base must be contiguous bf16 {_got(src_base)}"
    assert dst_base.dtype == _BF16T and dst_base.numel() >= src_base.numel() and dst_base.is_contiguous(), \
        f"transpose_bf16_batched: dst_base must be contiguous bf16 with the {src_base.numel()} elements of src_base {_got(dst_base)}"
    assert nseg > 0, f"transpose_bf16_batched: segs_dev: nseg must be positive (got {nseg})"
    _vec("transpose_bf16_batched", "segs_dev", segs_dev, _I64T, 4 * nseg)
    check(_lib.load().polus_transpose_bf16_batched(ptr(src_base), ptr(dst_base), ptr(segs_dev), int(nseg), int(total_tiles), _st()),
          "polus_transpose_bf16_batched")


def dense_bwd_params(dy, x, dw, db, accumulate=False, split_k=1):
    """dW (+)= dY^T X and db (+)= colsum(dY) in one pass over dY."""
    lib = _lib.load()
    _req_cuda(dy, x, dw, db)
    assert dy.dim() == 2 and dy.stride(1) == 1, f"dense_bwd_params: dy must be [T, n_out] with a unit inner stride {_got(dy)}"
    T, n_out = dy.shape
    assert x.dtype == dy.dtype and x.dim() == 2 and x.shape[0] == T and x.stride(1) == 1, \
        f"dense_bwd_params: x must be {dy.dtype} [{T}, n_in] with a unit inner stride {_got(x)}"
    n_in = x.shape[1]
    assert dw.dtype == _F32T and dw.shape == (n_out, n_in) and dw.stride(1) == 1, \
        f"dense_bwd_params: dw must be f32 [{n_out}, {n_in}] with a unit inner stride {_got(dw)}"
    if db is not None:
        _vec("dense_bwd_params", "db", db, _F32T, n_out)
    nb = lib.polus_dense_bwd_params_workspace_bytes(T, n_out, n_in, split_k)
    ws = workspace(dy.device).get(nb)
    prof = GEMM_PROFILE
    if prof is not None:
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
    check(lib.polus_dense_bwd_params(_dt("dense_bwd_params", "dy", dy), ptr(dy), dy.stride(0), ptr(x), x.stride(0), ptr(dw), dw.stride(0),
                                     ptr(db), T, n_out, n_in, int(accumulate), split_k, ptr(ws), nb, _st()),
          "polus_dense_bwd_params")
    if prof is not None:
        e1.record()
        prof.append(("dw", 2.0 * T * n_out * n_in, e0, e1))


def dropout(x, y, drop_p, seed):
    """y = inverted dropout of x under the counter-based mask of `seed`; x and y contiguous, of one dtype (f32 or bf16) and
    one size."""
    _req_cuda(x, y)
    assert x.is_contiguous(), f"dropout: x must be contiguous {_got(x)}"
    assert y.dtype == x.dtype and y.numel() == x.numel() and y.is_contiguous(), \
        f"dropout: y must be contiguous {x.dtype} with the {x.numel()} elements of x {_got(y)}"
    check(_lib.load().polus_dropout(_dt("dropout", "x", x), ptr(x), ptr(y), x.numel(), float(drop_p), int(seed) & 0xFFFFFFFF, _st()),
          "polus_dropout")


def dropout_mask(seed, drop_p, n, idx0=0, device=None):
    """uint8 keep-mask of elements idx0..idx0+n-1 for `seed` (reference for every dropout site)."""
    m = torch.empty(int(n), dtype=torch.uint8, device=device or "cuda")
    check(_lib.load().polus_dropout_mask(int(seed) & 0xFFFFFFFF, float(drop_p), int(idx0), int(n), ptr(m), _st()), "polus_dropout_mask")
    return m
