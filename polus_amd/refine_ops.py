"""Host-side launchers of the refine kernels (csrc/refine.hip, include/polus_hip.h "refine"): torch tensors in, raw pointers
through the C ABI, nothing computed here.  polus_amd/ops.py re-exports every function, so callers write ops.cls_rerank(...)
as for any other kernel; the module stands on _lib alone, like pq_ops.

The kernels take raw pointers, so these wrappers are the only place that sees a tensor's dtype, extent and strides: each
refuses what its kernel would misread, before the call, with a message that starts "<wrapper>: <parameter>"."""
import torch

from . import _lib
from ._lib import check, ptr

CLS_E_MAX, CLS_ROWS_MAX = 5120, 65535
_VEC = (torch.float32, torch.bfloat16)


def _got(t):
    return f"(got {t.dtype} {list(t.shape)}, strides {list(t.stride())})"


def _req_cuda(*ts):
    for t in ts:
        if not t.is_cuda:
            raise _lib.PolusHipError("polus_amd ops need device (HBM) tensors; there is no CPU path")


def _check_e(op, name, t, E):
    assert 16 <= E <= CLS_E_MAX and E % 16 == 0, f"{op}: {name} needs E a multiple of 16 in [16, {CLS_E_MAX}] {_got(t)}"


def _vectors(op, name, t, dtypes, rows, E):
    """Rows the kernel gathers in 16-byte pieces: a 2-D tensor of one of `dtypes`, `rows` x E (None: any number >= 1), inner
    stride one, a row stride >= E that keeps every row 16-byte aligned, a 16-byte aligned base; returns (rows, row stride)."""
    per = 16 // t.element_size() if t.dtype in dtypes else 1
    assert t.dtype in dtypes and t.dim() == 2 and t.shape[1] == E and t.shape[0] >= 1 and (rows is None or t.shape[0] == rows) \
        and t.stride(1) == 1 and (t.shape[0] == 1 or (t.stride(0) >= E and t.stride(0) % per == 0)) and t.data_ptr() % 16 == 0, \
        f"{op}: {name} must be {' or '.join(str(d) for d in dtypes)} [{'rows' if rows is None else rows}, {E}] with a unit inner " \
        f"stride, a row stride >= {E} that is a multiple of {per} elements (16 bytes) and a 16-byte aligned base {_got(t)}"
    ld = t.stride(0) if t.shape[0] > 1 else E
    return t.shape[0], ld


def _grid(op, name, t, dtype, rows, cols):
    """cand / score: a 2-D tensor of `dtype`, exactly rows x cols, inner stride one, rows that do not overlap; its row stride."""
    assert t.dtype == dtype and t.dim() == 2 and tuple(t.shape) == (rows, cols) and (t.stride(1) == 1 or cols == 1) \
        and (t.stride(0) >= cols or rows == 1), \
        f"{op}: {name} must be {dtype} [{rows}, {cols}] with a unit inner stride and a row stride >= {cols} {_got(t)}"
    return max(t.stride(0), cols)


def _check_launch(op, q, cand):
    assert q.dim() == 2 and q.dtype in _VEC, f"{op}: q must be f32 or bf16 [B, E] {_got(q)}"
    _check_e(op, "q", q, q.shape[1])
    assert 1 <= q.shape[0] <= CLS_ROWS_MAX, f"{op}: q holds {q.shape[0]} queries, a launch takes 1 .. {CLS_ROWS_MAX}"
    assert cand.dim() == 2 and cand.dtype == torch.int32 and 1 <= cand.shape[1] <= CLS_ROWS_MAX, \
        f"{op}: cand must be int32 [{q.shape[0]}, C] with 1 <= C <= {CLS_ROWS_MAX} {_got(cand)}"


def cls_rerank(q, d, cand, score):
    """score[b, c] (f32 [B, C], any row stride) = <q[b], d[n]> for n = cand[b, c] (int32 [B, C], any row stride); an id outside
    [0, N) gives -inf and nothing is read for it; a repeated id is scored once per copy.  q [B, E] and d [N, E] f32 or bf16,
    the same dtype, unit inner stride, 16-byte aligned rows (a column view of a wider matrix is fine); E a multiple of 16 in
    [16, 5120]; B and C at most 65535.  The sum's order is a function of E alone and the bits of a score depend on its
    (query, document) pair only (include/polus_hip.h polus_cls_rerank)."""
    op = "cls_rerank"
    _req_cuda(q, d, cand, score)
    _check_launch(op, q, cand)
    (B, E), C = q.shape, cand.shape[1]
    _, ldq = _vectors(op, "q", q, _VEC, None, E)
    N, ldd = _vectors(op, "d", d, (q.dtype,), None, E)
    ldcand = _grid(op, "cand", cand, torch.int32, B, C)
    lds = _grid(op, "score", score, torch.float32, B, C)
    check(_lib.load().polus_cls_rerank(_lib.dtype_code(q.dtype), ptr(q), ldq, ptr(d), ldd, ptr(cand), ldcand, ptr(score), lds,
                                       B, C, N, E, _lib.current_stream()), "polus_cls_rerank")


def cls_rerank_fp8(q, codes, scale, cand, score):
    """cls_rerank over documents stored as e4m3fn codes uint8 [N, E] (unit inner stride, 16-byte aligned rows) with one
    power-of-two scale f32 [N] (contiguous) each: score = scale[n] * the sum over f32(q) * f32(code) in cls_rerank's order,
    bit for bit cls_rerank over the dequantised matrix unless a product or partial sum under- or overflows.  q stays f32 or
    bf16 (include/polus_hip.h polus_cls_rerank_fp8)."""
    op = "cls_rerank_fp8"
    _req_cuda(q, codes, scale, cand, score)
    _check_launch(op, q, cand)
    (B, E), C = q.shape, cand.shape[1]
    _, ldq = _vectors(op, "q", q, _VEC, None, E)
    N, ldd = _vectors(op, "codes", codes, (torch.uint8,), None, E)
    assert scale.dtype == torch.float32 and tuple(scale.shape) == (N,) and scale.is_contiguous(), \
        f"{op}: scale must be contiguous f32 [{N}] {_got(scale)}"
    ldcand = _grid(op, "cand", cand, torch.int32, B, C)
    lds = _grid(op, "score", score, torch.float32, B, C)
    check(_lib.load().polus_cls_rerank_fp8(_lib.dtype_code(q.dtype), ptr(q), ldq, ptr(codes), ldd, ptr(scale), ptr(cand), ldcand,
                                           ptr(score), lds, B, C, N, E, _lib.current_stream()), "polus_cls_rerank_fp8")


def _check_rows(op, xname, x, codes, scale):
    assert x.dim() == 2 and x.dtype in _VEC and x.shape[0] >= 1 and x.is_contiguous() and x.data_ptr() % 16 == 0, \
        f"{op}: {xname} must be contiguous f32 or bf16 [rows >= 1, E], 16-byte aligned {_got(x)}"
    rows, E = x.shape
    _check_e(op, xname, x, E)
    assert codes.dtype == torch.uint8 and tuple(codes.shape) == (rows, E) and codes.is_contiguous() and codes.data_ptr() % 16 == 0, \
        f"{op}: codes must be contiguous uint8 [{rows}, {E}], 16-byte aligned {_got(codes)}"
    assert scale.dtype == torch.float32 and tuple(scale.shape) == (rows,) and scale.is_contiguous(), \
        f"{op}: scale must be contiguous f32 [{rows}] {_got(scale)}"
    return rows, E


def cls_fp8_quantize(x, codes, scale):
    """codes (uint8 [rows, E]) and scale (f32 [rows]) of the rows of x (f32 or bf16 [rows, E]), all contiguous: the quantiser
    of fp8_quantize, one power-of-two scale per row and nothing saturating, over whole vectors of up to 5120 features, E a
    multiple of 16 (include/polus_hip.h polus_cls_fp8_quantize)."""
    _req_cuda(x, codes, scale)
    rows, E = _check_rows("cls_fp8_quantize", "x", x, codes, scale)
    check(_lib.load().polus_cls_fp8_quantize(_lib.dtype_code(x.dtype), ptr(x), ptr(codes), ptr(scale), rows, E,
                                             _lib.current_stream()), "polus_cls_fp8_quantize")


def cls_fp8_dequantize(codes, scale, y):
    """y (f32 or bf16 [rows, E], contiguous) = T(codes) * scale, exact (include/polus_hip.h polus_cls_fp8_dequantize)."""
    _req_cuda(codes, scale, y)
    rows, E = _check_rows("cls_fp8_dequantize", "y", y, codes, scale)
    check(_lib.load().polus_cls_fp8_dequantize(_lib.dtype_code(y.dtype), ptr(codes), ptr(scale), ptr(y), rows, E,
                                               _lib.current_stream()), "polus_cls_fp8_dequantize")
