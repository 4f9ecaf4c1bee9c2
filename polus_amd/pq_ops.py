"""Host-side launchers of the product-quantisation kernels (csrc/pq.hip, include/polus_hip.h "product quantisation"):
torch tensors in, raw pointers through the C ABI, nothing computed here.  polus_amd/ops.py re-exports every function, so
callers write ops.pq_encode(...) as for any other kernel; the module stands on _lib alone, so either can be imported first.

The kernels take raw pointers, so these wrappers are the only place that sees a tensor's dtype, extent and strides: each
refuses what its kernel would misread, before the call, with a message that starts "<wrapper>: <parameter>"."""
import collections
import ctypes

import torch

from . import _lib
from ._lib import check, ptr

PQ_M_MAX, PQ_KSUB_MAX, PQ_DSUB_MAX = 160, 256, 32
PqRoute = collections.namedtuple("PqRoute", "qt lds_bytes")


def _got(t):
    return f"(got {t.dtype} {list(t.shape)}, strides {list(t.stride())})"


def _req_cuda(*ts):
    for t in ts:
        if not t.is_cuda:
            raise _lib.PolusHipError("polus_amd ops need device (HBM) tensors; there is no CPU path")


def _codebook(op, name, cb):
    """(m, ksub, dsub) of a contiguous f32 [m, ksub, dsub] codebook within the format's limits."""
    assert cb.dtype == torch.float32 and cb.dim() == 3 and cb.is_contiguous(), \
        f"{op}: {name} must be contiguous f32 [m, ksub, dsub] {_got(cb)}"
    m, ksub, dsub = cb.shape
    assert 4 <= m <= PQ_M_MAX and m % 4 == 0 and 1 <= ksub <= PQ_KSUB_MAX and 1 <= dsub <= PQ_DSUB_MAX, \
        f"{op}: {name} needs m a multiple of 4 in [4, {PQ_M_MAX}], 1 <= ksub <= {PQ_KSUB_MAX}, 1 <= dsub <= {PQ_DSUB_MAX} {_got(cb)}"
    return m, ksub, dsub


def _rows(op, name, t, dtypes, rows, cols):
    """A pointer and a row stride: a 2-D tensor of one of `dtypes`, exactly `rows` x `cols` (None: any number >= 1 of
    rows), inner stride one, rows that do not overlap; returns (rows, row stride)."""
    assert t.dtype in dtypes and t.dim() == 2 and t.shape[1] == cols and t.shape[0] >= 1 and (rows is None or t.shape[0] == rows) \
        and (t.stride(1) == 1 or cols == 1) and (t.stride(0) >= cols or t.shape[0] == 1), \
        f"{op}: {name} must be {' or '.join(str(d) for d in dtypes)} [{'rows' if rows is None else rows}, {cols}] with a unit " \
        f"inner stride and a row stride >= {cols} {_got(t)}"
    return t.shape[0], max(t.stride(0), cols)


_VEC = (torch.float32, torch.bfloat16)
_U8 = (torch.uint8,)


def pq_encode(x, codebook, codes):
    """codes[r, j] (uint8 [rows, m], any row stride) = the nearest codeword of sub-space j to x[r, j * dsub : (j + 1) * dsub]
    by squared distance, ties to the lower code, NaN never winning.  x f32 or bf16 [rows, m * dsub] (any row stride),
    codebook f32 [m, ksub, dsub] (include/polus_hip.h polus_pq_encode)."""
    _req_cuda(x, codebook, codes)
    m, ksub, dsub = _codebook("pq_encode", "codebook", codebook)
    rows, ldx = _rows("pq_encode", "x", x, _VEC, None, m * dsub)
    _, ldc = _rows("pq_encode", "codes", codes, _U8, rows, m)
    check(_lib.load().polus_pq_encode(_lib.dtype_code(x.dtype), ptr(x), ldx, ptr(codebook), ptr(codes), ldc, rows, m, ksub, dsub,
                                      _lib.current_stream()), "polus_pq_encode")


def pq_update(x, codes, prev, out, counts):
    """One Lloyd update: out[j, c] = the f32 sum of the sub-vectors j of the rows with codes[t, j] == c, divided by their
    number counts[j, c] (int32 [m, ksub]); prev[j, c] where there is none.  The sum's order is a function of T alone.
    x f32 or bf16 [T, m * dsub], codes uint8 [T, m] (any row strides), prev / out f32 [m, ksub, dsub], distinct buffers
    (include/polus_hip.h polus_pq_update)."""
    _req_cuda(x, codes, prev, out, counts)
    m, ksub, dsub = _codebook("pq_update", "prev", prev)
    assert out.dtype == torch.float32 and tuple(out.shape) == (m, ksub, dsub) and out.is_contiguous(), \
        f"pq_update: out must be contiguous f32 {[m, ksub, dsub]} like prev {_got(out)}"
    T, ldx = _rows("pq_update", "x", x, _VEC, None, m * dsub)
    _, ldc = _rows("pq_update", "codes", codes, _U8, T, m)
    assert counts.dtype == torch.int32 and tuple(counts.shape) == (m, ksub) and counts.is_contiguous(), \
        f"pq_update: counts must be contiguous int32 {[m, ksub]} {_got(counts)}"
    nbytes = prev.numel() * 4
    assert out.data_ptr() + nbytes <= prev.data_ptr() or prev.data_ptr() + nbytes <= out.data_ptr(), "pq_update: out must not overlap prev"
    check(_lib.load().polus_pq_update(_lib.dtype_code(x.dtype), ptr(x), ldx, ptr(codes), ldc, ptr(prev), ptr(out), ptr(counts), T, m,
                                      ksub, dsub, _lib.current_stream()), "polus_pq_update")


def pq_decode(codes, codebook, y):
    """y[r, j * dsub + t] (f32 or bf16 [rows, m * dsub], any row stride) = codebook[j, codes[r, j], t] rounded once to y's
    dtype; a code >= ksub decodes to zeros.  codes uint8 [rows, m] (any row stride) (include/polus_hip.h polus_pq_decode)."""
    _req_cuda(codes, codebook, y)
    m, ksub, dsub = _codebook("pq_decode", "codebook", codebook)
    rows, ldc = _rows("pq_decode", "codes", codes, _U8, None, m)
    _, ldy = _rows("pq_decode", "y", y, _VEC, rows, m * dsub)
    check(_lib.load().polus_pq_decode(ptr(codes), ldc, ptr(codebook), _lib.dtype_code(y.dtype), ptr(y), ldy, rows, m, ksub, dsub,
                                      _lib.current_stream()), "polus_pq_decode")


def pq_lut(q, codebook, lut):
    """lut[b, j, c] (f32 [Q, m, ksub], contiguous) = <q[b, j * dsub : (j + 1) * dsub], codebook[j, c]>, a sequential f32 sum
    without fma.  q f32 or bf16 [Q, m * dsub] (any row stride) (include/polus_hip.h polus_pq_lut)."""
    _req_cuda(q, codebook, lut)
    m, ksub, dsub = _codebook("pq_lut", "codebook", codebook)
    Q, ldq = _rows("pq_lut", "q", q, _VEC, None, m * dsub)
    assert lut.dtype == torch.float32 and tuple(lut.shape) == (Q, m, ksub) and lut.is_contiguous(), \
        f"pq_lut: lut must be contiguous f32 {[Q, m, ksub]} {_got(lut)}"
    check(_lib.load().polus_pq_lut(_lib.dtype_code(q.dtype), ptr(q), ldq, ptr(codebook), ptr(lut), Q, m, ksub, dsub,
                                   _lib.current_stream()), "polus_pq_lut")


def _check_scan(op, Q, N, m, ksub):
    assert 4 <= m <= PQ_M_MAX and m % 4 == 0 and 1 <= ksub <= PQ_KSUB_MAX, \
        f"{op}: lut needs m a multiple of 4 in [4, {PQ_M_MAX}] and 1 <= ksub <= {PQ_KSUB_MAX} (got m = {m}, ksub = {ksub})"
    assert 1 <= Q <= 65535, f"{op}: lut holds {Q} queries, a launch takes 1 .. 65535"
    assert 1 <= N <= 65535, f"{op}: codes holds {N} documents, a launch takes 1 .. 65535"


def pq_scores(lut, codes, score):
    """score[b, n] (f32 [Q, N], any row stride) = sum over j of lut[b, j, codes[n, j]], a sequential f32 sum in ascending
    j; a code >= ksub reads -inf.  lut f32 [Q, m, ksub] contiguous (pq_lut), codes uint8 [N, m] (any row stride); Q and N
    at most 65535 (include/polus_hip.h polus_pq_scores)."""
    _req_cuda(lut, codes, score)
    assert lut.dtype == torch.float32 and lut.dim() == 3 and lut.is_contiguous(), f"pq_scores: lut must be contiguous f32 [Q, m, ksub] {_got(lut)}"
    Q, m, ksub = lut.shape
    N, ldc = _rows("pq_scores", "codes", codes, _U8, None, m)
    _check_scan("pq_scores", Q, N, m, ksub)
    _, lds = _rows("pq_scores", "score", score, (torch.float32,), Q, N)
    check(_lib.load().polus_pq_scores(ptr(lut), ptr(codes), ldc, ptr(score), lds, Q, N, m, ksub, _lib.current_stream()),
          "polus_pq_scores")


def pq_scores_route(Q, N, m, ksub):
    """What `pq_scores` runs for these shapes (polus_pq_scores_route): the queries whose tables one workgroup holds and
    its dynamic LDS bytes; launches nothing and refuses what pq_scores refuses."""
    r = (ctypes.c_int * 2)()
    check(_lib.load().polus_pq_scores_route(int(Q), int(N), int(m), int(ksub), r), "polus_pq_scores_route")
    return PqRoute(r[0], r[1])
