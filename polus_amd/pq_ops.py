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


# ---------------------------------------------------------------- IVF-PQ (csrc/ivfpq.hip, include/polus_hip.h "IVF-PQ")
IVFPQ_K_MAX, IVFPQ_E_MAX = 65535, 5120
IvfPqRoute = collections.namedtuple("IvfPqRoute", "lds_bytes cols_per_block")
_I16 = (torch.int16,)


def _coarse(op, name, t, n):
    """Coarse codes: contiguous int16 [n] holding the unsigned bits (0xFFFF, or any code >= K: no list)."""
    assert t.dtype == torch.int16 and t.dim() == 1 and t.shape[0] == n and t.is_contiguous(), \
        f"{op}: {name} must be contiguous int16 [{n}] (the bits of the unsigned code) {_got(t)}"


def _centroids(op, name, c, dtype):
    """(K, E) of contiguous centroids [K, E] of `dtype` within the format's limits."""
    assert c.dtype == dtype and c.dim() == 2 and c.is_contiguous() and 1 <= c.shape[0] <= IVFPQ_K_MAX \
        and 1 <= c.shape[1] <= IVFPQ_E_MAX, \
        f"{op}: {name} must be contiguous {dtype} [K, E] with 1 <= K <= {IVFPQ_K_MAX} and 1 <= E <= {IVFPQ_E_MAX} {_got(c)}"
    return c.shape


def ivfpq_residual(x, cent, coarse, r):
    """r[t, e] (f32 [rows, E], any row stride) = f32(x[t, e]) - f32(cent[coarse[t], e]), one rounding; zeros for a row whose
    coarse code is >= K.  x f32 or bf16 [rows, E] (any row stride), cent [K, E] contiguous in x's dtype, coarse int16 [rows]
    (include/polus_hip.h polus_ivfpq_residual)."""
    _req_cuda(x, cent, coarse, r)
    assert x.dtype in _VEC, f"ivfpq_residual: x must be f32 or bf16 {_got(x)}"
    K, E = _centroids("ivfpq_residual", "cent", cent, x.dtype)
    rows, ldx = _rows("ivfpq_residual", "x", x, _VEC, None, E)
    _coarse("ivfpq_residual", "coarse", coarse, rows)
    _, ldr = _rows("ivfpq_residual", "r", r, (torch.float32,), rows, E)
    check(_lib.load().polus_ivfpq_residual(_lib.dtype_code(x.dtype), ptr(x), ldx, ptr(cent), ptr(coarse), ptr(r), ldr, rows, K, E,
                                           _lib.current_stream()), "polus_ivfpq_residual")


def ivfpq_coarse_update(x, coarse, prev, out, counts):
    """One Lloyd update of whole vectors: out[k] = the f32 sum of the rows x[t] with coarse[t] == k divided by their number
    counts[k] (int32 [K]), rounded once to x's dtype; prev[k] where there is none.  The sum's order is a function of T
    alone.  x f32 or bf16 [T, E] (any row stride), coarse int16 [T], prev / out [K, E] contiguous in x's dtype, buffers
    that do not overlap (include/polus_hip.h polus_ivfpq_coarse_update)."""
    _req_cuda(x, coarse, prev, out, counts)
    assert x.dtype in _VEC, f"ivfpq_coarse_update: x must be f32 or bf16 {_got(x)}"
    K, E = _centroids("ivfpq_coarse_update", "prev", prev, x.dtype)
    assert out.dtype == x.dtype and tuple(out.shape) == (K, E) and out.is_contiguous(), \
        f"ivfpq_coarse_update: out must be contiguous {x.dtype} {[K, E]} like prev {_got(out)}"
    T, ldx = _rows("ivfpq_coarse_update", "x", x, _VEC, None, E)
    _coarse("ivfpq_coarse_update", "coarse", coarse, T)
    assert counts.dtype == torch.int32 and tuple(counts.shape) == (K,) and counts.is_contiguous(), \
        f"ivfpq_coarse_update: counts must be contiguous int32 {[K]} {_got(counts)}"
    nbytes = prev.numel() * prev.element_size()
    assert out.data_ptr() + nbytes <= prev.data_ptr() or prev.data_ptr() + nbytes <= out.data_ptr(), \
        "ivfpq_coarse_update: out must not overlap prev"
    check(_lib.load().polus_ivfpq_coarse_update(_lib.dtype_code(x.dtype), ptr(x), ldx, ptr(coarse), ptr(prev), ptr(out), ptr(counts),
                                                T, K, E, _lib.current_stream()), "polus_ivfpq_coarse_update")


def ivfpq_scores_ids(lut, cdot, coarse, codes, cand, score):
    """score[b, c] (f32 [Q, C], any row stride) = cdot[b, coarse[n]] + sum over j of lut[b, j, codes[n, j]] for n = cand[b, c]
    (int32 [Q, C], any row stride), the sum sequential in ascending j and one more rounding for the centroid's term; an id
    outside [0, N), a coarse code >= K or a code byte >= ksub gives -inf.  cand=None: column c is document c and C = N.  lut
    f32 [Q, m, ksub] contiguous (pq_lut with the residual codebook), cdot f32 [Q, K] (any row stride), coarse int16 [N], codes
    uint8 [N, m] (any row stride); Q and C at most 65535 (include/polus_hip.h polus_ivfpq_scores_ids)."""
    _req_cuda(lut, cdot, coarse, codes, score, *(() if cand is None else (cand,)))
    assert lut.dtype == torch.float32 and lut.dim() == 3 and lut.is_contiguous(), \
        f"ivfpq_scores_ids: lut must be contiguous f32 [Q, m, ksub] {_got(lut)}"
    Q, m, ksub = lut.shape
    N, ldc = _rows("ivfpq_scores_ids", "codes", codes, _U8, None, m)
    assert cdot.dim() == 2 and 1 <= cdot.shape[1] <= IVFPQ_K_MAX, \
        f"ivfpq_scores_ids: cdot must be f32 [{Q}, K] with 1 <= K <= {IVFPQ_K_MAX} {_got(cdot)}"
    K = cdot.shape[1]
    _, ldd = _rows("ivfpq_scores_ids", "cdot", cdot, (torch.float32,), Q, K)
    _coarse("ivfpq_scores_ids", "coarse", coarse, N)
    if cand is None:
        C, ldcand = N, 0
    else:
        assert cand.dim() == 2 and cand.shape[1] >= 1, f"ivfpq_scores_ids: cand must be int32 [{Q}, C] with C >= 1 {_got(cand)}"
        C = cand.shape[1]
        _, ldcand = _rows("ivfpq_scores_ids", "cand", cand, (torch.int32,), Q, C)
    _check_scan("ivfpq_scores_ids", Q, 1, m, ksub)              # the format and Q; the columns are checked here
    assert C <= 65535, f"ivfpq_scores_ids: {'cand' if cand is not None else 'codes'} holds {C} columns, a launch takes 1 .. 65535"
    _, lds = _rows("ivfpq_scores_ids", "score", score, (torch.float32,), Q, C)
    check(_lib.load().polus_ivfpq_scores_ids(ptr(lut), ptr(cdot), ldd, ptr(coarse), ptr(codes), ldc, ptr(cand), ldcand, ptr(score),
                                             lds, Q, C, N, m, ksub, K, _lib.current_stream()), "polus_ivfpq_scores_ids")


def ivfpq_scores_ids_route(Q, C, m, ksub):
    """What `ivfpq_scores_ids` runs for these shapes (polus_ivfpq_scores_ids_route): the dynamic LDS bytes of a workgroup and
    the candidate columns it serves; launches nothing and refuses the shapes ivfpq_scores_ids refuses."""
    r = (ctypes.c_int * 2)()
    check(_lib.load().polus_ivfpq_scores_ids_route(int(Q), int(C), int(m), int(ksub), r), "polus_ivfpq_scores_ids_route")
    return IvfPqRoute(r[0], r[1])
