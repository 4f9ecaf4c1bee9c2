// Exact refine stage of the single-vector ([CLS]) indexes (polus_amd/ir/search.py: CorpusIndex(refine=...), rerank):
// every query scores its OWN candidate ids against stored whole vectors, in the model's dtype or as e4m3fn codes with one
// power-of-two scale per document.  Rules, order of the sum and limits: include/polus_hip.h "refine".
//
// polus_cls_rerank / polus_cls_rerank_fp8 are a gather of whole rows (1.5 KB at E = 768 in bf16), bound by memory
// latency.  One workgroup of 4 waves serves one query and a contiguous range of its candidate columns; a wave owns a
// candidate from the load to the store, so the candidate id is wave-uniform.  Lane l keeps the query's feature groups
// l, l + 64, ... (8 consecutive features each) in registers for the whole launch and reads the same groups of a
// document: 16 bytes a lane in bf16, 32 in f32, 8 as codes, the wave's lanes covering consecutive memory.  A wave takes
// U candidates at a time and issues the loads of the next U before it reduces the current ones (2 U rows in flight per
// wave).  The six cross-lane rounds go through DPP (1, 2), swizzles (4, 8, 16) and one bpermute (32): no LDS is
// allocated.  The partial of lane l and the xor tree are the header's rule, a function of E alone, so a score's bits
// depend on its (query, document) pair only.  The file compiles without contraction: every operation is one rounding.
#include <algorithm>

#include "fp8_common.h"

#pragma clang fp contract(off)

namespace {

constexpr int RF_EMAX = 5120;
constexpr int RF_ROWS_MAX = 65535;
constexpr int RF_WAVES = 4;                       // waves per workgroup

// ---------------------------------------------------------------- 8 consecutive features of a stored row
template <typename D> struct Piece;
template <> struct Piece<bf16_t> { uint4 r; };
template <> struct Piece<float> { float4 a, b; };
template <> struct Piece<uint8_t> { uint2 r; };

__device__ __forceinline__ void piece_load(Piece<bf16_t>& p, const bf16_t* at) { p.r = *reinterpret_cast<const uint4*>(at); }
__device__ __forceinline__ void piece_load(Piece<float>& p, const float* at) {
    p.a = *reinterpret_cast<const float4*>(at);
    p.b = *reinterpret_cast<const float4*>(at + 4);
}
__device__ __forceinline__ void piece_load(Piece<uint8_t>& p, const uint8_t* at) { p.r = *reinterpret_cast<const uint2*>(at); }
__device__ __forceinline__ void piece_zero(Piece<bf16_t>& p) { p.r = make_uint4(0, 0, 0, 0); }
__device__ __forceinline__ void piece_zero(Piece<float>& p) { p.a = p.b = make_float4(0.f, 0.f, 0.f, 0.f); }
__device__ __forceinline__ void piece_zero(Piece<uint8_t>& p) { p.r = make_uint2(0, 0); }

// widened to f32, exact
__device__ __forceinline__ void piece_widen(const Piece<bf16_t>& p, float (&v)[8]) {
    const unsigned w[4] = {p.r.x, p.r.y, p.r.z, p.r.w};
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        v[2 * k] = __uint_as_float(w[k] << 16);
        v[2 * k + 1] = __uint_as_float(w[k] & 0xffff0000u);
    }
}
__device__ __forceinline__ void piece_widen(const Piece<float>& p, float (&v)[8]) {
    v[0] = p.a.x; v[1] = p.a.y; v[2] = p.a.z; v[3] = p.a.w;
    v[4] = p.b.x; v[5] = p.b.y; v[6] = p.b.z; v[7] = p.b.w;
}
__device__ __forceinline__ void piece_widen(const Piece<uint8_t>& p, float (&v)[8]) {
    const f32x2 a = __builtin_amdgcn_cvt_pk_f32_fp8((int)p.r.x, false), b = __builtin_amdgcn_cvt_pk_f32_fp8((int)p.r.x, true);
    const f32x2 c = __builtin_amdgcn_cvt_pk_f32_fp8((int)p.r.y, false), d = __builtin_amdgcn_cvt_pk_f32_fp8((int)p.r.y, true);
    v[0] = a[0]; v[1] = a[1]; v[2] = b[0]; v[3] = b[1];
    v[4] = c[0]; v[5] = c[1]; v[6] = d[0]; v[7] = d[1];
}

// the value of lane (l xor O)
template <int O> __device__ __forceinline__ float lane_xor(float v) {
    const int x = __float_as_int(v);
    if constexpr (O == 1) return __int_as_float(__builtin_amdgcn_mov_dpp(x, 0xB1, 0xF, 0xF, true));        // quad_perm [1,0,3,2]
    else if constexpr (O == 2) return __int_as_float(__builtin_amdgcn_mov_dpp(x, 0x4E, 0xF, 0xF, true));   // quad_perm [2,3,0,1]
    else if constexpr (O <= 16) return __int_as_float(__builtin_amdgcn_ds_swizzle(x, (O << 10) | 0x1F));   // bit mode: xor O
    else return __shfl_xor(v, 32, 64);
}
// p_l = fl(p_l + p_(l xor o)) for o = 32, 16, 8, 4, 2, 1: every lane ends with the same bits
__device__ __forceinline__ float xor_tree(float p) {
    p = p + lane_xor<32>(p);
    p = p + lane_xor<16>(p);
    p = p + lane_xor<8>(p);
    p = p + lane_xor<4>(p);
    p = p + lane_xor<2>(p);
    p = p + lane_xor<1>(p);
    return p;
}

// The rows of the wave's next U columns c0, c0 + 4, ...: ids (-1: absent or past the range), scales and pieces.  Nothing
// is read for an absent candidate; a lane without a group j holds zeros, which add +0.0 to a partial that is never -0.0.
template <typename D, int NG, int U>
__device__ __forceinline__ void fetch(const D* __restrict__ Dm, long ldd, const float* __restrict__ scale,
                                      const int32_t* __restrict__ crow, int c0, int c_hi, int N, int G, int lane,
                                      Piece<D> (&p)[U][NG], int (&n)[U], float (&sc)[U]) {
#pragma unroll
    for (int u = 0; u < U; ++u) {
        const int c = c0 + RF_WAVES * u;
        int id = -1;
        if (c < c_hi) id = __builtin_amdgcn_readfirstlane(crow[c]);
        if (id >= N) id = -1;
        n[u] = id;
        sc[u] = 1.f;
        if (id >= 0) {                                                   // wave-uniform
            const D* row = Dm + (size_t)id * ldd;
            if constexpr (sizeof(D) == 1) sc[u] = scale[id];
#pragma unroll
            for (int j = 0; j < NG; ++j) {
                const int g = lane + 64 * j;
                if (g < G) piece_load(p[u][j], row + 8 * g);
                else piece_zero(p[u][j]);
            }
        } else {
#pragma unroll
            for (int j = 0; j < NG; ++j) piece_zero(p[u][j]);
        }
    }
}

// T: the queries' type; D: what a stored row holds (T, or uint8_t codes beside `scale`); NG: feature groups a lane
// holds, ceil(E / 512) at most; U: candidates a wave takes at a time.
template <typename T, typename D, int NG, int U>
__global__ __launch_bounds__(64 * RF_WAVES) void cls_rerank_kernel(
    const T* __restrict__ Q, long ldq, const D* __restrict__ Dm, long ldd, const float* __restrict__ scale,
    const int32_t* __restrict__ cand, long ldcand, float* __restrict__ score, long lds, int C, int N, int E, int cpb) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int b = blockIdx.y, G = E >> 3;

    float q[NG][8];
    const T* qrow = Q + (size_t)b * ldq;
#pragma unroll
    for (int j = 0; j < NG; ++j) {
        const int g = lane + 64 * j;
        Piece<T> t;
        if (g < G) piece_load(t, qrow + 8 * g);
        else piece_zero(t);
        piece_widen(t, q[j]);
    }

    const int c_lo = blockIdx.x * cpb, c_hi = min(C, c_lo + cpb);
    const int32_t* crow = cand + (size_t)b * ldcand;
    float* srow = score + (size_t)b * lds;

    Piece<D> cur[U][NG], nxt[U][NG];
    int ncur[U], nnxt[U];
    float scur[U], snxt[U];
    int c0 = c_lo + wave;
    fetch<D, NG, U>(Dm, ldd, scale, crow, c0, c_hi, N, G, lane, cur, ncur, scur);
    for (; c0 < c_hi; c0 += RF_WAVES * U) {                              // wave-uniform
        fetch<D, NG, U>(Dm, ldd, scale, crow, c0 + RF_WAVES * U, c_hi, N, G, lane, nxt, nnxt, snxt);
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int c = c0 + RF_WAVES * u;
            if (c >= c_hi) continue;
            float p = 0.f;
#pragma unroll
            for (int j = 0; j < NG; ++j) {
                float d[8];
                piece_widen(cur[u][j], d);
#pragma unroll
                for (int i = 0; i < 8; ++i) p = p + q[j][i] * d[i];
            }
            p = xor_tree(p);
            if constexpr (sizeof(D) == 1) p = scur[u] * p;
            if (lane == 0) srow[c] = ncur[u] >= 0 ? p : -INFINITY;
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            ncur[u] = nnxt[u];
            scur[u] = snxt[u];
#pragma unroll
            for (int j = 0; j < NG; ++j) cur[u][j] = nxt[u][j];
        }
    }
}

// Columns per workgroup: about 16 waves per CU over the launch, a wave taking at least one column and at most 64.
int rf_cols_per_block(int B, int C) {
    const long waves = 16L * polus_num_cus();
    const long per_wave = std::min(64L, std::max(1L, ((long)B * C + waves - 1) / waves));
    return (int)(RF_WAVES * per_wave);
}

template <typename T, typename D, int NG, int U>
int rf_launch(const char* what, const void* Q, long ldq, const void* Dm, long ldd, const float* scale, const int32_t* cand,
              long ldcand, float* score, long lds, int B, int C, int N, int E, hipStream_t st) {
    const int cpb = rf_cols_per_block(B, C);
    dim3 grid((unsigned)((C + cpb - 1) / cpb), (unsigned)B);
    hipLaunchKernelGGL((cls_rerank_kernel<T, D, NG, U>), grid, dim3(64 * RF_WAVES), 0, st, static_cast<const T*>(Q), ldq,
                       static_cast<const D*>(Dm), ldd, scale, cand, ldcand, score, lds, C, N, E, cpb);
    POLUS_CHECK_LAUNCH(what);
    return POLUS_OK;
}

template <typename T, typename D>
int rf_by_groups(const char* what, const void* Q, long ldq, const void* Dm, long ldd, const float* scale, const int32_t* cand,
                 long ldcand, float* score, long lds, int B, int C, int N, int E, hipStream_t st) {
    const int ng = (E / 8 + 63) / 64;                                    // 1 .. 10
#define RF_GO(NG, U) return rf_launch<T, D, NG, U>(what, Q, ldq, Dm, ldd, scale, cand, ldcand, score, lds, B, C, N, E, st)
    if (ng <= 1) RF_GO(1, 4);
    if (ng <= 2) RF_GO(2, 4);
    if (ng <= 3) RF_GO(3, 2);
    if (ng <= 4) RF_GO(4, 2);
    RF_GO(10, 1);
#undef RF_GO
}

// d_bytes: the size of a stored element (the queries' own, or 1 for codes, which come with `scale`)
int rf_check(const char* what, int dtype, const void* Q, long ldq, const void* Dm, long ldd, const char* dname, size_t d_bytes,
             const void* scale, const int32_t* cand, long ldcand, const float* score, long lds, int B, int C, int N, int E) {
    POLUS_REQUIRE(dtype == POLUS_F32 || dtype == POLUS_BF16, "%s: unknown dtype %d", what, dtype);
    POLUS_REQUIRE(E >= 16 && E <= RF_EMAX && E % 16 == 0, "%s: E must be a multiple of 16 in [16, %d] (got %d)", what, RF_EMAX, E);
    POLUS_REQUIRE(B >= 1 && B <= RF_ROWS_MAX, "%s: need 1 <= B <= %d (got %d)", what, RF_ROWS_MAX, B);
    POLUS_REQUIRE(C >= 1 && C <= RF_ROWS_MAX, "%s: need 1 <= C <= %d (got %d)", what, RF_ROWS_MAX, C);
    POLUS_REQUIRE(N >= 1, "%s: need 1 <= N <= 2^31 - 1 (got %d)", what, N);
    POLUS_REQUIRE(ldq >= E, "%s: query row stride ldq must be >= E (got %ld < %d)", what, ldq, E);
    POLUS_REQUIRE(ldd >= E, "%s: %s row stride ldd must be >= E (got %ld < %d)", what, dname, ldd, E);
    POLUS_REQUIRE(ldcand >= C, "%s: candidate row stride ldcand must be >= C (got %ld < %d)", what, ldcand, C);
    POLUS_REQUIRE(lds >= C, "%s: score row stride lds must be >= C (got %ld < %d)", what, lds, C);
    POLUS_REQUIRE(Q && Dm && (scale || d_bytes != 1) && cand && score, "%s: null pointer", what);
    POLUS_REQUIRE(polus_aligned16(Q) && polus_aligned16(Dm), "%s: Q and %s must be 16-byte aligned", what, dname);
    POLUS_REQUIRE((ldq * (long)polus_dtype_size(dtype)) % 16 == 0 && (ldd * (long)d_bytes) % 16 == 0,
                  "%s: the row strides must keep every row 16-byte aligned (got ldq = %ld, ldd = %ld)", what, ldq, ldd);
    return POLUS_OK;
}

// ---------------------------------------------------------------- the quantiser over whole rows: one wave per row, two passes
template <typename T>
__global__ __launch_bounds__(256) void cls_fp8_quantize_kernel(const T* __restrict__ x, uint8_t* __restrict__ codes,
                                                               float* __restrict__ scale, int rows, int E) {
    const int lane = threadIdx.x & 63;
    const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;                                             // the whole wave
    const T* xr = x + (size_t)row * E;
    float amax = 0.f;                                                    // fmaxf ignores a NaN element
    for (int e0 = 4 * lane; e0 < E; e0 += 256) {
        float v[4];
        load4<T>(xr + e0, v);
        amax = fmaxf(amax, fmaxf(fmaxf(fabsf(v[0]), fabsf(v[1])), fmaxf(fabsf(v[2]), fabsf(v[3]))));
    }
    amax = wave_max(amax);
    const int e = f8_row_exponent(amax);
    const float inv = f8_pow2(-e);
    for (int e0 = 4 * lane; e0 < E; e0 += 256) {
        float v[4];
        load4<T>(xr + e0, v);
        *reinterpret_cast<int*>(codes + (size_t)row * E + e0) = f8_pack4(v, inv);
    }
    if (lane == 0) scale[row] = f8_pow2(e);
}

template <typename T>
__global__ __launch_bounds__(256) void cls_fp8_dequantize_kernel(const uint8_t* __restrict__ codes, const float* __restrict__ scale,
                                                                 T* __restrict__ y, int rows, int E) {
    const int lane = threadIdx.x & 63;
    const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    const float s = scale[row];
    for (int e0 = 4 * lane; e0 < E; e0 += 256) {
        float v[4];
        f8_unpack4(*reinterpret_cast<const int*>(codes + (size_t)row * E + e0), s, v);
        store4<T>(y + (size_t)row * E + e0, v);
    }
}

int rf_rows_check(const char* what, int dtype, const void* a, const void* b, const void* c, int rows, int E) {
    POLUS_REQUIRE(dtype == POLUS_F32 || dtype == POLUS_BF16, "%s: unknown dtype %d", what, dtype);
    POLUS_REQUIRE(rows >= 1, "%s: need rows >= 1 (got %d)", what, rows);
    POLUS_REQUIRE(E >= 16 && E <= RF_EMAX && E % 16 == 0, "%s: E must be a multiple of 16 in [16, %d] (got %d)", what, RF_EMAX, E);
    POLUS_REQUIRE(a && b && c, "%s: null pointer", what);
    return POLUS_OK;
}

}  // namespace

extern "C" int polus_cls_rerank(int dtype, const void* Q, long ldq, const void* D, long ldd, const int32_t* cand, long ldcand,
                                float* score, long lds, int B, int C, int N, int E, void* stream) {
    const char* what = "polus_cls_rerank";
    if (int rc = rf_check(what, dtype, Q, ldq, D, ldd, "D", polus_dtype_size(dtype), nullptr, cand, ldcand, score, lds, B, C, N, E))
        return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (dtype == POLUS_BF16)
        return rf_by_groups<bf16_t, bf16_t>(what, Q, ldq, D, ldd, nullptr, cand, ldcand, score, lds, B, C, N, E, st);
    return rf_by_groups<float, float>(what, Q, ldq, D, ldd, nullptr, cand, ldcand, score, lds, B, C, N, E, st);
}

extern "C" int polus_cls_rerank_fp8(int dtype, const void* Q, long ldq, const uint8_t* codes, long ldd, const float* scale,
                                    const int32_t* cand, long ldcand, float* score, long lds, int B, int C, int N, int E,
                                    void* stream) {
    const char* what = "polus_cls_rerank_fp8";
    if (int rc = rf_check(what, dtype, Q, ldq, codes, ldd, "codes", 1, scale, cand, ldcand, score, lds, B, C, N, E)) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (dtype == POLUS_BF16)
        return rf_by_groups<bf16_t, uint8_t>(what, Q, ldq, codes, ldd, scale, cand, ldcand, score, lds, B, C, N, E, st);
    return rf_by_groups<float, uint8_t>(what, Q, ldq, codes, ldd, scale, cand, ldcand, score, lds, B, C, N, E, st);
}

extern "C" int polus_cls_fp8_quantize(int dtype, const void* x, uint8_t* codes, float* scale, int rows, int E, void* stream) {
    const char* what = "polus_cls_fp8_quantize";
    if (int rc = rf_rows_check(what, dtype, x, codes, scale, rows, E)) return rc;
    POLUS_REQUIRE(polus_aligned16(x) && polus_aligned16(codes), "%s: x and codes must be 16-byte aligned", what);
    hipStream_t st = static_cast<hipStream_t>(stream);
    const dim3 grid((unsigned)(((long)rows + 3) / 4));
    if (dtype == POLUS_BF16)
        hipLaunchKernelGGL(cls_fp8_quantize_kernel<bf16_t>, grid, dim3(256), 0, st, static_cast<const bf16_t*>(x), codes, scale,
                           rows, E);
    else
        hipLaunchKernelGGL(cls_fp8_quantize_kernel<float>, grid, dim3(256), 0, st, static_cast<const float*>(x), codes, scale,
                           rows, E);
    POLUS_CHECK_LAUNCH(what);
    return POLUS_OK;
}

extern "C" int polus_cls_fp8_dequantize(int dtype, const uint8_t* codes, const float* scale, void* y, int rows, int E,
                                        void* stream) {
    const char* what = "polus_cls_fp8_dequantize";
    if (int rc = rf_rows_check(what, dtype, codes, scale, y, rows, E)) return rc;
    POLUS_REQUIRE(polus_aligned16(y) && polus_aligned16(codes), "%s: y and codes must be 16-byte aligned", what);
    hipStream_t st = static_cast<hipStream_t>(stream);
    const dim3 grid((unsigned)(((long)rows + 3) / 4));
    if (dtype == POLUS_BF16)
        hipLaunchKernelGGL(cls_fp8_dequantize_kernel<bf16_t>, grid, dim3(256), 0, st, codes, scale, static_cast<bf16_t*>(y), rows,
                           E);
    else
        hipLaunchKernelGGL(cls_fp8_dequantize_kernel<float>, grid, dim3(256), 0, st, codes, scale, static_cast<float*>(y), rows, E);
    POLUS_CHECK_LAUNCH(what);
    return POLUS_OK;
}
