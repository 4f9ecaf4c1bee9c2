// FP8 token index: per-row quantisation to OCP e4m3fn with a power-of-two scale, and the MaxSim corpus scores and
// re-ranking (maxsim.hip, rerank.hip) over documents stored that way.
//
//   x[row, k]  ~  e4m3fn(codes[row, k]) * scale[row],     scale[row] = 2^e
//
// Every e4m3 value has at most 4 significant bits, so T(code) is exact in bf16 and in f32, and a power-of-two scale
// only moves exponents: T(code) * scale is exact too.  The scoring kernels convert the code bytes to the query's
// type in registers, feed the fragments and MFMAs of their bf16 / f32 counterparts in the same k order, and multiply
// every accumulator row (a document token) by its token's scale before the mask and the max.  An accumulator of
// scaled rows IS the scaled accumulator, bit for bit, because every product and partial sum moves by the same power
// of two (absent under- and overflow).  The reductions that follow are the counterparts' own, so
//   polus_maxsim_scores_fp8(Q, codes, scale) == polus_maxsim_scores(Q, dequantised D)      in bits
//   polus_maxsim_rerank_fp8(...)             == polus_maxsim_scores_fp8 of each pair        in bits
// and the quantiser below holds all of the error.
#include "maxsim_common.h"
#include "fp8_common.h"

namespace {

// 8 e4m3fn bytes (k ascending from the low byte of raw.x) -> one MFMA fragment of T; exact
__device__ __forceinline__ void f8_to_f32(float (&v)[8], uint2 raw) {
    const f32x2 a = __builtin_amdgcn_cvt_pk_f32_fp8((int)raw.x, false);
    const f32x2 b = __builtin_amdgcn_cvt_pk_f32_fp8((int)raw.x, true);
    const f32x2 c = __builtin_amdgcn_cvt_pk_f32_fp8((int)raw.y, false);
    const f32x2 d = __builtin_amdgcn_cvt_pk_f32_fp8((int)raw.y, true);
    v[0] = a[0]; v[1] = a[1]; v[2] = b[0]; v[3] = b[1];
    v[4] = c[0]; v[5] = c[1]; v[6] = d[0]; v[7] = d[1];
}
__device__ __forceinline__ void f8_frag(Frag<float>& f, uint2 raw) { f8_to_f32(f.v, raw); }
__device__ __forceinline__ void f8_frag(Frag<bf16_t>& f, uint2 raw) {
    float v[8];
    f8_to_f32(v, raw);
#pragma unroll
    for (int j = 0; j < 8; ++j) f.v[j] = (bf16_t)v[j];
}

// ---------------------------------------------------------------- quantise / dequantise, one wave per row
// lane l holds elements 4 l .. 4 l + 3 (E <= 256, a multiple of 4)
template <typename T>
__global__ __launch_bounds__(256) void fp8_quantize_kernel(const T* __restrict__ x, unsigned char* __restrict__ codes,
                                                           float* __restrict__ scale, int rows, int E) {
    const int lane = threadIdx.x & 63;
    const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    const int e0 = 4 * lane;
    const bool on = e0 < E;
    float v[4] = {0.f, 0.f, 0.f, 0.f};
    if (on) load4<T>(x + (size_t)row * E + e0, v);
    const float amax = wave_max(fmaxf(fmaxf(fabsf(v[0]), fabsf(v[1])), fmaxf(fabsf(v[2]), fabsf(v[3]))));
    const int e = f8_row_exponent(amax);
    const int w = f8_pack4(v, f8_pow2(-e));
    if (on) *reinterpret_cast<int*>(codes + (size_t)row * E + e0) = w;
    if (lane == 0) scale[row] = f8_pow2(e);
}

template <typename T>
__global__ __launch_bounds__(256) void fp8_dequantize_kernel(const unsigned char* __restrict__ codes,
                                                             const float* __restrict__ scale, T* __restrict__ y,
                                                             int rows, int E) {
    const int lane = threadIdx.x & 63;
    const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    const int e0 = 4 * lane;
    if (e0 >= E) return;
    const int w = *reinterpret_cast<const int*>(codes + (size_t)row * E + e0);
    float v[4];
    f8_unpack4(w, scale[row], v);
    store4<T>(y + (size_t)row * E + e0, v);
}

// ---------------------------------------------------------------- corpus scores
// maxsim_fwd_body (maxsim.hip) without the argmax, over code rows of E bytes: the same grid, query tiles, LDS stages
// (two buffers of 32 rows, rows padded by 16 B: the 8-byte fragment reads of 16 rows fall into distinct banks in each
// half of the wave) and reduction.  The document's scales sit in LDS beside its mask.  "No valid j" is told by the
// maximum staying -inf, which is when maxsim_fwd_body's winning j stays unset.
template <typename T, int KS>
__global__ __launch_bounds__(256) void maxsim_scores_fp8_kernel(const T* __restrict__ Q,
                                                                const unsigned char* __restrict__ codes,
                                                                const float* __restrict__ scale,
                                                                const int32_t* __restrict__ qmask,
                                                                const int32_t* __restrict__ dmask,
                                                                float* __restrict__ score, long lds, int B, int N,
                                                                int Lq, int Ld, int qpb) {
    using S = MsStageB<32 * KS>;
    constexpr int UT = MsTiles<T, KS>::UT;
    constexpr int E = 32 * KS;
    __shared__ float tsum[16 * 32];                           // per query tile: sum of its 16 maxima
    __shared__ __attribute__((aligned(16))) int smask[MS_LMAX];               // document mask, 0 past Ld
    __shared__ __attribute__((aligned(16))) float sscale[MS_LMAX];            // token scales, 0 past Ld
    __shared__ __attribute__((aligned(16))) unsigned char sd[2 * S::SR * S::RS];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int i = lane & 15, g = lane >> 4;
    const int c = blockIdx.x;
    const int b0 = blockIdx.y * qpb;
    const int nq = min(qpb, B - b0);
    const int nut = (Lq + 15) >> 4;                           // query tiles per query
    const int ntiles = nq * nut;
    const int nst = (Ld + S::SR - 1) / S::SR;                 // stages per document
    const unsigned char* Dc = codes + (size_t)c * Ld * E;
    const int32_t* dm = dmask ? dmask + (size_t)c * Ld : nullptr;
    const float* sc = scale + (size_t)c * Ld;
    for (int j = threadIdx.x; j < nst * S::SR; j += 256) {
        smask[j] = j < Ld && (!dm || dm[j] != 0);
        sscale[j] = j < Ld ? sc[j] : 0.f;
    }

    u32x4 stg[S::NCH];

    for (int r0w = 0; r0w < ntiles; r0w += 4 * UT) {
        const int u0 = r0w + wave * UT;
        const bool active = u0 < ntiles;                      // wave-uniform
        Frag<T> qf[UT][KS];
#pragma unroll
        for (int u = 0; u < UT; ++u) {
            const int uu = min(u0 + u, ntiles - 1);
            const int bq = b0 + uu / nut;
            const int tok = min(((uu % nut) << 4) + i, Lq - 1);
            const unsigned char* p = reinterpret_cast<const unsigned char*>(Q + ((size_t)bq * Lq + tok) * E + 8 * g);
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) frag_load_row(qf[u][ks], p + ks * 32 * sizeof(T));
        }
        float m[UT];
#pragma unroll
        for (int u = 0; u < UT; ++u) m[u] = -INFINITY;

        ms_gload<S>(stg, Dc, 0, Ld);
        ms_sstore<S>(stg, sd);
        __syncthreads();
        for (int st = 0; st < nst; ++st) {
            if (st + 1 < nst) ms_gload<S>(stg, Dc, st + 1, Ld);   // in flight while this stage is multiplied
            if (active) {
                const unsigned char* buf = sd + (st & 1) * S::SR * S::RS;
#pragma unroll
                for (int tt = 0; tt < S::SR / 16; ++tt) {
                    const int t16 = st * S::SR + tt * 16;
                    if (t16 >= Ld) break;                     // uniform
                    const int r0 = t16 + 4 * g;               // this lane's doc rows r0 .. r0+3
                    const int4 mk = *reinterpret_cast<const int4*>(&smask[r0]);
                    const float4 sk = *reinterpret_cast<const float4*>(&sscale[r0]);
                    const unsigned char* p = buf + (tt * 16 + i) * S::RS + 8 * g;
                    f32x4 acc[UT];
#pragma unroll
                    for (int u = 0; u < UT; ++u) acc[u] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
                    for (int ks = 0; ks < KS; ++ks) {
                        Frag<T> df;
                        f8_frag(df, *reinterpret_cast<const uint2*>(p + ks * 32));
#pragma unroll
                        for (int u = 0; u < UT; ++u) mma16(acc[u], df, qf[u][ks]);
                    }
                    const bool ok[4] = {mk.x != 0, mk.y != 0, mk.z != 0, mk.w != 0};
                    const float sr[4] = {sk.x, sk.y, sk.z, sk.w};
#pragma unroll
                    for (int u = 0; u < UT; ++u)
#pragma unroll
                        for (int r = 0; r < 4; ++r) {
                            const float a = acc[u][r] * sr[r];
                            if (ok[r] && a > m[u]) m[u] = a;
                        }
                }
            }
            // into the buffer every wave finished reading before the last barrier
            if (st + 1 < nst) ms_sstore<S>(stg, sd + ((st + 1) & 1) * S::SR * S::RS);
            __syncthreads();
        }
        if (!active) continue;

#pragma unroll
        for (int u = 0; u < UT; ++u) {
            float mu = m[u];
#pragma unroll
            for (int o = 16; o <= 32; o <<= 1) {
                const float m2 = __shfl_xor(mu, o, 64);
                if (m2 > mu) mu = m2;
            }
            const int uu = u0 + u;
            float contrib = 0.f;
            if (uu < ntiles) {
                const int bq = b0 + uu / nut;
                const int tok = ((uu % nut) << 4) + i;
                const bool qv = tok < Lq && (!qmask || qmask[(size_t)bq * Lq + tok] != 0);
                contrib = (qv && mu > -INFINITY) ? mu : 0.f;
            }
            // sum of the tile's 16 maxima (lanes 0..15; every group holds the same values)
#pragma unroll
            for (int o = 1; o < 16; o <<= 1) contrib += __shfl_xor(contrib, o, 64);
            if (lane == 0 && uu < ntiles) tsum[uu] = contrib;
        }
    }
    __syncthreads();
    if ((int)threadIdx.x < nq) {
        float s = 0.f;
        for (int t = 0; t < nut; ++t) s += tsum[threadIdx.x * nut + t];
        score[(size_t)(b0 + threadIdx.x) * lds + c] = s;
    }
}

// ---------------------------------------------------------------- re-ranking
// maxsim_rerank_kernel (rerank.hip) over code rows: a lane's 8 elements of a k-step are 8 bytes, converted where the
// tile is multiplied.  A tile carries one scale per lane, that of token 16 t + 4 g + (i & 3); the four scales of a
// lane's accumulator rows 4 g .. 4 g + 3 are then the four lanes of its quad (a DPP quad broadcast, no memory).
template <int KS> struct F8Tile {
    uint2 v[KS];
    float s;
};

template <int KS>
__device__ __forceinline__ void f8_tile_load(F8Tile<KS>& f, const unsigned char* base, const float* sc, int t, int i,
                                             int g, int Ld) {
    const unsigned char* p = base + (size_t)min(16 * t + i, Ld - 1) * (32 * KS);
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) f.v[ks] = *reinterpret_cast<const uint2*>(p + ks * 32);
    f.s = sc[min(16 * t + 4 * g + (i & 3), Ld - 1)];
}

template <int R> __device__ __forceinline__ float quad_bcast(float v) {
    return __builtin_bit_cast(float, __builtin_amdgcn_mov_dpp(__builtin_bit_cast(int, v),
                                                              R | (R << 2) | (R << 4) | (R << 6), 0xF, 0xF, true));
}

template <typename T, int KS, int UT>
__device__ __forceinline__ void f8_tile_max(float (&m)[UT], const F8Tile<KS>& tile, const Frag<T> (&qf)[UT][KS],
                                            unsigned bits, int nu) {
    Frag<T> df[KS];
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) f8_frag(df[ks], tile.v[ks]);
    const float sr[4] = {quad_bcast<0>(tile.s), quad_bcast<1>(tile.s), quad_bcast<2>(tile.s), quad_bcast<3>(tile.s)};
#pragma unroll
    for (int u = 0; u < UT; ++u) {
        if (u < nu) {                                         // uniform
            f32x4 acc = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) mma16(acc, df[ks], qf[u][ks]);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float a = acc[r] * sr[r];
                if (((bits >> r) & 1u) && a > m[u]) m[u] = a;
            }
        }
    }
}

template <typename T, int KS, bool RES>
__global__ __launch_bounds__(256) void maxsim_rerank_fp8_kernel(const T* __restrict__ Q,
                                                                const unsigned char* __restrict__ codes,
                                                                const float* __restrict__ scale,
                                                                const int32_t* __restrict__ qmask,
                                                                const int32_t* __restrict__ dmask,
                                                                const int32_t* __restrict__ cand, long ldc,
                                                                float* __restrict__ score, long lds, int C, int N,
                                                                int Lq, int Ld, int dpw) {
    constexpr int UT = MsTiles<T, KS>::UT;
    constexpr int E = 32 * KS;
    constexpr size_t ROWB = E;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int i = lane & 15, g = lane >> 4;
    const int b = blockIdx.y;
    const int c0 = blockIdx.x * 4 * dpw + wave;               // this wave's candidates: c0, c0 + 4, ...
    if (c0 >= C) return;                                      // wave-uniform; the kernel has no barrier
    const int nd = min(dpw, (C - c0 + 3) >> 2);
    const int myc = c0 + 4 * lane;
    const int idv = cand[(size_t)b * ldc + min(myc, C - 1)];
    const int ids = lane < nd ? idv : -1;                     // lane l: the wave's l-th candidate id

    const int nut = (Lq + 15) >> 4;                           // query tiles
    const T* Qb = Q + (size_t)b * Lq * E;
    const int32_t* qm = qmask ? qmask + (size_t)b * Lq : nullptr;
    const unsigned char* Dg = codes + 8 * g;

    const int idc = __builtin_amdgcn_readlane(ids, 0);
    bool pres = (unsigned)idc < (unsigned)N;                  // absent: nothing of the document is dereferenced
    const unsigned char* Dc = Dg + (size_t)(pres ? idc : 0) * Ld * ROWB;     // (document 0 stands in for the loads)
    const float* Sc = scale + (size_t)(pres ? idc : 0) * Ld;
    unsigned tm;
    int nvt;
    {
        int mv[8];
        rr_mask_load(mv, dmask ? dmask + (size_t)(pres ? idc : 0) * Ld : nullptr, lane, Ld);
        rr_mask_pack(mv, pres, lane, Ld, tm, nvt);
    }
    // two tile buffers in turn, as maxsim_rerank_kernel: at the top of the document loop ta = (document l, tile 0)
    F8Tile<KS> ta, tb;
    f8_tile_load<KS>(ta, Dc, Sc, 0, i, g, Ld);
    Frag<T> qf[UT][KS];
    bool qok[UT];
    if constexpr (RES) rr_query_load        // nut <= UT: the whole query stays in registers
       <T, KS, UT>(qf, qok, Qb, qm, 0, nut, Lq, i, g);

    for (int l = 0; l < nd; ++l) {
        const int idn = __builtin_amdgcn_readlane(ids, min(l + 1, nd - 1));
        const bool presn = (unsigned)idn < (unsigned)N;
        const unsigned char* Dn = Dg + (size_t)(presn ? idn : 0) * Ld * ROWB;
        const float* Sn = scale + (size_t)(presn ? idn : 0) * Ld;
        int mvn[8];
        rr_mask_load(mvn, dmask ? dmask + (size_t)(presn ? idn : 0) * Ld : nullptr, lane, Ld);

        float s = 0.f;
        if (nvt > 0) {
            for (int r0 = 0; r0 < nut; r0 += UT) {
                if constexpr (!RES) rr_query_load<T, KS, UT>(qf, qok, Qb, qm, r0, nut, Lq, i, g);
                const int nu = min(UT, nut - r0);
                const bool last_round = r0 + UT >= nut;
                float m[UT];
#pragma unroll
                for (int u = 0; u < UT; ++u) m[u] = -INFINITY;
                for (int t = 0; t < nvt; t += 2) {
                    const int t1 = min(t + 1, nvt - 1);
                    const bool last = t + 2 >= nvt;
                    f8_tile_load<KS>(tb, Dc, Sc, t1, i, g, Ld);
                    f8_tile_max<T, KS, UT>(m, ta, qf, __builtin_amdgcn_readlane(tm, t) >> (4 * g), nu);
                    const bool nxt = last && last_round;
                    f8_tile_load<KS>(ta, nxt ? Dn : Dc, nxt ? Sn : Sc, last ? 0 : t + 2, i, g, Ld);
                    f8_tile_max<T, KS, UT>(m, tb, qf, __builtin_amdgcn_readlane(tm, t1) >> (4 * g), nu);
                }
#pragma unroll
                for (int u = 0; u < UT; ++u) {
                    if (u < nu) {                             // uniform
                        float mu = m[u];
#pragma unroll
                        for (int o = 16; o <= 32; o <<= 1) {
                            const float m2 = __shfl_xor(mu, o, 64);
                            if (m2 > mu) mu = m2;
                        }
                        float contrib = (qok[u] && mu > -INFINITY) ? mu : 0.f;
#pragma unroll
                        for (int o = 1; o < 16; o <<= 1) contrib += __shfl_xor(contrib, o, 64);
                        s += contrib;
                    }
                }
            }
        } else {
            f8_tile_load<KS>(ta, Dn, Sn, 0, i, g, Ld);        // absent or empty document: nothing was streamed
        }
        if (lane == 0) score[(size_t)b * lds + c0 + 4 * l] = pres ? s : -INFINITY;
        rr_mask_pack(mvn, presn, lane, Ld, tm, nvt);
        pres = presn;
        Dc = Dn;
        Sc = Sn;
    }
}

// ---------------------------------------------------------------- host
int f8_rows_check(const char* what, int dtype, const void* a, const void* b, const void* c, int rows, int E) {
    POLUS_REQUIRE(dtype == POLUS_F32 || dtype == POLUS_BF16, "%s: unknown dtype %d", what, dtype);
    POLUS_REQUIRE(rows >= 1, "%s: need rows >= 1 (got %d)", what, rows);
    POLUS_REQUIRE(E >= 4 && E <= MS_EMAX && E % 4 == 0, "%s: E must be a multiple of 4 in [4, %d] (got %d)", what,
                  MS_EMAX, E);
    POLUS_REQUIRE(a && b && c, "%s: null pointer", what);
    return POLUS_OK;
}

int f8_check(const char* what, int dtype, int B, int Lq, int Ld, int E, const void* Q, const void* codes,
             const void* scale, const void* score) {
    int rc = ms_shape_check(what, dtype, B, Lq, Ld, E);
    if (rc != POLUS_OK) return rc;
    POLUS_REQUIRE(Q && codes && scale && score, "%s: null pointer", what);
    POLUS_REQUIRE(polus_aligned16(Q) && polus_aligned16(codes), "%s: Q and codes must be 16-byte aligned", what);
    return POLUS_OK;
}

}  // namespace

extern "C" int polus_fp8_quantize_rows(int dtype, const void* x, uint8_t* codes, float* scale, int rows, int E,
                                       void* stream) {
    const char* what = "polus_fp8_quantize_rows";
    int rc = f8_rows_check(what, dtype, x, codes, scale, rows, E);
    if (rc != POLUS_OK) return rc;
    POLUS_REQUIRE(polus_aligned16(x) && polus_aligned16(codes), "%s: x and codes must be 16-byte aligned", what);
    hipStream_t st = static_cast<hipStream_t>(stream);
    const dim3 grid((unsigned)(((long)rows + 3) / 4));
    if (dtype == POLUS_BF16)
        hipLaunchKernelGGL(fp8_quantize_kernel<bf16_t>, grid, dim3(256), 0, st, static_cast<const bf16_t*>(x), codes,
                           scale, rows, E);
    else
        hipLaunchKernelGGL(fp8_quantize_kernel<float>, grid, dim3(256), 0, st, static_cast<const float*>(x), codes,
                           scale, rows, E);
    POLUS_CHECK_LAUNCH(what);
    return POLUS_OK;
}

extern "C" int polus_fp8_dequantize_rows(int dtype, const uint8_t* codes, const float* scale, void* y, int rows, int E,
                                         void* stream) {
    const char* what = "polus_fp8_dequantize_rows";
    int rc = f8_rows_check(what, dtype, codes, scale, y, rows, E);
    if (rc != POLUS_OK) return rc;
    POLUS_REQUIRE(polus_aligned16(y) && polus_aligned16(codes), "%s: y and codes must be 16-byte aligned", what);
    hipStream_t st = static_cast<hipStream_t>(stream);
    const dim3 grid((unsigned)(((long)rows + 3) / 4));
    if (dtype == POLUS_BF16)
        hipLaunchKernelGGL(fp8_dequantize_kernel<bf16_t>, grid, dim3(256), 0, st, codes, scale,
                           static_cast<bf16_t*>(y), rows, E);
    else
        hipLaunchKernelGGL(fp8_dequantize_kernel<float>, grid, dim3(256), 0, st, codes, scale, static_cast<float*>(y),
                           rows, E);
    POLUS_CHECK_LAUNCH(what);
    return POLUS_OK;
}

extern "C" int polus_maxsim_scores_fp8(int dtype, const void* Q, const uint8_t* codes, const float* scale,
                                       const int32_t* qmask, const int32_t* dmask, float* score, long lds, int B, int N,
                                       int Lq, int Ld, int E, void* stream) {
    const char* what = "polus_maxsim_scores_fp8";
    int rc = f8_check(what, dtype, B, Lq, Ld, E, Q, codes, scale, score);
    if (rc != POLUS_OK) return rc;
    POLUS_REQUIRE(N >= 1 && N <= 65535, "%s: need 1 <= N <= 65535 (got %d)", what, N);
    POLUS_REQUIRE(lds >= N, "%s: score row stride lds must be >= N (got %ld < %d)", what, lds, N);
    ms_dispatch(dtype, E, [&](auto t, auto ks) {
        using T = typename decltype(t)::type;
        constexpr int KS = decltype(ks)::value;
        const int qpb = ms_queries_per_block<T, KS>(B, N, Lq);
        hipLaunchKernelGGL((maxsim_scores_fp8_kernel<T, KS>), dim3(N, (B + qpb - 1) / qpb), dim3(256), 0,
                           static_cast<hipStream_t>(stream), static_cast<const T*>(Q), codes, scale, qmask, dmask,
                           score, lds, B, N, Lq, Ld, qpb);
    });
    POLUS_CHECK_LAUNCH(what);
    return POLUS_OK;
}

extern "C" int polus_maxsim_rerank_fp8(int dtype, const void* Q, const uint8_t* codes, const float* scale,
                                       const int32_t* qmask, const int32_t* dmask, const int32_t* cand, long ldc,
                                       float* score, long lds, int B, int C, int N, int Lq, int Ld, int E,
                                       void* stream) {
    const char* what = "polus_maxsim_rerank_fp8";
    int rc = f8_check(what, dtype, B, Lq, Ld, E, Q, codes, scale, score);
    if (rc == POLUS_OK) rc = rr_args_check(what, C, N, ldc, lds);
    if (rc != POLUS_OK) return rc;
    POLUS_REQUIRE(cand, "%s: null pointer", what);
    ms_dispatch(dtype, E, [&](auto t, auto ks) {
        using T = typename decltype(t)::type;
        constexpr int KS = decltype(ks)::value;
        rr_launch<T, KS>(maxsim_rerank_fp8_kernel<T, KS, true>, maxsim_rerank_fp8_kernel<T, KS, false>, B, C, Lq,
                         static_cast<hipStream_t>(stream), static_cast<const T*>(Q), codes, scale, qmask, dmask, cand,
                         ldc, score, lds, C, N, Lq, Ld);
    });
    POLUS_CHECK_LAUNCH(what);
    return POLUS_OK;
}
