// IVF-PQ of single ([CLS]) vectors (polus_amd/ir/search.py: IVFPQCodec, CorpusIndex.fit_ivfpq, storage="ivfpq"): a coarse
// centroid id per document plus the product-quantisation codes of its residual (Jegou et al. 2011, IVFADC, for inner
// products).  Format, rules and limits: include/polus_hip.h.
//
// polus_ivfpq_scores_ids is the hot kernel: score[b, c] = cdot[b, coarse[n]] + sum over j of lut[b, j, codes[n, j]] with
// n = cand[b, c], the candidates of query b alone (or n = c without a candidate list).  One workgroup (16 waves, as in
// pq.hip) serves one query and a contiguous range of its candidate columns.  It copies the query's table into LDS as
// [m][256], every sub-space padded with -inf, so a code byte needs no clamp.  Candidate lists differ per query, so no code
// byte is shared between queries and there is one table per workgroup (pq.hip's QT = 1 layout).  A thread owns a candidate
// from the first look-up to the store and adds in ascending j: the bits are a function of the (query, document) pair
// alone.  The candidate id, the coarse code, the first piece of the code row and the centroid's dot product are loaded
// before the look-up loop, in which the next piece travels while the current one is looked up.  The kernel is bound by
// the LDS gathers (64 lanes read sub-space j at columns chosen by the data), as polus_pq_scores is at QT = 1.
// The build-time kernels (residual, coarse update) are plain.
#include "pq_common.h"

namespace {

constexpr int IVFPQ_KMAX = 65535;
constexpr int IVFPQ_EMAX = 5120;                  // PQ_MMAX * PQ_DMAX
constexpr int IVFPQ_CHUNK = 16;                   // features a lane of the coarse update keeps in registers

template <int PIECE, bool CAND>
__global__ __launch_bounds__(PQ_SCAN_THREADS) void ivfpq_scores_ids_kernel(
    const float* __restrict__ lut, const float* __restrict__ cdot, long ldd, const uint16_t* __restrict__ coarse,
    const uint8_t* __restrict__ codes, long ldc, const int32_t* __restrict__ cand, long ldcand, float* __restrict__ score,
    long lds, int C, int N, int m, int ksub, int K, int cpb) {
#pragma clang fp contract(off)
    extern __shared__ float4 ivfpq_lds[];                     // [m][256] floats; float4: a 16-byte aligned base
    float* tab = reinterpret_cast<float*>(ivfpq_lds);
    constexpr int W = PIECE == 16 ? 4 : 1;                    // words per piece
    const int b = blockIdx.y;

    const float* src = lut + (size_t)b * m * ksub;
    for (int r = threadIdx.x; r < m * 256; r += PQ_SCAN_THREADS) {
        const int j = r >> 8, c = r & 255;
        tab[r] = c < ksub ? src[j * ksub + c] : -INFINITY;
    }
    __syncthreads();

    const int c1 = min(C, (int)(blockIdx.x + 1) * cpb);
    for (int c = blockIdx.x * cpb + threadIdx.x; c < c1; c += PQ_SCAN_THREADS) {
        float* out = score + (size_t)b * lds + c;
        const int n = CAND ? cand[(size_t)b * ldcand + c] : c;
        if (n < 0 || n >= N) {                                // nothing is read for an absent candidate
            *out = -INFINITY;
            continue;
        }
        const uint8_t* row = codes + (size_t)n * ldc;
        const int cc = coarse[n];
        uint32_t cur[W], nxt[W];
        pq_piece<PIECE>(row, cur);
        float cd = -INFINITY;
        if (cc < K) cd = cdot[(size_t)b * ldd + cc];          // a code >= K is "no list": cdot is not read
        float acc = 0.f;
        for (int j0 = 0; j0 < m; j0 += 4 * W) {               // m is a multiple of 4 W on this instantiation
#pragma unroll
            for (int w = 0; w < W; ++w) nxt[w] = 0;
            if (j0 + 4 * W < m) pq_piece<PIECE>(row + j0 + 4 * W, nxt);      // uniform
            const float* sub = tab + j0 * 256;
#pragma unroll
            for (int w = 0; w < W; ++w)
#pragma unroll
                for (int k = 0; k < 4; ++k) acc = acc + sub[(4 * w + k) * 256 + ((cur[w] >> (8 * k)) & 255)];
#pragma unroll
            for (int w = 0; w < W; ++w) cur[w] = nxt[w];
        }
        *out = cc < K ? cd + acc : -INFINITY;
    }
}

template <int PIECE, bool CAND>
int ivfpq_scores_launch(const float* lut, const float* cdot, long ldd, const uint16_t* coarse, const uint8_t* codes, long ldc,
                        const int32_t* cand, long ldcand, float* score, long lds, int Q, int C, int N, int m, int ksub, int K,
                        hipStream_t st) {
    const size_t bytes = pq_lds_bytes(1, m);
    const int cpb = pq_docs_per_block(Q, C, bytes);
    dim3 grid((unsigned)((C + cpb - 1) / cpb), (unsigned)Q);
    return polus_launch_lds<ivfpq_scores_ids_kernel<PIECE, CAND>>("polus_ivfpq_scores_ids", grid, dim3(PQ_SCAN_THREADS),
                                                                  PQ_LDS_MAX, bytes, st, lut, cdot, ldd, coarse, codes, ldc, cand,
                                                                  ldcand, score, lds, C, N, m, ksub, K, cpb);
}

template <bool CAND>
int ivfpq_scores_pieces(const float* lut, const float* cdot, long ldd, const uint16_t* coarse, const uint8_t* codes, long ldc,
                        const int32_t* cand, long ldcand, float* score, long lds, int Q, int C, int N, int m, int ksub, int K,
                        hipStream_t st) {
    switch (pq_piece_bytes(codes, ldc, m)) {
        case 16: return ivfpq_scores_launch<16, CAND>(lut, cdot, ldd, coarse, codes, ldc, cand, ldcand, score, lds, Q, C, N, m, ksub, K, st);
        case 4: return ivfpq_scores_launch<4, CAND>(lut, cdot, ldd, coarse, codes, ldc, cand, ldcand, score, lds, Q, C, N, m, ksub, K, st);
    }
    return ivfpq_scores_launch<1, CAND>(lut, cdot, ldd, coarse, codes, ldc, cand, ldcand, score, lds, Q, C, N, m, ksub, K, st);
}

// ---------------------------------------------------------------- build-time kernels
// The pragma keeps every operation its own rounding: NumPy float32 gives the same bits.

template <typename T>
__global__ __launch_bounds__(256) void ivfpq_residual_kernel(const T* __restrict__ x, long ldx, const T* __restrict__ cent,
                                                             const uint16_t* __restrict__ coarse, float* __restrict__ r, long ldr,
                                                             int rows, int K, int E) {
#pragma clang fp contract(off)
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long)rows * E) return;
    const long t = i / E;
    const int e = (int)(i - t * E), c = coarse[t];
    r[(size_t)t * ldr + e] = c < K ? to_f<T>(x[(size_t)t * ldx + e]) - to_f<T>(cent[(size_t)c * E + e]) : 0.f;
}

// One workgroup of 4 waves per centroid; lane l of every wave holds partial l of the header's rule for IVFPQ_CHUNK
// features at a time and scans its rows [l P, (l + 1) P) once per chunk; the chunks are dealt to the waves round robin.
template <typename T>
__global__ __launch_bounds__(256) void ivfpq_coarse_update_kernel(const T* __restrict__ x, long ldx,
                                                                  const uint16_t* __restrict__ coarse, const T* __restrict__ prev,
                                                                  T* __restrict__ out, int32_t* __restrict__ counts, int Tn, int E) {
#pragma clang fp contract(off)
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, k = blockIdx.x;
    const int per = (Tn + 63) / 64;
    const long lo = (long)lane * per;
    const long t0 = lo < Tn ? lo : Tn, t1 = t0 + per < Tn ? t0 + per : Tn;
    for (int e0 = wave * IVFPQ_CHUNK; e0 < E; e0 += 4 * IVFPQ_CHUNK) {       // wave-uniform
        float p[IVFPQ_CHUNK];
#pragma unroll
        for (int i = 0; i < IVFPQ_CHUNK; ++i) p[i] = 0.f;
        int found = 0;
        for (long t = t0; t < t1; ++t) {
            if ((int)coarse[t] != k) continue;
            ++found;
            const T* xr = x + (size_t)t * ldx + e0;
#pragma unroll
            for (int i = 0; i < IVFPQ_CHUNK; ++i)
                if (e0 + i < E) p[i] = p[i] + to_f<T>(xr[i]);
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            found += __shfl_xor(found, o, 64);
#pragma unroll
            for (int i = 0; i < IVFPQ_CHUNK; ++i) p[i] = p[i] + __shfl_xor(p[i], o, 64);
        }
        if (e0 == 0 && lane == 0) counts[k] = found;
        const float cnt = (float)found;
#pragma unroll
        for (int i = 0; i < IVFPQ_CHUNK; ++i)
            if (lane == i && e0 + i < E)
                out[(size_t)k * E + e0 + i] = found > 0 ? from_f<T>(p[i] / cnt) : prev[(size_t)k * E + e0 + i];
    }
}

int ivfpq_check_scan(const char* what, int Q, int C, int m, int ksub) {
    if (int rc = pq_check_format(what, m, ksub, 1)) return rc;
    POLUS_REQUIRE(Q >= 1 && Q <= PQ_ROWS_MAX, "%s: need 1 <= Q <= %d (got %d)", what, PQ_ROWS_MAX, Q);
    POLUS_REQUIRE(C >= 1 && C <= PQ_ROWS_MAX, "%s: need 1 <= C <= %d (got %d)", what, PQ_ROWS_MAX, C);
    return POLUS_OK;
}

#define IVFPQ_CHECK_K(what, K) \
    POLUS_REQUIRE(K >= 1 && K <= IVFPQ_KMAX, "%s: need 1 <= K <= %d (got %d)", what, IVFPQ_KMAX, K)

}  // namespace

extern "C" int polus_ivfpq_scores_ids_route(int Q, int C, int m, int ksub, int* out) {
    const char* what = "polus_ivfpq_scores_ids_route";
    if (int rc = ivfpq_check_scan(what, Q, C, m, ksub)) return rc;
    POLUS_REQUIRE(out, "%s: null pointer", what);
    out[0] = (int)pq_lds_bytes(1, m);
    out[1] = pq_docs_per_block(Q, C, pq_lds_bytes(1, m));
    return POLUS_OK;
}

extern "C" int polus_ivfpq_scores_ids(const float* lut, const float* cdot, long ldd, const uint16_t* coarse,
                                      const uint8_t* codes, long ldc, const int32_t* cand, long ldcand, float* score, long lds,
                                      int Q, int C, int N, int m, int ksub, int K, void* stream) {
    const char* what = "polus_ivfpq_scores_ids";
    if (int rc = ivfpq_check_scan(what, Q, C, m, ksub)) return rc;
    IVFPQ_CHECK_K(what, K);
    POLUS_REQUIRE(N >= 1, "%s: need N >= 1 (got %d)", what, N);
    POLUS_REQUIRE(cand || C == N, "%s: without cand column c is document c, so C must be N (got C = %d, N = %d)", what, C, N);
    POLUS_REQUIRE(ldd >= K, "%s: cdot row stride ldd must be >= K (got %ld < %d)", what, ldd, K);
    POLUS_REQUIRE(ldc >= m, "%s: code row stride ldc must be >= m (got %ld < %d)", what, ldc, m);
    POLUS_REQUIRE(!cand || ldcand >= C, "%s: candidate row stride ldcand must be >= C (got %ld < %d)", what, ldcand, C);
    POLUS_REQUIRE(lds >= C, "%s: score row stride lds must be >= C (got %ld < %d)", what, lds, C);
    POLUS_REQUIRE(lut && cdot && coarse && codes && score, "%s: null pointer", what);
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (cand) return ivfpq_scores_pieces<true>(lut, cdot, ldd, coarse, codes, ldc, cand, ldcand, score, lds, Q, C, N, m, ksub, K, st);
    return ivfpq_scores_pieces<false>(lut, cdot, ldd, coarse, codes, ldc, cand, ldcand, score, lds, Q, C, N, m, ksub, K, st);
}

extern "C" int polus_ivfpq_residual(int dtype, const void* x, long ldx, const void* cent, const uint16_t* coarse, float* r,
                                    long ldr, int rows, int K, int E, void* stream) {
    const char* what = "polus_ivfpq_residual";
    PQ_CHECK_DTYPE(what, dtype);
    IVFPQ_CHECK_K(what, K);
    POLUS_REQUIRE(rows >= 1, "%s: need rows >= 1 (got %d)", what, rows);
    POLUS_REQUIRE(E >= 1 && E <= IVFPQ_EMAX, "%s: need 1 <= E <= %d (got %d)", what, IVFPQ_EMAX, E);
    POLUS_REQUIRE(ldx >= E, "%s: row stride ldx must be >= E (got %ld < %d)", what, ldx, E);
    POLUS_REQUIRE(ldr >= E, "%s: row stride ldr must be >= E (got %ld < %d)", what, ldr, E);
    POLUS_REQUIRE(x && cent && coarse && r, "%s: null pointer", what);
    hipStream_t st = static_cast<hipStream_t>(stream);
    const long total = (long)rows * E;
    POLUS_REQUIRE((total + 255) / 256 <= 0x7FFFFFFFL, "%s: rows * E = %ld elements are more than one launch takes", what, total);
    dim3 grid((unsigned)((total + 255) / 256));
    if (dtype == POLUS_BF16)
        hipLaunchKernelGGL(ivfpq_residual_kernel<bf16_t>, grid, dim3(256), 0, st, static_cast<const bf16_t*>(x), ldx,
                           static_cast<const bf16_t*>(cent), coarse, r, ldr, rows, K, E);
    else
        hipLaunchKernelGGL(ivfpq_residual_kernel<float>, grid, dim3(256), 0, st, static_cast<const float*>(x), ldx,
                           static_cast<const float*>(cent), coarse, r, ldr, rows, K, E);
    POLUS_CHECK_LAUNCH(what);
    return POLUS_OK;
}

extern "C" int polus_ivfpq_coarse_update(int dtype, const void* x, long ldx, const uint16_t* coarse, const void* prev, void* out,
                                         int32_t* counts, int T, int K, int E, void* stream) {
    const char* what = "polus_ivfpq_coarse_update";
    PQ_CHECK_DTYPE(what, dtype);
    IVFPQ_CHECK_K(what, K);
    POLUS_REQUIRE(T >= 1, "%s: need T >= 1 (got %d)", what, T);
    POLUS_REQUIRE(E >= 1 && E <= IVFPQ_EMAX, "%s: need 1 <= E <= %d (got %d)", what, IVFPQ_EMAX, E);
    POLUS_REQUIRE(ldx >= E, "%s: row stride ldx must be >= E (got %ld < %d)", what, ldx, E);
    POLUS_REQUIRE(x && coarse && prev && out && counts, "%s: null pointer", what);
    const size_t bytes = (size_t)K * E * polus_dtype_size(dtype);
    const char *po = static_cast<const char*>(out), *pp = static_cast<const char*>(prev);
    POLUS_REQUIRE(po + bytes <= pp || pp + bytes <= po, "%s: out must not overlap prev", what);
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (dtype == POLUS_BF16)
        hipLaunchKernelGGL(ivfpq_coarse_update_kernel<bf16_t>, dim3((unsigned)K), dim3(256), 0, st, static_cast<const bf16_t*>(x),
                           ldx, coarse, static_cast<const bf16_t*>(prev), static_cast<bf16_t*>(out), counts, T, E);
    else
        hipLaunchKernelGGL(ivfpq_coarse_update_kernel<float>, dim3((unsigned)K), dim3(256), 0, st, static_cast<const float*>(x),
                           ldx, coarse, static_cast<const float*>(prev), static_cast<float*>(out), counts, T, E);
    POLUS_CHECK_LAUNCH(what);
    return POLUS_OK;
}
