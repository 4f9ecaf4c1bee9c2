// Product quantisation of single ([CLS]) vectors (polus_amd/ir/search.py: PQCodec, CorpusIndex.fit_pq, storage="pq") and
// its asymmetric-distance (ADC) scan.  Format, rules and limits: include/polus_hip.h.
//
// polus_pq_scores is the hot kernel: score[b, n] = sum over j of lut[b, j, codes[n, j]].  One workgroup (16 waves: 4 per
// SIMD, what 4- and 8-byte LDS reads need for their rate) serves QT consecutive queries and a contiguous range of
// documents.  It first copies the QT tables into LDS interleaved as [m][256][QT], every sub-space padded to 256 entries
// with -inf, so that a code byte needs no clamp and one ds_read_b32 / b64 / b128 fetches the entry of all QT queries: the
// address arithmetic and the code bytes are paid once per QT queries.  A thread owns a document from the first look-up
// to the store and adds in ascending j, which makes the bits a function of the (query, document) pair alone.  All 64
// lanes of a step read sub-space j at columns chosen by the data: the kernel is bound by those LDS gathers, not by HBM.
// The code bytes travel in 16-byte pieces, the next piece loaded while the current one is looked up.
// The build-time kernels (encode, update, decode, lut) are plain: one thread per output, or one wave per codeword.
#include "pq_common.h"

namespace {

// Queries per workgroup: from Q, m and the LDS budget alone.
static inline int pq_qt(int Q, int m) {
    for (int qt = 4; qt > 1; qt >>= 1)
        if (qt <= Q && pq_lds_bytes(qt, m) <= PQ_LDS_MAX) return qt;
    return 1;
}

template <int QT> struct PqEntry;
template <> struct PqEntry<1> { typedef float type; };
template <> struct PqEntry<2> { typedef float2 type; };
template <> struct PqEntry<4> { typedef float4 type; };

template <int QT, int PIECE>
__global__ __launch_bounds__(PQ_SCAN_THREADS) void pq_scores_kernel(const float* __restrict__ lut,
                                                                    const uint8_t* __restrict__ codes, long ldc,
                                                                    float* __restrict__ score, long lds, int Q, int N,
                                                                    int m, int ksub, int dpb) {
    extern __shared__ float4 pq_lds[];                        // [m][256][QT] floats; float4: a 16-byte aligned base
    float* tab = reinterpret_cast<float*>(pq_lds);
    typedef typename PqEntry<QT>::type entry_t;
    constexpr int W = PIECE == 16 ? 4 : 1;                    // words per piece
    const int b0 = blockIdx.y * QT;

#pragma unroll
    for (int q = 0; q < QT; ++q) {                            // a spare slot of the last group repeats query Q - 1
        const float* src = lut + (size_t)min(b0 + q, Q - 1) * m * ksub;
        for (int r = threadIdx.x; r < m * 256; r += PQ_SCAN_THREADS) {
            const int j = r >> 8, c = r & 255;
            tab[r * QT + q] = c < ksub ? src[j * ksub + c] : -INFINITY;
        }
    }
    __syncthreads();

    const int n1 = min(N, (int)(blockIdx.x + 1) * dpb);
    for (int n = blockIdx.x * dpb + threadIdx.x; n < n1; n += PQ_SCAN_THREADS) {
        const uint8_t* row = codes + (size_t)n * ldc;
        float acc[QT];
#pragma unroll
        for (int q = 0; q < QT; ++q) acc[q] = 0.f;
        uint32_t cur[W], nxt[W];
        pq_piece<PIECE>(row, cur);
        for (int j0 = 0; j0 < m; j0 += 4 * W) {               // m is a multiple of 4 W on this instantiation
#pragma unroll
            for (int w = 0; w < W; ++w) nxt[w] = 0;
            if (j0 + 4 * W < m) pq_piece<PIECE>(row + j0 + 4 * W, nxt);      // uniform
            const entry_t* sub = reinterpret_cast<const entry_t*>(tab) + j0 * 256;
#pragma unroll
            for (int w = 0; w < W; ++w)
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const int code = (cur[w] >> (8 * k)) & 255;
                    const entry_t e = sub[(4 * w + k) * 256 + code];
                    const float* v = reinterpret_cast<const float*>(&e);
#pragma unroll
                    for (int q = 0; q < QT; ++q) acc[q] += v[q];
                }
#pragma unroll
            for (int w = 0; w < W; ++w) cur[w] = nxt[w];
        }
#pragma unroll
        for (int q = 0; q < QT; ++q)
            if (b0 + q < Q) score[(size_t)(b0 + q) * lds + n] = acc[q];
    }
}

template <int QT, int PIECE>
int pq_scores_launch(const float* lut, const uint8_t* codes, long ldc, float* score, long lds, int Q, int N, int m, int ksub,
                     hipStream_t st) {
    const int groups = (Q + QT - 1) / QT;
    const size_t bytes = pq_lds_bytes(QT, m);
    const int dpb = pq_docs_per_block(groups, N, bytes);
    dim3 grid((unsigned)((N + dpb - 1) / dpb), (unsigned)groups);
    return polus_launch_lds<pq_scores_kernel<QT, PIECE>>("polus_pq_scores", grid, dim3(PQ_SCAN_THREADS), PQ_LDS_MAX, bytes,
                                                         st, lut, codes, ldc, score, lds, Q, N, m, ksub, dpb);
}

template <int QT>
int pq_scores_pieces(const float* lut, const uint8_t* codes, long ldc, float* score, long lds, int Q, int N, int m, int ksub,
                     hipStream_t st) {
    switch (pq_piece_bytes(codes, ldc, m)) {
        case 16: return pq_scores_launch<QT, 16>(lut, codes, ldc, score, lds, Q, N, m, ksub, st);
        case 4: return pq_scores_launch<QT, 4>(lut, codes, ldc, score, lds, Q, N, m, ksub, st);
    }
    return pq_scores_launch<QT, 1>(lut, codes, ldc, score, lds, Q, N, m, ksub, st);
}

// ---------------------------------------------------------------- build-time kernels
// The pragma keeps every operation its own rounding (bm25_weights_kernel): NumPy float32 gives the same bits.

// Block (256 rows, sub-space j): the sub-space's codewords in LDS, read at wave-uniform addresses (a broadcast); a thread
// keeps its sub-vector in registers.  Codewords ascending and a strict <: ties go to the lower code, a NaN never enters.
template <typename T>
__global__ __launch_bounds__(256) void pq_encode_kernel(const T* __restrict__ x, long ldx, const float* __restrict__ codebook,
                                                        uint8_t* __restrict__ codes, long ldc, int rows, int m, int ksub,
                                                        int dsub) {
#pragma clang fp contract(off)
    __shared__ float cb[PQ_KMAX * PQ_DMAX];
    const int j = blockIdx.y;
    for (int i = threadIdx.x; i < ksub * dsub; i += 256) cb[i] = codebook[(size_t)j * ksub * dsub + i];
    __syncthreads();
    const long r = (long)blockIdx.x * 256 + threadIdx.x;
    if (r >= rows) return;
    const T* xr = x + (size_t)r * ldx + (size_t)j * dsub;
    float xs[PQ_DMAX];
#pragma unroll
    for (int t = 0; t < PQ_DMAX; ++t) xs[t] = t < dsub ? to_f<T>(xr[t]) : 0.f;
    float best = INFINITY;
    int bc = 0;
    for (int c = 0; c < ksub; ++c) {
        const float* cw = cb + c * dsub;
        float d = 0.f;
#pragma unroll
        for (int t = 0; t < PQ_DMAX; ++t)
            if (t < dsub) {                                   // uniform
                const float e = xs[t] - cw[t];
                const float e2 = e * e;
                d = d + e2;
            }
        if (d < best) { best = d; bc = c; }
    }
    codes[(size_t)r * ldc + j] = (uint8_t)bc;
}

// One wave per (j, c); the summation order is the header's.
template <typename T>
__global__ __launch_bounds__(256) void pq_update_kernel(const T* __restrict__ x, long ldx, const uint8_t* __restrict__ codes,
                                                        long ldc, const float* __restrict__ prev, float* __restrict__ out,
                                                        int32_t* __restrict__ counts, int Tn, int m, int ksub, int dsub) {
#pragma clang fp contract(off)
    const int lane = threadIdx.x & 63;
    const int jc = blockIdx.x * 4 + (threadIdx.x >> 6);       // wave-uniform
    if (jc >= m * ksub) return;
    const int j = jc / ksub, c = jc - j * ksub;
    const int per = (Tn + 63) / 64;
    const long lo = (long)lane * per;
    const long t0 = lo < Tn ? lo : Tn, t1 = t0 + per < Tn ? t0 + per : Tn;
    float p[PQ_DMAX];
#pragma unroll
    for (int t = 0; t < PQ_DMAX; ++t) p[t] = 0.f;
    int found = 0;
    for (long t = t0; t < t1; ++t) {
        if ((int)codes[(size_t)t * ldc + j] != c) continue;
        ++found;
        const T* xr = x + (size_t)t * ldx + (size_t)j * dsub;
#pragma unroll
        for (int e = 0; e < PQ_DMAX; ++e)
            if (e < dsub) p[e] = p[e] + to_f<T>(xr[e]);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        found += __shfl_xor(found, o, 64);
#pragma unroll
        for (int e = 0; e < PQ_DMAX; ++e)
            if (e < dsub) p[e] = p[e] + __shfl_xor(p[e], o, 64);
    }
    if (lane == 0) counts[jc] = found;
    const float cnt = (float)found;
#pragma unroll
    for (int e = 0; e < PQ_DMAX; ++e)
        if (e < dsub && lane == (e & 63)) out[(size_t)jc * dsub + e] = found > 0 ? p[e] / cnt : prev[(size_t)jc * dsub + e];
}

template <typename T>
__global__ __launch_bounds__(256) void pq_decode_kernel(const uint8_t* __restrict__ codes, long ldc,
                                                        const float* __restrict__ codebook, T* __restrict__ y, long ldy,
                                                        int rows, int m, int ksub, int dsub) {
    const int E = m * dsub;
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long)rows * E) return;
    const long r = i / E;
    const int e = (int)(i - r * E), j = e / dsub, t = e - j * dsub;
    const int c = codes[(size_t)r * ldc + j];
    y[(size_t)r * ldy + e] = from_f<T>(c < ksub ? codebook[((size_t)j * ksub + c) * dsub + t] : 0.f);
}

template <typename T>
__global__ __launch_bounds__(256) void pq_lut_kernel(const T* __restrict__ q, long ldq, const float* __restrict__ codebook,
                                                     float* __restrict__ lut, int Q, int m, int ksub, int dsub) {
#pragma clang fp contract(off)
    const long i = (long)blockIdx.x * 256 + threadIdx.x;      // (b, j, c), c fastest
    if (i >= (long)Q * m * ksub) return;
    const long b = i / ((long)m * ksub);
    const int jc = (int)(i - b * m * ksub), j = jc / ksub;
    const T* qs = q + (size_t)b * ldq + (size_t)j * dsub;
    const float* cw = codebook + (size_t)jc * dsub;
    float s = 0.f;
    for (int t = 0; t < dsub; ++t) {
        const float pr = to_f<T>(qs[t]) * cw[t];
        s = s + pr;
    }
    lut[i] = s;
}

int pq_check_scan(const char* what, int Q, int N, int m, int ksub) {
    if (int rc = pq_check_format(what, m, ksub, 1)) return rc;
    POLUS_REQUIRE(Q >= 1 && Q <= PQ_ROWS_MAX, "%s: need 1 <= Q <= %d (got %d)", what, PQ_ROWS_MAX, Q);
    POLUS_REQUIRE(N >= 1 && N <= PQ_ROWS_MAX, "%s: need 1 <= N <= %d (got %d)", what, PQ_ROWS_MAX, N);
    return POLUS_OK;
}

}  // namespace

extern "C" int polus_pq_scores_route(int Q, int N, int m, int ksub, int* out) {
    const char* what = "polus_pq_scores_route";
    if (int rc = pq_check_scan(what, Q, N, m, ksub)) return rc;
    POLUS_REQUIRE(out, "%s: null pointer", what);
    out[0] = pq_qt(Q, m);
    out[1] = (int)pq_lds_bytes(out[0], m);
    return POLUS_OK;
}

extern "C" int polus_pq_scores(const float* lut, const uint8_t* codes, long ldc, float* score, long lds, int Q, int N, int m,
                               int ksub, void* stream) {
    const char* what = "polus_pq_scores";
    if (int rc = pq_check_scan(what, Q, N, m, ksub)) return rc;
    POLUS_REQUIRE(ldc >= m, "%s: code row stride ldc must be >= m (got %ld < %d)", what, ldc, m);
    POLUS_REQUIRE(lds >= N, "%s: score row stride lds must be >= N (got %ld < %d)", what, lds, N);
    POLUS_REQUIRE(lut && codes && score, "%s: null pointer", what);
    hipStream_t st = static_cast<hipStream_t>(stream);
    switch (pq_qt(Q, m)) {
        case 4: return pq_scores_pieces<4>(lut, codes, ldc, score, lds, Q, N, m, ksub, st);
        case 2: return pq_scores_pieces<2>(lut, codes, ldc, score, lds, Q, N, m, ksub, st);
        default: return pq_scores_pieces<1>(lut, codes, ldc, score, lds, Q, N, m, ksub, st);
    }
}

extern "C" int polus_pq_encode(int dtype, const void* x, long ldx, const float* codebook, uint8_t* codes, long ldc, int rows,
                               int m, int ksub, int dsub, void* stream) {
    const char* what = "polus_pq_encode";
    PQ_CHECK_DTYPE(what, dtype);
    if (int rc = pq_check_format(what, m, ksub, dsub)) return rc;
    POLUS_REQUIRE(rows >= 1, "%s: need rows >= 1 (got %d)", what, rows);
    POLUS_REQUIRE(ldx >= (long)m * dsub, "%s: row stride ldx must be >= m*dsub (got %ld < %d)", what, ldx, m * dsub);
    POLUS_REQUIRE(ldc >= m, "%s: code row stride ldc must be >= m (got %ld < %d)", what, ldc, m);
    POLUS_REQUIRE(x && codebook && codes, "%s: null pointer", what);
    hipStream_t st = static_cast<hipStream_t>(stream);
    dim3 grid((unsigned)((rows + 255) / 256), (unsigned)m);
    if (dtype == POLUS_BF16)
        hipLaunchKernelGGL(pq_encode_kernel<bf16_t>, grid, dim3(256), 0, st, static_cast<const bf16_t*>(x), ldx, codebook,
                           codes, ldc, rows, m, ksub, dsub);
    else
        hipLaunchKernelGGL(pq_encode_kernel<float>, grid, dim3(256), 0, st, static_cast<const float*>(x), ldx, codebook, codes,
                           ldc, rows, m, ksub, dsub);
    POLUS_CHECK_LAUNCH(what);
    return POLUS_OK;
}

extern "C" int polus_pq_update(int dtype, const void* x, long ldx, const uint8_t* codes, long ldc, const float* prev,
                               float* out, int32_t* counts, int T, int m, int ksub, int dsub, void* stream) {
    const char* what = "polus_pq_update";
    PQ_CHECK_DTYPE(what, dtype);
    if (int rc = pq_check_format(what, m, ksub, dsub)) return rc;
    POLUS_REQUIRE(T >= 1, "%s: need T >= 1 (got %d)", what, T);
    POLUS_REQUIRE(ldx >= (long)m * dsub, "%s: row stride ldx must be >= m*dsub (got %ld < %d)", what, ldx, m * dsub);
    POLUS_REQUIRE(ldc >= m, "%s: code row stride ldc must be >= m (got %ld < %d)", what, ldc, m);
    POLUS_REQUIRE(x && codes && prev && out && counts, "%s: null pointer", what);
    POLUS_REQUIRE(out != prev, "%s: out must not alias prev", what);
    hipStream_t st = static_cast<hipStream_t>(stream);
    dim3 grid((unsigned)((m * ksub + 3) / 4));
    if (dtype == POLUS_BF16)
        hipLaunchKernelGGL(pq_update_kernel<bf16_t>, grid, dim3(256), 0, st, static_cast<const bf16_t*>(x), ldx, codes, ldc,
                           prev, out, counts, T, m, ksub, dsub);
    else
        hipLaunchKernelGGL(pq_update_kernel<float>, grid, dim3(256), 0, st, static_cast<const float*>(x), ldx, codes, ldc, prev,
                           out, counts, T, m, ksub, dsub);
    POLUS_CHECK_LAUNCH(what);
    return POLUS_OK;
}

extern "C" int polus_pq_decode(const uint8_t* codes, long ldc, const float* codebook, int dtype, void* y, long ldy, int rows,
                               int m, int ksub, int dsub, void* stream) {
    const char* what = "polus_pq_decode";
    PQ_CHECK_DTYPE(what, dtype);
    if (int rc = pq_check_format(what, m, ksub, dsub)) return rc;
    POLUS_REQUIRE(rows >= 1, "%s: need rows >= 1 (got %d)", what, rows);
    POLUS_REQUIRE(ldc >= m, "%s: code row stride ldc must be >= m (got %ld < %d)", what, ldc, m);
    POLUS_REQUIRE(ldy >= (long)m * dsub, "%s: row stride ldy must be >= m*dsub (got %ld < %d)", what, ldy, m * dsub);
    POLUS_REQUIRE(codes && codebook && y, "%s: null pointer", what);
    hipStream_t st = static_cast<hipStream_t>(stream);
    const long total = (long)rows * m * dsub;
    POLUS_REQUIRE((total + 255) / 256 <= 0x7FFFFFFFL, "%s: rows * m * dsub = %ld elements are more than one launch takes", what, total);
    dim3 grid((unsigned)((total + 255) / 256));
    if (dtype == POLUS_BF16)
        hipLaunchKernelGGL(pq_decode_kernel<bf16_t>, grid, dim3(256), 0, st, codes, ldc, codebook, static_cast<bf16_t*>(y), ldy,
                           rows, m, ksub, dsub);
    else
        hipLaunchKernelGGL(pq_decode_kernel<float>, grid, dim3(256), 0, st, codes, ldc, codebook, static_cast<float*>(y), ldy,
                           rows, m, ksub, dsub);
    POLUS_CHECK_LAUNCH(what);
    return POLUS_OK;
}

extern "C" int polus_pq_lut(int dtype, const void* q, long ldq, const float* codebook, float* lut, int Q, int m, int ksub,
                            int dsub, void* stream) {
    const char* what = "polus_pq_lut";
    PQ_CHECK_DTYPE(what, dtype);
    if (int rc = pq_check_format(what, m, ksub, dsub)) return rc;
    POLUS_REQUIRE(Q >= 1, "%s: need Q >= 1 (got %d)", what, Q);
    POLUS_REQUIRE(ldq >= (long)m * dsub, "%s: row stride ldq must be >= m*dsub (got %ld < %d)", what, ldq, m * dsub);
    POLUS_REQUIRE(q && codebook && lut, "%s: null pointer", what);
    hipStream_t st = static_cast<hipStream_t>(stream);
    const long total = (long)Q * m * ksub;
    POLUS_REQUIRE((total + 255) / 256 <= 0x7FFFFFFFL, "%s: Q * m * ksub = %ld entries are more than one launch takes", what, total);
    dim3 grid((unsigned)((total + 255) / 256));
    if (dtype == POLUS_BF16)
        hipLaunchKernelGGL(pq_lut_kernel<bf16_t>, grid, dim3(256), 0, st, static_cast<const bf16_t*>(q), ldq, codebook, lut, Q, m,
                           ksub, dsub);
    else
        hipLaunchKernelGGL(pq_lut_kernel<float>, grid, dim3(256), 0, st, static_cast<const float*>(q), ldq, codebook, lut, Q, m,
                           ksub, dsub);
    POLUS_CHECK_LAUNCH(what);
    return POLUS_OK;
}
