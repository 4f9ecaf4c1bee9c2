// Learned sparse retrieval (SPLADE) on gfx950: the vocabulary-wide max pooling of the masked-LM logits, forward and
// backward, the FLOPS sparsity regulariser, and the sparse-document x dense-query scoring kernel of the index
// (polus_amd/ir/models.py SpladeEncoder, ir/training.py SparseRetrievalTrainer, ir/search.py SparseCorpusIndex).
//
// polus_splade_pool_fwd / _bwd: pure HBM streaming.  A lane owns one 16-byte chunk of columns (4 f32 / 8 bf16) of one
// sequence and walks the S token rows, SP_UN rows in flight; consecutive lanes hold consecutive chunks, so a wave moves
// 1 KiB of one row per step.  Grid = (chunks / 256, B): 960 workgroups in bf16 and 1920 in f32 at 64 x 256 x 30522.  The
// columns behind the last whole chunk, and every column where a pointer or stride is not 16-byte aligned, go one
// element per lane through the same loop (a max, a compare and one log1pf per column: the bits cannot differ).
// A masked token's row is not read (the mask is uniform over a workgroup); backward reads nothing of the logits.
// polus_flops_reg: lane l of workgroup k (one wave) owns columns 256 k + 4 l .. + 3 and adds their rows in ascending
// b; the squares go through one xor tree per wave, the waves' partials through LDS in index order.
// polus_sparse_scores: one workgroup per (query, range of documents) with the query row in LDS, one wave per document,
// eight documents of a wave in flight.
// No atomics, no scratch, no workspace but the regulariser's partials; bitwise reproducible.
#include <algorithm>

#include "common.h"

namespace {

constexpr int SP_THREADS = 256;
constexpr int SP_UN = 8;                          // token rows a lane has in flight

template <typename T> struct SpChunk { static constexpr int E = 16 / (int)sizeof(T); };

// N consecutive elements as floats: one 16-byte load (N = E) or one element (N = 1)
template <typename T, int N> struct SpRaw;
template <typename T> struct SpRaw<T, 1> { T v; };
template <> struct SpRaw<float, 4> { uint4 v; };
template <> struct SpRaw<bf16_t, 8> { uint4 v; };

template <typename T> __device__ __forceinline__ void sp_load(SpRaw<T, 1>& r, const T* p) { r.v = *p; }
__device__ __forceinline__ void sp_load(SpRaw<float, 4>& r, const float* p) { r.v = *reinterpret_cast<const uint4*>(p); }
__device__ __forceinline__ void sp_load(SpRaw<bf16_t, 8>& r, const bf16_t* p) { r.v = *reinterpret_cast<const uint4*>(p); }

template <typename T> __device__ __forceinline__ void sp_unpack(const SpRaw<T, 1>& r, float (&v)[1]) { v[0] = to_f<T>(r.v); }
__device__ __forceinline__ void sp_unpack(const SpRaw<float, 4>& r, float (&v)[4]) {
    v[0] = __uint_as_float(r.v.x); v[1] = __uint_as_float(r.v.y); v[2] = __uint_as_float(r.v.z); v[3] = __uint_as_float(r.v.w);
}
__device__ __forceinline__ void sp_unpack(const SpRaw<bf16_t, 8>& r, float (&v)[8]) {
    const bf16x8 t = __builtin_bit_cast(bf16x8, r.v);
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = (float)t[j];
}

template <typename T> __device__ __forceinline__ void sp_store(T* p, const float (&v)[1]) { *p = from_f<T>(v[0]); }
__device__ __forceinline__ void sp_store(float* p, const float (&v)[4]) {
    *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]);
}
__device__ __forceinline__ void sp_store(bf16_t* p, const float (&v)[8]) {
    bf16x8 t;
#pragma unroll
    for (int j = 0; j < 8; ++j) t[j] = (bf16_t)v[j];
    *reinterpret_cast<uint4*>(p) = __builtin_bit_cast(uint4, t);
}

// N outputs of one f32 / int32 row: 16-byte stores when `wide` (uniform), single elements otherwise
template <typename U, int N> __device__ __forceinline__ void sp_put(U* p, const U (&v)[N], bool wide) {
    if (N >= 4 && wide) {
#pragma unroll
        for (int j = 0; j < N; j += 4) {
            if constexpr (sizeof(U) == 4 && N >= 4)
                *reinterpret_cast<uint4*>(p + j) = make_uint4(__builtin_bit_cast(uint32_t, v[j]), __builtin_bit_cast(uint32_t, v[j + 1]),
                                                              __builtin_bit_cast(uint32_t, v[j + 2]), __builtin_bit_cast(uint32_t, v[j + 3]));
        }
    } else {
#pragma unroll
        for (int j = 0; j < N; ++j) p[j] = v[j];
    }
}
template <typename U, int N> __device__ __forceinline__ void sp_get(const U* p, U (&v)[N], bool wide) {
    if (N >= 4 && wide) {
#pragma unroll
        for (int j = 0; j < N; j += 4) {
            if constexpr (sizeof(U) == 4 && N >= 4) {
                const uint4 q = *reinterpret_cast<const uint4*>(p + j);
                v[j] = __builtin_bit_cast(U, q.x); v[j + 1] = __builtin_bit_cast(U, q.y);
                v[j + 2] = __builtin_bit_cast(U, q.z); v[j + 3] = __builtin_bit_cast(U, q.w);
            }
        }
    } else {
#pragma unroll
        for (int j = 0; j < N; ++j) v[j] = p[j];
    }
}

// The running maximum starts at 0 with no winner: only a value > 0 can enter, the first (lowest s) to reach the
// maximum keeps it, NaN compares false.  That is the contract's "no valid token or m <= 0 -> (0, 0, -1)".
template <typename T, int N>
__device__ __forceinline__ void pool_fwd_cols(const T* x, long ldl, const int32_t* mrow, int S, float* rep, float* xmax,
                                              int32_t* arg, bool wide) {
    float m[N];
    int32_t a[N];
#pragma unroll
    for (int j = 0; j < N; ++j) { m[j] = 0.f; a[j] = -1; }
    // The mask of a group of rows is fetched one group ahead, behind the data loads of the group before: loads return in
    // order, so a mask load in front of data loads that do not depend on it would hold them back.
    int mk[SP_UN];
#pragma unroll
    for (int u = 0; u < SP_UN; ++u) mk[u] = mrow ? mrow[min(u, S - 1)] : 1;
    for (int s0 = 0; s0 < S; s0 += SP_UN) {
        SpRaw<T, N> raw[SP_UN];
        bool ok[SP_UN];
#pragma unroll
        for (int u = 0; u < SP_UN; ++u)
            ok[u] = s0 + u < S && __builtin_amdgcn_readfirstlane(mk[u]) != 0;        // uniform over the workgroup
#pragma unroll
        for (int u = 0; u < SP_UN; ++u)
            if (ok[u]) sp_load(raw[u], x + (long)(s0 + u) * ldl);
        if (mrow) {
#pragma unroll
            for (int u = 0; u < SP_UN; ++u) mk[u] = mrow[min(s0 + SP_UN + u, S - 1)];
        }
#pragma unroll
        for (int u = 0; u < SP_UN; ++u) {
            if (!ok[u]) continue;
            float v[N];
            sp_unpack(raw[u], v);
#pragma unroll
            for (int j = 0; j < N; ++j)
                if (v[j] > m[j]) { m[j] = v[j]; a[j] = s0 + u; }
        }
    }
    float r[N];
#pragma unroll
    for (int j = 0; j < N; ++j) r[j] = a[j] >= 0 ? log1pf(m[j]) : 0.f;
    sp_put<float, N>(rep, r, wide);
    sp_put<float, N>(xmax, m, wide);
    sp_put<int32_t, N>(arg, a, wide);
}

// items of a sequence: `nchunk` whole chunks of E columns, then the columns behind them one by one (VEC), or V columns
template <typename T, bool VEC>
__global__ __launch_bounds__(SP_THREADS) void splade_pool_fwd_kernel(const T* __restrict__ logits, long ldl,
                                                                     const int32_t* __restrict__ mask,
                                                                     float* __restrict__ rep, long ldr,
                                                                     float* __restrict__ xmax, long ldx,
                                                                     int32_t* __restrict__ arg, long lda, int S, int V,
                                                                     int wide) {
    constexpr int E = SpChunk<T>::E;
    const int b = blockIdx.y;
    const int item = blockIdx.x * SP_THREADS + threadIdx.x;
    const int nchunk = VEC ? V / E : 0;
    const T* x = logits + (long)b * S * ldl;
    const int32_t* mrow = mask ? mask + (long)b * S : nullptr;
    if (VEC && item < nchunk) {
        const int c = item * E;
        pool_fwd_cols<T, E>(x + c, ldl, mrow, S, rep + b * ldr + c, xmax + b * ldx + c, arg + b * lda + c, wide != 0);
        return;
    }
    const int c = nchunk * E + (item - nchunk);
    if (c < V) pool_fwd_cols<T, 1>(x + c, ldl, mrow, S, rep + b * ldr + c, xmax + b * ldx + c, arg + b * lda + c, false);
}

template <typename T, int N>
__device__ __forceinline__ void pool_bwd_cols(const float* drep, const float* xmax, const int32_t* arg, T* d, long lddl,
                                              int S, bool wide) {
    float g[N], m[N];
    int32_t a[N];
    sp_get<float, N>(drep, g, wide);
    sp_get<float, N>(xmax, m, wide);
    sp_get<int32_t, N>(arg, a, wide);
#pragma unroll
    for (int j = 0; j < N; ++j) g[j] = g[j] / (1.0f + m[j]);          // IEEE division; rounded to T once, in the store
    for (int s = 0; s < S; ++s) {
        float v[N];
#pragma unroll
        for (int j = 0; j < N; ++j) v[j] = a[j] == s ? g[j] : 0.f;
        sp_store(d + (long)s * lddl, v);
    }
}

template <typename T, bool VEC>
__global__ __launch_bounds__(SP_THREADS) void splade_pool_bwd_kernel(const float* __restrict__ drep, long lddr,
                                                                     const float* __restrict__ xmax, long ldx,
                                                                     const int32_t* __restrict__ arg, long lda,
                                                                     T* __restrict__ dlogits, long lddl, int S, int V,
                                                                     int wide) {
    constexpr int E = SpChunk<T>::E;
    const int b = blockIdx.y;
    const int item = blockIdx.x * SP_THREADS + threadIdx.x;
    const int nchunk = VEC ? V / E : 0;
    T* d = dlogits + (long)b * S * lddl;
    if (VEC && item < nchunk) {
        const int c = item * E;
        pool_bwd_cols<T, E>(drep + b * lddr + c, xmax + b * ldx + c, arg + b * lda + c, d + c, lddl, S, wide != 0);
        return;
    }
    const int c = nchunk * E + (item - nchunk);
    if (c < V) pool_bwd_cols<T, 1>(drep + b * lddr + c, xmax + b * ldx + c, arg + b * lda + c, d + c, lddl, S, false);
}

// ---------------------------------------------------------------- FLOPS regulariser
constexpr int FR_COLS = 256;                      // columns per workgroup (one wave, 4 per lane)
constexpr int FR_UN = 16;                         // rows a lane has in flight

// columns c .. c + 3 of one row: one 16-byte access (`wide`, and all four inside V) or up to four single elements
__device__ __forceinline__ float4 fr_load4(const float* p, int c, int V, bool wide) {
    if (wide) return *reinterpret_cast<const float4*>(p + c);
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (c < V) v.x = p[c];
    if (c + 1 < V) v.y = p[c + 1];
    if (c + 2 < V) v.z = p[c + 2];
    if (c + 3 < V) v.w = p[c + 3];
    return v;
}
__device__ __forceinline__ void fr_store4(float* p, int c, int V, bool wide, const float4& v) {
    if (wide) { *reinterpret_cast<float4*>(p + c) = v; return; }
    if (c < V) p[c] = v.x;
    if (c + 1 < V) p[c + 1] = v.y;
    if (c + 2 < V) p[c + 2] = v.z;
    if (c + 3 < V) p[c + 3] = v.w;
}

// FR_UN rows in flight on either access width: a contiguous [rows, 30522] matrix has every other row off the 16-byte
// grid, so the single-element form is the one a trainer's representations take.
__global__ __launch_bounds__(64) void flops_reg_cols_kernel(const float* __restrict__ rep, long ldr, int rows, int V,
                                                            float coef, float* __restrict__ drep, long lddr,
                                                            float* __restrict__ partial, int rep_wide, int drep_wide) {
    const int c = blockIdx.x * FR_COLS + 4 * threadIdx.x;
    const bool whole = c + 3 < V;
    const bool rw = whole && rep_wide, dw = whole && drep_wide;
    float s[4] = {0.f, 0.f, 0.f, 0.f};
    for (int b0 = 0; b0 < rows; b0 += FR_UN) {
        float4 v[FR_UN];
#pragma unroll
        for (int u = 0; u < FR_UN; ++u)
            v[u] = b0 + u < rows ? fr_load4(rep + (long)(b0 + u) * ldr, c, V, rw) : make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
        for (int u = 0; u < FR_UN; ++u)
            if (b0 + u < rows) { s[0] += v[u].x; s[1] += v[u].y; s[2] += v[u].z; s[3] += v[u].w; }
    }
    float mean[4], sq = 0.f;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        mean[j] = s[j] / (float)rows;
        sq += mean[j] * mean[j];
    }
    sq = wave_sum(sq);
    if (threadIdx.x == 0) partial[blockIdx.x] = sq;
    if (drep == nullptr) return;
    float g[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) g[j] = coef * mean[j];
    for (int b0 = 0; b0 < rows; b0 += FR_UN) {                  // a group's loads before its stores: rows do not overlap
        float4 v[FR_UN];
#pragma unroll
        for (int u = 0; u < FR_UN; ++u)
            if (b0 + u < rows) v[u] = fr_load4(drep + (long)(b0 + u) * lddr, c, V, dw);
#pragma unroll
        for (int u = 0; u < FR_UN; ++u)
            if (b0 + u < rows)
                fr_store4(drep + (long)(b0 + u) * lddr, c, V, dw, make_float4(v[u].x + g[0], v[u].y + g[1], v[u].z + g[2], v[u].w + g[3]));
    }
}

// the partials in index order, 1024 at a time through LDS; loss = (loss +) lambda * sum
__global__ __launch_bounds__(256) void flops_reg_finalize_kernel(const float* __restrict__ partial, int n, float lambda,
                                                                 float* __restrict__ loss, int accumulate) {
    __shared__ float sp[1024];
    float t = 0.f;
    for (int base = 0; base < n; base += 1024) {
        const int cnt = min(1024, n - base);
        for (int k = threadIdx.x; k < cnt; k += 256) sp[k] = partial[base + k];
        __syncthreads();
        if (threadIdx.x == 0)
            for (int k = 0; k < cnt; ++k) t += sp[k];
        __syncthreads();
    }
    if (threadIdx.x == 0) loss[0] = accumulate ? loss[0] + lambda * t : lambda * t;
}

// ---------------------------------------------------------------- sparse documents x dense queries
constexpr int SS_THREADS = 1024;                  // 16 waves: 4 per SIMD, as centroid_scores_kernel's LDS route
constexpr int SS_DU = 8;                         // documents a wave has in flight
constexpr int SS_MMAX = 1024;                     // what polus_topk_merge can produce
constexpr size_t SS_LDS_MAX = 160 * 1024;         // one CU's LDS; the kernel keeps nothing beside the query row

// Documents per workgroup: about four workgroups per CU over the launch, never fewer than one group of SS_DU per wave
// unless N is smaller, so that the copy of the query row is a small share of the work (centroid.hip cs_docs_per_block).
static int ss_docs_per_block(int B, int N, int nw) {
    const long per_query = std::max(1L, 4L * polus_num_cus() / B);
    long dpb = std::max(((long)N + per_query - 1) / per_query, (long)SS_DU * nw);
    dpb = (dpb + (long)SS_DU * nw - 1) / ((long)SS_DU * nw) * ((long)SS_DU * nw);
    return (int)std::min(dpb, (long)N);
}

__global__ __launch_bounds__(SS_THREADS) void sparse_scores_kernel(const float* __restrict__ q, long ldq,
                                                                   const int32_t* __restrict__ ids, long ldi,
                                                                   const float* __restrict__ w, long ldw,
                                                                   float* __restrict__ score, long lds, int N, int M,
                                                                   int V, int dpb, int nblk) {
    extern __shared__ __align__(16) float ss_q[];             // the query row, [V]
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int b = blockIdx.x / nblk;
    const int blk = blockIdx.x - b * nblk;
    const long n0 = (long)blk * dpb, n1 = min((long)N, n0 + dpb);
    const float* qrow = q + (long)b * ldq;
    if ((((uintptr_t)qrow) & 15) == 0) {                      // uniform
        const int nchunk = V >> 2;
        for (int c = threadIdx.x; c < nchunk; c += SS_THREADS)
            reinterpret_cast<float4*>(ss_q)[c] = reinterpret_cast<const float4*>(qrow)[c];
        const int i = (nchunk << 2) + threadIdx.x;
        if (i < V) ss_q[i] = qrow[i];
    } else {
        for (int i = threadIdx.x; i < V; i += SS_THREADS) ss_q[i] = qrow[i];
    }
    __syncthreads();
    // SS_DU documents of a wave at a time, their loads issued together: one document's few loads would leave the wave
    // waiting out a memory round trip per document.  A document's own arithmetic is the same whatever shares the group.
    for (long g = n0 + (long)wave * SS_DU; g < n1; g += (long)(SS_THREADS / 64) * SS_DU) {
        float p[SS_DU];
#pragma unroll
        for (int u = 0; u < SS_DU; ++u) p[u] = 0.f;
        for (int m = lane; m < M; m += 64) {                  // ascending m within a lane
            int id[SS_DU];
            float wv[SS_DU];
#pragma unroll
            for (int u = 0; u < SS_DU; ++u) {
                const long n = min(g + u, n1 - 1);            // a group's tail repeats the last document: not stored
                id[u] = ids[n * ldi + m];
                wv[u] = w[n * ldw + m];
            }
#pragma unroll
            for (int u = 0; u < SS_DU; ++u)
                if ((unsigned)id[u] < (unsigned)V) p[u] = fmaf(wv[u], ss_q[id[u]], p[u]);
        }
#pragma unroll
        for (int u = 0; u < SS_DU; ++u) {
            const float t = wave_sum(p[u]);
            if (lane == 0 && g + u < n1) score[(long)b * lds + g + u] = t;
        }
    }
}

int sp_check_pool(const char* who, int dtype, int B, int S, int V) {
    POLUS_REQUIRE(dtype == POLUS_F32 || dtype == POLUS_BF16, "%s: bad dtype %d", who, dtype);
    POLUS_REQUIRE(B >= 1 && B <= 65535 && S >= 1 && V >= 1, "%s: bad shape B=%d S=%d V=%d (need 1 <= B <= 65535, S >= 1, V >= 1)", who, B, S, V);
    return POLUS_OK;
}

static inline bool sp_wide4(const void* p, long ld) { return polus_aligned16(p) && ld % 4 == 0; }

}  // namespace

extern "C" int polus_splade_pool_fwd(int dtype, const void* logits, long ldl, const int32_t* mask, float* rep, long ldr,
                                     float* xmax, long ldx, int32_t* arg, long lda, int B, int S, int V, void* stream) {
    const char* who = "polus_splade_pool_fwd";
    if (int rc = sp_check_pool(who, dtype, B, S, V)) return rc;
    POLUS_REQUIRE(logits && rep && xmax && arg, "%s: null pointer", who);
    POLUS_REQUIRE(ldl >= V && ldr >= V && ldx >= V && lda >= V, "%s: bad stride ldl=%ld ldr=%ld ldx=%ld lda=%ld (each must be >= V = %d)",
                  who, ldl, ldr, ldx, lda, V);
    const size_t es = polus_dtype_size(dtype);
    POLUS_REQUIRE(((uintptr_t)logits % es) == 0 && ((uintptr_t)rep % 4) == 0 && ((uintptr_t)xmax % 4) == 0 && ((uintptr_t)arg % 4) == 0,
                  "%s: pointer not aligned to its element", who);
    const bool vec = polus_aligned16(logits) && ((size_t)ldl * es) % 16 == 0;
    const int wide = sp_wide4(rep, ldr) && sp_wide4(xmax, ldx) && sp_wide4(arg, lda);
    const int E = 16 / (int)es;
    const int items = vec ? V / E + V % E : V;
    const dim3 grid((unsigned)((items + SP_THREADS - 1) / SP_THREADS), (unsigned)B), block(SP_THREADS);
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (dtype == POLUS_BF16) {
        if (vec) hipLaunchKernelGGL((splade_pool_fwd_kernel<bf16_t, true>), grid, block, 0, st, (const bf16_t*)logits, ldl, mask, rep, ldr, xmax, ldx, arg, lda, S, V, wide);
        else hipLaunchKernelGGL((splade_pool_fwd_kernel<bf16_t, false>), grid, block, 0, st, (const bf16_t*)logits, ldl, mask, rep, ldr, xmax, ldx, arg, lda, S, V, wide);
    } else {
        if (vec) hipLaunchKernelGGL((splade_pool_fwd_kernel<float, true>), grid, block, 0, st, (const float*)logits, ldl, mask, rep, ldr, xmax, ldx, arg, lda, S, V, wide);
        else hipLaunchKernelGGL((splade_pool_fwd_kernel<float, false>), grid, block, 0, st, (const float*)logits, ldl, mask, rep, ldr, xmax, ldx, arg, lda, S, V, wide);
    }
    POLUS_CHECK_LAUNCH(who);
    return POLUS_OK;
}

extern "C" int polus_splade_pool_bwd(int dtype, const float* drep, long lddr, const float* xmax, long ldx,
                                     const int32_t* arg, long lda, void* dlogits, long lddl, int B, int S, int V,
                                     void* stream) {
    const char* who = "polus_splade_pool_bwd";
    if (int rc = sp_check_pool(who, dtype, B, S, V)) return rc;
    POLUS_REQUIRE(drep && xmax && arg && dlogits, "%s: null pointer", who);
    POLUS_REQUIRE(lddr >= V && ldx >= V && lda >= V && lddl >= V, "%s: bad stride lddr=%ld ldx=%ld lda=%ld lddl=%ld (each must be >= V = %d)",
                  who, lddr, ldx, lda, lddl, V);
    const size_t es = polus_dtype_size(dtype);
    POLUS_REQUIRE(((uintptr_t)dlogits % es) == 0 && ((uintptr_t)drep % 4) == 0 && ((uintptr_t)xmax % 4) == 0 && ((uintptr_t)arg % 4) == 0,
                  "%s: pointer not aligned to its element", who);
    const bool vec = polus_aligned16(dlogits) && ((size_t)lddl * es) % 16 == 0;
    const int wide = sp_wide4(drep, lddr) && sp_wide4(xmax, ldx) && sp_wide4(arg, lda);
    const int E = 16 / (int)es;
    const int items = vec ? V / E + V % E : V;
    const dim3 grid((unsigned)((items + SP_THREADS - 1) / SP_THREADS), (unsigned)B), block(SP_THREADS);
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (dtype == POLUS_BF16) {
        if (vec) hipLaunchKernelGGL((splade_pool_bwd_kernel<bf16_t, true>), grid, block, 0, st, drep, lddr, xmax, ldx, arg, lda, (bf16_t*)dlogits, lddl, S, V, wide);
        else hipLaunchKernelGGL((splade_pool_bwd_kernel<bf16_t, false>), grid, block, 0, st, drep, lddr, xmax, ldx, arg, lda, (bf16_t*)dlogits, lddl, S, V, wide);
    } else {
        if (vec) hipLaunchKernelGGL((splade_pool_bwd_kernel<float, true>), grid, block, 0, st, drep, lddr, xmax, ldx, arg, lda, (float*)dlogits, lddl, S, V, wide);
        else hipLaunchKernelGGL((splade_pool_bwd_kernel<float, false>), grid, block, 0, st, drep, lddr, xmax, ldx, arg, lda, (float*)dlogits, lddl, S, V, wide);
    }
    POLUS_CHECK_LAUNCH(who);
    return POLUS_OK;
}

// one f32 per workgroup of FR_COLS columns
extern "C" size_t polus_flops_reg_workspace_bytes(int V) {
    return (size_t)((std::max(V, 0) + FR_COLS - 1) / FR_COLS) * sizeof(float);
}

extern "C" int polus_flops_reg(const float* rep, long ldr, int rows, int V, float lambda, float* loss, int loss_accumulate,
                               float* drep, long lddr, void* workspace, size_t workspace_bytes, void* stream) {
    const char* who = "polus_flops_reg";
    POLUS_REQUIRE(rows >= 1 && V >= 1, "%s: bad shape rows=%d V=%d", who, rows, V);
    POLUS_REQUIRE(rep && loss, "%s: null pointer", who);
    POLUS_REQUIRE(ldr >= V && (!drep || lddr >= V), "%s: bad stride ldr=%ld lddr=%ld (each must be >= V = %d)", who, ldr, lddr, V);
    POLUS_REQUIRE(((uintptr_t)rep % 4) == 0 && ((uintptr_t)drep % 4) == 0 && ((uintptr_t)loss % 4) == 0, "%s: pointer not aligned to its element", who);
    POLUS_REQUIRE(drep != rep, "%s: drep must not be rep", who);
    if (!workspace || workspace_bytes < polus_flops_reg_workspace_bytes(V)) { polus_set_error("%s: workspace too small", who); return POLUS_ERR_WORKSPACE; }
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int nblk = (V + FR_COLS - 1) / FR_COLS;
    float* partial = static_cast<float*>(workspace);
    hipLaunchKernelGGL(flops_reg_cols_kernel, dim3((unsigned)nblk), dim3(64), 0, st, rep, ldr, rows, V,
                       lambda * (2.0f / (float)rows), drep, lddr, partial, (int)sp_wide4(rep, ldr), (int)(drep && sp_wide4(drep, lddr)));
    POLUS_CHECK_LAUNCH("polus_flops_reg(columns)");
    hipLaunchKernelGGL(flops_reg_finalize_kernel, dim3(1), dim3(256), 0, st, partial, nblk, lambda, loss, loss_accumulate);
    POLUS_CHECK_LAUNCH("polus_flops_reg(finalize)");
    return POLUS_OK;
}

extern "C" int polus_sparse_scores(const float* q, long ldq, const int32_t* ids, long ldi, const float* w, long ldw,
                                   float* score, long lds, int B, int N, int M, int V, void* stream) {
    const char* who = "polus_sparse_scores";
    POLUS_REQUIRE(M >= 1 && M <= SS_MMAX, "%s: need 1 <= M <= %d terms per document (got %d)", who, SS_MMAX, M);
    POLUS_REQUIRE(B >= 1 && N >= 1 && V >= 1, "%s: bad shape B=%d N=%d V=%d", who, B, N, V);
    POLUS_REQUIRE((size_t)V * sizeof(float) <= SS_LDS_MAX,
                  "%s: the query row must fit LDS: V * 4 = %zu bytes > %zu (V <= %zu); there is no global-memory route", who,
                  (size_t)V * sizeof(float), SS_LDS_MAX, SS_LDS_MAX / sizeof(float));
    POLUS_REQUIRE(q && ids && w && score, "%s: null pointer", who);
    POLUS_REQUIRE(ldq >= V && ldi >= M && ldw >= M && lds >= N, "%s: bad stride ldq=%ld ldi=%ld ldw=%ld lds=%ld (need ldq >= V, ldi, ldw >= M, lds >= N)",
                  who, ldq, ldi, ldw, lds);
    POLUS_REQUIRE(((uintptr_t)q % 4) == 0 && ((uintptr_t)ids % 4) == 0 && ((uintptr_t)w % 4) == 0 && ((uintptr_t)score % 4) == 0,
                  "%s: pointer not aligned to its element", who);
    const int dpb = ss_docs_per_block(B, N, SS_THREADS / 64);
    const long nblk = ((long)N + dpb - 1) / dpb;
    POLUS_REQUIRE(nblk * B <= 0x7FFFFFFFL, "%s: B * workgroups per query = %ld exceeds the grid limit 2^31 - 1", who, nblk * B);
    const size_t lds_bytes = ((size_t)V * sizeof(float) + 15) / 16 * 16;
    return polus_launch_lds<sparse_scores_kernel>(who, dim3((unsigned)(nblk * B)), dim3(SS_THREADS), SS_LDS_MAX, lds_bytes,
                                                  static_cast<hipStream_t>(stream), q, ldq, ids, ldi, w, ldw, score, lds, N, M, V,
                                                  dpb, (int)nblk);
}
