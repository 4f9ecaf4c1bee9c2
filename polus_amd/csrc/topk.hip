// Exact running top-k of score rows (corpus search, polus_amd/ir/search.py).
//
// One workgroup per row.  A candidate (score, id) becomes one 64-bit key,
//     key = orderable(score bits) << 32 | (0x7fffffff - id),
// so "score descending, ties to the lower id" is plain unsigned key order, and since ids are unique it is a total
// order: the k best keys of a set do not depend on the order they were seen in.  Key 0 is "no candidate" (it decodes
// to (-inf, -1)); no valid score maps to it.
// LDS holds S keys: the current top K = pow2 >= k in front and a candidate buffer of S - K behind it.  The row is
// streamed in tiles of 1024 columns with 16-byte loads (the next four tiles' loads in flight); a column whose key
// beats the current k-th key is appended to the buffer through an LDS integer counter.  Before a tile that might not
// fit (count + 1024 > S - K, decided by every thread from the same count) the whole array is bitonic-sorted
// descending, which leaves the new top K in front and raises the threshold.  The slot order inside the buffer varies
// from run to run; the sorted result cannot.
// polus_topk_merge_ids runs the same body with the id of a column read from an int32 row beside the scores instead
// of counted from id0; a column with a negative id is no candidate.
#include "common.h"

namespace {

constexpr int TK_THREADS = 256;
constexpr int TK_TILE = TK_THREADS * 4;            // columns per tile: one float4 per thread
constexpr int TK_AHEAD = 4;                        // tiles whose loads are in flight
constexpr int TK_KMAX = 1024;
typedef unsigned long long u64;

__device__ __forceinline__ u64 tk_key(float s, int id) {
    unsigned b = __float_as_uint(s);
    if ((b & 0x7fffffffu) > 0x7f800000u || b == 0xff800000u) return 0;      // NaN, -inf: not a candidate
    if (b == 0x80000000u) b = 0;                                            // -0.0 orders as +0.0
    const unsigned ord = (b & 0x80000000u) ? ~b : (b | 0x80000000u);        // >= 0x00800000 for every kept score
    return ((u64)ord << 32) | (unsigned)(0x7fffffff - id);
}

__device__ __forceinline__ void tk_unkey(u64 key, float& s, int& id) {
    if (key == 0) { s = -INFINITY; id = -1; return; }
    const unsigned ord = (unsigned)(key >> 32);
    s = __uint_as_float((ord & 0x80000000u) ? (ord ^ 0x80000000u) : ~ord);
    id = 0x7fffffff - (int)(unsigned)(key & 0xffffffffu);
}

// keys[0 .. m) descending, m a power of two <= S; every thread of the workgroup calls it
__device__ __forceinline__ void tk_sort_desc(u64* keys, int m) {
    for (int size = 2; size <= m; size <<= 1) {
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            for (int t = threadIdx.x; t < (m >> 1); t += TK_THREADS) {
                const int i = 2 * t - (t & (stride - 1)), j = i + stride;   // j < m
                const u64 a = keys[i], b = keys[j];
                const bool desc = (i & size) == 0;
                if ((a < b) == desc) { keys[i] = b; keys[j] = a; }
            }
            __syncthreads();
        }
    }
}

// the four columns c0 .. c0+3 of a row (c0 may be negative or reach past n at the row's ends); whole vectors inside
// [0, n) are 16-byte aligned by the choice of c0
__device__ __forceinline__ float4 tk_load(const float* row, long c0, int n) {
    if (c0 >= 0 && c0 + 4 <= n) return *reinterpret_cast<const float4*>(row + c0);
    float v[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const long c = c0 + e;
        v[e] = (c >= 0 && c < n) ? row[c] : -INFINITY;
    }
    return make_float4(v[0], v[1], v[2], v[3]);
}

// the ids of the same four columns; outside [0, n): -1, which is no candidate.  The id row need not share the score
// row's alignment, so a vector load is taken only where the address allows it.
__device__ __forceinline__ int4 tk_load_ids(const int32_t* row, long c0, int n) {
    if (c0 >= 0 && c0 + 4 <= n && (reinterpret_cast<uintptr_t>(row + c0) & 15) == 0)
        return *reinterpret_cast<const int4*>(row + c0);
    int v[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const long c = c0 + e;
        v[e] = (c >= 0 && c < n) ? row[c] : -1;
    }
    return make_int4(v[0], v[1], v[2], v[3]);
}

// The body of both kernels.  IDS = false: column c is document id0 + c (ids is not read); IDS = true: document
// ids[row][c], dropped where that is negative.
template <int S, bool IDS>
__device__ __forceinline__ void topk_merge_body(const float* __restrict__ scores, long lds,
                                                const int32_t* __restrict__ ids, long ldi, int n, int id0,
                                                float* __restrict__ top_val, int32_t* __restrict__ top_id, int k,
                                                int K, int init) {
    __shared__ u64 keys[S];                          // [0, K): the top; [K, S): candidates
    __shared__ int s_cnt;
    const int cap = S - K;                           // >= TK_TILE (host: S >= 2 K and S >= 2 TK_TILE)
    const float* row = scores + (size_t)blockIdx.x * lds;
    float* ov = top_val + (size_t)blockIdx.x * k;
    int32_t* oi = top_id + (size_t)blockIdx.x * k;
    const int32_t* idrow = IDS ? ids + (size_t)blockIdx.x * ldi : nullptr;

    for (int i = threadIdx.x; i < K; i += TK_THREADS) keys[i] = (init == 0 && i < k && oi[i] >= 0) ? tk_key(ov[i], oi[i]) : 0;
    if (threadIdx.x == 0) s_cnt = 0;
    __syncthreads();
    if (init == 0) tk_sort_desc(keys, K);            // the state need not arrive sorted for the threshold to be right
    u64 thresh = keys[k - 1];                        // 0 while fewer than k candidates are held: everything passes

    // columns are taken from c = -mis so that every whole vector is 16-byte aligned
    const int mis = (int)((reinterpret_cast<uintptr_t>(row) >> 2) & 3);
    const int ntiles = (int)(((long)n + mis + TK_TILE - 1) / TK_TILE);
    const long lane_c = 4 * (long)threadIdx.x - mis;            // n may be close to 2^31: column arithmetic in 64 bits
    float4 cur[TK_AHEAD], nxt[TK_AHEAD];
    int4 icur[TK_AHEAD], inxt[TK_AHEAD];             // IDS only
#pragma unroll
    for (int u = 0; u < TK_AHEAD; ++u) {
        cur[u] = tk_load(row, lane_c + (long)min(u, ntiles - 1) * TK_TILE, n);
        if constexpr (IDS) icur[u] = tk_load_ids(idrow, lane_c + (long)min(u, ntiles - 1) * TK_TILE, n);
    }

    for (int t0 = 0; t0 < ntiles; t0 += TK_AHEAD) {
#pragma unroll
        for (int u = 0; u < TK_AHEAD; ++u) {         // tiles past the end re-read the last tile and are not used
            nxt[u] = tk_load(row, lane_c + (long)min(t0 + TK_AHEAD + u, ntiles - 1) * TK_TILE, n);
            if constexpr (IDS) inxt[u] = tk_load_ids(idrow, lane_c + (long)min(t0 + TK_AHEAD + u, ntiles - 1) * TK_TILE, n);
        }
#pragma unroll
        for (int u = 0; u < TK_AHEAD; ++u) {
            if (t0 + u >= ntiles) break;             // uniform
            const int held = min(s_cnt, cap);
            __syncthreads();                         // every thread has read the same count
            if (held + TK_TILE > cap) {              // uniform: make room for a whole tile
                int m = 2 * K;
                while (m < K + held) m <<= 1;        // <= S
                for (int i = K + held + threadIdx.x; i < m; i += TK_THREADS) keys[i] = 0;
                if (threadIdx.x == 0) s_cnt = 0;
                __syncthreads();
                tk_sort_desc(keys, m);
                thresh = keys[k - 1];
                __syncthreads();                     // threshold read before anyone appends over keys[K ..]
            }
            const long c0 = lane_c + (long)(t0 + u) * TK_TILE;
            const float v[4] = {cur[u].x, cur[u].y, cur[u].z, cur[u].w};
            int id4[4] = {0, 0, 0, 0};
            if constexpr (IDS) { id4[0] = icur[u].x; id4[1] = icur[u].y; id4[2] = icur[u].z; id4[3] = icur[u].w; }
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const long c = c0 + e;
                u64 key;
                if constexpr (IDS)
                    key = (c >= 0 && c < n && id4[e] >= 0) ? tk_key(v[e], id4[e]) : 0;
                else
                    key = (c >= 0 && c < n) ? tk_key(v[e], id0 + (int)c) : 0;
                if (key > thresh) {
                    const int slot = atomicAdd(&s_cnt, 1);      // < cap: at most TK_TILE appends since the check
                    if (slot < cap) keys[K + slot] = key;
                }
            }
            __syncthreads();                         // appends done before the next count is read
        }
#pragma unroll
        for (int u = 0; u < TK_AHEAD; ++u) {
            cur[u] = nxt[u];
            if constexpr (IDS) icur[u] = inxt[u];
        }
    }

    const int held = min(s_cnt, cap);
    if (held > 0) {                                  // uniform (read after the last tile's barrier)
        int m = 2 * K;
        while (m < K + held) m <<= 1;
        for (int i = K + held + threadIdx.x; i < m; i += TK_THREADS) keys[i] = 0;
        __syncthreads();
        tk_sort_desc(keys, m);
    }
    for (int i = threadIdx.x; i < k; i += TK_THREADS) {
        float s;
        int id;
        tk_unkey(keys[i], s, id);
        ov[i] = s;
        oi[i] = id;
    }
}

template <int S>
__global__ __launch_bounds__(TK_THREADS) void topk_merge_kernel(const float* __restrict__ scores, long lds, int n,
                                                                int id0, float* __restrict__ top_val,
                                                                int32_t* __restrict__ top_id, int k, int K, int init) {
    topk_merge_body<S, false>(scores, lds, nullptr, 0, n, id0, top_val, top_id, k, K, init);
}

template <int S>
__global__ __launch_bounds__(TK_THREADS) void topk_merge_ids_kernel(const float* __restrict__ scores, long lds,
                                                                    const int32_t* __restrict__ ids, long ldi, int n,
                                                                    float* __restrict__ top_val,
                                                                    int32_t* __restrict__ top_id, int k, int K,
                                                                    int init) {
    topk_merge_body<S, true>(scores, lds, ids, ldi, n, 0, top_val, top_id, k, K, init);
}

}  // namespace

extern "C" int polus_topk_merge(const float* scores, long lds, int rows, int n, int32_t id0, float* top_val,
                                int32_t* top_id, int k, int init, void* stream) {
    POLUS_REQUIRE(k >= 1 && k <= TK_KMAX, "polus_topk_merge: need 1 <= k <= %d (got %d)", TK_KMAX, k);
    POLUS_REQUIRE(rows >= 1 && n >= 1, "polus_topk_merge: need rows >= 1 and n >= 1 (got %d, %d)", rows, n);
    POLUS_REQUIRE(id0 >= 0 && (long long)id0 + n <= 0x7fffffffLL,
                  "polus_topk_merge: need id0 >= 0 and id0 + n <= 2^31 - 1 (got id0 %d, n %d)", id0, n);
    POLUS_REQUIRE(lds >= n, "polus_topk_merge: score row stride lds must be >= n (got %ld < %d)", lds, n);
    POLUS_REQUIRE(scores && top_val && top_id, "polus_topk_merge: null pointer");
    int K = 1;
    while (K < k) K <<= 1;
    hipStream_t st = static_cast<hipStream_t>(stream);
    // S >= 2 K (a sort always covers the top and at least as many candidates) and S - K >= one tile
    if (K <= 512)
        hipLaunchKernelGGL(topk_merge_kernel<2048>, dim3((unsigned)rows), dim3(TK_THREADS), 0, st, scores, lds, n,
                           (int)id0, top_val, top_id, k, K, init);
    else
        hipLaunchKernelGGL(topk_merge_kernel<4096>, dim3((unsigned)rows), dim3(TK_THREADS), 0, st, scores, lds, n,
                           (int)id0, top_val, top_id, k, K, init);
    POLUS_CHECK_LAUNCH("polus_topk_merge");
    return POLUS_OK;
}

extern "C" int polus_topk_merge_ids(const float* scores, long lds, const int32_t* ids, long ldi, int rows, int n,
                                    float* top_val, int32_t* top_id, int k, int init, void* stream) {
    POLUS_REQUIRE(k >= 1 && k <= TK_KMAX, "polus_topk_merge_ids: need 1 <= k <= %d (got %d)", TK_KMAX, k);
    POLUS_REQUIRE(rows >= 1 && n >= 1, "polus_topk_merge_ids: need rows >= 1 and n >= 1 (got %d, %d)", rows, n);
    POLUS_REQUIRE(lds >= n, "polus_topk_merge_ids: score row stride lds must be >= n (got %ld < %d)", lds, n);
    POLUS_REQUIRE(ldi >= n, "polus_topk_merge_ids: id row stride ldi must be >= n (got %ld < %d)", ldi, n);
    POLUS_REQUIRE(scores && ids && top_val && top_id, "polus_topk_merge_ids: null pointer");
    int K = 1;
    while (K < k) K <<= 1;
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (K <= 512)
        hipLaunchKernelGGL(topk_merge_ids_kernel<2048>, dim3((unsigned)rows), dim3(TK_THREADS), 0, st, scores, lds, ids,
                           ldi, n, top_val, top_id, k, K, init);
    else
        hipLaunchKernelGGL(topk_merge_ids_kernel<4096>, dim3((unsigned)rows), dim3(TK_THREADS), 0, st, scores, lds, ids,
                           ldi, n, top_val, top_id, k, K, init);
    POLUS_CHECK_LAUNCH("polus_topk_merge_ids");
    return POLUS_OK;
}
