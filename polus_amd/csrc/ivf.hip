// Inverted centroid lists and probed candidate generation for a token index (polus_amd/ir/search.py refresh_lists,
// probe, search_pruned(nprobe=...)): the first step of PLAID.  include/polus_hip.h has the contracts in full.
//
//   lists     offsets int32 [K + 1], docs int32 [P]: docs[offsets[c] .. offsets[c + 1]) = the documents holding a present
//             token coded c, each once.  Built by count -> offsets -> fill over the index's uint16 codes [N, Ld]; a code
//             >= K (0xFFFF among them) is no token, as in centroid.hip.
//   mark      the union of the probed lists of a query as a bitmap row, uint32 [ceil(N / 32)].
//   compact   a bitmap row as ascending ids (or only their number).
// polus_centroid_scores_ids (centroid.hip) then scores the ids.
//
// Shapes and limits (refused before any launch): 1 <= Ld <= 512, 1 <= K <= 65535, N >= 1, B >= 1, 1 <= Lq <= 512,
// 1 <= nprobe <= 1024, 0 <= P < 2^31 (polus_ivf_offsets reports a larger P as offsets[K] = -1), row strides at least
// the row.
//
// Determinism.  Everything is integer arithmetic: counts, offsets, P, the lists as sets, the bitmap and the compacted
// ids are exact and the same from run to run.  The ORDER of the ids inside one list is not: a document takes the slot
// an atomic cursor hands it, so it follows the scheduling.  That is harmless because a list is only ever OR-ed into a
// bitmap, and it saves a sort at build time.
//
// Ownership.  The caller owns every buffer, `cursor` included (scratch of polus_ivf_fill, meaningless afterwards); the
// entry points zero what they accumulate into (counts, cursor, the bitmap rows) themselves, on the caller's stream.
//
// Bounds.  A probe outside [0, K) is skipped before anything is indexed with it; a list position outside [0, P) is
// never read; a list entry outside [0, N) is never written through; fill stores only inside its centroid's range and
// below P.  Lists that belong to other codes or another corpus give wrong candidates, not faults.
//
// count / fill: one wave per document (4 per workgroup, grid-stride).  The wave copies the document's codes to LDS and
// notes where its last present token sits; lane l then owns tokens l, l + 64, ... and a token "counts" iff no earlier
// token of the document has its code (the earlier codes are read one per step, every lane the same LDS address: a
// broadcast).  Ld (Ld / 64 + 1) / 2 steps per document at worst, no sort, and the documents' first tokens are what the
// atomics see: one int32 add per (document, distinct centroid), as bm25.hip does for document frequencies.
// offsets: one workgroup, each thread a contiguous run of counters, sums in 64 bits.
// mark: grid (G, B).  The G workgroups of a query walk its Lq * nprobe probes 256 at a time: a thread loads one probe's
// (start, length), a workgroup scan turns the lengths into a prefix in LDS, and the tile's W list entries are split
// evenly, workgroup g taking entries [W g / G, W (g + 1) / G) 256 at a time (consecutive threads read consecutive
// entries of docs; a binary search over the prefix names an entry's list).  So the work is dealt out by list entries:
// one centroid holding most of the corpus is spread over all G workgroups.  A bit already seen set is not OR-ed again
// (a stale read only costs a redundant atomic).
// compact: one workgroup per row, 256 words per step: popcount, workgroup scan, and each thread writes the positions of
// its word's bits behind the running total: ascending without atomics.
#include <algorithm>
#include <limits.h>

#include "common.h"

namespace {

constexpr int IVF_THREADS = 256;
constexpr int IVF_WAVES = IVF_THREADS / 64;
constexpr int IVF_LMAX = 512;                      // document tokens, as for the other centroid kernels
constexpr int IVF_KMAX = 65535;                    // 0xFFFF is "no token"
constexpr int IVF_NPROBE_MAX = 1024;               // what polus_topk_merge can keep
constexpr int IVF_MAX_BLOCKS = 4096;
constexpr int IVF_OFF_THREADS = 1024;
typedef unsigned long long u64;

// The exclusive prefix of v over the workgroup's threads, in thread order, and the sum of all in *total.  Every thread
// calls it; s_w holds one entry per wave; ends on a barrier, so s_w may be used again at once.
__device__ __forceinline__ u64 ivf_block_scan(u64 v, u64* s_w, u64* total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
    u64 inc = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const u64 t = __shfl_up(inc, o, 64);
        if (lane >= o) inc += t;
    }
    if (lane == 63) s_w[wave] = inc;
    __syncthreads();
    u64 base = 0, tot = 0;
    for (int w = 0; w < nw; ++w) {
        const u64 t = s_w[w];
        if (w < wave) base += t;
        tot += t;
    }
    __syncthreads();
    *total = tot;
    return base + inc - v;
}

// p[r * ld + c] = v for r < rows, c < cols.
__global__ __launch_bounds__(IVF_THREADS) void ivf_set_kernel(int32_t* __restrict__ p, long ld, int rows, int cols, int32_t v) {
    for (int r = blockIdx.y; r < rows; r += gridDim.y)
        for (long c = (long)blockIdx.x * IVF_THREADS + threadIdx.x; c < cols; c += (long)gridDim.x * IVF_THREADS)
            p[(size_t)r * ld + c] = v;
}

int ivf_set(const char* what, int32_t* p, long ld, int rows, int cols, int32_t v, hipStream_t st) {
    const long want = ((long)cols + IVF_THREADS - 1) / IVF_THREADS;
    dim3 grid((unsigned)std::min(want, 1024L), (unsigned)std::min(rows, 65535));
    hipLaunchKernelGGL(ivf_set_kernel, grid, dim3(IVF_THREADS), 0, st, p, ld, rows, cols, v);
    POLUS_CHECK_LAUNCH(what);
    return POLUS_OK;
}

// FILL = false: acc = counts.  FILL = true: acc = the cursors, and the document id goes to its centroid's list.
template <bool FILL>
__global__ __launch_bounds__(IVF_THREADS) void ivf_lists_kernel(const uint16_t* __restrict__ codes, int N, int Ld, int K,
                                                                int32_t* __restrict__ acc,
                                                                const int32_t* __restrict__ offsets, int P,
                                                                int32_t* __restrict__ docs) {
    __shared__ uint16_t s_codes[IVF_WAVES][IVF_LMAX];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint16_t* sc = s_codes[wave];
    for (long n0 = (long)blockIdx.x * IVF_WAVES; n0 < N; n0 += (long)gridDim.x * IVF_WAVES) {     // uniform: barriers inside
        const long n = n0 + wave;
        const bool live = n < N;
        const uint16_t* cn = codes + (size_t)(live ? n : 0) * Ld;
        int last = 0;                                         // one past the document's last present token
        for (int j0 = 0; j0 < Ld; j0 += 64) {
            const int j = j0 + lane;
            const int cv = (live && j < Ld) ? (int)cn[j] : 0xFFFF;
            if (j < Ld) sc[j] = (uint16_t)cv;
            const u64 pres = __ballot(cv < K);
            if (pres) last = j0 + 64 - __builtin_clzll(pres);
        }
        __syncthreads();
        for (int j0 = 0; j0 < last; j0 += 64) {               // uniform per wave; no barrier inside
            const int j = j0 + lane;
            const int c = j < last ? (int)sc[j] : 0xFFFF;
            bool first = c < K;
            const int stop = min(j0 + 64, last);
            for (int e = 0; e < stop; ++e) first = first && !(e < j && (int)sc[e] == c);
            if (first) {                                      // c < K: acc[c], offsets[c] and offsets[c + 1] exist
                const int slot = atomicAdd(&acc[c], 1);
                if constexpr (FILL) {
                    const long at = (long)offsets[c] + slot;
                    if (slot >= 0 && at >= 0 && at < (long)offsets[c + 1] && at < (long)P) docs[at] = (int32_t)n;
                }
            }
        }
        __syncthreads();                                      // the next document rewrites sc
    }
}

__global__ __launch_bounds__(IVF_OFF_THREADS) void ivf_offsets_kernel(const int32_t* __restrict__ counts, int K,
                                                                      int32_t* __restrict__ offsets) {
    __shared__ u64 s_w[IVF_OFF_THREADS / 64];
    const int per = (K + IVF_OFF_THREADS - 1) / IVF_OFF_THREADS;
    const int k0 = min(K, (int)threadIdx.x * per), k1 = min(K, k0 + per);
    u64 sum = 0;
    for (int k = k0; k < k1; ++k) sum += (u64)max(counts[k], 0);
    u64 total;
    u64 run = ivf_block_scan(sum, s_w, &total);
    for (int k = k0; k < k1; ++k) {
        offsets[k] = (int32_t)run;                            // unspecified when the total does not fit
        run += (u64)max(counts[k], 0);
    }
    if (threadIdx.x == 0) offsets[K] = total <= (u64)INT_MAX ? (int32_t)total : -1;
}

__global__ __launch_bounds__(IVF_THREADS) void ivf_mark_kernel(const int32_t* __restrict__ probes, long ldp,
                                                               const int32_t* __restrict__ qmask,
                                                               const int32_t* __restrict__ offsets,
                                                               const int32_t* __restrict__ docs, int P, int K, int N,
                                                               uint32_t* bitmap, long ldb, int B, int Lq, int nprobe) {
    __shared__ u64 s_pre[IVF_THREADS];                        // the tile's list lengths, exclusive prefix
    __shared__ int s_start[IVF_THREADS];
    __shared__ u64 s_w[IVF_WAVES];
    const u64 G = gridDim.x, g = blockIdx.x;
    const long total = (long)Lq * nprobe;
    for (int b = blockIdx.y; b < B; b += gridDim.y) {
        uint32_t* row = bitmap + (size_t)b * ldb;
        for (long t0 = 0; t0 < total; t0 += IVF_THREADS) {    // uniform: barriers inside
            const long t = t0 + threadIdx.x;
            int start = 0, len = 0;
            if (t < total) {
                const int i = (int)(t / nprobe), p = (int)(t - (long)i * nprobe);
                if (!qmask || qmask[(size_t)b * Lq + i] != 0) {
                    const int c = probes[((size_t)b * Lq + i) * ldp + p];
                    if (c >= 0 && c < K) {
                        const int a = offsets[c], e = min(offsets[c + 1], P);
                        if (a >= 0 && e > a) { start = a; len = e - a; }      // [a, e) lies inside [0, P)
                    }
                }
            }
            u64 W;
            const u64 pre = ivf_block_scan((u64)len, s_w, &W);
            s_pre[threadIdx.x] = pre;
            s_start[threadIdx.x] = start;
            __syncthreads();
            const u64 lo = W * g / G, hi = W * (g + 1) / G;   // W < 2^39, G <= 2^8
            for (u64 w = lo + threadIdx.x; w < hi; w += IVF_THREADS) {
                int a = 0, z = IVF_THREADS - 1;               // the last list of the tile whose prefix is <= w: its length is > 0
                while (a < z) {
                    const int mid = (a + z + 1) >> 1;
                    if (s_pre[mid] <= w) a = mid; else z = mid - 1;
                }
                const int d = docs[(long)s_start[a] + (long)(w - s_pre[a])];
                if (d >= 0 && d < N) {
                    uint32_t* wd = row + (d >> 5);
                    const uint32_t bit = 1u << (d & 31);
                    if (!(*wd & bit)) atomicOr(wd, bit);
                }
            }
            __syncthreads();                                  // the next tile rewrites s_pre and s_start
        }
    }
}

__global__ __launch_bounds__(IVF_THREADS) void ivf_compact_kernel(const uint32_t* __restrict__ bitmap, long ldb, int B, int N,
                                                                  int32_t* __restrict__ cand, long ldc, int cap,
                                                                  int32_t* __restrict__ count) {
    __shared__ u64 s_w[IVF_WAVES];
    const int W = (int)(((long)N + 31) >> 5);
    for (int b = blockIdx.x; b < B; b += gridDim.x) {
        const uint32_t* row = bitmap + (size_t)b * ldb;
        int32_t* out = cand ? cand + (size_t)b * ldc : nullptr;
        long base = 0;                                        // set bits in the words before this step
        for (long w0 = 0; w0 < W; w0 += IVF_THREADS) {        // uniform: barriers inside
            const long w = w0 + threadIdx.x;
            uint32_t v = w < W ? row[w] : 0u;
            if (w == W - 1 && (N & 31)) v &= (1u << (N & 31)) - 1u;
            u64 step;
            long at = base + (long)ivf_block_scan((u64)__popc(v), s_w, &step);
            if (out)
                while (v && at < cap) {
                    out[at++] = (int32_t)((w << 5) + __builtin_ctz(v));
                    v &= v - 1;
                }
            base += (long)step;
        }
        if (threadIdx.x == 0) count[b] = (int32_t)base;       // <= N
        if (out)
            for (long c = base + threadIdx.x; c < cap; c += IVF_THREADS) out[c] = -1;
    }
}

int ivf_check_codes(const char* what, int N, int Ld, int K) {
    POLUS_REQUIRE(N >= 1, "%s: need N >= 1 (got %d)", what, N);
    POLUS_REQUIRE(Ld >= 1 && Ld <= IVF_LMAX, "%s: need 1 <= Ld <= %d (got %d)", what, IVF_LMAX, Ld);
    POLUS_REQUIRE(K >= 1 && K <= IVF_KMAX, "%s: need 1 <= K <= %d (got %d)", what, IVF_KMAX, K);
    return POLUS_OK;
}

unsigned ivf_doc_blocks(int N) {
    return (unsigned)std::min(((long)N + IVF_WAVES - 1) / IVF_WAVES, (long)IVF_MAX_BLOCKS);
}

}  // namespace

extern "C" int polus_ivf_count(const uint16_t* codes, int N, int Ld, int K, int32_t* counts, void* stream) {
    const char* what = "polus_ivf_count";
    if (int rc = ivf_check_codes(what, N, Ld, K)) return rc;
    POLUS_REQUIRE(codes && counts, "%s: null pointer", what);
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (int rc = ivf_set(what, counts, K, 1, K, 0, st)) return rc;
    hipLaunchKernelGGL(ivf_lists_kernel<false>, dim3(ivf_doc_blocks(N)), dim3(IVF_THREADS), 0, st, codes, N, Ld, K, counts,
                       (const int32_t*)nullptr, 0, (int32_t*)nullptr);
    POLUS_CHECK_LAUNCH(what);
    return POLUS_OK;
}

extern "C" int polus_ivf_offsets(const int32_t* counts, int K, int32_t* offsets, void* stream) {
    const char* what = "polus_ivf_offsets";
    POLUS_REQUIRE(K >= 1 && K <= IVF_KMAX, "%s: need 1 <= K <= %d (got %d)", what, IVF_KMAX, K);
    POLUS_REQUIRE(counts && offsets, "%s: null pointer", what);
    hipLaunchKernelGGL(ivf_offsets_kernel, dim3(1), dim3(IVF_OFF_THREADS), 0, static_cast<hipStream_t>(stream), counts, K,
                       offsets);
    POLUS_CHECK_LAUNCH(what);
    return POLUS_OK;
}

extern "C" int polus_ivf_fill(const uint16_t* codes, int N, int Ld, int K, const int32_t* offsets, int P, int32_t* cursor,
                              int32_t* docs, void* stream) {
    const char* what = "polus_ivf_fill";
    if (int rc = ivf_check_codes(what, N, Ld, K)) return rc;
    POLUS_REQUIRE(P >= 0, "%s: need 0 <= P < 2^31, the pairs polus_ivf_offsets counted (got %d)", what, P);
    POLUS_REQUIRE(codes && offsets && cursor && (docs || P == 0), "%s: null pointer", what);
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (int rc = ivf_set(what, cursor, K, 1, K, 0, st)) return rc;
    if (P == 0) return POLUS_OK;
    hipLaunchKernelGGL(ivf_lists_kernel<true>, dim3(ivf_doc_blocks(N)), dim3(IVF_THREADS), 0, st, codes, N, Ld, K, cursor,
                       offsets, P, docs);
    POLUS_CHECK_LAUNCH(what);
    return POLUS_OK;
}

extern "C" int polus_ivf_mark(const int32_t* probes, long ldp, const int32_t* qmask, const int32_t* offsets,
                              const int32_t* docs, int P, int K, int N, uint32_t* bitmap, long ldb, int B, int Lq, int nprobe,
                              void* stream) {
    const char* what = "polus_ivf_mark";
    POLUS_REQUIRE(K >= 1 && K <= IVF_KMAX, "%s: need 1 <= K <= %d (got %d)", what, IVF_KMAX, K);
    POLUS_REQUIRE(N >= 1 && B >= 1, "%s: need N >= 1 and B >= 1 (got %d, %d)", what, N, B);
    POLUS_REQUIRE(Lq >= 1 && Lq <= IVF_LMAX, "%s: need 1 <= Lq <= %d (got %d)", what, IVF_LMAX, Lq);
    POLUS_REQUIRE(nprobe >= 1 && nprobe <= IVF_NPROBE_MAX, "%s: need 1 <= nprobe <= %d (got %d)", what, IVF_NPROBE_MAX, nprobe);
    POLUS_REQUIRE(P >= 0, "%s: need 0 <= P < 2^31 (got %d)", what, P);
    const long W = ((long)N + 31) >> 5;
    POLUS_REQUIRE(ldp >= nprobe, "%s: probe row stride ldp must be >= nprobe (got %ld < %d)", what, ldp, nprobe);
    POLUS_REQUIRE(ldb >= W, "%s: bitmap row stride ldb must be >= ceil(N/32) words (got %ld < %ld)", what, ldb, W);
    POLUS_REQUIRE(probes && offsets && bitmap && (docs || P == 0), "%s: null pointer", what);
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (int rc = ivf_set(what, reinterpret_cast<int32_t*>(bitmap), ldb, B, (int)W, 0, st)) return rc;
    const int rows = std::min(B, 65535);
    const int G = std::max(1, std::min(256, 4 * polus_num_cus() / rows));
    hipLaunchKernelGGL(ivf_mark_kernel, dim3((unsigned)G, (unsigned)rows), dim3(IVF_THREADS), 0, st, probes, ldp, qmask, offsets,
                       docs, P, K, N, bitmap, ldb, B, Lq, nprobe);
    POLUS_CHECK_LAUNCH(what);
    return POLUS_OK;
}

extern "C" int polus_ivf_compact(const uint32_t* bitmap, long ldb, int B, int N, int32_t* cand, long ldc, int cap,
                                 int32_t* count, void* stream) {
    const char* what = "polus_ivf_compact";
    POLUS_REQUIRE(N >= 1 && B >= 1, "%s: need N >= 1 and B >= 1 (got %d, %d)", what, N, B);
    const long W = ((long)N + 31) >> 5;
    POLUS_REQUIRE(ldb >= W, "%s: bitmap row stride ldb must be >= ceil(N/32) words (got %ld < %ld)", what, ldb, W);
    POLUS_REQUIRE(!cand || cap >= 1, "%s: need cap >= 1 with cand (got %d)", what, cap);
    POLUS_REQUIRE(!cand || ldc >= cap, "%s: candidate row stride ldc must be >= cap (got %ld < %d)", what, ldc, cap);
    POLUS_REQUIRE(bitmap && count, "%s: null pointer", what);
    hipLaunchKernelGGL(ivf_compact_kernel, dim3((unsigned)std::min(B, IVF_MAX_BLOCKS)), dim3(IVF_THREADS), 0,
                       static_cast<hipStream_t>(stream), bitmap, ldb, B, N, cand, ldc, cand ? cap : 0, count);
    POLUS_CHECK_LAUNCH(what);
    return POLUS_OK;
}
