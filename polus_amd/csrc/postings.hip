// Block-inverted postings and term-at-a-time search for the two lexical first stages (polus_amd/ir/postings.py, used by
// BM25Index and SparseCorpusIndex with postings=True).  include/polus_hip.h has the format and the contracts in full.
//
//   postings  the N documents in blocks of block_docs consecutive ids (a power of two in [64, 32768]); per block a CSR
//             over the V terms: offsets int32 [nblk, V + 1], base int64 [nblk + 1] (the exclusive scan of the block
//             totals, base[nblk] = P), post_doc uint16 [P] (the id local to the block), post_w f32 [P].  A forward slot
//             (id, w) is a posting iff 0 <= id < V and w != 0 (NaN counts, +-0.0 does not).  Built by count -> offsets ->
//             fill over the forward arrays ids / w [N, M].
//   queries   q_terms int32 / q_w f32 [Q, cap], q_count int32 [Q]: ascending term ids, then (-1, 0.0).  Made from a
//             dense row (compact_rows) or from polus_bm25_term_counts' query output (bm25_query_lists).
//   scores    one workgroup per (query, block): an f32 accumulator of block_docs entries in LDS, the query's entries in
//             order, each one's list spread over the threads, a barrier between terms.
//
// The score rule.  acc = +0.0f; for the entries j = 0 .. min(q_count, cap) - 1 in that order, skipping ids outside
// [0, V): acc = fl(acc + fl(q_w[j] * w)) where the document holds the term.  One rounding for the product, one for the
// sum, never an fma (the pragma below; __fmul_rn and __fadd_rn alone may be contracted).  The documents of one list
// are distinct, so within a term no two threads meet at an address, and the barrier orders the terms: the bits depend
// neither on the order inside a list nor on the grid.  There are no floating-point atomics in this file.
//
// Determinism.  counts, offsets, base and the lists as SETS are exact (integer arithmetic); the ORDER inside a list
// follows the atomic cursor and is unspecified, as in ivf.hip.
//
// Ownership.  The caller owns every buffer, `cursor` included; the entry points zero what they accumulate into (counts,
// cursor) themselves, on the caller's stream.
//
// Bounds.  fill stores only inside its own list and below P.  scores clamps every list to [0, P) before reading it and
// drops a local id that is not a document of its block, so stale or foreign postings give wrong scores, not faults, and
// nothing outside the N columns of a score row is written.
//
// count / fill: one thread per forward slot (grid-stride, consecutive threads read consecutive slots), one int32 add
// per posting into counts / cursor [nblk, V].  A term every document holds takes block_docs adds on one address per
// block; tools/postings_bench.py records what that costs.
// offsets: one workgroup per block scans its V counters (each thread a contiguous run, 64-bit sums), then one
// workgroup scans the nblk totals into base.
// compact_rows: one workgroup per row, 256 columns per step: __ballot and a popcount give a lane its place in the wave,
// four wave totals through LDS its place in the step: ascending without atomics.
// bm25_query_lists: one workgroup per row; the row's ids go to LDS and an entry's place is the number of smaller ids.
#include <algorithm>
#include <limits.h>

#include "common.h"

namespace {

constexpr int PS_THREADS = 256;
constexpr int PS_WAVES = PS_THREADS / 64;
constexpr int PS_MAX_BLOCKS = 8192;
constexpr int PS_SCAN_THREADS = 1024;
constexpr int PS_SCORE_THREADS = 512;
constexpr int PS_MIN_BLOCK_DOCS = 64;
constexpr int PS_MAX_BLOCK_DOCS = 32768;           // 128 KiB of f32 accumulators, of the 160 KiB of a CU
constexpr int PS_MAXM = 1024;                      // slots per row, as everywhere in the lexical path
typedef unsigned long long u64;

__global__ __launch_bounds__(PS_THREADS) void ps_zero_kernel(int32_t* __restrict__ p, long n) {
    for (long i = (long)blockIdx.x * PS_THREADS + threadIdx.x; i < n; i += (long)gridDim.x * PS_THREADS) p[i] = 0;
}

int ps_zero(const char* what, int32_t* p, long n, hipStream_t st) {
    const long want = (n + PS_THREADS - 1) / PS_THREADS;
    hipLaunchKernelGGL(ps_zero_kernel, dim3((unsigned)std::max(1L, std::min(want, (long)PS_MAX_BLOCKS))), dim3(PS_THREADS), 0,
                       st, p, n);
    POLUS_CHECK_LAUNCH(what);
    return POLUS_OK;
}

// FILL = false: acc = counts.  FILL = true: acc = the cursors, and the posting goes to its list.
template <bool FILL>
__global__ __launch_bounds__(PS_THREADS) void ps_walk_kernel(const int32_t* __restrict__ ids, long ldi,
                                                             const float* __restrict__ w, long ldw, int N, int M, int V,
                                                             int shift, int32_t* __restrict__ acc,
                                                             const int32_t* __restrict__ offsets,
                                                             const int64_t* __restrict__ base, long P,
                                                             uint16_t* __restrict__ post_doc, float* __restrict__ post_w) {
    const long total = (long)N * M;
    for (long i = (long)blockIdx.x * PS_THREADS + threadIdx.x; i < total; i += (long)gridDim.x * PS_THREADS) {
        const long d = i / M;
        const int m = (int)(i - d * M);
        const int t = ids[(size_t)d * ldi + m];
        if (t < 0 || t >= V) continue;
        const float x = w[(size_t)d * ldw + m];
        if (!(x != 0.0f)) continue;                           // +-0.0 is no posting, NaN is one
        const long b = d >> shift;
        const int slot = atomicAdd(&acc[(size_t)b * V + t], 1);
        if constexpr (FILL) {
            const int32_t* off = offsets + (size_t)b * ((size_t)V + 1);
            const long in = (long)off[t] + slot;              // the position inside the block
            const long at = (long)base[b] + in;
            if (slot >= 0 && in >= 0 && in < (long)off[t + 1] && at >= 0 && at < P) {
                post_doc[at] = (uint16_t)(d - (b << shift));
                post_w[at] = x;
            }
        }
    }
}

// The exclusive prefix of v over the workgroup's threads, in thread order, and the sum of all in *total.  Every thread
// calls it; s_w holds one entry per wave; ends on a barrier.
__device__ __forceinline__ u64 ps_block_scan(u64 v, u64* s_w, u64* total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
    u64 inc = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const u64 t = __shfl_up(inc, o, 64);
        if (lane >= o) inc += t;
    }
    if (lane == 63) s_w[wave] = inc;
    __syncthreads();
    u64 before = 0, tot = 0;
    for (int x = 0; x < nw; ++x) {
        const u64 t = s_w[x];
        if (x < wave) before += t;
        tot += t;
    }
    __syncthreads();
    *total = tot;
    return before + inc - v;
}

// One workgroup per block: offsets[b, 0 .. V] = the exclusive scan of counts[b, 0 .. V).
__global__ __launch_bounds__(PS_SCAN_THREADS) void ps_offsets_kernel(const int32_t* __restrict__ counts, int nblk, int V,
                                                                     int32_t* __restrict__ offsets) {
    __shared__ u64 s_w[PS_SCAN_THREADS / 64];
    const int per = (V + PS_SCAN_THREADS - 1) / PS_SCAN_THREADS;
    const int k0 = (int)std::min((long)V, (long)threadIdx.x * per), k1 = (int)std::min((long)V, (long)k0 + per);
    for (int b = blockIdx.x; b < nblk; b += gridDim.x) {      // uniform: barriers inside
        const int32_t* c = counts + (size_t)b * V;
        int32_t* o = offsets + (size_t)b * ((size_t)V + 1);
        u64 sum = 0;
        for (int k = k0; k < k1; ++k) sum += (u64)max(c[k], 0);
        u64 total;
        u64 run = ps_block_scan(sum, s_w, &total);
        for (int k = k0; k < k1; ++k) {
            o[k] = (int32_t)std::min(run, (u64)INT_MAX);      // true counts stay below 2^25; anything else is clamped
            run += (u64)max(c[k], 0);
        }
        if (threadIdx.x == 0) o[V] = (int32_t)std::min(total, (u64)INT_MAX);
    }
}

// One workgroup: base[0 .. nblk] = the exclusive scan of the block totals offsets[b, V], in 64 bits.
__global__ __launch_bounds__(PS_SCAN_THREADS) void ps_base_kernel(const int32_t* __restrict__ offsets, int nblk, int V,
                                                                  int64_t* __restrict__ base) {
    __shared__ u64 s_w[PS_SCAN_THREADS / 64];
    const int per = (nblk + PS_SCAN_THREADS - 1) / PS_SCAN_THREADS;
    const int b0 = (int)std::min((long)nblk, (long)threadIdx.x * per), b1 = (int)std::min((long)nblk, (long)b0 + per);
    const size_t ld = (size_t)V + 1;
    u64 sum = 0;
    for (int b = b0; b < b1; ++b) sum += (u64)max(offsets[(size_t)b * ld + V], 0);
    u64 total;
    u64 run = ps_block_scan(sum, s_w, &total);
    for (int b = b0; b < b1; ++b) {
        base[b] = (int64_t)run;
        run += (u64)max(offsets[(size_t)b * ld + V], 0);
    }
    if (threadIdx.x == 0) base[nblk] = (int64_t)total;
}

__global__ __launch_bounds__(PS_THREADS) void ps_compact_kernel(const float* __restrict__ q, long ldq, int Q, int V, int cap,
                                                                int32_t* __restrict__ q_terms, long ldt,
                                                                float* __restrict__ q_w, long ldw,
                                                                int32_t* __restrict__ q_count) {
    __shared__ int s_w[PS_WAVES];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const u64 below = (1ull << lane) - 1ull;
    for (int r = blockIdx.x; r < Q; r += gridDim.x) {         // uniform: barriers inside
        const float* row = q + (size_t)r * ldq;
        int32_t* ot = q_terms + (size_t)r * ldt;
        float* ow = q_w + (size_t)r * ldw;
        long kept_before = 0;                                 // kept entries in the columns before this step
        for (long v0 = 0; v0 < V; v0 += PS_THREADS) {
            const long v = v0 + threadIdx.x;
            const float x = v < V ? row[v] : 0.0f;
            const bool keep = x != 0.0f;                      // NaN is kept, +-0.0 is not
            const u64 bal = __ballot(keep);
            if (lane == 0) s_w[wave] = __popcll(bal);
            __syncthreads();
            int before = 0, step = 0;
            for (int x2 = 0; x2 < PS_WAVES; ++x2) {
                const int c = s_w[x2];
                if (x2 < wave) before += c;
                step += c;
            }
            __syncthreads();                                  // s_w is rewritten by the next step
            const long at = kept_before + before + __popcll(bal & below);
            if (keep && at < cap) {
                ot[at] = (int32_t)v;
                ow[at] = x;
            }
            kept_before += step;
        }
        if (threadIdx.x == 0) q_count[r] = (int32_t)kept_before;       // <= V
        for (long c = kept_before + threadIdx.x; c < cap; c += PS_THREADS) {
            ot[c] = -1;
            ow[c] = 0.0f;
        }
    }
}

__global__ __launch_bounds__(PS_THREADS) void ps_query_lists_kernel(const int32_t* __restrict__ terms, long ldt,
                                                                    const int32_t* __restrict__ tf, long ldf,
                                                                    const float* __restrict__ idf, int Q, int M, int V,
                                                                    int32_t* __restrict__ q_terms, long ldt2,
                                                                    float* __restrict__ q_w, long ldw,
                                                                    int32_t* __restrict__ q_count) {
    __shared__ int s_t[PS_MAXM];
    __shared__ int s_n;
    for (int r = blockIdx.x; r < Q; r += gridDim.x) {         // uniform: barriers inside
        const int32_t* rt = terms + (size_t)r * ldt;
        const int32_t* rf = tf + (size_t)r * ldf;
        int32_t* ot = q_terms + (size_t)r * ldt2;
        float* ow = q_w + (size_t)r * ldw;
        if (threadIdx.x == 0) s_n = 0;
        for (int m = threadIdx.x; m < M; m += PS_THREADS) {
            const int t = rt[m];
            s_t[m] = (t >= 0 && t < V) ? t : -1;
        }
        __syncthreads();
        int mine = 0;
        for (int m = threadIdx.x; m < M; m += PS_THREADS) {
            const int t = s_t[m];
            if (t < 0) continue;
            int rank = 0;                                     // the kept entries ordered before (t, m): a permutation
            for (int e = 0; e < M; ++e) {                     // even when the precondition (distinct ids) is broken
                const int o = s_t[e];
                rank += (o >= 0 && (o < t || (o == t && e < m))) ? 1 : 0;
            }
            ot[rank] = t;                                     // rank < the number of kept entries <= M
            ow[rank] = (float)rf[m] * idf[t];
            ++mine;
        }
        if (mine) atomicAdd(&s_n, mine);
        __syncthreads();
        const int n = s_n;
        if (threadIdx.x == 0) q_count[r] = n;
        for (int c = n + threadIdx.x; c < M; c += PS_THREADS) {
            ot[c] = -1;
            ow[c] = 0.0f;
        }
        __syncthreads();                                      // s_t and s_n are rewritten by the next row
    }
}

// grid = Q * nblk_launch: workgroup x is query x / nblk_launch and block blk0 + x % nblk_launch.
__global__ __launch_bounds__(PS_SCORE_THREADS) void ps_scores_kernel(
        const int32_t* __restrict__ q_terms, long ldt, const float* __restrict__ q_w, long ldw,
        const int32_t* __restrict__ q_count, int cap, const int32_t* __restrict__ offsets, const int64_t* __restrict__ base,
        const uint16_t* __restrict__ post_doc, const float* __restrict__ post_w, long P, int V, int block_docs, int blk0,
        int nblk_launch, int N, float* __restrict__ score, long lds) {
#pragma clang fp contract(off)
    extern __shared__ float ps_acc[];                         // block_docs entries
    const int q = blockIdx.x / nblk_launch, bl = blockIdx.x - q * nblk_launch;
    const long b = (long)blk0 + bl;
    const long left = (long)N - b * block_docs;               // >= 1: the host checked the block range
    const int docs = (int)std::min((long)block_docs, left);
    for (int i = threadIdx.x; i < block_docs; i += PS_SCORE_THREADS) ps_acc[i] = 0.0f;
    __syncthreads();
    const int32_t* off = offsets + (size_t)b * ((size_t)V + 1);
    const long start = (long)base[b];
    const int32_t* qt = q_terms + (size_t)q * ldt;
    const float* qw = q_w + (size_t)q * ldw;
    const int cnt = std::min(std::max(q_count[q], 0), cap);
    for (int j = 0; j < cnt; ++j) {                           // everything that decides a `continue` is uniform
        const int t = qt[j];
        if (t < 0 || t >= V) continue;
        const long lo = std::max(start + (long)off[t], 0L), hi = std::min(start + (long)off[t + 1], P);
        if (hi <= lo) continue;                               // an empty list: no store, no barrier needed
        const float x = qw[j];
        for (long p = lo + threadIdx.x; p < hi; p += PS_SCORE_THREADS) {
            const int d = (int)post_doc[p];
            if (d < docs) {
                const float prod = x * post_w[p];
                ps_acc[d] = ps_acc[d] + prod;
            }
        }
        __syncthreads();                                      // the next term may meet the same documents
    }
    float* out = score + (size_t)q * lds + (size_t)bl * block_docs;
    for (int i = threadIdx.x; i < docs; i += PS_SCORE_THREADS) out[i] = ps_acc[i];
}

// block_docs is a power of two in [64, 32768]: its log2, or -1.
int ps_shift(int block_docs) {
    if (block_docs < PS_MIN_BLOCK_DOCS || block_docs > PS_MAX_BLOCK_DOCS || (block_docs & (block_docs - 1))) return -1;
    int s = 0;
    while ((1 << s) < block_docs) ++s;
    return s;
}

int ps_check_forward(const char* what, int N, int M, int V, int block_docs, long ldi, long ldw) {
    POLUS_REQUIRE(N >= 1 && V >= 1 && V < INT_MAX, "%s: need N >= 1 and 1 <= V < 2^31 - 1 (got %d, %d)", what, N, V);
    POLUS_REQUIRE(M >= 1 && M <= PS_MAXM, "%s: need 1 <= M <= %d (got %d)", what, PS_MAXM, M);
    POLUS_REQUIRE(ps_shift(block_docs) >= 0, "%s: block_docs must be a power of two in [%d, %d] (got %d)", what,
                  PS_MIN_BLOCK_DOCS, PS_MAX_BLOCK_DOCS, block_docs);
    POLUS_REQUIRE(ldi >= M && ldw >= M, "%s: row strides ldi, ldw must be >= M (got %ld, %ld < %d)", what, ldi, ldw, M);
    return POLUS_OK;
}

unsigned ps_walk_blocks(int N, int M) {
    const long want = ((long)N * M + PS_THREADS - 1) / PS_THREADS;
    return (unsigned)std::min(want, (long)PS_MAX_BLOCKS);
}

}  // namespace

extern "C" int polus_postings_count(const int32_t* ids, long ldi, const float* w, long ldw, int N, int M, int V,
                                    int block_docs, int32_t* counts, void* stream) {
    const char* what = "polus_postings_count";
    if (int rc = ps_check_forward(what, N, M, V, block_docs, ldi, ldw)) return rc;
    POLUS_REQUIRE(ids && w && counts, "%s: null pointer", what);
    const int shift = ps_shift(block_docs);
    const long nblk = ((long)N + block_docs - 1) >> shift;
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (int rc = ps_zero(what, counts, nblk * V, st)) return rc;
    hipLaunchKernelGGL(ps_walk_kernel<false>, dim3(ps_walk_blocks(N, M)), dim3(PS_THREADS), 0, st, ids, ldi, w, ldw, N, M, V,
                       shift, counts, (const int32_t*)nullptr, (const int64_t*)nullptr, 0L, (uint16_t*)nullptr,
                       (float*)nullptr);
    POLUS_CHECK_LAUNCH(what);
    return POLUS_OK;
}

extern "C" int polus_postings_offsets(const int32_t* counts, int nblk, int V, int32_t* offsets, int64_t* base, void* stream) {
    const char* what = "polus_postings_offsets";
    POLUS_REQUIRE(nblk >= 1 && V >= 1 && V < INT_MAX, "%s: need nblk >= 1 and 1 <= V < 2^31 - 1 (got %d, %d)", what, nblk, V);
    POLUS_REQUIRE(counts && offsets && base, "%s: null pointer", what);
    hipStream_t st = static_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(ps_offsets_kernel, dim3((unsigned)std::min(nblk, PS_MAX_BLOCKS)), dim3(PS_SCAN_THREADS), 0, st, counts,
                       nblk, V, offsets);
    POLUS_CHECK_LAUNCH(what);
    hipLaunchKernelGGL(ps_base_kernel, dim3(1), dim3(PS_SCAN_THREADS), 0, st, (const int32_t*)offsets, nblk, V, base);
    POLUS_CHECK_LAUNCH(what);
    return POLUS_OK;
}

extern "C" int polus_postings_fill(const int32_t* ids, long ldi, const float* w, long ldw, int N, int M, int V,
                                   int block_docs, const int32_t* offsets, const int64_t* base, long P, int32_t* cursor,
                                   uint16_t* post_doc, float* post_w, void* stream) {
    const char* what = "polus_postings_fill";
    if (int rc = ps_check_forward(what, N, M, V, block_docs, ldi, ldw)) return rc;
    POLUS_REQUIRE(P >= 0, "%s: need P >= 0, the postings polus_postings_offsets counted (got %ld)", what, P);
    POLUS_REQUIRE(ids && w && offsets && base && cursor && ((post_doc && post_w) || P == 0), "%s: null pointer", what);
    const int shift = ps_shift(block_docs);
    const long nblk = ((long)N + block_docs - 1) >> shift;
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (int rc = ps_zero(what, cursor, nblk * V, st)) return rc;
    if (P == 0) return POLUS_OK;
    hipLaunchKernelGGL(ps_walk_kernel<true>, dim3(ps_walk_blocks(N, M)), dim3(PS_THREADS), 0, st, ids, ldi, w, ldw, N, M, V,
                       shift, cursor, offsets, base, P, post_doc, post_w);
    POLUS_CHECK_LAUNCH(what);
    return POLUS_OK;
}

extern "C" int polus_sparse_compact_rows(const float* q, long ldq, int Q, int V, int cap, int32_t* q_terms, long ldt,
                                         float* q_w, long ldw, int32_t* q_count, void* stream) {
    const char* what = "polus_sparse_compact_rows";
    POLUS_REQUIRE(Q >= 1 && V >= 1 && cap >= 1, "%s: need Q >= 1, V >= 1 and cap >= 1 (got %d, %d, %d)", what, Q, V, cap);
    POLUS_REQUIRE(ldq >= V, "%s: row stride ldq must be >= V (got %ld < %d)", what, ldq, V);
    POLUS_REQUIRE(ldt >= cap && ldw >= cap, "%s: row strides ldt, ldw must be >= cap (got %ld, %ld < %d)", what, ldt, ldw, cap);
    POLUS_REQUIRE(q && q_terms && q_w && q_count, "%s: null pointer", what);
    hipLaunchKernelGGL(ps_compact_kernel, dim3((unsigned)std::min(Q, PS_MAX_BLOCKS)), dim3(PS_THREADS), 0,
                       static_cast<hipStream_t>(stream), q, ldq, Q, V, cap, q_terms, ldt, q_w, ldw, q_count);
    POLUS_CHECK_LAUNCH(what);
    return POLUS_OK;
}

extern "C" int polus_bm25_query_lists(const int32_t* terms, long ldt, const int32_t* tf, long ldf, const float* idf, int Q,
                                      int M, int V, int32_t* q_terms, long ldt2, float* q_w, long ldw, int32_t* q_count,
                                      void* stream) {
    const char* what = "polus_bm25_query_lists";
    POLUS_REQUIRE(Q >= 1 && V >= 1, "%s: need Q >= 1 and V >= 1 (got %d, %d)", what, Q, V);
    POLUS_REQUIRE(M >= 1 && M <= PS_MAXM, "%s: need 1 <= M <= %d (got %d)", what, PS_MAXM, M);
    POLUS_REQUIRE(ldt >= M && ldf >= M && ldt2 >= M && ldw >= M,
                  "%s: row strides ldt, ldf, ldt2, ldw must be >= M (got %ld, %ld, %ld, %ld < %d)", what, ldt, ldf, ldt2, ldw, M);
    POLUS_REQUIRE(terms && tf && idf && q_terms && q_w && q_count, "%s: null pointer", what);
    hipLaunchKernelGGL(ps_query_lists_kernel, dim3((unsigned)std::min(Q, PS_MAX_BLOCKS)), dim3(PS_THREADS), 0,
                       static_cast<hipStream_t>(stream), terms, ldt, tf, ldf, idf, Q, M, V, q_terms, ldt2, q_w, ldw, q_count);
    POLUS_CHECK_LAUNCH(what);
    return POLUS_OK;
}

extern "C" int polus_postings_scores(const int32_t* q_terms, long ldt, const float* q_w, long ldw, const int32_t* q_count,
                                     int cap, const int32_t* offsets, const int64_t* base, const uint16_t* post_doc,
                                     const float* post_w, long P, int V, int block_docs, int blk0, int nblk_launch, int N,
                                     float* score, long lds, int Q, void* stream) {
    const char* what = "polus_postings_scores";
    POLUS_REQUIRE(Q >= 1 && N >= 1 && V >= 1 && V < INT_MAX && cap >= 1,
                  "%s: need Q >= 1, N >= 1, 1 <= V < 2^31 - 1 and cap >= 1 (got %d, %d, %d, %d)", what, Q, N, V, cap);
    const int shift = ps_shift(block_docs);
    POLUS_REQUIRE(shift >= 0, "%s: block_docs must be a power of two in [%d, %d] (got %d)", what, PS_MIN_BLOCK_DOCS,
                  PS_MAX_BLOCK_DOCS, block_docs);
    const long nblk = ((long)N + block_docs - 1) >> shift;
    POLUS_REQUIRE(blk0 >= 0 && nblk_launch >= 1 && (long)blk0 + nblk_launch <= nblk,
                  "%s: blocks [%d, %d + %d) must lie inside the %ld blocks of N = %d", what, blk0, blk0, nblk_launch, nblk, N);
    POLUS_REQUIRE((long)Q * nblk_launch <= (long)INT_MAX, "%s: Q * nblk_launch must be < 2^31 (got %d * %d)", what, Q,
                  nblk_launch);
    POLUS_REQUIRE(P >= 0, "%s: need P >= 0 (got %ld)", what, P);
    POLUS_REQUIRE(ldt >= cap && ldw >= cap, "%s: row strides ldt, ldw must be >= cap (got %ld, %ld < %d)", what, ldt, ldw, cap);
    const long cols = std::min((long)nblk_launch << shift, (long)N - ((long)blk0 << shift));
    POLUS_REQUIRE(lds >= cols, "%s: score row stride lds must be >= the %ld documents of the launch (got %ld)", what, cols, lds);
    POLUS_REQUIRE(q_terms && q_w && q_count && offsets && base && score && ((post_doc && post_w) || P == 0),
                  "%s: null pointer", what);
    return polus_launch_lds<ps_scores_kernel>(what, dim3((unsigned)((long)Q * nblk_launch)), dim3(PS_SCORE_THREADS),
                                              (size_t)PS_MAX_BLOCK_DOCS * 4, (size_t)block_docs * 4,
                                              static_cast<hipStream_t>(stream), q_terms, ldt, q_w, ldw, q_count, cap, offsets,
                                              base, post_doc, post_w, P, V, block_docs, blk0, nblk_launch, N, score, lds);
}
