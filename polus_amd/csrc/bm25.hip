// BM25 over token ids (polus_amd/ir/lexical.py): per-document (term, count) lists and the corpus statistics, the
// saturated term weights, and the dense query rows polus_sparse_scores reads.
//
// The rules (include/polus_hip.h has them in full).  term_counts: the valid tokens of a row are those whose mask is
// non-zero, in order; the first `head` and last `tail` are dropped (pairs.hip's strip); an id outside [0, V) is
// dropped and counted; the distinct ids that remain go out ordered by (count descending, id ascending), the first M
// of them.  weights: w = tf (k1 + 1) / (tf + K_r), K_r = c1 len_r + c0, every operation rounded once.  query:
// q[b, t] = tf idf[t] on the row's terms, 0 elsewhere.
//
// term_counts is one workgroup per document (grid-stride over the documents).  A first sweep over the mask counts the
// valid tokens of every 64-column chunk (__ballot and a popcount, as in pairs.hip), which gives each token its rank
// among the valid ones; a second sweep writes every column's id, or a sentinel for a token that is masked, stripped or
// out of range, into LDS as a 64-bit key, and the keys are bitonic-sorted ascending (topk.hip's network; the stages
// with a stride below 64 exchange between lanes, see bm_sort_asc).  Equal ids are
// then neighbours: a position whose left neighbour differs is the head of a run, its count is the distance to the
// upper bound of its id (a binary search over the sorted keys), and the head becomes the key
// (0xFFFFFFFF - count) << 32 | id, everything else the sentinel.  A second ascending sort leaves the distinct terms in
// front in (count descending, id ascending) order.  LDS: 2048 keys = 16 KiB whatever V is; a histogram over the
// vocabulary would take 4 V bytes.  Global atomics: one int32 add into df per distinct term of a document, and three
// int64 adds into stats per WORKGROUP (the per-document terms are summed in a register first).  Integer sums: exact
// in any order, so the results are bitwise reproducible.
#include "common.h"

namespace {

constexpr int BM_THREADS = 256;
constexpr int BM_WAVES = BM_THREADS / 64;
constexpr int BM_MAXL = 2048;                      // the attention kernels' longest sequence
constexpr int BM_MAXM = 1024;                      // what polus_sparse_scores accepts
constexpr int BM_MAX_STRIP = 8;
constexpr int BM_MAX_BLOCKS = 2048;
constexpr int BM_PER = BM_MAXL / BM_THREADS;       // key positions per thread
constexpr int BM_MAX_V_BYTES = 163840;             // polus_sparse_scores' limit on a query row
typedef unsigned long long u64;
constexpr u64 BM_NONE = ~0ull;                     // sorts behind every real key

// One compare-exchange stage of the bitonic network between lanes: position i holds v, its partner i ^ stride (the
// same wave: stride < 64) holds the other key.  The lower position of a pair keeps the minimum in an ascending block
// ((i & size) == 0) and the maximum in a descending one.
__device__ __forceinline__ u64 bm_exchange(u64 v, int i, int size, int stride) {
    const u64 o = __shfl_xor(v, stride, 64);
    const bool keep_min = ((i & stride) == 0) == ((i & size) == 0);
    return keep_min ? (v < o ? v : o) : (v > o ? v : o);
}

// keys[0 .. m) ascending, m a power of two >= 64; every thread of the workgroup calls it; ends on a barrier.  The
// network is topk.hip's; the stages whose stride is below 64 pair positions of one wave and run on lane shuffles, a
// key per lane, without LDS traffic or a barrier between them: at m = 256 six barriers instead of 36.
__device__ __forceinline__ void bm_sort_asc(u64* keys, int m) {
    for (int i = threadIdx.x; i < m; i += BM_THREADS) {         // uniform per wave: m is a multiple of 64
        u64 v = keys[i];
        for (int size = 2; size <= 64; size <<= 1)
            for (int stride = size >> 1; stride > 0; stride >>= 1) v = bm_exchange(v, i, size, stride);
        keys[i] = v;
    }
    __syncthreads();
    for (int size = 128; size <= m; size <<= 1) {
        for (int stride = size >> 1; stride >= 64; stride >>= 1) {
            for (int t = threadIdx.x; t < (m >> 1); t += BM_THREADS) {
                const int i = 2 * t - (t & (stride - 1)), j = i + stride;   // j < m
                const u64 a = keys[i], b = keys[j];
                const bool asc = (i & size) == 0;
                if ((a > b) == asc) { keys[i] = b; keys[j] = a; }
            }
            __syncthreads();
        }
        for (int i = threadIdx.x; i < m; i += BM_THREADS) {
            u64 v = keys[i];
            for (int stride = 32; stride > 0; stride >>= 1) v = bm_exchange(v, i, size, stride);
            keys[i] = v;
        }
        __syncthreads();
    }
}

__global__ __launch_bounds__(BM_THREADS) void bm25_term_counts_kernel(
        const int32_t* __restrict__ ids, long ldi, const int32_t* __restrict__ mask, long ldm, int n, int L, int P, int V,
        int head, int tail, int32_t* __restrict__ terms, long ldt, int32_t* __restrict__ tf, long ldf, int M,
        int32_t* __restrict__ doc_len, int32_t* __restrict__ df, int64_t* __restrict__ stats) {
    __shared__ u64 keys[BM_MAXL];                    // [0, P) in use, P = a power of two >= max(L, 64)
    __shared__ int s_chunk[BM_MAXL / 64];            // valid tokens of each 64-column chunk
    __shared__ int s_cnt[3];                         // tokens that remain, tokens rejected, distinct terms
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const u64 below = (1ull << lane) - 1ull;
    const int nchunk = (L + 63) >> 6;
    long long st_trunc = 0, st_rej = 0, st_len = 0;  // thread 0: this workgroup's share of stats

    for (long r = blockIdx.x; r < n; r += gridDim.x) {
        const int32_t* ri = ids + (size_t)r * ldi;
        const int32_t* rm = mask ? mask + (size_t)r * ldm : nullptr;
        if (threadIdx.x < 3) s_cnt[threadIdx.x] = 0;
        if (rm)
            for (int j = wave; j < nchunk; j += BM_WAVES) {
                const int c = j * 64 + lane;
                const int cnt = __popcll(__ballot(c < L && rm[c] != 0));
                if (lane == 0) s_chunk[j] = cnt;
            }
        __syncthreads();

        int valid = L;
        if (rm) {
            valid = 0;
            for (int i = 0; i < nchunk; ++i) valid += s_chunk[i];
        }
        const int end = valid - tail;                // the ranks [head, end) remain; none when valid <= head + tail
        for (int j = wave; j < (P >> 6); j += BM_WAVES) {
            const int c = j * 64 + lane;             // < P
            const bool kept = c < L && (rm ? rm[c] != 0 : true);
            int before = j * 64;
            if (rm) {
                before = 0;
                for (int i = 0; i < j && i < nchunk; ++i) before += s_chunk[i];
            }
            const int rank = before + __popcll(__ballot(kept) & below);
            const bool in = kept && rank >= head && rank < end;
            const int id = in ? ri[c] : 0;
            const bool ok = in && id >= 0 && id < V;
            keys[c] = ok ? (u64)(unsigned)id : BM_NONE;
            const int nk = __popcll(__ballot(ok)), nr = __popcll(__ballot(in && !ok));
            if (lane == 0) {
                if (nk) atomicAdd(&s_cnt[0], nk);
                if (nr) atomicAdd(&s_cnt[1], nr);
            }
        }
        __syncthreads();
        bm_sort_asc(keys, P);

        const int len = s_cnt[0];                    // the sorted ids are keys[0 .. len)
        u64 k2[BM_PER];
        int heads = 0;
#pragma unroll
        for (int e = 0; e < BM_PER; ++e) {
            const int i = threadIdx.x + e * BM_THREADS;
            k2[e] = BM_NONE;
            if (i < len) {
                const u64 v = keys[i];
                if (i == 0 || keys[i - 1] != v) {    // the head of a run: its count reaches to the upper bound of v
                    int lo = i + 1, hi = len;
                    while (lo < hi) {
                        const int mid = (lo + hi) >> 1;
                        if (keys[mid] == v) lo = mid + 1; else hi = mid;
                    }
                    k2[e] = ((u64)(0xFFFFFFFFu - (unsigned)(lo - i)) << 32) | v;
                    ++heads;
                    if (df) atomicAdd(&df[(int)v], 1);                     // v < V
                }
            }
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) heads += __shfl_xor(heads, o, 64);
        if (lane == 0 && heads) atomicAdd(&s_cnt[2], heads);
        __syncthreads();                             // every read of the sorted ids is done
#pragma unroll
        for (int e = 0; e < BM_PER; ++e) {
            const int i = threadIdx.x + e * BM_THREADS;
            if (i < P) keys[i] = k2[e];
        }
        __syncthreads();
        bm_sort_asc(keys, P);

        int32_t* ot = terms + (size_t)r * ldt;
        int32_t* of = tf + (size_t)r * ldf;
        for (int m = threadIdx.x; m < M; m += BM_THREADS) {
            const u64 key = m < P ? keys[m] : BM_NONE;
            const bool used = key != BM_NONE;
            ot[m] = used ? (int)(unsigned)(key & 0xFFFFFFFFull) : -1;
            of[m] = used ? (int)(0xFFFFFFFFu - (unsigned)(key >> 32)) : 0;
        }
        if (threadIdx.x == 0) {
            doc_len[r] = len;
            st_len += len;
            st_rej += s_cnt[1];
            st_trunc += s_cnt[2] > M ? 1 : 0;
        }
        __syncthreads();                             // s_cnt and keys are rewritten by the next document
    }
    if (threadIdx.x == 0 && stats) {
        u64* st = reinterpret_cast<u64*>(stats);
        if (st_trunc) atomicAdd(&st[0], (u64)st_trunc);
        if (st_rej) atomicAdd(&st[1], (u64)st_rej);
        if (st_len) atomicAdd(&st[2], (u64)st_len);
    }
}

// One wave per row.  The pragma keeps c1 * len + c0 a multiply and an add: contracted into an fma it rounds once
// instead of twice and NumPy's float32 arithmetic no longer gives the same bits.
__global__ __launch_bounds__(BM_THREADS) void bm25_weights_kernel(
        const int32_t* __restrict__ tf, long ldf, const int32_t* __restrict__ doc_len, float* __restrict__ w, long ldw,
        int n, int M, float c0, float c1, float k1p1) {
#pragma clang fp contract(off)
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (long r = (long)blockIdx.x * BM_WAVES + wave; r < n; r += (long)gridDim.x * BM_WAVES) {
        const float scaled = c1 * (float)doc_len[r];
        const float Kr = scaled + c0;
        const int32_t* rt = tf + (size_t)r * ldf;
        float* rw = w + (size_t)r * ldw;
        for (int m = lane; m < M; m += 64) {
            const int t = rt[m];
            const float x = (float)t;
            const float num = x * k1p1;
            const float den = x + Kr;
            rw[m] = t > 0 ? num / den : 0.0f;
        }
    }
}

// One workgroup per query row: zero the row, barrier, store the row's terms (distinct, so plain stores).
__global__ __launch_bounds__(BM_THREADS) void bm25_query_kernel(
        const int32_t* __restrict__ terms, long ldt, const int32_t* __restrict__ tf, long ldf,
        const float* __restrict__ idf, float* __restrict__ q, long ldq, int M, int V) {
    float* row = q + (size_t)blockIdx.x * ldq;
    const int32_t* rt = terms + (size_t)blockIdx.x * ldt;
    const int32_t* rf = tf + (size_t)blockIdx.x * ldf;
    for (int v = threadIdx.x; v < V; v += BM_THREADS) row[v] = 0.0f;
    __syncthreads();                                 // the zeros have left before a term's store to the same address
    for (int m = threadIdx.x; m < M; m += BM_THREADS) {
        const int t = rt[m];
        if (t >= 0 && t < V) row[t] = (float)rf[m] * idf[t];
    }
}

}  // namespace

extern "C" int polus_bm25_term_counts(const int32_t* ids, long ldi, const int32_t* mask, long ldm, int n, int L, int V,
                                      int head, int tail, int32_t* terms, long ldt, int32_t* tf, long ldf, int M,
                                      int32_t* doc_len, int32_t* df, int64_t* stats, void* stream) {
    POLUS_REQUIRE(ids && terms && tf && doc_len, "polus_bm25_term_counts: null pointer (ids, terms, tf or doc_len)");
    POLUS_REQUIRE(L >= 1 && L <= BM_MAXL, "polus_bm25_term_counts: need 1 <= L <= %d (got %d)", BM_MAXL, L);
    POLUS_REQUIRE(M >= 1 && M <= BM_MAXM, "polus_bm25_term_counts: need 1 <= M <= %d (got %d)", BM_MAXM, M);
    POLUS_REQUIRE(n >= 1 && V >= 1, "polus_bm25_term_counts: need n >= 1 and V >= 1 (got %d, %d)", n, V);
    POLUS_REQUIRE(head >= 0 && head <= BM_MAX_STRIP && tail >= 0 && tail <= BM_MAX_STRIP,
                  "polus_bm25_term_counts: strip counts must be in 0..%d (got %d/%d)", BM_MAX_STRIP, head, tail);
    POLUS_REQUIRE(ldi >= L, "polus_bm25_term_counts: id row stride ldi must be >= L (got %ld < %d)", ldi, L);
    POLUS_REQUIRE(!mask || ldm >= L, "polus_bm25_term_counts: mask row stride ldm must be >= L (got %ld < %d)", ldm, L);
    POLUS_REQUIRE(ldt >= M && ldf >= M, "polus_bm25_term_counts: output row strides ldt, ldf must be >= M (got %ld, %ld < %d)",
                  ldt, ldf, M);
    int P = 64;
    while (P < L) P <<= 1;
    const int blocks = n < BM_MAX_BLOCKS ? n : BM_MAX_BLOCKS;
    hipLaunchKernelGGL(bm25_term_counts_kernel, dim3(blocks), dim3(BM_THREADS), 0, static_cast<hipStream_t>(stream), ids,
                       ldi, mask, ldm, n, L, P, V, head, tail, terms, ldt, tf, ldf, M, doc_len, df, stats);
    POLUS_CHECK_LAUNCH("polus_bm25_term_counts");
    return POLUS_OK;
}

extern "C" int polus_bm25_weights(const int32_t* tf, long ldf, const int32_t* doc_len, float* w, long ldw, int n, int M,
                                  float c0, float c1, float k1p1, void* stream) {
    POLUS_REQUIRE(tf && doc_len && w, "polus_bm25_weights: null pointer");
    POLUS_REQUIRE(n >= 1, "polus_bm25_weights: need n >= 1 (got %d)", n);
    POLUS_REQUIRE(M >= 1 && M <= BM_MAXM, "polus_bm25_weights: need 1 <= M <= %d (got %d)", BM_MAXM, M);
    POLUS_REQUIRE(ldf >= M && ldw >= M, "polus_bm25_weights: row strides ldf, ldw must be >= M (got %ld, %ld < %d)", ldf, ldw, M);
    const long want = ((long)n + BM_WAVES - 1) / BM_WAVES;
    const int blocks = (int)(want < 2 * BM_MAX_BLOCKS ? want : 2 * BM_MAX_BLOCKS);
    hipLaunchKernelGGL(bm25_weights_kernel, dim3(blocks), dim3(BM_THREADS), 0, static_cast<hipStream_t>(stream), tf, ldf,
                       doc_len, w, ldw, n, M, c0, c1, k1p1);
    POLUS_CHECK_LAUNCH("polus_bm25_weights");
    return POLUS_OK;
}

extern "C" int polus_bm25_query(const int32_t* terms, long ldt, const int32_t* tf, long ldf, const float* idf, float* q,
                                long ldq, int B, int M, int V, void* stream) {
    POLUS_REQUIRE(terms && tf && idf && q, "polus_bm25_query: null pointer");
    POLUS_REQUIRE(B >= 1, "polus_bm25_query: need B >= 1 (got %d)", B);
    POLUS_REQUIRE(M >= 1 && M <= BM_MAXM, "polus_bm25_query: need 1 <= M <= %d (got %d)", BM_MAXM, M);
    POLUS_REQUIRE(V >= 1 && (long)V * 4 <= BM_MAX_V_BYTES,
                  "polus_bm25_query: need V >= 1 and V * 4 <= %d, the query row polus_sparse_scores holds in LDS (got V %d)",
                  BM_MAX_V_BYTES, V);
    POLUS_REQUIRE(ldt >= M && ldf >= M, "polus_bm25_query: row strides ldt, ldf must be >= M (got %ld, %ld < %d)", ldt, ldf, M);
    POLUS_REQUIRE(ldq >= V, "polus_bm25_query: query row stride ldq must be >= V (got %ld < %d)", ldq, V);
    hipLaunchKernelGGL(bm25_query_kernel, dim3((unsigned)B), dim3(BM_THREADS), 0, static_cast<hipStream_t>(stream), terms,
                       ldt, tf, ldf, idf, q, ldq, M, V);
    POLUS_CHECK_LAUNCH("polus_bm25_query");
    return POLUS_OK;
}
