// Rank fusion (polus_amd/ir/fusion.py): L ranked lists per query joined by document id and their scores fused by
// reciprocal rank (RRF), CombSUM or CombSUM over min-max normalised scores.
//
// The rule (include/polus_hip.h has it in full).  An entry is kept iff its id lies in [0, n_docs) and, with scores, its
// score is finite; the rank of a kept entry is 1 plus the kept entries of its list row at lower columns; its
// contribution is w / (rrf_k + rank), w s or w ((s - lo) / (hi - lo)), every operation rounded once; a document's fused
// score adds its contributions in (list, column) order; the row goes out as the distinct ids ascending with their
// scores, then (-1, -inf).
//
// One workgroup per query (grid-stride over the queries).  Pass 1 reads every list row once, a wave per 64-column step:
// the id becomes the 64-bit key id << 13 | slot (slot = l C + c < 4096; ~0 for a dropped entry) and the raw score goes to
// LDS beside it, the step's kept entries are counted by __ballot and its lo / hi taken by a wave reduction.  After a
// barrier the same wave returns to its steps: rank = the kept entries of the row's earlier steps plus the popcount of
// the step's ballot below the lane (mine.hip's idiom), and the score in LDS is replaced by the contribution.  Pass 2
// bitonic-sorts the keys ascending (bm25.hip's network): the order is then (id, list, column).  Pass 3: a position whose
// left neighbour has another id is the head of a run; it walks its run (L entries where the lists hold no repeats)
// adding contrib[slot] in order, and the heads are compacted by ballot and popcount with a running base.  LDS: 4096
// keys and 4096 floats = 48 KiB.  No atomics, no workspace, plain vector stores to distinct addresses.
#include "common.h"

namespace {

constexpr int FUSE_THREADS = 1024;
constexpr int FUSE_WAVES = FUSE_THREADS / 64;
constexpr int FUSE_MAXL = 8;
constexpr int FUSE_MAXN = 4096;                              // entries per query, L * C
constexpr int FUSE_MAXSTEP = FUSE_MAXN / 64 + FUSE_MAXL;     // L * ceil(C / 64) <= (L C + 63 L) / 64 < 72
constexpr int FUSE_MAX_BLOCKS = 512;                         // two workgroups of 16 waves per CU
constexpr int FUSE_SLOT_BITS = 13;
typedef unsigned long long u64;
constexpr u64 FUSE_NONE = ~0ull;                             // sorts behind every real key; its id field matches no id

struct FuseArgs {
    const int32_t* ids; long lsi, ldi;
    const float* scores; long lss, lds;
    int L, Q, C, P, n_docs, mode;
    float rrf_k;
    float w[FUSE_MAXL];
};

// bm25.hip's bm_exchange / bm_sort_asc for this kernel's workgroup: keys[0 .. m) ascending, m a power of two >= 64;
// every thread calls it; ends on a barrier.  The stages with a stride below 64 run on lane shuffles.
__device__ __forceinline__ u64 fuse_exchange(u64 v, int i, int size, int stride) {
    const u64 o = __shfl_xor(v, stride, 64);
    const bool keep_min = ((i & stride) == 0) == ((i & size) == 0);
    return keep_min ? (v < o ? v : o) : (v > o ? v : o);
}

__device__ __forceinline__ void fuse_sort_asc(u64* keys, int m) {
    for (int i = threadIdx.x; i < m; i += FUSE_THREADS) {       // uniform per wave: m is a multiple of 64
        u64 v = keys[i];
        for (int size = 2; size <= 64; size <<= 1)
            for (int stride = size >> 1; stride > 0; stride >>= 1) v = fuse_exchange(v, i, size, stride);
        keys[i] = v;
    }
    __syncthreads();
    for (int size = 128; size <= m; size <<= 1) {
        for (int stride = size >> 1; stride >= 64; stride >>= 1) {
            for (int t = threadIdx.x; t < (m >> 1); t += FUSE_THREADS) {
                const int i = 2 * t - (t & (stride - 1)), j = i + stride;   // j < m
                const u64 a = keys[i], b = keys[j];
                const bool asc = (i & size) == 0;
                if ((a > b) == asc) { keys[i] = b; keys[j] = a; }
            }
            __syncthreads();
        }
        for (int i = threadIdx.x; i < m; i += FUSE_THREADS) {
            u64 v = keys[i];
            for (int stride = 32; stride > 0; stride >>= 1) v = fuse_exchange(v, i, size, stride);
            keys[i] = v;
        }
        __syncthreads();
    }
}

__device__ __forceinline__ bool fuse_finite(float s) { return (__float_as_uint(s) & 0x7F800000u) != 0x7F800000u; }

// The pragma keeps every operation its own rounding (bm25_weights_kernel): NumPy float32 gives the same bits.
__device__ __forceinline__ float fuse_contribution(int mode, float w, float rrf_k, int rank, float s, float lo, float hi) {
#pragma clang fp contract(off)
    if (mode == POLUS_FUSE_RRF) {
        const float den = rrf_k + (float)rank;
        return w / den;
    }
    if (mode == POLUS_FUSE_SUM) return w * s;
    if (hi == lo) return w * 1.0f;
    const float num = s - lo;
    const float den = hi - lo;
    const float t = num / den;
    return w * t;
}

__global__ __launch_bounds__(FUSE_THREADS) void fuse_lists_kernel(FuseArgs a, int32_t* __restrict__ out_id, long ldoi,
                                                                  float* __restrict__ out_val, long ldov,
                                                                  int32_t* __restrict__ count) {
    __shared__ u64 keys[FUSE_MAXN];                  // [0, P) in use, P = a power of two >= max(L C, 64)
    __shared__ float contrib[FUSE_MAXN];             // by slot: the raw score, then the contribution
    __shared__ int s_kept[FUSE_MAXSTEP];             // kept entries of each 64-column step of each list row
    __shared__ float s_lo[FUSE_MAXSTEP], s_hi[FUSE_MAXSTEP];
    __shared__ int s_heads[FUSE_WAVES];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const u64 below = (1ull << lane) - 1ull;
    const int L = a.L, C = a.C, P = a.P, n = L * C;
    const int nstep = (C + 63) >> 6;                 // steps per list row; L * nstep <= FUSE_MAXSTEP

    for (long r = blockIdx.x; r < a.Q; r += gridDim.x) {
        // ---- pass 1a: keys and raw scores into LDS, each step's kept count and score range
        for (int p = wave; p < L * nstep; p += FUSE_WAVES) {
            const int l = p / nstep, c = (p - l * nstep) * 64 + lane;
            const int32_t* ri = a.ids + (size_t)l * a.lsi + (size_t)r * a.ldi;
            const float* rs = a.scores ? a.scores + (size_t)l * a.lss + (size_t)r * a.lds : nullptr;
            const int id = c < C ? ri[c] : -1;
            const float s = (rs && c < C) ? rs[c] : 0.0f;
            const bool kept = id >= 0 && id < a.n_docs && fuse_finite(s);
            const int cnt = __popcll(__ballot(kept));
            float lo = kept ? s : INFINITY, hi = kept ? s : -INFINITY;
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) {
                lo = fminf(lo, __shfl_xor(lo, o, 64));
                hi = fmaxf(hi, __shfl_xor(hi, o, 64));
            }
            if (c < C) {
                const int slot = l * C + c;          // < n <= FUSE_MAXN
                keys[slot] = kept ? ((u64)(unsigned)id << FUSE_SLOT_BITS) | (u64)slot : FUSE_NONE;
                contrib[slot] = s;
            }
            if (lane == 0) { s_kept[p] = cnt; s_lo[p] = lo; s_hi[p] = hi; }
        }
        for (int i = n + threadIdx.x; i < P; i += FUSE_THREADS) keys[i] = FUSE_NONE;
        __syncthreads();

        // ---- pass 1b: the same wave returns to its steps: rank, the row's lo / hi, the contribution
        for (int p = wave; p < L * nstep; p += FUSE_WAVES) {
            const int l = p / nstep, j = p - l * nstep, c = j * 64 + lane;
            int before = 0;
            float lo = INFINITY, hi = -INFINITY;
            for (int i = 0; i < nstep; ++i) {        // uniform
                const int q = l * nstep + i;
                if (i < j) before += s_kept[q];
                lo = fminf(lo, s_lo[q]);
                hi = fmaxf(hi, s_hi[q]);
            }
            const int slot = l * C + c;
            const bool kept = c < C && keys[slot] != FUSE_NONE;
            const int rank = before + __popcll(__ballot(kept) & below) + 1;
            if (kept) contrib[slot] = fuse_contribution(a.mode, a.w[l], a.rrf_k, rank, contrib[slot], lo, hi);
        }
        __syncthreads();

        // ---- pass 2: (id, list, column) order
        fuse_sort_asc(keys, P);

        // ---- pass 3: run heads add their run in order and go out compacted
        int32_t* oi = out_id + (size_t)r * ldoi;
        float* ov = out_val + (size_t)r * ldov;
        int done = 0;                                // distinct ids of earlier tiles (uniform)
        for (int t0 = 0; t0 < P; t0 += FUSE_THREADS) {
            const int i = t0 + threadIdx.x;
            u64 key = FUSE_NONE;
            bool head = false;
            if (i < P) {
                key = keys[i];
                head = key != FUSE_NONE && (i == 0 || (keys[i - 1] >> FUSE_SLOT_BITS) != (key >> FUSE_SLOT_BITS));
            }
            const u64 H = __ballot(head);
            if (lane == 0) s_heads[wave] = __popcll(H);
            __syncthreads();
            int pos = done;
            for (int w = 0; w < FUSE_WAVES; ++w) {
                const int h = s_heads[w];
                if (w < wave) pos += h;
                done += h;
            }
            if (head) {
                pos += __popcll(H & below);          // < the number of kept entries <= n
                const u64 id = key >> FUSE_SLOT_BITS;
                float acc = contrib[(int)(key & (FUSE_MAXN - 1))];
                for (int j = i + 1; j < P; ++j) {
                    const u64 k2 = keys[j];
                    if ((k2 >> FUSE_SLOT_BITS) != id) break;
                    acc = acc + contrib[(int)(k2 & (FUSE_MAXN - 1))];
                }
                oi[pos] = (int32_t)id;
                ov[pos] = acc;
            }
            __syncthreads();                         // s_heads is rewritten by the next tile
        }
        for (int m = done + threadIdx.x; m < n; m += FUSE_THREADS) {
            oi[m] = -1;
            ov[m] = -INFINITY;
        }
        if (threadIdx.x == 0) count[r] = done;
        // the barrier that ended the last tile separates this row's LDS reads from the next row's writes
    }
}

}  // namespace

extern "C" int polus_fuse_lists(const int32_t* ids, long lsi, long ldi, const float* scores, long lss, long lds, int L,
                                int Q, int C, int n_docs, int mode, const float* weights, float rrf_k, int32_t* out_id,
                                long ldoi, float* out_val, long ldov, int32_t* count, void* stream) {
    POLUS_REQUIRE(ids && out_id && out_val && count, "polus_fuse_lists: null pointer (ids, out_id, out_val or count)");
    POLUS_REQUIRE(mode == POLUS_FUSE_RRF || mode == POLUS_FUSE_SUM || mode == POLUS_FUSE_MINMAX,
                  "polus_fuse_lists: mode must be 0 (rrf), 1 (sum) or 2 (minmax) (got %d)", mode);
    POLUS_REQUIRE(L >= 1 && L <= FUSE_MAXL, "polus_fuse_lists: need 1 <= L <= %d (got %d)", FUSE_MAXL, L);
    POLUS_REQUIRE(Q >= 1 && C >= 1, "polus_fuse_lists: need Q >= 1 and C >= 1 (got %d, %d)", Q, C);
    POLUS_REQUIRE((long)L * C <= FUSE_MAXN, "polus_fuse_lists: need L*C <= %d (got %d x %d)", FUSE_MAXN, L, C);
    POLUS_REQUIRE(n_docs >= 1, "polus_fuse_lists: need 1 <= n_docs <= 2^31 - 1 (got %d)", n_docs);
    POLUS_REQUIRE(scores || mode == POLUS_FUSE_RRF, "polus_fuse_lists: null pointer (scores) with mode %d; only rrf fuses without scores", mode);
    POLUS_REQUIRE(mode != POLUS_FUSE_RRF || (rrf_k >= 0.0f && isfinite(rrf_k)),
                  "polus_fuse_lists: rrf_k must be finite and >= 0 (got %g)", (double)rrf_k);
    POLUS_REQUIRE(ldi >= C, "polus_fuse_lists: id row stride ldi must be >= C (got %ld < %d)", ldi, C);
    POLUS_REQUIRE(L == 1 || lsi >= (long)(Q - 1) * ldi + C,
                  "polus_fuse_lists: id list stride lsi must be >= (Q - 1) ldi + C, the extent of one list (got %ld)", lsi);
    POLUS_REQUIRE(!scores || lds >= C, "polus_fuse_lists: score row stride lds must be >= C (got %ld < %d)", lds, C);
    POLUS_REQUIRE(!scores || L == 1 || lss >= (long)(Q - 1) * lds + C,
                  "polus_fuse_lists: score list stride lss must be >= (Q - 1) lds + C, the extent of one list (got %ld)", lss);
    POLUS_REQUIRE(ldoi >= (long)L * C && ldov >= (long)L * C,
                  "polus_fuse_lists: output row strides ldoi, ldov must be >= L*C (got %ld, %ld < %d)", ldoi, ldov, L * C);
    FuseArgs a = {ids, lsi, ldi, scores, lss, lds, L, Q, C, 64, n_docs, mode, rrf_k, {}};
    for (int l = 0; l < FUSE_MAXL; ++l) {
        a.w[l] = (weights && l < L) ? weights[l] : 1.0f;
        POLUS_REQUIRE(isfinite(a.w[l]), "polus_fuse_lists: weights must be finite (weights[%d] = %g)", l, (double)a.w[l]);
    }
    while (a.P < L * C) a.P <<= 1;
    const int blocks = Q < FUSE_MAX_BLOCKS ? Q : FUSE_MAX_BLOCKS;
    hipLaunchKernelGGL(fuse_lists_kernel, dim3(blocks), dim3(FUSE_THREADS), 0, static_cast<hipStream_t>(stream), a, out_id,
                       ldoi, out_val, ldov, count);
    POLUS_CHECK_LAUNCH("polus_fuse_lists");
    return POLUS_OK;
}
