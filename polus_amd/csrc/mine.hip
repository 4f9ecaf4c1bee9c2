// Hard-negative mining: k negatives per query sampled from a ranked candidate list (polus_amd/ir/mining.py).
//
// The rule (include/polus_hip.h has it in full): the pool of a row is its columns c >= skip_top, in column order,
// whose id is non-negative, is not in the row's exclude list and, with scores, scores above min_score.  With R such
// columns, R <= k copies the pool and pads with -1; R > k cuts the pool into k rank strata [floor(j R / k),
// floor((j + 1) R / k)) and slot j takes position lo + polus_hash32(seed, r k + j) mod (hi - lo) of its stratum.
//
// One wave per query, lanes over 64 consecutive columns per step, as in pairs.hip: the first sweep counts the pool
// (R decides the rule); in the second a column's position in the pool is the popcount of the step's __ballot below
// the lane plus the pool columns of earlier steps, the column finds its own stratum from that position and stores
// itself if it is the stratum's pick.  Every store goes to a distinct address: no LDS, no atomics, no workspace.
#include "common.h"

namespace {

constexpr int MINE_THREADS = 256;                  // 4 waves = 4 queries per workgroup
constexpr int MINE_WAVES = MINE_THREADS / 64;
constexpr int MINE_MAX_BLOCKS = 4096;
constexpr int MINE_MAXK = 1024;
constexpr int MINE_MAXP = 1024;
typedef unsigned long long u64;

struct MineArgs {
    const int32_t* cand; long ldc;
    const float* score; long lds;
    const int32_t* exclude; long lde;
    int Q, C, P, skip_top, k;
    float min_score;
    uint32_t seed;
};

// column c of row r is in the pool; `id` is its candidate (valid where the result is true)
__device__ __forceinline__ bool mine_pass(const MineArgs& a, const int32_t* __restrict__ cr, const float* __restrict__ sr,
                                          const int32_t* __restrict__ er, int c, int& id) {
    bool ok = c < a.C && c >= a.skip_top;
    id = ok ? cr[c] : -1;
    ok = ok && id >= 0;
    if (sr) ok = ok && sr[c] > a.min_score;                    // read for c < C only; a NaN fails
    if (__ballot(ok) != 0)                                     // uniform
        for (int e = 0; e < a.P; ++e) ok = ok && er[e] != id;  // id >= 0: a negative entry of exclude never matches
    return ok;
}

__global__ __launch_bounds__(MINE_THREADS) void mine_negatives_kernel(MineArgs a, int32_t* __restrict__ neg,
                                                                      int32_t* __restrict__ neg_col,
                                                                      int32_t* __restrict__ n_pool) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const u64 below = (1ull << lane) - 1ull;
    const int k = a.k;
    const int first = a.skip_top < a.C ? (a.skip_top & ~63) : a.C;         // no pool column lies before this step
    for (long r = (long)blockIdx.x * MINE_WAVES + wave; r < a.Q; r += (long)gridDim.x * MINE_WAVES) {
        const int32_t* cr = a.cand + (size_t)r * a.ldc;
        const float* sr = a.score ? a.score + (size_t)r * a.lds : nullptr;
        const int32_t* er = a.exclude + (size_t)r * a.lde;                 // not read when P == 0
        int32_t* on = neg + (size_t)r * k;
        int32_t* oc = neg_col ? neg_col + (size_t)r * k : nullptr;

        int R = 0;
        for (int base = first; base < a.C; base += 64) {
            int id;
            R += __popcll(__ballot(mine_pass(a, cr, sr, er, base + lane, id)));
        }
        const bool all = R <= k;
        if (all)
            for (int j = R + lane; j < k; j += 64) {
                on[j] = -1;
                if (oc) oc[j] = -1;
            }
        int seen = 0;                              // pool columns of earlier steps (uniform)
        for (int base = first; base < a.C && seen < R; base += 64) {
            const int c = base + lane;
            int id;
            const bool ok = mine_pass(a, cr, sr, er, c, id);
            const u64 K = __ballot(ok);
            const long pos = seen + __popcll(K & below);                   // position in the pool, < R
            if (ok) {
                long slot = pos;
                bool take = all;
                if (!all) {
                    // the stratum of pos: the largest j with floor(j R / k) <= pos
                    slot = ((pos + 1) * k - 1) / R;
                    const long lo = slot * R / k, hi = (slot + 1) * R / k;   // lo <= pos < hi
                    const uint32_t h = polus_hash32(a.seed, (uint32_t)((u64)r * (u64)k + (u64)slot));
                    take = lo + (long)(h % (uint32_t)(hi - lo)) == pos;
                }
                if (take) {
                    on[slot] = id;
                    if (oc) oc[slot] = c;
                }
            }
            seen += __popcll(K);
        }
        if (lane == 0) n_pool[r] = R;
    }
}

}  // namespace

extern "C" int polus_mine_negatives(const int32_t* cand, long ldc, const float* score, long lds, const int32_t* exclude,
                                    long lde, int Q, int C, int P, int skip_top, float min_score, int k, uint32_t seed,
                                    int32_t* neg, int32_t* neg_col, int32_t* n_pool, void* stream) {
    POLUS_REQUIRE(cand && neg && n_pool, "polus_mine_negatives: null pointer (cand, neg or n_pool)");
    POLUS_REQUIRE(Q >= 1 && C >= 1, "polus_mine_negatives: need Q, C >= 1 (got %d, %d)", Q, C);
    POLUS_REQUIRE(k >= 1 && k <= MINE_MAXK, "polus_mine_negatives: need 1 <= k <= %d (got %d)", MINE_MAXK, k);
    POLUS_REQUIRE(P >= 0 && P <= MINE_MAXP, "polus_mine_negatives: need 0 <= P <= %d (got %d)", MINE_MAXP, P);
    POLUS_REQUIRE(P == 0 || exclude, "polus_mine_negatives: null pointer (exclude) with P = %d", P);
    POLUS_REQUIRE(skip_top >= 0, "polus_mine_negatives: need skip_top >= 0 (got %d)", skip_top);
    POLUS_REQUIRE((long long)Q * k < (1LL << 32), "polus_mine_negatives: Q*k must be < 2^32 (got %d x %d)", Q, k);
    POLUS_REQUIRE(ldc >= C, "polus_mine_negatives: candidate row stride ldc must be >= C (got %ld < %d)", ldc, C);
    POLUS_REQUIRE(!score || lds >= C, "polus_mine_negatives: score row stride lds must be >= C (got %ld < %d)", lds, C);
    POLUS_REQUIRE(P == 0 || lde >= P, "polus_mine_negatives: exclude row stride lde must be >= P (got %ld < %d)", lde, P);
    const MineArgs a = {cand, ldc, score, lds, P ? exclude : nullptr, P ? lde : 0, Q, C, P, skip_top, k, min_score, seed};
    const long want = ((long)Q + MINE_WAVES - 1) / MINE_WAVES;
    const int blocks = (int)(want < MINE_MAX_BLOCKS ? want : MINE_MAX_BLOCKS);
    hipLaunchKernelGGL(mine_negatives_kernel, dim3(blocks), dim3(MINE_THREADS), 0, static_cast<hipStream_t>(stream), a, neg,
                       neg_col, n_pool);
    POLUS_CHECK_LAUNCH("polus_mine_negatives");
    return POLUS_OK;
}
