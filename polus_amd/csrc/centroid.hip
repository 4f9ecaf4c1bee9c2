// Centroid-pruned search of a token index (polus_amd/ir/search.py search_pruned, fit_centroids): every stored
// document token is replaced by the id of its nearest centroid (a 16-bit code), a query token's similarity to all K
// centroids is one row segment of a table, and MaxSim is approximated by look-ups:
//
//   score[b, n] = sum over valid i of  max over present j of  table[codes[n, j], b * Lq + i]
//
// polus_centroid_scores: one workgroup per (query, contiguous range of documents); each wave takes the documents
// wave, wave + nw, ... of the range and owns a (query, document) pair from the first look-up to the store, so the bits
// of an entry depend on nothing but that pair.  Lanes spread over query tokens:
//   MODE 0  Lq > 32:   lane l holds the running maxima of query tokens l, l + 64, ... (1, 2, 4 or 8 rounds); one
//                      document token per step, its code wave-uniform (v_readlane): a step reads one contiguous row.
//   MODE 1  17..32:    lanes (i, sub): query token i = lane & 31, document token 2 s + sub of step s; the two codes of
//                      a step travel as one 32-bit pair (one v_readlane), so a step reads two whole rows.
//   MODE 2  Lq <= 16:  P = the power of two >= Lq lanes per document token, 64 / P tokens per step (ds_bpermute).
// A wave loads 64 codes at once (one per lane), clamps absent ones (0xFFFF or >= K) to K and skips the steps behind the
// block's last present token.  The maxima are exact; the sub-groups' maxima are combined by xor shuffles, a query
// token without a present document token (-inf) or with a zero mask adds 0.0, and one wave_sum adds the query tokens:
// an order fixed by Lq alone, on either route.
//   LDS route:    the workgroup (16 waves: 4 per SIMD, what 4-byte LDS reads need for their rate) first copies the
//                 query's [K, Lq] slice of the table into LDS, rows packed at stride Lq floats (no padding: a step's
//                 lanes read consecutive floats of one row), and adds row K = -inf, which absent codes read.
//                 LDS bytes = (K + 1) * Lq * 4, route taken iff that is <= 160 KiB (K <= 1279 at Lq = 32).
//   global route: 4 waves, the same loop with the rows read from global memory (L2 / Infinity Cache in practice);
//                 an absent code reads nothing.
// polus_centroid_scores_ids: the same kernel with the document of a column read from a candidate list (ivf.hip makes
// the lists); a pair's bits are those of polus_centroid_scores.
// polus_centroid_codes: one wave per row of a similarity matrix, 16-byte reads, the first maximum wins.
// polus_centroid_update: one workgroup per centroid sums its tokens in a fixed order and normalises.
#include <algorithm>
#include <limits.h>

#include "common.h"

namespace {

constexpr int CS_LMAX = 512;                      // query / document tokens, as for MaxSim
constexpr int CS_KMAX = 65535;                    // 0xFFFF is "no token"
constexpr size_t CS_LDS_MAX = 160 * 1024;         // one CU's LDS
constexpr int CS_LDS_THREADS = 1024, CS_GLB_THREADS = 256;
constexpr int CS_EMAX = 256;

static inline size_t cs_lds_bytes(int Lq, int K) { return ((size_t)K + 1) * (size_t)Lq * sizeof(float); }
static inline bool cs_lds_route(int Lq, int K) { return cs_lds_bytes(Lq, K) <= CS_LDS_MAX; }
static inline int cs_mode(int Lq) { return Lq > 32 ? 0 : (Lq > 16 ? 1 : 2); }

// Documents per workgroup: about four workgroups per CU over the launch (the LDS route holds one per CU at a time),
// never fewer than 4 per wave unless N is smaller, so that the copy of the table is a small share of the work.
static int cs_docs_per_block(int B, int N, int nw) {
    const long per_query = std::max(1L, 4L * polus_num_cus() / B);
    long dpb = std::max(((long)N + per_query - 1) / per_query, 4L * nw);
    dpb = (dpb + nw - 1) / nw * nw;
    return (int)std::min(dpb, (long)N);
}

// One look-up: query token ic of centroid row c.  LDS: absent codes were clamped to row K = -inf.  Global: the load is
// unconditional on a clamped row (a load under a per-lane condition is waited for where it is issued) and an absent
// code's value is replaced by -inf.
template <bool LDS>
__device__ __forceinline__ float cs_fetch(const float* cs_rows, const float* tq, long ldt, int c, int ic, int Lq, int K) {
    if constexpr (LDS) return cs_rows[__umul24(c, Lq) + ic];
    const float v = tq[(size_t)min(c, K - 1) * ldt + ic];
    return c < K ? v : -INFINITY;
}

// RM (MODE 0): the rounds ceil(Lq / 64) rounded up to a power of two; a lane's rounds past Lq re-read token Lq - 1 and add
// nothing, which keeps the look-ups of a step free of branches.  Steps are taken UN at a time, every look-up of a group
// issued before the first maximum is taken, so that a wave has UN * RM reads in flight, not one; a group may run past
// the last step: the lanes behind it hold absent codes (-inf), or, by wrap-around, tokens already seen (a max is
// idempotent).
// IDS (polus_centroid_scores_ids): the launch has N columns per query and column n is document cand[b, n] of a corpus of
// `docs` documents; an id outside [0, docs) stores -inf and reads nothing.  Everything behind the document's address is
// the code of the other instantiation, so a pair has the same bits from either.
template <int MODE, int RM, bool LDS, bool IDS>
__global__ __launch_bounds__(CS_LDS_THREADS) void centroid_scores_kernel(const float* __restrict__ table, long ldt,
                                                                         const int32_t* __restrict__ qmask,
                                                                         const uint16_t* __restrict__ codes,
                                                                         const int32_t* __restrict__ cand, long ldc,
                                                                         int docs, float* __restrict__ score, long lds,
                                                                         int N, int Lq, int Ld, int K, int dpb) {
    extern __shared__ float cs_rows[];                        // LDS route: [K + 1, Lq]
    constexpr int UN = MODE == 0 ? (RM >= 4 ? 2 : 8 / RM) : (MODE == 1 ? 8 : 4);
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int nw = blockDim.x >> 6;
    const int b = blockIdx.y;
    const int n0 = blockIdx.x * dpb, n1 = min(N, n0 + dpb);
    const float* tq = table + (size_t)b * Lq;                 // this query's columns of every row

    if constexpr (LDS) {
        int cp = 1, cl = 0;                                   // cp = 2^cl lanes copy one row
        while (cp < Lq && cp < 256) { cp <<= 1; ++cl; }
        const int ci = threadIdx.x & (cp - 1), per = blockDim.x >> cl;
        for (int c = threadIdx.x >> cl; c < K; c += per)
            for (int i = ci; i < Lq; i += cp) cs_rows[c * Lq + i] = tq[(size_t)c * ldt + i];
        for (int i = threadIdx.x; i < Lq; i += blockDim.x) cs_rows[K * Lq + i] = -INFINITY;
        __syncthreads();
    }

    // lane -> query token(s); a lane past Lq reads token Lq - 1 and adds nothing
    int lp = 6;                                               // log2 of the lanes per document token
    if constexpr (MODE == 1) lp = 5;
    if constexpr (MODE == 2) { lp = 0; while ((1 << lp) < Lq) ++lp; }
    const int sub = lane >> lp;
    int ic[RM];
    bool ok[RM];
#pragma unroll
    for (int r = 0; r < RM; ++r) {
        const int i = 64 * r + (lane & ((1 << lp) - 1));
        ic[r] = min(i, Lq - 1);
        ok[r] = i < Lq && sub == 0 && (qmask ? qmask[(size_t)b * Lq + ic[r]] != 0 : true);
    }

    for (int n = n0 + wave; n < n1; n += nw) {
        int d = n;
        if constexpr (IDS) {
            d = __builtin_amdgcn_readfirstlane(cand[(size_t)b * ldc + n]);
            if (d < 0 || d >= docs) {                         // uniform
                if (lane == 0) score[(size_t)b * lds + n] = -INFINITY;
                continue;
            }
        }
        const uint16_t* cn = codes + (size_t)d * Ld;
        float m[RM];
#pragma unroll
        for (int r = 0; r < RM; ++r) m[r] = -INFINITY;
        for (int j0 = 0; j0 < Ld; j0 += 64) {
            const int j = j0 + lane;
            int cv = j < Ld ? (int)cn[j] : 0xFFFF;
            cv = min(cv, K);                                  // absent (0xFFFF >= K always, or any code >= K) -> K
            const unsigned long long pres = __ballot(cv < K);
            if (pres == 0) continue;                          // uniform
            const int cnt = 64 - __builtin_clzll(pres);       // steps behind the last present token are skipped
            if constexpr (MODE == 0) {
                for (int s0 = 0; s0 < cnt; s0 += UN) {        // cnt <= 64 and UN divides 64: s0 + u <= 63
                    float v[UN][RM];
#pragma unroll
                    for (int u = 0; u < UN; ++u) {
                        const int c = __builtin_amdgcn_readlane(cv, s0 + u);
#pragma unroll
                        for (int r = 0; r < RM; ++r) v[u][r] = cs_fetch<LDS>(cs_rows, tq, ldt, c, ic[r], Lq, K);
                    }
#pragma unroll
                    for (int u = 0; u < UN; ++u)
#pragma unroll
                        for (int r = 0; r < RM; ++r) m[r] = fmaxf(m[r], v[u][r]);
                }
            } else {
                int pair = 0;
                if constexpr (MODE == 1)                      // lane l < 32: the codes of tokens 2 l and 2 l + 1
                    pair = __shfl(cv, (2 * lane) & 63, 64) | (__shfl(cv, (2 * lane + 1) & 63, 64) << 16);
                const int steps = (cnt + (64 >> lp) - 1) >> (6 - lp);
                for (int s0 = 0; s0 < steps; s0 += UN) {      // MODE 1: steps <= 32 and UN divides 32: s0 + u <= 31
                    float v[UN];
#pragma unroll
                    for (int u = 0; u < UN; ++u) {
                        int c;
                        if constexpr (MODE == 1) c = (__builtin_amdgcn_readlane(pair, s0 + u) >> (16 * sub)) & 0xFFFF;
                        else c = __shfl(cv, (((s0 + u) << (6 - lp)) + sub) & 63, 64);
                        v[u] = cs_fetch<LDS>(cs_rows, tq, ldt, c, ic[0], Lq, K);
                    }
#pragma unroll
                    for (int u = 0; u < UN; ++u) m[0] = fmaxf(m[0], v[u]);
                }
            }
        }
        if constexpr (MODE != 0) {
            for (int o = 1 << lp; o < 64; o <<= 1)            // the sub-groups' maxima of one query token
                m[0] = fmaxf(m[0], __shfl_xor(m[0], o, 64));
        }
        float s = 0.f;
#pragma unroll
        for (int r = 0; r < RM; ++r) s += (ok[r] && m[r] > -INFINITY) ? m[r] : 0.f;
        s = wave_sum(s);
        if (lane == 0) score[(size_t)b * lds + n] = s;
    }
}

// N = the columns of the launch: documents 0 .. N, or with IDS the candidates per query out of `docs` documents.
template <int MODE, int RM, bool IDS>
int cs_launch(const float* table, long ldt, const int32_t* qmask, const uint16_t* codes, const int32_t* cand, long ldc,
              int docs, float* score, long lds, int B, int N, int Lq, int Ld, int K, hipStream_t st) {
    const char* what = IDS ? "polus_centroid_scores_ids" : "polus_centroid_scores";
    if (cs_lds_route(Lq, K)) {
        const int dpb = cs_docs_per_block(B, N, CS_LDS_THREADS / 64);
        dim3 grid((unsigned)((N + dpb - 1) / dpb), (unsigned)B);
        return polus_launch_lds<centroid_scores_kernel<MODE, RM, true, IDS>>(what, grid, dim3(CS_LDS_THREADS), CS_LDS_MAX,
                                                                             cs_lds_bytes(Lq, K), st, table, ldt, qmask,
                                                                             codes, cand, ldc, docs, score, lds, N, Lq, Ld,
                                                                             K, dpb);
    }
    const int dpb = cs_docs_per_block(B, N, CS_GLB_THREADS / 64);
    dim3 grid((unsigned)((N + dpb - 1) / dpb), (unsigned)B);
    hipLaunchKernelGGL((centroid_scores_kernel<MODE, RM, false, IDS>), grid, dim3(CS_GLB_THREADS), 0, st, table, ldt, qmask,
                       codes, cand, ldc, docs, score, lds, N, Lq, Ld, K, dpb);
    POLUS_CHECK_LAUNCH(what);
    return POLUS_OK;
}

template <bool IDS>
int cs_dispatch(const float* table, long ldt, const int32_t* qmask, const uint16_t* codes, const int32_t* cand, long ldc,
                int docs, float* score, long lds, int B, int N, int Lq, int Ld, int K, hipStream_t st) {
    if (cs_mode(Lq) == 1) return cs_launch<1, 1, IDS>(table, ldt, qmask, codes, cand, ldc, docs, score, lds, B, N, Lq, Ld, K, st);
    if (cs_mode(Lq) == 2) return cs_launch<2, 1, IDS>(table, ldt, qmask, codes, cand, ldc, docs, score, lds, B, N, Lq, Ld, K, st);
    const int R = (Lq + 63) / 64;
    if (R == 1) return cs_launch<0, 1, IDS>(table, ldt, qmask, codes, cand, ldc, docs, score, lds, B, N, Lq, Ld, K, st);
    if (R == 2) return cs_launch<0, 2, IDS>(table, ldt, qmask, codes, cand, ldc, docs, score, lds, B, N, Lq, Ld, K, st);
    if (R <= 4) return cs_launch<0, 4, IDS>(table, ldt, qmask, codes, cand, ldc, docs, score, lds, B, N, Lq, Ld, K, st);
    return cs_launch<0, 8, IDS>(table, ldt, qmask, codes, cand, ldc, docs, score, lds, B, N, Lq, Ld, K, st);
}

// ---------------------------------------------------------------- nearest centroid of each row
// Total order: the larger value, then the lower column; NaN compares false and never enters.  col = INT_MAX: nothing yet
// (a -inf entry still wins over it by the column rule).
__device__ __forceinline__ void cc_take(float& bv, int& bc, float v, int c) {
    if (v > bv || (v == bv && c < bc)) { bv = v; bc = c; }
}

__global__ __launch_bounds__(256) void centroid_codes_kernel(const float* __restrict__ sim, long lds,
                                                             const int32_t* __restrict__ mask,
                                                             uint16_t* __restrict__ codes, int rows, int K) {
    const int lane = threadIdx.x & 63;
    const long r = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= rows) return;
    if (mask && mask[r] == 0) {
        if (lane == 0) codes[r] = 0xFFFF;
        return;
    }
    const float* row = sim + (size_t)r * lds;
    float bv = -INFINITY;
    int bc = INT_MAX;
    if ((((uintptr_t)row) & 15) == 0) {                         // wave-uniform
        for (int c = 4 * lane; c < K; c += 256) {
            if (c + 3 < K) {
                const float4 v = *reinterpret_cast<const float4*>(row + c);
                cc_take(bv, bc, v.x, c); cc_take(bv, bc, v.y, c + 1); cc_take(bv, bc, v.z, c + 2); cc_take(bv, bc, v.w, c + 3);
            } else {
                for (int e = c; e < K; ++e) cc_take(bv, bc, row[e], e);
            }
        }
    } else {
        for (int c = lane; c < K; c += 64) cc_take(bv, bc, row[c], c);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float v2 = __shfl_xor(bv, o, 64);
        const int c2 = __shfl_xor(bc, o, 64);
        cc_take(bv, bc, v2, c2);
    }
    if (lane == 0) codes[r] = (uint16_t)(bc == INT_MAX ? 0 : bc);
}

// ---------------------------------------------------------------- one spherical k-means update
// Workgroup k, 4 waves: wave w scans tokens [w * slice, (w + 1) * slice) in ascending order, 64 codes at a time, and
// adds the rows whose code is k (lane l: features l, l + 64, ...); the partials are added as (w0 + w1) + (w2 + w3).
template <typename T>
__global__ __launch_bounds__(256) void centroid_update_kernel(const T* __restrict__ x, const uint16_t* __restrict__ codes,
                                                              const T* __restrict__ prev, T* __restrict__ out,
                                                              int32_t* __restrict__ counts, int Tn, int E, float eps) {
    __shared__ float part[4][CS_EMAX];
    __shared__ int cnt[4];
    __shared__ float sq[CS_EMAX];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int k = blockIdx.x;
    const int slice = (Tn + 3) / 4;
    const int t0 = min(Tn, wave * slice), t1 = min(Tn, t0 + slice);
    float acc[CS_EMAX / 64] = {0.f, 0.f, 0.f, 0.f};
    int found = 0;
    for (int tb = t0; tb < t1; tb += 64) {
        const int t = tb + lane;
        unsigned long long hit = __ballot(t < t1 && (int)codes[t] == k);
        found += __builtin_popcountll(hit);
        while (hit) {                                         // uniform; ascending t
            const int l = __builtin_ctzll(hit);
            hit &= hit - 1;
            const T* xr = x + (size_t)(tb + l) * E;
#pragma unroll
            for (int q = 0; q < CS_EMAX / 64; ++q)
                if (lane + 64 * q < E) acc[q] += to_f<T>(xr[lane + 64 * q]);
        }
    }
#pragma unroll
    for (int q = 0; q < CS_EMAX / 64; ++q) part[wave][lane + 64 * q] = acc[q];
    if (lane == 0) cnt[wave] = found;
    __syncthreads();
    const int e = threadIdx.x;
    const float s = (part[0][e] + part[1][e]) + (part[2][e] + part[3][e]);
    sq[e] = e < E ? s * s : 0.f;
    __syncthreads();
    float ss = (sq[lane] + sq[lane + 64]) + (sq[lane + 128] + sq[lane + 192]);      // every wave: the same bits
    ss = wave_sum(ss);
    const float nrm = sqrtf(ss);
    const int total = cnt[0] + cnt[1] + cnt[2] + cnt[3];
    if (e == 0) counts[k] = total;
    if (e < E) out[(size_t)k * E + e] = (total > 0 && nrm > eps) ? from_f<T>(s / nrm) : prev[(size_t)k * E + e];
}

int cs_check_shape(const char* what, int B, int N, int Lq, int Ld, int K) {
    POLUS_REQUIRE(Lq >= 1 && Lq <= CS_LMAX, "%s: need 1 <= Lq <= %d (got %d)", what, CS_LMAX, Lq);
    POLUS_REQUIRE(Ld >= 1 && Ld <= CS_LMAX, "%s: need 1 <= Ld <= %d (got %d)", what, CS_LMAX, Ld);
    POLUS_REQUIRE(K >= 1 && K <= CS_KMAX, "%s: need 1 <= K <= %d (got %d)", what, CS_KMAX, K);
    POLUS_REQUIRE(B >= 1 && B <= 65535, "%s: need 1 <= B <= 65535 (got %d)", what, B);
    POLUS_REQUIRE(N >= 1 && N <= 65535, "%s: need 1 <= N <= 65535 (got %d)", what, N);
    return POLUS_OK;
}

}  // namespace

extern "C" int polus_centroid_scores_route(int B, int N, int Lq, int Ld, int K, int* out) {
    const char* what = "polus_centroid_scores_route";
    if (int rc = cs_check_shape(what, B, N, Lq, Ld, K)) return rc;
    POLUS_REQUIRE(out, "%s: null pointer", what);
    const bool l = cs_lds_route(Lq, K);
    out[0] = l ? 1 : 2;
    out[1] = l ? (int)cs_lds_bytes(Lq, K) : 0;
    return POLUS_OK;
}

extern "C" int polus_centroid_scores(const float* table, long ldt, const int32_t* qmask, const uint16_t* codes,
                                     float* score, long lds, int B, int N, int Lq, int Ld, int K, void* stream) {
    const char* what = "polus_centroid_scores";
    if (int rc = cs_check_shape(what, B, N, Lq, Ld, K)) return rc;
    POLUS_REQUIRE(ldt >= (long)B * Lq, "%s: table row stride ldt must be >= B*Lq (got %ld < %ld)", what, ldt, (long)B * Lq);
    POLUS_REQUIRE(lds >= N, "%s: score row stride lds must be >= N (got %ld < %d)", what, lds, N);
    POLUS_REQUIRE(table && codes && score, "%s: null pointer", what);
    return cs_dispatch<false>(table, ldt, qmask, codes, nullptr, 0, N, score, lds, B, N, Lq, Ld, K,
                              static_cast<hipStream_t>(stream));
}

extern "C" int polus_centroid_scores_ids(const float* table, long ldt, const int32_t* qmask, const uint16_t* codes,
                                         const int32_t* cand, long ldc, float* score, long lds, int B, int C, int N, int Lq,
                                         int Ld, int K, void* stream) {
    const char* what = "polus_centroid_scores_ids";
    POLUS_REQUIRE(Lq >= 1 && Lq <= CS_LMAX, "%s: need 1 <= Lq <= %d (got %d)", what, CS_LMAX, Lq);
    POLUS_REQUIRE(Ld >= 1 && Ld <= CS_LMAX, "%s: need 1 <= Ld <= %d (got %d)", what, CS_LMAX, Ld);
    POLUS_REQUIRE(K >= 1 && K <= CS_KMAX, "%s: need 1 <= K <= %d (got %d)", what, CS_KMAX, K);
    POLUS_REQUIRE(B >= 1 && B <= 65535, "%s: need 1 <= B <= 65535 (got %d)", what, B);
    POLUS_REQUIRE(C >= 1 && C <= 65535, "%s: need 1 <= C <= 65535 (got %d)", what, C);
    POLUS_REQUIRE(N >= 1, "%s: need N >= 1 (got %d)", what, N);
    POLUS_REQUIRE(ldt >= (long)B * Lq, "%s: table row stride ldt must be >= B*Lq (got %ld < %ld)", what, ldt, (long)B * Lq);
    POLUS_REQUIRE(ldc >= C, "%s: candidate row stride ldc must be >= C (got %ld < %d)", what, ldc, C);
    POLUS_REQUIRE(lds >= C, "%s: score row stride lds must be >= C (got %ld < %d)", what, lds, C);
    POLUS_REQUIRE(table && codes && cand && score, "%s: null pointer", what);
    return cs_dispatch<true>(table, ldt, qmask, codes, cand, ldc, N, score, lds, B, C, Lq, Ld, K,
                             static_cast<hipStream_t>(stream));
}

extern "C" int polus_centroid_codes(const float* sim, long lds, const int32_t* mask, uint16_t* codes, int rows, int K,
                                    void* stream) {
    const char* what = "polus_centroid_codes";
    POLUS_REQUIRE(rows >= 1, "%s: need rows >= 1 (got %d)", what, rows);
    POLUS_REQUIRE(K >= 1 && K <= CS_KMAX, "%s: need 1 <= K <= %d (got %d)", what, CS_KMAX, K);
    POLUS_REQUIRE(lds >= K, "%s: row stride lds must be >= K (got %ld < %d)", what, lds, K);
    POLUS_REQUIRE(sim && codes, "%s: null pointer", what);
    hipLaunchKernelGGL(centroid_codes_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0,
                       static_cast<hipStream_t>(stream), sim, lds, mask, codes, rows, K);
    POLUS_CHECK_LAUNCH(what);
    return POLUS_OK;
}

extern "C" int polus_centroid_update(int dtype, const void* x, const uint16_t* codes, const void* prev, void* out,
                                     int32_t* counts, int T, int K, int E, float eps, void* stream) {
    const char* what = "polus_centroid_update";
    POLUS_REQUIRE(dtype == POLUS_F32 || dtype == POLUS_BF16, "%s: unknown dtype %d", what, dtype);
    POLUS_REQUIRE(E >= 32 && E <= CS_EMAX && E % 32 == 0, "%s: E must be a multiple of 32 in [32, %d] (got %d)", what,
                  CS_EMAX, E);
    POLUS_REQUIRE(T >= 1, "%s: need T >= 1 (got %d)", what, T);
    POLUS_REQUIRE(K >= 1 && K <= CS_KMAX, "%s: need 1 <= K <= %d (got %d)", what, CS_KMAX, K);
    POLUS_REQUIRE(x && codes && prev && out && counts, "%s: null pointer", what);
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (dtype == POLUS_BF16)
        hipLaunchKernelGGL(centroid_update_kernel<bf16_t>, dim3((unsigned)K), dim3(256), 0, st,
                           static_cast<const bf16_t*>(x), codes, static_cast<const bf16_t*>(prev),
                           static_cast<bf16_t*>(out), counts, T, E, eps);
    else
        hipLaunchKernelGGL(centroid_update_kernel<float>, dim3((unsigned)K), dim3(256), 0, st,
                           static_cast<const float*>(x), codes, static_cast<const float*>(prev),
                           static_cast<float*>(out), counts, T, E, eps);
    POLUS_CHECK_LAUNCH(what);
    return POLUS_OK;
}
