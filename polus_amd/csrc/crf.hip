// Linear-chain CRF for 17 <= C <= 128 tags (gfx950): one workgroup per sequence, lane j owns tag j.
// C <= 16 stays on the one-thread-per-sequence kernels of loss.hip; polus_crf_nll / polus_crf_viterbi
// (loss.hip) send the larger tag sets here.  Compile-time buckets C_PAD in {32, 64, 128}; padded tags
// carry exact zeros through every sum and are never read back.
//
// NLL: the scans run in the scaled domain.  E[k][j] = exp(T[k][j] - cmax_j) (cmax_j = column j's max;
// an all-masked column of -10000 entries stays finite) lives in LDS with a padded row stride, so that
// the forward's column reads (lane j, fixed k) and the backward's row reads (lane k, fixed j) are both
// free of bank conflicts.  alpha[j] = M + d[j] and beta[k] = N + e[k]: the parts M, N that every tag shares
// (and logZ) are doubles, uniform over the workgroup, the per-tag parts f32 of small magnitude, and the two
// are never added in f32.  alpha grows with S and with the potentials' scale; summed in f32 it rounds at its
// ulp every step (1e-3 at |alpha| = 1e4), and the marginals exp(alpha + beta - logZ) see that at full size.
// Per step:
//   forward   dm = max(d), a = exp(d - dm), M += dm, d'[j] = (pot[j] + cmax_j) + log(sum_k a[k] E[k][j])
//   backward  v = (pot + e) + cmax, vm = max(v), q = exp(v - vm), e'[k] = log(sum_j E[k][j] q[j]), N += vm
// (one GEMV plus C exps and C logs; M after its update is the step's largest alpha).  The forward stores a
// and dm per step in the workspace, the backward steps M back down by the same dm.  Marginals come back as
// a * exp(e + c), c = M + N - logZ (one double, rounded to f32 where it is used), pair marginals as E[k][j] *
// a_prev[k] * q[j] * exp(g), g = M_prev + N + vm - logZ: the lane owning row k keeps sum_s a_prev[k] q_s[j] exp(g_s) for every
// j in registers, and E multiplies the sum once at the end.  Gold counts are subtracted by the owning lane,
// the sequence's [C,C] slab goes to the workspace and a finalize launch sums the slabs in b order: no
// atomics, bitwise reproducible.
//
// Where the scaled domain runs out of range the same quantities are taken in the log domain, as loss.hip
// does for C <= 16, so that any finite f32 potentials give the float64 definition's result (confident
// emissions against a BIO mask: both allowed predecessors of an I-X tag more than 88 below the step's best
// tag, so that their a is 0 and the sum was once floored at FLT_MIN):
//   - a lane whose GEMV sum falls under CRF_RESCUE_SUM recomputes d'[j] = pot[j] + (lse_k(d[k] + T[k][j]) -
//     dm), resp. e'[k] = lse_j(T[k][j] + pot[j] + e[j]) - vm, from the step's d, resp. pot + e, kept in LDS
//     beside a, resp. q, and trans in global memory;
//   - where a is below FLT_MIN the workspace holds log a = d - dm in its place (negative, so the two cannot
//     be confused), and a marginal whose exponent e + c exceeds CRF_RESCUE_EXP is exp(log a + (e + c));
//   - at a step whose g exceeds CRF_RESCUE_EXP, a_prev * exp(g) would be 0 * inf: lane k adds
//     exp(log a_prev[k] + T[k][j] + pot[j] + e[j] + c_prev) straight into row k of the sequence's slab
//     (zeroed at the first such step) and folds the row in at the end.
// Under the two thresholds an underflowed factor costs a sum or a marginal at most e^-29 resp. e^-47 of
// its value, and the rescues change nothing.
//
// Viterbi: f32 max-plus, the same arithmetic and tie-break (first maximum over ascending k, first
// maximum for the final tag) as crf_viterbi_kernel; back-pointers as uint8 [B,S,C_PAD] in the
// workspace, one lane backtracks.
#include <float.h>
#include "common.h"

namespace {

template <int CP> struct CrfCfg {
    static constexpr int NT = CP < 64 ? 64 : CP;   // threads per workgroup (lanes >= C idle in the tag work)
    static constexpr int NW = NT / 64;
    static constexpr int LDE = CP + 1;              // E row stride (floats): rows start on distinct banks
    static constexpr size_t NLL_LDS = (size_t)(CP * LDE + 4 * CP + 8) * sizeof(float);
    static constexpr size_t VIT_LDS = (size_t)(CP * CP + 2 * CP) * sizeof(float);
};

__device__ __forceinline__ int clamp_tag(int t, int C) { return t < 0 ? 0 : (t >= C ? C - 1 : t); }

// A GEMV sum below this is recomputed in the log domain.  Far above the denormal range: whatever a or E flushed
// to zero (each factor < 2^-126 ~ e^-87) is below C * e^-29 of a sum that stays on the scaled path.
constexpr float CRF_RESCUE_SUM = 1e-25f;
// A scale exponent above this leaves the scaled products: below it an underflowed factor costs at most e^-47.
constexpr float CRF_RESCUE_EXP = 40.f;

// The workspace keeps per step and tag a = exp(d - dm), or where that is below FLT_MIN the negative log a =
// d - dm itself (the backward scan then takes a as 0).
// log a back from it, for the rescues alone: the empty asm is never executed speculatively, so the logf stays
// inside their branches and out of the common path.
__device__ __forceinline__ float crf_log_a(float v) {
    asm volatile("" : "+v"(v));
    return v < 0.f ? v : logf(v);
}

// max + log(sum(exp(. - max))) of v[i] + t[i * stride], i < n: the rescue of one lane, trans read from global memory
__device__ __forceinline__ float lse_rescue(const float* v, const float* __restrict__ t, int stride, int n) {
    float mx = -FLT_MAX;
    for (int i = 0; i < n; ++i) mx = fmaxf(mx, v[i] + t[(long)i * stride]);
    float sm = 0.f;
    for (int i = 0; i < n; ++i) sm += expf(v[i] + t[(long)i * stride] - mx);
    return mx + logf(sm);
}

// block-wide max / sum in fixed order.  red[slot], red[slot + 1] are written before the barrier; a caller
// separates two uses of the same slot by another barrier.
template <int NW> __device__ __forceinline__ float block_max(float v, float* red, int slot) {
    v = wave_max(v);
    if constexpr (NW == 1) {
        return v;
    } else {
        if ((threadIdx.x & 63) == 0) red[slot + (threadIdx.x >> 6)] = v;
        __syncthreads();
        return fmaxf(red[slot], red[slot + 1]);
    }
}
template <int NW> __device__ __forceinline__ float block_sum(float v, float* red, int slot) {
    v = wave_sum(v);
    if constexpr (NW == 1) {
        return v;
    } else {
        if ((threadIdx.x & 63) == 0) red[slot + (threadIdx.x >> 6)] = v;
        __syncthreads();
        return red[slot] + red[slot + 1];
    }
}

template <int CP, typename T>
__global__ __launch_bounds__(CrfCfg<CP>::NT) void crf_nll_wg_kernel(
        const float* __restrict__ pot, const int32_t* __restrict__ tags, const int32_t* __restrict__ lengths,
        const float* __restrict__ trans, const float* __restrict__ sw, float* __restrict__ nll_b, T* __restrict__ dpot,
        float* __restrict__ dtrans_b, float* __restrict__ ahat_ws, float* __restrict__ m_ws, int B, int S, int C) {
    using Cfg = CrfCfg<CP>;
    constexpr int NT = Cfg::NT, NW = Cfg::NW, LDE = Cfg::LDE;
    extern __shared__ __attribute__((aligned(16))) float lds[];
    float* E = lds;                      // [CP][LDE]
    float* vec = E + CP * LDE;           // [2][CP] double-buffered a (forward) / q (backward)
    float* lvec = vec + 2 * CP;          // [2][CP] the same steps' alpha (forward) / pot + beta (backward), for the rescues
    float* red = lvec + 2 * CP;          // [8]
    const int b = blockIdx.x, j = threadIdx.x;
    const bool live = j < C;             // C <= CP <= NT
    const float* x = pot + (long)b * S * C;
    const int32_t* t = tags + (long)b * S;
    T* dx = dpot + (long)b * S * C;
    float* dT = dtrans_b + (long)b * C * C;
    float* ah = ahat_ws + (long)b * S * CP;
    float* ms = m_ws + (long)b * S;
    int L = lengths ? lengths[b] : S;
    L = L < 0 ? 0 : (L > S ? S : L);
    const float wsw = sw ? sw[b] : 1.0f;
    const float w = wsw / (float)B;      // d(mean(-ll*w))/d(ll) = -w/B
    for (long i = (long)L * C + j; i < (long)S * C; i += NT) dx[i] = from_f<T>(0.f);
    if (L == 0) {
        for (int i = j; i < C * C; i += NT) dT[i] = 0.f;
        if (j == 0) nll_b[b] = 0.f;
        return;
    }

    // E = exp(T - column max), zero outside [C, C)
    float cmax = 0.f;
    if (live) {
        float mx = -FLT_MAX;
        for (int k = 0; k < C; ++k) mx = fmaxf(mx, trans[k * C + j]);
        cmax = mx;
    }
    if (j < CP)
        for (int k = 0; k < CP; ++k) E[k * LDE + j] = (live && k < C) ? expf(trans[k * C + j] - cmax) : 0.f;

    // d of step 0 (alpha itself: M starts at 0), loaded here so that the gold score's reduction has waited for it
    // before the forward loop
    const int jj = live ? j : 0;
    float d = live ? x[j] : -FLT_MAX;

    // gold path score
    float sc = 0.f;
    for (int s = j; s < L; s += NT) {
        const int ts = clamp_tag(t[s], C);
        sc += x[(long)s * C + ts];
        if (s + 1 < L) sc += trans[ts * C + clamp_tag(t[s + 1], C)];
    }
    const float score = block_sum<NW>(sc, red, 2);
    __syncthreads();                     // E complete; red[2..3] free again

    // forward.  The loops' global loads are unconditional (index clamped, idle lanes read tag 0) and a step ahead
    // of their use: the rescues' own loads make the compiler wait for everything in flight wherever it waits for
    // one load, so what a step waits for was issued a step before.
    float a_last = 0.f, va_last = 0.f;
    double M = 0.0;                      // uniform; after a step's update, that step's largest alpha
    for (int s = 0; s < L; ++s) {
        const float xn = x[(long)(s + 1 < L ? s + 1 : s) * C + jj];  // the last step's is not used
        const float dm = block_max<NW>(live ? d : -FLT_MAX, red, 0);
        const float la = d - dm;
        const float a = live ? expf(la) : 0.f;
        const float va = a >= FLT_MIN ? a : la;                     // a denormal a carries too few bits for its log
        if (live) ah[(long)s * CP + j] = va;
        if (j == 0) ms[s] = dm;
        M += (double)dm;
        if (s + 1 == L) { a_last = a; va_last = va; break; }
        float* av = vec + (s & 1) * CP;
        float* lv = lvec + (s & 1) * CP;
        if (j < CP) { av[j] = a; lv[j] = d; }
        __syncthreads();
        if (live) {
            float acc[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll 8
            for (int k = 0; k < CP; k += 4) {
                const float4 a4 = *reinterpret_cast<const float4*>(av + k);
                acc[0] = fmaf(a4.x, E[(k + 0) * LDE + j], acc[0]);
                acc[1] = fmaf(a4.y, E[(k + 1) * LDE + j], acc[1]);
                acc[2] = fmaf(a4.z, E[(k + 2) * LDE + j], acc[2]);
                acc[3] = fmaf(a4.w, E[(k + 3) * LDE + j], acc[3]);
            }
            const float sum = (acc[0] + acc[1]) + (acc[2] + acc[3]);
            if (sum >= CRF_RESCUE_SUM) d = (xn + cmax) + logf(sum);
            else d = xn + (lse_rescue(lv, trans + j, C, C) - dm);   // every predecessor far below the step's best tag
        }
    }
    const double logz = M + (double)logf(block_sum<NW>(a_last, red, 2));
    if (j == 0) nll_b[b] = -(score - (float)logz) * wsw;

    // backward + gradients
    float accT[CP];
#pragma unroll
    for (int i = 0; i < CP; ++i) accT[i] = 0.f;
    float e = 0.f, va_s = va_last, a_s = a_last;
    double c = M - logz;                 // uniform: M + N - logZ, M stepped back down by each dm, N up by each vm
    bool slab = false;                   // uniform: some step added its pair marginals to the slab directly
    __syncthreads();                     // lane 0's ms[] visible to every wave
    // what step s reads (a of s - 1, dm, pot and tag of s) is loaded during step s + 1, clamped at the bottom
    const int s0 = L >= 2 ? L - 2 : 0;
    float va_n = ah[(long)s0 * CP + jj], dm_n = ms[L - 1], x_n = x[(long)(L - 1) * C + jj];
    int t_n = t[L - 1];
    for (int s = L - 1; s >= 0; --s) {
        const float va_p = va_n, dm_s = dm_n, xs = x_n;
        const int ts = clamp_tag(t_n, C);
        const int s1 = s >= 1 ? s - 1 : 0, s2 = s >= 2 ? s - 2 : 0;
        va_n = ah[(long)s2 * CP + jj];
        dm_n = ms[s1];
        x_n = x[(long)s1 * C + jj];
        t_n = t[s1];
        if (live) {
            const float ec = e + (float)c;                          // beta + m - logZ
            float marg;
            if (ec > CRF_RESCUE_EXP) marg = expf(crf_log_a(va_s) + ec);     // = exp(alpha + beta - logZ)
            else marg = a_s * expf(ec);
            dx[(long)s * C + j] = from_f<T>((marg - (j == ts ? 1.0f : 0.0f)) * w);
        }
        if (s == 0) break;
        c -= (double)dm_s;                                          // M is now the largest alpha of step s - 1
        const float a_p = live ? fmaxf(va_p, 0.f) : 0.f;
        const float u = live ? xs + e : -FLT_MAX;
        const float v = live ? u + cmax : -FLT_MAX;
        const float vm = block_max<NW>(v, red, 0);
        float* qv = vec + (s & 1) * CP;
        float* uv = lvec + (s & 1) * CP;
        if (j < CP) { qv[j] = live ? expf(v - vm) : 0.f; uv[j] = u; }
        __syncthreads();
        const float cp = (float)c;
        c += (double)vm;
        const float g = (float)c;                                   // uniform over the workgroup
        const bool direct = g > CRF_RESCUE_EXP;
        if (direct) {
            // a_prev * exp(g) would be 0 * inf: this step's pair marginals go straight into the lane's slab row
            if (live) {
                float* row = dT + (long)j * C;
                const float* Tr = trans + (long)j * C;
                if (!slab)
                    for (int i = 0; i < C; ++i) row[i] = 0.f;
                const float la_p = crf_log_a(va_p);
                for (int i = 0; i < C; ++i) row[i] += expf((la_p + Tr[i] + uv[i]) + cp);
            }
            slab = true;
        }
        if (j < CP) {
            const float ck = direct ? 0.f : a_p * expf(g);
            const float* Er = E + j * LDE;
            float acc[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int i = 0; i < CP; i += 4) {
                const float4 q4 = *reinterpret_cast<const float4*>(qv + i);
                acc[0] = fmaf(Er[i + 0], q4.x, acc[0]);
                acc[1] = fmaf(Er[i + 1], q4.y, acc[1]);
                acc[2] = fmaf(Er[i + 2], q4.z, acc[2]);
                acc[3] = fmaf(Er[i + 3], q4.w, acc[3]);
                accT[i + 0] = fmaf(ck, q4.x, accT[i + 0]);
                accT[i + 1] = fmaf(ck, q4.y, accT[i + 1]);
                accT[i + 2] = fmaf(ck, q4.z, accT[i + 2]);
                accT[i + 3] = fmaf(ck, q4.w, accT[i + 3]);
            }
            const float sum = (acc[0] + acc[1]) + (acc[2] + acc[3]);
            if (sum >= CRF_RESCUE_SUM) e = logf(sum);
            else if (live) e = lse_rescue(uv, trans + (long)j * C, 1, C) - vm;
        }
        va_s = va_p;
        a_s = a_p;
    }
    // row k of the slab: E[k][.] * accT - gold counts, in place of E's row (each lane owns its row)
    if (j < CP) {
        float* Er = E + j * LDE;
#pragma unroll
        for (int i = 0; i < CP; ++i) Er[i] *= accT[i];
        if (live && slab) {
            const float* row = dT + (long)j * C;
            for (int i = 0; i < C; ++i) Er[i] += row[i];
        }
    }
    if (live)
        for (int s = 1; s < L; ++s)
            if (clamp_tag(t[s - 1], C) == j) E[j * LDE + clamp_tag(t[s], C)] -= 1.0f;
    __syncthreads();
    for (int i = j; i < C * C; i += NT) {
        const int k = i / C;
        dT[i] = E[k * LDE + (i - k * C)] * w;
    }
}

// loss = mean_b nll_b ; dtrans (+)= sum_b dtrans_b in b order
__global__ __launch_bounds__(256) void crf_wg_finalize_kernel(const float* __restrict__ nll_b, const float* __restrict__ dtrans_b,
                                                              int B, int C, float* __restrict__ loss,
                                                              float* __restrict__ dtrans, int accumulate) {
    const int k = blockIdx.x * 256 + threadIdx.x;
    const int cc = C * C;
    if (k < cc) {
        float s = 0.f;
        for (int b = 0; b < B; ++b) s += dtrans_b[(long)b * cc + k];
        dtrans[k] = accumulate ? dtrans[k] + s : s;
    }
    if (k == 0) {
        float s = 0.f;
        for (int b = 0; b < B; ++b) s += nll_b[b];
        *loss = s / (float)B;
    }
}

template <int CP>
__global__ __launch_bounds__(CrfCfg<CP>::NT) void crf_viterbi_wg_kernel(
        const float* __restrict__ pot, const int32_t* __restrict__ lengths, const float* __restrict__ trans,
        int32_t* __restrict__ out, uint8_t* __restrict__ back_ws, int B, int S, int C) {
    using Cfg = CrfCfg<CP>;
    constexpr int NT = Cfg::NT;
    constexpr int Q = CP / 4;
    extern __shared__ __attribute__((aligned(16))) float lds[];
    float* Tm = lds;                     // [CP][CP], zero outside [C, C)
    float* sv = Tm + CP * CP;            // [2][CP] double-buffered scores
    const int b = blockIdx.x, j = threadIdx.x;
    const bool live = j < C;
    const float* x = pot + (long)b * S * C;
    uint8_t* back = back_ws + (long)b * S * CP;
    int32_t* o = out + (long)b * S;
    int L = lengths ? lengths[b] : S;
    L = L < 0 ? 0 : (L > S ? S : L);
    for (int s = L + j; s < S; s += NT) o[s] = 0;
    if (L == 0) return;
    if (j < CP)
        for (int k = 0; k < CP; ++k) Tm[k * CP + j] = (live && k < C) ? trans[k * C + j] : 0.f;
    float score = live ? x[j] : -FLT_MAX;
    for (int s = 1; s < L; ++s) {
        const float xs = live ? x[(long)s * C + j] : 0.f;
        float* cur = sv + (s & 1) * CP;
        if (j < CP) cur[j] = score;      // padded tags: -FLT_MAX, never strictly above a real candidate
        __syncthreads();
        if (live) {
            // four chains over consecutive quarters of k, each keeping its first maximum; merged in
            // quarter order with a strict compare = the first maximum over ascending k
            float bv[4];
            int bi[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) { bv[r] = cur[r * Q] + Tm[(r * Q) * CP + j]; bi[r] = r * Q; }
#pragma unroll
            for (int i = 1; i < Q; ++i)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int k = r * Q + i;
                    const float v = cur[k] + Tm[k * CP + j];
                    if (v > bv[r]) { bv[r] = v; bi[r] = k; }
                }
#pragma unroll
            for (int r = 1; r < 4; ++r)
                if (bv[r] > bv[0]) { bv[0] = bv[r]; bi[0] = bi[r]; }
            back[(long)s * CP + j] = (uint8_t)bi[0];
            score = bv[0] + xs;
        }
    }
    float* fin = sv + (L & 1) * CP;
    if (j < CP) fin[j] = score;
    __syncthreads();
    if (j == 0) {
        int best = 0;
        float bv = fin[0];
        for (int c = 1; c < C; ++c) if (fin[c] > bv) { bv = fin[c]; best = c; }
        o[L - 1] = best;
        for (int s = L - 1; s > 0; --s) { best = back[(long)s * CP + best]; o[s - 1] = best; }
    }
}

inline int crf_bucket(int C) { return C <= 32 ? 32 : (C <= 64 ? 64 : 128); }

template <int CP>
int nll_launch(int dtype, const float* pot, const int32_t* tags, const int32_t* lengths, const float* trans,
               const float* sw, float* nll_b, void* dpot, float* dtb, float* ahat, float* m, int B, int S, int C,
               hipStream_t st) {
    using Cfg = CrfCfg<CP>;
    // not polus_launch_lds: the limit is raised on every call and only above 64 KiB here; folding it in would change when it is set per device
    auto kf = crf_nll_wg_kernel<CP, float>;
    auto kb = crf_nll_wg_kernel<CP, bf16_t>;
    if (dtype == POLUS_BF16) {
        if (Cfg::NLL_LDS > 64 * 1024)
            POLUS_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(kb), hipFuncAttributeMaxDynamicSharedMemorySize, (int)Cfg::NLL_LDS));
        hipLaunchKernelGGL(kb, dim3(B), dim3(Cfg::NT), Cfg::NLL_LDS, st, pot, tags, lengths, trans, sw, nll_b,
                           (bf16_t*)dpot, dtb, ahat, m, B, S, C);
    } else if (dtype == POLUS_F32) {
        if (Cfg::NLL_LDS > 64 * 1024)
            POLUS_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(kf), hipFuncAttributeMaxDynamicSharedMemorySize, (int)Cfg::NLL_LDS));
        hipLaunchKernelGGL(kf, dim3(B), dim3(Cfg::NT), Cfg::NLL_LDS, st, pot, tags, lengths, trans, sw, nll_b,
                           (float*)dpot, dtb, ahat, m, B, S, C);
    } else {
        POLUS_FAIL("polus_crf_nll: bad dtype");
    }
    POLUS_CHECK_LAUNCH("polus_crf_nll");
    return POLUS_OK;
}

template <int CP>
int viterbi_launch(const float* pot, const int32_t* lengths, const float* trans, int32_t* out, uint8_t* back,
                   int B, int S, int C, hipStream_t st) {
    using Cfg = CrfCfg<CP>;
    auto k = crf_viterbi_wg_kernel<CP>;
    if (Cfg::VIT_LDS > 64 * 1024)
        POLUS_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(k), hipFuncAttributeMaxDynamicSharedMemorySize, (int)Cfg::VIT_LDS));
    hipLaunchKernelGGL(k, dim3(B), dim3(Cfg::NT), Cfg::VIT_LDS, st, pot, lengths, trans, out, back, B, S, C);
    POLUS_CHECK_LAUNCH("polus_crf_viterbi");
    return POLUS_OK;
}

}  // namespace

// Workspace of the workgroup-per-sequence path: scaled alpha, or its log where that is below FLT_MIN, [B,S,C_PAD]
// (Viterbi: uint8 back-pointers in the same bytes) + each step's increment of the log scale [B,S] + per-sequence
// nll [B] + per-sequence dtrans [B,C,C], f32.
size_t polus_crf_wg_workspace_bytes(int B, int S, int C) {
    const int CP = crf_bucket(C);
    return ((size_t)B * S * CP + (size_t)B * S + (size_t)B + (size_t)B * C * C) * sizeof(float) + 64;
}

// 17 <= C <= 128; arguments already checked by polus_crf_nll (loss.hip)
int polus_crf_nll_wg(int dtype, const float* pot, const int32_t* tags, const int32_t* lengths, const float* trans,
                     const float* sw, float* loss, void* dpot, float* dtrans, int accumulate, int B, int S, int C,
                     void* workspace, hipStream_t st) {
    const int CP = crf_bucket(C);
    float* ahat = static_cast<float*>(workspace);
    float* m = ahat + (size_t)B * S * CP;
    float* nll_b = m + (size_t)B * S;
    float* dtb = nll_b + B;
    int rc = CP == 32 ? nll_launch<32>(dtype, pot, tags, lengths, trans, sw, nll_b, dpot, dtb, ahat, m, B, S, C, st)
           : CP == 64 ? nll_launch<64>(dtype, pot, tags, lengths, trans, sw, nll_b, dpot, dtb, ahat, m, B, S, C, st)
                      : nll_launch<128>(dtype, pot, tags, lengths, trans, sw, nll_b, dpot, dtb, ahat, m, B, S, C, st);
    if (rc != POLUS_OK) return rc;
    hipLaunchKernelGGL(crf_wg_finalize_kernel, dim3((C * C + 255) / 256), dim3(256), 0, st, nll_b, dtb, B, C, loss,
                       dtrans, accumulate);
    POLUS_CHECK_LAUNCH("polus_crf_nll(finalize)");
    return POLUS_OK;
}

int polus_crf_viterbi_wg(const float* pot, const int32_t* lengths, const float* trans, int32_t* out, int B, int S,
                         int C, void* workspace, hipStream_t st) {
    const int CP = crf_bucket(C);
    uint8_t* back = static_cast<uint8_t*>(workspace);
    return CP == 32 ? viterbi_launch<32>(pot, lengths, trans, out, back, B, S, C, st)
         : CP == 64 ? viterbi_launch<64>(pot, lengths, trans, out, back, B, S, C, st)
                    : viterbi_launch<128>(pot, lengths, trans, out, back, B, S, C, st);
}
