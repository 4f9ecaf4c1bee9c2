// Token-level late interaction (ColBERT MaxSim) and row L2 normalisation, forward and backward.
//
//   score[b, c]     = sum over valid i of max over valid j of <Q[b, i], D[c, j]>
//   argmax[b, c, i] = the winning j (lowest j on ties), -1 for an invalid query token or an empty document
//
// Forward: one workgroup per (document c, block of queries); each wave keeps UT 16-token query tiles of
// MFMA B fragments in registers.  The workgroup copies the document through two LDS buffers (the next stage's
// global loads in flight while the current one is multiplied) and every wave reads its 16-token tiles from there
// as A fragments, so an accumulator holds S[doc 16t + 4g + r][query token 16u + i] and the max over j is a
// per-lane running compare, closed by two cross-group shuffles.  The document mask sits in LDS too.  Only B*N
// scores and the argmax leave the chip; polus_maxsim_scores (corpus search) runs the same body without the argmax.
// Backward (no atomics, fixed summation orders):
//   dQ: one wave per query token, ascending c;
//   dD: one workgroup per (document, 64- or 32-wide column chunk), f32 accumulators in LDS; wave w of 16 owns
//       a sixteenth of the document tokens and adds the entries whose argmax falls there in ascending (b, i).
#include "maxsim_common.h"

namespace {

__device__ __forceinline__ void ms_pick(float& m, int& j, float m2, int j2) {
    if (m2 > m || (m2 == m && j2 < j)) { m = m2; j = j2; }
}

// a document row of T in the LDS stages of maxsim_common.h
template <typename T, int KS> using MsStage = MsStageB<32 * KS * (int)sizeof(T)>;

// The forward of both entry points.  ARGMAX = false (polus_maxsim_scores) compiles the argmax stores out and nothing
// else: the winning j is still tracked, because "no valid j" is how an empty document is told, so the scores are
// the same bits.
template <typename T, int KS, bool ARGMAX>
__device__ __forceinline__ void maxsim_fwd_body(const T* Q, const T* D, const int32_t* qmask, const int32_t* dmask,
                                                float* score, long lds, int32_t* argmax, int B, int N, int Lq, int Ld,
                                                int qpb) {
    using S = MsStage<T, KS>;
    constexpr int UT = MsTiles<T, KS>::UT;
    constexpr int E = 32 * KS;
    __shared__ float tsum[16 * 32];                           // per query tile: sum of its 16 maxima
    __shared__ __attribute__((aligned(16))) int smask[MS_LMAX];               // document mask, 0 past Ld
    __shared__ __attribute__((aligned(16))) unsigned char sd[2 * S::SR * S::RS];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int i = lane & 15, g = lane >> 4;
    const int c = blockIdx.x;
    const int b0 = blockIdx.y * qpb;
    const int nq = min(qpb, B - b0);
    const int nut = (Lq + 15) >> 4;                           // query tiles per query
    const int ntiles = nq * nut;
    const int nst = (Ld + S::SR - 1) / S::SR;                 // stages per document
    const unsigned char* Dc = reinterpret_cast<const unsigned char*>(D + (size_t)c * Ld * E);
    const int32_t* dm = dmask ? dmask + (size_t)c * Ld : nullptr;
    for (int j = threadIdx.x; j < nst * S::SR; j += 256) smask[j] = j < Ld && (!dm || dm[j] != 0);

    u32x4 stg[S::NCH];

    // every wave takes UT query tiles per round; all waves sweep the document together, stage by stage
    for (int r0w = 0; r0w < ntiles; r0w += 4 * UT) {
        const int u0 = r0w + wave * UT;
        const bool active = u0 < ntiles;                      // wave-uniform
        // B fragments of the query tiles u0 .. u0+UT-1 (rows past Lq / past the block re-read a valid row)
        Frag<T> qf[UT][KS];
#pragma unroll
        for (int u = 0; u < UT; ++u) {
            const int uu = min(u0 + u, ntiles - 1);
            const int bq = b0 + uu / nut;
            const int tok = min(((uu % nut) << 4) + i, Lq - 1);
            const unsigned char* p = reinterpret_cast<const unsigned char*>(Q + ((size_t)bq * Lq + tok) * E + 8 * g);
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) frag_load_row(qf[u][ks], p + ks * 32 * sizeof(T));
        }
        float m[UT];
        int jb[UT];
#pragma unroll
        for (int u = 0; u < UT; ++u) { m[u] = -INFINITY; jb[u] = MS_NOJ; }

        ms_gload<S>(stg, Dc, 0, Ld);
        ms_sstore<S>(stg, sd);
        __syncthreads();
        for (int st = 0; st < nst; ++st) {
            if (st + 1 < nst) ms_gload<S>(stg, Dc, st + 1, Ld);   // in flight while this stage is multiplied
            if (active) {
                const unsigned char* buf = sd + (st & 1) * S::SR * S::RS;
#pragma unroll
                for (int tt = 0; tt < S::SR / 16; ++tt) {
                    const int t16 = st * S::SR + tt * 16;
                    if (t16 >= Ld) break;                     // uniform
                    const int r0 = t16 + 4 * g;               // this lane's doc rows r0 .. r0+3
                    const int4 mk = *reinterpret_cast<const int4*>(&smask[r0]);
                    const bool tile_full = __all(mk.x & mk.y & mk.z & mk.w);
                    const unsigned char* p = buf + (tt * 16 + i) * S::RS + 8 * g * sizeof(T);
                    f32x4 acc[UT];
#pragma unroll
                    for (int u = 0; u < UT; ++u) acc[u] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
                    for (int ks = 0; ks < KS; ++ks) {
                        Frag<T> df;
                        frag_load_row(df, p + ks * 32 * sizeof(T));
#pragma unroll
                        for (int u = 0; u < UT; ++u) mma16(acc[u], df, qf[u][ks]);
                    }
                    // ascending j per lane: a strict > keeps the lowest j of equal values
                    if (tile_full) {
#pragma unroll
                        for (int u = 0; u < UT; ++u)
#pragma unroll
                            for (int r = 0; r < 4; ++r)
                                if (acc[u][r] > m[u]) { m[u] = acc[u][r]; jb[u] = r0 + r; }
                    } else {
                        const bool ok[4] = {mk.x != 0, mk.y != 0, mk.z != 0, mk.w != 0};
#pragma unroll
                        for (int u = 0; u < UT; ++u)
#pragma unroll
                            for (int r = 0; r < 4; ++r)
                                if (ok[r] && acc[u][r] > m[u]) { m[u] = acc[u][r]; jb[u] = r0 + r; }
                    }
                }
            }
            // into the buffer every wave finished reading before the last barrier
            if (st + 1 < nst) ms_sstore<S>(stg, sd + ((st + 1) & 1) * S::SR * S::RS);
            __syncthreads();
        }
        if (!active) continue;

#pragma unroll
        for (int u = 0; u < UT; ++u) {
            float mu = m[u];
            int ju = jb[u];
#pragma unroll
            for (int o = 16; o <= 32; o <<= 1) {
                const float m2 = __shfl_xor(mu, o, 64);
                const int j2 = __shfl_xor(ju, o, 64);
                ms_pick(mu, ju, m2, j2);
            }
            const int uu = u0 + u;
            float contrib = 0.f;
            if (uu < ntiles) {
                const int bq = b0 + uu / nut;
                const int tok = ((uu % nut) << 4) + i;
                const bool qv = tok < Lq && (!qmask || qmask[(size_t)bq * Lq + tok] != 0);
                const bool hit = qv && ju != MS_NOJ;
                if constexpr (ARGMAX)
                    if (g == 0 && tok < Lq) argmax[((size_t)bq * N + c) * Lq + tok] = hit ? ju : -1;
                contrib = hit ? mu : 0.f;
            }
            // sum of the tile's 16 maxima (lanes 0..15; every group holds the same values)
#pragma unroll
            for (int o = 1; o < 16; o <<= 1) contrib += __shfl_xor(contrib, o, 64);
            if (lane == 0 && uu < ntiles) tsum[uu] = contrib;
        }
    }
    __syncthreads();
    if ((int)threadIdx.x < nq) {
        float s = 0.f;
        for (int t = 0; t < nut; ++t) s += tsum[threadIdx.x * nut + t];
        score[(size_t)(b0 + threadIdx.x) * lds + c] = s;
    }
}

template <typename T, int KS>
__global__ __launch_bounds__(256) void maxsim_fwd_kernel(const T* __restrict__ Q, const T* __restrict__ D,
                                                         const int32_t* __restrict__ qmask,
                                                         const int32_t* __restrict__ dmask,
                                                         float* __restrict__ score, long lds,
                                                         int32_t* __restrict__ argmax, int B, int N, int Lq,
                                                         int Ld, int qpb) {
    maxsim_fwd_body<T, KS, true>(Q, D, qmask, dmask, score, lds, argmax, B, N, Lq, Ld, qpb);
}

template <typename T, int KS>
__global__ __launch_bounds__(256) void maxsim_scores_kernel(const T* __restrict__ Q, const T* __restrict__ D,
                                                            const int32_t* __restrict__ qmask,
                                                            const int32_t* __restrict__ dmask,
                                                            float* __restrict__ score, long lds, int B, int N, int Lq,
                                                            int Ld, int qpb) {
    maxsim_fwd_body<T, KS, false>(Q, D, qmask, dmask, score, lds, nullptr, B, N, Lq, Ld, qpb);
}

// dQ[b, i, :] = sum over c ascending of dscore[b, c] * D[c, argmax[b, c, i], :]; one wave per query token
template <typename T>
__global__ __launch_bounds__(256) void maxsim_bwd_dq_kernel(const T* __restrict__ D, const float* __restrict__ dscore,
                                                            long lds, const int32_t* __restrict__ argmax,
                                                            T* __restrict__ dQ, int B, int N, int Lq, int Ld, int E) {
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);                 // b * Lq + i (B * Lq < 2^25)
    if (row >= B * Lq) return;
    const int b = row / Lq, i = row % Lq;
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
    for (int c0 = 0; c0 < N; c0 += 64) {
        const int cl = c0 + lane;
        const int jv = cl < N ? argmax[((size_t)b * N + cl) * Lq + i] : -1;
        const float dv = cl < N ? dscore[(size_t)b * lds + cl] : 0.f;
        const int n = min(64, N - c0);
        for (int l0 = 0; l0 < n; l0 += 8) {
            float x[8][4];
            int js[8];
#pragma unroll
            for (int q = 0; q < 8; ++q) {
                const int l = min(l0 + q, n - 1);
                js[q] = __builtin_amdgcn_readlane(jv, l);
                const T* dr = D + ((size_t)(c0 + l) * Ld + min(max(js[q], 0), Ld - 1)) * E;
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const int e = lane + 64 * k;
                    x[q][k] = e < E ? to_f<T>(dr[e]) : 0.f;
                }
            }
#pragma unroll
            for (int q = 0; q < 8; ++q) {
                if (l0 + q < n && js[q] >= 0 && js[q] < Ld) {
                    const float ds = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, dv), l0 + q));
#pragma unroll
                    for (int k = 0; k < 4; ++k) acc[k] = fmaf(ds, x[q][k], acc[k]);
                }
            }
        }
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int e = lane + 64 * k;
        if (e < E) dQ[(size_t)row * E + e] = from_f<T>(acc[k]);
    }
}

// dD[c, j, e0 .. e0+ec) = sum over (b, i) ascending with argmax[b, c, i] == j of dscore[b, c] * Q[b, i, :]
constexpr int DD_WAVES = 16;

template <typename T>
__global__ __launch_bounds__(64 * DD_WAVES) void maxsim_bwd_dd_kernel(const T* __restrict__ Q, const float* __restrict__ dscore,
                                                            long lds, const int32_t* __restrict__ argmax,
                                                            T* __restrict__ dD, int B, int N, int Lq, int Ld, int E,
                                                            int ec) {
    __shared__ float acc[16384];                                  // [Ld][ec], Ld * ec <= 16384
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int c = blockIdx.x;
    const int e0 = blockIdx.y * ec;
    const int e = e0 + lane;
    const bool col = lane < ec && e < E;
    for (int k = threadIdx.x; k < Ld * ec; k += 64 * DD_WAVES) acc[k] = 0.f;
    __syncthreads();
    const int j0 = wave * Ld / DD_WAVES, j1 = (wave + 1) * Ld / DD_WAVES;
    const int total = B * Lq;                                    // < 2^25
    for (int n0 = 0; n0 < total; n0 += 64) {
        const int n = n0 + lane;
        int key = -1;
        if (n < total) {
            const int b = n / Lq, i = n % Lq;
            key = argmax[((size_t)b * N + c) * Lq + i];
        }
        unsigned long long mine = __ballot(key >= j0 && key < j1);
        while (mine) {
            // up to 16 entries at a time: loads first, then the in-order LDS updates
            constexpr int NB = 16;
            int ls[NB];
            int cnt = 0;
#pragma unroll
            for (int q = 0; q < NB; ++q) {
                ls[q] = mine ? (int)__builtin_ctzll(mine) : -1;
                if (mine) { mine &= mine - 1; ++cnt; }
            }
            float x[NB], ds[NB];
            int js[NB];
#pragma unroll
            for (int q = 0; q < NB; ++q) {
                const int l = ls[q] < 0 ? ls[0] : ls[q];
                const int nn = n0 + l;
                const int b = nn / Lq, i = nn % Lq;
                js[q] = __builtin_amdgcn_readlane(key, l);
                ds[q] = dscore[(size_t)b * lds + c];
                x[q] = col ? to_f<T>(Q[((size_t)b * Lq + i) * E + e]) : 0.f;
            }
#pragma unroll
            for (int q = 0; q < NB; ++q) {
                if (q < cnt && col) {
                    float* a = &acc[js[q] * ec + lane];
                    *a = fmaf(ds[q], x[q], *a);
                }
            }
        }
    }
    __syncthreads();
    for (int k = threadIdx.x; k < Ld * ec; k += 64 * DD_WAVES) {
        const int j = k / ec, el = k - j * ec;
        if (e0 + el < E) dD[((size_t)c * Ld + j) * E + e0 + el] = from_f<T>(acc[k]);
    }
}

// y = x / max(|x|, eps) (f32 arithmetic), rnorm = 1 / max(|x|, eps); one wave per row
template <typename T>
__global__ __launch_bounds__(256) void l2norm_fwd_kernel(const T* __restrict__ x, T* __restrict__ y,
                                                         float* __restrict__ rnorm, int rows, int E, float eps) {
    const int lane = threadIdx.x & 63;
    const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    float v[4], ss = 0.f;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int e = lane + 64 * k;
        v[k] = e < E ? to_f<T>(x[(size_t)row * E + e]) : 0.f;
        ss = fmaf(v[k], v[k], ss);
    }
    ss = wave_sum(ss);
    const float rn = 1.0f / fmaxf(sqrtf(ss), eps);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int e = lane + 64 * k;
        if (e < E) y[(size_t)row * E + e] = from_f<T>(v[k] * rn);
    }
    if (lane == 0) rnorm[row] = rn;
}

// dx = (dy - y <y, dy>) * rnorm where |x| > eps, dy / eps otherwise
template <typename T>
__global__ __launch_bounds__(256) void l2norm_bwd_kernel(const T* __restrict__ y, const float* __restrict__ rnorm,
                                                         const T* __restrict__ dy, T* __restrict__ dx, int rows, int E,
                                                         float eps) {
    const int lane = threadIdx.x & 63;
    const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    float yv[4], gv[4], dot = 0.f;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int e = lane + 64 * k;
        yv[k] = e < E ? to_f<T>(y[(size_t)row * E + e]) : 0.f;
        gv[k] = e < E ? to_f<T>(dy[(size_t)row * E + e]) : 0.f;
        dot = fmaf(yv[k], gv[k], dot);
    }
    dot = wave_sum(dot);
    const float rn = rnorm[row];
    const bool inner = rn < 1.0f / eps;                           // forward took |x| > eps
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int e = lane + 64 * k;
        if (e < E) dx[(size_t)row * E + e] = from_f<T>(inner ? (gv[k] - yv[k] * dot) * rn : gv[k] * rn);
    }
}

int ms_check(const char* what, int dtype, int B, int N, int Lq, int Ld, int E, long lds, bool with_argmax = true) {
    int rc = ms_shape_check(what, dtype, B, Lq, Ld, E);
    if (rc != POLUS_OK) return rc;
    POLUS_REQUIRE(N >= 1 && N <= 65535, "%s: need 1 <= N <= 65535 (got %d)", what, N);
    POLUS_REQUIRE(!with_argmax || (long long)B * N * Lq < (1LL << 31), "%s: B*N*Lq must be < 2^31 (got %lld)", what,
                  (long long)B * N * Lq);
    POLUS_REQUIRE(lds >= N, "%s: score row stride lds must be >= N (got %ld < %d)", what, lds, N);
    return POLUS_OK;
}

// am == nullptr: polus_maxsim_scores (polus_maxsim_fwd refuses a null argmax)
void fwd_dispatch(int dtype, int E, const void* Q, const void* D, const int32_t* qm, const int32_t* dm, float* score,
                  long lds, int32_t* am, int B, int N, int Lq, int Ld, hipStream_t st) {
    ms_dispatch(dtype, E, [&](auto t, auto ks) {
        using T = typename decltype(t)::type;
        constexpr int KS = decltype(ks)::value;
        const int qpb = ms_queries_per_block<T, KS>(B, N, Lq);
        dim3 grid(N, (B + qpb - 1) / qpb);
        if (am)
            hipLaunchKernelGGL((maxsim_fwd_kernel<T, KS>), grid, dim3(256), 0, st, static_cast<const T*>(Q),
                               static_cast<const T*>(D), qm, dm, score, lds, am, B, N, Lq, Ld, qpb);
        else
            hipLaunchKernelGGL((maxsim_scores_kernel<T, KS>), grid, dim3(256), 0, st, static_cast<const T*>(Q),
                               static_cast<const T*>(D), qm, dm, score, lds, B, N, Lq, Ld, qpb);
    });
}

template <typename T>
void bwd_launch(const void* Q, const void* D, const float* ds, long lds, const int32_t* am, void* dQ, void* dD, int B,
                int N, int Lq, int Ld, int E, hipStream_t st) {
    const int rows = B * Lq;
    hipLaunchKernelGGL(maxsim_bwd_dq_kernel<T>, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, st,
                       static_cast<const T*>(D), ds, lds, am, static_cast<T*>(dQ), B, N, Lq, Ld, E);
    const int ec = Ld <= 256 ? 64 : 32;
    hipLaunchKernelGGL(maxsim_bwd_dd_kernel<T>, dim3(N, (E + ec - 1) / ec), dim3(64 * DD_WAVES), 0, st,
                       static_cast<const T*>(Q), ds, lds, am, static_cast<T*>(dD), B, N, Lq, Ld, E, ec);
}

}  // namespace

extern "C" int polus_maxsim_fwd(int dtype, const void* Q, const void* D, const int32_t* qmask, const int32_t* dmask,
                                float* score, long lds, int32_t* argmax, int B, int N, int Lq, int Ld, int E,
                                void* stream) {
    int rc = ms_check("polus_maxsim_fwd", dtype, B, N, Lq, Ld, E, lds);
    if (rc != POLUS_OK) return rc;
    POLUS_REQUIRE(Q && D && score && argmax, "polus_maxsim_fwd: null pointer");
    POLUS_REQUIRE(polus_aligned16(Q) && polus_aligned16(D), "polus_maxsim_fwd: Q and D must be 16-byte aligned");
    fwd_dispatch(dtype, E, Q, D, qmask, dmask, score, lds, argmax, B, N, Lq, Ld, static_cast<hipStream_t>(stream));
    POLUS_CHECK_LAUNCH("polus_maxsim_fwd");
    return POLUS_OK;
}

extern "C" int polus_maxsim_scores(int dtype, const void* Q, const void* D, const int32_t* qmask, const int32_t* dmask,
                                   float* score, long lds, int B, int N, int Lq, int Ld, int E, void* stream) {
    int rc = ms_check("polus_maxsim_scores", dtype, B, N, Lq, Ld, E, lds, false);
    if (rc != POLUS_OK) return rc;
    POLUS_REQUIRE(Q && D && score, "polus_maxsim_scores: null pointer");
    POLUS_REQUIRE(polus_aligned16(Q) && polus_aligned16(D), "polus_maxsim_scores: Q and D must be 16-byte aligned");
    fwd_dispatch(dtype, E, Q, D, qmask, dmask, score, lds, nullptr, B, N, Lq, Ld, static_cast<hipStream_t>(stream));
    POLUS_CHECK_LAUNCH("polus_maxsim_scores");
    return POLUS_OK;
}

extern "C" int polus_maxsim_bwd(int dtype, const void* Q, const void* D, const float* dscore, long lds,
                                const int32_t* argmax, void* dQ, void* dD, int B, int N, int Lq, int Ld, int E,
                                void* stream) {
    int rc = ms_check("polus_maxsim_bwd", dtype, B, N, Lq, Ld, E, lds);
    if (rc != POLUS_OK) return rc;
    POLUS_REQUIRE(Q && D && dscore && argmax && dQ && dD, "polus_maxsim_bwd: null pointer");
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (dtype == POLUS_BF16)
        bwd_launch<bf16_t>(Q, D, dscore, lds, argmax, dQ, dD, B, N, Lq, Ld, E, st);
    else
        bwd_launch<float>(Q, D, dscore, lds, argmax, dQ, dD, B, N, Lq, Ld, E, st);
    POLUS_CHECK_LAUNCH("polus_maxsim_bwd");
    return POLUS_OK;
}

extern "C" int polus_l2norm_fwd(int dtype, const void* x, void* y, float* rnorm, int rows, int E, float eps,
                                void* stream) {
    POLUS_REQUIRE(dtype == POLUS_F32 || dtype == POLUS_BF16, "polus_l2norm_fwd: unknown dtype %d", dtype);
    POLUS_REQUIRE(rows >= 1 && E >= 1 && E <= MS_EMAX, "polus_l2norm_fwd: need rows >= 1 and 1 <= E <= %d (got %d, %d)",
                  MS_EMAX, rows, E);
    POLUS_REQUIRE(eps > 0.f, "polus_l2norm_fwd: eps must be > 0");
    POLUS_REQUIRE(x && y && rnorm, "polus_l2norm_fwd: null pointer");
    hipStream_t st = static_cast<hipStream_t>(stream);
    const dim3 grid((unsigned)(((long)rows + 3) / 4));
    if (dtype == POLUS_BF16)
        hipLaunchKernelGGL(l2norm_fwd_kernel<bf16_t>, grid, dim3(256), 0, st, static_cast<const bf16_t*>(x),
                           static_cast<bf16_t*>(y), rnorm, rows, E, eps);
    else
        hipLaunchKernelGGL(l2norm_fwd_kernel<float>, grid, dim3(256), 0, st, static_cast<const float*>(x),
                           static_cast<float*>(y), rnorm, rows, E, eps);
    POLUS_CHECK_LAUNCH("polus_l2norm_fwd");
    return POLUS_OK;
}

extern "C" int polus_l2norm_bwd(int dtype, const void* y, const float* rnorm, const void* dy, void* dx, int rows, int E,
                                float eps, void* stream) {
    POLUS_REQUIRE(dtype == POLUS_F32 || dtype == POLUS_BF16, "polus_l2norm_bwd: unknown dtype %d", dtype);
    POLUS_REQUIRE(rows >= 1 && E >= 1 && E <= MS_EMAX, "polus_l2norm_bwd: need rows >= 1 and 1 <= E <= %d (got %d, %d)",
                  MS_EMAX, rows, E);
    POLUS_REQUIRE(eps > 0.f, "polus_l2norm_bwd: eps must be > 0");
    POLUS_REQUIRE(y && rnorm && dy && dx, "polus_l2norm_bwd: null pointer");
    hipStream_t st = static_cast<hipStream_t>(stream);
    const dim3 grid((unsigned)(((long)rows + 3) / 4));
    if (dtype == POLUS_BF16)
        hipLaunchKernelGGL(l2norm_bwd_kernel<bf16_t>, grid, dim3(256), 0, st, static_cast<const bf16_t*>(y), rnorm,
                           static_cast<const bf16_t*>(dy), static_cast<bf16_t*>(dx), rows, E, eps);
    else
        hipLaunchKernelGGL(l2norm_bwd_kernel<float>, grid, dim3(256), 0, st, static_cast<const float*>(y), rnorm,
                           static_cast<const float*>(dy), static_cast<float*>(dx), rows, E, eps);
    POLUS_CHECK_LAUNCH("polus_l2norm_bwd");
    return POLUS_OK;
}
