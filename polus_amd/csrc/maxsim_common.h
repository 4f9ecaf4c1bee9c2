// What the MaxSim kernels share: maxsim.hip (training forward, corpus scores), rerank.hip (candidate lists),
// maxsim_fp8.hip (the same two over an FP8 token index), residual.hip (candidate lists over a residual-compressed
// index) and tuples.hip (every query against its own n documents).
// Device side, what must be the same in all of them for their scores to agree bit for bit: how many query tiles a
// wave holds (MsTiles), how a query tile becomes B fragments (rr_query_load), how a document's mask becomes per-tile
// bit words (rr_mask_load, rr_mask_pack), how a document tile is loaded and meets the query's fragments (rr_tile_load,
// rr_tile_max), and the LDS stages of the corpus-score kernels (MsStageB, ms_gload, ms_sstore).  The streaming loop of
// the rerank kernels, the corpus-score body and the tile reduce (max across the row groups xor 16, 32; the value where
// the query token counts; the 16-lane xor-shuffle sum) are still written out per kernel: moved into a shared
// __forceinline__ function they compile to other code than in place (profiles/maxsim_family_refactor.txt), so a
// change to one of them has to be made in every kernel that has it.
// Host side, once for the family: the argument checks with their messages (ms_shape_check, rr_args_check), the
// dispatch on dtype and E / 32 (ms_dispatch), the in-register route's condition (ms_query_fits), the
// queries-per-workgroup rule (ms_queries_per_block) and the rerank launch (rr_docs_per_wave, rr_launch).
#pragma once
#include <type_traits>

#include "common.h"

constexpr int MS_LMAX = 512;            // Lq, Ld limit
constexpr int MS_EMAX = 256;            // E limit (multiple of 32)
constexpr int MS_NOJ = 0x7fffffff;      // "no valid j yet" while reducing with the winning j

constexpr int RR_MAXDPW = 8;            // rerank: documents per wave, at most

// query tiles held per wave: the B fragments of UT tiles x KS k-steps stay within 64 (bf16) VGPRs
template <typename T, int KS> struct MsTiles {
    static constexpr int FR = sizeof(T) == 2 ? 4 : 8;           // VGPRs per fragment
    static constexpr int U = (64 / FR) / KS;
    static constexpr int UT = U < 1 ? 1 : (U > 8 ? 8 : U);
};

typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));

// document rows staged in LDS: SR rows per buffer (two buffers), rows padded by 16 B so that the 16 rows of a
// fragment read fall into distinct banks; the workgroup copies a stage with 16-B loads, NCH per thread
template <int ROWB_> struct MsStageB {
    static constexpr int ROWB = ROWB_;                           // bytes of one document row
    static constexpr int RS = ROWB + 16;                         // LDS row stride
    static constexpr int SR = ROWB <= 512 ? 32 : 16;             // rows per stage
    static constexpr int CPR = ROWB / 16;                        // 16-B chunks per row
    static constexpr int NCH = (SR * CPR + 255) / 256;           // chunks per thread per stage
};

// stage st of a document: global -> registers, 16 B per chunk (rows past Ld re-read row Ld-1)
template <typename S>
__device__ __forceinline__ void ms_gload(u32x4* stg, const unsigned char* Dc, int st, int Ld) {
#pragma unroll
    for (int k = 0; k < S::NCH; ++k) {
        // unconditional (a clamped chunk past the stage): no branch, so nothing waits for the load here
        const int ch = min((int)threadIdx.x + 256 * k, S::SR * S::CPR - 1);
        const int row = min(st * S::SR + ch / S::CPR, Ld - 1);
        stg[k] = *reinterpret_cast<const u32x4*>(Dc + (size_t)row * S::ROWB + (ch % S::CPR) * 16);
    }
}

// registers -> one LDS stage buffer
template <typename S>
__device__ __forceinline__ void ms_sstore(const u32x4* stg, unsigned char* buf) {
#pragma unroll
    for (int k = 0; k < S::NCH; ++k) {
        const int ch = threadIdx.x + 256 * k;
        if (ch < S::SR * S::CPR)
            *reinterpret_cast<u32x4*>(buf + (ch / S::CPR) * S::RS + (ch % S::CPR) * 16) = stg[k];
    }
}

// raw document mask, token 64 k + lane in mv[k], for use a whole document later: the loads are unconditional (tokens
// past Ld re-read token Ld - 1), because a load under a per-lane condition is waited for where it is issued
__device__ __forceinline__ void rr_mask_load(int (&mv)[8], const int32_t* dm, int lane, int Ld) {
    if (dm) {                                                 // uniform
#pragma unroll
        for (int k = 0; k < 8; ++k) mv[k] = dm[min(64 * k + lane, Ld - 1)];
    } else {
#pragma unroll
        for (int k = 0; k < 8; ++k) mv[k] = 1;
    }
}

// tm: lane t < 32 holds the 16 mask bits of document tile t; nvt: tiles up to the last valid token (0 for an absent
// document)
__device__ __forceinline__ void rr_mask_pack(const int (&mv)[8], bool present, int lane, int Ld, unsigned& tm, int& nvt) {
    tm = 0;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const unsigned long long bk = __ballot(present && 64 * k + lane < Ld && mv[k] != 0);
        if ((lane >> 2) == k) tm = (unsigned)(bk >> (16 * (lane & 3))) & 0xffffu;
    }
    const unsigned long long nz = __ballot(tm != 0);
    nvt = nz ? 64 - (int)__builtin_clzll(nz) : 0;
}

// B fragments of the query tiles r0 .. r0 + UT - 1 (tiles past the query and rows past Lq re-read a valid row) and
// whether this lane's token of each tile counts
template <typename T, int KS, int UT>
__device__ __forceinline__ void rr_query_load(Frag<T> (&qf)[UT][KS], bool (&qok)[UT], const T* Qb, const int32_t* qm,
                                              int r0, int nut, int Lq, int i, int g) {
#pragma unroll
    for (int u = 0; u < UT; ++u) {
        const int tok = 16 * (r0 + u) + i;
        const int tk = min(16 * min(r0 + u, nut - 1) + i, Lq - 1);
        const unsigned char* p = reinterpret_cast<const unsigned char*>(Qb + (size_t)tk * (32 * KS) + 8 * g);
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) frag_load_row(qf[u][ks], p + ks * 32 * sizeof(T));
        const bool on = !qm || qm[min(tok, Lq - 1)] != 0;
        qok[u] = tok < Lq && on;
    }
}

// A fragments of document tile t: lane (i, g) takes row 16 t + i (rows past Ld re-read row Ld - 1), k = 8 g .. 8 g + 7
// of every 32-wide k-step.  `base` is the document's first row plus this lane's 8 g elements.
template <typename T, int KS>
__device__ __forceinline__ void rr_tile_load(Frag<T> (&f)[KS], const unsigned char* base, int t, int i, int Ld) {
    const unsigned char* p = base + (size_t)min(16 * t + i, Ld - 1) * (32 * KS * sizeof(T));
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) frag_load_row(f[ks], p + ks * 32 * sizeof(T));
}

// one document tile against the wave's nu query tiles: m[u] = max(m[u], products of the valid rows).  bits: the
// tile's 16 mask bits shifted to this lane's rows 4 g .. 4 g + 3
template <typename T, int KS, int UT>
__device__ __forceinline__ void rr_tile_max(float (&m)[UT], const Frag<T> (&df)[KS], const Frag<T> (&qf)[UT][KS],
                                            unsigned bits, int nu) {
#pragma unroll
    for (int u = 0; u < UT; ++u) {
        if (u < nu) {                                         // uniform
            f32x4 acc = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) mma16(acc, df[ks], qf[u][ks]);
#pragma unroll
            for (int r = 0; r < 4; ++r)
                if (((bits >> r) & 1u) && acc[r] > m[u]) m[u] = acc[r];
        }
    }
}

// ---------------------------------------------------------------- host side
// the checks every entry point of the family makes first, in this order
static inline int ms_shape_check(const char* what, int dtype, int B, int Lq, int Ld, int E) {
    POLUS_REQUIRE(dtype == POLUS_F32 || dtype == POLUS_BF16, "%s: unknown dtype %d", what, dtype);
    POLUS_REQUIRE(E >= 32 && E <= MS_EMAX && E % 32 == 0, "%s: E must be a multiple of 32 in [32, %d] (got %d)", what,
                  MS_EMAX, E);
    POLUS_REQUIRE(Lq >= 1 && Lq <= MS_LMAX, "%s: need 1 <= Lq <= %d (got %d)", what, MS_LMAX, Lq);
    POLUS_REQUIRE(Ld >= 1 && Ld <= MS_LMAX, "%s: need 1 <= Ld <= %d (got %d)", what, MS_LMAX, Ld);
    POLUS_REQUIRE(B >= 1 && B <= 65535, "%s: need 1 <= B <= 65535 (got %d)", what, B);
    return POLUS_OK;
}

// a rerank's candidate lists [B, C] (row stride ldc) over a corpus of N documents and its scores (row stride lds)
static inline int rr_args_check(const char* what, int C, int N, long ldc, long lds) {
    POLUS_REQUIRE(C >= 1 && C <= 65535, "%s: need 1 <= C <= 65535 (got %d)", what, C);
    POLUS_REQUIRE(N >= 1, "%s: need 1 <= N <= 2^31 - 1 (got %d)", what, N);
    POLUS_REQUIRE(ldc >= C, "%s: candidate row stride ldc must be >= C (got %ld < %d)", what, ldc, C);
    POLUS_REQUIRE(lds >= C, "%s: score row stride lds must be >= C (got %ld < %d)", what, lds, C);
    return POLUS_OK;
}

// f(MsType<T>{}, std::integral_constant<int, E / 32>{}) for a dtype and an E that ms_shape_check has passed: the one
// place where the family's kernels are instantiated over T and KS
template <typename T> struct MsType { using type = T; };

template <typename F> void ms_dispatch(int dtype, int E, F&& f) {
    const auto by_ks = [&](auto t) {
        switch (E / 32) {
#define MS_KS_CASE(KS_) f(t, std::integral_constant<int, KS_>{}); break
        case 1: MS_KS_CASE(1);
        case 2: MS_KS_CASE(2);
        case 3: MS_KS_CASE(3);
        case 4: MS_KS_CASE(4);
        case 5: MS_KS_CASE(5);
        case 6: MS_KS_CASE(6);
        case 7: MS_KS_CASE(7);
        default: MS_KS_CASE(8);
#undef MS_KS_CASE
        }
    };
    if (dtype == POLUS_BF16) by_ks(MsType<bf16_t>{});
    else by_ks(MsType<float>{});
}

// does the whole query stay in one wave's registers (the RES = true kernels)?
template <typename T, int KS> bool ms_query_fits(int Lq) { return (Lq + 15) / 16 <= MsTiles<T, KS>::UT; }

// corpus scores: queries per workgroup: one round of 4 x UT query tiles where the queries are short (at most 16
// queries), halved while that leaves fewer than 512 workgroups
template <typename T, int KS> int ms_queries_per_block(int B, int N, int Lq) {
    const int nut = (Lq + 15) / 16;
    const int per = 4 * MsTiles<T, KS>::UT;
    int qpb = nut >= per ? 1 : min(16, per / nut);
    while (qpb > 1 && (long)N * ((B + qpb - 1) / qpb) < 512) qpb >>= 1;
    return qpb;
}

// rerank: documents per wave, as many as leave at least 1024 workgroups
static inline int rr_docs_per_wave(int B, int C) {
    int dpw = RR_MAXDPW;
    while (dpw > 1 && (long)B * ((C + 4 * dpw - 1) / (4 * dpw)) < 1024) dpw >>= 1;
    return dpw;
}

// launches a rerank kernel over its grid, one workgroup per (query, 4 * dpw candidates): `resident` where the query
// fits a wave's registers, else `rounds` (the kernel's two RES instantiations); args: the kernel's, up to Ld
template <typename T, int KS, typename Kern, typename... Args>
void rr_launch(Kern* resident, Kern* rounds, int B, int C, int Lq, hipStream_t st, Args... args) {
    const int dpw = rr_docs_per_wave(B, C);
    dim3 grid((unsigned)((C + 4 * dpw - 1) / (4 * dpw)), (unsigned)B);
    Kern* kern = ms_query_fits<T, KS>(Lq) ? resident : rounds;
    hipLaunchKernelGGL(kern, grid, dim3(256), 0, st, args..., dpw);
}
