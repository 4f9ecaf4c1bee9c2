// Device helpers shared by the MaxSim kernels: maxsim.hip (training forward, corpus scores), rerank.hip (candidate
// lists), maxsim_fp8.hip (the same two over an FP8 token index) and residual.hip (candidate lists over a
// residual-compressed index).  What is here is what must be the same in all of them for their scores to agree bit for
// bit: how many query tiles a wave holds, how a query tile becomes B fragments, how a document's mask becomes per-tile
// bit words, and how a tile's fragments meet the query's (rr_tile_max).
#pragma once
#include "common.h"

constexpr int MS_LMAX = 512;            // Lq, Ld limit
constexpr int MS_EMAX = 256;            // E limit (multiple of 32)

constexpr int RR_MAXDPW = 8;            // rerank: documents per wave, at most

// rerank: documents per wave, as many as leave at least 1024 workgroups
static inline int rr_docs_per_wave(int B, int C) {
    int dpw = RR_MAXDPW;
    while (dpw > 1 && (long)B * ((C + 4 * dpw - 1) / (4 * dpw)) < 1024) dpw >>= 1;
    return dpw;
}

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
