// What the product-quantisation scans share (pq.hip: polus_pq_scores over all documents; ivfpq.hip: polus_ivfpq_scores_ids
// over residual codes and per-query candidate ids): the format's limits and their check, the size of a table image in
// LDS, the split of a launch's columns over the CUs and the loads of a code row in pieces.
#pragma once
#include <algorithm>

#include "common.h"

constexpr int PQ_MMAX = 160, PQ_KMAX = 256, PQ_DMAX = 32;
constexpr size_t PQ_LDS_MAX = 160 * 1024;         // one CU's LDS
constexpr int PQ_SCAN_THREADS = 1024;
constexpr int PQ_ROWS_MAX = 65535;

// qt tables in LDS, every sub-space padded to 256 entries.
static inline size_t pq_lds_bytes(int qt, int m) { return (size_t)qt * m * 256 * sizeof(float); }

// Documents per workgroup: one workgroup per CU over the launch where the tables leave room for one, two where they
// leave room for two (2048 threads per CU), never fewer than 256 documents unless N is smaller: the copy of the tables is
// a fixed price per workgroup, and a CU without a workgroup pays nothing either.
static inline int pq_docs_per_block(int groups, int N, size_t lds) {
    const long per_cu = lds * 2 <= PQ_LDS_MAX ? 2 : 1;
    const long per_group = std::max(1L, per_cu * polus_num_cus() / groups);
    long dpb = ((long)N + per_group - 1) / per_group;
    dpb = std::max((dpb + 63) / 64 * 64, 256L);
    return (int)std::min(dpb, (long)N);
}

// Four code bytes at p as one word (byte k in bits 8k .. 8k+7): one load where p is 4-byte aligned.
template <bool ALIGNED> __device__ __forceinline__ uint32_t pq_word(const uint8_t* p) {
    if constexpr (ALIGNED) return *reinterpret_cast<const uint32_t*>(p);
    return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24);
}

// PIECE: 16 (codes, ldc and m multiples of 16), 4 (multiples of 4) or 1 (anything: four byte loads per word).
template <int PIECE> __device__ __forceinline__ void pq_piece(const uint8_t* p, uint32_t (&w)[PIECE == 16 ? 4 : 1]) {
    if constexpr (PIECE == 16) {
        const uint4 v = *reinterpret_cast<const uint4*>(p);
        w[0] = v.x; w[1] = v.y; w[2] = v.z; w[3] = v.w;
    } else {
        w[0] = pq_word<PIECE == 4>(p);
    }
}

// The piece a scan reads its code rows in: the widest that the base, the row stride and the row length all allow.
static inline int pq_piece_bytes(const uint8_t* codes, long ldc, int m) {
    const uintptr_t bits = (uintptr_t)codes | (uintptr_t)ldc | (uintptr_t)m;
    return (bits & 15) == 0 ? 16 : (bits & 3) == 0 ? 4 : 1;
}

static inline int pq_check_format(const char* what, int m, int ksub, int dsub) {
    POLUS_REQUIRE(m >= 4 && m <= PQ_MMAX && m % 4 == 0, "%s: m must be a multiple of 4 in [4, %d] (got %d)", what, PQ_MMAX, m);
    POLUS_REQUIRE(ksub >= 1 && ksub <= PQ_KMAX, "%s: need 1 <= ksub <= %d (got %d)", what, PQ_KMAX, ksub);
    POLUS_REQUIRE(dsub >= 1 && dsub <= PQ_DMAX, "%s: need 1 <= dsub <= %d (got %d)", what, PQ_DMAX, dsub);
    return POLUS_OK;
}

#define PQ_CHECK_DTYPE(what, dtype) \
    POLUS_REQUIRE(dtype == POLUS_F32 || dtype == POLUS_BF16, "%s: unknown dtype %d", what, dtype)
