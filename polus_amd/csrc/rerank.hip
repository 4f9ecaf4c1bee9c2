// MaxSim re-ranking: every query scores its OWN list of candidate documents (polus_amd/ir/search.py rerank).
//
//   score[b, c] = MaxSim(Q[b], D[cand[b, c]])      -inf where cand[b, c] is outside [0, N)
//
// polus_maxsim_scores (maxsim.hip) keeps a block of queries per workgroup so that a document leaves L2 once; here a
// document is read by one query only, so the kernel is a row gather with MFMAs beside it.  One workgroup per
// (query, block of 4 * dpw candidates), no LDS and no barrier: each wave keeps the query's 16-token tiles as MFMA B
// fragments in registers and takes its own documents (candidates wave, wave + 4, ...).  It streams a document's
// 16-token tiles from global memory straight into A fragments with 16-byte loads, the next tile (or the next
// document's first tile) in flight while the current one is multiplied (two register buffers taken in turn).  The
// wave's candidate ids are read once (one per lane), and the next document's mask is loaded a whole document ahead;
// the mask becomes one 16-bit word per tile (ballots), held one tile per lane, so tiles behind the last valid token
// are never fetched.
// Queries of more tiles than a wave holds (RES = false) take rounds over the document: the query tiles are loaded
// again each round and the document's tiles then come from L2.  The two routes are separate instantiations, because
// one kernel with both keeps two sets of query registers.
// The arithmetic is that of maxsim_fwd_body: the same fragments and MFMAs in ascending k, a max over document
// tokens (a value, so order-free), the 16 maxima of a query tile summed by the same xor-shuffle tree, tiles added in
// ascending order.  A present entry therefore has the bits polus_maxsim_scores gives that (query, document) pair.
#include "maxsim_common.h"

namespace {

template <typename T, int KS, bool RES>
__global__ __launch_bounds__(256) void maxsim_rerank_kernel(const T* __restrict__ Q, const T* __restrict__ D,
                                                            const int32_t* __restrict__ qmask,
                                                            const int32_t* __restrict__ dmask,
                                                            const int32_t* __restrict__ cand, long ldc,
                                                            float* __restrict__ score, long lds, int C, int N, int Lq,
                                                            int Ld, int dpw) {
    constexpr int UT = MsTiles<T, KS>::UT;
    constexpr int E = 32 * KS;
    constexpr size_t ROWB = E * sizeof(T);
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int i = lane & 15, g = lane >> 4;
    const int b = blockIdx.y;
    const int c0 = blockIdx.x * 4 * dpw + wave;               // this wave's candidates: c0, c0 + 4, ...
    if (c0 >= C) return;                                      // wave-uniform; the kernel has no barrier
    const int nd = min(dpw, (C - c0 + 3) >> 2);
    const int myc = c0 + 4 * lane;
    const int idv = cand[(size_t)b * ldc + min(myc, C - 1)];
    const int ids = lane < nd ? idv : -1;                     // lane l: the wave's l-th candidate id

    const int nut = (Lq + 15) >> 4;                           // query tiles
    const T* Qb = Q + (size_t)b * Lq * E;
    const int32_t* qm = qmask ? qmask + (size_t)b * Lq : nullptr;
    const unsigned char* Dg = reinterpret_cast<const unsigned char*>(D) + 8 * g * sizeof(T);

    const int idc = __builtin_amdgcn_readlane(ids, 0);
    bool pres = (unsigned)idc < (unsigned)N;                  // absent: nothing of the document is dereferenced
    const unsigned char* Dc = Dg + (size_t)(pres ? idc : 0) * Ld * ROWB;     // (document 0 stands in for the loads)
    unsigned tm;
    int nvt;
    {
        int mv[8];
        rr_mask_load(mv, dmask ? dmask + (size_t)(pres ? idc : 0) * Ld : nullptr, lane, Ld);
        rr_mask_pack(mv, pres, lane, Ld, tm, nvt);
    }
    // Two tile buffers used in turn, two tiles per trip, so that no tile is ever copied (a copy would wait for the
    // load it copies).  Invariant: at the top of the document loop ta = (document l, tile 0).  A document of an odd
    // number of tiles takes its last tile twice (from cache; a max is idempotent), which keeps the turns in step.
    Frag<T> ta[KS], tb[KS];
    rr_tile_load<T, KS>(ta, Dc, 0, i, Ld);
    Frag<T> qf[UT][KS];
    bool qok[UT];
    if constexpr (RES) rr_query_load        // nut <= UT: the whole query stays in registers
       <T, KS, UT>(qf, qok, Qb, qm, 0, nut, Lq, i, g);

    for (int l = 0; l < nd; ++l) {
        // the next document (the last one stands in for its own successor): id known, mask loads issued now, used
        // after this document's tiles
        const int idn = __builtin_amdgcn_readlane(ids, min(l + 1, nd - 1));
        const bool presn = (unsigned)idn < (unsigned)N;
        const unsigned char* Dn = Dg + (size_t)(presn ? idn : 0) * Ld * ROWB;
        int mvn[8];
        rr_mask_load(mvn, dmask ? dmask + (size_t)(presn ? idn : 0) * Ld : nullptr, lane, Ld);

        float s = 0.f;
        if (nvt > 0) {
            for (int r0 = 0; r0 < nut; r0 += UT) {
                if constexpr (!RES) rr_query_load<T, KS, UT>(qf, qok, Qb, qm, r0, nut, Lq, i, g);
                const int nu = min(UT, nut - r0);
                const bool last_round = r0 + UT >= nut;
                float m[UT];
#pragma unroll
                for (int u = 0; u < UT; ++u) m[u] = -INFINITY;
                for (int t = 0; t < nvt; t += 2) {
                    const int t1 = min(t + 1, nvt - 1);
                    const bool last = t + 2 >= nvt;
                    rr_tile_load<T, KS>(tb, Dc, t1, i, Ld);
                    rr_tile_max<T, KS, UT>(m, ta, qf, __builtin_amdgcn_readlane(tm, t) >> (4 * g), nu);
                    rr_tile_load<T, KS>(ta, (last && last_round) ? Dn : Dc, last ? 0 : t + 2, i, Ld);
                    rr_tile_max<T, KS, UT>(m, tb, qf, __builtin_amdgcn_readlane(tm, t1) >> (4 * g), nu);
                }
#pragma unroll
                for (int u = 0; u < UT; ++u) {
                    if (u < nu) {                             // uniform
                        float mu = m[u];
#pragma unroll
                        for (int o = 16; o <= 32; o <<= 1) {
                            const float m2 = __shfl_xor(mu, o, 64);
                            if (m2 > mu) mu = m2;
                        }
                        // -inf: no valid document token gave a comparable value (maxsim_fwd_body's "no j")
                        float contrib = (qok[u] && mu > -INFINITY) ? mu : 0.f;
#pragma unroll
                        for (int o = 1; o < 16; o <<= 1) contrib += __shfl_xor(contrib, o, 64);
                        s += contrib;
                    }
                }
            }
        } else {
            rr_tile_load<T, KS>(ta, Dn, 0, i, Ld);            // absent or empty document: nothing was streamed
        }
        if (lane == 0) score[(size_t)b * lds + c0 + 4 * l] = pres ? s : -INFINITY;
        rr_mask_pack(mvn, presn, lane, Ld, tm, nvt);
        pres = presn;
        Dc = Dn;
    }
}

}  // namespace

extern "C" int polus_maxsim_rerank(int dtype, const void* Q, const void* D, const int32_t* qmask, const int32_t* dmask,
                                   const int32_t* cand, long ldc, float* score, long lds, int B, int C, int N, int Lq,
                                   int Ld, int E, void* stream) {
    const char* what = "polus_maxsim_rerank";
    int rc = ms_shape_check(what, dtype, B, Lq, Ld, E);
    if (rc == POLUS_OK) rc = rr_args_check(what, C, N, ldc, lds);
    if (rc != POLUS_OK) return rc;
    POLUS_REQUIRE(Q && D && cand && score, "%s: null pointer", what);
    POLUS_REQUIRE(polus_aligned16(Q) && polus_aligned16(D), "%s: Q and D must be 16-byte aligned", what);
    ms_dispatch(dtype, E, [&](auto t, auto ks) {
        using T = typename decltype(t)::type;
        constexpr int KS = decltype(ks)::value;
        rr_launch<T, KS>(maxsim_rerank_kernel<T, KS, true>, maxsim_rerank_kernel<T, KS, false>, B, C, Lq,
                         static_cast<hipStream_t>(stream), static_cast<const T*>(Q), static_cast<const T*>(D), qmask,
                         dmask, cand, ldc, score, lds, C, N, Lq, Ld);
    });
    POLUS_CHECK_LAUNCH(what);
    return POLUS_OK;
}
