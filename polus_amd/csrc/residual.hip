// Residual-compressed token index (ColBERTv2): a document token is the 16-bit id of its nearest centroid plus
// nbits = 1, 2 or 4 bits per dimension that name a bucket of the residual x - centroid.
//
//   compress     r_k = f32(x_k) - f32(centroids[code][k]);   bucket_k = #{j : r_k > cutoffs[j]}
//   decompress   y_k = T(f32(centroids[code][k]) + weights[bucket_k])
//
// (include/polus_hip.h has the rules to the bit).  Element k sits in byte k nbits / 8 at bits nbits (k mod 8 / nbits),
// so the 8 elements k = 8 c .. 8 c + 7 that one MFMA lane holds of a 32-wide k-step are the nbits bytes c nbits ..,
// read as ONE little-endian word whose bits [nbits j, +nbits) are element 8 c + j.  Everything here works on such
// 8-element chunks: res_decode8 turns a centroid chunk and a word into a fragment, the decoder stores it, and the
// re-ranking kernel (maxsim_rerank_kernel of rerank.hip with another A-fragment load) multiplies it.  Same function,
// same fragments, same MFMAs in the same k order:
//   polus_maxsim_rerank_res(Q, codes, packed, ...) == polus_maxsim_rerank(Q, polus_residual_decompress(...))  in bits.
// The bucket weights (at most 16 floats) live in registers, one per lane (lane l holds weights[l mod 2^nbits]), and are
// picked by a lane permute; no LDS memory, no barrier.
#include "maxsim_common.h"

namespace {

// lane l holds weights[l & (2^NB - 1)]; a bucket's weight comes from lane `bucket` by a lane permute (the LDS
// crossbar, no LDS memory).  Every lane of the wave must be active.
template <int NB> struct ResWeights {
    float wl;
    __device__ __forceinline__ void load(const float* w, int lane) { wl = w[lane & ((1 << NB) - 1)]; }
    __device__ __forceinline__ float get(unsigned b) const {
        return __builtin_bit_cast(float, __builtin_amdgcn_ds_bpermute((int)(b << 2), __builtin_bit_cast(int, wl)));
    }
};

// the NB bytes of an 8-element chunk as one little-endian word
template <int NB> __device__ __forceinline__ unsigned res_word_load(const unsigned char* p) {
    if constexpr (NB == 4) return *reinterpret_cast<const unsigned*>(p);
    else if constexpr (NB == 2) return *reinterpret_cast<const unsigned short*>(p);
    else return *p;
}
template <int NB> __device__ __forceinline__ void res_word_store(unsigned char* p, unsigned w) {
    if constexpr (NB == 4) *reinterpret_cast<unsigned*>(p) = w;
    else if constexpr (NB == 2) *reinterpret_cast<unsigned short*>(p) = (unsigned short)w;
    else *p = (unsigned char)w;
}

__device__ __forceinline__ float frag_get(const Frag<float>& f, int j) { return f.v[j]; }
__device__ __forceinline__ float frag_get(const Frag<bf16_t>& f, int j) { return (float)f.v[j]; }
__device__ __forceinline__ void frag_set(Frag<float>& f, int j, float x) { f.v[j] = x; }
__device__ __forceinline__ void frag_set(Frag<bf16_t>& f, int j, float x) { f.v[j] = (bf16_t)x; }

// THE decode: y_j = T(f32(c_j) + weights[bucket_j]), one f32 addition and one round-to-nearest-even conversion; a
// chunk of a row without a centroid (ok false) is zeros
template <typename T, int NB>
__device__ __forceinline__ void res_decode8(Frag<T>& y, const Frag<T>& c, unsigned word, const ResWeights<NB>& w, bool ok) {
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const float v = frag_get(c, j) + w.get((word >> (NB * j)) & ((1u << NB) - 1u));
        frag_set(y, j, ok ? v : 0.f);
    }
}

__device__ __forceinline__ void frag_store_row(const Frag<bf16_t>& f, unsigned char* p) {
    *reinterpret_cast<bf16x8*>(p) = f.v;
}
__device__ __forceinline__ void frag_store_row(const Frag<float>& f, unsigned char* p) {
    *reinterpret_cast<float4*>(p) = make_float4(f.v[0], f.v[1], f.v[2], f.v[3]);
    *reinterpret_cast<float4*>(p + 16) = make_float4(f.v[4], f.v[5], f.v[6], f.v[7]);
}

// ---------------------------------------------------------------- compress / decompress, one thread per 8-element chunk
template <typename T, int NB>
__global__ __launch_bounds__(256) void residual_compress_kernel(const T* __restrict__ x,
                                                                const unsigned short* __restrict__ codes,
                                                                const T* __restrict__ cent, int K,
                                                                const float* __restrict__ cutoffs,
                                                                unsigned char* __restrict__ packed, long chunks, int E) {
    const long ch = (long)blockIdx.x * 256 + threadIdx.x;
    if (ch >= chunks) return;
    const int cpr = E >> 3;                                   // chunks per row
    const long row = ch / cpr;
    const int c = (int)(ch - row * cpr);
    const unsigned code = codes[row];
    unsigned word = 0;
    if (code < (unsigned)K) {                                 // a row without a centroid: zero bytes, nothing dereferenced
        Frag<T> xf, cf;
        frag_load_row(xf, reinterpret_cast<const unsigned char*>(x + (size_t)row * E + 8 * c));
        frag_load_row(cf, reinterpret_cast<const unsigned char*>(cent + (size_t)code * E + 8 * c));
        float cut[(1 << NB) - 1];
#pragma unroll
        for (int j = 0; j < (1 << NB) - 1; ++j) cut[j] = cutoffs[j];
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const float r = frag_get(xf, e) - frag_get(cf, e);
            unsigned b = 0;
#pragma unroll
            for (int j = 0; j < (1 << NB) - 1; ++j) b += r > cut[j] ? 1u : 0u;     // NaN: no cutoff is below it
            word |= b << (NB * e);
        }
    }
    res_word_store<NB>(packed + (size_t)ch * NB, word);
}

template <typename T, int NB>
__global__ __launch_bounds__(256) void residual_decompress_kernel(const unsigned short* __restrict__ codes,
                                                                  const unsigned char* __restrict__ packed,
                                                                  const T* __restrict__ cent, int K,
                                                                  const float* __restrict__ weights, T* __restrict__ y,
                                                                  long chunks, int E) {
    ResWeights<NB> w;
    w.load(weights, threadIdx.x & 63);
    const long mine = (long)blockIdx.x * 256 + threadIdx.x;
    const long ch = min(mine, chunks - 1);                    // every lane stays active for the weight look-up
    const int cpr = E >> 3;
    const long row = ch / cpr;
    const int c = (int)(ch - row * cpr);
    const unsigned code = codes[row];
    const bool ok = code < (unsigned)K;
    Frag<T> cf, yf;
    frag_load_row(cf, reinterpret_cast<const unsigned char*>(cent + (size_t)(ok ? code : 0u) * E + 8 * c));
    res_decode8<T, NB>(yf, cf, res_word_load<NB>(packed + (size_t)ch * NB), w, ok);
    if (mine < chunks) frag_store_row(yf, reinterpret_cast<unsigned char*>(y + (size_t)ch * 8));
}

// ---------------------------------------------------------------- re-ranking
// A document tile before it is decoded: per k-step this lane's centroid chunk and its word of residual bits.
template <typename T, int KS> struct ResTile {
    Frag<T> c[KS];
    unsigned p[KS];
    bool ok;                                                  // the row has a centroid
};

// a document's codes, token 64 k + lane in c<k>, loaded a whole document ahead like its mask (rr_mask_load).  Eight
// named members picked by masks: of an array, or of selects between the members, the compiler made a per-thread copy
// in LDS read by a variable index (8 KiB a workgroup)
struct ResCodes {
    unsigned c0, c1, c2, c3, c4, c5, c6, c7;
    __device__ __forceinline__ void load(const unsigned short* dc, int lane, int Ld) {
        c0 = dc[min(lane, Ld - 1)];
        c1 = dc[min(64 + lane, Ld - 1)];
        c2 = dc[min(128 + lane, Ld - 1)];
        c3 = dc[min(192 + lane, Ld - 1)];
        c4 = dc[min(256 + lane, Ld - 1)];
        c5 = dc[min(320 + lane, Ld - 1)];
        c6 = dc[min(384 + lane, Ld - 1)];
        c7 = dc[min(448 + lane, Ld - 1)];
    }
    // c<kk> for a wave-uniform kk
    __device__ __forceinline__ unsigned pick(int kk) const {
        const auto on = [kk](int k) { return kk == k ? ~0u : 0u; };
        return (c0 & on(0)) | (c1 & on(1)) | (c2 & on(2)) | (c3 & on(3)) | (c4 & on(4)) | (c5 & on(5)) | (c6 & on(6)) |
               (c7 & on(7));
    }
};

// tile t of a document: lane (i, g) takes row 16 t + i (rows past Ld re-read row Ld - 1), k = 8 g .. 8 g + 7 of every
// 32-wide k-step.  `held` is this lane's register of the document's codes that covers tile t (tokens 64 (t >> 2) + lane);
// Pg = the document's packed rows + NB g, Cg = centroids + 8 g elements.  A row whose code is >= K reads centroid 0
// (K >= 1) and decodes to zeros.
template <typename T, int KS, int NB>
__device__ __forceinline__ void res_tile_load(ResTile<T, KS>& f, const unsigned char* Pg, const unsigned char* Cg,
                                              unsigned held, int t, int i, int Ld, int K) {
    const int row = min(16 * t + i, Ld - 1);
    const unsigned code = (unsigned)__shfl((int)held, row & 63, 64);
    f.ok = code < (unsigned)K;
    const unsigned char* cp = Cg + (size_t)(f.ok ? code : 0u) * (32 * KS * sizeof(T));
    const unsigned char* pp = Pg + (size_t)row * (4 * KS * NB);
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
        frag_load_row(f.c[ks], cp + ks * 32 * sizeof(T));
        f.p[ks] = res_word_load<NB>(pp + ks * 4 * NB);
    }
}

template <typename T, int KS, int UT, int NB>
__device__ __forceinline__ void res_tile_max(float (&m)[UT], const ResTile<T, KS>& tile, const Frag<T> (&qf)[UT][KS],
                                             const ResWeights<NB>& w, unsigned bits, int nu) {
    Frag<T> df[KS];
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) res_decode8<T, NB>(df[ks], tile.c[ks], tile.p[ks], w, tile.ok);
    rr_tile_max<T, KS, UT>(m, df, qf, bits, nu);
}

template <typename T, int KS, int NB, bool RES>
__global__ __launch_bounds__(256) void maxsim_rerank_res_kernel(const T* __restrict__ Q,
                                                                const unsigned short* __restrict__ codes,
                                                                const unsigned char* __restrict__ packed,
                                                                const T* __restrict__ cent, int K,
                                                                const float* __restrict__ weights,
                                                                const int32_t* __restrict__ qmask,
                                                                const int32_t* __restrict__ dmask,
                                                                const int32_t* __restrict__ cand, long ldc,
                                                                float* __restrict__ score, long lds, int C, int N,
                                                                int Lq, int Ld, int dpw) {
    constexpr int UT = MsTiles<T, KS>::UT;
    constexpr int E = 32 * KS;
    constexpr size_t ROWB = E * NB / 8;                       // packed bytes of a token
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

    ResWeights<NB> w;
    w.load(weights, lane);
    const int nut = (Lq + 15) >> 4;                           // query tiles
    const T* Qb = Q + (size_t)b * Lq * E;
    const int32_t* qm = qmask ? qmask + (size_t)b * Lq : nullptr;
    const unsigned char* Pg = packed + NB * g;
    const unsigned char* Cg = reinterpret_cast<const unsigned char*>(cent) + 8 * g * sizeof(T);

    const int idc = __builtin_amdgcn_readlane(ids, 0);
    bool pres = (unsigned)idc < (unsigned)N;                  // absent: nothing of the document is dereferenced
    const unsigned char* Pc = Pg + (size_t)(pres ? idc : 0) * Ld * ROWB;     // (document 0 stands in for the loads)
    ResCodes cv;
    cv.load(codes + (size_t)(pres ? idc : 0) * Ld, lane, Ld);
    unsigned tm;
    int nvt;
    {
        int mv[8];
        rr_mask_load(mv, dmask ? dmask + (size_t)(pres ? idc : 0) * Ld : nullptr, lane, Ld);
        rr_mask_pack(mv, pres, lane, Ld, tm, nvt);
    }
    // two tile buffers in turn, as maxsim_rerank_kernel: at the top of the document loop ta = (document l, tile 0)
    ResTile<T, KS> ta, tb;
    res_tile_load<T, KS, NB>(ta, Pc, Cg, cv.c0, 0, i, Ld, K);
    Frag<T> qf[UT][KS];
    bool qok[UT];
    if constexpr (RES) rr_query_load        // nut <= UT: the whole query stays in registers
       <T, KS, UT>(qf, qok, Qb, qm, 0, nut, Lq, i, g);

    for (int l = 0; l < nd; ++l) {
        const int idn = __builtin_amdgcn_readlane(ids, min(l + 1, nd - 1));
        const bool presn = (unsigned)idn < (unsigned)N;
        const unsigned char* Pn = Pg + (size_t)(presn ? idn : 0) * Ld * ROWB;
        ResCodes cvn;
        cvn.load(codes + (size_t)(presn ? idn : 0) * Ld, lane, Ld);
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
                    res_tile_load<T, KS, NB>(tb, Pc, Cg, cv.pick(t1 >> 2), t1, i, Ld, K);
                    res_tile_max<T, KS, UT, NB>(m, ta, qf, w, __builtin_amdgcn_readlane(tm, t) >> (4 * g), nu);
                    const bool nxt = last && last_round;
                    const int t2 = last ? 0 : t + 2;
                    res_tile_load<T, KS, NB>(ta, nxt ? Pn : Pc, Cg, nxt ? cvn.c0 : cv.pick(t2 >> 2), t2, i,
                                             Ld, K);
                    res_tile_max<T, KS, UT, NB>(m, tb, qf, w, __builtin_amdgcn_readlane(tm, t1) >> (4 * g), nu);
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
                        float contrib = (qok[u] && mu > -INFINITY) ? mu : 0.f;
#pragma unroll
                        for (int o = 1; o < 16; o <<= 1) contrib += __shfl_xor(contrib, o, 64);
                        s += contrib;
                    }
                }
            }
        } else {
            res_tile_load<T, KS, NB>(ta, Pn, Cg, cvn.c0, 0, i, Ld, K);      // absent or empty document: nothing was streamed
        }
        if (lane == 0) score[(size_t)b * lds + c0 + 4 * l] = pres ? s : -INFINITY;
        rr_mask_pack(mvn, presn, lane, Ld, tm, nvt);
        pres = presn;
        Pc = Pn;
        cv = cvn;
    }
}

// ---------------------------------------------------------------- host
int res_codec_check(const char* what, int dtype, int K, int nbits, int E) {
    POLUS_REQUIRE(dtype == POLUS_F32 || dtype == POLUS_BF16, "%s: unknown dtype %d", what, dtype);
    POLUS_REQUIRE(nbits == 1 || nbits == 2 || nbits == 4, "%s: nbits must be 1, 2 or 4 (got %d)", what, nbits);
    POLUS_REQUIRE(E >= 32 && E <= MS_EMAX && E % 32 == 0, "%s: E must be a multiple of 32 in [32, %d] (got %d)", what,
                  MS_EMAX, E);
    POLUS_REQUIRE(K >= 1 && K <= 65535, "%s: need 1 <= K <= 65535 centroids (got %d)", what, K);
    return POLUS_OK;
}

#define RES_BY_NB(CALL)                                        \
    switch (nbits) {                                           \
    case 1: CALL(1); break;                                    \
    case 2: CALL(2); break;                                    \
    default: CALL(4); break;                                   \
    }

}  // namespace

extern "C" int polus_residual_compress(int dtype, const void* x, const uint16_t* codes, const void* centroids, int K,
                                       const float* cutoffs, int nbits, uint8_t* packed, int rows, int E,
                                       void* stream) {
    const char* what = "polus_residual_compress";
    int rc = res_codec_check(what, dtype, K, nbits, E);
    if (rc != POLUS_OK) return rc;
    POLUS_REQUIRE(rows >= 1, "%s: need rows >= 1 (got %d)", what, rows);
    POLUS_REQUIRE(x && codes && centroids && cutoffs && packed, "%s: null pointer", what);
    POLUS_REQUIRE(polus_aligned16(x) && polus_aligned16(centroids), "%s: x and centroids must be 16-byte aligned", what);
    POLUS_REQUIRE((((uintptr_t)packed) & 3) == 0, "%s: packed must be 4-byte aligned", what);
    hipStream_t st = static_cast<hipStream_t>(stream);
    const long chunks = (long)rows * (E / 8);
    const dim3 grid((unsigned)((chunks + 255) / 256));
#define RES_CALL(NB_)                                                                                                  \
    if (dtype == POLUS_BF16)                                                                                           \
        hipLaunchKernelGGL((residual_compress_kernel<bf16_t, NB_>), grid, dim3(256), 0, st,                            \
                           static_cast<const bf16_t*>(x), codes, static_cast<const bf16_t*>(centroids), K, cutoffs,    \
                           packed, chunks, E);                                                                         \
    else                                                                                                               \
        hipLaunchKernelGGL((residual_compress_kernel<float, NB_>), grid, dim3(256), 0, st,                             \
                           static_cast<const float*>(x), codes, static_cast<const float*>(centroids), K, cutoffs,      \
                           packed, chunks, E)
    RES_BY_NB(RES_CALL)
#undef RES_CALL
    POLUS_CHECK_LAUNCH(what);
    return POLUS_OK;
}

extern "C" int polus_residual_decompress(int dtype, const uint16_t* codes, const uint8_t* packed, const void* centroids,
                                         int K, const float* weights, int nbits, void* y, int rows, int E,
                                         void* stream) {
    const char* what = "polus_residual_decompress";
    int rc = res_codec_check(what, dtype, K, nbits, E);
    if (rc != POLUS_OK) return rc;
    POLUS_REQUIRE(rows >= 1, "%s: need rows >= 1 (got %d)", what, rows);
    POLUS_REQUIRE(codes && packed && centroids && weights && y, "%s: null pointer", what);
    POLUS_REQUIRE(polus_aligned16(y) && polus_aligned16(centroids), "%s: y and centroids must be 16-byte aligned", what);
    POLUS_REQUIRE((((uintptr_t)packed) & 3) == 0, "%s: packed must be 4-byte aligned", what);
    hipStream_t st = static_cast<hipStream_t>(stream);
    const long chunks = (long)rows * (E / 8);
    const dim3 grid((unsigned)((chunks + 255) / 256));
#define RES_CALL(NB_)                                                                                                  \
    if (dtype == POLUS_BF16)                                                                                           \
        hipLaunchKernelGGL((residual_decompress_kernel<bf16_t, NB_>), grid, dim3(256), 0, st, codes, packed,           \
                           static_cast<const bf16_t*>(centroids), K, weights, static_cast<bf16_t*>(y), chunks, E);     \
    else                                                                                                               \
        hipLaunchKernelGGL((residual_decompress_kernel<float, NB_>), grid, dim3(256), 0, st, codes, packed,            \
                           static_cast<const float*>(centroids), K, weights, static_cast<float*>(y), chunks, E)
    RES_BY_NB(RES_CALL)
#undef RES_CALL
    POLUS_CHECK_LAUNCH(what);
    return POLUS_OK;
}

extern "C" int polus_maxsim_rerank_res(int dtype, const void* Q, const uint16_t* codes, const uint8_t* packed,
                                       const void* centroids, int K, const float* weights, int nbits,
                                       const int32_t* qmask, const int32_t* dmask, const int32_t* cand, long ldc,
                                       float* score, long lds, int B, int C, int N, int Lq, int Ld, int E,
                                       void* stream) {
    const char* what = "polus_maxsim_rerank_res";
    int rc = res_codec_check(what, dtype, K, nbits, E);
    if (rc != POLUS_OK) return rc;
    // (dtype and E have passed above: from here on the order is Lq, Ld, B, then the candidate lists)
    rc = ms_shape_check(what, dtype, B, Lq, Ld, E);
    if (rc == POLUS_OK) rc = rr_args_check(what, C, N, ldc, lds);
    if (rc != POLUS_OK) return rc;
    POLUS_REQUIRE(Q && codes && packed && centroids && weights && cand && score, "%s: null pointer", what);
    POLUS_REQUIRE(polus_aligned16(Q) && polus_aligned16(centroids), "%s: Q and centroids must be 16-byte aligned", what);
    POLUS_REQUIRE((((uintptr_t)packed) & 3) == 0, "%s: packed must be 4-byte aligned", what);
    ms_dispatch(dtype, E, [&](auto t, auto ks) {
        using T = typename decltype(t)::type;
        constexpr int KS = decltype(ks)::value;
#define RES_CALL(NB_)                                                                                                  \
    rr_launch<T, KS>(maxsim_rerank_res_kernel<T, KS, NB_, true>, maxsim_rerank_res_kernel<T, KS, NB_, false>, B, C, Lq, \
                     static_cast<hipStream_t>(stream), static_cast<const T*>(Q), codes, packed,                        \
                     static_cast<const T*>(centroids), K, weights, qmask, dmask, cand, ldc, score, lds, C, N, Lq, Ld)
        RES_BY_NB(RES_CALL)
#undef RES_CALL
    });
    POLUS_CHECK_LAUNCH(what);
    return POLUS_OK;
}
