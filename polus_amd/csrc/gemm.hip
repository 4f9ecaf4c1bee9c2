// GEMM for the Dense layers of the BERT step and their gradients (gfx950).  This file holds
//   - the general MFMA kernel (128 x 128 tile, f32 / bf16, any layout and alignment) and the split-K reduce kernels;
//   - the host side of every Dense GEMM: polus_gemm / polus_gemm_dropout, whose choice among this kernel and the ones of
//     gemm_ring.hip / gemm_pp.hip is gemm_route(), and polus_dense_bwd_params(_grouped), whose workspace layout is
//     grouped_dw_plan() (kernels in gemm_ring.hip / gemm_ppks.hip).
//
// The general kernel: one 256-thread workgroup (4 waves, 2x2) computes a 128x128 tile of C; each wave owns
// 64x64 = 4x4 MFMA 16x16 tiles (64 accumulator registers).  A K-step is 128 bytes of K per
// row (64 bf16 / 32 f32).  Operands are staged HBM -> registers -> LDS (double-buffered,
// one barrier per K-step, the next tile's global loads in flight under the MFMAs).
//
// LDS images:
//   K-contiguous operand ([rows][K] in memory): [128 rows][128 B + 32 B pad] = 160-B rows;
//     fragments are ds_read_b128 of (row i, 16 B at k-group g) — 160 B puts the 16 rows of a
//     b128 lane group on 16 distinct 16-B slots.
//   K-strided operand ([K][rows] in memory: dY and X in dW = dY^T X, W in dX = dY W):
//     kept k-major exactly as loaded (coalesced 16-B chunks along the row index), bf16 rows
//     of 288 B with byte-bit-7 XOR for odd k-octets, f32 rows of 512 B with bit-6 XOR;
//     bf16 fragments come out of ds_read_b64_tr_b16 (hardware transpose), f32 ones from
//     ds_read_b32.
// The MFMA is issued as D[n][m] (B rows as the A operand) so that a lane ends up with four
// consecutive n of one output row: 8/16-byte epilogue accesses.
#include <stdlib.h>
#include "gemm_common.h"

using namespace pgemm;

namespace {

constexpr int BM = 128, BN = 128, NTHREADS = 256;
constexpr int KC_STRIDE = 160;
constexpr int OPERAND_BYTES = 128 * KC_STRIDE;  // 20480, >= every K-strided image
constexpr int SMEM_BYTES = 4 * OPERAND_BYTES;   // A0 B0 A1 B1

template <typename T> struct Cfg;
template <> struct Cfg<bf16_t> {
    static constexpr int BK = 64, EPC = 8, NSUB = 2;
    static constexpr int KS_STRIDE = 288, KS_SWZ = 7, LOG_RCH = 4;
};
template <> struct Cfg<float> {
    static constexpr int BK = 32, EPC = 4, NSUB = 1;
    static constexpr int KS_STRIDE = 512, KS_SWZ = 6, LOG_RCH = 5;
};

typedef unsigned int u32x4_t __attribute__((ext_vector_type(4)));
template <typename T> union Chunk { uint4 u; u32x4_t w; T e[16 / sizeof(T)]; };

// ---- HBM -> registers: one operand tile = 1024 16-byte chunks, 4 per thread.
// Branch-free on purpose: a per-lane `if` around a global load makes hipcc wait vmcnt(0)
// at every join, which serialises the eight loads of a K-step.  Invalid chunks read a clamped
// (in-bounds) address and are zeroed by a select.  VEC = every 16-byte chunk is wholly valid
// or wholly invalid and 16-byte aligned (checked on the host); otherwise the element path
// loads each element with its own predicate (tiny heads only).
// 16 zero bytes in HBM: invalid chunks load from here, so no select has to consume the loaded
// value (a select right after the load would pull its s_waitcnt in front of the MFMAs).
__device__ const uint4 g_zero_chunk[1] = {{0u, 0u, 0u, 0u}};

template <typename T, bool VEC>
__device__ __forceinline__ uint4 load_chunk(const T* __restrict__ base, long off, bool ok, int nvalid) {
    constexpr int EPC = Cfg<T>::EPC;
    // both arms in the global address space: a generic-pointer select would turn into flat_load
    typedef const __attribute__((address_space(1))) u32x4_t* gp16_t;
    typedef const __attribute__((address_space(1))) T* gpe_t;
    Chunk<T> v;
    if (VEC) {
        gp16_t p = ok ? (gp16_t)(base + off) : (gp16_t)g_zero_chunk;
        v.w = *p;
    } else {
#pragma unroll
        for (int e = 0; e < EPC; ++e) {
            gpe_t p = (ok && e < nvalid) ? (gpe_t)(base + off + e) : (gpe_t)g_zero_chunk;
            v.e[e] = *p;
        }
    }
    return v.u;
}
template <typename T, bool VEC>
__device__ __forceinline__ void gload_kc(uint4 (&r)[4], const T* __restrict__ base, long ld, int rows,
                                         int r0, int k0, int kend, int tid) {
    constexpr int EPC = Cfg<T>::EPC;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        int c = tid + NTHREADS * i;
        int gr = r0 + (c >> 3), gk = k0 + (c & 7) * EPC;
        r[i] = load_chunk<T, VEC>(base, (long)gr * ld + gk, gr < rows && gk < kend, kend - gk);
    }
}
template <typename T>
__device__ __forceinline__ void sstore_kc(unsigned char* tile, const uint4 (&r)[4], int tid) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        int c = tid + NTHREADS * i;
        *reinterpret_cast<uint4*>(tile + (c >> 3) * KC_STRIDE + (c & 7) * 16) = r[i];
    }
}
template <typename T, bool VEC>
__device__ __forceinline__ void gload_ks(uint4 (&r)[4], const T* __restrict__ base, long ld, int rows,
                                         int r0, int k0, int kend, int tid) {
    constexpr int EPC = Cfg<T>::EPC, LOG = Cfg<T>::LOG_RCH;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        int c = tid + NTHREADS * i;
        int gk = k0 + (c >> LOG), gr = r0 + (c & ((1 << LOG) - 1)) * EPC;
        r[i] = load_chunk<T, VEC>(base, (long)gk * ld + gr, gk < kend && gr < rows, rows - gr);
    }
}
template <typename T>
__device__ __forceinline__ void sstore_ks(unsigned char* tile, const uint4 (&r)[4], int tid) {
    constexpr int LOG = Cfg<T>::LOG_RCH;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        int c = tid + NTHREADS * i;
        int krow = c >> LOG, rc = c & ((1 << LOG) - 1);
        int off = krow * Cfg<T>::KS_STRIDE + ((rc * 16) ^ (((krow >> 3) & 1) << Cfg<T>::KS_SWZ));
        *reinterpret_cast<uint4*>(tile + off) = r[i];
    }
}

// ---- LDS -> fragments
// K-contiguous image: tile row `row`, k-substep `sub`, lane group g
template <typename T>
__device__ __forceinline__ void frag_kc(Frag<T>& f, const unsigned char* tile, int row, int sub, int g) {
    frag_load_row(f, tile + row * KC_STRIDE + sub * (32 * (int)sizeof(T)) + g * (8 * (int)sizeof(T)));
}
// K-strided image: rows col0..col0+15 of the operand, k = sub*32 + 8g + j
__device__ __forceinline__ void frag_ks(Frag<bf16_t>& f, const unsigned char* tile, int col0, int sub, int i, int g) {
    int kb = sub * 32 + 8 * g + (i >> 2);
    int cb = (col0 + 4 * (i & 3)) * 2;
    int swz = (g & 1) << 7;  // ((k >> 3) & 1) for k = sub*32 + 8g + (0..7)
    s16x4 lo = lds_tr16(tile + kb * 288 + (cb ^ swz));
    s16x4 hi = lds_tr16(tile + (kb + 4) * 288 + (cb ^ swz));
    typedef short s16x8 __attribute__((ext_vector_type(8)));
    s16x8 w = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
    f.v = __builtin_bit_cast(bf16x8, w);
}
__device__ __forceinline__ void frag_ks(Frag<float>& f, const unsigned char* tile, int col0, int sub, int i, int g) {
    int cb = ((col0 + i) * 4) ^ ((g & 1) << 6);
#pragma unroll
    for (int j = 0; j < 8; ++j)
        f.v[j] = *reinterpret_cast<const float*>(tile + (8 * g + j) * 512 + cb);
}

template <typename T, bool A_KS, bool B_KS, typename TC, bool VEC, bool DROP>
__global__ __launch_bounds__(NTHREADS) void gemm_kernel(GemmArgs p) {
    if (DROP) p.drop_seed = polus_eff_seed(p.drop_seed, p.dyn);
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    constexpr int BK = Cfg<T>::BK, NSUB = Cfg<T>::NSUB;
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int i = lane & 15, g = lane >> 4;
    const int wm = wid >> 1, wn = wid & 1;

    const int tiles_n = (p.N + BN - 1) / BN;
    const int wg = xcd_remap(blockIdx.x, gridDim.x);
    const int m0 = (wg / tiles_n) * BM, n0 = (wg % tiles_n) * BN;

    const int kbeg = blockIdx.z * p.k_per_split;
    const int kend = min(p.K, kbeg + p.k_per_split);
    const int nk = (kend - kbeg + BK - 1) / BK;

    const T* A = static_cast<const T*>(p.A);
    const T* B = static_cast<const T*>(p.B);

    f32x4 acc[4][4];
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b) acc[a][b] = (f32x4){0.f, 0.f, 0.f, 0.f};

    uint4 ra[4], rb[4];
    auto gload = [&](int k0) {
        if (A_KS) gload_ks<T, VEC>(ra, A, p.lda, p.M, m0, k0, kend, tid);
        else      gload_kc<T, VEC>(ra, A, p.lda, p.M, m0, k0, kend, tid);
        if (B_KS) gload_ks<T, VEC>(rb, B, p.ldb, p.N, n0, k0, kend, tid);
        else      gload_kc<T, VEC>(rb, B, p.ldb, p.N, n0, k0, kend, tid);
    };
    auto sstore = [&](int buf) {
        unsigned char* ta = smem + buf * 2 * OPERAND_BYTES;
        unsigned char* tb = ta + OPERAND_BYTES;
        if (A_KS) sstore_ks<T>(ta, ra, tid); else sstore_kc<T>(ta, ra, tid);
        if (B_KS) sstore_ks<T>(tb, rb, tid); else sstore_kc<T>(tb, rb, tid);
    };

    if (nk > 0) { gload(kbeg); sstore(0); }
    __syncthreads();
    for (int kt = 0; kt < nk; ++kt) {
        const int cur = kt & 1;
        if (kt + 1 < nk) gload(kbeg + (kt + 1) * BK);
        const unsigned char* ta = smem + cur * 2 * OPERAND_BYTES;
        const unsigned char* tb = ta + OPERAND_BYTES;
#pragma unroll
        for (int sub = 0; sub < NSUB; ++sub) {
            Frag<T> af[4], bf[4];
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                if (A_KS) frag_ks(af[t], ta, wm * 64 + t * 16, sub, i, g);
                else      frag_kc<T>(af[t], ta, wm * 64 + t * 16 + i, sub, g);
                if (B_KS) frag_ks(bf[t], tb, wn * 64 + t * 16, sub, i, g);
                else      frag_kc<T>(bf[t], tb, wn * 64 + t * 16 + i, sub, g);
            }
#pragma unroll
            for (int tm = 0; tm < 4; ++tm)
#pragma unroll
                for (int tn = 0; tn < 4; ++tn) mma16(acc[tm][tn], bf[tn], af[tm]);
        }
        if (kt + 1 < nk) sstore(cur ^ 1);
        __syncthreads();
    }

    // ---- epilogue
#pragma unroll
    for (int tm = 0; tm < 4; ++tm)
#pragma unroll
        for (int tn = 0; tn < 4; ++tn)
            epilogue_tile<T, TC, DROP>(p, acc[tm][tn], m0 + wm * 64 + tm * 16 + i, n0 + wn * 64 + tn * 16 + 4 * g, blockIdx.z);
}

// order-fixed split-K reduction: C = alpha * sum_z slab[z] (+ bias) (+ C)
template <typename TC>
__global__ void splitk_reduce_kernel(const float* __restrict__ slabs, int splits, int M, int N,
                                     TC* C, long ldc, float alpha, const float* bias, int accum) {
    long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
    long total = (long)M * N;
    if (idx >= total) return;
    int m = idx / N, n = idx % N;
    float s = 0.f;
    for (int z = 0; z < splits; ++z) s += slabs[(long)z * total + idx];
    s *= alpha;
    if (bias) s += bias[n];
    TC* c = C + (long)m * ldc + n;
    if (accum) s += to_f<TC>(*c);
    *c = from_f<TC>(s);
}

// order-fixed split-K reduction with the FULL epilogue of the unsplit kernels (bf16 engine, K-contiguous operands,
// bf16 C): a thread sums the slabs of four columns in slice order and hands them to pgemm::epilogue_tile -- bias,
// activation (+ pre-activation store), activation gradient, dropout, residual.  Lets a Dense GEMM that would fill
// less than half of the chip with 256-row tiles (a few thousand tokens, N = 768) run its K range in several slices.
template <bool DROP>
__global__ __launch_bounds__(256) void splitk_reduce_epi_kernel(GemmArgs p, const float* __restrict__ slabs, int splits) {
    if (DROP) p.drop_seed = polus_eff_seed(p.drop_seed, p.dyn);
    const int nq = (p.N + 3) / 4;
    const long q = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= (long)p.M * nq) return;
    const int m = (int)(q / nq), n = (int)(q % nq) * 4;
    const long total = (long)p.M * p.N;
    const float* s0 = slabs + (long)m * p.N + n;
    const int nvalid = p.N - n;
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    for (int z = 0; z < splits; ++z) {
        float v[4] = {0.f, 0.f, 0.f, 0.f};
        ld4x<float>(s0 + (long)z * total, v, (p.N & 3) == 0, nvalid);
        acc[0] += v[0]; acc[1] += v[1]; acc[2] += v[2]; acc[3] += v[3];
    }
    epilogue_tile<bf16_t, bf16_t, DROP>(p, acc, m, n, 0);
}

template <typename T, bool A_KS, bool B_KS, typename TC, bool VEC, bool DROP = false>
int launch_v(const GemmArgs& a, dim3 grid, hipStream_t st) {
    return polus_launch_lds<gemm_kernel<T, A_KS, B_KS, TC, VEC, DROP>>("polus_gemm", grid, dim3(NTHREADS), SMEM_BYTES, SMEM_BYTES, st, a);
}

template <typename T, bool A_KS, bool B_KS, typename TC>
int launch(const GemmArgs& a, dim3 grid, hipStream_t st) {
    if (a.a_vec && a.b_vec) return launch_v<T, A_KS, B_KS, TC, true>(a, grid, st);
    return launch_v<T, A_KS, B_KS, TC, false>(a, grid, st);
}

template <typename T, typename TC>
int dispatch_layout(int al, int bl, const GemmArgs& a, dim3 grid, hipStream_t st) {
    if (al == POLUS_K_CONTIG && bl == POLUS_K_CONTIG) return launch<T, false, false, TC>(a, grid, st);
    if (al == POLUS_K_CONTIG && bl == POLUS_K_STRIDED) return launch<T, false, true, TC>(a, grid, st);
    if (al == POLUS_K_STRIDED && bl == POLUS_K_STRIDED) return launch<T, true, true, TC>(a, grid, st);
    return launch<T, true, false, TC>(a, grid, st);
}

}  // namespace

extern "C" size_t polus_gemm_workspace_bytes(int M, int N, int split_k) {
    if (split_k <= 1) return 0;
    return (size_t)split_k * (size_t)M * (size_t)N * sizeof(float);
}

// ---- Which kernel a polus_gemm call runs: gemm_route below is the whole decision; the three heuristics it consults come first.

// Epilogue class of an unsplit launch for the kernels with compile-time epilogues (gemm_pp.hip, the ring tiles):
// 0 = alpha / bias, 1 = activation forward (+ pre-activation to aux), 2 = residual (+ dropout), 3 = activation backward
// (aux read); -1 = a combination they are not built for (the launch stays on the run-time epilogue of the ring kernel).
static int epi_mode(const GemmArgs& a, bool c_is_f32) {
    if (c_is_f32 || (a.flags & POLUS_GEMM_ACCUM_C)) return -1;
    const bool fwd = a.flags & POLUS_GEMM_ACT_FWD, bwd = a.flags & POLUS_GEMM_ACT_BWD, drop = a.flags & POLUS_GEMM_DROPOUT;
    if (fwd && (bwd || a.resid || drop)) return -1;
    if (bwd && (a.resid || drop || !a.aux)) return -1;
    if (drop && !a.resid) return -1;
    if (fwd) return 1;
    if (bwd) return 3;
    if (a.resid) return 2;
    return 0;
}

// CUs a ping-pong launch can count on: all of them, minus what a concurrent gradient exchange holds (POLUS_GEMM_RESERVE_CUS: a
// ping-pong workgroup fills a CU's registers and LDS, so a CU running an RCCL channel kernel takes no tile, and a
// 256-tile launch that finds 240 free CUs runs two rounds)
static int pp_cus() { return max(32, polus_num_cus() - polus_reserved_cus()); }

// The ping-pong kernel (gemm_pp.hip, one 8-wave workgroup per CU, 256 x 256 or 256 x 192 tile): more
// FLOP per byte filled into LDS than the ring kernel's 256 x 128, which is what bounds these GEMMs.
// Returns the tile width to use, 0 = stay on the ring kernel.  Needs K % 64 == 0, a compile-time
// epilogue mode and enough tiles to fill the chip: a launch is whole rounds of #CU tiles, so the
// tile width is chosen by the share of the last round that is busy (256 is ~10 % faster per tile).
static int pp_tile(int M, int N, int K, int mode, bool vec16) {
    const int sel = polus_cfg().gemm_pp;
    if (sel < 0 || mode < 0 || K % 64 != 0 || M < 256 || N < 192 || !vec16) return 0;
    if (sel == 256 || sel == 192) return sel;
    const int ncu = pp_cus();
    const long tm = (M + 255) / 256;
    double best = 0.0; int best_tn = 0;
    for (int tn : {256, 192}) {
        const long tiles = tm * ((N + tn - 1) / tn);
        const long rounds = (tiles + ncu - 1) / ncu;
        const double useful = (double)M * N / ((double)rounds * ncu * 256.0 * tn);   // busy share incl. edge waste
        const double score = useful * (tn == 256 ? 1.10 : 1.0);
        if (score > best) { best = score; best_tn = tn; }
    }
    return best >= 0.70 ? best_tn : 0;
}

// Persistent form of a ping-pong launch with several rounds of tiles: one workgroup per CU walks them, the next tile's operand
// prologue under the epilogue.  Returns the number of workgroups, 0 = one workgroup per tile.
// measured (tools/pp_bench.py --ab POLUS_GEMM_PERSIST=0,1,2; bench.py --config c3 | c4 | c5): wins on the 256-wide launches --
// the GELU ones of BERT-base (FFN1 forward, dU: -8 % from cold caches) and every multi-round launch of BERT-large (+0.5 %
// on the c4 step) -- and is neutral to slightly negative on the 192-wide bias-only QKV launch of BERT-base (three exact
// rounds, an epilogue too short to hide anything; c5, 512 tiles of 256 x 192: 34.4 -> 34.8 ms/step); POLUS_GEMM_PERSIST=2
// forces it on every multi-round launch
static int pp_persist_cus(int M, int N, int tn) {
    const int sel = polus_cfg().gemm_persist;
    if (!sel || (tn != 256 && sel < 2)) return 0;
    const int tiles = ((M + 255) / 256) * ((N + tn - 1) / tn);
    return tiles > pp_cus() ? pp_cus() : 0;
}

// 128 x 128 ring tile instead of 256 x 128 (bf16 C, both operands K-contiguous, a compile-time epilogue mode).
// Chosen where the 256 x 128 tiles would take at most 55 % of their 2 x #CU slots (the ping-pong tile has already been
// ruled out by then): tools/ring128_sweep.py, profiles/r02_ring128_sweep.txt -- 4096 x 768 x 3072: 60.6 -> 40.6 us,
// 8192 x 768 x 3072: 61.5 -> 49.5 us, 4096 x 1024 x 4096: 77.0 -> 53.6 us, 8192 x 1024 x 4096 (50 %): 81.0 -> 76.3 us.
static bool use_ring128(int M, int N, int K, int mode) {
    const int sel = polus_cfg().gemm_ring128;
    if (sel < 0 || mode < 0 || M < 128 || N < 128) return false;
    if (sel > 0) return true;
    const long slots = 2L * polus_num_cus();
    const long t256 = (long)((M + 255) / 256) * ((N + 127) / 128);
    return 20 * t256 <= 11 * slots;
}

// Number of K slices a bf16 Dense GEMM (both operands K-contiguous, bf16 C, any epilogue) should be cut into (f32 slabs
// + splitk_reduce_epi_kernel).  1 unless even the 128 x 128 ring tiles would take an eighth or less of their 3 x #CU
// slots (about two thousand tokens at N = 768) and K >= 2048; then enough slices to bring the 256 x 128 slab launch to
// ~3/4 of its slots, each at least 768 deep (<= 8).  Slicing wins in isolation over a wider range
// (profiles/r02_split_sweep.txt) but in the step its f32 slabs cost far more (profiles/r02_ab_auto_split.txt: 6144 and
// 8192 tokens lose 2.5-3 %), and the 128 x 128 tile beats it wherever that tile fills more than an eighth of the chip
// (profiles/r02_ring128_sweep.txt).  The caller passes the result as split_k with polus_gemm_workspace_bytes(M, N, split_k).
extern "C" int polus_gemm_auto_split(int M, int N, int K) {
    if (!polus_cfg().gemm_auto_split || M < 256 || N < 128 || K % 64 != 0 || K < 2048) return 1;
    if (pp_tile(M, N, K, 0, true)) return 1;
    const long ncu = polus_num_cus();
    if (polus_cfg().gemm_ring128 >= 0) {
        const long t128 = (long)((M + 127) / 128) * ((N + 127) / 128);
        if (8 * t128 > 3 * ncu) return 1;
    }
    const long slots = 2 * ncu;
    const long t = (long)((M + 255) / 256) * ((N + 127) / 128);
    if (4 * t > slots) return 1;
    long s = (slots * 3 / 4) / t;
    if (s > K / 768) s = K / 768;
    if (s > 8) s = 8;
    return s < 2 ? 1 : (int)s;
}

enum GemmKernel {
    GEMM_V1,         // gemm.hip, 128 x 128, any dtype / layout / alignment
    GEMM_RING,       // gemm_ring.hip, 256 x 128 (compile-time epilogue when mode >= 0)
    GEMM_RING128,    // gemm_ring.hip, 128 x 128
    GEMM_RING_DROP,  // gemm_ring.hip, 256 x 128 with the dropout epilogue
    GEMM_PP,         // gemm_pp.hip, 256 x tn, one workgroup per tile
    GEMM_PP_PERSIST  // gemm_pp.hip, 256 x tn, persist_cus workgroups walk the tiles
};
enum GemmReduce { REDUCE_NONE, REDUCE_PLAIN /* splitk_reduce_kernel */, REDUCE_EPI /* splitk_reduce_epi_kernel */ };
struct GemmRoute {
    GemmKernel kernel;
    int tn;           // tile width
    int mode;         // compile-time epilogue class (epi_mode), -1 = run-time epilogue
    int drop;
    int splits;       // K slices launched; > 1: the kernel writes f32 slabs and `reduce` follows
    GemmReduce reduce;
    int persist_cus;  // GEMM_PP_PERSIST: workgroups
};

// Everything polus_gemm / polus_gemm_dropout decide about a validated call.  `a` is filled but for k_per_split and partial,
// which follow from the route; splits is the number of non-empty K slices the caller's split_k gives.
static GemmRoute gemm_route(const GemmArgs& a, int dtype, bool c_is_f32, bool a_ks, bool b_ks, int splits) {
    const bool both_kc = !a_ks && !b_ks;
    const int drop = (a.flags & POLUS_GEMM_DROPOUT) != 0;
    const bool epi = a.resid || a.aux || (a.flags & (POLUS_GEMM_ACT_FWD | POLUS_GEMM_ACT_BWD | POLUS_GEMM_DROPOUT));
    // the direct-to-LDS kernels: bf16, whole 16-byte chunks, at least one 256 x 128 tile
    const bool fast = dtype == POLUS_BF16 && a.a_vec && a.b_vec && a.M >= 256 && a.N >= 128 && !polus_cfg().gemm_v1;
    GemmRoute r = {fast ? GEMM_RING : GEMM_V1, 128, -1, drop, splits, REDUCE_NONE, 0};
    if (splits > 1) {
        if (!epi) r.reduce = REDUCE_PLAIN;
        else if (fast && both_kc && !c_is_f32) r.reduce = REDUCE_EPI;
        else r.splits = 1;           // small or unaligned problem: one slice, in-kernel epilogue
    }
    if (!fast || r.splits > 1) return r;
    r.mode = both_kc ? epi_mode(a, c_is_f32) : -1;     // with dropout: 2 or -1
    if (const int tn = pp_tile(a.M, a.N, a.K, r.mode, a.epi_vec16)) {
        r.tn = tn;
        r.persist_cus = pp_persist_cus(a.M, a.N, tn);
        r.kernel = r.persist_cus ? GEMM_PP_PERSIST : GEMM_PP;
    } else if (use_ring128(a.M, a.N, a.K, r.mode)) {
        r.kernel = GEMM_RING128;
    } else if (drop) {
        r.kernel = GEMM_RING_DROP;
    }
    return r;
}

// The slab launch of a split ring GEMM: plain f32 stores of every K slice, the epilogue is left to the reduce kernel.
static GemmArgs slab_args(const GemmArgs& a) {
    GemmArgs s = a;
    s.C = a.partial; s.ldc = a.N; s.c_split_stride = (long)a.M * a.N; s.partial = nullptr;
    s.alpha = 1.0f; s.bias = nullptr; s.flags = 0; s.resid = nullptr; s.aux = nullptr;
    s.epi_vec = (a.N % 4 == 0); s.epi_vec16 = (a.N % 4 == 0) && polus_aligned16(a.partial);
    return s;
}

static int launch_splitk_reduce_epi(const GemmArgs& a, int splits, hipStream_t st) {
    GemmArgs e = a;
    e.partial = nullptr;
    const long quads = (long)a.M * ((a.N + 3) / 4);
    const int blocks = (int)((quads + 255) / 256);
    if (a.flags & POLUS_GEMM_DROPOUT)
        hipLaunchKernelGGL(splitk_reduce_epi_kernel<true>, dim3(blocks), dim3(256), 0, st, e, a.partial, splits);
    else
        hipLaunchKernelGGL(splitk_reduce_epi_kernel<false>, dim3(blocks), dim3(256), 0, st, e, a.partial, splits);
    POLUS_CHECK_LAUNCH("polus_gemm(splitk_reduce_epi)");
    return POLUS_OK;
}

static int launch_v1(int dtype, int c_dtype, int a_layout, int b_layout, const GemmArgs& a, int drop, int splits, hipStream_t st) {
    const dim3 grid(((a.M + BM - 1) / BM) * ((a.N + BN - 1) / BN), 1, splits);
    if (drop) {                       // forward Dense only: K-contiguous operands, C in the compute dtype
        const bool v = a.a_vec && a.b_vec;
        if (dtype == POLUS_BF16) return v ? launch_v<bf16_t, false, false, bf16_t, true, true>(a, grid, st) : launch_v<bf16_t, false, false, bf16_t, false, true>(a, grid, st);
        return v ? launch_v<float, false, false, float, true, true>(a, grid, st) : launch_v<float, false, false, float, false, true>(a, grid, st);
    }
    if (dtype == POLUS_BF16)
        return c_dtype == POLUS_F32 ? dispatch_layout<bf16_t, float>(a_layout, b_layout, a, grid, st)
                                    : dispatch_layout<bf16_t, bf16_t>(a_layout, b_layout, a, grid, st);
    return dispatch_layout<float, float>(a_layout, b_layout, a, grid, st);
}

// C (+)= alpha * sum of the f32 slabs (+ bias), in slice order
static int launch_splitk_reduce(int c_dtype, const float* slabs, int splits, int M, int N, void* C, long ldc, float alpha,
                                const float* bias, int accumulate, const char* what, hipStream_t st) {
    const int blocks = (int)(((long)M * N + 255) / 256);
    if (c_dtype == POLUS_F32)
        hipLaunchKernelGGL(splitk_reduce_kernel<float>, dim3(blocks), dim3(256), 0, st, slabs, splits, M, N, static_cast<float*>(C), ldc, alpha, bias, accumulate);
    else
        hipLaunchKernelGGL(splitk_reduce_kernel<bf16_t>, dim3(blocks), dim3(256), 0, st, slabs, splits, M, N, static_cast<bf16_t*>(C), ldc, alpha, bias, accumulate);
    POLUS_CHECK_LAUNCH(what);
    return POLUS_OK;
}

// K slicing, stated once: a contraction of K > 0 rows in tiles of bk, cut into at most split_k slices of whole tiles.
// asked: split_k brought into 1 .. K tiles (what workspaces are sized for); rows: per slice; count: non-empty slices <= asked.
struct KSlices { int asked, rows, count; };
static KSlices k_slices(int K, int bk, int split_k) {
    const int nkt = (K + bk - 1) / bk;
    const int asked = split_k < 1 ? 1 : (split_k > nkt ? nkt : split_k);
    const int kt_per_split = (nkt + asked - 1) / asked;
    return {asked, kt_per_split * bk, (nkt + kt_per_split - 1) / kt_per_split};
}

// A validated polus_gemm(_dropout) call: the kernels' argument block (but for k_per_split and partial, which the launch
// derives from the route), the route, and the K slicing the route was asked with.
struct GemmPlan {
    GemmArgs a;
    GemmRoute r;
    int bk; KSlices ks;
};

// Validates a call and decides its route; launches nothing and dereferences no pointer (polus_gemm_route hands it made-up
// addresses).  ws_bytes: the caller's workspace size, null where there is no workspace to check (the route query).
static int gemm_plan(int dtype, int a_layout, int b_layout, int c_dtype,
                     const void* A, long lda, const void* B, long ldb, void* C, long ldc,
                     int M, int N, int K, float alpha,
                     const float* bias, const void* resid, long ldr, void* aux, long ldaux,
                     int act, int flags, int split_k, const void* workspace, const size_t* ws_bytes,
                     float drop_p, uint32_t seed, GemmPlan* p) {
    POLUS_REQUIRE(dtype == POLUS_F32 || dtype == POLUS_BF16, "polus_gemm: bad dtype %d", dtype);
    POLUS_REQUIRE(c_dtype == POLUS_F32 || c_dtype == dtype, "polus_gemm: c_dtype must be f32 or dtype");
    POLUS_REQUIRE(M > 0 && N > 0 && K > 0, "polus_gemm: empty problem M=%d N=%d K=%d", M, N, K);
    POLUS_REQUIRE(A && B && C, "polus_gemm: null operand");
    POLUS_REQUIRE((a_layout | 1) == 1 && (b_layout | 1) == 1, "polus_gemm: bad layout");
    POLUS_REQUIRE(lda >= (a_layout == POLUS_K_CONTIG ? K : M), "polus_gemm: lda %ld too small", lda);
    POLUS_REQUIRE(ldb >= (b_layout == POLUS_K_CONTIG ? K : N), "polus_gemm: ldb %ld too small", ldb);
    POLUS_REQUIRE(ldc >= N, "polus_gemm: ldc %ld < N %d", ldc, N);
    POLUS_REQUIRE(!resid || ldr >= N, "polus_gemm: ldr too small");
    POLUS_REQUIRE(!((flags & POLUS_GEMM_ACT_BWD) && !aux), "polus_gemm: ACT_BWD needs aux");
    POLUS_REQUIRE(!aux || ldaux >= N, "polus_gemm: ldaux too small");
    const size_t es = polus_dtype_size(dtype), ecs = polus_dtype_size(c_dtype);
    const int bk = dtype == POLUS_BF16 ? 64 : 32;
    const KSlices ks = k_slices(K, bk, split_k);
    split_k = ks.asked;
    const bool both_kc = a_layout == POLUS_K_CONTIG && b_layout == POLUS_K_CONTIG;
    if (split_k > 1) {
        const bool epi = resid || aux || (flags & (POLUS_GEMM_ACT_FWD | POLUS_GEMM_ACT_BWD | POLUS_GEMM_DROPOUT));
        POLUS_REQUIRE(!epi || (dtype == POLUS_BF16 && c_dtype == POLUS_BF16 && both_kc && !(flags & POLUS_GEMM_ACCUM_C)),
                      "polus_gemm: split_k with a residual / activation / dropout epilogue needs bf16 K-contiguous operands and a bf16 C");
        if (ws_bytes && (!workspace || *ws_bytes < polus_gemm_workspace_bytes(M, N, split_k))) {
            polus_set_error("polus_gemm: workspace %zu < %zu", *ws_bytes, polus_gemm_workspace_bytes(M, N, split_k));
            return POLUS_ERR_WORKSPACE;
        }
    }
    // forward Dense only: K-contiguous operands, C in the compute dtype
    POLUS_REQUIRE(!(flags & POLUS_GEMM_DROPOUT) || (both_kc && c_dtype == dtype), "polus_gemm_dropout: needs K-contiguous operands and c_dtype == dtype");
    GemmArgs& a = p->a;
    a = GemmArgs{};
    a.A = A; a.B = B; a.C = C; a.lda = lda; a.ldb = ldb; a.ldc = ldc;
    a.M = M; a.N = N; a.K = K; a.alpha = alpha;
    a.bias = bias; a.resid = resid; a.ldr = ldr; a.aux = aux; a.ldaux = ldaux;
    a.act = act; a.flags = flags;
    a.drop_inv = 1.0f / (1.0f - drop_p); a.drop_thresh = polus_drop_thresh(drop_p); a.drop_seed = seed;
    a.dyn = polus_dyn();
    const int epc = (int)(16 / es);
    // whole-chunk validity: the contiguous extent of each operand must be a multiple of a chunk
    a.a_vec = polus_aligned16(A) && ((lda * es) % 16 == 0) && ((a_layout == POLUS_K_CONTIG ? K : M) % epc == 0);
    a.b_vec = polus_aligned16(B) && ((ldb * es) % 16 == 0) && ((b_layout == POLUS_K_CONTIG ? K : N) % epc == 0);
    // 4-wide epilogue accesses: every touched row start must be 4-element aligned
    bool ev = (((uintptr_t)C) % (4 * ecs) == 0) && (ldc % 4 == 0);
    if (bias) ev = ev && (((uintptr_t)bias) % 16 == 0);
    if (resid) ev = ev && (((uintptr_t)resid) % (4 * es) == 0) && (ldr % 4 == 0);
    if (aux) ev = ev && (((uintptr_t)aux) % (4 * es) == 0) && (ldaux % 4 == 0);
    a.epi_vec = ev;
    bool ev16 = (((uintptr_t)C) % 16 == 0) && ((ldc * ecs) % 16 == 0);
    if (bias) ev16 = ev16 && (((uintptr_t)bias) % 16 == 0);
    if (resid) ev16 = ev16 && (((uintptr_t)resid) % 16 == 0) && ((ldr * es) % 16 == 0);
    if (aux) ev16 = ev16 && (((uintptr_t)aux) % 16 == 0) && ((ldaux * es) % 16 == 0);
    a.epi_vec16 = ev16 && dtype == POLUS_BF16;
    a.order = polus_cfg().gemm_order;

    p->r = gemm_route(a, dtype, c_dtype == POLUS_F32, a_layout == POLUS_K_STRIDED, b_layout == POLUS_K_STRIDED, ks.count);
    p->bk = bk; p->ks = ks;
    return POLUS_OK;
}

// Launches a plan; dtype, c_dtype and the layouts are those it was made with.
static int gemm_launch(GemmPlan& pl, int dtype, int a_layout, int b_layout, int c_dtype, void* workspace, void* stream) {
    GemmArgs& a = pl.a;
    const GemmRoute& r = pl.r;
    const bool c_is_f32 = c_dtype == POLUS_F32;
    const int a_ks = a_layout == POLUS_K_STRIDED, b_ks = b_layout == POLUS_K_STRIDED;
    if (r.splits > 1) { a.k_per_split = pl.ks.rows; a.partial = static_cast<float*>(workspace); }
    else a.k_per_split = r.kernel == GEMM_V1 ? ((a.K + pl.bk - 1) / pl.bk) * pl.bk : ((a.K + 31) / 32) * 32;    // all of K in whole tiles
    hipStream_t st = static_cast<hipStream_t>(stream);
    int rc = POLUS_ERR_INVALID;
    switch (r.kernel) {
        case GEMM_V1: rc = launch_v1(dtype, c_dtype, a_layout, b_layout, a, r.drop, r.splits, st); break;
        case GEMM_RING:
            rc = r.splits > 1 ? polus_launch_gemm_ring(slab_args(a), 1, a_ks, b_ks, r.splits, -1, st)
                              : polus_launch_gemm_ring(a, c_is_f32, a_ks, b_ks, 1, r.mode, st);
            break;
        case GEMM_RING128: rc = polus_launch_gemm_ring128(a, r.mode, r.drop, st); break;
        case GEMM_RING_DROP: rc = polus_launch_gemm_ring_dropout(a, r.mode, st); break;
        case GEMM_PP:
        case GEMM_PP_PERSIST: rc = polus_launch_gemm_pp(a, r.mode, r.drop, r.tn, r.persist_cus, st); break;
    }
    if (rc != POLUS_OK) return rc;
    switch (r.reduce) {
        case REDUCE_NONE: break;
        case REDUCE_EPI: return launch_splitk_reduce_epi(a, r.splits, st);
        case REDUCE_PLAIN:
            return launch_splitk_reduce(c_dtype, a.partial, r.splits, a.M, a.N, a.C, a.ldc, a.alpha, a.bias,
                                        (a.flags & POLUS_GEMM_ACCUM_C) ? 1 : 0, "polus_gemm(splitk_reduce)", st);
    }
    return POLUS_OK;
}

static int gemm_impl(int dtype, int a_layout, int b_layout, int c_dtype,
                     const void* A, long lda, const void* B, long ldb, void* C, long ldc, int M, int N, int K, float alpha,
                     const float* bias, const void* resid, long ldr, void* aux, long ldaux, int act, int flags, int split_k,
                     void* workspace, size_t workspace_bytes, float drop_p, uint32_t seed, void* stream) {
    GemmPlan pl;
    int rc = gemm_plan(dtype, a_layout, b_layout, c_dtype, A, lda, B, ldb, C, ldc, M, N, K, alpha, bias, resid, ldr, aux, ldaux,
                       act, flags, split_k, workspace, &workspace_bytes, drop_p, seed, &pl);
    return rc != POLUS_OK ? rc : gemm_launch(pl, dtype, a_layout, b_layout, c_dtype, workspace, stream);
}

extern "C" int polus_gemm(int dtype, int a_layout, int b_layout, int c_dtype,
                          const void* A, long lda, const void* B, long ldb, void* C, long ldc,
                          int M, int N, int K, float alpha,
                          const float* bias, const void* resid, long ldr, void* aux, long ldaux,
                          int act, int flags, int split_k, void* workspace, size_t workspace_bytes,
                          void* stream) {
    POLUS_REQUIRE(!(flags & POLUS_GEMM_DROPOUT), "polus_gemm: use polus_gemm_dropout for POLUS_GEMM_DROPOUT");
    return gemm_impl(dtype, a_layout, b_layout, c_dtype, A, lda, B, ldb, C, ldc, M, N, K, alpha, bias, resid, ldr,
                     aux, ldaux, act, flags, split_k, workspace, workspace_bytes, 0.0f, 0u, stream);
}

extern "C" int polus_gemm_dropout(int dtype, int a_layout, int b_layout, int c_dtype,
                                  const void* A, long lda, const void* B, long ldb, void* C, long ldc,
                                  int M, int N, int K, float alpha,
                                  const float* bias, const void* resid, long ldr, void* aux, long ldaux,
                                  int act, int flags, int split_k, void* workspace, size_t workspace_bytes,
                                  float drop_p, uint32_t seed, void* stream) {
    POLUS_REQUIRE(drop_p >= 0.0f && drop_p < 1.0f, "polus_gemm_dropout: need 0 <= p < 1 (got %f)", drop_p);
    POLUS_REQUIRE((long)M * N < (1LL << 32), "polus_gemm_dropout: M*N must fit 32 bits");
    if (drop_p > 0.0f) flags |= POLUS_GEMM_DROPOUT; else flags &= ~POLUS_GEMM_DROPOUT;
    return gemm_impl(dtype, a_layout, b_layout, c_dtype, A, lda, B, ldb, C, ldc, M, N, K, alpha, bias, resid, ldr,
                     aux, ldaux, act, flags, split_k, workspace, workspace_bytes, drop_p, seed, stream);
}

// Host only, no HIP call: what polus_gemm (drop_p == 0) or polus_gemm_dropout (drop_p > 0) would decide for these arguments
// under the current switches.  The pointers count for their alignment alone.  Fails where those calls fail in validation.
extern "C" int polus_gemm_route(int dtype, int a_layout, int b_layout, int c_dtype,
                                const void* A, long lda, const void* B, long ldb, void* C, long ldc,
                                int M, int N, int K, float alpha,
                                const float* bias, const void* resid, long ldr, void* aux, long ldaux,
                                int act, int flags, int split_k, float drop_p, int* out) {
    POLUS_REQUIRE(out, "polus_gemm_route: null out");
    if (drop_p > 0.0f) {
        POLUS_REQUIRE(drop_p < 1.0f, "polus_gemm_dropout: need 0 <= p < 1 (got %f)", drop_p);
        POLUS_REQUIRE((long)M * N < (1LL << 32), "polus_gemm_dropout: M*N must fit 32 bits");
        flags |= POLUS_GEMM_DROPOUT;
    } else {
        POLUS_REQUIRE(drop_p == 0.0f, "polus_gemm_dropout: need 0 <= p < 1 (got %f)", drop_p);
        POLUS_REQUIRE(!(flags & POLUS_GEMM_DROPOUT), "polus_gemm: use polus_gemm_dropout for POLUS_GEMM_DROPOUT");
    }
    GemmPlan pl;
    int rc = gemm_plan(dtype, a_layout, b_layout, c_dtype, A, lda, B, ldb, C, ldc, M, N, K, alpha, bias, resid, ldr, aux, ldaux,
                       act, flags, split_k, nullptr, nullptr, drop_p, 0u, &pl);
    if (rc != POLUS_OK) return rc;
    const GemmRoute& r = pl.r;
    const GemmArgs& a = pl.a;
    const int v[POLUS_GEMM_ROUTE_INTS] = {r.kernel, r.tn, r.mode, r.drop, r.splits, r.reduce, r.persist_cus,
                                          a.a_vec, a.b_vec, a.epi_vec, a.epi_vec16, r.kernel == GEMM_V1 && a.a_vec && a.b_vec};
    for (int i = 0; i < POLUS_GEMM_ROUTE_INTS; ++i) out[i] = v[i];
    return POLUS_OK;
}

// ---- Dense backward for the parameters: dW = dY^T X (+)= and db = column sums of dY, one pass
// over dY.  On the ring kernel the bias gradient rides on the matrix pipe (ones-fragment MFMA).
// Workspace of one call with split_k >= 1 slices: f32 slabs [split_k][n_out][n_in] (none for one slice), then at the next 256-byte
// boundary (cs_off) the ring kernel's column sums [split_k][n_out] or polus_colsum's scratch; the 256-byte tail covers the rounding.
struct DwLayout { size_t cs_off, bytes; };
static DwLayout dw_layout(int T, int n_out, int n_in, int split_k) {
    const size_t slabs = split_k > 1 ? (size_t)split_k * n_out * n_in * sizeof(float) : 0;
    const size_t cs = (size_t)split_k * n_out * sizeof(float), fallback = polus_colsum_workspace_bytes(T, n_out);
    return {(slabs + 255) / 256 * 256, slabs + (cs > fallback ? cs : fallback) + 256};
}
// Shape only, so split_k is taken as asked: the launcher lays out min(split_k, K tiles of its dtype) slices in no more room.
extern "C" size_t polus_dense_bwd_params_workspace_bytes(int T, int n_out, int n_in, int split_k) {
    return dw_layout(T, n_out, n_in, split_k < 1 ? 1 : split_k).bytes;
}

namespace {
__global__ void colsum_splits_kernel(const float* __restrict__ partial, int splits, int n, float* __restrict__ out, int accumulate) {
    int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= n) return;
    float s = 0.f;
    for (int z = 0; z < splits; ++z) s += partial[(long)z * n + c];
    out[c] = accumulate ? out[c] + s : s;
}
}  // namespace

static int launch_colsum_splits(const float* partial, int splits, int n, float* out, int accumulate, const char* what, hipStream_t st) {
    hipLaunchKernelGGL(colsum_splits_kernel, dim3((n + 255) / 256), dim3(256), 0, st, partial, splits, n, out, accumulate);
    POLUS_CHECK_LAUNCH(what);
    return POLUS_OK;
}

// GemmArgs of one dW problem for the ring / ping-pong kernels: A = dY, B = X, both K-strided and whole 16-byte chunks,
// K slices of kps rows, their column sums of dY (the bias gradient) to colsum.
static GemmArgs dw_args(const polus_dw_problem& q, int T, int kps, float* colsum) {
    GemmArgs a = {};
    a.A = q.dY; a.B = q.X; a.lda = q.lddy; a.ldb = q.ldx;
    a.M = q.n_out; a.N = q.n_in; a.K = T; a.alpha = 1.0f;
    a.k_per_split = kps;
    a.a_vec = a.b_vec = 1;
    a.colsum_a = colsum;
    return a;
}
// ... and where the product goes: several slices write f32 slabs [splits][n_out][n_in], a single one writes (or adds to) dW.
static void dw_dest(GemmArgs& a, const polus_dw_problem& q, void* slabs, int accumulate) {
    if (slabs) {
        a.C = slabs; a.ldc = q.n_in; a.c_split_stride = (long)q.n_out * q.n_in;
        a.epi_vec = a.epi_vec16 = (q.n_in % 4 == 0);
    } else {
        a.C = q.dW; a.ldc = q.lddw; a.flags = accumulate ? POLUS_GEMM_ACCUM_C : 0;
        a.epi_vec = a.epi_vec16 = polus_aligned16(q.dW) && (q.lddw % 4 == 0);
    }
}

// The problem fits the ring dW kernel: bf16, dY and X in whole aligned 16-byte chunks (8 elements), at least one 256 x 128 tile.
// The single call adds `db != nullptr`, the grouped one "not POLUS_DW_UNGROUPED, and every problem fits".
static bool dw_fits_ring(int dtype, const polus_dw_problem& q) {
    return dtype == POLUS_BF16 && polus_aligned16(q.dY) && polus_aligned16(q.X) && q.lddy % 8 == 0 && q.ldx % 8 == 0 &&
           q.n_out % 8 == 0 && q.n_in % 8 == 0 && q.n_out >= 256 && q.n_in >= 128 && !polus_cfg().gemm_v1;
}
// Its dW allows the 16-byte accesses of the one-launch reductions of a group (polus_launch_dw_group_reduce / _sk).
static bool dw_reduce_aligned(const polus_dw_problem& q) { return (q.n_in % 4 == 0) && (q.lddw % 4 == 0) && polus_aligned16(q.dW); }

// A validated polus_dense_bwd_params call: the ring kernel or polus_gemm + polus_colsum, and what either form launches with.
struct DwPlan {
    bool ring;
    int kps, splits;    // contraction rows per K slice, K slices launched
    size_t cs_off;      // workspace: the slabs at 0, the column sums (fallback: polus_colsum's scratch) here
    GemmPlan gemm;      // !ring: the polus_gemm the call stands for
};

// Validates and decides, like gemm_plan: no launch, no pointer dereferenced, ws_bytes null where there is no workspace to check.
static int dw_plan(int dtype, const polus_dw_problem& q, int T, int accumulate, int split_k,
                   const void* workspace, const size_t* ws_bytes, DwPlan* p) {
    POLUS_REQUIRE(q.dY && q.X && q.dW, "polus_dense_bwd_params: null pointer");
    POLUS_REQUIRE(T > 0 && q.n_out > 0 && q.n_in > 0, "polus_dense_bwd_params: bad shape");
    const size_t need = polus_dense_bwd_params_workspace_bytes(T, q.n_out, q.n_in, split_k);
    if (ws_bytes && (!workspace || *ws_bytes < need)) { polus_set_error("polus_dense_bwd_params: workspace %zu < %zu", *ws_bytes, need); return POLUS_ERR_WORKSPACE; }
    const KSlices ks = k_slices(T, dtype == POLUS_BF16 ? 64 : 32, split_k);
    p->ring = q.db != nullptr && dw_fits_ring(dtype, q);
    p->kps = ks.rows; p->splits = ks.count;
    p->cs_off = dw_layout(T, q.n_out, q.n_in, ks.asked).cs_off;
    if (p->ring) return POLUS_OK;
    int rc = gemm_plan(dtype, POLUS_K_STRIDED, POLUS_K_STRIDED, POLUS_F32, q.dY, q.lddy, q.X, q.ldx, q.dW, q.lddw, q.n_out, q.n_in, T,
                       1.0f, nullptr, nullptr, 0, nullptr, 0, 0, accumulate ? POLUS_GEMM_ACCUM_C : 0, ks.asked,
                       workspace, ws_bytes ? &p->cs_off : nullptr, 0.0f, 0u, &p->gemm);
    p->splits = p->gemm.r.splits;
    return rc;
}

// polus_dense_bwd_params: plan, then launch
static int dw_impl(int dtype, const polus_dw_problem& q, int T, int accumulate, int split_k, void* workspace, size_t workspace_bytes, void* stream) {
    DwPlan pl;
    int rc = dw_plan(dtype, q, T, accumulate, split_k, workspace, &workspace_bytes, &pl);
    if (rc != POLUS_OK) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    unsigned char* ws = static_cast<unsigned char*>(workspace);
    float* cs_ws = reinterpret_cast<float*>(ws + pl.cs_off);
    if (!pl.ring) {
        rc = gemm_launch(pl.gemm, dtype, POLUS_K_STRIDED, POLUS_K_STRIDED, POLUS_F32, ws, stream);
        if (rc != POLUS_OK || !q.db) return rc;
        return polus_colsum(dtype, q.dY, q.lddy, T, q.n_out, q.db, accumulate, cs_ws, workspace_bytes - pl.cs_off, stream);
    }
    GemmArgs a = dw_args(q, T, pl.kps, cs_ws);
    dw_dest(a, q, pl.splits > 1 ? ws : nullptr, accumulate);
    rc = polus_launch_gemm_ring(a, 1, 1, 1, pl.splits, -1, st);
    if (rc != POLUS_OK) return rc;
    if (pl.splits > 1) {
        rc = launch_splitk_reduce(POLUS_F32, reinterpret_cast<const float*>(ws), pl.splits, q.n_out, q.n_in, q.dW, q.lddw, 1.0f, nullptr,
                                  accumulate ? 1 : 0, "polus_dense_bwd_params(reduce)", st);
        if (rc != POLUS_OK) return rc;
    }
    return launch_colsum_splits(cs_ws, pl.splits, q.n_out, q.db, accumulate ? 1 : 0, "polus_dense_bwd_params(colsum)", st);
}

extern "C" int polus_dense_bwd_params(int dtype, const void* dY, long lddy, const void* X, long ldx,
                                      float* dW, long lddw, float* db, int T, int n_out, int n_in,
                                      int accumulate, int split_k, void* workspace, size_t workspace_bytes,
                                      void* stream) {
    return dw_impl(dtype, {dY, lddy, X, ldx, dW, lddw, db, n_out, n_in}, T, accumulate, split_k, workspace, workspace_bytes, stream);
}

// Host only, no HIP call: out[0] = 1 the ring kernel, 0 the fallback (polus_gemm + polus_colsum); out[1] = K slices launched.
// Fails where polus_dense_bwd_params fails in validation (the workspace aside).
extern "C" int polus_dense_bwd_params_route(int dtype, const void* dY, long lddy, const void* X, long ldx,
                                            float* dW, long lddw, float* db, int T, int n_out, int n_in, int split_k, int* out) {
    POLUS_REQUIRE(out, "polus_dense_bwd_params_route: null out");
    DwPlan pl;
    int rc = dw_plan(dtype, {dY, lddy, X, ldx, dW, lddw, db, n_out, n_in}, T, 0, split_k, nullptr, nullptr, &pl);
    if (rc != POLUS_OK) return rc;
    out[0] = pl.ring; out[1] = pl.splits;
    return POLUS_OK;
}

// ---- The same for several Dense layers at once (all four of an encoder layer): one ring launch
// over the concatenated (split, tile) lists, so the chip fills with 2-3 K-splits instead of 7-28 per
// matrix (each split is an f32 slab written and read back).  All problems share T and accumulate.
// split_k > 0: that many splits for every problem; split_k <= 0: chosen per problem so that the
// launch is one full round of the 2 x #CU workgroup slots.
// Which kernel runs the grouped dW launch: the ping-pong 256 x 256 kernel (gemm_ppks.hip, one workgroup per CU)
// when every problem is at least one tile in both directions and T is whole K-tiles, else the ring kernel
// (256 x 128 tiles, two workgroups per CU).
static bool grouped_use_pp(int n, const polus_dw_problem* pr, int T) {
    if (polus_cfg().gemm_pp < 0 || T % 64 != 0) return false;
    for (int k = 0; k < n; ++k)
        if (pr[k].n_out < 256 || pr[k].n_in < 256) return false;
    return true;
}

// The stream-K hybrid replaces the even split when the library chooses the slices itself (split_k <= 0), the ping-pong
// kernel applies and the even split would leave at least 1/16 of the CUs without a workgroup.
static bool grouped_sk_plan(int n, const polus_dw_problem* pr, int T, int split_k, bool pp, PPKSSKPlan* pl) {
    if (!polus_cfg().dw_streamk || split_k > 0 || !pp) return false;
    int no[POLUS_MAX_GROUP], ni[POLUS_MAX_GROUP];
    for (int k = 0; k < n; ++k) { no[k] = pr[k].n_out; ni[k] = pr[k].n_in; }
    int ncu = polus_num_cus() - polus_reserved_cus();
    if (polus_cfg().dw_sk_cus > 0 && polus_cfg().dw_sk_cus < ncu) ncu = polus_cfg().dw_sk_cus;
    return polus_ppks_sk_plan(no, ni, n, T, ncu, polus_cfg().dw_sk_delta, pl) != 0;
}

static void grouped_splits(int n, const polus_dw_problem* pr, int T, int split_k, int* splits, bool pp) {
    const int nkt = (T + 63) / 64;
    int tiles[POLUS_MAX_GROUP];
    for (int k = 0; k < n; ++k)
        tiles[k] = pp ? polus_ppks_tiles(pr[k].n_out, pr[k].n_in) : ((pr[k].n_out + 255) / 256) * ((pr[k].n_in + 127) / 128);
    if (split_k > 0) {
        for (int k = 0; k < n; ++k) splits[k] = split_k < nkt ? split_k : nkt;
        return;
    }
    // Workgroups go to the 8 XCDs round-robin and each tile list is padded to a multiple of 8, so
    // XCD 0 receives ceil(tiles/8) workgroups of every (problem, split).  All workgroups run for
    // about the same (long) time: one more than the resident workgroups per XCD (2 per CU for the ring
    // kernel, 1 for the ping-pong kernel) on any XCD doubles the kernel.
    const int slots_xcd = (pp ? 1 : 2) * polus_num_cus() / 8;
    int per_xcd[POLUS_MAX_GROUP], total_xcd = 0;
    for (int k = 0; k < n; ++k) { per_xcd[k] = (tiles[k] + 7) / 8; total_xcd += per_xcd[k]; }
    int base = slots_xcd / (total_xcd > 0 ? total_xcd : 1);
    if (base < 1) base = 1;
    const int cap = nkt / 4 > 0 ? nkt / 4 : 1;          // >= 256 contraction rows per split
    if (base > cap) base = cap;
    int used = 0;
    for (int k = 0; k < n; ++k) { splits[k] = base; used += per_xcd[k] * base; }
    // hand the remaining slots to the problems with the most tiles that still fit, one extra split each
    bool given[POLUS_MAX_GROUP] = {false};
    for (;;) {
        int best = -1;
        for (int k = 0; k < n; ++k)
            if (!given[k] && splits[k] < cap && used + per_xcd[k] <= slots_xcd && (best < 0 || tiles[k] > tiles[best])) best = k;
        if (best < 0) break;
        given[best] = true; ++splits[best]; used += per_xcd[best];
    }
}

// What runs a grouped dW call: one polus_dense_bwd_params call per problem, or one launch over every problem's (slice, tile)
// list by the ring kernel, by the ping-pong kernel with an even split, or by its stream-K hybrid.  The values are the codes of
// out[0] of polus_dense_bwd_params_grouped_route and the indices of ops.DW_GROUPED_KERNELS (tests/gemm_cases.py restates them).
enum DwGroupedKernel { DWG_ONE_BY_ONE, DWG_RING, DWG_PP, DWG_PP_SK };

// The plan has two stages.  grouped_dw_layout: everything the workspace query and the launcher of a grouped dW must agree on,
// computed in one place from what the query knows: (n, problems' shapes, T, split_k) and the switches.
// `pp` is grouped_use_pp, decided from shapes alone: the query cannot see the dtype and the pointers that can send the launcher
// to its one-by-one fallback.  That is safe.  Where the grouped kernel runs, the launcher's conditions imply those of the
// ring kernel, so pp (and sk, which needs pp) are exactly the kernel it takes and the layout here is the one it writes.
// Where it does not, no grouped kernel writes anything: each problem runs alone with splits[k] slices -- a count sized for
// ping-pong tiles is as valid a split_k as any -- in a workspace of at least `single` bytes, which is sized for those counts.
// grouped_dw_plan: the route, which needs dtype and pointers; the launcher switches on it and the report copies it.
struct GroupedDwPlan {
    bool pp, sk;                                             // layout: ping-pong tiles; there is a stream-K launch (skp)
    int splits[POLUS_MAX_GROUP];                             // K slices asked for, per problem
    int kps[POLUS_MAX_GROUP], eff[POLUS_MAX_GROUP];          // even split: contraction rows per slice, non-empty slices
    size_t slab_off[POLUS_MAX_GROUP], cs_off[POLUS_MAX_GROUP];   // even split: slabs [splits][n_out][n_in], column sums [splits][n_out]
    PPKSSKPlan skp;                                          // sk: the stream-K launch, its slabs at offset 0 ...
    size_t sk_cs_off[POLUS_MAX_GROUP];                       // ... and its column sums [slots][n_out]
    size_t bytes;                                            // the largest of the even, stream-K and one-by-one layouts
    DwGroupedKernel kernel; bool fused_reduce;               // route; every slab reduction and bias gradient in one launch
    int slices[POLUS_MAX_GROUP];                             // K slices each problem runs with (stream-K: its slots per tile)
};

static void grouped_dw_layout(int n, const polus_dw_problem* pr, int T, int split_k, GroupedDwPlan* pl) {
    pl->pp = grouped_use_pp(n, pr, T);
    grouped_splits(n, pr, T, split_k, pl->splits, pl->pp);
    size_t off = 0, single = 0;
    for (int k = 0; k < n; ++k) {
        const KSlices ks = k_slices(T, 64, pl->splits[k]);
        pl->kps[k] = ks.rows; pl->eff[k] = ks.count;
        pl->slab_off[k] = off;
        if (pl->splits[k] > 1) off += (((size_t)pl->splits[k] * pr[k].n_out * pr[k].n_in * sizeof(float) + 255) / 256) * 256;
        pl->cs_off[k] = off;
        off += (((size_t)pl->splits[k] * pr[k].n_out * sizeof(float) + 255) / 256) * 256;
        const size_t b = polus_dense_bwd_params_workspace_bytes(T, pr[k].n_out, pr[k].n_in, pl->splits[k]);   // the fallback runs them one by one
        if (b > single) single = b;
    }
    pl->bytes = off + 256;
    pl->sk = grouped_sk_plan(n, pr, T, split_k, pl->pp, &pl->skp);
    if (pl->sk) {
        off = (size_t)pl->skp.ttot * pl->skp.slots * 256 * 256 * sizeof(float);
        for (int k = 0; k < n; ++k) {
            pl->sk_cs_off[k] = off;
            off += (((size_t)pl->skp.slots * pr[k].n_out * sizeof(float) + 255) / 256) * 256;
        }
        if (off + 256 > pl->bytes) pl->bytes = off + 256;
    }
    if (single > pl->bytes) pl->bytes = single;
}

extern "C" size_t polus_dense_bwd_params_grouped_workspace_bytes(int n, const polus_dw_problem* problems, int T, int split_k) {
    if (n < 1 || n > POLUS_MAX_GROUP || !problems || T < 1) return 0;
    GroupedDwPlan pl;
    grouped_dw_layout(n, problems, T, split_k, &pl);
    return pl.bytes;
}

// Validates a grouped dW call and decides all of it, like gemm_plan: no launch, ws_bytes null where there is no workspace to check.
static int grouped_dw_plan(int dtype, int n, const polus_dw_problem* problems, int T, int split_k,
                           const void* workspace, const size_t* ws_bytes, GroupedDwPlan* pl) {
    POLUS_REQUIRE(problems && n >= 1 && n <= POLUS_MAX_GROUP && T > 0, "polus_dense_bwd_params_grouped: bad arguments");
    bool ring = !polus_cfg().dw_ungrouped, aligned = true;
    for (int k = 0; k < n; ++k) {
        const polus_dw_problem& q = problems[k];
        POLUS_REQUIRE(q.dY && q.X && q.dW && q.n_out > 0 && q.n_in > 0, "polus_dense_bwd_params_grouped: problem %d: bad arguments", k);
        ring = ring && dw_fits_ring(dtype, q);
        aligned = aligned && dw_reduce_aligned(q);
    }
    grouped_dw_layout(n, problems, T, split_k, pl);
    if (ws_bytes && (!workspace || *ws_bytes < pl->bytes)) { polus_set_error("polus_dense_bwd_params_grouped: workspace %zu < %zu", *ws_bytes, pl->bytes); return POLUS_ERR_WORKSPACE; }
    // an unaligned dW drops the stream-K launch for the even split, and the one-launch reduce of either
    pl->kernel = !ring ? DWG_ONE_BY_ONE : pl->sk && aligned ? DWG_PP_SK : pl->pp ? DWG_PP : DWG_RING;
    pl->fused_reduce = ring && aligned && (pl->kernel == DWG_PP_SK || polus_cfg().dw_fused_reduce);
    for (int k = 0; k < n; ++k) pl->slices[k] = pl->kernel == DWG_PP_SK ? pl->skp.slots : pl->eff[k];
    for (int k = 0; k < n && !ring; ++k) {      // one by one: the plan that each problem's call will make for itself
        DwPlan one;
        int rc = dw_plan(dtype, problems[k], T, 0, pl->splits[k], nullptr, nullptr, &one);
        if (rc != POLUS_OK) return rc;
        pl->slices[k] = one.splits;
    }
    return POLUS_OK;
}

// Per-problem arrays for the one-launch reductions of a group (polus_launch_dw_group_reduce / _sk).
struct DwGroupOut {
    const float* slabs[POLUS_MAX_GROUP]; float* cs[POLUS_MAX_GROUP];
    float* dW[POLUS_MAX_GROUP]; float* db[POLUS_MAX_GROUP];
    long lddw[POLUS_MAX_GROUP]; int n_out[POLUS_MAX_GROUP], n_in[POLUS_MAX_GROUP];
};
// slab_off: null where the slabs are not per problem (stream-K) -- else problem k has slabs iff eff[k] > 1
static DwGroupOut dw_group_out(int n, const polus_dw_problem* pr, unsigned char* ws, const size_t* cs_off, const size_t* slab_off, const int* eff) {
    DwGroupOut o;
    for (int k = 0; k < n; ++k) {
        const polus_dw_problem& q = pr[k];
        o.slabs[k] = slab_off && eff[k] > 1 ? reinterpret_cast<const float*>(ws + slab_off[k]) : nullptr;
        o.cs[k] = q.db ? reinterpret_cast<float*>(ws + cs_off[k]) : nullptr;
        o.dW[k] = q.dW; o.db[k] = q.db; o.lddw[k] = q.lddw; o.n_out[k] = q.n_out; o.n_in[k] = q.n_in;
    }
    return o;
}

// DWG_PP_SK: the stream-K launch and its one-launch reduce.
static int launch_dwg_sk(int n, const polus_dw_problem* problems, int T, int accumulate, const GroupedDwPlan& pl, unsigned char* ws, hipStream_t st) {
    const DwGroupOut o = dw_group_out(n, problems, ws, pl.sk_cs_off, nullptr, nullptr);
    GemmArgs ga[POLUS_MAX_GROUP];
    for (int k = 0; k < n; ++k) {
        ga[k] = dw_args(problems[k], T, 0, nullptr);     // the stream-K kernel addresses slabs and column sums itself
        ga[k].epi_vec = ga[k].epi_vec16 = 1;
    }
    int rc = polus_launch_gemm_ppks_sk(ga, pl.skp, reinterpret_cast<float*>(ws), o.cs, st);
    if (rc != POLUS_OK) return rc;
    return polus_launch_dw_group_reduce_sk(pl.skp, reinterpret_cast<const float*>(ws), o.cs, o.dW, o.db, o.lddw, o.n_out, o.n_in, accumulate ? 1 : 0, st);
}

// DWG_RING / DWG_PP: eff[k] even slices per problem in one launch, then the reductions in one launch or one by one.
static int launch_dwg_even(int n, const polus_dw_problem* problems, int T, int accumulate, const GroupedDwPlan& pl, unsigned char* ws, hipStream_t st) {
    const DwGroupOut o = dw_group_out(n, problems, ws, pl.cs_off, pl.slab_off, pl.eff);
    GemmArgs ga[POLUS_MAX_GROUP];
    for (int k = 0; k < n; ++k) {
        ga[k] = dw_args(problems[k], T, pl.kps[k], o.cs[k]);
        dw_dest(ga[k], problems[k], pl.eff[k] > 1 ? ws + pl.slab_off[k] : nullptr, accumulate);
    }
    int rc = pl.kernel == DWG_PP ? polus_launch_gemm_ppks_grouped_dw(ga, n, pl.eff, st) : polus_launch_gemm_ring_grouped_dw(ga, n, pl.eff, st);
    if (rc != POLUS_OK) return rc;
    if (pl.fused_reduce)
        return polus_launch_dw_group_reduce(n, o.slabs, o.cs, o.dW, o.db, o.lddw, o.n_out, o.n_in, pl.eff, accumulate ? 1 : 0, st);
    for (int k = 0; k < n; ++k) {
        const polus_dw_problem& q = problems[k];
        if (pl.eff[k] > 1) {
            rc = launch_splitk_reduce(POLUS_F32, o.slabs[k], pl.eff[k], q.n_out, q.n_in, q.dW, q.lddw, 1.0f, nullptr, accumulate ? 1 : 0,
                                      "polus_dense_bwd_params_grouped(reduce)", st);
            if (rc != POLUS_OK) return rc;
        }
        if (q.db) {
            rc = launch_colsum_splits(o.cs[k], pl.eff[k], q.n_out, q.db, accumulate ? 1 : 0, "polus_dense_bwd_params_grouped(colsum)", st);
            if (rc != POLUS_OK) return rc;
        }
    }
    return POLUS_OK;
}

extern "C" int polus_dense_bwd_params_grouped(int dtype, int n, const polus_dw_problem* problems, int T, int accumulate,
                                              int split_k, void* workspace, size_t workspace_bytes, void* stream) {
    GroupedDwPlan pl;
    int rc = grouped_dw_plan(dtype, n, problems, T, split_k, workspace, &workspace_bytes, &pl);
    if (rc != POLUS_OK) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    unsigned char* ws = static_cast<unsigned char*>(workspace);
    switch (pl.kernel) {
        case DWG_ONE_BY_ONE:            // each problem as a call of its own; one without db takes the fallback, then polus_gemm alone
            for (int k = 0; k < n && rc == POLUS_OK; ++k)
                rc = dw_impl(dtype, problems[k], T, accumulate, pl.splits[k], workspace, workspace_bytes, stream);
            return rc;
        case DWG_RING:
        case DWG_PP: return launch_dwg_even(n, problems, T, accumulate, pl, ws, st);
        case DWG_PP_SK: return launch_dwg_sk(n, problems, T, accumulate, pl, ws, st);
    }
    return POLUS_ERR_INVALID;
}

// Host only, no HIP call: out[0] = the DwGroupedKernel of a grouped dW call, out[1] = 1 when the slab reductions and bias
// gradients of the group take one launch, out[2 + k] = K slices of problem k (stream-K: its slots per tile).
extern "C" int polus_dense_bwd_params_grouped_route(int dtype, int n, const polus_dw_problem* problems, int T, int split_k, int* out) {
    POLUS_REQUIRE(out, "polus_dense_bwd_params_grouped_route: null out");
    GroupedDwPlan pl;
    int rc = grouped_dw_plan(dtype, n, problems, T, split_k, nullptr, nullptr, &pl);
    if (rc != POLUS_OK) return rc;
    out[0] = pl.kernel; out[1] = pl.fused_reduce;
    for (int k = 0; k < n; ++k) out[2 + k] = pl.slices[k];
    return POLUS_OK;
}
