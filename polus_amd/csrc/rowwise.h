// What the row-wise kernel files share: norm.hip (LayerNorm, column sums) and embed.hip (embedding gather + LayerNorm).
// All HBM-bound: one wave64 owns one row, lanes read 4 consecutive features per chunk
// (8-B bf16 / 16-B f32 accesses, 512 B / 1 KiB per wave-instruction), row statistics by
// wave reductions, cross-row (per-feature) sums accumulated in registers over a
// grid-stride row loop and finished by an order-fixed two-stage reduction (no atomics,
// bitwise reproducible).
#pragma once
#include <type_traits>

#include "common.h"

// ---------------------------------------------------------------- host side
// norm.hip's launchers that embed.hip uses too.  polus_ln_finalize: the fixed-order reduction of partial[blocks][3H] into
// dgamma / dbeta (/ dbias when want_bias) in `stages` launches -- what POLUS_LN_FIN_SINGLE says for the LayerNorm proper, 1 for
// the embedding whatever the switch says (its sums have always been one stage over up to 256 workgroups; two would change
// their order).  `who` names the caller in a launch error.
int polus_ln_finalize(float* partial, int blocks, int H, int want_bias, float* dgamma, float* dbeta, float* dbias,
                      int accumulate, int stages, hipStream_t st, const char* who);
int polus_colsum_launch(int dtype, const void* x, long ldx, int rows, int cols, float* out, int accumulate,
                        const int32_t* sel, int sel_value, void* workspace, size_t workspace_bytes, hipStream_t st);

// Calls f(std::integral_constant<int, NC>{}) for the smallest listed NC (ascending) with n <= NC, the last one if there is
// none: turns a chunk count into a template argument and instantiates f for exactly the listed values.
template <int NC, int... REST, typename F>
void for_chunks(int n, F&& f) {
    if constexpr (sizeof...(REST) == 0) f(std::integral_constant<int, NC>{});
    else if (n <= NC) f(std::integral_constant<int, NC>{});
    else for_chunks<REST...>(n, f);
}
// f(T{}, NC) with T the element type of `dtype` (POLUS_BF16, else float) as well
template <int... NCS, typename F>
void for_dtype_chunks(int dtype, int n, F&& f) {
    if (dtype == POLUS_BF16) for_chunks<NCS...>(n, [&](auto nc) { f(bf16_t{}, nc); });
    else for_chunks<NCS...>(n, [&](auto nc) { f(float{}, nc); });
}

// The anonymous namespace is deliberate: the kernels of both files live in one, and their symbols carry DropArgs.
namespace {

constexpr int MAXC = 8;           // chunks of 256 features per row: H <= 2048 (template NC <= MAXC)
constexpr int WAVES = 16;         // waves per workgroup (1024 threads): 4096 waves at 256 workgroups
constexpr int LN_THREADS = 64 * WAVES;
constexpr int MAX_PARTIAL_BLOCKS = 256;   // per-feature partial sums [blocks][3][H] f32, flushed once per 64 rows
constexpr int ROW_GRID_CAP = 4096;        // workgroups of the kernels that keep no partials; more rows go round the grid-stride loop
constexpr int HW_FWD_GRID_CAP = 16384;    // the same for ln_fwd_hw_kernel's 4-wave workgroups

inline int chunks256(int H) { return (H + 255) / 256; }
// workgroups for `rows` rows at `per_block` rows each, at most `cap` (the kernels stride over the rest)
inline int capped_blocks(int rows, int per_block, int cap) {
    int b = (rows + per_block - 1) / per_block;
    return b > cap ? cap : (b < 1 ? 1 : b);
}
inline int row_blocks(int rows) { return capped_blocks(rows, WAVES, ROW_GRID_CAP); }       // 16 waves, a wave per row
inline int ln_blocks(int rows) { return capped_blocks(rows, WAVES, MAX_PARTIAL_BLOCKS); }  // embed_bwd_ln_kernel: a partial per workgroup

// word-table scatter of the embedding backward: 1..4 = embed_scatter_atomic_kernel<NC> (NC chunks cover H), else one of
enum { SCATTER_WIDE = 5, SCATTER_OWNER = 6 };
inline int scatter_route(int H, int deterministic) {
    return deterministic ? SCATTER_OWNER : (chunks256(H) <= 4 ? chunks256(H) : SCATTER_WIDE);
}

// What every LayerNorm and embedding entry point asks of its shape and its dropout arguments: rows of whole quads, at
// most MAXC chunks; p in [0, 1) and, with dropout on, an element index row * H + col that fits the hash's 32 bits.
inline bool rowwise_shape_ok(long rows, int H) { return rows > 0 && H > 0 && H % 4 == 0 && H <= 256 * MAXC; }
inline bool rowwise_drop_ok(float drop_p, long rows, int H) {
    return drop_p >= 0.f && drop_p < 1.f && (!(drop_p > 0.f) || rows * H < (1LL << 32));
}

struct DropArgs { unsigned thresh, seed; float inv; const PolusDyn* dyn = nullptr; };   // thresh == 0: no dropout; dyn: see common.h
inline DropArgs drop_args(float drop_p, uint32_t seed) {
    return DropArgs{drop_p > 0.f ? polus_drop_thresh(drop_p) : 0u, seed, 1.0f / (1.0f - drop_p), polus_dyn()};
}

// a token or type id outside its table takes the nearest row of it
__device__ __forceinline__ int clamp_id(int v, int n) { return v < 0 ? 0 : (v >= n ? n - 1 : v); }

template <typename T, int NC>
__device__ __forceinline__ void load_row(const T* row, int H, int lane, float (&v)[NC][4]) {
#pragma unroll
    for (int c = 0; c < NC; ++c) {
        int col = (lane + 64 * c) * 4;
        if (col < H) load4<T>(row + col, v[c]);
        else { v[c][0] = v[c][1] = v[c][2] = v[c][3] = 0.f; }
    }
}

// per-feature f32 vector (gamma / beta) -> registers, once per wave
template <int NC>
__device__ __forceinline__ void load_feat(const float* __restrict__ p, int H, int lane, float (&v)[NC][4]) {
#pragma unroll
    for (int c = 0; c < NC; ++c) {
        int col = (lane + 64 * c) * 4;
        if (col < H) load4<float>(p + col, v[c]);
        else { v[c][0] = v[c][1] = v[c][2] = v[c][3] = 0.f; }
    }
}

// mean / rstd of one row held in registers (two-pass, biased variance)
template <int NC>
__device__ __forceinline__ void row_stats(const float (&v)[NC][4], int H, int lane, float eps,
                                          float& mean, float& rstd) {
    float s = 0.f;
#pragma unroll
    for (int c = 0; c < NC; ++c) s += (v[c][0] + v[c][1]) + (v[c][2] + v[c][3]);
    mean = wave_sum(s) / (float)H;
    float q = 0.f;
#pragma unroll
    for (int c = 0; c < NC; ++c) {
        int col = (lane + 64 * c) * 4;
        if (col < H) {
#pragma unroll
            for (int e = 0; e < 4; ++e) { float d = v[c][e] - mean; q += d * d; }
        }
    }
    float var = wave_sum(q) / (float)H;
    rstd = 1.0f / sqrtf(var + eps);
}

template <typename T, int NC>
__device__ __forceinline__ void normalize_store(const float (&v)[NC][4], const float (&gv)[NC][4], const float (&bv)[NC][4],
                                                T* y, int H, int lane, float mean, float rstd,
                                                unsigned dthresh = 0, unsigned dseed = 0, float dinv = 1.f, unsigned rowbase = 0) {
#pragma unroll
    for (int c = 0; c < NC; ++c) {
        int col = (lane + 64 * c) * 4;
        if (col < H) {
            float o[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) o[e] = (v[c][e] - mean) * rstd * gv[c][e] + bv[c][e];
            // rowbase = row * H and col are multiples of 4: even-aligned run
            if (dthresh) polus_dropout_run<4>(o, dseed, rowbase + col, dthresh, dinv, true);
            store4<T>(y + col, o);
        }
    }
}

// Shared tail of the LN backward kernels: given x-hat pieces and dy for one row, produce dx
// and accumulate the per-feature sums.
template <int NC> struct ColAcc { float dg[NC][4], db[NC][4], dbias[NC][4]; };

template <int NC>
__device__ __forceinline__ void colacc_zero(ColAcc<NC>& a) {
#pragma unroll
    for (int c = 0; c < NC; ++c)
#pragma unroll
        for (int e = 0; e < 4; ++e) a.dg[c][e] = a.db[c][e] = a.dbias[c][e] = 0.f;
}

// block-level, order-fixed combine of the WAVES waves' column accumulators into
// partial[block][3][H]
template <int NC>
__device__ __forceinline__ void colacc_flush(const ColAcc<NC>& a, float* lds /*[3*H]*/, float* partial, int H,
                                             int lane, int wid, int want_bias) {
    for (int w = 0; w < WAVES; ++w) {
        if (wid == w) {
#pragma unroll
            for (int c = 0; c < NC; ++c) {
                int col = (lane + 64 * c) * 4;
                if (col < H) {
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        if (w == 0) {
                            lds[col + e] = a.dg[c][e]; lds[H + col + e] = a.db[c][e]; lds[2 * H + col + e] = a.dbias[c][e];
                        } else {
                            lds[col + e] += a.dg[c][e]; lds[H + col + e] += a.db[c][e]; lds[2 * H + col + e] += a.dbias[c][e];
                        }
                    }
                }
            }
        }
        __syncthreads();
    }
    float* dst = partial + (long)blockIdx.x * 3 * H;
    int n = (want_bias ? 3 : 2) * H;
    for (int idx = threadIdx.x; idx < n; idx += blockDim.x) dst[idx] = lds[idx];
}

// Same for small workgroups (W waves): every wave drops its sums into its own LDS slice
// [W][3H], then all threads add the W slices in fixed order -- one barrier instead of W.
template <int NC, int W>
__device__ __forceinline__ void colacc_flush_par(const ColAcc<NC>& a, float* lds /*[W][3*H]*/, float* partial, int H,
                                                 int lane, int wid, int want_bias) {
    float* mine = lds + (long)wid * 3 * H;
#pragma unroll
    for (int c = 0; c < NC; ++c) {
        int col = (lane + 64 * c) * 4;
        if (col < H) {
            *reinterpret_cast<float4*>(mine + col) = make_float4(a.dg[c][0], a.dg[c][1], a.dg[c][2], a.dg[c][3]);
            *reinterpret_cast<float4*>(mine + H + col) = make_float4(a.db[c][0], a.db[c][1], a.db[c][2], a.db[c][3]);
            *reinterpret_cast<float4*>(mine + 2 * H + col) = make_float4(a.dbias[c][0], a.dbias[c][1], a.dbias[c][2], a.dbias[c][3]);
        }
    }
    __syncthreads();
    float* dst = partial + (long)blockIdx.x * 3 * H;
    int n = (want_bias ? 3 : 2) * H;
    for (int idx = threadIdx.x; idx < n; idx += blockDim.x) {
        float t = lds[idx];
#pragma unroll
        for (int w = 1; w < W; ++w) t += lds[(long)w * 3 * H + idx];
        dst[idx] = t;
    }
}

template <typename T, typename TDX, int NC>
__device__ __forceinline__ void ln_bwd_row(const float (&xv)[NC][4], const T* dyrow, const float (&gv)[NC][4],
                                           TDX* dxrow, int H, int lane, float mu, float rs, ColAcc<NC>& acc,
                                           int want_bias, TDX* dxm_row = nullptr, DropArgs out_drop = DropArgs{0, 0, 1.f},
                                           DropArgs in_drop = DropArgs{0, 0, 1.f}, unsigned rowbase = 0) {
    float dy[NC][4];
    load_row<T, NC>(dyrow, H, lane, dy);
    if (in_drop.thresh) {   // y = dropout(LN(x)): the incoming gradient passes through the same mask
#pragma unroll
        for (int c = 0; c < NC; ++c) {
            int col = (lane + 64 * c) * 4;
            polus_dropout_run<4>(dy[c], in_drop.seed, rowbase + col, in_drop.thresh, in_drop.inv, true);
        }
    }
    float s1 = 0.f, s2 = 0.f;
    float xh[NC][4], dxh[NC][4];
#pragma unroll
    for (int c = 0; c < NC; ++c) {
        int col = (lane + 64 * c) * 4;
        if (col < H) {
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                xh[c][e] = (xv[c][e] - mu) * rs;
                dxh[c][e] = dy[c][e] * gv[c][e];
                s1 += dxh[c][e];
                s2 += dxh[c][e] * xh[c][e];
                acc.dg[c][e] += dy[c][e] * xh[c][e];
                acc.db[c][e] += dy[c][e];
            }
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e) xh[c][e] = dxh[c][e] = 0.f;
        }
    }
    s1 = wave_sum(s1) / (float)H;
    s2 = wave_sum(s2) / (float)H;
#pragma unroll
    for (int c = 0; c < NC; ++c) {
        int col = (lane + 64 * c) * 4;
        if (col < H) {
            float o[4], om[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) { o[e] = (dxh[c][e] - s1 - xh[c][e] * s2) * rs; om[e] = o[e]; }
            // x = dropout(dense) + residual: the Dense (and its bias) see the masked gradient
            if (out_drop.thresh) polus_dropout_run<4>(om, out_drop.seed, rowbase + col, out_drop.thresh, out_drop.inv, true);
            if (want_bias) {
#pragma unroll
                for (int e = 0; e < 4; ++e) acc.dbias[c][e] += om[e];
            }
            store4<TDX>(dxrow + col, o);
            if (dxm_row) store4<TDX>(dxm_row + col, om);
        }
    }
}

}  // namespace
