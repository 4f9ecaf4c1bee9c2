// LayerNorm fwd / bwd with its deferred finalize, and deterministic column sums (gfx950).  The device helpers and the
// conventions of the row-wise kernels are in rowwise.h; the embedding layer that shares them is embed.hip.
#include "rowwise.h"

namespace {

template <typename T, int NC>
__global__ __launch_bounds__(LN_THREADS) void ln_fwd_kernel(const T* __restrict__ x, const float* __restrict__ gamma,
                                                     const float* __restrict__ beta, T* __restrict__ y,
                                                     float* __restrict__ mean, float* __restrict__ rstd,
                                                     int rows, int H, float eps) {
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    float gv[NC][4], bv[NC][4];
    load_feat<NC>(gamma, H, lane, gv);
    load_feat<NC>(beta, H, lane, bv);
    for (int row = blockIdx.x * WAVES + wid; row < rows; row += gridDim.x * WAVES) {
        float v[NC][4];
        load_row<T, NC>(x + (long)row * H, H, lane, v);
        float mu, rs;
        row_stats<NC>(v, H, lane, eps, mu, rs);
        normalize_store<T, NC>(v, gv, bv, y + (long)row * H, H, lane, mu, rs);
        if (lane == 0) { mean[row] = mu; rstd[row] = rs; }
    }
}

// ---- bf16, H % 256 == 0: a HALF-wave per row, 16-byte accesses.  Lane (half = lane >> 5, hl = lane & 31) owns
// columns 8 (hl + 32 c) .. +7 of row 2 w + half: one wave-instruction moves 2 x 512 contiguous bytes (two rows) at
// 16 B per lane instead of 512 B at 8 B per lane -- 8-byte accesses run at 0.54-0.70 of the 16-byte rate.
typedef __bf16 bf16x8v __attribute__((ext_vector_type(8)));
__device__ __forceinline__ float half_sum(float v) {
#pragma unroll
    for (int o = 16; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
template <int NC>
__global__ __launch_bounds__(LN_THREADS) void ln_fwd_hw_kernel(const bf16_t* __restrict__ x, const float* __restrict__ gamma,
                                                                const float* __restrict__ beta, bf16_t* __restrict__ y,
                                                                float* __restrict__ mean, float* __restrict__ rstd,
                                                                int rows, int H, float eps) {
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6, half = lane >> 5, hl = lane & 31;
    float gv[NC][8], bv[NC][8];
#pragma unroll
    for (int c = 0; c < NC; ++c) {
        const int col = (hl + 32 * c) * 8;
        load4<float>(gamma + col, *reinterpret_cast<float(*)[4]>(&gv[c][0])); load4<float>(gamma + col + 4, *reinterpret_cast<float(*)[4]>(&gv[c][4]));
        load4<float>(beta + col, *reinterpret_cast<float(*)[4]>(&bv[c][0])); load4<float>(beta + col + 4, *reinterpret_cast<float(*)[4]>(&bv[c][4]));
    }
    const float invH = 1.0f / (float)H;
    const int nw = blockDim.x >> 6;                      // waves of this workgroup (the launch picks 4 or 16)
    for (int row = (blockIdx.x * nw + wid) * 2 + half; row < rows; row += gridDim.x * nw * 2) {
        float v[NC][8];
        float s = 0.f;
#pragma unroll
        for (int c = 0; c < NC; ++c) {
            const bf16x8v t = *reinterpret_cast<const bf16x8v*>(x + (long)row * H + (hl + 32 * c) * 8);
#pragma unroll
            for (int e = 0; e < 8; ++e) { v[c][e] = (float)t[e]; s += v[c][e]; }
        }
        const float mu = half_sum(s) * invH;
        float q = 0.f;
#pragma unroll
        for (int c = 0; c < NC; ++c)
#pragma unroll
            for (int e = 0; e < 8; ++e) { const float d = v[c][e] - mu; q += d * d; }
        const float rs = 1.0f / sqrtf(half_sum(q) * invH + eps);
#pragma unroll
        for (int c = 0; c < NC; ++c) {
            bf16x8v o;
#pragma unroll
            for (int e = 0; e < 8; ++e) o[e] = (bf16_t)((v[c][e] - mu) * rs * gv[c][e] + bv[c][e]);
            *reinterpret_cast<bf16x8v*>(y + (long)row * H + (hl + 32 * c) * 8) = o;
        }
        if (hl == 0) { mean[row] = mu; rstd[row] = rs; }
    }
}

// LayerNorm backward proper runs 4-wave workgroups.  At ~210 VGPRs two of them fit a CU, so 512 are resident at
// once: the default cap (POLUS_LN_BWD_BLOCKS).  Their [blocks][3H] partials are reduced in fixed order by one
// finalize launch up to POLUS_LN_FIN_SINGLE (512) rows, above that in two stages, groups of FIN_GROUP first.
// Single-stream kernel time per step (profiles/r02_ln_bwd_reduce_shapes.txt): 1024 blocks / two stages 25.8 us +
// 2 x 4.8 us per LayerNorm; 512 / two stages 22.0 + 2 x 4.7; 512 / one stage 21.8 + 4.8.
constexpr int BWD_WAVES = 4, BWD_MAX_BLOCKS = 1024, FIN_GROUP = 128;
template <typename T, int NC>
__global__ __launch_bounds__(64 * BWD_WAVES) void ln_bwd_kernel(const T* __restrict__ dy, const T* __restrict__ x,
                                                     const float* __restrict__ gamma, const float* __restrict__ mean,
                                                     const float* __restrict__ rstd, T* __restrict__ dx,
                                                     float* __restrict__ partial, int rows, int H, int want_bias,
                                                     T* __restrict__ dxm, DropArgs drop) {
    if (drop.thresh) drop.seed = polus_eff_seed(drop.seed, drop.dyn);
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    float* lds = reinterpret_cast<float*>(smem_raw);
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    ColAcc<NC> acc;
    colacc_zero(acc);
    float gv[NC][4];
    load_feat<NC>(gamma, H, lane, gv);
    for (int row = blockIdx.x * BWD_WAVES + wid; row < rows; row += gridDim.x * BWD_WAVES) {
        float xv[NC][4];
        load_row<T, NC>(x + (long)row * H, H, lane, xv);
        ln_bwd_row<T, T, NC>(xv, dy + (long)row * H, gv, dx + (long)row * H, H, lane, mean[row], rstd[row], acc, want_bias,
                             dxm ? dxm + (long)row * H : nullptr, drop, DropArgs{0, 0, 1.f}, (unsigned)row * (unsigned)H);
    }
    colacc_flush_par<NC, BWD_WAVES>(acc, lds, partial, H, lane, wid, want_bias);
}

// out_k[c] (+)= sum_p partial[p][k*seg + c]: 64 columns x 16 partial groups per block,
// groups combined in fixed order.
// blockIdx.y selects a group of `pgroup` consecutive partial rows (first stage of a two-stage
// reduction: out0 then is a [groups][ncols] array, seg = ncols, written at row blockIdx.y).
__global__ __launch_bounds__(1024) void colsum_finalize_kernel(const float* __restrict__ partial, int P, int pstride,
                                                               int ncols, int seg, float* out0, float* out1,
                                                               float* out2, int accumulate, int pgroup = 0) {
    __shared__ float red[16][64];
    const int cx = threadIdx.x & 63, gy = threadIdx.x >> 6;
    const int col = blockIdx.x * 64 + cx;
    float s = 0.f;
    if (pgroup > 0) {
        const int p0 = blockIdx.y * pgroup;
        partial += (long)p0 * pstride;
        P = min(pgroup, P - p0);
        out0 += (long)blockIdx.y * ncols;
    }
    if (col < ncols) {
        // fixed order p = gy, gy + 16, ...; eight loads in flight (the rows are latency-, not bandwidth-bound)
#pragma unroll 8
        for (int p = gy; p < P; p += 16) s += partial[(long)p * pstride + col];
    }
    red[gy][cx] = s;
    __syncthreads();
    if (gy == 0 && col < ncols) {
        float t = 0.f;
#pragma unroll
        for (int k = 0; k < 16; ++k) t += red[k][cx];
        int which = col / seg, c = col % seg;
        float* out = which == 0 ? out0 : which == 1 ? out1 : out2;
        if (out) out[c] = accumulate ? out[c] + t : t;
    }
}

// LayerNorm backward, half-wave per row (see ln_fwd_hw_kernel).  The two half-waves of a wave own the SAME columns
// (of two different rows), so the per-feature sums of a wave are the lane-wise sums of its halves (one xor-32
// shuffle at flush time); the block's waves are then combined through LDS exactly as in the wave-per-row kernel.
template <int NC>
__global__ __launch_bounds__(64 * BWD_WAVES) void ln_bwd_hw_kernel(const bf16_t* __restrict__ dy, const bf16_t* __restrict__ x,
                                                                    const float* __restrict__ gamma, const float* __restrict__ mean,
                                                                    const float* __restrict__ rstd, bf16_t* __restrict__ dx,
                                                                    float* __restrict__ partial, int rows, int H, int want_bias,
                                                                    bf16_t* __restrict__ dxm, DropArgs drop) {
    if (drop.thresh) drop.seed = polus_eff_seed(drop.seed, drop.dyn);
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    float* lds = reinterpret_cast<float*>(smem_raw);
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6, half = lane >> 5, hl = lane & 31;
    float gv[NC][8], adg[NC][8], adb[NC][8], abias[NC][8];
#pragma unroll
    for (int c = 0; c < NC; ++c) {
        const int col = (hl + 32 * c) * 8;
        load4<float>(gamma + col, *reinterpret_cast<float(*)[4]>(&gv[c][0])); load4<float>(gamma + col + 4, *reinterpret_cast<float(*)[4]>(&gv[c][4]));
#pragma unroll
        for (int e = 0; e < 8; ++e) adg[c][e] = adb[c][e] = abias[c][e] = 0.f;
    }
    const float invH = 1.0f / (float)H;
    for (int row = (blockIdx.x * BWD_WAVES + wid) * 2 + half; row < rows; row += gridDim.x * BWD_WAVES * 2) {
        const float mu = mean[row], rs = rstd[row];
        float xh[NC][8], dxh[NC][8];
        float s1 = 0.f, s2 = 0.f;
#pragma unroll
        for (int c = 0; c < NC; ++c) {
            const long off = (long)row * H + (hl + 32 * c) * 8;
            const bf16x8v tx = *reinterpret_cast<const bf16x8v*>(x + off);
            const bf16x8v td = *reinterpret_cast<const bf16x8v*>(dy + off);
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const float d = (float)td[e];
                xh[c][e] = ((float)tx[e] - mu) * rs;
                dxh[c][e] = d * gv[c][e];
                s1 += dxh[c][e];
                s2 += dxh[c][e] * xh[c][e];
                adg[c][e] += d * xh[c][e];
                adb[c][e] += d;
            }
        }
        s1 = half_sum(s1) * invH;
        s2 = half_sum(s2) * invH;
#pragma unroll
        for (int c = 0; c < NC; ++c) {
            const int col = (hl + 32 * c) * 8;
            float o[8], om[8];
#pragma unroll
            for (int e = 0; e < 8; ++e) { o[e] = (dxh[c][e] - s1 - xh[c][e] * s2) * rs; om[e] = o[e]; }
            if (drop.thresh) polus_dropout_run<8>(om, drop.seed, (unsigned)row * (unsigned)H + col, drop.thresh, drop.inv, true);
            if (want_bias) {
#pragma unroll
                for (int e = 0; e < 8; ++e) abias[c][e] += om[e];
            }
            bf16x8v t;
#pragma unroll
            for (int e = 0; e < 8; ++e) t[e] = (bf16_t)o[e];
            *reinterpret_cast<bf16x8v*>(dx + (long)row * H + col) = t;
            if (dxm) {
#pragma unroll
                for (int e = 0; e < 8; ++e) t[e] = (bf16_t)om[e];
                *reinterpret_cast<bf16x8v*>(dxm + (long)row * H + col) = t;
            }
        }
    }
    // the wave's sums = its two halves, lane-wise; then the block's waves through LDS in fixed order
    float* mine = lds + (long)wid * 3 * H;
#pragma unroll
    for (int c = 0; c < NC; ++c) {
        const int col = (hl + 32 * c) * 8;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            adg[c][e] += __shfl_xor(adg[c][e], 32, 64);
            adb[c][e] += __shfl_xor(adb[c][e], 32, 64);
            abias[c][e] += __shfl_xor(abias[c][e], 32, 64);
        }
        if (half == 0) {
            *reinterpret_cast<float4*>(mine + col) = make_float4(adg[c][0], adg[c][1], adg[c][2], adg[c][3]);
            *reinterpret_cast<float4*>(mine + col + 4) = make_float4(adg[c][4], adg[c][5], adg[c][6], adg[c][7]);
            *reinterpret_cast<float4*>(mine + H + col) = make_float4(adb[c][0], adb[c][1], adb[c][2], adb[c][3]);
            *reinterpret_cast<float4*>(mine + H + col + 4) = make_float4(adb[c][4], adb[c][5], adb[c][6], adb[c][7]);
            *reinterpret_cast<float4*>(mine + 2 * H + col) = make_float4(abias[c][0], abias[c][1], abias[c][2], abias[c][3]);
            *reinterpret_cast<float4*>(mine + 2 * H + col + 4) = make_float4(abias[c][4], abias[c][5], abias[c][6], abias[c][7]);
        }
    }
    __syncthreads();
    float* dst = partial + (long)blockIdx.x * 3 * H;
    const int n = (want_bias ? 3 : 2) * H;
    for (int idx = threadIdx.x; idx < n; idx += blockDim.x) {
        float t = lds[idx];
#pragma unroll
        for (int w = 1; w < BWD_WAVES; ++w) t += lds[(long)w * 3 * H + idx];
        dst[idx] = t;
    }
}

// ---- generic column sums: grid (col tiles of 1024, row chunks); thread owns 4 columns
template <typename T>
__global__ __launch_bounds__(256) void colsum_partial_kernel(const T* __restrict__ x, long ldx, int rows, int cols,
                                                             int rows_per_chunk, float* __restrict__ partial,
                                                             const int32_t* __restrict__ sel, int sel_value, int vec) {
    const int col = (blockIdx.x * 256 + threadIdx.x) * 4;
    const int r0 = blockIdx.y * rows_per_chunk, r1 = min(rows, r0 + rows_per_chunk);
    float a[4] = {0.f, 0.f, 0.f, 0.f};
    if (col < cols) {
        const int nv = cols - col;
        for (int r = r0; r < r1; ++r) {
            if (sel && sel[r] != sel_value) continue;
            float v[4];
            const T* p = x + (long)r * ldx + col;
            if (vec && nv >= 4) load4<T>(p, v);
            else {
#pragma unroll
                for (int e = 0; e < 4; ++e) v[e] = e < nv ? to_f<T>(p[e]) : 0.f;
            }
#pragma unroll
            for (int e = 0; e < 4; ++e) a[e] += v[e];
        }
#pragma unroll
        for (int e = 0; e < 4; ++e)
            if (e < nv) partial[(long)blockIdx.y * cols + col + e] = a[e];
    }
}

}  // namespace

// ---------------------------------------------------------------- routes and grids: decided here, once; polus_rowwise_route reports them
enum LnRoute { LN_ROUTE_NONE = 0, LN_WAVE_F32 = 1, LN_WAVE_BF16 = 2, LN_HALFWAVE = 3 };   // NONE: bad dtype
static LnRoute ln_route(int dtype, int rows, int H) {
    if (dtype == POLUS_F32) return LN_WAVE_F32;
    if (dtype != POLUS_BF16) return LN_ROUTE_NONE;
    // a half-wave per row wants whole 256-feature chunks, at most four of them, and rows in pairs
    return H % 256 == 0 && H <= 1024 && rows % 2 == 0 && polus_cfg().ln_halfwave ? LN_HALFWAVE : LN_WAVE_BF16;
}
// 4-wave workgroups for the half-wave forward: a 16-wave one (98 registers) fills a CU alone, so the launch ran as two rounds of 256
// workgroups that all load, then all store; small workgroups keep five per CU in different phases (10.4 -> 9.4 us at 16384 x 768,
// tools/ln_bench.py, round 4)
constexpr int HW_FWD_WAVES = 4;
static int ln_fwd_blocks(LnRoute route, int rows) {
    return route == LN_HALFWAVE ? capped_blocks(rows / 2, HW_FWD_WAVES, HW_FWD_GRID_CAP) : row_blocks(rows);
}
static int ln_bwd_blocks(int rows) {
    int cap = polus_cfg().ln_bwd_blocks;
    return capped_blocks(rows, BWD_WAVES, cap < 64 ? 64 : (cap > BWD_MAX_BLOCKS ? BWD_MAX_BLOCKS : cap));
}
static int ln_finalize_stages(int blocks) { return blocks > polus_cfg().ln_fin_single ? 2 : 1; }

extern "C" int polus_rowwise_route(int dtype, int rows, int H, int deterministic, int* out) {
    const LnRoute route = ln_route(dtype, rows, H);
    POLUS_REQUIRE(route != LN_ROUTE_NONE, "polus_rowwise_route: bad dtype %d", dtype);
    POLUS_REQUIRE(rowwise_shape_ok(rows, H) && out, "polus_rowwise_route: bad arguments (rows=%d, H=%d)", rows, H);
    const int r[POLUS_ROWWISE_ROUTE_INTS] = {route, ln_fwd_blocks(route, rows), ln_bwd_blocks(rows), ln_finalize_stages(ln_bwd_blocks(rows)),
                                             scatter_route(H, deterministic), row_blocks(rows), ln_blocks(rows)};
    memcpy(out, r, sizeof r);
    return POLUS_OK;
}

int polus_ln_finalize(float* partial, int blocks, int H, int want_bias, float* dgamma, float* dbeta, float* dbias,
                      int accumulate, int stages, hipStream_t st, const char* who) {
    const int ncols = (want_bias ? 3 : 2) * H, tiles = (ncols + 63) / 64;
    int pstride = 3 * H;
    if (stages > 1) {
        // two fixed-order stages: [blocks] -> [groups] -> result (a single stage would leave most
        // of the chip idle: ncols/64 workgroups walking 1024 rows each)
        const int groups = (blocks + FIN_GROUP - 1) / FIN_GROUP;
        float* part2 = partial + (size_t)blocks * 3 * H;
        hipLaunchKernelGGL(colsum_finalize_kernel, dim3(tiles, groups), dim3(1024), 0, st,
                           partial, blocks, pstride, ncols, ncols, part2, (float*)nullptr, (float*)nullptr, 0, FIN_GROUP);
        POLUS_CHECK_LAUNCH(who);
        partial = part2; blocks = groups; pstride = ncols;
    }
    hipLaunchKernelGGL(colsum_finalize_kernel, dim3(tiles), dim3(1024), 0, st,
                       partial, blocks, pstride, ncols, H, dgamma, dbeta, dbias, accumulate, 0);
    POLUS_CHECK_LAUNCH(who);
    return POLUS_OK;
}

// partial rows of a column sum: the workspace holds this many; the launch may need fewer once the rows are dealt out evenly
static int colsum_chunks(int rows) { return capped_blocks(rows, 64, 256); }

int polus_colsum_launch(int dtype, const void* x, long ldx, int rows, int cols, float* out, int accumulate,
                        const int32_t* sel, int sel_value, void* workspace, size_t workspace_bytes, hipStream_t st) {
    int chunks = colsum_chunks(rows);
    int rpc = (rows + chunks - 1) / chunks;
    chunks = (rows + rpc - 1) / rpc;
    size_t need = (size_t)chunks * cols * sizeof(float);
    if (!workspace || workspace_bytes < need) { polus_set_error("polus_colsum: workspace %zu < %zu", workspace_bytes, need); return POLUS_ERR_WORKSPACE; }
    float* partial = static_cast<float*>(workspace);
    dim3 grid((cols + 1023) / 1024, chunks);
    size_t es = polus_dtype_size(dtype);
    int vec = (((uintptr_t)x) % (4 * es) == 0) && (ldx % 4 == 0);
    if (dtype == POLUS_BF16)
        hipLaunchKernelGGL(colsum_partial_kernel<bf16_t>, grid, dim3(256), 0, st, (const bf16_t*)x, ldx, rows, cols, rpc, partial, sel, sel_value, vec);
    else
        hipLaunchKernelGGL(colsum_partial_kernel<float>, grid, dim3(256), 0, st, (const float*)x, ldx, rows, cols, rpc, partial, sel, sel_value, vec);
    POLUS_CHECK_LAUNCH("polus_colsum(partial)");
    hipLaunchKernelGGL(colsum_finalize_kernel, dim3((cols + 63) / 64), dim3(1024), 0, st,
                       partial, chunks, cols, cols, cols, out, (float*)nullptr, (float*)nullptr, accumulate);
    POLUS_CHECK_LAUNCH("polus_colsum(finalize)");
    return POLUS_OK;
}

extern "C" size_t polus_layernorm_bwd_workspace_bytes(int rows, int H) {
    // [blocks][3H] block partials (max of the two users: LayerNorm proper, embedding LayerNorm)
    // + [groups][3H] second-stage partials
    int b = max(ln_bwd_blocks(rows), ln_blocks(rows));
    int groups = (b + FIN_GROUP - 1) / FIN_GROUP;
    return ((size_t)b + groups) * 3 * (size_t)H * sizeof(float);
}

extern "C" int polus_layernorm_fwd(int dtype, const void* x, const float* gamma, const float* beta,
                                   void* y, float* mean, float* rstd, int rows, int H, float eps, void* stream) {
    POLUS_REQUIRE(x && gamma && beta && y && mean && rstd, "polus_layernorm_fwd: null pointer");
    POLUS_REQUIRE(rowwise_shape_ok(rows, H), "polus_layernorm_fwd: H=%d must be a multiple of 4, <= %d", H, 256 * MAXC);
    POLUS_REQUIRE(polus_aligned16(x) && polus_aligned16(y) && polus_aligned16(gamma) && polus_aligned16(beta),
                  "polus_layernorm_fwd: pointers must be 16-byte aligned");
    hipStream_t st = static_cast<hipStream_t>(stream);
    const LnRoute route = ln_route(dtype, rows, H);
    const dim3 grid(ln_fwd_blocks(route, rows));
    if (route == LN_HALFWAVE)
        for_chunks<1, 2, 3, 4>(chunks256(H), [&](auto nc) {
            hipLaunchKernelGGL(ln_fwd_hw_kernel<nc()>, grid, dim3(64 * HW_FWD_WAVES), 0, st, (const bf16_t*)x, gamma, beta, (bf16_t*)y, mean, rstd, rows, H, eps);
        });
    else if (route != LN_ROUTE_NONE)
        for_dtype_chunks<1, 2, 3, 4, 8>(dtype, chunks256(H), [&](auto t, auto nc) {
            using T = decltype(t);
            hipLaunchKernelGGL((ln_fwd_kernel<T, nc()>), grid, dim3(LN_THREADS), 0, st, (const T*)x, gamma, beta, (T*)y, mean, rstd, rows, H, eps);
        });
    else POLUS_FAIL("polus_layernorm_fwd: bad dtype");
    POLUS_CHECK_LAUNCH("polus_layernorm_fwd");
    return POLUS_OK;
}

extern "C" int polus_layernorm_bwd(int dtype, const void* dy, const void* x, const float* gamma,
                                   const float* mean, const float* rstd, void* dx,
                                   float* dgamma, float* dbeta, float* dbias, int accumulate,
                                   int rows, int H, void* dx_masked, float drop_p, uint32_t seed,
                                   void* workspace, size_t workspace_bytes, void* stream) {
    // dgamma == dbeta == null: leave the per-workgroup partial sums in `workspace` (which the caller then owns until
    // polus_layernorm_bwd_finalize has run on it, on any stream ordered behind this call); `dbias` non-null still says
    // that the bias-gradient column sums are wanted
    const bool defer = !dgamma && !dbeta;
    POLUS_REQUIRE(dy && x && gamma && mean && rstd && dx && (defer || (dgamma && dbeta)), "polus_layernorm_bwd: null pointer");
    POLUS_REQUIRE(rowwise_drop_ok(drop_p, rows, H) && (long)rows * H < (1LL << 32), "polus_layernorm_bwd: bad dropout arguments");
    POLUS_REQUIRE(!(drop_p > 0.f) || dx_masked, "polus_layernorm_bwd: dropout needs dx_masked");
    POLUS_REQUIRE(rowwise_shape_ok(rows, H), "polus_layernorm_bwd: bad H=%d", H);
    POLUS_REQUIRE(polus_aligned16(x) && polus_aligned16(dy) && polus_aligned16(dx) && polus_aligned16(gamma),
                  "polus_layernorm_bwd: pointers must be 16-byte aligned");
    size_t need = polus_layernorm_bwd_workspace_bytes(rows, H);
    if (!workspace || workspace_bytes < need) { polus_set_error("polus_layernorm_bwd: workspace %zu < %zu", workspace_bytes, need); return POLUS_ERR_WORKSPACE; }
    hipStream_t st = static_cast<hipStream_t>(stream);
    LnRoute route = ln_route(dtype, rows, H);
    // the backward's own rule: the half-wave kernel stores dx_masked 16 bytes at a time, so one that is not aligned so takes a wave per row
    if (route == LN_HALFWAVE && !polus_aligned16(dx_masked)) route = LN_WAVE_BF16;
    const DropArgs drop = drop_args(drop_p, seed);
    const int blocks = ln_bwd_blocks(rows), wb = dbias ? 1 : 0;
    const dim3 grid(blocks), block(64 * BWD_WAVES);
    float* partial = static_cast<float*>(workspace);
    const size_t lds = (size_t)BWD_WAVES * 3 * (size_t)H * sizeof(float);
    if (route == LN_HALFWAVE)
        for_chunks<1, 2, 3, 4>(chunks256(H), [&](auto nc) {
            hipLaunchKernelGGL(ln_bwd_hw_kernel<nc()>, grid, block, lds, st, (const bf16_t*)dy, (const bf16_t*)x, gamma, mean, rstd, (bf16_t*)dx, partial, rows, H, wb, (bf16_t*)dx_masked, drop);
        });
    else if (route != LN_ROUTE_NONE)
        for_dtype_chunks<1, 2, 3, 4, 8>(dtype, chunks256(H), [&](auto t, auto nc) {
            using T = decltype(t);
            hipLaunchKernelGGL((ln_bwd_kernel<T, nc()>), grid, block, lds, st, (const T*)dy, (const T*)x, gamma, mean, rstd, (T*)dx, partial, rows, H, wb, (T*)dx_masked, drop);
        });
    else POLUS_FAIL("polus_layernorm_bwd: bad dtype");
    POLUS_CHECK_LAUNCH("polus_layernorm_bwd");
    if (defer) return POLUS_OK;
    return polus_ln_finalize(partial, blocks, H, wb, dgamma, dbeta, dbias, accumulate, ln_finalize_stages(blocks), st,
                             "polus_layernorm_bwd(finalize)");
}

// Second half of polus_layernorm_bwd when it was called with dgamma = dbeta = null: the fixed-order reduction of the
// [workgroups][3H] partials left in `workspace` into dgamma / dbeta (/ dbias), by the launcher the direct form calls.
extern "C" int polus_layernorm_bwd_finalize(void* workspace, size_t workspace_bytes, int rows, int H, float* dgamma, float* dbeta,
                                            float* dbias, int accumulate, void* stream) {
    POLUS_REQUIRE(workspace && dgamma && dbeta && rows > 0 && H > 0 && H % 4 == 0, "polus_layernorm_bwd_finalize: bad arguments");
    size_t need = polus_layernorm_bwd_workspace_bytes(rows, H);
    if (workspace_bytes < need) { polus_set_error("polus_layernorm_bwd_finalize: workspace %zu < %zu", workspace_bytes, need); return POLUS_ERR_WORKSPACE; }
    const int blocks = ln_bwd_blocks(rows);
    return polus_ln_finalize(static_cast<float*>(workspace), blocks, H, dbias ? 1 : 0, dgamma, dbeta, dbias, accumulate,
                             ln_finalize_stages(blocks), static_cast<hipStream_t>(stream), "polus_layernorm_bwd_finalize");
}

extern "C" size_t polus_colsum_workspace_bytes(int rows, int cols) {
    return (size_t)colsum_chunks(rows) * (size_t)cols * sizeof(float);
}

extern "C" int polus_colsum(int dtype, const void* x, long ldx, int rows, int cols, float* out, int accumulate,
                            void* workspace, size_t workspace_bytes, void* stream) {
    POLUS_REQUIRE(x && out && rows > 0 && cols > 0 && ldx >= cols, "polus_colsum: bad arguments");
    POLUS_REQUIRE(dtype == POLUS_F32 || dtype == POLUS_BF16, "polus_colsum: bad dtype");
    return polus_colsum_launch(dtype, x, ldx, rows, cols, out, accumulate, nullptr, 0, workspace, workspace_bytes,
                               static_cast<hipStream_t>(stream));
}
