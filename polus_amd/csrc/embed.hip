// Embedding layer (gfx950): gather word + position + type -> LayerNorm forward; backward = LayerNorm backward of the
// gathered sum, three forms of the word-table scatter, position and type gradients.  Device helpers: rowwise.h.
#include "rowwise.h"

namespace {

template <int NC>
__device__ __forceinline__ void gather_sum(const float* word, const float* pos, const float* type, int id, int s,
                                           int tt, int H, int lane, float (&v)[NC][4]) {
    const float* w = word + (long)id * H;
    const float* p = pos + (long)s * H;
    const float* t = type + (long)tt * H;
#pragma unroll
    for (int c = 0; c < NC; ++c) {
        int col = (lane + 64 * c) * 4;
        if (col < H) {
            float a[4], b[4], d[4];
            load4<float>(w + col, a); load4<float>(p + col, b); load4<float>(t + col, d);
#pragma unroll
            for (int e = 0; e < 4; ++e) v[c][e] = (a[e] + d[e]) + b[e];  // word + type + pos (oracle order)
        } else { v[c][0] = v[c][1] = v[c][2] = v[c][3] = 0.f; }
    }
}

template <typename T, int NC>
__global__ __launch_bounds__(LN_THREADS) void embed_fwd_kernel(const int32_t* __restrict__ ids, const int32_t* __restrict__ tts,
                                                        const float* __restrict__ word, const float* __restrict__ pos,
                                                        const float* __restrict__ type, const float* __restrict__ gamma,
                                                        const float* __restrict__ beta, T* __restrict__ y,
                                                        float* __restrict__ mean, float* __restrict__ rstd,
                                                        int B, int S, int H, int vocab, int type_vocab, float eps,
                                                        unsigned dthresh, unsigned dseed, float dinv, const PolusDyn* dyn) {
    if (dthresh) dseed = polus_eff_seed(dseed, dyn);
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const int rows = B * S;
    float gv[NC][4], bv[NC][4];
    load_feat<NC>(gamma, H, lane, gv);
    load_feat<NC>(beta, H, lane, bv);
    for (int row = blockIdx.x * WAVES + wid; row < rows; row += gridDim.x * WAVES) {
        const int id = clamp_id(ids[row], vocab);
        const int tt = clamp_id(tts ? tts[row] : 0, type_vocab);
        float v[NC][4];
        gather_sum<NC>(word, pos, type, id, row % S, tt, H, lane, v);
        float mu, rs;
        row_stats<NC>(v, H, lane, eps, mu, rs);
        normalize_store<T, NC>(v, gv, bv, y + (long)row * H, H, lane, mu, rs, dthresh, dseed, dinv, (unsigned)row * (unsigned)H);
        if (lane == 0) { mean[row] = mu; rstd[row] = rs; }
    }
}

// LN backward of the embedding sum: de (f32 workspace) + gamma/beta partials
template <typename T, int NC>
__global__ __launch_bounds__(LN_THREADS) void embed_bwd_ln_kernel(const T* __restrict__ dy, const int32_t* __restrict__ ids,
                                                           const int32_t* __restrict__ tts, const float* __restrict__ word,
                                                           const float* __restrict__ pos, const float* __restrict__ type,
                                                           const float* __restrict__ gamma, const float* __restrict__ mean,
                                                           const float* __restrict__ rstd, float* __restrict__ de,
                                                           float* __restrict__ partial, int B, int S, int H, int vocab,
                                                           int type_vocab, DropArgs in_drop) {
    if (in_drop.thresh) in_drop.seed = polus_eff_seed(in_drop.seed, in_drop.dyn);
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    float* lds = reinterpret_cast<float*>(smem_raw);
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const int rows = B * S;
    ColAcc<NC> acc;
    colacc_zero(acc);
    float gv[NC][4];
    load_feat<NC>(gamma, H, lane, gv);
    for (int row = blockIdx.x * WAVES + wid; row < rows; row += gridDim.x * WAVES) {
        const int id = clamp_id(ids[row], vocab);
        const int tt = clamp_id(tts ? tts[row] : 0, type_vocab);
        float xv[NC][4];
        gather_sum<NC>(word, pos, type, id, row % S, tt, H, lane, xv);
        ln_bwd_row<T, float, NC>(xv, dy + (long)row * H, gv, de + (long)row * H, H, lane, mean[row], rstd[row], acc, 0,
                                 nullptr, DropArgs{0, 0, 1.f}, in_drop, (unsigned)row * (unsigned)H);
    }
    colacc_flush(acc, lds, partial, H, lane, wid, 0);
}

// word-table gradient, atomic form.  f32 atomics run at the memory side at ~1.3 TB/s when spread over rows but 14x
// slower when many adders meet on ONE row (MI355X_MICROARCH.md, Global float atomics), and a quarter of a padded
// batch is the [PAD] id, in runs at the end of every sequence.  Each wave therefore takes SC_RUN consecutive tokens,
// loads all of their rows first (every row is needed exactly once; vmcnt retires in order, so a load issued after
// an atomic would wait for it), combines the duplicates among them in registers -- the first occurrence sums, in
// token order -- and issues one atomic row-add per distinct id, 256 contiguous bytes per wave-instruction.  No LDS,
// no workgroup synchronisation, no wave sums more than SC_RUN rows.  168 -> 79 us with the combining alone at the
// headline shape (runs of 4: 96 us, of 16: 140 us -- fewer, longer waves).  NC = ceil(H / 256) <= 4.
constexpr int SC_RUN = 8, SC_WAVES = 8;
template <int NC>
__global__ __launch_bounds__(64 * SC_WAVES) void embed_scatter_atomic_kernel(const float* __restrict__ de, const int32_t* __restrict__ ids,
                                                                      float* __restrict__ gword, int rows, int H, int vocab) {
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const long stride = (long)gridDim.x * SC_WAVES * SC_RUN;
    for (long r0 = ((long)blockIdx.x * SC_WAVES + wid) * SC_RUN; r0 < rows; r0 += stride) {
        int mine = -1;                                       // lanes 0 .. SC_RUN-1 hold the (clamped) ids of the run
        if (lane < SC_RUN && r0 + lane < rows) mine = clamp_id(ids[r0 + lane], vocab);
        float row[SC_RUN][NC][4];
#pragma unroll
        for (int j = 0; j < SC_RUN; ++j) {
            const bool valid = r0 + j < rows;                // wave-uniform
            const float* src = de + (r0 + j) * H + lane;
#pragma unroll
            for (int c = 0; c < NC; ++c)
#pragma unroll
                for (int k = 0; k < 4; ++k)
                    row[j][c][k] = (valid && c * 256 + k * 64 + lane < H) ? src[c * 256 + k * 64] : 0.f;
        }
#pragma unroll
        for (int t = 0; t < SC_RUN; ++t) {
            const int id = __shfl(mine, t, 64);              // wave-uniform
            const unsigned same = (unsigned)__ballot(mine == id);
            if (id < 0 || (same & ((1u << t) - 1u))) continue;   // past the last row, or an earlier token owns this id
            float* dst = gword + (long)id * H + lane;
#pragma unroll
            for (int c = 0; c < NC; ++c)
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    float acc = row[t][c][k];
#pragma unroll
                    for (int j = t + 1; j < SC_RUN; ++j)
                        if ((same >> j) & 1u) acc += row[j][c][k];
                    if (c * 256 + k * 64 + lane < H) atomicAdd(dst + c * 256 + k * 64, acc);
                }
        }
    }
}
// any H: one wave per token, no combining
__global__ __launch_bounds__(LN_THREADS) void embed_scatter_atomic_wide_kernel(const float* __restrict__ de, const int32_t* __restrict__ ids,
                                                                        float* __restrict__ gword, int rows, int H, int vocab) {
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    for (int row = blockIdx.x * WAVES + wid; row < rows; row += gridDim.x * WAVES) {
        const int id = clamp_id(ids[row], vocab);
        const float* src = de + (long)row * H;
        float* dst = gword + (long)id * H;
        for (int col = lane; col < H; col += 64) atomicAdd(dst + col, src[col]);
    }
}

// word-table gradient, reproducible form: the first occurrence of an id owns it and adds
// the rows of every occurrence in token order.
__global__ __launch_bounds__(LN_THREADS) void embed_scatter_owner_kernel(const float* __restrict__ de, const int32_t* __restrict__ ids,
                                                                  float* __restrict__ gword, int rows, int H, int vocab) {
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    for (int row = blockIdx.x * WAVES + wid; row < rows; row += gridDim.x * WAVES) {
        // duplicates are found on the CLAMPED id: two different out-of-range ids land on the same table row
        auto clampid = [vocab](int v) { return clamp_id(v, vocab); };
        const int cid = clampid(ids[row]);
        bool dup = false;
        for (int j0 = 0; j0 < row && !dup; j0 += 64) {
            int j = j0 + lane;
            bool hit = (j < row) && (clampid(ids[j]) == cid);
            dup = __any(hit);
        }
        if (dup) continue;  // wave-uniform
        float* dst = gword + (long)cid * H;
        for (int c0 = 0; c0 < H; c0 += 64 * 4) {  // 256-feature slabs held in registers
            int col = c0 + lane * 4;
            float a[4] = {0.f, 0.f, 0.f, 0.f};
            for (int j0 = row; j0 < rows; j0 += 64) {
                int j = j0 + lane;
                unsigned long long m = __ballot((j < rows) && (clampid(ids[j]) == cid));
                while (m) {
                    int b = __ffsll((long long)m) - 1;
                    m &= m - 1;
                    if (col < H) {
                        float v[4];
                        load4<float>(de + (long)(j0 + b) * H + col, v);
#pragma unroll
                        for (int e = 0; e < 4; ++e) a[e] += v[e];
                    }
                }
            }
            if (col < H) {
                float o[4];
                load4<float>(dst + col, o);
#pragma unroll
                for (int e = 0; e < 4; ++e) o[e] += a[e];
                store4<float>(dst + col, o);
            }
        }
    }
}

// position-table gradient: gpos[s] (+)= sum_b de[b, s]  (fixed b order)
__global__ __launch_bounds__(256) void embed_pos_grad_kernel(const float* __restrict__ de, float* __restrict__ gpos,
                                                             int B, int S, int H, int accumulate) {
    long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (long)S * H) return;
    float s = 0.f;
    for (int b = 0; b < B; ++b) s += de[(long)b * S * H + idx];
    gpos[idx] = accumulate ? gpos[idx] + s : s;
}

}  // namespace

extern "C" size_t polus_embed_bwd_workspace_bytes(int B, int S, int H) {
    size_t rows = (size_t)B * S;
    size_t de = rows * H * sizeof(float);
    size_t part = polus_layernorm_bwd_workspace_bytes((int)rows, H);
    size_t cs = polus_colsum_workspace_bytes((int)rows, H);
    return de + (part > cs ? part : cs) + 256;
}

extern "C" int polus_embed_ln_fwd(int dtype, const int32_t* ids, const int32_t* type_ids,
                                  const float* word, const float* pos, const float* type,
                                  const float* gamma, const float* beta, void* y, float* mean, float* rstd,
                                  int B, int S, int H, int vocab, int max_pos, int type_vocab, float eps,
                                  float drop_p, uint32_t seed, void* stream) {
    POLUS_REQUIRE(ids && word && pos && type && gamma && beta && y && mean && rstd, "polus_embed_ln_fwd: null pointer");
    POLUS_REQUIRE(rowwise_drop_ok(drop_p, (long)B * S, H), "polus_embed_ln_fwd: bad drop_p");
    POLUS_REQUIRE(B > 0 && S > 0 && S <= max_pos, "polus_embed_ln_fwd: S=%d exceeds max_position_embeddings=%d", S, max_pos);
    POLUS_REQUIRE(rowwise_shape_ok((long)B * S, H) && vocab > 0 && type_vocab > 0, "polus_embed_ln_fwd: bad H=%d", H);
    POLUS_REQUIRE(polus_aligned16(word) && polus_aligned16(pos) && polus_aligned16(type) && polus_aligned16(y) &&
                  polus_aligned16(gamma) && polus_aligned16(beta), "polus_embed_ln_fwd: pointers must be 16-byte aligned");
    hipStream_t st = static_cast<hipStream_t>(stream);
    const DropArgs d = drop_args(drop_p, seed);
    const dim3 grid(row_blocks(B * S));
    POLUS_REQUIRE(dtype == POLUS_BF16 || dtype == POLUS_F32, "polus_embed_ln_fwd: bad dtype");
    for_dtype_chunks<1, 2, 3, 4, 8>(dtype, chunks256(H), [&](auto t, auto nc) {
        using T = decltype(t);
        hipLaunchKernelGGL((embed_fwd_kernel<T, nc()>), grid, dim3(LN_THREADS), 0, st, ids, type_ids, word, pos, type, gamma, beta, (T*)y, mean, rstd, B, S, H, vocab, type_vocab, eps, d.thresh, d.seed, d.inv, d.dyn);
    });
    POLUS_CHECK_LAUNCH("polus_embed_ln_fwd");
    return POLUS_OK;
}

extern "C" int polus_embed_ln_bwd(int dtype, const void* dy, const int32_t* ids, const int32_t* type_ids,
                                  const float* word, const float* pos, const float* type, const float* gamma,
                                  const float* mean, const float* rstd,
                                  float* gword, float* gpos, float* gtype, float* ggamma, float* gbeta,
                                  int accumulate, int deterministic,
                                  int B, int S, int H, int vocab, int max_pos, int type_vocab,
                                  float drop_p, uint32_t seed,
                                  void* workspace, size_t workspace_bytes, void* stream) {
    POLUS_REQUIRE(dy && ids && word && pos && type && gamma && mean && rstd && gword && gpos && gtype && ggamma && gbeta,
                  "polus_embed_ln_bwd: null pointer");
    POLUS_REQUIRE(rowwise_drop_ok(drop_p, (long)B * S, H), "polus_embed_ln_bwd: bad drop_p");
    POLUS_REQUIRE(B > 0 && S > 0 && S <= max_pos && rowwise_shape_ok((long)B * S, H), "polus_embed_ln_bwd: bad shape");
    POLUS_REQUIRE(polus_aligned16(dy) && polus_aligned16(gword) && polus_aligned16(workspace),
                  "polus_embed_ln_bwd: pointers must be 16-byte aligned");
    size_t need = polus_embed_bwd_workspace_bytes(B, S, H);
    if (!workspace || workspace_bytes < need) { polus_set_error("polus_embed_ln_bwd: workspace %zu < %zu", workspace_bytes, need); return POLUS_ERR_WORKSPACE; }
    hipStream_t st = static_cast<hipStream_t>(stream);
    const DropArgs in_drop = drop_args(drop_p, seed);
    const int rows = B * S;
    float* de = static_cast<float*>(workspace);
    size_t de_bytes = ((size_t)rows * H * sizeof(float) + 255) / 256 * 256;
    float* partial = reinterpret_cast<float*>(static_cast<unsigned char*>(workspace) + de_bytes);
    size_t partial_bytes = workspace_bytes - de_bytes;
    const int blocks = ln_blocks(rows);
    const size_t lds = 3 * (size_t)H * sizeof(float);
    POLUS_REQUIRE(dtype == POLUS_BF16 || dtype == POLUS_F32, "polus_embed_ln_bwd: bad dtype");
    for_dtype_chunks<1, 2, 3, 4, 8>(dtype, chunks256(H), [&](auto t, auto nc) {
        using T = decltype(t);
        hipLaunchKernelGGL((embed_bwd_ln_kernel<T, nc()>), dim3(blocks), dim3(LN_THREADS), lds, st, (const T*)dy, ids, type_ids, word, pos, type, gamma, mean, rstd, de, partial, B, S, H, vocab, type_vocab, in_drop);
    });
    POLUS_CHECK_LAUNCH("polus_embed_ln_bwd(ln)");
    // one stage whatever POLUS_LN_FIN_SINGLE says: at most MAX_PARTIAL_BLOCKS partials
    int rc = polus_ln_finalize(partial, blocks, H, 0, ggamma, gbeta, nullptr, accumulate, 1, st, "polus_embed_ln_bwd(finalize)");
    if (rc != POLUS_OK) return rc;

    if (!accumulate) {
        POLUS_HIP(hipMemsetAsync(gword, 0, (size_t)vocab * H * sizeof(float), st));
        POLUS_HIP(hipMemsetAsync(gpos, 0, (size_t)max_pos * H * sizeof(float), st));
    }
    const int route = scatter_route(H, deterministic);
    if (route == SCATTER_OWNER)
        hipLaunchKernelGGL(embed_scatter_owner_kernel, dim3(row_blocks(rows)), dim3(LN_THREADS), 0, st, de, ids, gword, rows, H, vocab);
    else if (route == SCATTER_WIDE)
        hipLaunchKernelGGL(embed_scatter_atomic_wide_kernel, dim3(row_blocks(rows)), dim3(LN_THREADS), 0, st, de, ids, gword, rows, H, vocab);
    else
        for_chunks<1, 2, 3, 4>(route, [&](auto nc) {
            hipLaunchKernelGGL(embed_scatter_atomic_kernel<nc()>, dim3(capped_blocks(rows, SC_RUN * SC_WAVES, ROW_GRID_CAP)), dim3(64 * SC_WAVES), 0, st, de, ids, gword, rows, H, vocab);
        });
    POLUS_CHECK_LAUNCH("polus_embed_ln_bwd(scatter)");
    hipLaunchKernelGGL(embed_pos_grad_kernel, dim3(((long)S * H + 255) / 256), dim3(256), 0, st, de, gpos, B, S, H, accumulate);
    POLUS_CHECK_LAUNCH("polus_embed_ln_bwd(pos)");
    for (int t = 0; t < type_vocab; ++t) {   // without type_ids every token is type 0
        if (type_ids || t == 0) {
            rc = polus_colsum_launch(POLUS_F32, de, H, rows, H, gtype + (long)t * H, accumulate, type_ids, t, partial, partial_bytes, st);
            if (rc != POLUS_OK) return rc;
        } else if (!accumulate) {
            POLUS_HIP(hipMemsetAsync(gtype + (long)t * H, 0, (size_t)H * sizeof(float), st));
        }
    }
    return POLUS_OK;
}
