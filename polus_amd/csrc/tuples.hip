// Tuple scoring for retrieval distillation: every query is scored against its OWN n documents only, forward and
// backward, for token vectors (MaxSim) and single vectors (dot), and the two distillation losses over the resulting
// [B, n] score matrix (KL divergence to a teacher's distribution, MarginMSE to a teacher's margins).
//
//   document (b, j) of N = B n documents in one buffer sits at row  j B + b  (layout 0, slot-major: what the retrieval
//   trainers build, positives first, then negative block i)  or  b n + j  (layout 1, query-major).
//
// MaxSim forward: rerank.hip's body -- one wave per (query, document), the query's 16-token tiles as MFMA B fragments
// in registers, the document streamed from global memory straight into A fragments, no LDS, no barrier -- with
// maxsim_fwd_body's running (value, j) pick beside it.  The fragments, the MFMAs in ascending k, the strict > per lane
// over ascending document rows, the (value, lowest j) pick across the four row groups, the xor-shuffle sum of a tile's
// 16 maxima and the ascending tile sum are those of maxsim_fwd_body, so score and argmax are bit for bit what
// polus_maxsim_fwd writes for the pair.  A document of an odd number of tiles takes its last tile twice (two register
// buffers in turn, as in rerank.hip): under a strict > the second visit changes nothing.
// MaxSim backward (no atomics, no workspace, fixed summation orders):
//   dQ: one wave per query token, its n documents in ascending j;
//   dD: one wave per 16 document tokens of one document; the wave holds the query's Lq argmax values in registers
//       (one per lane and 64-token block) and finds a token's contributors, in ascending i, by ballot.
// Dot tuples: one wave per pair; 16-byte chunk c of a row belongs to lane c % 64 whatever the access width.
// Losses: one wave per row, per-row results combined in index order by a second single-block kernel.
#include <initializer_list>

#include "maxsim_common.h"

namespace {

__device__ __forceinline__ long tp_doc(int b, int j, int B, int n, int layout) {
    return layout ? (long)b * n + j : (long)j * B + b;
}

// rr_tile_max with the winning row: ascending rows per lane, a strict > keeps the lowest j of equal values
template <typename T, int KS, int UT>
__device__ __forceinline__ void tp_tile_pick(float (&m)[UT], int (&jb)[UT], const Frag<T> (&df)[KS],
                                             const Frag<T> (&qf)[UT][KS], unsigned bits, int r0, int nu) {
#pragma unroll
    for (int u = 0; u < UT; ++u) {
        if (u < nu) {                                         // uniform
            f32x4 acc = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) mma16(acc, df[ks], qf[u][ks]);
#pragma unroll
            for (int r = 0; r < 4; ++r)
                if (((bits >> r) & 1u) && acc[r] > m[u]) { m[u] = acc[r]; jb[u] = r0 + r; }
        }
    }
}

template <typename T, int KS, bool RES>
__global__ __launch_bounds__(256) void maxsim_tuples_fwd_kernel(const T* __restrict__ Q, const T* __restrict__ D,
                                                                const int32_t* __restrict__ qmask,
                                                                const int32_t* __restrict__ dmask,
                                                                float* __restrict__ score, long lds,
                                                                int32_t* __restrict__ argmax, int B, int n, int layout,
                                                                int Lq, int Ld) {
    constexpr int UT = MsTiles<T, KS>::UT;
    constexpr int E = 32 * KS;
    constexpr size_t ROWB = E * sizeof(T);
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int i = lane & 15, g = lane >> 4;
    const int b = blockIdx.y;
    const int j = blockIdx.x * 4 + wave;                      // this wave's document of query b
    if (j >= n) return;                                       // wave-uniform; the kernel has no barrier
    const long row = tp_doc(b, j, B, n, layout);
    const int nut = (Lq + 15) >> 4;                           // query tiles
    const T* Qb = Q + (size_t)b * Lq * E;
    const int32_t* qm = qmask ? qmask + (size_t)b * Lq : nullptr;
    const unsigned char* Dc = reinterpret_cast<const unsigned char*>(D) + (size_t)row * Ld * ROWB + 8 * g * sizeof(T);
    int32_t* am = argmax + ((size_t)b * n + j) * Lq;

    unsigned tm;
    int nvt;
    {
        int mv[8];
        rr_mask_load(mv, dmask ? dmask + (size_t)row * Ld : nullptr, lane, Ld);
        rr_mask_pack(mv, true, lane, Ld, tm, nvt);
    }
    if (nvt == 0) {                                           // empty document: 0.0 and no winner anywhere
        for (int t = lane; t < Lq; t += 64) am[t] = -1;
        if (lane == 0) score[(size_t)b * lds + j] = 0.f;
        return;
    }
    // two tile buffers used in turn, two tiles per trip (rerank.hip): at the top of a round ta = tile 0
    Frag<T> ta[KS], tb[KS];
    rr_tile_load<T, KS>(ta, Dc, 0, i, Ld);
    Frag<T> qf[UT][KS];
    bool qok[UT];
    if constexpr (RES) rr_query_load<T, KS, UT>(qf, qok, Qb, qm, 0, nut, Lq, i, g);

    float s = 0.f;
    for (int r0 = 0; r0 < nut; r0 += UT) {
        if constexpr (!RES) rr_query_load<T, KS, UT>(qf, qok, Qb, qm, r0, nut, Lq, i, g);
        const int nu = min(UT, nut - r0);
        float m[UT];
        int jb[UT];
#pragma unroll
        for (int u = 0; u < UT; ++u) { m[u] = -INFINITY; jb[u] = MS_NOJ; }
        for (int t = 0; t < nvt; t += 2) {
            const int t1 = min(t + 1, nvt - 1);
            const bool last = t + 2 >= nvt;
            rr_tile_load<T, KS>(tb, Dc, t1, i, Ld);
            tp_tile_pick<T, KS, UT>(m, jb, ta, qf, __builtin_amdgcn_readlane(tm, t) >> (4 * g), 16 * t + 4 * g, nu);
            rr_tile_load<T, KS>(ta, Dc, last ? 0 : t + 2, i, Ld);   // the next round starts at tile 0 again
            tp_tile_pick<T, KS, UT>(m, jb, tb, qf, __builtin_amdgcn_readlane(tm, t1) >> (4 * g), 16 * t1 + 4 * g, nu);
        }
#pragma unroll
        for (int u = 0; u < UT; ++u) {
            if (u < nu) {                                     // uniform
                float mu = m[u];
                int ju = jb[u];
#pragma unroll
                for (int o = 16; o <= 32; o <<= 1) {
                    const float m2 = __shfl_xor(mu, o, 64);
                    const int j2 = __shfl_xor(ju, o, 64);
                    if (m2 > mu || (m2 == mu && j2 < ju)) { mu = m2; ju = j2; }
                }
                const int tok = 16 * (r0 + u) + i;
                const bool hit = qok[u] && ju != MS_NOJ;
                if (g == 0 && tok < Lq) am[tok] = hit ? ju : -1;
                float contrib = hit ? mu : 0.f;
#pragma unroll
                for (int o = 1; o < 16; o <<= 1) contrib += __shfl_xor(contrib, o, 64);
                s += contrib;
            }
        }
    }
    if (lane == 0) score[(size_t)b * lds + j] = s;
}

// dQ[b, i, :] = sum over j ascending of dscore[b, j] * D[doc(b, j), argmax[b, j, i], :]; one wave per query token
// (maxsim_bwd_dq_kernel over the query's own n documents)
template <typename T>
__global__ __launch_bounds__(256) void maxsim_tuples_dq_kernel(const T* __restrict__ D, const float* __restrict__ dscore,
                                                               long lds, const int32_t* __restrict__ argmax,
                                                               T* __restrict__ dQ, int B, int n, int layout, int Lq,
                                                               int Ld, int E) {
    const int lane = threadIdx.x & 63;
    const int i = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int b = blockIdx.y;
    if (i >= Lq) return;
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
    for (int c0 = 0; c0 < n; c0 += 64) {
        const int cl = c0 + lane;
        const int jv = cl < n ? argmax[((size_t)b * n + cl) * Lq + i] : -1;
        const float dv = cl < n ? dscore[(size_t)b * lds + cl] : 0.f;
        const int nn = min(64, n - c0);
        for (int l0 = 0; l0 < nn; l0 += 8) {
            float x[8][4];
            int js[8];
#pragma unroll
            for (int q = 0; q < 8; ++q) {
                const int l = min(l0 + q, nn - 1);
                js[q] = __builtin_amdgcn_readlane(jv, l);
                const T* dr = D + ((size_t)tp_doc(b, c0 + l, B, n, layout) * Ld + min(max(js[q], 0), Ld - 1)) * E;
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const int e = lane + 64 * k;
                    x[q][k] = e < E ? to_f<T>(dr[e]) : 0.f;
                }
            }
#pragma unroll
            for (int q = 0; q < 8; ++q) {
                if (l0 + q < nn && js[q] >= 0 && js[q] < Ld) {
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
        if (e < E) dQ[((size_t)b * Lq + i) * E + e] = from_f<T>(acc[k]);
    }
}

// dD[doc(b, j), t, :] = sum over i ascending with argmax[b, j, i] == t of dscore[b, j] * Q[b, i, :].  One query's Lq
// argmax values decide the document's whole gradient: a wave keeps them in registers (token 64 k + lane in key[k])
// and owns 16 document tokens; rows without a contributor are written as zeros.
constexpr int DD_ROWS = 64;             // document tokens per workgroup (4 waves x 16)

template <typename T>
__global__ __launch_bounds__(256) void maxsim_tuples_dd_kernel(const T* __restrict__ Q, const float* __restrict__ dscore,
                                                               long lds, const int32_t* __restrict__ argmax,
                                                               T* __restrict__ dD, int B, int n, int layout, int Lq,
                                                               int Ld, int E) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int j = blockIdx.x, b = blockIdx.y;
    const int t0 = blockIdx.z * DD_ROWS + wave * 16;
    if (t0 >= Ld) return;
    const int t1 = min(t0 + 16, Ld);
    const int32_t* am = argmax + ((size_t)b * n + j) * Lq;
    int key[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) key[k] = 64 * k + lane < Lq ? am[64 * k + lane] : -1;
    const float ds = dscore[(size_t)b * lds + j];
    const T* Qb = Q + (size_t)b * Lq * E;
    T* out = dD + (size_t)tp_doc(b, j, B, n, layout) * Ld * E;
    const int nk = (Lq + 63) >> 6;
    for (int t = t0; t < t1; ++t) {
        float acc[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            if (k < nk) {                                     // uniform
                unsigned long long hit = __ballot(key[k] == t);
                while (hit) {                                 // ascending i
                    const int iq = 64 * k + (int)__builtin_ctzll(hit);
                    hit &= hit - 1;
                    const T* qr = Qb + (size_t)iq * E;
#pragma unroll
                    for (int c = 0; c < 4; ++c) {
                        const int e = lane + 64 * c;
                        acc[c] = fmaf(ds, e < E ? to_f<T>(qr[e]) : 0.f, acc[c]);
                    }
                }
            }
        }
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const int e = lane + 64 * c;
            if (e < E) out[(size_t)t * E + e] = from_f<T>(acc[c]);
        }
    }
}

// ---------------------------------------------------------------- dot tuples
// A row of W elements is cut into chunks of V = 16 / sizeof(T) elements; chunk c belongs to lane c % 64 (forward) or to
// thread c of the grid (backward).  VEC: whole chunks move as one 16-byte access; the arithmetic does not depend on it.
template <typename T> struct TpVec { static constexpr int V = 16 / (int)sizeof(T); };

template <typename T, bool VEC>
__device__ __forceinline__ void tp_load(const T* p, long w0, int W, float (&v)[TpVec<T>::V]) {
    constexpr int V = TpVec<T>::V;
    if (VEC && w0 + V <= W) {
        if constexpr (sizeof(T) == 4) {
            const float4 t = *reinterpret_cast<const float4*>(p + w0);
            v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
        } else {
            const bf16x8 t = *reinterpret_cast<const bf16x8*>(p + w0);
#pragma unroll
            for (int k = 0; k < V; ++k) v[k] = (float)t[k];
        }
    } else {
#pragma unroll
        for (int k = 0; k < V; ++k) v[k] = w0 + k < W ? to_f<T>(p[w0 + k]) : 0.f;
    }
}

template <typename T, bool VEC>
__device__ __forceinline__ void tp_store(T* p, long w0, int W, const float (&v)[TpVec<T>::V]) {
    constexpr int V = TpVec<T>::V;
    if (VEC && w0 + V <= W) {
        if constexpr (sizeof(T) == 4) {
            *reinterpret_cast<float4*>(p + w0) = make_float4(v[0], v[1], v[2], v[3]);
        } else {
            bf16x8 t;
#pragma unroll
            for (int k = 0; k < V; ++k) t[k] = (bf16_t)v[k];
            *reinterpret_cast<bf16x8*>(p + w0) = t;
        }
    } else {
#pragma unroll
        for (int k = 0; k < V; ++k)
            if (w0 + k < W) p[w0 + k] = from_f<T>(v[k]);
    }
}

// score[b, j] = sum_w q[b, w] d[doc(b, j), w]: lane l adds its chunks l, l + 64, ... element by element in ascending w
// (one fmaf chain from +0), the 64 lane sums meet in the xor-shuffle tree 32, 16, .., 1
template <typename T, bool VEC>
__global__ __launch_bounds__(256) void dot_tuples_fwd_kernel(const T* __restrict__ q, long ldq, const T* __restrict__ d,
                                                             long ldd, float* __restrict__ score, long lds, int B, int n,
                                                             int layout, int W) {
    constexpr int V = TpVec<T>::V;
    const int lane = threadIdx.x & 63;
    const int j = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int b = blockIdx.y;
    if (j >= n) return;
    const T* qr = q + (size_t)b * ldq;
    const T* dr = d + (size_t)tp_doc(b, j, B, n, layout) * ldd;
    float acc = 0.f;
    for (long w0 = (long)lane * V; w0 < W; w0 += 64 * V) {
        float a[V], x[V];
        tp_load<T, VEC>(qr, w0, W, a);
        tp_load<T, VEC>(dr, w0, W, x);
#pragma unroll
        for (int k = 0; k < V; ++k) acc = fmaf(a[k], x[k], acc);   // elements past W are 0 * 0
    }
    acc = wave_sum(acc);
    if (lane == 0) score[(size_t)b * lds + j] = acc;
}

// dq[b, w] = sum over j ascending of dscore[b, j] * d[doc(b, j), w] (fmaf chain from +0); one thread per chunk
template <typename T, bool VEC>
__global__ __launch_bounds__(256) void dot_tuples_dq_kernel(const T* __restrict__ d, long ldd,
                                                            const float* __restrict__ dscore, long lds,
                                                            T* __restrict__ dq, long lddq, int B, int n, int layout,
                                                            int W) {
    constexpr int V = TpVec<T>::V;
    const long w0 = ((long)blockIdx.x * 256 + threadIdx.x) * V;
    const int b = blockIdx.y;
    if (w0 >= W) return;
    float acc[V];
#pragma unroll
    for (int k = 0; k < V; ++k) acc[k] = 0.f;
    for (int j = 0; j < n; ++j) {
        const float ds = dscore[(size_t)b * lds + j];
        float x[V];
        tp_load<T, VEC>(d + (size_t)tp_doc(b, j, B, n, layout) * ldd, w0, W, x);
#pragma unroll
        for (int k = 0; k < V; ++k) acc[k] = fmaf(ds, x[k], acc[k]);
    }
    tp_store<T, VEC>(dq + (size_t)b * lddq, w0, W, acc);
}

// dd[doc(b, j), w] = dscore[b, j] * q[b, w]
template <typename T, bool VEC>
__global__ __launch_bounds__(256) void dot_tuples_dd_kernel(const T* __restrict__ q, long ldq,
                                                            const float* __restrict__ dscore, long lds,
                                                            T* __restrict__ dd, long lddd, int B, int n, int layout,
                                                            int W) {
    constexpr int V = TpVec<T>::V;
    const long w0 = ((long)blockIdx.x * 256 + threadIdx.x) * V;
    const int j = blockIdx.y, b = blockIdx.z;
    if (w0 >= W) return;
    const float ds = dscore[(size_t)b * lds + j];
    float x[V];
    tp_load<T, VEC>(q + (size_t)b * ldq, w0, W, x);
#pragma unroll
    for (int k = 0; k < V; ++k) x[k] = ds * x[k];
    tp_store<T, VEC>(dd + (size_t)tp_doc(b, j, B, n, layout) * lddd, w0, W, x);
}

// ---------------------------------------------------------------- distillation losses
// One wave per row; lane l takes columns l, l + 64, ... in ascending order, lane sums meet in wave_sum.  A column is
// present where its teacher score is not -inf; an absent column's student score is never used.
constexpr int DL_MAXN = 1024;

__device__ __forceinline__ bool dl_present(float t) { return t != -INFINITY; }

// KL(softmax(teacher) || softmax(student)) of one row -> partial[row]; dstudent = (softmax(student) - p) / rows
__global__ __launch_bounds__(256) void distill_kl_kernel(const float* __restrict__ student, long lds,
                                                         const float* __restrict__ teacher, long ldt,
                                                         float* __restrict__ partial, float* __restrict__ dstudent,
                                                         long ldd, int rows, int n) {
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    const float* s = student + (size_t)row * lds;
    const float* t = teacher + (size_t)row * ldt;
    float* g = dstudent + (size_t)row * ldd;
    float tmax = -INFINITY, smax = -INFINITY;
    for (int c = lane; c < n; c += 64) {
        const float tv = t[c];
        if (dl_present(tv)) { tmax = fmaxf(tmax, tv); smax = fmaxf(smax, s[c]); }
    }
    tmax = wave_max(tmax);
    smax = wave_max(smax);
    if (tmax == -INFINITY) {                                  // no present column (uniform)
        for (int c = lane; c < n; c += 64) g[c] = 0.f;
        if (lane == 0) partial[row] = 0.f;
        return;
    }
    float zt = 0.f, zs = 0.f;
    for (int c = lane; c < n; c += 64) {
        const float tv = t[c];
        if (dl_present(tv)) { zt += expf(tv - tmax); zs += expf(s[c] - smax); }
    }
    const float lzt = logf(wave_sum(zt)), lzs = logf(wave_sum(zs));
    const float inv = 1.0f / (float)rows;
    float loss = 0.f;
    for (int c = lane; c < n; c += 64) {
        const float tv = t[c];
        float gv = 0.f;
        if (dl_present(tv)) {
            const float lp = (tv - tmax) - lzt, ls = (s[c] - smax) - lzs;
            const float p = expf(lp);
            loss += p * (lp - ls);
            gv = (expf(ls) - p) * inv;
        }
        g[c] = gv;
    }
    loss = wave_sum(loss);
    if (lane == 0) partial[row] = loss;
}

// cnt[row] = present negatives of the row (0 when column 0 is absent)
__global__ __launch_bounds__(256) void margin_mse_count_kernel(const float* __restrict__ teacher, long ldt,
                                                               int32_t* __restrict__ cnt, int rows, int n) {
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    const float* t = teacher + (size_t)row * ldt;
    int m = 0;
    for (int c = lane; c < n; c += 64) m += (c >= 1 && dl_present(t[c])) ? 1 : 0;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) m += __shfl_xor(m, o, 64);
    if (lane == 0) cnt[row] = dl_present(t[0]) ? m : 0;
}

// integer total of cnt[0 .. rows): exact in any order
__device__ __forceinline__ int dl_total(const int32_t* cnt, int rows, int lane) {
    int m = 0;
    for (int r = lane; r < rows; r += 64) m += cnt[r];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) m += __shfl_xor(m, o, 64);
    return m;
}

// row sum of ((s_0 - s_j) - (t_0 - t_j))^2 over the present negatives -> partial[row]; dstudent = the gradient of
// the sum over all rows divided by max(M, 1)
__global__ __launch_bounds__(256) void margin_mse_kernel(const float* __restrict__ student, long lds,
                                                         const float* __restrict__ teacher, long ldt,
                                                         const int32_t* __restrict__ cnt, float* __restrict__ partial,
                                                         float* __restrict__ dstudent, long ldd, int rows, int n) {
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    const float* s = student + (size_t)row * lds;
    const float* t = teacher + (size_t)row * ldt;
    float* g = dstudent + (size_t)row * ldd;
    const int M = dl_total(cnt, rows, lane);
    const float t0 = t[0];
    if (!dl_present(t0)) {                                    // uniform: the row has no positive
        for (int c = lane; c < n; c += 64) g[c] = 0.f;
        if (lane == 0) partial[row] = 0.f;
        return;
    }
    const float s0 = s[0];
    const float inv2 = 2.0f / (float)max(M, 1);
    float loss = 0.f, esum = 0.f;
    for (int c = lane; c < n; c += 64) {
        const float tv = t[c];
        float gv = 0.f;
        if (c >= 1 && dl_present(tv)) {
            const float e = (s0 - s[c]) - (t0 - tv);
            loss = fmaf(e, e, loss);
            esum += e;
            gv = -e * inv2;
        }
        if (c >= 1) g[c] = gv;
    }
    loss = wave_sum(loss);
    esum = wave_sum(esum);
    if (lane == 0) { partial[row] = loss; g[0] = esum * inv2; }
}

// loss = (partial[0] + partial[1] + ..., loss.hip's finalize_sum_kernel order) * (cnt ? 1 / max(sum cnt, 1) : mul)
__global__ __launch_bounds__(256) void distill_finalize_kernel(const float* __restrict__ partial,
                                                               const int32_t* __restrict__ cnt, int rows, float mul,
                                                               float* __restrict__ out) {
    __shared__ float red[256];
    __shared__ int redc[256];
    float s = 0.f;
    int m = 0;
    for (int k = threadIdx.x; k < rows; k += 256) { s += partial[k]; if (cnt) m += cnt[k]; }
    red[threadIdx.x] = s;
    redc[threadIdx.x] = m;
    __syncthreads();
    if (threadIdx.x == 0) {
        float t = 0.f;
        int M = 0;
        for (int k = 0; k < 256; ++k) { t += red[k]; M += redc[k]; }
        *out = t * (cnt ? 1.0f / (float)max(M, 1) : mul);
    }
}

// ---------------------------------------------------------------- host
int tp_check(const char* what, int dtype, int B, int n, int layout, int Lq, int Ld, int E, long lds) {
    int rc = ms_shape_check(what, dtype, B, Lq, Ld, E);
    if (rc != POLUS_OK) return rc;
    POLUS_REQUIRE(n >= 1 && n <= 65535, "%s: need 1 <= n <= 65535 (got %d)", what, n);
    POLUS_REQUIRE((long long)B * n <= 0x7fffffffLL, "%s: B*n must be <= 2^31 - 1 (got %lld)", what, (long long)B * n);
    POLUS_REQUIRE((long long)B * n * Lq < (1LL << 31), "%s: B*n*Lq must be < 2^31 (got %lld)", what,
                  (long long)B * n * Lq);
    POLUS_REQUIRE(lds >= n, "%s: score row stride lds must be >= n (got %ld < %d)", what, lds, n);
    POLUS_REQUIRE(layout == 0 || layout == 1, "%s: layout must be 0 (slot-major) or 1 (query-major) (got %d)", what,
                  layout);
    return POLUS_OK;
}

template <typename T>
void tp_bwd_launch(const void* Q, const void* D, const float* ds, long lds, const int32_t* am, void* dQ, void* dD, int B,
                   int n, int layout, int Lq, int Ld, int E, hipStream_t st) {
    hipLaunchKernelGGL(maxsim_tuples_dq_kernel<T>, dim3((unsigned)((Lq + 3) / 4), (unsigned)B), dim3(256), 0, st,
                       static_cast<const T*>(D), ds, lds, am, static_cast<T*>(dQ), B, n, layout, Lq, Ld, E);
    hipLaunchKernelGGL(maxsim_tuples_dd_kernel<T>, dim3((unsigned)n, (unsigned)B, (unsigned)((Ld + DD_ROWS - 1) / DD_ROWS)),
                       dim3(256), 0, st, static_cast<const T*>(Q), ds, lds, am, static_cast<T*>(dD), B, n, layout, Lq,
                       Ld, E);
}

int dot_check(const char* what, int dtype, int B, int n, int layout, int W, long lds) {
    POLUS_REQUIRE(dtype == POLUS_F32 || dtype == POLUS_BF16, "%s: unknown dtype %d", what, dtype);
    POLUS_REQUIRE(W >= 1, "%s: need W >= 1 (got %d)", what, W);
    POLUS_REQUIRE(B >= 1 && B <= 65535, "%s: need 1 <= B <= 65535 (got %d)", what, B);
    POLUS_REQUIRE(n >= 1 && n <= 65535, "%s: need 1 <= n <= 65535 (got %d)", what, n);
    POLUS_REQUIRE((long long)B * n <= 0x7fffffffLL, "%s: B*n must be <= 2^31 - 1 (got %lld)", what, (long long)B * n);
    POLUS_REQUIRE(lds >= n, "%s: score row stride lds must be >= n (got %ld < %d)", what, lds, n);
    POLUS_REQUIRE(layout == 0 || layout == 1, "%s: layout must be 0 (slot-major) or 1 (query-major) (got %d)", what,
                  layout);
    return POLUS_OK;
}

// 16-byte accesses need every base and every row stride in bytes to be a multiple of 16
static bool tp_vec_ok(size_t esz, std::initializer_list<const void*> ptrs, std::initializer_list<long> strides) {
    for (const void* p : ptrs) if (!polus_aligned16(p)) return false;
    for (long s : strides) if (((size_t)s * esz) % 16 != 0) return false;
    return true;
}

template <typename T>
void dot_fwd_launch(bool vec, const void* q, long ldq, const void* d, long ldd, float* score, long lds, int B, int n,
                    int layout, int W, hipStream_t st) {
    dim3 grid((unsigned)((n + 3) / 4), (unsigned)B);
    if (vec)
        hipLaunchKernelGGL((dot_tuples_fwd_kernel<T, true>), grid, dim3(256), 0, st, static_cast<const T*>(q), ldq,
                           static_cast<const T*>(d), ldd, score, lds, B, n, layout, W);
    else
        hipLaunchKernelGGL((dot_tuples_fwd_kernel<T, false>), grid, dim3(256), 0, st, static_cast<const T*>(q), ldq,
                           static_cast<const T*>(d), ldd, score, lds, B, n, layout, W);
}

template <typename T>
void dot_bwd_launch(bool vec, const void* q, long ldq, const void* d, long ldd, const float* ds, long lds, void* dq,
                    long lddq, void* dd, long lddd, int B, int n, int layout, int W, hipStream_t st) {
    constexpr int V = TpVec<T>::V;
    const unsigned gx = (unsigned)(((long)W + 256L * V - 1) / (256L * V));
    if (vec) {
        hipLaunchKernelGGL((dot_tuples_dq_kernel<T, true>), dim3(gx, (unsigned)B), dim3(256), 0, st,
                           static_cast<const T*>(d), ldd, ds, lds, static_cast<T*>(dq), lddq, B, n, layout, W);
        hipLaunchKernelGGL((dot_tuples_dd_kernel<T, true>), dim3(gx, (unsigned)n, (unsigned)B), dim3(256), 0, st,
                           static_cast<const T*>(q), ldq, ds, lds, static_cast<T*>(dd), lddd, B, n, layout, W);
    } else {
        hipLaunchKernelGGL((dot_tuples_dq_kernel<T, false>), dim3(gx, (unsigned)B), dim3(256), 0, st,
                           static_cast<const T*>(d), ldd, ds, lds, static_cast<T*>(dq), lddq, B, n, layout, W);
        hipLaunchKernelGGL((dot_tuples_dd_kernel<T, false>), dim3(gx, (unsigned)n, (unsigned)B), dim3(256), 0, st,
                           static_cast<const T*>(q), ldq, ds, lds, static_cast<T*>(dd), lddd, B, n, layout, W);
    }
}

int dl_check(const char* what, const float* student, long lds, const float* teacher, long ldt, float* loss,
             float* dstudent, long ldd, int rows, int n, void* workspace, size_t workspace_bytes) {
    POLUS_REQUIRE(rows >= 1, "%s: need rows >= 1 (got %d)", what, rows);
    POLUS_REQUIRE(n >= 1 && n <= DL_MAXN, "%s: need 1 <= n <= %d (got %d)", what, DL_MAXN, n);
    POLUS_REQUIRE(lds >= n && ldt >= n && ldd >= n, "%s: row strides must be >= n (got %ld, %ld, %ld < %d)", what, lds,
                  ldt, ldd, n);
    POLUS_REQUIRE(student && teacher && loss && dstudent, "%s: null pointer", what);
    if (!workspace || workspace_bytes < polus_distill_workspace_bytes(rows)) {
        polus_set_error("%s: workspace too small", what);
        return POLUS_ERR_WORKSPACE;
    }
    return POLUS_OK;
}

}  // namespace

extern "C" int polus_maxsim_tuples_fwd(int dtype, const void* Q, const void* D, const int32_t* qmask,
                                       const int32_t* dmask, float* score, long lds, int32_t* argmax, int B, int n,
                                       int layout, int Lq, int Ld, int E, void* stream) {
    const char* what = "polus_maxsim_tuples_fwd";
    int rc = tp_check(what, dtype, B, n, layout, Lq, Ld, E, lds);
    if (rc != POLUS_OK) return rc;
    POLUS_REQUIRE(Q && D && score && argmax, "%s: null pointer", what);
    POLUS_REQUIRE(polus_aligned16(Q) && polus_aligned16(D), "%s: Q and D must be 16-byte aligned", what);
    ms_dispatch(dtype, E, [&](auto t, auto ks) {
        using T = typename decltype(t)::type;
        constexpr int KS = decltype(ks)::value;
        const auto kern = ms_query_fits<T, KS>(Lq) ? maxsim_tuples_fwd_kernel<T, KS, true>
                                                   : maxsim_tuples_fwd_kernel<T, KS, false>;
        hipLaunchKernelGGL(kern, dim3((unsigned)((n + 3) / 4), (unsigned)B), dim3(256), 0,
                           static_cast<hipStream_t>(stream), static_cast<const T*>(Q), static_cast<const T*>(D), qmask,
                           dmask, score, lds, argmax, B, n, layout, Lq, Ld);
    });
    POLUS_CHECK_LAUNCH(what);
    return POLUS_OK;
}

extern "C" int polus_maxsim_tuples_bwd(int dtype, const void* Q, const void* D, const float* dscore, long lds,
                                       const int32_t* argmax, void* dQ, void* dD, int B, int n, int layout, int Lq,
                                       int Ld, int E, void* stream) {
    const char* what = "polus_maxsim_tuples_bwd";
    int rc = tp_check(what, dtype, B, n, layout, Lq, Ld, E, lds);
    if (rc != POLUS_OK) return rc;
    POLUS_REQUIRE(Q && D && dscore && argmax && dQ && dD, "%s: null pointer", what);
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (dtype == POLUS_BF16)
        tp_bwd_launch<bf16_t>(Q, D, dscore, lds, argmax, dQ, dD, B, n, layout, Lq, Ld, E, st);
    else
        tp_bwd_launch<float>(Q, D, dscore, lds, argmax, dQ, dD, B, n, layout, Lq, Ld, E, st);
    POLUS_CHECK_LAUNCH(what);
    return POLUS_OK;
}

extern "C" int polus_dot_tuples_fwd(int dtype, const void* q, long ldq, const void* d, long ldd, float* score, long lds,
                                    int B, int n, int layout, int W, void* stream) {
    const char* what = "polus_dot_tuples_fwd";
    int rc = dot_check(what, dtype, B, n, layout, W, lds);
    if (rc != POLUS_OK) return rc;
    POLUS_REQUIRE(ldq >= W && ldd >= W, "%s: row strides must be >= W (got %ld, %ld < %d)", what, ldq, ldd, W);
    POLUS_REQUIRE(q && d && score, "%s: null pointer", what);
    hipStream_t st = static_cast<hipStream_t>(stream);
    const bool vec = tp_vec_ok(polus_dtype_size(dtype), {q, d}, {ldq, ldd});
    if (dtype == POLUS_BF16)
        dot_fwd_launch<bf16_t>(vec, q, ldq, d, ldd, score, lds, B, n, layout, W, st);
    else
        dot_fwd_launch<float>(vec, q, ldq, d, ldd, score, lds, B, n, layout, W, st);
    POLUS_CHECK_LAUNCH(what);
    return POLUS_OK;
}

extern "C" int polus_dot_tuples_bwd(int dtype, const void* q, long ldq, const void* d, long ldd, const float* dscore,
                                    long lds, void* dq, long lddq, void* dd, long lddd, int B, int n, int layout, int W,
                                    void* stream) {
    const char* what = "polus_dot_tuples_bwd";
    int rc = dot_check(what, dtype, B, n, layout, W, lds);
    if (rc != POLUS_OK) return rc;
    POLUS_REQUIRE(ldq >= W && ldd >= W && lddq >= W && lddd >= W,
                  "%s: row strides must be >= W (got %ld, %ld, %ld, %ld < %d)", what, ldq, ldd, lddq, lddd, W);
    POLUS_REQUIRE(q && d && dscore && dq && dd, "%s: null pointer", what);
    hipStream_t st = static_cast<hipStream_t>(stream);
    const bool vec = tp_vec_ok(polus_dtype_size(dtype), {q, d, dq, dd}, {ldq, ldd, lddq, lddd});
    if (dtype == POLUS_BF16)
        dot_bwd_launch<bf16_t>(vec, q, ldq, d, ldd, dscore, lds, dq, lddq, dd, lddd, B, n, layout, W, st);
    else
        dot_bwd_launch<float>(vec, q, ldq, d, ldd, dscore, lds, dq, lddq, dd, lddd, B, n, layout, W, st);
    POLUS_CHECK_LAUNCH(what);
    return POLUS_OK;
}

// per-row loss (f32) and per-row count (int32)
extern "C" size_t polus_distill_workspace_bytes(int rows) { return (size_t)(rows > 0 ? rows : 0) * 8 + 16; }

extern "C" int polus_distill_kl(const float* student, long lds, const float* teacher, long ldt, float* loss,
                                float* dstudent, long ldd, int rows, int n, void* workspace, size_t workspace_bytes,
                                void* stream) {
    const char* what = "polus_distill_kl";
    int rc = dl_check(what, student, lds, teacher, ldt, loss, dstudent, ldd, rows, n, workspace, workspace_bytes);
    if (rc != POLUS_OK) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    float* partial = static_cast<float*>(workspace);
    hipLaunchKernelGGL(distill_kl_kernel, dim3((unsigned)(((long)rows + 3) / 4)), dim3(256), 0, st, student, lds, teacher,
                       ldt, partial, dstudent, ldd, rows, n);
    POLUS_CHECK_LAUNCH(what);
    hipLaunchKernelGGL(distill_finalize_kernel, dim3(1), dim3(256), 0, st, partial, (const int32_t*)nullptr, rows,
                       1.0f / (float)rows, loss);
    POLUS_CHECK_LAUNCH("polus_distill_kl(finalize)");
    return POLUS_OK;
}

extern "C" int polus_margin_mse(const float* student, long lds, const float* teacher, long ldt, float* loss,
                                float* dstudent, long ldd, int rows, int n, void* workspace, size_t workspace_bytes,
                                void* stream) {
    const char* what = "polus_margin_mse";
    int rc = dl_check(what, student, lds, teacher, ldt, loss, dstudent, ldd, rows, n, workspace, workspace_bytes);
    if (rc != POLUS_OK) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    float* partial = static_cast<float*>(workspace);
    int32_t* cnt = reinterpret_cast<int32_t*>(partial + rows);
    const dim3 grid((unsigned)(((long)rows + 3) / 4));
    hipLaunchKernelGGL(margin_mse_count_kernel, grid, dim3(256), 0, st, teacher, ldt, cnt, rows, n);
    POLUS_CHECK_LAUNCH("polus_margin_mse(count)");
    hipLaunchKernelGGL(margin_mse_kernel, grid, dim3(256), 0, st, student, lds, teacher, ldt, (const int32_t*)cnt,
                       partial, dstudent, ldd, rows, n);
    POLUS_CHECK_LAUNCH(what);
    hipLaunchKernelGGL(distill_finalize_kernel, dim3(1), dim3(256), 0, st, partial, (const int32_t*)cnt, rows, 1.0f,
                       loss);
    POLUS_CHECK_LAUNCH("polus_margin_mse(finalize)");
    return POLUS_OK;
}
