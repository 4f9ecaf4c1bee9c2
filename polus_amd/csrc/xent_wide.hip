// Masked-LM loss path (gfx950): softmax cross-entropy over rows of ANY width with ignored rows, and the row gather /
// scatter that picks the masked positions out of [B S, H] and puts their gradient back.
//
// polus_softmax_xent_wide: one workgroup of 1024 lanes per row (loss.hip gives one THREAD a row: right for a few
// dozen classes, a 120 KB stride between lanes at V = 30522).  Two paths, chosen on the host by the row's bytes:
//   staged     the row fits XW_STAGE_BYTES of LDS: one HBM read into LDS, max / sum / gradient from LDS, one HBM
//              write -- the compulsory traffic;
//   streaming  wider rows: online max / sum in one read, a second read for the gradient.
// Both move 16 bytes per lane where base and stride of logits AND dlogits allow, single elements where not; the LDS
// copy is always read in 16-byte chunks, so the staged path gives the same bits for both access widths.
// dlogits may be the logits buffer (same stride): a workgroup owns its row, the staged path has read all of it
// before the first write, the streaming path's second pass reads and writes an element in the same lane.
// No atomics: a first single-workgroup launch counts the labels (the gradient needs 1 / counted), the row kernel
// leaves one f32 per row, a last single-workgroup launch adds them in index order.  Bitwise reproducible.
#include "common.h"

namespace {

constexpr int XW_THREADS = 1024;
constexpr int XW_WAVES = XW_THREADS / 64;
constexpr int XW_STAGE_BYTES = 128 * 1024;   // of the 160 KiB a CU has: one workgroup per CU at V = 30522 f32, two in bf16

template <typename T> struct Chunk16 { static constexpr int E = 16 / (int)sizeof(T); };

template <typename T> __device__ __forceinline__ void unpack16(const uint4& q, float (&v)[Chunk16<T>::E]);
template <> __device__ __forceinline__ void unpack16<float>(const uint4& q, float (&v)[4]) {
    v[0] = __uint_as_float(q.x); v[1] = __uint_as_float(q.y); v[2] = __uint_as_float(q.z); v[3] = __uint_as_float(q.w);
}
template <> __device__ __forceinline__ void unpack16<bf16_t>(const uint4& q, float (&v)[8]) {
    const bf16x8 t = __builtin_bit_cast(bf16x8, q);
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = (float)t[j];
}
template <typename T> __device__ __forceinline__ uint4 pack16(const float (&v)[Chunk16<T>::E]);
template <> __device__ __forceinline__ uint4 pack16<float>(const float (&v)[4]) {
    return make_uint4(__float_as_uint(v[0]), __float_as_uint(v[1]), __float_as_uint(v[2]), __float_as_uint(v[3]));
}
template <> __device__ __forceinline__ uint4 pack16<bf16_t>(const float (&v)[8]) {
    bf16x8 t;
#pragma unroll
    for (int j = 0; j < 8; ++j) t[j] = (bf16_t)v[j];
    return __builtin_bit_cast(uint4, t);
}

// f(v, n, i0) over this lane's share of p[0..V): whole 16-byte chunks (n = E) plus the row's scalar tail (n = 1) when
// VEC, else single elements.  Lane `tid` of `nthr`.
template <typename T, bool VEC, typename F>
__device__ __forceinline__ void row_foreach(const T* p, int V, int tid, int nthr, F f) {
    constexpr int E = Chunk16<T>::E;
    float v[E];
    if (VEC) {
        const int nchunk = V / E;
        for (int c = tid; c < nchunk; c += nthr) {
            unpack16<T>(reinterpret_cast<const uint4*>(p)[c], v);
            f(v, E, c * E);
        }
        const int i = nchunk * E + tid;
        if (i < V) { v[0] = to_f<T>(p[i]); f(v, 1, i); }
    } else {
        for (int i = tid; i < V; i += nthr) { v[0] = to_f<T>(p[i]); f(v, 1, i); }
    }
}

// dst[i] = g(src[i], i) over this lane's share; the same split as row_foreach.  src may be dst (element read before written,
// by the same lane).
template <typename T, bool VEC, typename G>
__device__ __forceinline__ void row_map(const T* src, T* dst, int V, int tid, int nthr, G g) {
    constexpr int E = Chunk16<T>::E;
    if (VEC) {
        const int nchunk = V / E;
        float v[E];
        for (int c = tid; c < nchunk; c += nthr) {
            unpack16<T>(reinterpret_cast<const uint4*>(src)[c], v);
#pragma unroll
            for (int j = 0; j < E; ++j) v[j] = g(v[j], c * E + j);
            reinterpret_cast<uint4*>(dst)[c] = pack16<T>(v);
        }
        const int i = nchunk * E + tid;
        if (i < V) dst[i] = from_f<T>(g(to_f<T>(src[i]), i));
    } else {
        for (int i = tid; i < V; i += nthr) dst[i] = from_f<T>(g(to_f<T>(src[i]), i));
    }
}

template <typename T, bool VEC>
__device__ __forceinline__ void row_zero(T* dst, int V, int tid, int nthr) {
    constexpr int E = Chunk16<T>::E;
    if (VEC) {
        const int nchunk = V / E;
        for (int c = tid; c < nchunk; c += nthr) reinterpret_cast<uint4*>(dst)[c] = make_uint4(0, 0, 0, 0);
        const int i = nchunk * E + tid;
        if (i < V) dst[i] = from_f<T>(0.f);
    } else {
        for (int i = tid; i < V; i += nthr) dst[i] = from_f<T>(0.f);
    }
}

// workgroup reductions in a fixed order: xor tree inside a wave, then the XW_WAVES wave results in index order
__device__ __forceinline__ float xw_block_max(float v, float* red) {
    v = wave_max(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    float r = red[0];
#pragma unroll
    for (int w = 1; w < XW_WAVES; ++w) r = fmaxf(r, red[w]);
    return r;
}
__device__ __forceinline__ float xw_block_sum(float v, float* red) {
    v = wave_sum(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    float r = red[0];
#pragma unroll
    for (int w = 1; w < XW_WAVES; ++w) r += red[w];
    return r;
}

// hdr[0] = rows with 0 <= label < V (counted), hdr[1] = rows with label >= V (rejected).  Integer sums: exact in any order.
__global__ __launch_bounds__(256) void xent_wide_count_kernel(const int32_t* __restrict__ labels, int rows, int V,
                                                              int32_t* __restrict__ hdr) {
    __shared__ int cnt[256], rej[256];
    int c = 0, r = 0;
    for (int k = threadIdx.x; k < rows; k += 256) {
        const int lab = labels[k];
        c += (lab >= 0 && lab < V);
        r += (lab >= V);
    }
    cnt[threadIdx.x] = c;
    rej[threadIdx.x] = r;
    __syncthreads();
    if (threadIdx.x == 0) {
        int tc = 0, tr = 0;
        for (int k = 0; k < 256; ++k) { tc += cnt[k]; tr += rej[k]; }
        hdr[0] = tc;
        hdr[1] = tr;
    }
}

// per-row losses in index order -> mean over the counted rows; stats = {counted, rejected}
__global__ __launch_bounds__(256) void xent_wide_finalize_kernel(const float* __restrict__ rowloss, int rows,
                                                                 const int32_t* __restrict__ hdr, float* __restrict__ loss,
                                                                 int32_t* __restrict__ stats) {
    __shared__ float red[256];
    float s = 0.f;
    for (int k = threadIdx.x; k < rows; k += 256) s += rowloss[k];
    red[threadIdx.x] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        float t = 0.f;
        for (int k = 0; k < 256; ++k) t += red[k];
        const int counted = hdr[0];
        *loss = t / (float)(counted > 0 ? counted : 1);
        if (stats) { stats[0] = counted; stats[1] = hdr[1]; }
    }
}

// logits and dlogits carry no __restrict__: they may be one buffer
template <typename T, bool VEC>
__global__ __launch_bounds__(XW_THREADS) void xent_wide_staged_kernel(const T* logits, long ldl,
                                                                      const int32_t* __restrict__ labels,
                                                                      const int32_t* __restrict__ hdr,
                                                                      float* __restrict__ rowloss, T* dlogits, long lddl, int V) {
    extern __shared__ __align__(16) unsigned char xw_smem[];
    __shared__ float red[XW_WAVES];
    T* row = reinterpret_cast<T*>(xw_smem);
    const int tid = threadIdx.x;
    const long r = blockIdx.x;
    const int lab = labels[r];
    T* d = dlogits + r * lddl;
    if ((unsigned)lab >= (unsigned)V) {            // ignored (< 0) or rejected (>= V): no loss, a zero gradient row
        row_zero<T, VEC>(d, V, tid, XW_THREADS);
        if (tid == 0) rowloss[r] = 0.f;
        return;
    }
    const T* x = logits + r * ldl;
    constexpr int E = Chunk16<T>::E;
    if (VEC) {
        const int nchunk = V / E;
        for (int c = tid; c < nchunk; c += XW_THREADS) reinterpret_cast<uint4*>(row)[c] = reinterpret_cast<const uint4*>(x)[c];
        const int i = nchunk * E + tid;
        if (i < V) row[i] = x[i];
    } else {
        for (int i = tid; i < V; i += XW_THREADS) row[i] = x[i];
    }
    __syncthreads();
    float mx = -INFINITY;
    row_foreach<T, true>(row, V, tid, XW_THREADS, [&](const float* v, int n, int) {
        for (int j = 0; j < n; ++j) mx = fmaxf(mx, v[j]);
    });
    mx = xw_block_max(mx, red);
    float se = 0.f;
    row_foreach<T, true>(row, V, tid, XW_THREADS, [&](const float* v, int n, int) {
        for (int j = 0; j < n; ++j) se += expf(v[j] - mx);
    });
    se = xw_block_sum(se, red);
    const float lz = logf(se);
    if (tid == 0) rowloss[r] = lz - (to_f<T>(row[lab]) - mx);     // = lse - x[label]
    const int counted = hdr[0];
    const float inv = 1.0f / (float)(counted > 0 ? counted : 1);
    // (x - mx) - log(se), not x - lse: loss.hip:57
    row_map<T, VEC>(row, d, V, tid, XW_THREADS, [&](float v, int i) {
        return (expf((v - mx) - lz) - (i == lab ? 1.0f : 0.0f)) * inv;
    });
}

template <typename T, bool VEC>
__global__ __launch_bounds__(XW_THREADS) void xent_wide_stream_kernel(const T* logits, long ldl,
                                                                      const int32_t* __restrict__ labels,
                                                                      const int32_t* __restrict__ hdr,
                                                                      float* __restrict__ rowloss, T* dlogits, long lddl, int V) {
    __shared__ float red[XW_WAVES];
    const int tid = threadIdx.x;
    const long r = blockIdx.x;
    const int lab = labels[r];
    T* d = dlogits + r * lddl;
    if ((unsigned)lab >= (unsigned)V) {
        row_zero<T, VEC>(d, V, tid, XW_THREADS);
        if (tid == 0) rowloss[r] = 0.f;
        return;
    }
    const T* x = logits + r * ldl;
    const float xl = to_f<T>(x[lab]);              // before the second pass overwrites it (in place)
    // online max / sum: a lane's sum is rescaled only when a chunk raises its maximum
    float m = -INFINITY, s = 0.f;
    row_foreach<T, VEC>(x, V, tid, XW_THREADS, [&](const float* v, int n, int) {
        float cm = v[0];
        for (int j = 1; j < n; ++j) cm = fmaxf(cm, v[j]);
        if (cm > m) { s *= expf(m - cm); m = cm; }
        for (int j = 0; j < n; ++j) s += expf(v[j] - m);
    });
    const float mx = xw_block_max(m, red);
    const float se = xw_block_sum(s > 0.f ? s * expf(m - mx) : 0.f, red);   // a lane without elements: m = -inf, s = 0
    const float lz = logf(se);
    if (tid == 0) rowloss[r] = lz - (xl - mx);
    const int counted = hdr[0];
    const float inv = 1.0f / (float)(counted > 0 ? counted : 1);
    row_map<T, VEC>(x, d, V, tid, XW_THREADS, [&](float v, int i) {
        return (expf((v - mx) - lz) - (i == lab ? 1.0f : 0.0f)) * inv;
    });
}

// y[i] = x[idx[i]] (0 <= idx[i] < rows) or a zero row: one wave per output row
template <typename T, bool VEC>
__global__ __launch_bounds__(256) void gather_rows_kernel(const T* __restrict__ x, long ldx, const int32_t* __restrict__ idx,
                                                          T* __restrict__ y, long ldy, int n, int rows, int H) {
    const long i = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= n) return;
    const int lane = threadIdx.x & 63;
    const int src = idx[i];
    const bool valid = (unsigned)src < (unsigned)rows;
    const T* xs = x + (long)(valid ? src : 0) * ldx;
    T* yd = y + i * ldy;
    constexpr int E = Chunk16<T>::E;
    if (VEC) {
        const int nchunk = H / E;
        for (int c = lane; c < nchunk; c += 64)
            reinterpret_cast<uint4*>(yd)[c] = valid ? reinterpret_cast<const uint4*>(xs)[c] : make_uint4(0, 0, 0, 0);
        const int e = nchunk * E + lane;
        if (e < H) yd[e] = valid ? xs[e] : from_f<T>(0.f);
    } else {
        for (int e = lane; e < H; e += 64) yd[e] = valid ? xs[e] : from_f<T>(0.f);
    }
}

// inv[j] = the last i with idx[i] == j, or -1.  One workgroup walks idx in order, 256 entries a round: inside a round an
// entry is dropped when a later lane of the round holds the same target, and the barrier orders the rounds.
__global__ __launch_bounds__(256) void inverse_map_kernel(const int32_t* __restrict__ idx, int n, int32_t* __restrict__ inv, int rows) {
    __shared__ int32_t cur[256];
    const int tid = threadIdx.x;
    for (int j = tid; j < rows; j += 256) inv[j] = -1;
    __syncthreads();
    for (int base = 0; base < n; base += 256) {
        const int i = base + tid;
        const int v = i < n ? idx[i] : -1;
        cur[tid] = v;
        __syncthreads();
        bool write = (unsigned)v < (unsigned)rows;
        for (int t = tid + 1; t < 256 && write; ++t) write = cur[t] != v;
        if (write) inv[v] = i;
        __syncthreads();
    }
}

struct XwRoute { int streaming, vec, lds; };

int xw_validate(const char* who, int dtype, const void* logits, long ldl, const void* dlogits, long lddl, int rows, int V) {
    POLUS_REQUIRE(dtype == POLUS_F32 || dtype == POLUS_BF16, "%s: bad dtype %d", who, dtype);
    POLUS_REQUIRE(logits && dlogits, "%s: null pointer", who);
    POLUS_REQUIRE(rows > 0 && V > 0 && ldl >= V && lddl >= V, "%s: bad shape rows=%d V=%d ldl=%ld lddl=%ld", who, rows, V, ldl, lddl);
    POLUS_REQUIRE(logits != dlogits || ldl == lddl, "%s: in place needs lddl == ldl (%ld vs %ld)", who, lddl, ldl);
    const size_t es = polus_dtype_size(dtype);
    POLUS_REQUIRE(((uintptr_t)logits % es) == 0 && ((uintptr_t)dlogits % es) == 0, "%s: pointer not aligned to its element", who);
    return POLUS_OK;
}

XwRoute xw_route(int dtype, const void* logits, long ldl, const void* dlogits, long lddl, int V) {
    const size_t es = polus_dtype_size(dtype);
    XwRoute r;
    r.streaming = (size_t)V * es > (size_t)XW_STAGE_BYTES;
    r.vec = polus_aligned16(logits) && polus_aligned16(dlogits) && ((size_t)ldl * es) % 16 == 0 && ((size_t)lddl * es) % 16 == 0;
    r.lds = r.streaming ? 0 : (int)(((size_t)V * es + 15) / 16 * 16);
    return r;
}

template <typename T, bool VEC>
int xw_launch(const XwRoute& rt, const void* logits, long ldl, const int32_t* labels, const int32_t* hdr, float* rowloss,
              void* dlogits, long lddl, int rows, int V, hipStream_t st) {
    if (rt.streaming) {
        hipLaunchKernelGGL((xent_wide_stream_kernel<T, VEC>), dim3(rows), dim3(XW_THREADS), 0, st,
                           (const T*)logits, ldl, labels, hdr, rowloss, (T*)dlogits, lddl, V);
        POLUS_CHECK_LAUNCH("polus_softmax_xent_wide(streaming)");
        return POLUS_OK;
    }
    // the attribute is raised once per kernel to the most any launch asks for, not to this call's row
    return polus_launch_lds<xent_wide_staged_kernel<T, VEC>>("polus_softmax_xent_wide(staged)", dim3(rows), dim3(XW_THREADS),
                                                             XW_STAGE_BYTES, rt.lds, st, (const T*)logits, ldl, labels, hdr,
                                                             rowloss, (T*)dlogits, lddl, V);
}

}  // namespace

// {counted, rejected} + pad to 16 bytes, then one f32 per row
extern "C" size_t polus_softmax_xent_wide_workspace_bytes(int rows) {
    return 16 + (size_t)(rows > 0 ? rows : 0) * sizeof(float);
}

extern "C" int polus_softmax_xent_wide_route(int dtype, const void* logits, long ldl, const void* dlogits, long lddl,
                                             int rows, int V, int* out) {
    POLUS_REQUIRE(out, "polus_softmax_xent_wide_route: null out");
    int rc = xw_validate("polus_softmax_xent_wide", dtype, logits, ldl, dlogits, lddl, rows, V);
    if (rc != POLUS_OK) return rc;
    const XwRoute r = xw_route(dtype, logits, ldl, dlogits, lddl, V);
    out[0] = r.streaming; out[1] = r.vec; out[2] = r.lds;
    return POLUS_OK;
}

extern "C" int polus_softmax_xent_wide(int dtype, const void* logits, long ldl, const int32_t* labels, float* loss,
                                       void* dlogits, long lddl, int32_t* stats, int rows, int V,
                                       void* workspace, size_t workspace_bytes, void* stream) {
    int rc = xw_validate("polus_softmax_xent_wide", dtype, logits, ldl, dlogits, lddl, rows, V);
    if (rc != POLUS_OK) return rc;
    POLUS_REQUIRE(labels && loss, "polus_softmax_xent_wide: null pointer");
    if (!workspace || workspace_bytes < polus_softmax_xent_wide_workspace_bytes(rows)) { polus_set_error("polus_softmax_xent_wide: workspace too small"); return POLUS_ERR_WORKSPACE; }
    hipStream_t st = static_cast<hipStream_t>(stream);
    int32_t* hdr = static_cast<int32_t*>(workspace);
    float* rowloss = reinterpret_cast<float*>(static_cast<unsigned char*>(workspace) + 16);
    const XwRoute rt = xw_route(dtype, logits, ldl, dlogits, lddl, V);
    hipLaunchKernelGGL(xent_wide_count_kernel, dim3(1), dim3(256), 0, st, labels, rows, V, hdr);
    POLUS_CHECK_LAUNCH("polus_softmax_xent_wide(count)");
    if (dtype == POLUS_BF16)
        rc = rt.vec ? xw_launch<bf16_t, true>(rt, logits, ldl, labels, hdr, rowloss, dlogits, lddl, rows, V, st)
                    : xw_launch<bf16_t, false>(rt, logits, ldl, labels, hdr, rowloss, dlogits, lddl, rows, V, st);
    else
        rc = rt.vec ? xw_launch<float, true>(rt, logits, ldl, labels, hdr, rowloss, dlogits, lddl, rows, V, st)
                    : xw_launch<float, false>(rt, logits, ldl, labels, hdr, rowloss, dlogits, lddl, rows, V, st);
    if (rc != POLUS_OK) return rc;
    hipLaunchKernelGGL(xent_wide_finalize_kernel, dim3(1), dim3(256), 0, st, rowloss, rows, hdr, loss, stats);
    POLUS_CHECK_LAUNCH("polus_softmax_xent_wide(finalize)");
    return POLUS_OK;
}

extern "C" int polus_gather_rows(int dtype, const void* x, long ldx, const int32_t* idx, void* y, long ldy,
                                 int n, int rows, int H, void* stream) {
    POLUS_REQUIRE(dtype == POLUS_F32 || dtype == POLUS_BF16, "polus_gather_rows: bad dtype %d", dtype);
    POLUS_REQUIRE(x && idx && y && x != y, "polus_gather_rows: null pointer or y == x");
    POLUS_REQUIRE(n > 0 && rows > 0 && H > 0 && ldx >= H && ldy >= H, "polus_gather_rows: bad shape n=%d rows=%d H=%d ldx=%ld ldy=%ld", n, rows, H, ldx, ldy);
    const size_t es = polus_dtype_size(dtype);
    POLUS_REQUIRE(((uintptr_t)x % es) == 0 && ((uintptr_t)y % es) == 0, "polus_gather_rows: pointer not aligned to its element");
    const bool vec = polus_aligned16(x) && polus_aligned16(y) && ((size_t)ldx * es) % 16 == 0 && ((size_t)ldy * es) % 16 == 0;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const dim3 grid((unsigned)(((long)n + 3) / 4)), block(256);
    if (dtype == POLUS_BF16) {
        if (vec) hipLaunchKernelGGL((gather_rows_kernel<bf16_t, true>), grid, block, 0, st, (const bf16_t*)x, ldx, idx, (bf16_t*)y, ldy, n, rows, H);
        else hipLaunchKernelGGL((gather_rows_kernel<bf16_t, false>), grid, block, 0, st, (const bf16_t*)x, ldx, idx, (bf16_t*)y, ldy, n, rows, H);
    } else {
        if (vec) hipLaunchKernelGGL((gather_rows_kernel<float, true>), grid, block, 0, st, (const float*)x, ldx, idx, (float*)y, ldy, n, rows, H);
        else hipLaunchKernelGGL((gather_rows_kernel<float, false>), grid, block, 0, st, (const float*)x, ldx, idx, (float*)y, ldy, n, rows, H);
    }
    POLUS_CHECK_LAUNCH("polus_gather_rows");
    return POLUS_OK;
}

extern "C" int polus_inverse_map(const int32_t* idx, int n, int32_t* inv, int rows, void* stream) {
    POLUS_REQUIRE(idx && inv && idx != inv, "polus_inverse_map: null pointer or inv == idx");
    POLUS_REQUIRE(n > 0 && rows > 0, "polus_inverse_map: bad shape n=%d rows=%d", n, rows);
    hipLaunchKernelGGL(inverse_map_kernel, dim3(1), dim3(256), 0, static_cast<hipStream_t>(stream), idx, n, inv, rows);
    POLUS_CHECK_LAUNCH("polus_inverse_map");
    return POLUS_OK;
}
