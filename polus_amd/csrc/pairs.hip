// Cross-encoder pair rows `cls q' sep d' sep pad...` built on the device from query rows, document rows and a
// candidate table (polus_amd/ir/cross.py, CrossEncoderTrainer in polus_amd/ir/training.py).
//
// The rule (include/polus_hip.h has it in full): the valid tokens of a row are those whose mask is non-zero, in
// order; the first `head` and last `tail` of them are dropped; of what remains the query keeps its first
// nq' = min(nq, max_q) and the document its first nd' = min(nd, S - 3 - nq').  A candidate id outside [0, N) is the
// empty document.
//
// One wave per output row, lanes over 64 consecutive source tokens per step, as in bio.hip: K = __ballot(mask != 0)
// and a token's rank among the valid ones is the popcount of K below the lane plus the valid tokens of earlier steps
// (a wave-uniform running count).  A first sweep over the mask gives the row's number of valid tokens (the tail
// strip needs it before any token can be placed); the second sweep stores token `rank` at its output column and
// stops at the step that places the last kept one.  Without a mask the rank is the column and there is no first
// sweep.  The special tokens, the padding, token_type_ids and attention_mask are one sweep over the S output
// columns.  Every store is a plain vector store to a distinct address: no LDS, no atomics, no workspace.
#include "common.h"

namespace {

constexpr int PAIR_THREADS = 256;                  // 4 waves = 4 output rows per workgroup
constexpr int PAIR_WAVES = PAIR_THREADS / 64;
constexpr int PAIR_MAX_BLOCKS = 4096;
constexpr int PAIR_MAX_STRIP = 8;
typedef unsigned long long u64;

struct PairArgs {
    const int32_t* qmask; long ldqm;
    const int32_t* dmask; long lddm;
    const int32_t* cand; long ldc;
    const int32_t* rows;
    int R, B, n, N, Lq, Ld;
    int q_head, q_tail, d_head, d_tail, max_q, S;
};

// valid tokens of one row (wave-uniform); a NULL mask row is all ones
__device__ __forceinline__ int pair_count(const int32_t* __restrict__ m, int L, int lane) {
    if (!m) return L;
    int cnt = 0;
    for (int base = 0; base < L; base += 64) {
        const int c = base + lane;
        cnt += __popcll(__ballot(c < L && m[c] != 0));
    }
    return cnt;
}

// tokens left of `valid` after the strips
__device__ __forceinline__ int pair_stripped(int valid, int head, int tail) {
    const int k = valid - head - tail;
    return k > 0 ? k : 0;
}

struct PairRow {
    int b, doc;            // query row; document row or -1 for the empty document
    int nq, nd;            // tokens kept after strips and truncation
};

__device__ __forceinline__ PairRow pair_resolve(const PairArgs& a, long r, int lane) {
    PairRow p;
    const int pi = a.rows ? a.rows[r] : (int)r;
    p.b = pi / a.n;
    const int c = a.cand[(size_t)p.b * a.ldc + (pi - p.b * a.n)];
    p.doc = (c >= 0 && c < a.N) ? c : -1;
    const int vq = pair_count(a.qmask ? a.qmask + (size_t)p.b * a.ldqm : nullptr, a.Lq, lane);
    const int nq = pair_stripped(vq, a.q_head, a.q_tail);
    p.nq = nq < a.max_q ? nq : a.max_q;
    p.nd = 0;
    if (p.doc >= 0) {                              // no document memory is read for a missing candidate
        const int vd = pair_count(a.dmask ? a.dmask + (size_t)p.doc * a.lddm : nullptr, a.Ld, lane);
        const int nd = pair_stripped(vd, a.d_head, a.d_tail);
        const int room = a.S - 3 - p.nq;           // >= 0: S >= max_q + 3
        p.nd = nd < room ? nd : room;
    }
    return p;
}

// out[col0 + k] = the k-th kept token, k < keep: the valid tokens of rank head .. head + keep - 1
__device__ __forceinline__ void pair_place(const int32_t* __restrict__ ids, const int32_t* __restrict__ m, int L, int head,
                                           int keep, int32_t* __restrict__ out, int col0, int lane) {
    if (keep <= 0) return;
    const int end = head + keep;
    if (!m) {                                      // rank == column; end <= L
        for (int c = head + lane; c < end; c += 64) out[col0 + c - head] = ids[c];
        return;
    }
    const u64 below = (1ull << lane) - 1ull;
    int seen = 0;                                  // valid tokens of earlier steps (uniform)
    for (int base = 0; base < L && seen < end; base += 64) {
        const int c = base + lane;
        const bool kept = c < L && m[c] != 0;
        const u64 K = __ballot(kept);
        const int rank = seen + __popcll(K & below);
        if (kept && rank >= head && rank < end) out[col0 + rank - head] = ids[c];
        seen += __popcll(K);
    }
}

__global__ __launch_bounds__(PAIR_THREADS) void pair_lengths_kernel(PairArgs a, int32_t* __restrict__ length) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (long r = (long)blockIdx.x * PAIR_WAVES + wave; r < a.R; r += (long)gridDim.x * PAIR_WAVES) {
        const PairRow p = pair_resolve(a, r, lane);
        if (lane == 0) length[r] = p.nq + p.nd + 3;
    }
}

__global__ __launch_bounds__(PAIR_THREADS) void pair_pack_kernel(
        PairArgs a, const int32_t* __restrict__ q_ids, long ldq, const int32_t* __restrict__ d_ids, long ldd,
        int cls, int sep, int pad, int32_t* __restrict__ input_ids, int32_t* __restrict__ token_type_ids,
        int32_t* __restrict__ attention_mask, long ldo, int32_t* __restrict__ length) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (long r = (long)blockIdx.x * PAIR_WAVES + wave; r < a.R; r += (long)gridDim.x * PAIR_WAVES) {
        const PairRow p = pair_resolve(a, r, lane);
        int32_t* oi = input_ids + (size_t)r * ldo;
        int32_t* ot = token_type_ids + (size_t)r * ldo;
        int32_t* om = attention_mask + (size_t)r * ldo;
        const int sep1 = 1 + p.nq, sep2 = 2 + p.nq + p.nd, len = sep2 + 1;      // len <= S
        pair_place(q_ids + (size_t)p.b * ldq, a.qmask ? a.qmask + (size_t)p.b * a.ldqm : nullptr, a.Lq, a.q_head, p.nq,
                   oi, 1, lane);
        if (p.doc >= 0)
            pair_place(d_ids + (size_t)p.doc * ldd, a.dmask ? a.dmask + (size_t)p.doc * a.lddm : nullptr, a.Ld, a.d_head,
                       p.nd, oi, sep1 + 1, lane);
        for (int c = lane; c < a.S; c += 64) {
            if (c == 0) oi[c] = cls;
            else if (c == sep1 || c == sep2) oi[c] = sep;
            else if (c >= len) oi[c] = pad;
            ot[c] = (c > sep1 && c < len) ? 1 : 0;
            om[c] = c < len ? 1 : 0;
        }
        if (length && lane == 0) length[r] = len;
    }
}

__global__ __launch_bounds__(PAIR_THREADS) void pair_scatter_scores_kernel(
        const float* __restrict__ s, const int32_t* __restrict__ rows, const int32_t* __restrict__ cand, long ldc,
        int R, int n, int N, float* __restrict__ out, long ldo) {
    for (long r = (long)blockIdx.x * PAIR_THREADS + threadIdx.x; r < R; r += (long)gridDim.x * PAIR_THREADS) {
        const int pi = rows ? rows[r] : (int)r;
        const int b = pi / n, j = pi - b * n;
        const int c = cand[(size_t)b * ldc + j];
        out[(size_t)b * ldo + j] = (c >= 0 && c < N) ? s[r] : -INFINITY;
    }
}

int pair_blocks(int R, int per_block) {
    const long blocks = ((long)R + per_block - 1) / per_block;
    return (int)(blocks < PAIR_MAX_BLOCKS ? blocks : PAIR_MAX_BLOCKS);
}

// the checks the two row-building entry points share
int pair_check(const char* who, const PairArgs& a) {
    POLUS_REQUIRE(a.cand, "%s: null pointer (cand)", who);
    POLUS_REQUIRE(a.R >= 1 && a.B >= 1 && a.n >= 1 && a.N >= 1 && a.Lq >= 1 && a.Ld >= 1,
                  "%s: need R, B, n, N, Lq, Ld >= 1 (got %d, %d, %d, %d, %d, %d)", who, a.R, a.B, a.n, a.N, a.Lq, a.Ld);
    POLUS_REQUIRE((long)a.B * a.n <= 2147483647L, "%s: B*n must be <= 2^31 - 1 (got %d x %d)", who, a.B, a.n);
    POLUS_REQUIRE(a.ldc >= a.n, "%s: candidate row stride ldc must be >= n (got %ld < %d)", who, a.ldc, a.n);
    POLUS_REQUIRE(!a.qmask || a.ldqm >= a.Lq, "%s: query mask row stride must be >= Lq (got %ld < %d)", who, a.ldqm, a.Lq);
    POLUS_REQUIRE(!a.dmask || a.lddm >= a.Ld, "%s: document mask row stride must be >= Ld (got %ld < %d)", who, a.lddm, a.Ld);
    POLUS_REQUIRE(a.q_head >= 0 && a.q_head <= PAIR_MAX_STRIP && a.q_tail >= 0 && a.q_tail <= PAIR_MAX_STRIP &&
                  a.d_head >= 0 && a.d_head <= PAIR_MAX_STRIP && a.d_tail >= 0 && a.d_tail <= PAIR_MAX_STRIP,
                  "%s: strip counts must be in 0..%d (got %d/%d, %d/%d)", who, PAIR_MAX_STRIP, a.q_head, a.q_tail,
                  a.d_head, a.d_tail);
    POLUS_REQUIRE(a.max_q >= 0, "%s: need max_q >= 0 (got %d)", who, a.max_q);
    POLUS_REQUIRE((long)a.S >= (long)a.max_q + 3, "%s: need S >= max_q + 3 (got S %d, max_q %d)", who, a.S, a.max_q);
    return POLUS_OK;
}

}  // namespace

extern "C" int polus_pair_lengths(const int32_t* qmask, long ldqm, const int32_t* dmask, long lddm, const int32_t* cand,
                                  long ldc, const int32_t* rows, int R, int B, int n, int N, int Lq, int Ld, int q_head,
                                  int q_tail, int d_head, int d_tail, int max_q, int S, int32_t* length, void* stream) {
    const PairArgs a = {qmask, ldqm, dmask, lddm, cand, ldc, rows, R, B, n, N, Lq, Ld, q_head, q_tail, d_head, d_tail, max_q, S};
    POLUS_REQUIRE(length, "polus_pair_lengths: null pointer (length)");
    if (int rc = pair_check("polus_pair_lengths", a)) return rc;
    hipLaunchKernelGGL(pair_lengths_kernel, dim3(pair_blocks(R, PAIR_WAVES)), dim3(PAIR_THREADS), 0,
                       static_cast<hipStream_t>(stream), a, length);
    POLUS_CHECK_LAUNCH("polus_pair_lengths");
    return POLUS_OK;
}

extern "C" int polus_pair_pack(const int32_t* q_ids, long ldq, const int32_t* qmask, long ldqm, const int32_t* d_ids, long ldd,
                               const int32_t* dmask, long lddm, const int32_t* cand, long ldc, const int32_t* rows, int R,
                               int B, int n, int N, int Lq, int Ld, int q_head, int q_tail, int d_head, int d_tail, int max_q,
                               int S, int cls, int sep, int pad, int32_t* input_ids, int32_t* token_type_ids,
                               int32_t* attention_mask, long ldo, int32_t* length, void* stream) {
    const PairArgs a = {qmask, ldqm, dmask, lddm, cand, ldc, rows, R, B, n, N, Lq, Ld, q_head, q_tail, d_head, d_tail, max_q, S};
    POLUS_REQUIRE(q_ids && d_ids && input_ids && token_type_ids && attention_mask, "polus_pair_pack: null pointer");
    if (int rc = pair_check("polus_pair_pack", a)) return rc;
    POLUS_REQUIRE(ldq >= Lq && ldd >= Ld, "polus_pair_pack: id row strides must be >= Lq, Ld (got %ld < %d or %ld < %d)",
                  ldq, Lq, ldd, Ld);
    POLUS_REQUIRE(ldo >= S, "polus_pair_pack: output row stride ldo must be >= S (got %ld < %d)", ldo, S);
    hipLaunchKernelGGL(pair_pack_kernel, dim3(pair_blocks(R, PAIR_WAVES)), dim3(PAIR_THREADS), 0,
                       static_cast<hipStream_t>(stream), a, q_ids, ldq, d_ids, ldd, cls, sep, pad, input_ids, token_type_ids,
                       attention_mask, ldo, length);
    POLUS_CHECK_LAUNCH("polus_pair_pack");
    return POLUS_OK;
}

extern "C" int polus_pair_scatter_scores(const float* s, const int32_t* rows, const int32_t* cand, long ldc, int R, int B,
                                         int n, int N, float* out, long ldo, void* stream) {
    POLUS_REQUIRE(s && cand && out, "polus_pair_scatter_scores: null pointer");
    POLUS_REQUIRE(R >= 1 && B >= 1 && n >= 1 && N >= 1, "polus_pair_scatter_scores: need R, B, n, N >= 1 (got %d, %d, %d, %d)",
                  R, B, n, N);
    POLUS_REQUIRE((long)B * n <= 2147483647L, "polus_pair_scatter_scores: B*n must be <= 2^31 - 1 (got %d x %d)", B, n);
    POLUS_REQUIRE(ldc >= n && ldo >= n, "polus_pair_scatter_scores: row strides ldc, ldo must be >= n (got %ld, %ld < %d)",
                  ldc, ldo, n);
    hipLaunchKernelGGL(pair_scatter_scores_kernel, dim3(pair_blocks(R, PAIR_THREADS)), dim3(PAIR_THREADS), 0,
                       static_cast<hipStream_t>(stream), s, rows, cand, ldc, R, n, N, out, ldo);
    POLUS_CHECK_LAUNCH("polus_pair_scatter_scores");
    return POLUS_OK;
}
