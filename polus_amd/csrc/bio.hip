// BIO span decoding and strict entity matching over tag tensors (polus_amd/ner/bio.py, polus_amd/ner/metrics.py).
//
// The rule (include/polus_hip.h has it in full): scheme[tag] is -1 for an outside tag and 2 * type + (1 for I-) otherwise;
// masked-out tokens are removed before decoding; a kept token is IN an entity iff its code is not -1, STARTS one iff
// it is B-x, or I-x whose previous kept token is absent, outside or of another type, and ENDS one iff it is in one and
// the next kept token is absent, outside or a start.
//
// One wave per row, lanes over 64 consecutive tokens per step.  The kept (K), start (ST) and disagree (D) flags of a step
// are 64-bit __ballot masks and everything else is a bit operation on them: the previous kept lane is the highest set
// bit of K below the lane.  A token's end flag needs the NEXT kept token, which may lie any number of steps ahead (a
// mask hole), so it is evaluated there: lane j holds the bit
//     CLOSE(j) = previous kept token is in an entity && (j is outside || j starts),
// which is the end flag of the previous kept token, and one virtual token behind the row closes what is still open.
// The entity closed at lane j began at the highest ST bit below j (or in an earlier step: carry) and its index in the
// row is the number of ST bits below j plus the starts of earlier steps, minus one: start order without a slot counter.
// Matching: token j DISAGREES (bit D) when the two sides differ in in-entity, or are both in one and differ in type or
// start.  An entity of side a closed at j is common iff no D bit lies between its start and j - 1 and side b closes
// there too (b is outside or starts at j): that is agreement on (in, start, end, type) at each of its tokens.
// The carry between steps is uniform across the wave: per side the last kept token's code, for side a whether the open
// entity still agrees, for spans the open entity's start, the last kept column and the row's span count.
// Per-type counts go to a per-workgroup LDS histogram, then one global integer atomic per non-zero cell: exact and
// independent of launch order.
#include "common.h"

namespace {

constexpr int BIO_THREADS = 256;                   // 4 waves = 4 rows in flight per workgroup
constexpr int BIO_WAVES = BIO_THREADS / 64;
constexpr int BIO_MAXC = 256;
constexpr int BIO_MAXT = 128;
constexpr int BIO_MAX_BLOCKS = 2048;
typedef unsigned long long u64;

__device__ __forceinline__ u64 bio_below(int lane) { return (1ull << lane) - 1ull; }          // bits of lanes < lane
__device__ __forceinline__ int bio_top(u64 m) { return 63 - __clzll((long long)m); }          // highest set bit, m != 0

// scheme -> LDS; a code that names a type >= T (the wrapper refuses such a table) is outside rather than out of bounds
__device__ __forceinline__ void bio_load_scheme(int* s_scheme, const int32_t* __restrict__ scheme, int C, int T) {
    for (int k = threadIdx.x; k < C; k += BIO_THREADS) {
        const int code = scheme[k];
        s_scheme[k] = (code >= 0 && code < 2 * T) ? code : -1;
    }
}

// One side of one step.  `tag` is interpreted on kept lanes only.  Out: the lane's code (-1 on lanes that are not
// kept), the previous kept token's code (carry when no kept lane lies below), and the step's masks.
struct BioSide {
    int code, prev;
    bool in, start, close;
    u64 ST;
    int rejected, i_after_other, i_other_type;     // uniform counts of this step
};

__device__ __forceinline__ BioSide bio_decode(int tag, bool kept, int prev_lane, bool has_prev, int carry_code,
                                              const int* s_scheme, int C) {
    BioSide r;
    const bool valid = kept && (unsigned)tag < (unsigned)C;
    r.code = valid ? s_scheme[tag] : -1;
    const int shuffled = __shfl(r.code, prev_lane, 64);        // every lane takes part; prev_lane is 0 without one
    r.prev = has_prev ? shuffled : carry_code;
    r.in = r.code >= 0;
    const bool inside_tag = r.in && (r.code & 1);
    const bool after_other = inside_tag && r.prev < 0;
    const bool other_type = inside_tag && r.prev >= 0 && (r.prev >> 1) != (r.code >> 1);
    r.start = r.in && (!(r.code & 1) || after_other || other_type);
    r.close = kept && r.prev >= 0 && (!r.in || r.start);
    r.ST = __ballot(r.start);
    r.rejected = __popcll(__ballot(kept && !valid));
    r.i_after_other = __popcll(__ballot(after_other));
    r.i_other_type = __popcll(__ballot(other_type));
    return r;
}

__global__ __launch_bounds__(BIO_THREADS) void bio_entity_counts_kernel(
        const int32_t* __restrict__ tags_a, long lda, const int32_t* __restrict__ tags_b, long ldb,
        const int32_t* __restrict__ mask, long ldm, const int32_t* __restrict__ scheme, int C, int T, int B, int S,
        int32_t* __restrict__ counts, int32_t* __restrict__ stats) {
    __shared__ int s_scheme[BIO_MAXC];
    __shared__ int s_hist[BIO_MAXT * 3];
    __shared__ int s_stats[6];
    bio_load_scheme(s_scheme, scheme, C, T);
    for (int k = threadIdx.x; k < T * 3; k += BIO_THREADS) s_hist[k] = 0;
    if (threadIdx.x < 6) s_stats[threadIdx.x] = 0;
    __syncthreads();

    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const u64 below = bio_below(lane);
    for (long row = (long)blockIdx.x * BIO_WAVES + wave; row < B; row += (long)gridDim.x * BIO_WAVES) {
        const int32_t* ra = tags_a + (size_t)row * lda;
        const int32_t* rb = tags_b + (size_t)row * ldb;
        const int32_t* rm = mask ? mask + (size_t)row * ldm : nullptr;
        int carry_a = -1, carry_b = -1;            // code of the last kept token so far
        bool carry_agree = true;                   // no D bit since side a's open entity began
        int st[6] = {0, 0, 0, 0, 0, 0};            // uniform; added to LDS once per row

        // the next step's loads are issued before this step's bit work; a tag at a masked-out position is loaded
        // (it lies inside the row) and never interpreted
        int ta = lane < S ? ra[lane] : 0, tb = lane < S ? rb[lane] : 0;
        int mk = lane < S ? (rm ? rm[lane] : 1) : 0;
        for (int base = 0; base < S; base += 64) {
            const int cn = base + 64 + lane;
            const bool more = cn < S;
            const int ta_n = more ? ra[cn] : 0, tb_n = more ? rb[cn] : 0;
            const int mk_n = more ? (rm ? rm[cn] : 1) : 0;

            const bool kept = mk != 0;             // 0 behind the row's end
            const u64 K = __ballot(kept);
            if (K != 0) {                          // uniform; a step without a kept token changes nothing
                const u64 kb = K & below;
                const bool has_prev = kb != 0;
                const int prev_lane = has_prev ? bio_top(kb) : 0;
                const BioSide a = bio_decode(ta, kept, prev_lane, has_prev, carry_a, s_scheme, C);
                const BioSide b = bio_decode(tb, kept, prev_lane, has_prev, carry_b, s_scheme, C);
                const bool disagree = a.in != b.in || (a.in && ((a.code >> 1) != (b.code >> 1) || a.start != b.start));
                const u64 D = __ballot(disagree);
                // side a's entity closed here: D bits from its start (this step's, else the carry) to lane - 1
                const u64 sb = a.ST & below;
                const u64 span = sb ? below & ~bio_below(bio_top(sb)) : below;
                const bool agree = (sb != 0 || carry_agree) && (D & span) == 0;
                if (a.close && agree && (!b.in || b.start)) atomicAdd(&s_hist[(a.prev >> 1) * 3 + 0], 1);
                if (a.start) atomicAdd(&s_hist[(a.code >> 1) * 3 + 1], 1);
                if (b.start) atomicAdd(&s_hist[(b.code >> 1) * 3 + 2], 1);

                const int last = bio_top(K);
                carry_a = __shfl(a.code, last, 64);
                carry_b = __shfl(b.code, last, 64);
                carry_agree = a.ST ? (D & ~bio_below(bio_top(a.ST))) == 0 : (carry_agree && D == 0);
                st[0] += __popcll(K);
                st[1] += a.rejected + b.rejected;
                st[2] += a.i_after_other; st[3] += a.i_other_type;
                st[4] += b.i_after_other; st[5] += b.i_other_type;
            }
            ta = ta_n; tb = tb_n; mk = mk_n;
        }
        if (lane == 0) {
            // the virtual token behind the row closes the open entity on both sides
            if (carry_a >= 0 && carry_b >= 0 && carry_agree) atomicAdd(&s_hist[(carry_a >> 1) * 3 + 0], 1);
#pragma unroll
            for (int k = 0; k < 6; ++k)
                if (st[k]) atomicAdd(&s_stats[k], st[k]);
        }
    }
    __syncthreads();
    for (int k = threadIdx.x; k < T * 3; k += BIO_THREADS)
        if (s_hist[k]) atomicAdd(&counts[k], s_hist[k]);
    if (threadIdx.x < 6 && s_stats[threadIdx.x]) atomicAdd(&stats[threadIdx.x], s_stats[threadIdx.x]);
}

__global__ __launch_bounds__(BIO_THREADS) void bio_spans_kernel(
        const int32_t* __restrict__ tags, long ldt, const int32_t* __restrict__ mask, long ldm,
        const int32_t* __restrict__ scheme, int C, int B, int S, int32_t* __restrict__ spans, int M,
        int32_t* __restrict__ count, int32_t* __restrict__ rejected) {
    __shared__ int s_scheme[BIO_MAXC];
    bio_load_scheme(s_scheme, scheme, C, 1 << 29);             // every type is written out as it stands
    __syncthreads();

    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const u64 below = bio_below(lane);
    for (long row = (long)blockIdx.x * BIO_WAVES + wave; row < B; row += (long)gridDim.x * BIO_WAVES) {
        const int32_t* rt = tags + (size_t)row * ldt;
        const int32_t* rm = mask ? mask + (size_t)row * ldm : nullptr;
        int32_t* out = spans + (size_t)row * M * 3;
        int carry = -1;                            // code of the last kept token so far
        int carry_col = -1, carry_start = -1;      // its column; the column where the open entity began
        int n = 0, bad = 0;                        // entities begun so far; rejected ids

        int tg = lane < S ? rt[lane] : 0;
        int mk = lane < S ? (rm ? rm[lane] : 1) : 0;
        for (int base = 0; base < S; base += 64) {
            const int cn = base + 64 + lane;
            const bool more = cn < S;
            const int tg_n = more ? rt[cn] : 0;
            const int mk_n = more ? (rm ? rm[cn] : 1) : 0;

            const bool kept = mk != 0;
            const u64 K = __ballot(kept);
            if (K != 0) {                          // uniform
                const u64 kb = K & below;
                const bool has_prev = kb != 0;
                const int prev_lane = has_prev ? bio_top(kb) : 0;
                const BioSide a = bio_decode(tg, kept, prev_lane, has_prev, carry, s_scheme, C);
                if (a.close) {
                    const u64 sb = a.ST & below;
                    const int idx = n + __popcll(sb) - 1;      // >= 0: the closed entity began before this lane
                    if (idx < M) {
                        int32_t* o = out + (size_t)idx * 3;
                        o[0] = sb ? base + bio_top(sb) : carry_start;
                        o[1] = (has_prev ? base + prev_lane : carry_col) + 1;
                        o[2] = a.prev >> 1;
                    }
                }
                const int last = bio_top(K);
                carry = __shfl(a.code, last, 64);
                carry_col = base + last;
                if (a.ST) carry_start = base + bio_top(a.ST);
                n += __popcll(a.ST);
                bad += a.rejected;
            }
            tg = tg_n; mk = mk_n;
        }
        if (lane == 0) {
            if (carry >= 0 && n - 1 < M) {         // the virtual token behind the row closes the open entity
                int32_t* o = out + (size_t)(n - 1) * 3;
                o[0] = carry_start;
                o[1] = carry_col + 1;
                o[2] = carry >> 1;
            }
            count[row] = n;
            if (rejected && bad) atomicAdd(rejected, bad);
        }
    }
}

int bio_blocks(int B) {
    const int blocks = (B + BIO_WAVES - 1) / BIO_WAVES;
    return blocks < BIO_MAX_BLOCKS ? blocks : BIO_MAX_BLOCKS;
}

}  // namespace

extern "C" int polus_bio_entity_counts(const int32_t* tags_a, long lda, const int32_t* tags_b, long ldb,
                                       const int32_t* mask, long ldm, const int32_t* scheme, int C, int T,
                                       int B, int S, int32_t* counts, int32_t* stats, void* stream) {
    POLUS_REQUIRE(C > 0 && C <= BIO_MAXC, "polus_bio_entity_counts: need 0 < C <= %d tags (got %d)", BIO_MAXC, C);
    POLUS_REQUIRE(T > 0 && T <= BIO_MAXT, "polus_bio_entity_counts: need 0 < T <= %d entity types (got %d)", BIO_MAXT, T);
    POLUS_REQUIRE(B >= 0 && S >= 1, "polus_bio_entity_counts: need B >= 0 and S >= 1 (got %d, %d)", B, S);
    POLUS_REQUIRE(lda >= S && ldb >= S, "polus_bio_entity_counts: tag row strides must be >= S (got %ld, %ld < %d)", lda, ldb, S);
    POLUS_REQUIRE(!mask || ldm >= S, "polus_bio_entity_counts: mask row stride ldm must be >= S (got %ld < %d)", ldm, S);
    POLUS_REQUIRE(tags_a && tags_b && scheme && counts && stats, "polus_bio_entity_counts: null pointer");
    if (B == 0) return POLUS_OK;
    hipLaunchKernelGGL(bio_entity_counts_kernel, dim3(bio_blocks(B)), dim3(BIO_THREADS), 0, static_cast<hipStream_t>(stream),
                       tags_a, lda, tags_b, ldb, mask, ldm, scheme, C, T, B, S, counts, stats);
    POLUS_CHECK_LAUNCH("polus_bio_entity_counts");
    return POLUS_OK;
}

extern "C" int polus_bio_spans(const int32_t* tags, long ldt, const int32_t* mask, long ldm, const int32_t* scheme,
                               int C, int B, int S, int32_t* spans, int M, int32_t* count, int32_t* rejected,
                               void* stream) {
    POLUS_REQUIRE(C > 0 && C <= BIO_MAXC, "polus_bio_spans: need 0 < C <= %d tags (got %d)", BIO_MAXC, C);
    POLUS_REQUIRE(B >= 0 && S >= 1 && M >= 1, "polus_bio_spans: need B >= 0, S >= 1 and M >= 1 (got %d, %d, %d)", B, S, M);
    POLUS_REQUIRE(ldt >= S, "polus_bio_spans: tag row stride ldt must be >= S (got %ld < %d)", ldt, S);
    POLUS_REQUIRE(!mask || ldm >= S, "polus_bio_spans: mask row stride ldm must be >= S (got %ld < %d)", ldm, S);
    POLUS_REQUIRE(tags && scheme && spans && count, "polus_bio_spans: null pointer");
    if (B == 0) return POLUS_OK;
    hipLaunchKernelGGL(bio_spans_kernel, dim3(bio_blocks(B)), dim3(BIO_THREADS), 0, static_cast<hipStream_t>(stream),
                       tags, ldt, mask, ldm, scheme, C, B, S, spans, M, count, rejected);
    POLUS_CHECK_LAUNCH("polus_bio_spans");
    return POLUS_OK;
}
