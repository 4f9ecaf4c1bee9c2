// The e4m3fn row quantiser's device code (include/polus_hip.h polus_fp8_quantize_rows), shared by its two entry points:
// maxsim_fp8.hip (token rows of up to 256 features, one pass in registers) and refine.hip (whole [CLS] rows of up to 5120
// features, two passes over the row).  One rule, one place: the exponent from the row's largest magnitude, the exact
// multiplication by 2^-e, the hardware's round-to-nearest-even conversion.
#pragma once
#include "common.h"

typedef float f32x2 __attribute__((ext_vector_type(2)));
constexpr int F8_EMIN = -100;           // lowest scale exponent

// e of the rule for a row whose largest |x_k| is amax (NaN elements ignored by the caller's fmaxf).
// amax = m 2^k, m in [0.5, 1): k = (exponent field) - 126, m > 0.875 where the fraction passes 1.75.  A subnormal amax
// (field 0) lands below the clamp like every amax < 2^-91.
__device__ __forceinline__ int f8_row_exponent(float amax) {
    const unsigned bits = __float_as_uint(amax);
    int e = (int)(bits >> 23) - 126 - 9 + ((bits & 0x7fffffu) > 0x600000u ? 1 : 0);
    e = max(e, F8_EMIN);
    if (amax == 0.f) e = 0;
    return e;
}
__device__ __forceinline__ float f8_pow2(int e) { return __uint_as_float((unsigned)(e + 127) << 23); }

// Four codes (element k in bits 8k .. 8k+7) of v[0..3] * inv, inv = 2^-e: the products are exact.
__device__ __forceinline__ int f8_pack4(const float (&v)[4], float inv) {
    int w = 0;
    w = __builtin_amdgcn_cvt_pk_fp8_f32(v[0] * inv, v[1] * inv, w, false);
    w = __builtin_amdgcn_cvt_pk_fp8_f32(v[2] * inv, v[3] * inv, w, true);
    return w;
}

// T(code) * s for the four codes of w; exact for a power-of-two s
__device__ __forceinline__ void f8_unpack4(int w, float s, float (&v)[4]) {
    const f32x2 a = __builtin_amdgcn_cvt_pk_f32_fp8(w, false), b = __builtin_amdgcn_cvt_pk_f32_fp8(w, true);
    v[0] = a[0] * s; v[1] = a[1] * s; v[2] = b[0] * s; v[3] = b[1] * s;
}
