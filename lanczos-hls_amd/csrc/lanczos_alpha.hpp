// lanczos_alpha.hpp -- the two per-pixel conversions of LANCZOS_RESIZE_ALPHA (include/lanczos_hip.h):
// Pillow's RGBA -> RGBa before the passes and RGBa -> RGBA after them.  A pixel is one dword, alpha in the top byte, as the
// resize kernels hold it.  tests/native/resize_alpha_check.hip runs both over every (value, alpha) pair on the device and
// compares with the literal integer formulas.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace lz {

// c' = ((t >> 8) + t) >> 8 with t = c * A + 128 for the three colour bytes; alpha is unchanged
__device__ __forceinline__ uint32_t rs_premul_px(uint32_t p) {
    const uint32_t A = p >> 24;
    uint32_t r = p & 0xff000000u;
#pragma unroll
    for (int b = 0; b < 3; b++) {
        const uint32_t t = __umul24((p >> (8 * b)) & 255u, A) + 128u;
        r |= (((t >> 8) + t) >> 8) << (8 * b);
    }
    return r;
}

// c = min(255, 255 * c' / A) (truncating) for the three colour bytes unless A is 0 or 255.  The division runs in f32:
// with r = 255 / A to within a few ulp, c' * r is off the true quotient by less than 2^-14 wherever that quotient is below
// 256 (larger ones are clamped, and the error stays far below 1).  A true quotient has a fraction of j / A, j < A <= 254,
// so adding 1/512 (< 1/254) lifts every one of them clear of the integer below it without reaching the one above
// (1 - 1/254 + 1/512 + 2^-14 < 1): the truncation is the exact floor.
__device__ __forceinline__ uint32_t rs_unpremul_px(uint32_t p) {
    const uint32_t A = p >> 24;
    const float r = 255.0f * __builtin_amdgcn_rcpf((float)max(A, 1u));   // A = 0 is not divided by: p is returned
    uint32_t q = p & 0xff000000u;
#pragma unroll
    for (int b = 0; b < 3; b++) {
        const float v = __builtin_fmaf((float)((p >> (8 * b)) & 255u), r, 1.0f / 512.0f);
        q |= min((uint32_t)v, 255u) << (8 * b);
    }
    return (A == 0u || A == 255u) ? p : q;
}

}  // namespace lz
