// MX-FP8 (OCP e4m3fn elements, one E8M0 scale byte per 32 consecutive K elements) helpers shared by gemm_mx8.hip and mx8_rows.hip.
//
// Block scale (include/lpi_hip.h): for the block maximum amax = m 2^x (m in [0.5, 1)) the scale exponent is e = x - 9, raised by one if
// amax 2^-e > 448 (m > 0.875) and clamped to [-127, 127]; the byte is e + 127.  In bits of the f32 amax (biased exponent E, 23 fraction bits F):
// byte = max(E - 8 + (F > 0x600000), 0) — a subnormal or zero amax (E = 0) gives byte 0, and E <= 254 keeps the byte below 248.  The elements are
// y 2^-e (exact: a power of two) rounded to nearest even by v_cvt_pk_fp8_f32, which on gfx950 is the OCP encoding with subnormals; by construction
// no element exceeds 448, so the conversion never saturates.
#pragma once
#include "common.h"

__device__ __forceinline__ int mx8_scale_byte(float amax) {
    const uint32_t b = __float_as_uint(amax);      // amax >= 0
    const int v = (int)(b >> 23) - 8 + ((b & 0x7FFFFFu) > 0x600000u ? 1 : 0);
    return v < 0 ? 0 : v;
}
// four values of one block -> four e4m3 bytes (element j in byte j), scaled by 2^(127 - byte)
__device__ __forceinline__ uint32_t mx8_pack4(f32x4 v, int byte) {
    const int sh = 127 - byte;
    int w = 0;
    w = __builtin_amdgcn_cvt_pk_fp8_f32(__builtin_amdgcn_ldexpf(v[0], sh), __builtin_amdgcn_ldexpf(v[1], sh), w, false);
    w = __builtin_amdgcn_cvt_pk_fp8_f32(__builtin_amdgcn_ldexpf(v[2], sh), __builtin_amdgcn_ldexpf(v[3], sh), w, true);
    return (uint32_t)w;
}
__device__ __forceinline__ float mx8_amax4(f32x4 v) { return fmaxf(fmaxf(fabsf(v[0]), fabsf(v[1])), fmaxf(fabsf(v[2]), fabsf(v[3]))); }
// maximum over the 8 consecutive lanes that hold one 32-element block (4 elements each): lane ^ 1, lane ^ 2, then the other quad of the 8
__device__ __forceinline__ float mx8_max8(float v) {
    v = fmaxf(v, dpp_move<0xB1>(v));
    v = fmaxf(v, dpp_move<0x4E>(v));
    v = fmaxf(v, dpp_move<0x141>(v));
    return v;
}
