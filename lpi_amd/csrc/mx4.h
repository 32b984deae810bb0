// MX-FP4 (OCP e2m1 elements, two per byte, one E8M0 scale byte per 32 consecutive K elements) helpers shared by the streamed search (search_tile.h,
// search_mx4.hip) and the quantiser (mx4_rows.hip).
//
// Format (include/lpi_hip.h; tests/mx4_emulate.py is the definition): a code is a sign bit and a magnitude in
// {0, 0.5, 1, 1.5, 2, 3, 4, 6}; element 2 j of a row is the low nibble of byte j, element 2 j + 1 the high one.  Block scale: for the block maximum amax with
// biased f32 exponent Eb the byte is max(Eb - 2, 0), the OCP rule e = floor(log2 amax) - 2 (a zero or subnormal amax: byte 0).  An element is
// y 2^(127 - byte) (exact: a power of two; below 8 in magnitude) rounded to nearest even on the e2m1 grid and saturating at +-6: values in (6, 8) become 6.
//
// Operand map of v_mfma_scale_f32_16x16x128_f8f6f4 with FP4 operands (cbsz = blgp = 4), measured on an MI355X (tools/probe/mx4_map_probe.hip; one wave, one
// instruction, integer nibbles and per-block scales against the host's sum): lane l holds row (l & 15) and, with g = l >> 4, the 32 CONSECUTIVE K elements
// 32 g .. 32 g + 31 in its four operand registers (16 bytes in K order; the upper four registers of the builtin's vector are not read) - unlike FP8, whose
// lane holds elements 16 g .. + 15 and 64 + 16 g .. + 15.  The scale of K block b of that row is byte `opsel` of the scale register of lane (l & 15) + 16 b,
// as for FP8: a lane's scale register holds the scale of its own 32 elements.  The other bytes of a scale register are not read.  The instruction pairs
// nibble positions with each other; two operands packed alike give the same sum in either nibble order, so the order inside a byte is the format's
// choice (low nibble first), not the instruction's.  Output as FP8: D[i = 4 (l >> 4) + e][j = l & 15] in register e, the first operand's rows are i.
#pragma once
#include "common.h"

// Element TAG of size 1: staging, swizzle and pointer arithmetic see a one-byte element, which is TWO FP4 values; a staged 128-byte row piece is 256
// elements = two instructions' K, and a 16-byte chunk is the 32 elements (one scale block) a lane hands one instruction.
struct mx4_t { uint8_t v; };
template <typename T> inline constexpr bool kIsMx4 = false;
template <> inline constexpr bool kIsMx4<mx4_t> = true;
template <> struct Elem<mx4_t> {
    static constexpr int DT = LPI_MX4;
    static constexpr int EPC = 16;      // bytes per 16-byte chunk
};
typedef __attribute__((ext_vector_type(8))) int mx4_i32x8;
// acc += W (x) X over 128 K elements: `w`, `x` = the lane's 16-byte chunk g of the step's 64 row bytes, `ws`, `xs` = registers whose low byte is the scale of
// that chunk (opsel 0).
__device__ __forceinline__ void mx4_mma(f32x4& acc, const Chunk& w, const Chunk& x, int ws, int xs) {
    const mx4_i32x8 w8{(int)w.u.x, (int)w.u.y, (int)w.u.z, (int)w.u.w, 0, 0, 0, 0};
    const mx4_i32x8 x8{(int)x.u.x, (int)x.u.y, (int)x.u.z, (int)x.u.w, 0, 0, 0, 0};
    acc = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(w8, x8, acc, 4, 4, 0, ws, 0, xs);
}

__device__ __forceinline__ int mx4_scale_byte(float amax) {
    const int v = (int)(__float_as_uint(amax) >> 23) - 2;      // amax >= 0, finite
    return v < 0 ? 0 : v;
}
// one value, already scaled (|v| < 8), -> its e2m1 code.  Codes 0 .. 4 are 0, 0.5 .. 2 (steps of 0.5), 4 .. 6 are 2, 3, 4 (steps of 1), 6 and 7 are 4 and 6
// (steps of 2): in each range rint (v_rndne_f32, ties to even) of the value in units of the step is the round to nearest even of the grid, because an
// even count of steps is a code with an even mantissa bit; 8 saturates to 6.
__device__ __forceinline__ uint32_t mx4_code(float v) {
    const float a = fabsf(v);
    int c;
    if (a < 2.f) c = (int)rintf(a * 2.f);
    else if (a < 4.f) c = (int)rintf(a) + 2;
    else c = min((int)rintf(a * 0.5f) + 4, 7);
    return (uint32_t)c | ((__float_as_uint(v) >> 28) & 8u);
}
// eight values of one block -> four bytes, element j in nibble j, scaled by 2^(127 - byte)
__device__ __forceinline__ uint32_t mx4_pack8(f32x4 lo, f32x4 hi, int byte) {
    const int sh = 127 - byte;
    uint32_t w = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        w |= mx4_code(__builtin_amdgcn_ldexpf(lo[j], sh)) << (4 * j);
        w |= mx4_code(__builtin_amdgcn_ldexpf(hi[j], sh)) << (16 + 4 * j);
    }
    return w;
}
