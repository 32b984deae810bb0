// MX-FP8 (OCP e4m3fn elements, one E8M0 scale byte per 32 consecutive K elements) helpers shared by gemm_mx8.hip and mx8_rows.hip.
//
// Block scale (include/lpi_hip.h): for the block maximum amax = m 2^x (m in [0.5, 1)) the scale exponent is e = x - 9, raised by one if
// amax 2^-e > 448 (m > 0.875) and clamped to [-127, 127]; the byte is e + 127.  In bits of the f32 amax (biased exponent E, 23 fraction bits F):
// byte = max(E - 8 + (F > 0x600000), 0) — a subnormal or zero amax (E = 0) gives byte 0, and E <= 254 keeps the byte below 248.  The elements are
// y 2^-e (exact: a power of two) rounded to nearest even by v_cvt_pk_fp8_f32, which on gfx950 is the OCP encoding with subnormals; by construction
// no element exceeds 448, so the conversion never saturates.
#pragma once
#include "gemm_host.h"
#include "gemm_epilogue.h"

// Element TAG of size 1 for the phased 256x256 tile (gemm256_tile.h): staging, swizzle and pointer arithmetic see a one-byte element, so a staged
// 128-byte row is 128 elements = one block-scaled instruction's K.  mx8_out_t is the C type tag of an MX output (e4m3 bytes + scales along N).
struct mx8_t { uint8_t v; };
struct mx8_out_t { uint8_t v; };
template <typename T> inline constexpr bool kIsMx8 = false;
template <> inline constexpr bool kIsMx8<mx8_t> = true;
template <> struct Elem<mx8_t> {
    static constexpr int DT = LPI_MX8;
    static constexpr int EPC = 16;
};
template <> struct AuxT<mx8_t> { typedef bf16_t type; };      // no MX epilogue takes an aux: the type only completes the shared signatures
// what an MX GEMM carries beside the element pointers: the operands' scale arrays and, for an MX output, C's
struct Mx8Side {
    const uint8_t* a_scales; int ldas;
    const uint8_t* b_scales; int ldbs;
    uint8_t* c_scales; int ldcs;
};
typedef __attribute__((ext_vector_type(8))) int mx8_i32x8;
// acc += W (x) X over 128 K elements: `w`, `x` = mx8_operand of the lane's chunks g and 4 + g of the weight / activation row, e4m3 both; the scale a lane holds
// is that of row l & 15, K block l >> 4 (gemm_mx8.hip has the measured operand map).
__device__ __forceinline__ mx8_i32x8 mx8_operand(const Chunk& c0, const Chunk& c1) {
    return mx8_i32x8{(int)c0.u.x, (int)c0.u.y, (int)c0.u.z, (int)c0.u.w, (int)c1.u.x, (int)c1.u.y, (int)c1.u.z, (int)c1.u.w};
}
// `ws`, `xs`: the registers that hold the lane's scale bytes, the instruction's in byte `wsel` / `xsel` (opsel: an immediate, hence the switch — the callers'
// loops are unrolled and it folds)
__device__ __forceinline__ void mx8_mma(f32x4& acc, const mx8_i32x8& w, const mx8_i32x8& x, int wsel, int ws, int xsel, int xs) {
#define LPI_MX8_MMA(I) case I: acc = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(w, x, acc, 0, 0, (I) >> 2, ws, (I) & 3, xs); break;
    switch (wsel * 4 + xsel) {
        LPI_MX8_MMA(0) LPI_MX8_MMA(1) LPI_MX8_MMA(2) LPI_MX8_MMA(3) LPI_MX8_MMA(4) LPI_MX8_MMA(5) LPI_MX8_MMA(6) LPI_MX8_MMA(7)
        LPI_MX8_MMA(8) LPI_MX8_MMA(9) LPI_MX8_MMA(10) LPI_MX8_MMA(11) LPI_MX8_MMA(12) LPI_MX8_MMA(13) LPI_MX8_MMA(14) LPI_MX8_MMA(15)
    }
#undef LPI_MX8_MMA
}

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

// Host: everything lpi_gemm_nt_mx8 and lpi_gemm_nt_mx8_256 check beside their shape predicates; 0 or the code to return before any launch.
inline int mx8_gemm_check_args(const GemmCall& c, const Mx8Side& mx)
{
    const lpi_gemm_desc& d = c.p;
    const int c_dtype = c.c_dtype, N = d.N, K = d.K;
    if (!d.A || !d.B || !d.C || !mx.a_scales || !mx.b_scales) return LPI_EINVAL;
    if (c.epilogue != LPI_EPI_NONE && c.epilogue != LPI_EPI_QUICKGELU) return LPI_EINVAL;
    if (c_dtype != LPI_F32 && c_dtype != LPI_BF16 && c_dtype != LPI_F16 && c_dtype != LPI_MX8) return LPI_EINVAL;
    if (d.lda < K || d.ldb < K || (d.lda & 15) || (d.ldb & 15) || mx.ldas < K / 32 || mx.ldbs < K / 32 || (mx.ldas & 3) || (mx.ldbs & 3) || d.ldc < N) return LPI_EINVAL;
    if ((((uintptr_t)d.A | (uintptr_t)d.B) & 15) || (((uintptr_t)mx.a_scales | (uintptr_t)mx.b_scales) & 3)) return LPI_EINVAL;
    if (d.bias && ((uintptr_t)d.bias & 15)) return LPI_EINVAL;
    const int csz = c_dtype == LPI_F32 ? 4 : c_dtype == LPI_MX8 ? 1 : 2;
    if (((uintptr_t)d.C & 15) || (d.ldc * csz) % (4 * csz)) return LPI_EINVAL;
    if (c_dtype == LPI_MX8 && (!mx.c_scales || mx.ldcs < N / 32 || d.residual)) return LPI_EINVAL;
    if (d.residual) {      // the residual has C's type: fp16 with an fp16 C (the residual stream of the 2-byte modes), f32 with an f32 C
        if (c.epilogue != LPI_EPI_NONE || c_dtype == LPI_BF16) return LPI_ENOSYS;
        if (d.ldr < N || (d.ldr & 3) || ((uintptr_t)d.residual & 15)) return LPI_EINVAL;
    }
    return 0;
}

// Host: a checked call's c_dtype, epilogue and residual -> f(Tag<TC>, Int<EPI>, Bool<RES>); MxOut is the caller's C type tag of an MX output.  A residual is
// built for the f32 and the fp16 C alone; LPI_EINVAL for any other c_dtype.
template <typename MxOut, typename F> int mx8_pick(const GemmCall& c, F f)
{
    auto epi = [&](auto tc, auto has_res) {
        if (c.epilogue == LPI_EPI_QUICKGELU) return f(tc, Int<LPI_EPI_QUICKGELU>{}, Bool<false>{});
        if constexpr (decltype(has_res)::value)
            if (c.p.residual) return f(tc, Int<LPI_EPI_NONE>{}, Bool<true>{});
        return f(tc, Int<LPI_EPI_NONE>{}, Bool<false>{});
    };
    switch (c.c_dtype) {
    case LPI_F32: return epi(Tag<float>{}, Bool<true>{});
    case LPI_BF16: return epi(Tag<bf16_t>{}, Bool<false>{});
    case LPI_F16: return epi(Tag<f16_t>{}, Bool<true>{});
    case LPI_MX8: return epi(Tag<MxOut>{}, Bool<false>{});
    }
    return LPI_EINVAL;
}
