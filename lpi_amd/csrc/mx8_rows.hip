// Row kernels of the MX-FP8 forward (EngineOptions.mx8_forward): the producers of the MX operands that no GEMM epilogue writes.
//   lpi_mx8_quantize        rows of f32 / bf16 / f16 -> e4m3 + E8M0 scales, one pass (weights at construction, the attention output ctx)
//   lpi_layernorm_mx8_fwd   a row of the fp16 / f32 residual stream -> two-sweep f32 statistics in registers, affine LayerNorm in f32, e4m3 + scales:
//                           LN(x) is never written in a 2-byte type (model.py:154-160,172-177 of the reference: ln_1 -> in_proj, ln_2 -> c_fc)
// Format: mx8.h.  A 32-element block is held by 8 consecutive lanes, 4 elements each: the block maximum is three DPP steps, a lane stores one dword of
// elements and the first of the 8 the scale byte.
#include "mx8.h"
#include "dispatch.h"

namespace {

template <typename TX>
__global__ __launch_bounds__(256) void mx8_quantize_kernel(long nblk8, int kb, const TX* __restrict__ x, int ldx, uint8_t* __restrict__ q, int ldq,
                                                           uint8_t* __restrict__ sc, int lds)
{
    const long t = (long)blockIdx.x * 256 + threadIdx.x;      // lane t holds elements 4 t .. 4 t + 3 of the [rows, K] matrix in row-major block order
    const bool live = t < nblk8;                              // nblk8 = rows * K / 4: a multiple of 8, so the 8 lanes of a block live or die together
    const long blk = (live ? t : 0) >> 3;
    const int row = (int)(blk / kb), b = (int)(blk - (long)row * kb), sub = (int)(t & 7);
    const f32x4 v = Elem<TX>::ld4(x + (size_t)row * ldx + b * 32 + sub * 4);
    const int byte = mx8_scale_byte(mx8_max8(mx8_amax4(v)));
    if (!live) return;
    *reinterpret_cast<uint32_t*>(q + (size_t)row * ldq + b * 32 + sub * 4) = mx8_pack4(v, byte);
    if (sub == 0) sc[(size_t)row * lds + b] = (uint8_t)byte;
}

// one wave per row; lane l holds elements 256 c + 4 l .. + 3 of chunk c < NC (d <= 256 NC, a multiple of 32: a block's 8 lanes are all inside or all outside)
template <typename TX, int NC>
__global__ __launch_bounds__(256) void ln_mx8_kernel(int rows, int d, const TX* __restrict__ x, int ldx, const float* __restrict__ gamma,
                                                     const float* __restrict__ beta, uint8_t* __restrict__ q, int ldq, uint8_t* __restrict__ sc, int lds,
                                                     float* __restrict__ mean, float* __restrict__ rstd)
{
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;      // whole waves leave
    const TX* xr = x + (size_t)row * ldx;
    f32x4 v[NC];
    float s = 0.f;
#pragma unroll
    for (int c = 0; c < NC; ++c) {
        const int e = c * 256 + lane * 4;
        v[c] = e < d ? Elem<TX>::ld4(xr + e) : f32x4{0.f, 0.f, 0.f, 0.f};
        s += (v[c][0] + v[c][1]) + (v[c][2] + v[c][3]);
    }
    const float mu = wave_sum(s) / (float)d;
    float ss = 0.f;
#pragma unroll
    for (int c = 0; c < NC; ++c) {
        const int e = c * 256 + lane * 4;
        const f32x4 t = v[c] - mu;
        if (e < d) ss += (t[0] * t[0] + t[1] * t[1]) + (t[2] * t[2] + t[3] * t[3]);
    }
    const float rs = 1.0f / sqrtf(wave_sum(ss) / (float)d + 1e-5f);
    if (lane == 0) {
        if (mean) mean[row] = mu;
        if (rstd) rstd[row] = rs;
    }
#pragma unroll
    for (int c = 0; c < NC; ++c) {
        const int e = c * 256 + lane * 4;
        const bool in = e < d;
        const int ec = in ? e : 0;
        const f32x4 g = *reinterpret_cast<const f32x4*>(gamma + ec), b = *reinterpret_cast<const f32x4*>(beta + ec);
        const f32x4 y = (v[c] - mu) * rs * g + b;
        const int byte = mx8_scale_byte(mx8_max8(mx8_amax4(y)));      // every lane takes part in the DPP steps
        if (in) {
            *reinterpret_cast<uint32_t*>(q + (size_t)row * ldq + e) = mx8_pack4(y, byte);
            if ((lane & 7) == 0) sc[(size_t)row * lds + (e >> 5)] = (uint8_t)byte;
        }
    }
}

}  // namespace

extern "C" int lpi_mx8_quantize(int x_dtype, int rows, int K, const void* x, int ldx, void* q, int ldq, void* scales, int lds, void* stream)
{
    if (!x || !q || !scales || rows <= 0 || K <= 0 || (K & 31) || ldx < K || ldq < K || lds < K / 32 || (ldq & 3)) return LPI_EINVAL;
    const int esz = x_dtype == LPI_F32 ? 4 : 2;
    if ((ldx & 3) || ((uintptr_t)x & (4 * esz - 1)) || ((uintptr_t)q & 3)) return LPI_EINVAL;
    const long n = (long)rows * (K / 4);
    const dim3 g((unsigned)((n + 255) / 256)), b(256);
    hipStream_t s = (hipStream_t)stream;
    uint8_t *qp = (uint8_t*)q, *sp = (uint8_t*)scales;
    if (!dispatch_types(TypeList<Types<float>, Types<bf16_t>, Types<f16_t>>{}, [&](auto t) {
            typedef type_of<decltype(t)> TX;
            LPI_LAUNCH(mx8_quantize_kernel<TX>, g, b, 0, s, n, K / 32, (const TX*)x, ldx, qp, ldq, sp, lds);
        }, x_dtype))
        return LPI_EINVAL;
    LPI_CHECK_LAST();
    return 0;
}

extern "C" int lpi_layernorm_mx8_fwd(int x_dtype, int rows, int d, const void* x, int ldx, const float* gamma, const float* beta, void* q, int ldq,
                                     void* scales, int lds, float* mean, float* rstd, void* stream)
{
    if (!x || !gamma || !beta || !q || !scales || rows <= 0 || d <= 0 || (d & 31) || d > 1024 || ldx < d || ldq < d || lds < d / 32 || (ldq & 3) || (ldx & 3))
        return LPI_EINVAL;
    if (((uintptr_t)x & (x_dtype == LPI_F32 ? 15 : 7)) || ((uintptr_t)q & 3) || (((uintptr_t)gamma | (uintptr_t)beta) & 15)) return LPI_EINVAL;
    const dim3 g((unsigned)((rows + 3) / 4)), b(256);
    hipStream_t s = (hipStream_t)stream;
    uint8_t *qp = (uint8_t*)q, *sp = (uint8_t*)scales;
    if (!dispatch_types(TypeList<Types<float>, Types<f16_t>>{}, [&](auto t) {
            typedef type_of<decltype(t)> TX;
            dispatch_nc<1, 2, 3, 4>(d, [&](auto nc) {
                LPI_LAUNCH((ln_mx8_kernel<TX, nc>), g, b, 0, s, rows, d, (const TX*)x, ldx, gamma, beta, qp, ldq, sp, lds, mean, rstd);
            });
        }, x_dtype))
        return LPI_EINVAL;
    LPI_CHECK_LAST();
    return 0;
}
