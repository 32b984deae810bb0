// The producer of MX-FP4 rows for the streamed search (lpi_amd.search.quantize_mx4):
//   lpi_mx4_quantize        rows of f32 / bf16 / f16 -> e2m1 nibbles + E8M0 scales, one pass
// Format: mx4.h.  A 32-element block is held by 4 consecutive lanes, 8 elements each: the block maximum is two DPP steps inside the quad, a lane stores one
// dword of codes (element j of its eight in nibble j) and the first of the 4 the scale byte.  Plain arithmetic, bit for bit tests/mx4_emulate.py.
#include "mx4.h"
#include "dispatch.h"

namespace {

template <typename TX>
__global__ __launch_bounds__(256) void mx4_quantize_kernel(long nblk4, int kb, const TX* __restrict__ x, int ldx, uint8_t* __restrict__ q, int ldq,
                                                           uint8_t* __restrict__ sc, int lds)
{
    const long t = (long)blockIdx.x * 256 + threadIdx.x;      // lane t holds elements 8 t .. 8 t + 7 of the [rows, K] matrix in row-major block order
    const bool live = t < nblk4;                              // nblk4 = rows * K / 8: a multiple of 4, so the 4 lanes of a block live or die together
    const long blk = (live ? t : 0) >> 2;
    const int row = (int)(blk / kb), b = (int)(blk - (long)row * kb), sub = (int)(t & 3);
    const TX* p = x + (size_t)row * ldx + b * 32 + sub * 8;
    const f32x4 lo = Elem<TX>::ld4(p), hi = Elem<TX>::ld4(p + 4);
    float am = fmaxf(fmaxf(fmaxf(fabsf(lo[0]), fabsf(lo[1])), fmaxf(fabsf(lo[2]), fabsf(lo[3]))),
                     fmaxf(fmaxf(fabsf(hi[0]), fabsf(hi[1])), fmaxf(fabsf(hi[2]), fabsf(hi[3]))));
    am = fmaxf(am, dpp_move<0xB1>(am));      // lane ^ 1
    am = fmaxf(am, dpp_move<0x4E>(am));      // lane ^ 2: every lane takes part
    const int byte = mx4_scale_byte(am);
    if (!live) return;
    *reinterpret_cast<uint32_t*>(q + (size_t)row * ldq + b * 16 + sub * 4) = mx4_pack8(lo, hi, byte);
    if (sub == 0) sc[(size_t)row * lds + b] = (uint8_t)byte;
}

}  // namespace

extern "C" int lpi_mx4_quantize(int x_dtype, int rows, int K, const void* x, int ldx, void* q, int ldq, void* scales, int lds, void* stream)
{
    if (!x || !q || !scales || rows <= 0 || K <= 0 || (K & 31) || ldx < K || ldq < K / 2 || lds < K / 32 || (ldq & 3)) return LPI_EINVAL;
    const int esz = x_dtype == LPI_F32 ? 4 : 2;
    if ((ldx & 3) || ((uintptr_t)x & (4 * esz - 1)) || ((uintptr_t)q & 3)) return LPI_EINVAL;
    const long n = (long)rows * (K / 8);
    const dim3 g((unsigned)((n + 255) / 256)), b(256);
    hipStream_t s = (hipStream_t)stream;
    uint8_t *qp = (uint8_t*)q, *sp = (uint8_t*)scales;
    if (!dispatch_types(TypeList<Types<float>, Types<bf16_t>, Types<f16_t>>{}, [&](auto t) {
            typedef type_of<decltype(t)> TX;
            LPI_LAUNCH(mx4_quantize_kernel<TX>, g, b, 0, s, n, K / 32, (const TX*)x, ldx, qp, ldq, sp, lds);
        }, x_dtype))
        return LPI_EINVAL;
    LPI_CHECK_LAST();
    return 0;
}
