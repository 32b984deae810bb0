// Resampling of a ViT position table to another patch grid (lpi_pos_embed_resample): what OpenCLIP's and timm's resize_pos_embed do with
// torch.nn.functional.interpolate(table.reshape(1, g, g, d).permute(0, 3, 1, 2), size=(g', g'), mode=..., align_corners=False, antialias=...) when a
// checkpoint runs at a resolution other than the one its table was trained at.  Called once per engine, never per step: written plainly, one workgroup per
// output row, no tuning.
//
// torch's arithmetic, restated per axis (scale = g_in / g_out; verified against torch on the CPU in float64, tests/test_front_geometry_gpu.py):
//   bicubic, antialias 0:  s = scale (o + 0.5) - 0.5 (NOT clamped), i = floor(s), t = s - i; Keys' cubic convolution with A = -0.75 on the four taps
//                          i-1 .. i+2 at distances t+1, t, 1-t, 2-t; a tap outside the grid reads the nearest edge element (its weight moves there);
//   bilinear, antialias 0: s = max(scale (o + 0.5) - 0.5, 0), i = min(floor(s), g_in - 1), weights 1 - (s - i) on i and s - i on min(i + 1, g_in - 1);
//   antialias 1 (Pillow's scheme): centre c = scale (o + 0.5), support = h max(scale, 1) with h = 2 (bicubic) or 1 (bilinear), taps j from
//                          max(int(c - support + 0.5), 0) up to min(int(c + support + 0.5), g_in), weight f((j - c + 0.5) / max(scale, 1)) with f the cubic
//                          convolution with A = -0.5, or the triangle 1 - |x|; the weights of a window are divided by their sum, so a window cut by the
//                          border is renormalised, not padded.  (A = -0.5 here and -0.75 above: torch's two bicubics differ even when upsampling.)
// The two axes are separable in every mode.  Weights, products and sums are float64, the result is rounded to f32 once: half an ulp of the result, where
// torch's own f32 path is up to ~20 ulp of the table's largest element off its f64 path on these grids (it sums f32 products of f32 weights).
#include <cmath>

#include "common.h"

namespace {

constexpr int kMaxGrid = 64;

__device__ __forceinline__ double cubic_near(double x, double A) { return ((A + 2.0) * x - (A + 3.0)) * x * x + 1.0; }                // |x| <= 1
__device__ __forceinline__ double cubic_far(double x, double A) { return ((A * x - 5.0 * A) * x + 8.0 * A) * x - 4.0 * A; }          // 1 < |x| < 2

// the dense weight row w[0 .. g_in) of output index o along one axis, and the range [lo, hi) outside which it is zero
__device__ void axis_weights(int g_in, int g_out, int o, int filter, int antialias, double* w, int& lo, int& hi) {
    const double scale = (double)g_in / (double)g_out;
    for (int j = 0; j < g_in; ++j) w[j] = 0.0;
    if (antialias) {
        const double half = filter == LPI_POS_BILINEAR ? 1.0 : 2.0;
        const double support = scale >= 1.0 ? half * scale : half, inv = scale >= 1.0 ? 1.0 / scale : 1.0;
        const double c = scale * (o + 0.5);
        lo = max((int)(c - support + 0.5), 0);
        hi = min((int)(c + support + 0.5), g_in);
        double total = 0.0;
        for (int j = lo; j < hi; ++j) {
            const double x = fabs((j - c + 0.5) * inv);
            double f;
            if (filter == LPI_POS_BILINEAR) f = x < 1.0 ? 1.0 - x : 0.0;
            else f = x < 1.0 ? cubic_near(x, -0.5) : x < 2.0 ? cubic_far(x, -0.5) : 0.0;
            w[j] = f;
            total += f;
        }
        for (int j = lo; j < hi; ++j) w[j] /= total;
    } else if (filter == LPI_POS_BILINEAR) {
        const double s = fmax(scale * (o + 0.5) - 0.5, 0.0);
        const int i0 = min((int)s, g_in - 1), i1 = min(i0 + 1, g_in - 1);
        const double t = s - i0;
        w[i0] += 1.0 - t;
        w[i1] += t;
        lo = i0;
        hi = i1 + 1;
    } else {
        const double s = scale * (o + 0.5) - 0.5, fl = floor(s), t = s - fl, A = -0.75;
        const int i = (int)fl;
        const double c[4] = {cubic_far(t + 1.0, A), cubic_near(t, A), cubic_near(1.0 - t, A), cubic_far(2.0 - t, A)};
        for (int k = 0; k < 4; ++k) w[min(max(i - 1 + k, 0), g_in - 1)] += c[k];
        lo = min(max(i - 1, 0), g_in - 1);
        hi = min(max(i + 2, 0), g_in - 1) + 1;
    }
}

// block r writes row r of dst [1 + g_out^2, d]: row 0 (the class row) and, with copy != 0 (equal grids), every row is src's row as it is
__global__ __launch_bounds__(256) void pos_embed_resample_kernel(int g_in, int g_out, int d, const float* __restrict__ src, long lds, float* __restrict__ dst,
                                                                 long ldd, int filter, int antialias, int copy) {
    __shared__ double s_wy[kMaxGrid], s_wx[kMaxGrid];
    __shared__ int s_rng[4];
    const int r = blockIdx.x;
    float* out = dst + (size_t)r * ldd;
    if (r == 0 || copy) {
        const float* in = src + (size_t)r * lds;
        for (int col = threadIdx.x * 4; col < d; col += 1024) *reinterpret_cast<f32x4*>(out + col) = *reinterpret_cast<const f32x4*>(in + col);
        return;
    }
    const int oy = (r - 1) / g_out, ox = (r - 1) % g_out;
    if (threadIdx.x < 2) {      // thread 0: the vertical weights, thread 1: the horizontal ones
        int lo, hi;
        axis_weights(g_in, g_out, threadIdx.x ? ox : oy, filter, antialias, threadIdx.x ? s_wx : s_wy, lo, hi);
        s_rng[2 * threadIdx.x] = lo;
        s_rng[2 * threadIdx.x + 1] = hi;
    }
    __syncthreads();
    const int y0 = s_rng[0], y1 = s_rng[1], x0 = s_rng[2], x1 = s_rng[3];
    for (int col = threadIdx.x * 4; col < d; col += 1024) {
        double acc[4] = {0.0, 0.0, 0.0, 0.0};
        for (int iy = y0; iy < y1; ++iy) {
            double line[4] = {0.0, 0.0, 0.0, 0.0};
            for (int ix = x0; ix < x1; ++ix) {
                const f32x4 v = *reinterpret_cast<const f32x4*>(src + (size_t)(1 + iy * g_in + ix) * lds + col);
                const double wx = s_wx[ix];
#pragma unroll
                for (int j = 0; j < 4; ++j) line[j] += wx * (double)v[j];
            }
            const double wy = s_wy[iy];
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[j] += wy * line[j];
        }
        *reinterpret_cast<f32x4*>(out + col) = f32x4{(float)acc[0], (float)acc[1], (float)acc[2], (float)acc[3]};
    }
}

}  // namespace

extern "C" int lpi_pos_embed_resample(int g_in, int g_out, int d, const float* src, long lds, float* dst, long ldd, int filter, int antialias, void* stream) {
    if (g_in < 1 || g_in > kMaxGrid || g_out < 1 || g_out > kMaxGrid || d <= 0 || (d & 3) || lds < d || (lds & 3) || ldd < d || (ldd & 3)) return LPI_EINVAL;
    if (!src || !dst || ((uintptr_t)src & 15) || ((uintptr_t)dst & 15)) return LPI_EINVAL;
    if ((filter != LPI_POS_BICUBIC && filter != LPI_POS_BILINEAR) || (antialias != 0 && antialias != 1)) return LPI_EINVAL;
    // the footprints [first element, one past the last element of the last row) must not meet
    const uintptr_t s0 = (uintptr_t)src, s1 = s0 + ((uintptr_t)g_in * g_in * lds + d) * sizeof(float);
    const uintptr_t d0 = (uintptr_t)dst, d1 = d0 + ((uintptr_t)g_out * g_out * ldd + d) * sizeof(float);
    if (s0 < d1 && d0 < s1) return LPI_EINVAL;
    LPI_LAUNCH(pos_embed_resample_kernel, dim3(1 + g_out * g_out), dim3(256), 0, (hipStream_t)stream, g_in, g_out, d, src, lds, dst, ldd, filter, antialias,
               (int)(g_in == g_out));
    LPI_CHECK_LAST();
    return 0;
}
