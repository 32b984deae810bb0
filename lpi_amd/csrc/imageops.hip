// Decoded pixels -> the [B,3,S,S] uint8 batch of pixel_format='u8', on the GPU (pixel_format='decoded', lpi_amd/imageops.py).
//
// What it replaces: the host's crop(box).resize((rw, rh), FILTER) [+ window crop] [+ FLIP_LEFT_RIGHT] of the training / evaluation transforms
// (lpi_amd/retrieval/utils/data.py train_transform / test_transform) and their HWC -> CHW copy, FILTER = BILINEAR (the reference's retrieval loader),
// BICUBIC (CLIP's own preprocessing) or BOX.  The output equals Pillow 12's byte for byte: the same coefficients (ImagingResample's precompute_coeffs
// in double with the filter's function and support, normalize_coeffs_8bpc to 22-bit fixed point), the horizontal pass rounded to a uint8
// intermediate, then the vertical pass on that intermediate.  The crop comes first, so the filter clamps at the crop's edges.  The filter is per
// call and only the coefficient kernel knows it: the resample kernels read taps from the workspace, whichever filter made them.
//
// Pillow's Image.resize runs the vertical pass first for crops more than 100 times taller than wide that it shrinks vertically (whatever the
// filter): those images take a third launch, resample_vfirst_kernel (the other two skip them).
//
// Two launches (three with such an image):
//   resample_coeffs_kernel   per (image, axis, output position of the S-wide window): tap range and fixed-point taps -> workspace
//   resample_u8_kernel       per (image, band of R output rows, 256 of the 3*S (channel, column) items): every thread owns one (c, x) and R 32-bit
//                            accumulators; it walks the band's source rows, computes its intermediate pixel of each row (horizontal taps straight from
//                            the source, L1/L2-cached) and adds it into the accumulators with the row's vertical taps, staged per chunk of YC source
//                            rows in LDS as a dense [R][YC] matrix (zero outside a row's taps).  LDS stays bounded whatever the downscale factor; the
//                            chunking is exact (integer sums, one rounding per intermediate pixel, as Pillow).
//
// Signed taps and the 32-bit sums.  Bicubic taps are negative on part of their support, so "every partial sum is below the whole sum" no longer
// holds.  Two arguments, the first unconditional:
//   (1) Every sum here is accumulated in uint32_t and read as int32 once, at clip8.  Addition modulo 2^32 is associative and commutative, so the
//       chunks of YC rows, in any order and for any YC, give exactly the bits of Pillow's sequential `int ss` loop; no signed addition is executed,
//       so no partial sum can overflow in the language's sense.
//   (2) The value never wraps either.  Let T = sum |tap| of one output position.  Every partial sum over ANY subset of the taps is within
//       2^21 + 255 * T of zero, which stays inside int32 while T <= (2^31 - 2^21) / 255 = 2.0059 * 2^22.  A tap is round(2^22 * w_i / W), W = sum
//       w_i, so T <= 2^22 * (P + N) / (P - N) + K / 2, P / N the sums of the positive / negative weights' magnitudes and K the number of nonzero
//       taps.  BOX and BILINEAR: N = 0, T <= 2^22 + K / 2.  BICUBIC, f = Pillow's bicubic_filter (a = -0.5), samples f(u_j), u_j spaced 1 / filterscale:
//       - filterscale = 1 (no shrink): at most four samples, the Catmull-Rom weights of a phase t in [0, 1): the negative ones are -(t - 2t^2 +
//         t^3) / 2 and -(t^2 - t^3) / 2, N <= (t - t^2) / 2 <= 1/8.  The window always holds the sample nearest the centre (center lies inside
//         (0, in), so clamping at an edge never removes it), whose weight is >= f(1/2) = 9/16: P >= 9/16 with or without clamped edges, and
//         (P + N) / (P - N) <= (11/16) / (7/16) = 11/7 = 1.5715.
//       - filterscale = m > 1: the samples are a lattice of spacing 1 / m; |f| <= 2/27 on the negative lobes 1 < |u| < 2, whose integrals are 1/24
//         each, and f is unimodal on each lobe, so N <= m / 12 + 4/27; clamping at an edge removes samples from one end of the lattice only, and
//         the centre's distance to an edge is >= m / 2 source pixels, so a negative lobe is present only together with the whole positive half
//         [0, 1] (integral 13/24) on its side: P >= 13 m / 24 - 1 per present side.  For m >= 3 this gives N / P <= 0.318 and (P + N) / (P - N)
//         <= 1.94; towards large m it tends to the integrals' (7/6) / 1 = 1.1667.  For 1 < m < 3 the lattice has at most 3 samples per negative
//         lobe and the unimodal bounds are too coarse to close the gap by hand: tests/test_image_filters_host.py sweeps that range (every
//         in, out <= 64 pair and a dense set of larger ones, every output position, clamped edges included) and asserts 255 * T + 2^21 < 2^31
//         for each; the largest T it meets is 1.269 * 2^22 (255 * T + 2^21 = 1.36e9), at an interior position of the slight shrink 14 -> 13.
//       K / 2 matters only for sources of millions of pixels a side (every |tap| < 1/2 rounds to zero): there (1) alone carries the equality, as
//       it does in Pillow's own loop.
#include <cmath>

#include "common.h"

namespace {

constexpr int RB = 16;          // output rows per workgroup
constexpr int YC = 64;          // source rows per LDS chunk of vertical taps
constexpr int PREC = 22;        // Pillow's PRECISION_BITS (32 - 8 - 2)

// descriptor fields (include/lpi_hip.h LPI_RESAMPLE_DESC)
enum { D_OFF, D_W, D_H, D_X0, D_Y0, D_X1, D_Y1, D_RW, D_RH, D_OX, D_OY, D_FLIP };

// Pillow's filter support (BOX 0.5, BILINEAR 1, BICUBIC 2); 0 for a filter this file does not restate
__host__ __device__ constexpr double filter_support(int filter) {
    return filter == LPI_FILTER_BOX ? 0.5 : filter == LPI_FILTER_BILINEAR ? 1.0 : filter == LPI_FILTER_BICUBIC ? 2.0 : 0.0;
}

// Pillow's ksize for one axis: (int)ceil(support) * 2 + 1, support = filter support * filterscale, filterscale = max(in / out, 1)
long ksize_of(int filter, long in, long out) {
    double scale = (double)in / (double)out;
    double filterscale = scale < 1.0 ? 1.0 : scale;
    double support = filter_support(filter) * filterscale;
    return (long)std::ceil(support) * 2 + 1;
}

// Workspace: the validated descriptor table (copied there by lpi_image_resample_u8 itself, so the kernels never read a table the host did not check),
// padded to 256 bytes, then per image an int32 block: [S][2] x bounds, [S][KX] x taps, [S][2] y bounds, [S][KY] y taps
inline long desc_bytes(int B) { return ((long)B * LPI_RESAMPLE_DESC * 8 + 255) / 256 * 256; }
__host__ __device__ inline long image_ints(int S, int KX, int KY) { return (long)S * (4 + KX + KY); }

// The coefficient arithmetic is Pillow's, operation by operation: hipcc contracts device double arithmetic into v_fma_f64 by default (center - support
// + 0.5 would round once instead of twice), hence fp contract(off) in every function; IEEE division (no fast-math for this file).  The filter is a
// template parameter: each instantiation holds one filter function inline, so no filter pays for another's branches.
__device__ inline double bilinear_filter(double x) {
#pragma clang fp contract(off)
    if (x < 0.0) x = -x;
    if (x < 1.0) return 1.0 - x;
    return 0.0;
}

// Pillow's bicubic_filter (a = -0.5), in its association order
__device__ inline double bicubic_filter(double x) {
#pragma clang fp contract(off)
    const double a = -0.5;
    if (x < 0.0) x = -x;
    if (x < 1.0) return ((a + 2.0) * x - (a + 3.0)) * x * x + 1;
    if (x < 2.0) return (((x - 5) * x + 8) * x - 4) * a;
    return 0.0;
}

__device__ inline double box_filter(double x) {
    if (x > -0.5 && x <= 0.5) return 1.0;
    return 0.0;
}

template <int F>
__device__ inline double filter_fn(double x) {
    if constexpr (F == LPI_FILTER_BICUBIC) return bicubic_filter(x);
    else if constexpr (F == LPI_FILTER_BOX) return box_filter(x);
    else return bilinear_filter(x);
}

template <int F>
__global__ __launch_bounds__(256) void resample_coeffs_kernel(const long* __restrict__ desc, int S, int KX, int KY, int* __restrict__ ws) {
#pragma clang fp contract(off)
    const int o = blockIdx.x * 256 + threadIdx.x;
    const int b = blockIdx.y, axis = blockIdx.z;
    if (o >= S) return;
    const long* d = desc + (long)b * LPI_RESAMPLE_DESC;
    const int in = axis ? (int)(d[D_Y1] - d[D_Y0]) : (int)(d[D_X1] - d[D_X0]);
    const int out = axis ? (int)d[D_RH] : (int)d[D_RW];
    const int first = axis ? (int)d[D_OY] : (int)d[D_OX];
    const int K = axis ? KY : KX;
    int* base = ws + (long)b * image_ints(S, KX, KY) + (axis ? (long)S * (2 + KX) : 0);
    int* bounds = base + 2 * o;
    int* kk = base + 2L * S + (long)o * K;

    const double scale = (double)in / out;
    const double filterscale = scale < 1.0 ? 1.0 : scale;
    const double support = filter_support(F) * filterscale;
    const double ss = 1.0 / filterscale;
    const int xx = first + o;
    const double center = (xx + 0.5) * scale;
    int xmin = (int)(center - support + 0.5);
    if (xmin < 0) xmin = 0;
    int xmax = (int)(center + support + 0.5);
    if (xmax > in) xmax = in;
    xmax -= xmin;
    if (xmax > K) xmax = K;         // cannot happen (xmax <= ceil(support) * 2 + 1): keeps the writes inside the block regardless
    double ww = 0.0;
    for (int x = 0; x < xmax; ++x) ww += filter_fn<F>((x + xmin - center + 0.5) * ss);
    for (int x = 0; x < xmax; ++x) {
        double k = filter_fn<F>((x + xmin - center + 0.5) * ss);
        if (ww != 0.0) k /= ww;
        kk[x] = k < 0 ? (int)(-0.5 + k * (1 << PREC)) : (int)(0.5 + k * (1 << PREC));
    }
    bounds[0] = xmin;
    bounds[1] = xmax;
}

// the sums are uint32_t (header, "Signed taps"): read as int32 here, once
__device__ inline int clip8(uint32_t u) {
    int s = (int)u;
    s >>= PREC;
    return s < 0 ? 0 : (s > 255 ? 255 : s);
}

// Pillow 12's Image.resize runs the vertical pass FIRST for a crop more than 100 times taller than wide that it shrinks vertically (two one-axis resizes);
// such images take resample_vfirst_kernel instead
__host__ __device__ inline bool vertical_first(long cw, long ch, long rh) { return ch > cw * 100 && rh < ch; }

__global__ __launch_bounds__(256) void resample_u8_kernel(const long* __restrict__ desc, int S, int KX, int KY, const int* __restrict__ ws,
                                                          const uint8_t* __restrict__ src, uint8_t* __restrict__ out) {
    __shared__ int ky_s[RB][YC];
    __shared__ int yb_s[RB][2];
    const int tid = threadIdx.x;
    const int item = blockIdx.x * 256 + tid;
    const int r0 = blockIdx.y * RB;
    const int b = blockIdx.z;
    const int nr = S - r0 < RB ? S - r0 : RB;
    const long* d = desc + (long)b * LPI_RESAMPLE_DESC;
    if (vertical_first(d[D_X1] - d[D_X0], d[D_Y1] - d[D_Y0], d[D_RH])) return;        // uniform per workgroup: before any barrier
    const int* wsb = ws + (long)b * image_ints(S, KX, KY);
    const int* xb = wsb;
    const int* kx = wsb + 2L * S;
    const int* yb = wsb + (long)S * (2 + KX);
    const int* ky = yb + 2L * S;

    if (tid < RB) {
        yb_s[tid][0] = tid < nr ? yb[2 * (r0 + tid)] : 0;
        yb_s[tid][1] = tid < nr ? yb[2 * (r0 + tid) + 1] : 0;
    }
    __syncthreads();
    int ylo = 0x7fffffff, yhi = 0;
    for (int r = 0; r < nr; ++r) {
        ylo = yb_s[r][0] < ylo ? yb_s[r][0] : ylo;
        yhi = yb_s[r][0] + yb_s[r][1] > yhi ? yb_s[r][0] + yb_s[r][1] : yhi;
    }

    const bool valid = item < 3 * S;
    const int c = valid ? item / S : 0, x = valid ? item % S : 0;
    const int xmin = xb[2 * x], nx = xb[2 * x + 1];
    const int* kxp = kx + (long)x * KX;
    const long w = d[D_W];
    // this thread's first source byte of crop row 0: pixel (x0 + xmin, y0), channel c
    const uint8_t* col = src + d[D_OFF] + ((long)d[D_Y0] * w + d[D_X0] + xmin) * 3 + c;

    uint32_t acc[RB];
#pragma unroll
    for (int r = 0; r < RB; ++r) acc[r] = 1u << (PREC - 1);

    for (int yc = ylo; yc < yhi; yc += YC) {
        __syncthreads();            // the previous chunk's taps are consumed
        for (int j = tid; j < RB * YC; j += 256) {
            const int r = j / YC, t = yc + j % YC - yb_s[r][0];
            ky_s[r][j % YC] = (r < nr && t >= 0 && t < yb_s[r][1]) ? ky[(long)(r0 + r) * KY + t] : 0;
        }
        __syncthreads();
        if (valid) {
            const int yend = yc + YC < yhi ? yc + YC : yhi;
            for (int y = yc; y < yend; ++y) {
                const uint8_t* p = col + (long)y * w * 3;
                uint32_t s = 1u << (PREC - 1);
                for (int t = 0; t < nx; ++t) s += (uint32_t)p[3 * t] * (uint32_t)kxp[t];
                const uint32_t v = (uint32_t)clip8(s);
#pragma unroll
                for (int r = 0; r < RB; ++r) acc[r] += v * (uint32_t)ky_s[r][y - yc];
            }
        }
    }
    if (!valid) return;
    const int xo = d[D_FLIP] ? S - 1 - x : x;
    uint8_t* o = out + (((long)b * 3 + c) * S + r0) * S + xo;
#pragma unroll
    for (int r = 0; r < RB; ++r)
        if (r < nr) o[(long)r * S] = (uint8_t)clip8(acc[r]);
}

// The vertical-first order, one thread per output byte (c, x) of row blockIdx.y: for each horizontal tap column, the vertical sum over the row's taps
// rounded to uint8 (Pillow's intermediate), then the horizontal sum of those.  Only images of that aspect (rare) do any work here.
__global__ __launch_bounds__(256) void resample_vfirst_kernel(const long* __restrict__ desc, int S, int KX, int KY, const int* __restrict__ ws,
                                                              const uint8_t* __restrict__ src, uint8_t* __restrict__ out) {
    const int item = blockIdx.x * 256 + threadIdx.x;
    const int r = blockIdx.y, b = blockIdx.z;
    const long* d = desc + (long)b * LPI_RESAMPLE_DESC;
    if (!vertical_first(d[D_X1] - d[D_X0], d[D_Y1] - d[D_Y0], d[D_RH]) || item >= 3 * S) return;
    const int* wsb = ws + (long)b * image_ints(S, KX, KY);
    const int* xb = wsb;
    const int* kx = wsb + 2L * S;
    const int* yb = wsb + (long)S * (2 + KX);
    const int* ky = yb + 2L * S + (long)r * KY;
    const int c = item / S, x = item % S;
    const int xmin = xb[2 * x], nx = xb[2 * x + 1];
    const int ymin = yb[2 * r], ny = yb[2 * r + 1];
    const int* kxp = kx + (long)x * KX;
    const long w = d[D_W];
    const uint8_t* p0 = src + d[D_OFF] + ((d[D_Y0] + ymin) * w + d[D_X0] + xmin) * 3 + c;
    uint32_t s = 1u << (PREC - 1);
    for (int t = 0; t < nx; ++t) {
        uint32_t v = 1u << (PREC - 1);
        for (int y = 0; y < ny; ++y) v += (uint32_t)p0[(long)y * w * 3 + 3 * t] * (uint32_t)ky[y];
        s += (uint32_t)clip8(v) * (uint32_t)kxp[t];
    }
    const int xo = d[D_FLIP] ? S - 1 - x : x;
    out[(((long)b * 3 + c) * S + r) * S + xo] = (uint8_t)clip8(s);
}

// validates the host copy of the descriptors; the tap-table strides and the workspace size
int plan(int filter, int B, int S, const long* desc, long src_bytes, int* KX, int* KY, long* bytes, bool* any_vfirst = nullptr) {
    if (filter != LPI_FILTER_BILINEAR && filter != LPI_FILTER_BICUBIC && filter != LPI_FILTER_BOX) return LPI_EINVAL;
    if (B < 1 || B > 65535 || S < 1 || S > LPI_RESAMPLE_MAX_SIZE || !desc) return LPI_EINVAL;
    bool vf = false;
    long kx = 1, ky = 1;
    for (int i = 0; i < B; ++i) {
        const long* d = desc + (long)i * LPI_RESAMPLE_DESC;
        const long w = d[D_W], h = d[D_H];
        if (w < 1 || h < 1 || w > LPI_RESAMPLE_MAX_SIDE || h > LPI_RESAMPLE_MAX_SIDE || d[D_OFF] < 0) return LPI_EINVAL;
        if (src_bytes >= 0 && d[D_OFF] > src_bytes - w * h * 3) return LPI_EINVAL;
        if (!(0 <= d[D_X0] && d[D_X0] < d[D_X1] && d[D_X1] <= w && 0 <= d[D_Y0] && d[D_Y0] < d[D_Y1] && d[D_Y1] <= h)) return LPI_EINVAL;
        if (d[D_RW] < 1 || d[D_RH] < 1 || d[D_RW] > LPI_RESAMPLE_MAX_SIDE || d[D_RH] > LPI_RESAMPLE_MAX_SIDE) return LPI_EINVAL;
        if (d[D_OX] < 0 || d[D_OX] > d[D_RW] - S || d[D_OY] < 0 || d[D_OY] > d[D_RH] - S) return LPI_EINVAL;
        if (d[D_FLIP] != 0 && d[D_FLIP] != 1) return LPI_EINVAL;
        const long a = ksize_of(filter, d[D_X1] - d[D_X0], d[D_RW]), e = ksize_of(filter, d[D_Y1] - d[D_Y0], d[D_RH]);
        kx = a > kx ? a : kx;
        ky = e > ky ? e : ky;
        vf = vf || vertical_first(d[D_X1] - d[D_X0], d[D_Y1] - d[D_Y0], d[D_RH]);
    }
    if (any_vfirst) *any_vfirst = vf;
    if ((long)B * image_ints(S, (int)kx, (int)ky) > (1L << 40)) return LPI_EINVAL;      // a 4 TiB workspace: not a real request
    *KX = (int)kx;
    *KY = (int)ky;
    *bytes = desc_bytes(B) + (long)B * image_ints(S, (int)kx, (int)ky) * 4;
    return 0;
}

}  // namespace

extern "C" int lpi_image_resample_workspace_f(int filter, int B, int S, const long* desc, long* bytes) {
    int kx = 0, ky = 0;
    if (!bytes) return LPI_EINVAL;
    return plan(filter, B, S, desc, -1, &kx, &ky, bytes);
}

extern "C" int lpi_image_resample_u8_f(int filter, int B, int S, const long* desc, const void* src, long src_bytes, void* ws, long ws_bytes, void* out,
                                       void* stream) {
    int kx = 0, ky = 0;
    long need = 0;
    bool vfirst = false;
    if (!src || !ws || !out || src_bytes < 1) return LPI_EINVAL;
    const int rc = plan(filter, B, S, desc, src_bytes, &kx, &ky, &need, &vfirst);      // an unknown filter ends here: before any copy or launch
    if (rc != 0) return rc;
    if (ws_bytes < need) return LPI_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    // the kernels read the table the host just validated: copied into the workspace's head on the stream (from pageable memory the copy has read
    // `desc` when it returns; from pinned memory the caller keeps it unchanged until the stream has passed the copy)
    const long* desc_dev = static_cast<const long*>(ws);
    int* taps = reinterpret_cast<int*>(static_cast<char*>(ws) + desc_bytes(B));
    const hipError_t e = hipMemcpyAsync(ws, desc, (size_t)B * LPI_RESAMPLE_DESC * 8, hipMemcpyHostToDevice, s);
    if (e != hipSuccess) return (int)e;
    const dim3 cgrid((S + 255) / 256, B, 2);
    if (filter == LPI_FILTER_BICUBIC) {
        LPI_LAUNCH(resample_coeffs_kernel<LPI_FILTER_BICUBIC>, cgrid, dim3(256), 0, s, desc_dev, S, kx, ky, taps);
    } else if (filter == LPI_FILTER_BOX) {
        LPI_LAUNCH(resample_coeffs_kernel<LPI_FILTER_BOX>, cgrid, dim3(256), 0, s, desc_dev, S, kx, ky, taps);
    } else {
        LPI_LAUNCH(resample_coeffs_kernel<LPI_FILTER_BILINEAR>, cgrid, dim3(256), 0, s, desc_dev, S, kx, ky, taps);
    }
    LPI_CHECK_LAST();
    LPI_LAUNCH(resample_u8_kernel, dim3((3 * S + 255) / 256, (S + RB - 1) / RB, B), dim3(256), 0, s, desc_dev, S, kx, ky, (const int*)taps,
               (const uint8_t*)src, (uint8_t*)out);
    LPI_CHECK_LAST();
    if (vfirst) {
        LPI_LAUNCH(resample_vfirst_kernel, dim3((3 * S + 255) / 256, S, B), dim3(256), 0, s, desc_dev, S, kx, ky, (const int*)taps, (const uint8_t*)src,
                   (uint8_t*)out);
        LPI_CHECK_LAST();
    }
    return 0;
}

// the entry points of ABI <= 606: the bilinear case
extern "C" int lpi_image_resample_workspace(int B, int S, const long* desc, long* bytes) {
    return lpi_image_resample_workspace_f(LPI_FILTER_BILINEAR, B, S, desc, bytes);
}

extern "C" int lpi_image_resample_u8(int B, int S, const long* desc, const void* src, long src_bytes, void* ws, long ws_bytes, void* out, void* stream) {
    return lpi_image_resample_u8_f(LPI_FILTER_BILINEAR, B, S, desc, src, src_bytes, ws, ws_bytes, out, stream);
}
