// Decoded pixels -> the [B,3,S,S] uint8 batch of pixel_format='u8', on the GPU (pixel_format='decoded', lpi_amd/imageops.py).
//
// What it replaces: the host's crop(box).resize((rw, rh), BILINEAR) [+ window crop] [+ FLIP_LEFT_RIGHT] of the training / evaluation transforms
// (lpi_amd/retrieval/utils/data.py train_transform / test_transform) and their HWC -> CHW copy.  The output equals Pillow 12's byte for byte: the same
// coefficients (ImagingResample's precompute_coeffs in double, normalize_coeffs_8bpc to 22-bit fixed point), the horizontal pass rounded to a uint8
// intermediate, then the vertical pass on that intermediate.  The crop comes first, so the filter clamps at the crop's edges.
//
// Pillow's Image.resize runs the vertical pass first for crops more than 100 times taller than wide that it shrinks vertically: those images take a third
// launch, resample_vfirst_kernel (the other two skip them).
//
// Two launches (three with such an image):
//   resample_coeffs_kernel   per (image, axis, output position of the S-wide window): tap range and fixed-point taps -> workspace
//   resample_u8_kernel       per (image, band of R output rows, 256 of the 3*S (channel, column) items): every thread owns one (c, x) and R int32
//                            accumulators; it walks the band's source rows, computes its intermediate pixel of each row (horizontal taps straight from
//                            the source, L1/L2-cached) and adds it into the accumulators with the row's vertical taps, staged per chunk of YC source
//                            rows in LDS as a dense [R][YC] matrix (zero outside a row's taps).  LDS stays bounded whatever the downscale factor; the
//                            chunking is exact (integer sums, one rounding per intermediate pixel, as Pillow).  No overflow: bilinear taps are >= 0 and
//                            sum to 2^22 (+- rounding), so a sum stays below 256 * 2^22 + 2^21 < 2^31.
#include <cmath>

#include "common.h"

namespace {

constexpr int RB = 16;          // output rows per workgroup
constexpr int YC = 64;          // source rows per LDS chunk of vertical taps
constexpr int PREC = 22;        // Pillow's PRECISION_BITS (32 - 8 - 2)

// descriptor fields (include/lpi_hip.h LPI_RESAMPLE_DESC)
enum { D_OFF, D_W, D_H, D_X0, D_Y0, D_X1, D_Y1, D_RW, D_RH, D_OX, D_OY, D_FLIP };

// Pillow's ksize for one axis: (int)ceil(support) * 2 + 1, support = filterscale = max(in / out, 1)
long ksize_of(long in, long out) {
    double scale = (double)in / (double)out;
    double support = scale < 1.0 ? 1.0 : scale;
    return (long)std::ceil(support) * 2 + 1;
}

// Workspace: the validated descriptor table (copied there by lpi_image_resample_u8 itself, so the kernels never read a table the host did not check),
// padded to 256 bytes, then per image an int32 block: [S][2] x bounds, [S][KX] x taps, [S][2] y bounds, [S][KY] y taps
inline long desc_bytes(int B) { return ((long)B * LPI_RESAMPLE_DESC * 8 + 255) / 256 * 256; }
__host__ __device__ inline long image_ints(int S, int KX, int KY) { return (long)S * (4 + KX + KY); }

// The coefficient arithmetic is Pillow's, operation by operation: hipcc contracts device double arithmetic into v_fma_f64 by default (center - support
// + 0.5 would round once instead of twice), hence fp contract(off) in both functions; IEEE division (no fast-math for this file).
__device__ inline double bilinear_filter(double x) {
#pragma clang fp contract(off)
    if (x < 0.0) x = -x;
    if (x < 1.0) return 1.0 - x;
    return 0.0;
}

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
    const double support = 1.0 * filterscale;
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
    for (int x = 0; x < xmax; ++x) ww += bilinear_filter((x + xmin - center + 0.5) * ss);
    for (int x = 0; x < xmax; ++x) {
        double k = bilinear_filter((x + xmin - center + 0.5) * ss);
        if (ww != 0.0) k /= ww;
        kk[x] = k < 0 ? (int)(-0.5 + k * (1 << PREC)) : (int)(0.5 + k * (1 << PREC));
    }
    bounds[0] = xmin;
    bounds[1] = xmax;
}

__device__ inline int clip8(int s) {
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

    int acc[RB];
#pragma unroll
    for (int r = 0; r < RB; ++r) acc[r] = 1 << (PREC - 1);

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
                int s = 1 << (PREC - 1);
                for (int t = 0; t < nx; ++t) s += (int)p[3 * t] * kxp[t];
                const int v = clip8(s);
#pragma unroll
                for (int r = 0; r < RB; ++r) acc[r] += v * ky_s[r][y - yc];
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
    int s = 1 << (PREC - 1);
    for (int t = 0; t < nx; ++t) {
        int v = 1 << (PREC - 1);
        for (int y = 0; y < ny; ++y) v += (int)p0[(long)y * w * 3 + 3 * t] * ky[y];
        s += clip8(v) * kxp[t];
    }
    const int xo = d[D_FLIP] ? S - 1 - x : x;
    out[(((long)b * 3 + c) * S + r) * S + xo] = (uint8_t)clip8(s);
}

// validates the host copy of the descriptors; the tap-table strides and the workspace size
int plan(int B, int S, const long* desc, long src_bytes, int* KX, int* KY, long* bytes, bool* any_vfirst = nullptr) {
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
        const long a = ksize_of(d[D_X1] - d[D_X0], d[D_RW]), e = ksize_of(d[D_Y1] - d[D_Y0], d[D_RH]);
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

extern "C" int lpi_image_resample_workspace(int B, int S, const long* desc, long* bytes) {
    int kx = 0, ky = 0;
    if (!bytes) return LPI_EINVAL;
    return plan(B, S, desc, -1, &kx, &ky, bytes);
}

extern "C" int lpi_image_resample_u8(int B, int S, const long* desc, const void* src, long src_bytes, void* ws, long ws_bytes, void* out, void* stream) {
    int kx = 0, ky = 0;
    long need = 0;
    bool vfirst = false;
    if (!src || !ws || !out || src_bytes < 1) return LPI_EINVAL;
    const int rc = plan(B, S, desc, src_bytes, &kx, &ky, &need, &vfirst);
    if (rc != 0) return rc;
    if (ws_bytes < need) return LPI_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    // the kernels read the table the host just validated: copied into the workspace's head on the stream (from pageable memory the copy has read
    // `desc` when it returns; from pinned memory the caller keeps it unchanged until the stream has passed the copy)
    const long* desc_dev = static_cast<const long*>(ws);
    int* taps = reinterpret_cast<int*>(static_cast<char*>(ws) + desc_bytes(B));
    const hipError_t e = hipMemcpyAsync(ws, desc, (size_t)B * LPI_RESAMPLE_DESC * 8, hipMemcpyHostToDevice, s);
    if (e != hipSuccess) return (int)e;
    LPI_LAUNCH(resample_coeffs_kernel, dim3((S + 255) / 256, B, 2), dim3(256), 0, s, desc_dev, S, kx, ky, taps);
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
