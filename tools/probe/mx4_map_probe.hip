// Diagnostic: the operand map of v_mfma_scale_f32_16x16x128_f8f6f4 with FP4 (e2m1) operands (cbsz = blgp = 4), measured the way gemm_mx8.hip's FP8 map
// was.  One wave, one instruction per launch.  W [16, 128] and X [16, 128] hold random integer-valued nibbles (0, +-1, 2, 3, 4, 6) and a random E8M0
// scale in 125 .. 129 per (row, 32-block), so D[i][j] = sum_k W[i][k] sw[i][k / 32] X[j][k] sx[j][k / 32] is exact in f32 in every summation order and no
// two layouts give the same D.  The host packs the lane registers under every combination of
//   K map    c: lane (row r = l & 15, group g = l >> 4) holds elements 32 g .. 32 g + 31        s: 16 g .. + 15 and 64 + 16 g .. + 15 (the FP8 map, halved)
//   nibbles  l: element 2 j in the low nibble of byte j                                        h: in the high nibble
//   scales   g: block b of row r in byte `opsel` of lane r + 16 b's register                   r: block b in byte b of lane r's register (opsel unused)
// with the other bytes of every scale register holding a wrong scale, runs the instruction (opsel 0 / 0, then 2 / 1), and prints which combination
// reproduces the host's D bit for bit.  A product of two FP4 operands packed alike cannot see the nibble order (the two nibbles of a byte are two k-values
// of the same block, and a sum does not care which comes first): both nibble orders must match, which shows that nibble positions pair with each other and
// leaves the order to the format (include/lpi_hip.h: element 2 j in the low nibble).  Output: D[i = 4 (l >> 4) + e][j = l & 15] in register e of lane l, first operand = rows i (the FP8 layout).
//   hipcc --offload-arch=gfx950 -O2 tools/probe/mx4_map_probe.hip -o tools/probe/bin/mx4_map_probe
#include <hip/hip_runtime.h>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cmath>
typedef __attribute__((ext_vector_type(8))) int i32x8;
typedef __attribute__((ext_vector_type(4))) float f32x4;

template <int OA, int OB>
__global__ __launch_bounds__(64) void one_mma(const uint32_t* __restrict__ w, const uint32_t* __restrict__ x, const uint32_t* __restrict__ sw,
                                              const uint32_t* __restrict__ sx, float* __restrict__ d)
{
    const int l = threadIdx.x;
    i32x8 a = {(int)w[l * 4], (int)w[l * 4 + 1], (int)w[l * 4 + 2], (int)w[l * 4 + 3], 0, 0, 0, 0};
    i32x8 b = {(int)x[l * 4], (int)x[l * 4 + 1], (int)x[l * 4 + 2], (int)x[l * 4 + 3], 0, 0, 0, 0};
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    acc = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(a, b, acc, 4, 4, OA, (int)sw[l], OB, (int)sx[l]);
    for (int e = 0; e < 4; ++e) d[l * 4 + e] = acc[e];
}

static const float GRID[8] = {0.f, 0.5f, 1.f, 1.5f, 2.f, 3.f, 4.f, 6.f};
static const int INT_CODES[11] = {0, 2, 4, 5, 6, 7, 10, 12, 13, 14, 15};      // 0, 1, 2, 3, 4, 6 and the negatives
static float decode(int c) { return (c & 8 ? -1.f : 1.f) * GRID[c & 7]; }

struct Mat { int code[16][128]; int sc[16][4]; };

static void pack(const Mat& m, int kmap, int nib, int smap, int opsel, uint32_t* regs, uint32_t* sreg)
{
    for (int l = 0; l < 64; ++l) {
        const int r = l & 15, g = l >> 4;
        uint8_t bytes[16] = {0};
        for (int p = 0; p < 32; ++p) {
            const int k = kmap == 0 ? 32 * g + p : (p < 16 ? 16 * g + p : 64 + 16 * g + p - 16);
            const int hi = nib == 0 ? (p & 1) : !(p & 1);
            bytes[p >> 1] |= (uint8_t)(m.code[r][k] << (hi ? 4 : 0));
        }
        for (int q = 0; q < 4; ++q) regs[l * 4 + q] = bytes[4 * q] | bytes[4 * q + 1] << 8 | bytes[4 * q + 2] << 16 | (uint32_t)bytes[4 * q + 3] << 24;
        uint32_t s = 0x78787878u;      // 120 = 2^-7 in every byte that should not be read
        if (smap == 0) { s &= ~(0xFFu << (8 * opsel)); s |= (uint32_t)m.sc[r][g] << (8 * opsel); }
        else s = m.sc[r][0] | m.sc[r][1] << 8 | m.sc[r][2] << 16 | (uint32_t)m.sc[r][3] << 24;
        sreg[l] = s;
    }
}

#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { printf("HIP error %s at line %d\n", hipGetErrorString(e_), __LINE__); return 2; } } while (0)

int main()
{
    srand(12345);
    Mat W, X;
    for (Mat* m : {&W, &X})
        for (int r = 0; r < 16; ++r) {
            for (int k = 0; k < 128; ++k) m->code[r][k] = INT_CODES[rand() % 11];
            for (int b = 0; b < 4; ++b) m->sc[r][b] = 125 + rand() % 5;
        }
    double D[16][16];
    for (int i = 0; i < 16; ++i)
        for (int j = 0; j < 16; ++j) {
            double s = 0;
            for (int k = 0; k < 128; ++k)
                s += (double)decode(W.code[i][k]) * ldexp(1.0, W.sc[i][k / 32] - 127) * decode(X.code[j][k]) * ldexp(1.0, X.sc[j][k / 32] - 127);
            D[i][j] = s;
        }
    uint32_t *dw, *dx, *dsw, *dsx;
    float* dd;
    CK(hipMalloc(&dw, 1024)); CK(hipMalloc(&dx, 1024)); CK(hipMalloc(&dsw, 256)); CK(hipMalloc(&dsx, 256)); CK(hipMalloc(&dd, 1024));
    int found = 0;
    for (int pass = 0; pass < 2; ++pass) {
        const int oa = pass ? 2 : 0, ob = pass ? 1 : 0;
        for (int kmap = 0; kmap < 2; ++kmap)
            for (int nib = 0; nib < 2; ++nib)
                for (int smap = 0; smap < 2; ++smap) {
                    uint32_t hw[256], hx[256], hsw[64], hsx[64];
                    float hd[256];
                    pack(W, kmap, nib, smap, oa, hw, hsw);
                    pack(X, kmap, nib, smap, ob, hx, hsx);
                    CK(hipMemcpy(dw, hw, 1024, hipMemcpyHostToDevice)); CK(hipMemcpy(dx, hx, 1024, hipMemcpyHostToDevice));
                    CK(hipMemcpy(dsw, hsw, 256, hipMemcpyHostToDevice)); CK(hipMemcpy(dsx, hsx, 256, hipMemcpyHostToDevice));
                    if (pass) one_mma<2, 1><<<1, 64>>>(dw, dx, dsw, dsx, dd);
                    else one_mma<0, 0><<<1, 64>>>(dw, dx, dsw, dsx, dd);
                    CK(hipGetLastError());
                    CK(hipDeviceSynchronize());
                    CK(hipMemcpy(hd, dd, 1024, hipMemcpyDeviceToHost));
                    int bad = 0;
                    double worst = 0;
                    for (int l = 0; l < 64; ++l)
                        for (int e = 0; e < 4; ++e) {
                            const double want = D[4 * (l >> 4) + e][l & 15], err = fabs((double)hd[l * 4 + e] - want);
                            bad += err != 0;
                            if (err > worst) worst = err;
                        }
                    printf("opsel %d/%d  K map %c  nibbles %c  scales %c : %3d of 256 differ, worst %.6g%s\n", oa, ob, "cs"[kmap], "lh"[nib], "gr"[smap], bad,
                           worst, bad ? "" : "   <== MATCH");
                    found += !bad;
                }
    }
    printf("%d matching combinations (4 expected: one K map and one scale map, either nibble order, both opsel passes)\n", found);
    return 0;
}
