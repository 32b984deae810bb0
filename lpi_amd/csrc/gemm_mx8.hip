// NT GEMM on MX-FP8 operands (gfx950 block-scaled matrix instruction):  C[M,N] = epi(alpha * A[M,K] . B[N,K]^T + bias) + residual
//
// replaces, in the no-grad forwards of EngineOptions.mx8_forward: the in_proj / out_proj / c_fc / c_proj projections of a full block
// (retrieval/models/clip/model.py:172-177 of the reference).
//
// A and B are OCP e4m3fn bytes with one E8M0 scale byte per 32 consecutive K elements ([rows, K/32] row-major with a leading dimension; mx8.h has the
// format), multiplied by v_mfma_scale_f32_16x16x128_f8f6f4 with f32 accumulation.
//
// Structure: the 128x128 tile of gemm.hip with one-byte elements —
//  * 4 waves as 2x2, each 64x64 = 4x4 tiles of 16x16 (64 accumulator VGPRs); a staged tile row is 128 bytes = 128 elements = ONE instruction's K, so a K
//    step is 16 matrix instructions per wave;
//  * global -> LDS by global_load_lds_dwordx4, double buffered, one barrier per K step, the same chunk ^ ((row >> 1) & 7) swizzle on the source address
//    and on the ds_read_b128;
//  * operand map of the instruction (measured on the hardware with one-lane-group operands and per-group scales; the 16x16x64 map twice): lane l holds
//    row (l & 15) and, with g = l >> 4, K elements 16 g .. 16 g + 15 in its first four registers and 64 + 16 g .. 64 + 16 g + 15 in the other four — NOT
//    32 consecutive elements — while the scale of K block b (elements 32 b .. 32 b + 31) of that row is byte `opsel` of the scale register of lane
//    (l & 15) + 16 b.  So a lane's fragment is the 16-byte chunks g and 4 + g of the staged row, and its scale register holds the row's byte g;
//  * the scales of a K step are 4 bytes per tile row: one global_load_lds_dword per lane of two waves per operand (rows of the [rows, K/32] array are
//    4-byte aligned because K is a multiple of 128), read back with ds_read_u8 at row * 4 + (l >> 4);
//  * every byte of LDS is in ONE extern array (a second object de-pipelines the K loop);
//  * weights are the instruction's A operand and activations its B operand, as in gemm.hip: a lane ends with 4 CONSECUTIVE columns of one output row.
//    For the MX output a block of 32 columns is then two adjacent column tiles x the four lanes l, l ^ 16, l ^ 32, l ^ 48: the block maximum is a
//    register maximum and two cross-row exchanges, a lane stores one dword of elements and the lanes l < 16 the scale byte.
#include "common.h"
#include "gemm_epilogue.h"
#include "mx8.h"

namespace {

constexpr int BM = 128, BN = 128, BK = 128;
constexpr int ROW_BYTES = 128;
constexpr int TILE_BYTES = BM * ROW_BYTES;      // 16 KiB per operand per stage
constexpr int SCALE_BYTES = BM * 4;             // 512 B per operand per stage
constexpr int STAGE_BYTES = 2 * TILE_BYTES + 2 * SCALE_BYTES;
constexpr int NTHREADS = 256;

typedef __attribute__((ext_vector_type(8))) int i32x8;
struct Mx8Out {};      // C type tag: e4m3 elements + scales along N

template <typename TC, int EPI, bool RES>
__global__ __launch_bounds__(NTHREADS, 2) void gemm_mx8_kernel(
    int M, int N, int K, const uint8_t* __restrict__ A, int lda, const uint8_t* __restrict__ As, int ldas, const uint8_t* __restrict__ B, int ldb,
    const uint8_t* __restrict__ Bs, int ldbs, void* __restrict__ Cv, int ldc, uint8_t* __restrict__ Cs, int ldcs, const float* __restrict__ bias,
    const float* __restrict__ residual, int ldr, float alpha, int tiles_m, int tiles_n)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];

    // XCD-aware tile order (gemm.hip): each XCD walks a contiguous run of the (n-panel major, m minor) tile list
    const int nwg = tiles_m * tiles_n;
    int bid = blockIdx.x;
    {
        const int q = nwg >> 3, r = nwg & 7, xcd = bid & 7, idx = bid >> 3;
        bid = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + idx;
    }
    constexpr int GROUP_M = 8;
    const int group = bid / (GROUP_M * tiles_n);
    const int first_m = group * GROUP_M;
    const int gsz = min(tiles_m - first_m, GROUP_M);
    const int in_group = bid - group * GROUP_M * tiles_n;
    const int tm = first_m + in_group % gsz;
    const int tn = in_group / gsz;
    const int m0 = tm * BM, n0 = tn * BN;

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1;

    // ---- staging: thread t, instruction i writes LDS byte i*4096 + t*16 of the tile: row i*32 + t/8, physical chunk t%8 ----
    const int srow = tid >> 3;
    const int schunk = (tid & 7) ^ (((wave & 1) << 2) | (lane >> 4));
    const uint8_t* a_src = A + (size_t)(m0 + srow) * lda + schunk * 16;
    const uint8_t* b_src = B + (size_t)(n0 + srow) * ldb + schunk * 16;
    const size_t a_step = (size_t)32 * lda, b_step = (size_t)32 * ldb;
    // scales: waves 0, 1 bring the A tile's 128 rows x 4 bytes, waves 2, 3 the B tile's
    const int sc_row = (wave & 1) * 64 + lane;
    const uint8_t* s_src = wave < 2 ? As + (size_t)(m0 + sc_row) * ldas : Bs + (size_t)(n0 + sc_row) * ldbs;
    const int s_dst = 2 * TILE_BYTES + (wave >> 1) * SCALE_BYTES + (wave & 1) * 256;

    auto stage = [&](int kt, int buf) {
        char* base = smem + buf * STAGE_BYTES + wave * 1024;
        const uint8_t* ap = a_src + (size_t)kt * BK;
        const uint8_t* bp = b_src + (size_t)kt * BK;
#pragma unroll
        for (int i = 0; i < 4; ++i)
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(ap + i * a_step),
                                             (__attribute__((address_space(3))) void*)(base + i * 4096), 16, 0, 0);
#pragma unroll
        for (int i = 0; i < 4; ++i)
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(bp + i * b_step),
                                             (__attribute__((address_space(3))) void*)(base + TILE_BYTES + i * 4096), 16, 0, 0);
        __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(s_src + kt * 4),
                                         (__attribute__((address_space(3))) void*)(smem + buf * STAGE_BYTES + s_dst), 4, 0, 0);
    };

    // ---- fragment reads: lane reads row (l & 15) of a 16-row sub tile, logical chunks (l >> 4) and 4 + (l >> 4); its scale byte is the row's (l >> 4)-th ----
    const int frow = lane & 15;
    const int fsw = frow >> 1;
    const int fg = lane >> 4;
    const int foff0 = frow * ROW_BYTES + (fg ^ fsw) * 16;
    const int foff1 = frow * ROW_BYTES + ((4 | fg) ^ fsw) * 16;
    const int a_frag_base = (wm * 64) * ROW_BYTES;               // activations
    const int b_frag_base = TILE_BYTES + (wn * 64) * ROW_BYTES;  // weights
    const int a_sc_base = 2 * TILE_BYTES + (wm * 64 + frow) * 4 + fg;
    const int b_sc_base = 2 * TILE_BYTES + SCALE_BYTES + (wn * 64 + frow) * 4 + fg;

    f32x4 acc[4][4];  // [n sub tile][m sub tile]
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

    const int nk = K / BK;
    stage(0, 0);
    for (int kt = 0; kt < nk; ++kt) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        if (kt + 1 < nk) stage(kt + 1, (kt + 1) & 1);
        const char* buf = smem + (kt & 1) * STAGE_BYTES;
        i32x8 fa[4], fb[4];
        int sa[4], sb[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const uint4 a0 = *reinterpret_cast<const uint4*>(buf + a_frag_base + i * 16 * ROW_BYTES + foff0);
            const uint4 a1 = *reinterpret_cast<const uint4*>(buf + a_frag_base + i * 16 * ROW_BYTES + foff1);
            const uint4 b0 = *reinterpret_cast<const uint4*>(buf + b_frag_base + i * 16 * ROW_BYTES + foff0);
            const uint4 b1 = *reinterpret_cast<const uint4*>(buf + b_frag_base + i * 16 * ROW_BYTES + foff1);
            fa[i] = i32x8{(int)a0.x, (int)a0.y, (int)a0.z, (int)a0.w, (int)a1.x, (int)a1.y, (int)a1.z, (int)a1.w};
            fb[i] = i32x8{(int)b0.x, (int)b0.y, (int)b0.z, (int)b0.w, (int)b1.x, (int)b1.y, (int)b1.z, (int)b1.w};
            sa[i] = *reinterpret_cast<const uint8_t*>(buf + a_sc_base + i * 64);
            sb[i] = *reinterpret_cast<const uint8_t*>(buf + b_sc_base + i * 64);
        }
#pragma unroll
        for (int ni = 0; ni < 4; ++ni)
#pragma unroll
            for (int mi = 0; mi < 4; ++mi)
                acc[ni][mi] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(fb[ni], fa[mi], acc[ni][mi], 0, 0, 0, sb[ni], 0, sa[mi]);
    }

    // ---- epilogue: lane holds C[m = .. + (l&15)][n = .. + 4*(l>>4) + 0..3] ----
    const int row_base = m0 + wm * 64 + (lane & 15);
    const int col_base = n0 + wn * 64 + ((lane >> 4) << 2);
    f32x4 bvs[4];
#pragma unroll
    for (int ni = 0; ni < 4; ++ni) bvs[ni] = f32x4{0.f, 0.f, 0.f, 0.f};
    if (bias) {
#pragma unroll
        for (int ni = 0; ni < 4; ++ni) bvs[ni] = *reinterpret_cast<const f32x4*>(bias + col_base + ni * 16);
    }
    if constexpr (__is_same(TC, Mx8Out)) {
        uint8_t* C = (uint8_t*)Cv;
#pragma unroll
        for (int mi = 0; mi < 4; ++mi) {
            const int row = row_base + mi * 16;
#pragma unroll
            for (int p = 0; p < 2; ++p) {      // one 32-column block: column tiles 2p and 2p + 1
                f32x4 v0 = acc[2 * p][mi] * alpha + bvs[2 * p], v1 = acc[2 * p + 1][mi] * alpha + bvs[2 * p + 1];
                if constexpr (EPI == LPI_EPI_QUICKGELU) { v0 = quick_gelu_x4(v0); v1 = quick_gelu_x4(v1); }
                float am = fmaxf(mx8_amax4(v0), mx8_amax4(v1));
                auto r = __builtin_amdgcn_permlane16_swap(__float_as_uint(am), __float_as_uint(am), false, false);      // the other 16-lane row of the half
                am = fmaxf(__uint_as_float(r[0]), __uint_as_float(r[1]));
                r = __builtin_amdgcn_permlane32_swap(__float_as_uint(am), __float_as_uint(am), false, false);           // the other half of the wave
                am = fmaxf(__uint_as_float(r[0]), __uint_as_float(r[1]));
                const int byte = mx8_scale_byte(am);
                const int col = col_base + p * 32;
                *reinterpret_cast<uint32_t*>(C + (size_t)row * ldc + col) = mx8_pack4(v0, byte);
                *reinterpret_cast<uint32_t*>(C + (size_t)row * ldc + col + 16) = mx8_pack4(v1, byte);
                if (lane < 16) Cs[(size_t)row * ldcs + (col >> 5)] = (uint8_t)byte;
            }
        }
    } else {
        TC* C = (TC*)Cv;
#pragma unroll
        for (int ni = 0; ni < 4; ++ni) {
            const int col = col_base + ni * 16;
#pragma unroll
            for (int mi = 0; mi < 4; ++mi)      // plain stores: streaming ones cost the bf16 in_proj output 45 % here ("MX-FP8 forward")
                gemm_epilogue_store<bf16_t, TC, EPI, RES, false, false>(acc[ni][mi], row_base + mi * 16, col, C, ldc, bvs[ni], alpha, residual, ldr, nullptr, 0);
        }
    }
}

template <typename TC, int EPI, bool RES>
int launch(const GemmCall& c, const Mx8Side& mx, Tag<TC>, Int<EPI>, Bool<RES>)
{
    const lpi_gemm_desc& d = c.p;
    const int tm = d.M / BM, tn = d.N / BN;
    auto kern = gemm_mx8_kernel<TC, EPI, RES>;
    static LdsOnce once;
    lpi_note_gemm_kernel(LPI_GEMM_K_MX8);
    if (int e = lpi_ensure_lds(once, (const void*)kern, 2 * STAGE_BYTES)) return e;
    LPI_LAUNCH(kern, dim3(tm * tn), dim3(NTHREADS), 2 * STAGE_BYTES, c.s, d.M, d.N, d.K, (const uint8_t*)d.A, d.lda, mx.a_scales, mx.ldas, (const uint8_t*)d.B, d.ldb,
               mx.b_scales, mx.ldbs, d.C, d.ldc, mx.c_scales, mx.ldcs, d.bias, (const float*)d.residual, d.ldr, c.alpha, tm, tn);
    LPI_CHECK_LAST();
    return 0;
}

}  // namespace

extern "C" int lpi_gemm_mx8_ok(int M, int N, int K)
{
    return M > 0 && N > 0 && K > 0 && M % BM == 0 && N % BN == 0 && K % BK == 0 ? 1 : 0;
}

extern "C" int lpi_gemm_nt_mx8(int c_dtype, int M, int N, int K, const void* A, int lda, const void* a_scales, int ldas, const void* B, int ldb,
                               const void* b_scales, int ldbs, void* C, int ldc, void* c_scales, int ldcs, const float* bias, const void* residual,
                               int ldr, int epilogue, float alpha, void* stream)
{
    if (!lpi_gemm_mx8_ok(M, N, K)) return LPI_EINVAL;
    const GemmCall c{.dtype = LPI_MX8, .c_dtype = c_dtype, .epilogue = epilogue, .alpha = alpha, .s = (hipStream_t)stream,
                     .p = {.M = M, .N = N, .K = K, .A = A, .lda = lda, .B = B, .ldb = ldb, .C = C, .ldc = ldc, .bias = bias, .residual = residual, .ldr = ldr}};
    const Mx8Side mx = {(const uint8_t*)a_scales, ldas, (const uint8_t*)b_scales, ldbs, (uint8_t*)c_scales, ldcs};
    if (int e = mx8_gemm_check_args(c, mx)) return e;
    return mx8_pick<Mx8Out>(c, [&](auto... k) { return launch(c, mx, k...); });
}
