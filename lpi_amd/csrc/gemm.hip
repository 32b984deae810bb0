// NT GEMM on the gfx950 matrix cores:  C[M,N] = epi(alpha * A[M,K] . B[N,K]^T + bias) + residual
//
// replaces: nn.Linear / nn.MultiheadAttention projections / conv1-as-matmul / x @ proj of the reference
// (retrieval/models/clip/model.py:172-177,185,215,228,257; prompt_learner.py:61) and all their dgrads
// (the backbone is frozen, so backward is dgrad only and B is then the pre-transposed weight).
//
// Design (MI355X first):
//  * block tile 128x128, 4 waves as 2x2, each wave 64x64 = 4x4 MFMA 16x16 tiles (64 accumulator VGPRs);
//  * both operands are K-contiguous, so one LDS tile row = 128 bytes = 8 x 16-byte chunks for either element
//    type (bf16: BK=64, f32: BK=32); the same staging/fragment code serves both, only mma_chunk differs;
//    bf16x3 (T = f32x3_t, LPI_F32X3) stages f32 rows the same way and splits each fragment into hi + lo bf16 in registers: a K tile of 32 is
//    one v_mfma_f32_16x16x32_bf16 triple (hi.hi + hi.lo + lo.hi) per 16x16 tile;
//  * global -> LDS by `global_load_lds_dwordx4` (16 B/lane, no VGPR round trip), double buffered, one barrier
//    per K tile; the LDS image is lane-linear so the bank swizzle chunk ^= (row>>1)&7 is applied to the
//    per-lane SOURCE address and again on the ds_read_b128 (conflict-free for the 16x16 fragment pattern);
//  * operands are swapped in the MFMA (weights = "A", activations = "B") so that each lane ends up holding 4
//    CONSECUTIVE columns of one output row: the epilogue (bias, QuickGELU, gelu', residual) runs on float4s and
//    stores 16 B (f32) / 8 B (bf16) per lane;
//  * blockIdx is remapped so that the blocks sharing one XCD's L2 walk neighbouring M tiles of the same N panel.
#include "gemm_host.h"
#include "gemm_epilogue.h"

namespace {

constexpr int BM = 128, BN = 128;
constexpr int ROW_BYTES = 128;              // one staged tile row (BK elements)
constexpr int TILE_BYTES = BM * ROW_BYTES;  // 16 KiB per operand per stage
constexpr int STAGE_BYTES = 2 * TILE_BYTES;
constexpr int NTHREADS = 256;

template <typename T, typename TC, int EPI, bool RES, bool SAVE_U>
__device__ __forceinline__ void gemm_nt_tile(
    int bx, char* smem, int M, int N, int K, const T* __restrict__ A, int lda, const T* __restrict__ B, int ldb,
    TC* __restrict__ C, int ldc, const float* __restrict__ bias, const float* __restrict__ residual, int ldr,
    typename AuxT<T>::type* __restrict__ aux, int ldaux, float alpha, int tiles_m, int tiles_n)
{
    constexpr int EPC = Elem<T>::EPC;
    constexpr int BK = ROW_BYTES / (int)sizeof(T);

    // XCD-aware tile order: consecutive block ids round-robin over the 8 XCDs; give each XCD a contiguous
    // run of the (n-panel major, m minor) tile list so the B panel and neighbouring A tiles stay in its L2.
    const int nwg = tiles_m * tiles_n;
    int bid = bx;
    {
        const int q = nwg >> 3, r = nwg & 7, xcd = bid & 7, idx = bid >> 3;
        bid = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + idx;
    }
    // group GROUP_M m-tiles per n-tile sweep so one XCD reuses a B panel against several A tiles
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
    const int wm = wave >> 1, wn = wave & 1;   // wave's 64x64 quadrant

    // ---- staging addresses: thread t, instruction i writes LDS byte i*4096 + t*16 of the tile ----------
    // row = i*32 + t/8, physical chunk = t%8, logical chunk = phys ^ ((row>>1)&7) = phys ^ (4*(wave&1) + lane/16)
    const int srow = tid >> 3;
    const int schunk = (tid & 7) ^ (((wave & 1) << 2) | (lane >> 4));
    const T* a_src = A + (size_t)(m0 + srow) * lda + schunk * EPC;
    const T* b_src = B + (size_t)(n0 + srow) * ldb + schunk * EPC;
    const size_t a_step = (size_t)32 * lda, b_step = (size_t)32 * ldb;

    auto stage = [&](int kt, int buf) {
        char* base = smem + buf * STAGE_BYTES + wave * 1024;
        const T* ap = a_src + (size_t)kt * BK;
        const T* bp = b_src + (size_t)kt * BK;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(ap + i * a_step),
                                             (__attribute__((address_space(3))) void*)(base + i * 4096), 16, 0, 0);
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(bp + i * b_step),
                                             (__attribute__((address_space(3))) void*)(base + TILE_BYTES + i * 4096), 16, 0, 0);
        }
    };

    // ---- fragment read offsets: lane reads row (l&15) of a 16-row sub tile, logical chunk 4*ks + (l>>4) ----
    const int frow = lane & 15;
    const int fsw = frow >> 1;                 // (row>>1)&7, sub-tile bases are multiples of 16
    const int fg = lane >> 4;
    int foff[2];
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) foff[ks] = frow * ROW_BYTES + (((ks << 2) | fg) ^ fsw) * 16;
    const int a_frag_base = (wm * 64) * ROW_BYTES;               // activations: rows of the A tile
    const int b_frag_base = TILE_BYTES + (wn * 64) * ROW_BYTES;  // weights: rows of the B tile

    f32x4 acc[4][4];  // [n sub tile][m sub tile]
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

    const int nk = K / BK;
    stage(0, 0);
    for (int kt = 0; kt < nk; ++kt) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // this wave's LDS-DMA of tile kt has landed
        __syncthreads();                                  // ... and everyone's; buffer (kt+1)&1 is free again
        if (kt + 1 < nk) stage(kt + 1, (kt + 1) & 1);
        const char* buf = smem + (kt & 1) * STAGE_BYTES;
        if constexpr (kIsX3<T>) {
            // bf16x3: a lane's two chunks of a row are one 16x16x32 instruction's 8 k-values; split each fragment once, then 3 x 16 instructions
            Chunk fa[4][2], fb[4][2];
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int ks = 0; ks < 2; ++ks) {
                    fa[i][ks].u = *reinterpret_cast<const uint4*>(buf + a_frag_base + i * 16 * ROW_BYTES + foff[ks]);
                    fb[i][ks].u = *reinterpret_cast<const uint4*>(buf + b_frag_base + i * 16 * ROW_BYTES + foff[ks]);
                }
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                split_bf16x3(fa[i][0], fa[i][1]);
                split_bf16x3(fb[i][0], fb[i][1]);
            }
#pragma unroll
            for (int t = 0; t < 3; ++t)
#pragma unroll
                for (int ni = 0; ni < 4; ++ni)
#pragma unroll
                    for (int mi = 0; mi < 4; ++mi) mma_chunk<bf16_t>(acc[ni][mi], fb[ni][t >> 1], fa[mi][t & 1]);
        } else {
#pragma unroll
            for (int ks = 0; ks < 2; ++ks) {
                Chunk fa[4], fb[4];
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    fa[i].u = *reinterpret_cast<const uint4*>(buf + a_frag_base + i * 16 * ROW_BYTES + foff[ks]);
                    fb[i].u = *reinterpret_cast<const uint4*>(buf + b_frag_base + i * 16 * ROW_BYTES + foff[ks]);
                }
#pragma unroll
                for (int ni = 0; ni < 4; ++ni)
#pragma unroll
                    for (int mi = 0; mi < 4; ++mi) mma_chunk<T>(acc[ni][mi], fb[ni], fa[mi]);
            }
        }
    }

    // ---- epilogue: lane holds C[m = .. + (l&15)][n = .. + 4*(l>>4) + 0..3] ------------------------------
    const int row_base = m0 + wm * 64 + (lane & 15);
    const int col_base = n0 + wn * 64 + ((lane >> 4) << 2);
    f32x4 bvs[4];
#pragma unroll
    for (int ni = 0; ni < 4; ++ni) bvs[ni] = f32x4{0.f, 0.f, 0.f, 0.f};
    if (bias) {   // ONE branch for all bias loads
#pragma unroll
        for (int ni = 0; ni < 4; ++ni) bvs[ni] = *reinterpret_cast<const f32x4*>(bias + col_base + ni * 16);
    }
#pragma unroll
    for (int ni = 0; ni < 4; ++ni) {
        const int col = col_base + ni * 16;
#pragma unroll
        for (int mi = 0; mi < 4; ++mi)
            gemm_epilogue_store<T, TC, EPI, RES, SAVE_U>(acc[ni][mi], row_base + mi * 16, col, C, ldc, bvs[ni], alpha, residual, ldr, aux, ldaux);
    }
}

template <typename T, typename TC, int EPI, bool RES, bool SAVE_U>
__global__ __launch_bounds__(NTHREADS, 2) void gemm_nt_kernel(
    int M, int N, int K, const T* __restrict__ A, int lda, const T* __restrict__ B, int ldb,
    TC* __restrict__ C, int ldc, const float* __restrict__ bias, const float* __restrict__ residual, int ldr,
    typename AuxT<T>::type* __restrict__ aux, int ldaux, float alpha, int tiles_m, int tiles_n)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    gemm_nt_tile<T, TC, EPI, RES, SAVE_U>(blockIdx.x, smem, M, N, K, A, lda, B, ldb, C, ldc, bias, residual, ldr, aux, ldaux, alpha, tiles_m, tiles_n);
}

template <typename T, typename TC, int EPI, bool RES, bool SAVE_U>
int launch(const GemmCall& c, Tag<T>, Tag<TC>, Int<EPI>, Bool<RES>, Bool<SAVE_U>)
{
    const lpi_gemm_desc& d = c.p;
    const int tm = d.M / BM, tn = d.N / BN;
    auto kern = gemm_nt_kernel<T, TC, EPI, RES, SAVE_U>;
    static LdsOnce once;
    lpi_note_gemm_kernel(kIsX3<T> ? LPI_GEMM_K_X3 : LPI_GEMM_K_128);
    if (int e = lpi_ensure_lds(once, (const void*)kern, 2 * STAGE_BYTES)) return e;
    LPI_LAUNCH(kern, dim3(tm * tn), dim3(NTHREADS), 2 * STAGE_BYTES, c.s, d.M, d.N, d.K, (const T*)d.A, d.lda, (const T*)d.B, d.ldb, (TC*)d.C, d.ldc, d.bias,
               (const float*)d.residual, d.ldr, (typename AuxT<T>::type*)d.aux, d.ldaux, c.alpha, tm, tn);
    LPI_CHECK_LAST();
    return 0;
}

// the (T, TC) pairs of the 128x128 kernel; bf16 -> f16 is the fp16 residual stream: x_out = x_in + (A.B^T + bias), both fp16
typedef TypeList<Types<float, float>, Types<f32x3_t, float>, Types<bf16_t, bf16_t>, Types<bf16_t, float>, Types<bf16_t, f16_t, ResidualOnly>, Types<f16_t, f16_t>,
                 Types<f16_t, float>> Built;

}  // namespace

// argument checks shared by lpi_gemm_nt and lpi_gemm_nt_grouped
static int gemm_nt_check(const GemmCall& c, const lpi_gemm_desc& d)
{
    const int dtype = c.dtype, c_dtype = c.c_dtype, epilogue = c.epilogue;
    const void* aux = d.aux;
    if (dtype == LPI_F32X3) {      // bf16x3: everything in memory is f32; the epilogues of the f32 mode
        if (c_dtype != LPI_F32) return LPI_ENOSYS;
        if (epilogue != LPI_EPI_NONE && epilogue != LPI_EPI_QUICKGELU && epilogue != LPI_EPI_DQUICKGELU) return LPI_ENOSYS;
    }
    const int esz = gemm_rows4(dtype) ? 4 : 2;
    const int csz = c_dtype == LPI_F32 ? 4 : 2;
    if (epilogue == LPI_EPI_RES_ROWSTATS) {      // the fp16 residual epilogue + the row statistics of its output: aux = f32 slots, N/128 x 2 x ldaux
        if (c_dtype != LPI_F16 || dtype == LPI_F32) return LPI_ENOSYS;
        if (!d.residual || !aux || d.ldaux < d.M || (d.ldaux & 3) || ((uintptr_t)aux & 15)) return LPI_EINVAL;
        aux = nullptr;      // the checks below are for an operand-typed [M, N] aux tile
    }
    if (c_dtype == LPI_F16 && dtype == LPI_BF16 && ((epilogue != LPI_EPI_NONE && epilogue != LPI_EPI_RES_ROWSTATS) || !d.residual)) return LPI_ENOSYS;
    if (c_dtype == LPI_F16 && dtype == LPI_F32) return LPI_ENOSYS;
    const bool ln = gemm_epi_ln(epilogue);
    if (c_dtype == LPI_BF16 && dtype == LPI_F16 && !ln) return LPI_ENOSYS;      // f16 operands write f16 or f32 (bf16: the LN-fold GEMMs of bf16 mode)
    if (ln) {      // LayerNorm folded into the GEMM: residual = mean[ldr] | rstd[ldr] | c1[N] (f32)
        if (dtype == LPI_F32 || c_dtype == LPI_F32) return LPI_ENOSYS;
        if (!d.residual || !d.bias || d.ldr < d.M || (d.ldr & 3) || ((uintptr_t)d.residual & 15)) return LPI_EINVAL;
        if (epilogue == LPI_EPI_LN && aux) return LPI_EINVAL;
    }
    const int bk = ROW_BYTES / esz;
    if (!d.A || !d.B || !d.C || d.M <= 0 || d.N <= 0 || d.K <= 0) return LPI_EINVAL;
    if (d.M % BM || d.N % BN || d.K % bk) return LPI_EINVAL;
    // Every row of every operand starts on a 16-byte boundary (include/lpi_hip.h).  Which kernel runs is the dispatcher's choice (tuning keys, CU count), and
    // the widest access any of them makes decides: most epilogues move four elements per lane (8 bytes of a 2-byte C / residual / aux), but the persistent
    // kernel stores whole 16-byte pieces of a 2-byte C row (half-width staging) and brings the 2-byte residual / gelu' tiles to LDS 16 bytes per lane, and an
    // f32 C / residual / aux moves as f32x4 everywhere ("Leading dimensions of the GEMM family").
    const int rsz = c_dtype == LPI_F16 ? 2 : 4;      // the residual tile has C's type on the fp16 stream, f32 otherwise
    if ((d.lda * esz) % 16 || (d.ldb * esz) % 16 || (d.ldc * csz) % 16 || d.lda < d.K || d.ldb < d.K || d.ldc < d.N) return LPI_EINVAL;
    if (((uintptr_t)d.A | (uintptr_t)d.B | (uintptr_t)d.C) & 15) return LPI_EINVAL;
    if (d.residual && !ln && (d.ldr < d.N || (d.ldr * rsz) % 16 || ((uintptr_t)d.residual & 15))) return LPI_EINVAL;
    if (d.bias && ((uintptr_t)d.bias & 15)) return LPI_EINVAL;
    if (aux && (d.ldaux < d.N || ((uintptr_t)aux & 15) || (d.ldaux * esz) % 16)) return LPI_EINVAL;
    if (epilogue == LPI_EPI_DQUICKGELU && !aux) return LPI_EINVAL;
    return 0;
}

// one checked problem -> the kernel for its shape
static int gemm_nt_one(const GemmCall& c)
{
    const lpi_gemm_desc& d = c.p;
    if (int e = gemm_nt_check(c, d)) return e;
    if (gemm_epi_ln(c.epilogue) && c.alpha != 1.0f) return LPI_EINVAL;      // LN(x) W^T + b has no scale (the epilogue does not multiply by one)
    const bool big = lpi_gemm256_eligible(c.dtype, d);
    if (gemm_epi_ln(c.epilogue) || c.epilogue == LPI_EPI_RES_ROWSTATS)      // only the persistent 256x256 kernel has the LN-fold and the row-statistics epilogues
        return big ? lpi_gemm256p_launch(c) : LPI_ENOSYS;
    // Half-empty launches: fewer than tuning key 5 (default 160) 256x256 tiles -> 256x128 tiles, twice the workgroups (bf16 only:
    // the f32 path is MFMA-bound at any tile size).  Key 5 = 0 disables it.
    const bool f32_rows = gemm_rows4(c.dtype);
    const int tiles256 = (d.M / 256) * (d.N / 256);
    if (!f32_rows && g_lpi_tuning[5] > 0 && big && tiles256 < g_lpi_tuning[5] && tiles256 >= 16 && lpi_gemm256x128_eligible(c.dtype, d)) {
        const int rc = lpi_gemm256x128_launch(c);
        if (rc != LPI_ENOSYS) return rc;
    }
    // 256x256 8-phase kernel when the shape gives it enough tiles to fill the chip (tuning keys 0 / 1 = minimum tile count for bf16 / f32)
    if (big && tiles256 >= g_lpi_tuning[f32_rows ? 1 : 0]) return lpi_gemm256_launch(c);
    return gemm_pick(Built{}, c.dtype, c.c_dtype, c.epilogue, d.residual != nullptr, d.aux != nullptr, [&](auto... k) { return launch(c, k...); });
}

// residual: fp16 when c_dtype == LPI_F16 (re-typed in the epilogue)
extern "C" int lpi_gemm_nt(int dtype, int c_dtype, int M, int N, int K, const void* A, int lda, const void* B, int ldb,
                           void* C, int ldc, const float* bias, const void* residual, int ldr, int epilogue, void* aux,
                           int ldaux, float alpha, void* stream)
{
    return gemm_nt_one(GemmCall{.dtype = dtype, .c_dtype = c_dtype, .epilogue = epilogue, .alpha = alpha, .s = (hipStream_t)stream,
                                .p = {.M = M, .N = N, .K = K, .A = A, .lda = lda, .B = B, .ldb = ldb, .C = C, .ldc = ldc, .bias = bias, .residual = residual,
                                      .ldr = ldr, .aux = aux, .ldaux = ldaux}});
}

// 1 if lpi_gemm_nt takes LPI_EPI_LN / LPI_EPI_LN_QUICKGELU for this operand type and shape (the persistent 256x256 kernel's shapes), else 0
extern "C" int lpi_gemm_ln_supported(int dtype, int M, int N, int K)
{
    return (dtype == LPI_F16 || dtype == LPI_BF16) && M > 0 && N > 0 && K > 0 && lpi_gemm256_eligible(dtype, lpi_gemm_desc{.M = M, .N = N, .K = K}) ? 1 : 0;
}

static thread_local int t_last_grouped = 0;
extern "C" int lpi_gemm_last_grouped(void) { return t_last_grouped; }

extern "C" int lpi_gemm_nt_grouped(int dtype, int c_dtype, int epilogue, float alpha, int count, const lpi_gemm_desc* d, void* stream)
{
    GemmCall c{.dtype = dtype, .c_dtype = c_dtype, .epilogue = epilogue, .alpha = alpha, .s = (hipStream_t)stream};
    if (gemm_epi_ln(epilogue) && alpha != 1.0f) return LPI_EINVAL;
    if (count <= 0 || !d) return LPI_EINVAL;
    t_last_grouped = 0;
    for (int i = 0; i < count; ++i)
        if (int e = gemm_nt_check(c, d[i])) return e;
    // one persistent launch: two problems that the 256x256 kernel takes, with operands and an epilogue the persistent kernel has, together at
    // least a round of tiles, agreeing on residual and aux (tuning key 8 != 0 = never group: A/B switch)
    bool group = count == 2 && g_lpi_tuning[8] == 0;
    int tiles = 0;
    for (int i = 0; i < 2 && group; ++i) {
        group = gemm256p_takes(c, d[i]) && lpi_gemm256_eligible(dtype, d[i]);
        tiles += (d[i].M / 256) * (d[i].N / 256);
    }
    group = group && tiles >= 256 && (d[0].residual != nullptr) == (d[1].residual != nullptr) && (d[0].aux != nullptr) == (d[1].aux != nullptr);
    if (group) {
        const int rc = lpi_gemm256p_launch2(c, d);
        if (rc == 0) t_last_grouped = 1;
        if (rc != LPI_ENOSYS) return rc;
    }
    for (int i = 0; i < count; ++i) {
        c.p = d[i];
        if (int e = gemm_nt_one(c)) return e;
    }
    return 0;
}
