// 256x256-tile NT GEMM, 8 waves, phased schedule with LDS-DMA kept in flight across barriers (counted vmcnt).
//
// Same contract and epilogues as gemm.hip (C = epi(alpha * A . B^T + bias) + residual); selected by lpi_gemm_nt for
// shapes with enough 256x256 tiles.  Why a second kernel: a 128x128 tile needs 64 KB of L2->LDS traffic per CU per 1024
// MFMA cycles (56+ B/clk/CU), i.e. it is L2-bandwidth bound at about half the bf16 MFMA rate; a 256x256 tile halves the
// bytes per FLOP (128 FLOP/B) and, at one 512-thread workgroup per CU, leaves room for a deep staging pipeline.
//
// Geometry: BK = 128 bytes of K per tile row (bf16 64, f32 32).  LDS = 2 K-tile buffers x {A half 0, A half 1, B half 0,
// B half 1} x 16 KiB = 128 KiB.  Wave (wm in 0..1, wn in 0..3) owns rows {h*128 + wm*64 + 0..63 : h = 0,1} and columns
// {h*128 + wn*32 + 0..31 : h = 0,1} of the tile, so each of its four 64x32 output quadrants reads ONE A half and ONE B half.
// Per K-tile two phases of two quadrants (32 MFMA 16x16x32 per wave in bf16), each between two raw barriers:
//     X: read B(0), B(1), A(0)   compute (0,0), (1,0)   stage A-half1 of K-tile kt+1          ; s_waitcnt vmcnt(8)
//     Y: read A(1)               compute (1,1), (0,1)   stage A-half0, B-half0, B-half1 of kt+2 ; s_waitcnt vmcnt(8)
// (the B fragments stay in registers across X and Y).  A half tile is restaged only after the phase whose lgkmcnt(0)+barrier
// retired its last ds_read (WAR), and read only after the counted vmcnt that retires it plus a barrier every wave has passed
// (RAW).  vmcnt(8) leaves the four newest half tiles (2 LDS-DMA instructions each) in flight.  Raw s_barrier only — a
// __syncthreads() would drain the LDS-DMA queue (cdna_hip_programming.md, "Pipelining across barriers").  The first version had
// four phases of one quadrant (8 barriers per K-tile, three half tiles in flight): an empty loop of those barriers alone costs
// 0.64 us per K-tile against 0.87 us of MFMA work (profiles/r01_gemm_ablation.md).
// 1 (default): two phases of 32 MFMAs per K-tile; 0: the earlier four phases of 16 (kept for A/B: same results bit for bit,
// 2.9 % slower over the eight vision-layer GEMMs, 11 % on the qkv shape)
#include "gemm256_tile.h"
#include "gemm256x128_tile.h"
#include "gemm_host.h"

namespace {

using namespace t256;

// workgroup id -> origin of its tile: the bijective XCD remap (blocks that share an XCD, bid % 8, get a contiguous run of tiles), then groups of
// group_m row tiles walked column by column
__device__ __forceinline__ void tile_origin(int tiles_m, int tiles_n, int group_m, int& m0, int& n0)
{
    const int nwg = tiles_m * tiles_n;
    int bid = blockIdx.x;
    {
        const int q = nwg >> 3, r = nwg & 7, xcd = bid & 7, idx = bid >> 3;
        bid = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + idx;
    }
    const int group = bid / (group_m * tiles_n);
    const int first_m = group * group_m;
    const int gsz = min(tiles_m - first_m, group_m);
    const int in_group = bid - group * group_m * tiles_n;
    m0 = (first_m + in_group % gsz) * T256;
    n0 = (in_group / gsz) * T256;
}

template <typename T, typename TC, int EPI, bool RES, bool SAVE_U>
__global__ __launch_bounds__(NTHR, 2) void gemm256_kernel(
    int M, int N, int K, const T* __restrict__ A, int lda, const T* __restrict__ B, int ldb,
    TC* __restrict__ C, int ldc, const float* __restrict__ bias, const float* __restrict__ residual, int ldr,
    typename AuxT<T>::type* __restrict__ aux, int ldaux, float alpha, int tiles_m, int tiles_n, int stagger, int group_m)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    constexpr int EPC = Elem<T>::EPC;
    constexpr int BK = ROWB / (int)sizeof(T);

    // One workgroup per CU and identical tiles keep the CUs in lockstep: all stream HBM (epilogue) together, then all run the
    // matrix cores together.  Delaying every other first-round workgroup once makes the two halves of the chip alternate, so one
    // half's epilogue gets the whole HBM bandwidth while the other half computes (later workgroups inherit their CU's phase).
    if (stagger > 0 && blockIdx.x < 256 && ((blockIdx.x >> 3) & 1)) {
        for (int i = 0; i < stagger; ++i) __builtin_amdgcn_s_sleep(127);
    }
    int m0, n0;
    tile_origin(tiles_m, tiles_n, group_m, m0, n0);
    t256::tile<T, TC, EPI, RES, SAVE_U>(m0, n0, K, A, lda, B, ldb, C, ldc, bias, residual, ldr, aux, ldaux, alpha, smem);
}

// The same launch on MX-FP8 operands (lpi_gemm_nt_mx8_256): one tile per workgroup, no stagger, no aux; the scale arrays travel in `mx`, which the other
// element types' kernel does not have.
template <typename TC, int EPI, bool RES>
__global__ __launch_bounds__(NTHR, 2) void gemm256_mx8_kernel(
    int K, const mx8_t* __restrict__ A, int lda, const mx8_t* __restrict__ B, int ldb, TC* __restrict__ C, int ldc, const float* __restrict__ bias,
    const float* __restrict__ residual, int ldr, float alpha, int tiles_m, int tiles_n, int group_m, Mx8Side mx)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    int m0, n0;
    tile_origin(tiles_m, tiles_n, group_m, m0, n0);
    t256::tile<mx8_t, TC, EPI, RES, false>(m0, n0, K, A, lda, B, ldb, C, ldc, bias, residual, ldr, nullptr, 0, alpha, smem, mx);
}

// Hybrid launch for tile counts that leave a short last round: the first n_full (a multiple of 256) tiles run as 256x256 tiles,
// the remaining rem <= 128 tiles as 2*rem tiles of 256x128 — one round of half tiles instead of one round of a half-empty chip
// (at M = 54 528 every N = 768 GEMM has 639 = 512 + 127 tiles).  Tile ids follow the same XCD-aware order as the plain kernel;
// the two halves of a tail tile sit 8 workgroup ids apart, i.e. on the same XCD, so they share the A rows in its L2.
template <typename T, typename TC, int EPI, bool RES, bool SAVE_U>
__global__ __launch_bounds__(NTHR, 2) void gemm256_tail_kernel(
    int M, int N, int K, const T* __restrict__ A, int lda, const T* __restrict__ B, int ldb,
    TC* __restrict__ C, int ldc, const float* __restrict__ bias, const float* __restrict__ residual, int ldr,
    typename AuxT<T>::type* __restrict__ aux, int ldaux, float alpha, int tiles_m, int tiles_n, int n_full, int group_m)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int nwg = tiles_m * tiles_n;
    int tile_id, half = -1;
    if ((int)blockIdx.x < n_full) {
        const int bid = blockIdx.x;       // n_full % 8 == 0: the XCD remap of the first n_full ids over the FULL tile list
        const int q = nwg >> 3, r = nwg & 7, xcd = bid & 7, idx = bid >> 3;
        tile_id = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + idx;
    } else {
        const int j = blockIdx.x - n_full;
        tile_id = -1 - ((j >> 4) * 8 + (j & 7));      // k-th tile NOT taken by the first n_full ids (resolved below)
        half = (j >> 3) & 1;
    }
    // The first n_full workgroup ids take, per XCD x, that XCD's first n_full/8 tiles; the tail takes the rest in the same order.
    if (tile_id < 0) {
        const int k = -1 - tile_id;                   // 0 .. rem-1 (padded to a multiple of 8: guard below)
        const int q = nwg >> 3, r = nwg & 7, per = n_full >> 3;
        const int xcd = k & 7, idx = per + (k >> 3);  // the (k>>3)-th leftover tile of XCD `xcd`
        const int count = q + (xcd < r ? 1 : 0);
        if (idx >= count) return;
        tile_id = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + idx;
    }
    const int group = tile_id / (group_m * tiles_n);
    const int first_m = group * group_m;
    const int gsz = min(tiles_m - first_m, group_m);
    const int in_group = tile_id - group * group_m * tiles_n;
    const int tm = first_m + in_group % gsz;
    const int tn = in_group / gsz;
    if (half < 0) t256::tile<T, TC, EPI, RES, SAVE_U>(tm * 256, tn * 256, K, A, lda, B, ldb, C, ldc, bias, residual, ldr, aux, ldaux, alpha, smem);
    else t128::tile<T, TC, EPI, RES, SAVE_U>(tm * 256, tn * 256 + half * 128, K, A, lda, B, ldb, C, ldc, bias, residual, ldr, aux, ldaux, alpha, smem);
}

template <typename T, typename TC, int EPI, bool RES, bool SAVE_U>
int launch256(const GemmCall& c, Tag<T>, Tag<TC>, Int<EPI>, Bool<RES>, Bool<SAVE_U>)
{
    const lpi_gemm_desc& d = c.p;
    const int tm = d.M / T256, tn = d.N / T256;
    const int nwg = tm * tn, rem = nwg % 256, n_full = nwg - rem;
    // a short last round (<= 128 of 256 CUs busy) runs as 256x128 half tiles inside the same launch (tuning key 6, default on;
    // bf16 operands only: the f32 path is MFMA-bound and its K-tile count per 128-byte row differs)
    if constexpr (!kIsX3<T>)      // (no 256x128 tile for bf16x3: its rows are f32)
    if (sizeof(T) == 2 && g_lpi_tuning[6] != 0 && n_full >= 256 && rem > 0 && rem <= 128 && d.K / (ROWB / (int)sizeof(T)) >= 2) {
        auto tk = gemm256_tail_kernel<T, TC, EPI, RES, SAVE_U>;
        constexpr int LDS_TAIL = t128::LDS_BYTES > LDS_BYTES ? t128::LDS_BYTES : LDS_BYTES;
        static LdsOnce tail_once;
        lpi_note_gemm_kernel(LPI_GEMM_K_256_TAIL);
        if (int e = lpi_ensure_lds(tail_once, (const void*)tk, LDS_TAIL)) return e;
        const int q = nwg >> 3, r = nwg & 7;
        const int max_left = q + (r ? 1 : 0) - (n_full >> 3);      // leftover tiles of the fullest XCD
        LPI_LAUNCH(tk, dim3(n_full + 16 * max_left), dim3(NTHR), LDS_TAIL, c.s, d.M, d.N, d.K, (const T*)d.A, d.lda, (const T*)d.B, d.ldb, (TC*)d.C, d.ldc, d.bias,
                   (const float*)d.residual, d.ldr, (typename AuxT<T>::type*)d.aux, d.ldaux, c.alpha, tm, tn, n_full, gemm_group_m());
        LPI_CHECK_LAST();
        return 0;
    }
    auto kern = gemm256_kernel<T, TC, EPI, RES, SAVE_U>;
    static LdsOnce once;
    lpi_note_gemm_kernel(kIsX3<T> ? LPI_GEMM_K_X3 : LPI_GEMM_K_256);
    if (int e = lpi_ensure_lds(once, (const void*)kern, LDS_BYTES)) return e;
    LPI_LAUNCH(kern, dim3(tm * tn), dim3(NTHR), LDS_BYTES, c.s, d.M, d.N, d.K, (const T*)d.A, d.lda, (const T*)d.B, d.ldb, (TC*)d.C, d.ldc, d.bias,
               (const float*)d.residual, d.ldr, (typename AuxT<T>::type*)d.aux, d.ldaux, c.alpha, tm, tn, 0, gemm_group_m());
    LPI_CHECK_LAST();
    return 0;
}

template <typename TC, int EPI, bool RES>
int launch256_mx8(const GemmCall& c, const Mx8Side& mx, Tag<TC>, Int<EPI>, Bool<RES>)
{
    const lpi_gemm_desc& d = c.p;
    const int tm = d.M / T256, tn = d.N / T256;
    auto kern = gemm256_mx8_kernel<TC, EPI, RES>;
    static LdsOnce once;
    lpi_note_gemm_kernel(LPI_GEMM_K_MX8_256);
    if (int e = lpi_ensure_lds(once, (const void*)kern, LDS_BYTES_MX8)) return e;
    LPI_LAUNCH(kern, dim3(tm * tn), dim3(NTHR), LDS_BYTES_MX8, c.s, d.K, (const mx8_t*)d.A, d.lda, (const mx8_t*)d.B, d.ldb, (TC*)d.C, d.ldc, d.bias,
               (const float*)d.residual, d.ldr, c.alpha, tm, tn, gemm_group_m(), mx);
    LPI_CHECK_LAST();
    return 0;
}

// the (T, TC) pairs of the one-tile-per-workgroup 256x256 kernels
typedef TypeList<Types<float, float>, Types<f32x3_t, float>, Types<bf16_t, bf16_t>, Types<bf16_t, float>, Types<bf16_t, f16_t, ResidualOnly>, Types<f16_t, f16_t>,
                 Types<f16_t, float>> Built;

}  // namespace

// true if the 256x256 kernel can take this shape
bool lpi_gemm256_eligible(int dtype, const lpi_gemm_desc& d) {
    const int bk = ROWB / (gemm_rows4(dtype) ? 4 : 2);
    if (d.M % T256 || d.N % T256 || d.K % bk) return false;
    const int nk = d.K / bk;
    return nk >= 2 && (nk % 2) == 0;
}

int lpi_gemm256_launch(const GemmCall& c)
{
    // bf16 operands: the persistent kernel (gemm256p.hip: the K-tile ring runs across a workgroup's tiles, the next tile's first K-tile
    // lands under the epilogue); tuning key 2 = -1 keeps one tile per workgroup (A/B switch; same results bit for bit)
    // Store-only epilogues: the next tile's first K-tile lands under the epilogue (qkv 184 -> 162 us, fc+gelu 297 -> 275, dout 61 -> 56).
    // Epilogues that LOAD a 2-byte tile (the fp16 residual stream, the bf16 u of gelu'(u)): that tile comes to LDS by LDS-DMA two
    // passes ahead, so the epilogue issues no vector-memory load (with plain loads they queued behind the in-flight DMA in the in-order
    // vmcnt queue and the persistent kernel LOST 8-30 % on them).  f32 residuals (few-row GEMMs only) stay on the one-tile kernels.
    if (gemm256p_takes(c, c.p)) {
        const int rc = lpi_gemm256p_launch(c);
        if (rc != LPI_ENOSYS) return rc;
    }
    return gemm_pick(Built{}, c.dtype, c.c_dtype, c.epilogue, c.p.residual != nullptr, c.p.aux != nullptr, [&](auto... k) { return launch256(c, k...); });
}

// ---- MX-FP8 operands on the 256x256 tile (include/lpi_hip.h) ----
extern "C" int lpi_gemm_mx8_256_ok(int M, int N, int K)
{
    if (M <= 0 || N <= 0 || K <= 0 || M % T256 || N % T256 || K % ROWB) return 0;      // a staged row is ROWB = 128 elements of K
    const int nk = K / ROWB;
    return nk >= 2 && (nk % 2) == 0 ? 1 : 0;
}

extern "C" int lpi_gemm_nt_mx8_256(int c_dtype, int M, int N, int K, const void* A, int lda, const void* a_scales, int ldas, const void* B, int ldb,
                                   const void* b_scales, int ldbs, void* C, int ldc, void* c_scales, int ldcs, const float* bias, const void* residual,
                                   int ldr, int epilogue, float alpha, void* stream)
{
    if (!lpi_gemm_mx8_256_ok(M, N, K)) return LPI_EINVAL;
    const GemmCall c{.dtype = LPI_MX8, .c_dtype = c_dtype, .epilogue = epilogue, .alpha = alpha, .s = (hipStream_t)stream,
                     .p = {.M = M, .N = N, .K = K, .A = A, .lda = lda, .B = B, .ldb = ldb, .C = C, .ldc = ldc, .bias = bias, .residual = residual, .ldr = ldr}};
    const Mx8Side mx = {(const uint8_t*)a_scales, ldas, (const uint8_t*)b_scales, ldbs, (uint8_t*)c_scales, ldcs};
    if (int e = mx8_gemm_check_args(c, mx)) return e;
    return mx8_pick<mx8_out_t>(c, [&](auto... k) { return launch256_mx8(c, mx, k...); });
}
