// 256x128-tile NT GEMM, 8 waves (4x2, each 64x64), 3-stage LDS ring, two phases per K-tile, staggered wave groups.
//
// Same contract and epilogues as gemm256.hip, same results bit for bit.  Used by lpi_gemm_nt for launches that would leave the
// chip half empty with 256x256 tiles: the text tower's N = 512 GEMMs at B = 256 have 118 such tiles for 256 CUs; with 256x128
// tiles they have 236.  (On shapes with plenty of tiles it loses to the 256x256 kernel — 1.5x the L2->LDS bytes per FLOP and 0.5
// ds_read_b128 per MFMA instead of 0.375 — which is why it is not used there: profiles/r01_gemm_ablation.md.)
//
// Pipeline: a K-tile (128 B of K per row; 256 A rows + 128 B rows = 48 KiB) is staged by 6 LDS-DMA instructions per thread into a
// ring of 3 stages (144 KiB), two K-tiles ahead: at K-tile kt, phase 1 issues the DMA of kt+2 into the stage K-tile kt-1 just
// vacated, phase 2 waits with a counted vmcnt(6) (kt+2 stays in flight) so that kt+1 has landed before the next iteration.
// Each phase = 8 ds_read_b128 + 16 MFMA per wave between two raw barriers; waves 4-7 run one barrier behind waves 0-3 so one
// group's LDS reads overlap the other's MFMAs (lgkmcnt(0) before the barrier keeps the restage WAR-safe, as in gemm256.hip).
#include "gemm256x128_tile.h"
#include "gemm_host.h"

namespace {

using namespace t128;

template <typename T, typename TC, int EPI, bool RES, bool SAVE_U>
__global__ __launch_bounds__(NTHR, 2) void gemm256x128_kernel(
    int M, int N, int K, const T* __restrict__ A, int lda, const T* __restrict__ B, int ldb,
    TC* __restrict__ C, int ldc, const float* __restrict__ bias, const float* __restrict__ residual, int ldr,
    typename AuxT<T>::type* __restrict__ aux, int ldaux, float alpha, int tiles_m, int tiles_n, int group_m)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    constexpr int EPC = Elem<T>::EPC;
    constexpr int BK = ROWB / (int)sizeof(T);

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
    const int tm = first_m + in_group % gsz;
    const int tn = in_group / gsz;
    const int m0 = tm * TM, n0 = tn * TN;

    t128::tile<T, TC, EPI, RES, SAVE_U>(m0, n0, K, A, lda, B, ldb, C, ldc, bias, residual, ldr, aux, ldaux, alpha, smem);
}

template <typename T, typename TC, int EPI, bool RES, bool SAVE_U>
int launch(const GemmCall& c, Tag<T>, Tag<TC>, Int<EPI>, Bool<RES>, Bool<SAVE_U>)
{
    const lpi_gemm_desc& d = c.p;
    const int tm = d.M / TM, tn = d.N / TN;
    auto kern = gemm256x128_kernel<T, TC, EPI, RES, SAVE_U>;
    static LdsOnce once;
    lpi_note_gemm_kernel(LPI_GEMM_K_256X128);
    if (int e = lpi_ensure_lds(once, (const void*)kern, LDS_BYTES)) return e;
    LPI_LAUNCH(kern, dim3(tm * tn), dim3(NTHR), LDS_BYTES, c.s, d.M, d.N, d.K, (const T*)d.A, d.lda, (const T*)d.B, d.ldb, (TC*)d.C, d.ldc, d.bias,
               (const float*)d.residual, d.ldr, (typename AuxT<T>::type*)d.aux, d.ldaux, c.alpha, tm, tn, gemm_group_m());
    LPI_CHECK_LAST();
    return 0;
}

// the (T, TC) pairs of the 256x128 kernel (no bf16x3: its rows are f32)
typedef TypeList<Types<float, float>, Types<bf16_t, bf16_t>, Types<bf16_t, float>, Types<bf16_t, f16_t, ResidualOnly>, Types<f16_t, f16_t>, Types<f16_t, float>> Built;

}  // namespace

bool lpi_gemm256x128_eligible(int dtype, const lpi_gemm_desc& d) {
    const int bk = ROWB / (dtype == LPI_F32 ? 4 : 2);      // (LPI_F32X3 never asks: lpi_gemm_nt sends 2-byte operands only)
    return d.M % TM == 0 && d.N % TN == 0 && d.K % bk == 0 && d.K / bk >= 2;
}

int lpi_gemm256x128_launch(const GemmCall& c)
{
    return gemm_pick(Built{}, c.dtype, c.c_dtype, c.epilogue, c.p.residual != nullptr, c.p.aux != nullptr, [&](auto... k) { return launch(c, k...); });
}
