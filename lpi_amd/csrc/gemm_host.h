// Host layer of the GEMM family (gemm.hip, gemm256.hip, gemm256p.hip, gemm256x128.hip, gemm_rows.hip): one call struct carried by reference, the internal
// launchers declared once, the small predicates two files must agree on, and ONE pick from the run-time values (dtype, c_dtype, epilogue, residual present,
// aux present) to the template arguments <T, TC, EPI, RES, SAVE_U>.  A file lists the (T, TC) pairs it builds and writes its launch once:
//     typedef TypeList<Types<float, float>, Types<bf16_t, f16_t, ResidualOnly>, ...> Built;
//     return gemm_pick(Built{}, c.dtype, c.c_dtype, c.epilogue, res, aux, [&](auto... k) { return launch(c, k...); });
// with   template <typename T, typename TC, int EPI, bool RES, bool SAVE_U> int launch(const GemmCall&, Tag<T>, Tag<TC>, Int<EPI>, Bool<RES>, Bool<SAVE_U>);
// A new type pair is one row in that file's list; a new epilogue is one case in gemm_pick_epi.  ("The GEMM host layer".)
#pragma once
#include "dispatch.h"

extern int g_lpi_tuning[16];

// What is common to a launch, and the problem of a single one.  The grouped and the few-row forms carry the caller's descriptors beside the call.
struct GemmCall {
    int dtype, c_dtype, epilogue;
    float alpha;
    hipStream_t s;
    lpi_gemm_desc p;
};

bool lpi_gemm256_eligible(int dtype, const lpi_gemm_desc& d);      // gemm256.hip: a shape the 256x256 kernels take
bool lpi_gemm256x128_eligible(int dtype, const lpi_gemm_desc& d);  // gemm256x128.hip
int lpi_gemm256_launch(const GemmCall& c);                          // gemm256.hip: persistent where gemm256p_takes() says so, else one tile per workgroup
int lpi_gemm256x128_launch(const GemmCall& c);                      // gemm256x128.hip
int lpi_gemm256p_launch(const GemmCall& c);                         // gemm256p.hip: the persistent kernel on c.p
int lpi_gemm256p_launch2(const GemmCall& c, const lpi_gemm_desc* d);      // ... on d[0] and d[1] in one launch; LPI_ENOSYS: not built, issue them one by one

// group_m of the one-tile-per-workgroup kernels: tuning key 4, or the default
inline int gemm_group_m(int dflt = 8) { return g_lpi_tuning[4] > 0 ? g_lpi_tuning[4] : dflt; }
// operand rows are 4-byte elements in memory (LPI_F32X3 splits them in registers)
inline bool gemm_rows4(int dtype) { return dtype == LPI_F32 || dtype == LPI_F32X3; }
inline bool gemm_epi_ln(int epilogue) { return epilogue == LPI_EPI_LN || epilogue == LPI_EPI_LN_QUICKGELU; }
// Does the persistent kernel take this problem's operands and epilogue?  bf16 / f16 operands; a store-only epilogue, or one that LOADS a 2-byte side tile (the
// fp16 residual stream, the bf16 u of gelu'(u): LPI_EPI_RES_ROWSTATS is res and fp16 by its checks), which comes to LDS by LDS-DMA.  f32 residuals stay on the
// one-tile kernels.  The LN block of the LN-fold epilogues is not a tile.  Tuning key 2: -1 = never, 2 = store-only epilogues only (A/B switches).  A single and
// a grouped launch ask here, so a group picks the kernel its two problems would get one by one.
inline bool gemm256p_takes(const GemmCall& c, const lpi_gemm_desc& d)
{
    const bool res = d.residual != nullptr && !gemm_epi_ln(c.epilogue);
    const bool loads_in_epilogue = res || c.epilogue == LPI_EPI_DQUICKGELU;
    const bool side16 = (res && c.c_dtype == LPI_F16) || c.epilogue == LPI_EPI_DQUICKGELU;
    return !gemm_rows4(c.dtype) && g_lpi_tuning[2] >= 0 && (!loads_in_epilogue || (side16 && g_lpi_tuning[2] != 2));
}

template <int V> using Int = std::integral_constant<int, V>;
template <bool V> using Bool = std::bool_constant<V>;
struct ResidualOnly {};      // third entry of a Types<T, TC, ResidualOnly> row: built for LPI_EPI_NONE with a residual alone (bf16 -> f16, the fp16 residual stream)

// epilogue code and pointer presence -> <EPI, RES, SAVE_U>: a residual only with LPI_EPI_NONE, the saved derivative only with LPI_EPI_QUICKGELU
template <typename T, typename TC, typename F> int gemm_pick_epi(Types<T, TC>, int epi, bool res, bool aux, F& f)
{
    const Tag<T> t;
    const Tag<TC> tc;
    switch (epi) {
    case LPI_EPI_NONE: return res ? f(t, tc, Int<LPI_EPI_NONE>{}, Bool<true>{}, Bool<false>{}) : f(t, tc, Int<LPI_EPI_NONE>{}, Bool<false>{}, Bool<false>{});
    case LPI_EPI_QUICKGELU:
        if (res) return LPI_ENOSYS;
        return aux ? f(t, tc, Int<LPI_EPI_QUICKGELU>{}, Bool<false>{}, Bool<true>{}) : f(t, tc, Int<LPI_EPI_QUICKGELU>{}, Bool<false>{}, Bool<false>{});
    case LPI_EPI_DQUICKGELU:
        if (res) return LPI_ENOSYS;
        return aux ? f(t, tc, Int<LPI_EPI_DQUICKGELU>{}, Bool<false>{}, Bool<false>{}) : LPI_EINVAL;
    }
    return LPI_EINVAL;
}
template <typename T, typename TC, typename F> int gemm_pick_epi(Types<T, TC, ResidualOnly>, int epi, bool res, bool, F& f)
{
    return epi == LPI_EPI_NONE && res ? f(Tag<T>{}, Tag<TC>{}, Int<LPI_EPI_NONE>{}, Bool<true>{}, Bool<false>{}) : LPI_ENOSYS;
}
template <typename T, typename TC, typename... R, typename F> bool gemm_pick_row(Types<T, TC, R...> row, int dtype, int c_dtype, int epi, bool res, bool aux, F& f, int& rc)
{
    if (dtype != Elem<T>::DT || c_dtype != Elem<TC>::DT) return false;
    rc = gemm_pick_epi(row, epi, res, aux, f);
    return true;
}
// f(Tag<T>, Tag<TC>, Int<EPI>, Bool<RES>, Bool<SAVE_U>) of the listed row and the epilogue, or the code to return: LPI_ENOSYS for a pair that is not built
// or a residual with a GELU epilogue, LPI_EINVAL for an unknown epilogue or LPI_EPI_DQUICKGELU without its aux
template <typename... C, typename F> int gemm_pick(TypeList<C...>, int dtype, int c_dtype, int epi, bool res, bool aux, F f)
{
    int rc = LPI_ENOSYS;
    (void)(gemm_pick_row(C{}, dtype, c_dtype, epi, res, aux, f, rc) || ...);
    return rc;
}
