// Streamed search on MX-FP8 operands read in place: the tile code of search_tile.h for mx8_t (e4m3 bytes with one E8M0 scale byte per 32 elements, mx8.h;
// v_mfma_scale_f32_16x16x128_f8f6f4, 128 k-values per slab, E a multiple of 128), and its two entry points.  A score is the f32 result of the
// block-scaled instruction chain over E in one fixed order; lists, ranks and thresholds are the f32 kernels' (the epilogues see f32 accumulators), and the
// merge kernel is search.hip's.
#include "search_tile.h"

extern "C" int lpi_search_topk_mx8(int nq, int ng, int E, const void* Q, int ldq, const void* q_scales, int ldqs, const void* G, int ldg,
                                   const void* g_scales, int ldgs, int k, int col_base, int accumulate, int32_t* idx, float* val, void* ws, long ws_bytes,
                                   void* stream)
{
    return search_topk<mx8_t, MODE_TOPK>(SearchCall{.nq = nq, .ng = ng, .E = E, .Q = Q, .ldq = ldq, .G = G, .ldg = ldg, .sc = {q_scales, ldqs, g_scales, ldgs},
                                                    .k = k, .col_base = col_base, .accumulate = accumulate, .idx = idx, .val = val, .ws = ws, .ws_bytes = ws_bytes,
                                                    .stream = stream});
}

extern "C" int lpi_search_rank_mx8(int nq, int ng, int E, const void* Q, int ldq, const void* q_scales, int ldqs, const void* G, int ldg,
                                   const void* g_scales, int ldgs, const int32_t* gt, int gt_per_row, int32_t* rank, void* ws, long ws_bytes, void* stream)
{
    return search_rank<mx8_t>(SearchCall{.nq = nq, .ng = ng, .E = E, .Q = Q, .ldq = ldq, .G = G, .ldg = ldg, .sc = {q_scales, ldqs, g_scales, ldgs}, .gt = gt,
                                         .gt_per_row = gt_per_row, .rank = rank, .ws = ws, .ws_bytes = ws_bytes, .stream = stream});
}
