// Streamed search on MX-FP4 operands read in place: the tile code of search_tile.h for mx4_t (e2m1 nibbles, two per byte, with one E8M0 scale byte per 32
// elements, mx4.h; v_mfma_scale_f32_16x16x128_f8f6f4 with cbsz = blgp = 4, 256 k-values per slab in two steps, E a multiple of 128), and its narrow and
// wide entry points.  A coarse operand: its lists are candidate lists for lpi_search_rerank, so there is no rank form.  A score is the f32 result of the
// block-scaled instruction chain over E in one fixed order; the lists are the f32 kernels' (the epilogues see f32 accumulators), and the merge kernels
// are search.hip's and search_wide.hip's.
#include "search_tile.h"

extern "C" int lpi_search_topk_mx4(int nq, int ng, int E, const void* Q, int ldq, const void* q_scales, int ldqs, const void* G, int ldg,
                                   const void* g_scales, int ldgs, int k, int col_base, int accumulate, int32_t* idx, float* val, void* ws, long ws_bytes,
                                   void* stream)
{
    return search_topk<mx4_t, MODE_TOPK>(SearchCall{.nq = nq, .ng = ng, .E = E, .Q = Q, .ldq = ldq, .G = G, .ldg = ldg, .sc = {q_scales, ldqs, g_scales, ldgs},
                                                    .k = k, .col_base = col_base, .accumulate = accumulate, .idx = idx, .val = val, .ws = ws, .ws_bytes = ws_bytes,
                                                    .stream = stream});
}

extern "C" int lpi_search_topk_wide_mx4(int nq, int ng, int E, const void* Q, int ldq, const void* q_scales, int ldqs, const void* G, int ldg,
                                        const void* g_scales, int ldgs, int k, int col_base, int accumulate, int32_t* idx, float* val, void* ws,
                                        long ws_bytes, void* stream)
{
    return search_topk<mx4_t, MODE_WIDE>(SearchCall{.nq = nq, .ng = ng, .E = E, .Q = Q, .ldq = ldq, .G = G, .ldg = ldg, .sc = {q_scales, ldqs, g_scales, ldgs},
                                                    .k = k, .col_base = col_base, .accumulate = accumulate, .idx = idx, .val = val, .ws = ws, .ws_bytes = ws_bytes,
                                                    .stream = stream});
}
