// Streamed search on 2-byte operands read in place: the tile code of search_tile.h for bf16_t / f16_t (v_mfma_f32_16x16x32_bf16 / _f16, 64 k-values per
// slab, E a multiple of 32), and the typed entry points.  A score is the f32 accumulation, in one fixed order over E, of the exact products of the 2-byte
// values; lists, ranks and thresholds are the f32 kernels' (the epilogues see f32 accumulators), and the merge kernel is search.hip's.
// This object instantiates the 2-byte sweeps only: LPI_F32 goes on to the f32 entry points, whose sweeps are search.hip's.
#include "search_tile.h"

extern "C" int lpi_search_topk_t(int dt, int nq, int ng, int E, const void* Q, int ldq, const void* G, int ldg, int k, int col_base, int accumulate,
                                 int32_t* idx, float* val, void* ws, long ws_bytes, void* stream)
{
    if (dt == LPI_F32) return lpi_search_topk(nq, ng, E, (const float*)Q, ldq, (const float*)G, ldg, k, col_base, accumulate, idx, val, ws, ws_bytes, stream);
    const SearchCall c{.nq = nq, .ng = ng, .E = E, .Q = Q, .ldq = ldq, .G = G, .ldg = ldg, .k = k, .col_base = col_base, .accumulate = accumulate, .idx = idx,
                       .val = val, .ws = ws, .ws_bytes = ws_bytes, .stream = stream};
    return search_pick(TwoByte{}, dt, [&](auto t) { return search_topk<type_of<decltype(t)>, MODE_TOPK>(c); });
}

extern "C" int lpi_search_rank_t(int dt, int nq, int ng, int E, const void* Q, int ldq, const void* G, int ldg, const int32_t* gt, int gt_per_row,
                                 int32_t* rank, void* ws, long ws_bytes, void* stream)
{
    if (dt == LPI_F32) return lpi_search_rank(nq, ng, E, (const float*)Q, ldq, (const float*)G, ldg, gt, gt_per_row, rank, ws, ws_bytes, stream);
    const SearchCall c{.nq = nq, .ng = ng, .E = E, .Q = Q, .ldq = ldq, .G = G, .ldg = ldg, .gt = gt, .gt_per_row = gt_per_row, .rank = rank, .ws = ws,
                       .ws_bytes = ws_bytes, .stream = stream};
    return search_pick(TwoByte{}, dt, [&](auto t) { return search_rank<type_of<decltype(t)>>(c); });
}
