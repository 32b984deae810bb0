// Streamed retrieval search: score tiles on the matrix cores, consumed from the accumulators, never stored.
//
//   lpi_search_topk: the k best gallery rows of every query row, order (value desc, index desc) = lpi_topk's
//   lpi_search_rank: rank of the best ground-truth gallery row of every query row                = lpi_retrieval_rank's
//
// replaces: `score_matrix` + lpi_topk / lpi_retrieval_rank where only neighbours or ranks are wanted (the evaluation's
// (image_feats @ text_feats.t()) of methods/sprompt.py:509 followed by the np.argsort rank search of :558-599): O(N k) memory, not O(N M).
//
// This file: the f32 instantiations of the tile code (search_tile.h, where the design is described), the merge kernel and the workspace function,
// which do not depend on the operand type.  The 2-byte instantiations and the typed entry points are search16.hip's.
#include "search_tile.h"

namespace {

// one thread per query row: the partial lists (and, with accumulate, the list idx / val already hold) -> idx / val
__global__ __launch_bounds__(64) void search_merge_kernel(int nq, int k, int nparts, const float* __restrict__ part_val,
                                                          const int32_t* __restrict__ part_idx, int col_base, int accumulate,
                                                          int32_t* idx, float* val)
{
    __shared__ float lvs[KMAX * 64];
    __shared__ int lis[KMAX * 64];
    const int row = blockIdx.x * 64 + threadIdx.x;
    if (row >= nq) return;
    lds_f32* lv = (lds_f32*)lvs + threadIdx.x * KMAX;
    lds_i32* li = (lds_i32*)lis + threadIdx.x * KMAX;
    for (int t = 0; t < k; ++t) { lv[t] = -INFINITY; li[t] = -1; }
    if (accumulate) {
        for (int t = 0; t < k; ++t) {
            const int j = idx[(size_t)row * k + t];
            if (j >= 0) list_insert(lv, li, k, val[(size_t)row * k + t], j);
        }
    }
    for (int p = 0; p < nparts; ++p) {
        const size_t o = ((size_t)p * nq + row) * k;
        for (int t = 0; t < k; ++t) {
            const int j = part_idx[o + t];
            if (j < 0) break;
            const float s = part_val[o + t];
            if (!beats(s, j + col_base, lv[k - 1], li[k - 1])) break;      // the part is sorted: nothing after this one enters either
            list_insert(lv, li, k, s, j + col_base);
        }
    }
    for (int t = 0; t < k; ++t) {
        idx[(size_t)row * k + t] = li[t];
        val[(size_t)row * k + t] = lv[t];
    }
}

}  // namespace

int lpi_search_merge(int nq, int k, int nparts, const float* part_val, const int32_t* part_idx, int col_base, int accumulate, int32_t* idx, float* val,
                     hipStream_t s)
{
    LPI_LAUNCH(search_merge_kernel, dim3((nq + 63) / 64), dim3(64), 0, s, nq, k, nparts, part_val, part_idx, col_base, accumulate, idx, val);
    LPI_CHECK_LAST();
    return 0;
}

// An upper bound of what the launches use (search_blocks, search_tile.h): the two lists of k pairs that every row of every block leaves.
extern "C" long lpi_search_workspace(int nq, int ng, int k)
{
    if (nq <= 0 || ng <= 0 || k < 0 || k > KMAX) return LPI_EINVAL;
    if (k == 0) return 8L * nq;      // thr f32 [nq] | gstar int32 [nq]
    return search_blocks(nq, ng) * BM * 2 * k * 8;
}

extern "C" int lpi_search_topk(int nq, int ng, int E, const float* Q, int ldq, const float* G, int ldg, int k, int col_base, int accumulate,
                               int32_t* idx, float* val, void* ws, long ws_bytes, void* stream)
{
    return search_topk<float, MODE_TOPK>(SearchCall{.nq = nq, .ng = ng, .E = E, .Q = Q, .ldq = ldq, .G = G, .ldg = ldg, .k = k, .col_base = col_base,
                                                    .accumulate = accumulate, .idx = idx, .val = val, .ws = ws, .ws_bytes = ws_bytes, .stream = stream});
}

extern "C" int lpi_search_rank(int nq, int ng, int E, const float* Q, int ldq, const float* G, int ldg, const int32_t* gt, int gt_per_row,
                               int32_t* rank, void* ws, long ws_bytes, void* stream)
{
    return search_rank<float>(SearchCall{.nq = nq, .ng = ng, .E = E, .Q = Q, .ldq = ldq, .G = G, .ldg = ldg, .gt = gt, .gt_per_row = gt_per_row,
                                         .rank = rank, .ws = ws, .ws_bytes = ws_bytes, .stream = stream});
}
