// Streamed search, wide lists: the k best gallery rows of every query row for k up to 256 in ONE sweep of the gallery, for every operand type.
//
//   lpi_search_topk_wide / _wide_t / _wide_mx8: what lpi_search_topk / _t / _mx8 give, with 1 <= k <= 256 (_wide_mx4: search_mx4.hip, the same code)
//
// The scores are the narrow kernels', bit for bit: the sweep is search_tile.h's kernel (same tile, staging, accumulator chain and masking) with another
// epilogue, MODE_WIDE.  Keeping a sorted list of 256 per row in LDS is out of reach (64 rows x 256 x 8 bytes per wave), so the selection is lazy:
//  * per tile row the workgroup keeps a threshold, the row's current k-th best (value, index), and a fill counter in LDS (1.5 KB beside the staging
//    buffers: two workgroups per CU as before);
//  * a score that `beats` the threshold is appended, unordered, to the (split, row) candidate buffer in the workspace: wide_cap(k) = 256 or 512 pairs,
//    at least k + one tile's columns;
//  * when the next tile could overflow a buffer, one wave sorts it in registers (a bitonic network over `beats`, 4 or 8 pairs per lane), keeps the k
//    best and raises the threshold; after the first few tiles a row sees about k (1 + ln(columns / k)) appends in all, so this is rare;
//  * after its last tile every buffer is selected once more: its first k pairs are the split's sorted list;
//  * the merge kernel (one wave per query row) folds the lists of all splits, and the held list when accumulating, into idx / val: two sorted lists of
//    256 are merged by taking the better of a[i] and b[255 - i], which are the 256 best as a bitonic sequence, and one merge level.
// The order is total, so the lists are unique: they do not depend on the order of the appends, the split count or the chunking.  Two launches per call.
#include "search_tile.h"

namespace {

constexpr int MERGE_ROWS = 4;      // waves (= query rows) per merge workgroup

__global__ __launch_bounds__(64 * MERGE_ROWS) void search_wide_merge_kernel(int nq, int k, int nparts, int cap, const float* __restrict__ part_val,
                                                                            const int32_t* __restrict__ part_idx, int col_base, int accumulate,
                                                                            int32_t* idx, float* val)
{
    constexpr int R = KWIDE / 64;
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * MERGE_ROWS + (threadIdx.x >> 6);
    if (row >= nq) return;
    float v[R];      // pair i = lane * R + r of the row's list so far, sorted
    int x[R];
#pragma unroll
    for (int r = 0; r < R; ++r) { v[r] = -INFINITY; x[r] = -1; }
    if (accumulate) {      // the held list need not be sorted; its entries with idx < 0 are empty
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const int i = lane * R + r;
            const int j = i < k ? idx[(size_t)row * k + i] : -1;
            if (j >= 0) { v[r] = val[(size_t)row * k + i]; x[r] = j; }
        }
        wide_sort<R>(v, x, lane);
    }
    for (int p = 0; p < nparts; ++p) {
        const size_t o = ((size_t)p * nq + row) * cap;
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const int i = KWIDE - 1 - (lane * R + r);      // the part backwards
            const int j = i < k ? part_idx[o + i] : -1;
            if (j >= 0) {
                const float s = part_val[o + i];
                if (beats(s, j + col_base, v[r], x[r])) { v[r] = s; x[r] = j + col_base; }
            }
        }
        wide_pass<R>(v, x, lane, KWIDE);
    }
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const int i = lane * R + r;
        if (i < k) { idx[(size_t)row * k + i] = x[r]; val[(size_t)row * k + i] = v[r]; }
    }
}

}  // namespace

// the launch of search_wide_merge_kernel (search_tile.h's search_topk<T, MODE_WIDE> calls it from every object that instantiates a wide sweep)
int lpi_search_wide_merge(int nq, int k, int nparts, int cap, const float* part_val, const int32_t* part_idx, int col_base, int accumulate, int32_t* idx,
                          float* val, hipStream_t s)
{
    LPI_LAUNCH(search_wide_merge_kernel, dim3((nq + MERGE_ROWS - 1) / MERGE_ROWS), dim3(64 * MERGE_ROWS), 0, s, nq, k, nparts, cap, part_val, part_idx,
               col_base, accumulate, idx, val);
    LPI_CHECK_LAST();
    return 0;
}

// An upper bound of what the launches use (search_blocks, search_tile.h): one candidate buffer for every row of every block.
extern "C" long lpi_search_wide_workspace(int nq, int ng, int k)
{
    if (nq <= 0 || ng <= 0 || k < 1 || k > KWIDE) return LPI_EINVAL;
    return search_blocks(nq, ng) * BM * wide_cap(k) * 8;
}

// the f32 form is the typed one at LPI_F32: the three wide sweeps of the plain types are instantiated here, once
extern "C" int lpi_search_topk_wide_t(int dt, int nq, int ng, int E, const void* Q, int ldq, const void* G, int ldg, int k, int col_base, int accumulate,
                                      int32_t* idx, float* val, void* ws, long ws_bytes, void* stream)
{
    const SearchCall c{.nq = nq, .ng = ng, .E = E, .Q = Q, .ldq = ldq, .G = G, .ldg = ldg, .k = k, .col_base = col_base, .accumulate = accumulate, .idx = idx,
                       .val = val, .ws = ws, .ws_bytes = ws_bytes, .stream = stream};
    return search_pick(PlainTypes{}, dt, [&](auto t) { return search_topk<type_of<decltype(t)>, MODE_WIDE>(c); });
}

extern "C" int lpi_search_topk_wide(int nq, int ng, int E, const float* Q, int ldq, const float* G, int ldg, int k, int col_base, int accumulate,
                                    int32_t* idx, float* val, void* ws, long ws_bytes, void* stream)
{
    return lpi_search_topk_wide_t(LPI_F32, nq, ng, E, Q, ldq, G, ldg, k, col_base, accumulate, idx, val, ws, ws_bytes, stream);
}

extern "C" int lpi_search_topk_wide_mx8(int nq, int ng, int E, const void* Q, int ldq, const void* q_scales, int ldqs, const void* G, int ldg,
                                        const void* g_scales, int ldgs, int k, int col_base, int accumulate, int32_t* idx, float* val, void* ws,
                                        long ws_bytes, void* stream)
{
    return search_topk<mx8_t, MODE_WIDE>(SearchCall{.nq = nq, .ng = ng, .E = E, .Q = Q, .ldq = ldq, .G = G, .ldg = ldg, .sc = {q_scales, ldqs, g_scales, ldgs},
                                                    .k = k, .col_base = col_base, .accumulate = accumulate, .idx = idx, .val = val, .ws = ws, .ws_bytes = ws_bytes,
                                                    .stream = stream});
}
