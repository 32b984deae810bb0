// Streamed search, second stage: exact scores of a short candidate list per query row, and the k best of them.
//
//   lpi_search_rerank / _rerank_t: for query row i the candidates cand[i, 0..kc) (gallery row indices, kc <= 256) are scored against Q[i, :] and the k
//   best distinct ones go to idx / val [nq, k] in lpi_topk's order (value descending, then index descending; unfilled slots (-1, -inf) last)
//
// A coarse sweep (bf16 / MX-FP8 operands, search_tile.h) that over-fetches a little, then this call on the f32 rows, gives the f32 sweep's lists at close
// to the coarse sweep's cost: neither `score_matrix` (the nq x ng matrix) nor the rank call's gathered launch (a 128 x 128 tile per diagonal) fits.
//
// Design:
//  * one wave per query row, four per workgroup, one launch; no LDS memory, no workspace;
//  * a score has the bits the sweeps of search_tile.h give the same (query row, gallery row): the same instruction (mma_chunk<T>: gallery rows its
//    first operand, the query row its second), the same accumulator chain from zero over K in the same order.  The sweep's slab loop (kt, then ks = 0, 1,
//    the last slab shortened to ks = 0 when E % BK == BK / 2) visits, for lane group g = lane >> 4, the 16-byte piece at element j * (BK / 2) + g * EPC
//    for j = 0 .. E / (BK / 2) - 1: that is the loop below;
//  * a sub tile is 16 gathered candidate rows (lane l supplies row l & 15, piece g, straight from global memory: 16 lanes x 64 contiguous bytes); the
//    second operand carries the query row in all 16 columns (the lanes of a group read the same 16 bytes), so 1/16 of the instruction's work is wanted:
//    at 5 000 x 256 x 512 about 21 GFLOP on the pipe against the sweep's 128.  Every column of the result is the same: lane (g, c) holds the scores of
//    the sub tile's candidates 4g .. 4g + 3 whatever its column c, and keeps them from sub tile t == c.  After 16 sub tiles lane l holds candidates
//    16 (l & 15) + 4 (l >> 4) + 0..3: every candidate once, 4 per lane;
//  * up to four sub tiles run together (independent accumulators); the count follows kc, so kc = 20 costs two sub tiles, not sixteen;
//  * an entry outside [0, ng) and a slot past kc are padding: the row read in their place is row 0, their pair is (-inf, -1) by a select, never by
//    arithmetic, and cand is not read past kc;
//  * the 256 pairs are sorted with the bitonic network of search_tile.h (wide_sort<4>).  A repeated index carries the same score bits, so its copies
//    are adjacent after the sort: all but the first are dropped, a ballot per register gives every kept pair its place, the rest of the row is filled.
#include "search_tile.h"

namespace {

constexpr int RR_ROWS = 4;      // waves (= query rows) per workgroup

// U sub tiles, t0 .. t0 + U - 1, of the row's candidates: lane (g, c) leaves the scores of sub tile t == c in v[0..3] (candidates 16 t + 4 g + 0..3)
template <typename T, int U>
__device__ __forceinline__ void rerank_subtiles(int t0, int ng, int steps, const T* qp, const T* __restrict__ G, int ldg, const int32_t* crow, int kc,
                                                int g, int r16, float (&v)[4])
{
    constexpr int EPC = Elem<T>::EPC;
    constexpr int HALF = 4 * EPC;      // the k-values of one k step: half a slab
    const T* gp[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
        const int slot = (t0 + u) * 16 + r16;
        int c = slot < kc ? crow[slot] : -1;
        if ((unsigned)c >= (unsigned)ng) c = 0;      // padding: row 0 in its place, the score is never looked at
        gp[u] = G + (size_t)c * ldg + g * EPC;
    }
    f32x4 acc[U];
#pragma unroll
    for (int u = 0; u < U; ++u) acc[u] = f32x4{0.f, 0.f, 0.f, 0.f};
    // the pieces of step j + 1 are asked for before the instructions of step j (the last step asks for its own again: inside the rows)
    Chunk fq, fg[U];
    fq.u = *reinterpret_cast<const uint4*>(qp);
#pragma unroll
    for (int u = 0; u < U; ++u) fg[u].u = *reinterpret_cast<const uint4*>(gp[u]);
#pragma unroll 1
    for (int j = 0; j < steps; ++j) {
        const int jn = min(j + 1, steps - 1) * HALF;
        Chunk nq, nx[U];
        nq.u = *reinterpret_cast<const uint4*>(qp + jn);
#pragma unroll
        for (int u = 0; u < U; ++u) nx[u].u = *reinterpret_cast<const uint4*>(gp[u] + jn);
#pragma unroll
        for (int u = 0; u < U; ++u) mma_chunk<T>(acc[u], fg[u], fq);
        fq = nq;
#pragma unroll
        for (int u = 0; u < U; ++u) fg[u] = nx[u];
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
        if (t0 + u == r16) {
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] = acc[u][e];
        }
    }
}

template <typename T>
__global__ __launch_bounds__(64 * RR_ROWS) void search_rerank_kernel(int nq, int ng, int E, const T* __restrict__ Q, int ldq, const T* __restrict__ G,
                                                                     int ldg, const int32_t* __restrict__ cand, int ldc, int kc, int k, int32_t* idx,
                                                                     float* val)
{
    constexpr int EPC = Elem<T>::EPC;
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * RR_ROWS + (threadIdx.x >> 6);
    if (row >= nq) return;      // the whole wave: there is no barrier below
    const int g = lane >> 4, r16 = lane & 15;
    const int32_t* crow = cand + (size_t)row * ldc;
    const T* qp = Q + (size_t)row * ldq + g * EPC;
    const int steps = E / (4 * EPC);

    float v[4];
    int x[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = -INFINITY;
    const int nsub = (kc + 15) >> 4;
    int t = 0;
#pragma unroll 1
    for (; t + 4 <= nsub; t += 4) rerank_subtiles<T, 4>(t, ng, steps, qp, G, ldg, crow, kc, g, r16, v);
    if (t + 2 <= nsub) {
        rerank_subtiles<T, 2>(t, ng, steps, qp, G, ldg, crow, kc, g, r16, v);
        t += 2;
    }
    if (t < nsub) rerank_subtiles<T, 1>(t, ng, steps, qp, G, ldg, crow, kc, g, r16, v);
    // the pairs this lane holds: candidates 16 r16 + 4 g + e
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const int slot = 16 * r16 + 4 * g + e;
        const int c = slot < kc ? crow[slot] : -1;
        const bool ok = (unsigned)c < (unsigned)ng;
        x[e] = ok ? c : -1;
        v[e] = ok ? v[e] : -INFINITY;
    }

    wide_sort<4>(v, x, lane);      // pair i = lane * 4 + r, descending in `beats`; the empty pairs last

    // the copies of an index are adjacent: keep the first
    const int px = __shfl_up(x[3], 1, 64);
    bool keep[4];
    keep[0] = x[0] >= 0 && (lane == 0 || x[0] != px);
#pragma unroll
    for (int r = 1; r < 4; ++r) keep[r] = x[r] >= 0 && x[r] != x[r - 1];
    const unsigned long long below = (1ull << lane) - 1;
    int pos = 0, total = 0;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const unsigned long long b = __ballot(keep[r]);
        pos += __popcll(b & below);
        total += __popcll(b);
    }
    int32_t* orow_i = idx + (size_t)row * k;
    float* orow_v = val + (size_t)row * k;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        if (keep[r]) {
            if (pos < k) { orow_i[pos] = x[r]; orow_v[pos] = v[r]; }
            ++pos;
        }
    }
    for (int p = total + lane; p < k; p += 64) { orow_i[p] = -1; orow_v[p] = -INFINITY; }
}

template <typename T>
int search_rerank(const SearchCall& c)
{
    if (int e = search_check<T>(c)) return e;
    if (!rerank_ok(c)) return LPI_EINVAL;
    LPI_LAUNCH(search_rerank_kernel<T>, dim3((c.nq + RR_ROWS - 1) / RR_ROWS), dim3(64 * RR_ROWS), 0, (hipStream_t)c.stream, c.nq, c.ng, c.E, (const T*)c.Q,
               c.ldq, (const T*)c.G, c.ldg, c.cand, c.ldc, c.kc, c.k, c.idx, c.val);
    LPI_CHECK_LAST();
    return 0;
}

}  // namespace

// the f32 form is the typed one at LPI_F32: the three kernels are instantiated here, once
extern "C" int lpi_search_rerank_t(int dt, int nq, int ng, int E, const void* Q, int ldq, const void* G, int ldg, const int32_t* cand, int ldc, int kc,
                                   int k, int32_t* idx, float* val, void* stream)
{
    const SearchCall c{.nq = nq, .ng = ng, .E = E, .Q = Q, .ldq = ldq, .G = G, .ldg = ldg, .k = k, .idx = idx, .val = val, .cand = cand, .ldc = ldc, .kc = kc,
                       .stream = stream};
    return search_pick(PlainTypes{}, dt, [&](auto t) { return search_rerank<type_of<decltype(t)>>(c); });
}

extern "C" int lpi_search_rerank(int nq, int ng, int E, const float* Q, int ldq, const float* G, int ldg, const int32_t* cand, int ldc, int kc, int k,
                                 int32_t* idx, float* val, void* stream)
{
    return lpi_search_rerank_t(LPI_F32, nq, ng, E, Q, ldq, G, ldg, cand, ldc, kc, k, idx, val, stream);
}
