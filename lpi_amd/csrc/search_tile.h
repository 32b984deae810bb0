// The tile code of the streamed search and the host layer of the whole family (at the end), for an operand type T: float (search.hip), bf16_t / f16_t (search16.hip),
// mx8_t (search_mx8.hip: e4m3 bytes + one E8M0 scale per 32 elements, mx8.h) or mx4_t (search_mx4.hip: e2m1 nibbles + the same scales, mx4.h; top-k only).
//
// Design:
//  * the main loop is gemm.hip's: 128x128 tile, 4 waves as 2x2, K-contiguous operands staged one 128-byte row piece (BK = 32 f32 / 64 2-byte k-values) at
//    a time by `global_load_lds_dwordx4`, double buffered, swizzled on the source address; f32: exact products on v_mfma_f32_16x16x4_f32, 2-byte: exact
//    products of the 2-byte values on v_mfma_f32_16x16x32_bf16 / _f16, f32 accumulators.  Every score is one accumulator chain over K in a fixed order, so
//    its bits depend on its two rows only: not on the tile position, the gallery split or the chunking;
//  * a workgroup owns 128 query rows and walks the gallery tiles of its split; the query block is re-staged from L2 with every gallery tile (at E = 1024
//    it would be 512 KB of LDS in f32).  The staging of the next tile's first K slab is issued before the epilogue of the current one;
//  * edges: a staged row past the end of an operand is the operand's last row again, a staged 16-byte piece past E (E % BK == BK / 2, last slab) is a
//    piece of the same slab below E and is never read from LDS: nothing outside the n x E elements is read; scores of such rows / columns are masked;
//  * rank: a first launch of the same tile code over the ground-truth rows GATHERED by index (tile p, column c = ground truth p of query row c) leaves the
//    threshold scores on the tiles' diagonals, with the bits the sweep computes for those columns; the sweep keeps one counter per owned row in registers
//    and ends with one reduction and one integer atomicAdd per (row, workgroup);
//  * MX-FP8 (T = mx8_t, everything under `if constexpr (kIsMx8<T>)`): a staged 128-byte row piece is 128 elements = ONE v_mfma_scale_f32_16x16x128_f8f6f4's
//    K, so a slab is one k step and E is a multiple of 128: the two ds_read_b128 of a lane per sub tile (chunks g and 4 + g) are the instruction's eight
//    operand registers.  The scale bytes of a slab, 4 per tile row, are staged behind the element tiles of the stage (2 x 512 B) by one
//    global_load_lds of a dword per lane (waves 0, 1 the query rows, waves 2, 3 the gallery rows: clamped or gathered by the same row index as the
//    elements) and read back with ds_read_u8 at row * 4 + (l >> 4): the register a lane hands the instruction holds the scale of row l & 15, K block
//    l >> 4 (gemm_mx8.hip has the measured operand map).  Gallery = the instruction's first operand, queries its second, as mma_chunk's: the lane ends
//    with the same acc[n][m], and the epilogues below are the same lines for every type;
//  * MX-FP4 (T = mx4_t, everything under `if constexpr (kIsMx4<T>)`): the element is a BYTE of two nibbles and SearchArgs::E the row length in bytes, so
//    staging, swizzle, the edges and the shortened last slab (E % 256 == 128 elements) are the 1-byte type's lines.  A staged 128-byte row piece is 256
//    elements = TWO instructions' K: a slab is two k steps, and step ks reads ONE ds_read_b128 per lane and sub tile, chunk 4 ks + g, the 32 consecutive
//    elements the instruction wants from that lane (mx4.h has the measured operand map; MX-FP8 reads chunks g and 4 + g of one step).  A slab has 8 scale
//    bytes per tile row: two global_load_lds of a dword per lane (global_load_lds has no 8-byte form), step-major behind the element tiles,
//    [operand][step][row][4 bytes] = 4 x 512 B per stage, read back with ds_read_u8 at step * 512 + row * 4 + g; the second dword of a shortened last slab
//    lies past the row's scales and is staged from the first again, never read.  No rank form;
//  * top-k: every wave keeps a sorted list per row of its 64x64 quadrant's columns in LDS; scores are compared in registers with the row's current k-th
//    and only survivors are inserted (the four lanes that share a row take turns).  Per-(split, wave column) lists go to the workspace, the merge
//    kernel (search.hip, one for every operand type: it sees f32 scores only) writes idx / val;
//  * wide top-k (MODE_WIDE, k <= 256, instantiated by search_wide.hip, where the design is described): the same main loop and masks; scores that beat a
//    row's threshold are appended to a candidate buffer in the workspace and a wave selects the k best with a bitonic network in registers.
#pragma once
#include "dispatch.h"
#include "mx8.h"
#include "mx4.h"
#include <math.h>

// search.hip: the launch of search_merge_kernel, the partial lists (and, with accumulate, the list idx / val already hold) -> idx / val
int lpi_search_merge(int nq, int k, int nparts, const float* part_val, const int32_t* part_idx, int col_base, int accumulate, int32_t* idx, float* val,
                     hipStream_t s);

// search_wide.hip: the launch of search_wide_merge_kernel, the splits' sorted lists in the candidate buffers (and, with accumulate, the held list) -> idx / val
int lpi_search_wide_merge(int nq, int k, int nparts, int cap, const float* part_val, const int32_t* part_idx, int col_base, int accumulate, int32_t* idx,
                          float* val, hipStream_t s);

namespace {

constexpr int BM = 128, BN = 128;
constexpr int ROW_BYTES = 128;
constexpr int TILE_BYTES = BM * ROW_BYTES;
constexpr int STAGE_BYTES = 2 * TILE_BYTES;
constexpr int SCALE_BYTES = BM * 4;      // MX-FP8: the scale bytes of one operand's tile rows for one slab
template <typename T> inline constexpr bool kHasScales = kIsMx8<T> || kIsMx4<T>;
template <typename T> inline constexpr int kScaleOperandBytes = kIsMx4<T> ? 2 * SCALE_BYTES : SCALE_BYTES;      // MX-FP4: two k steps per slab
template <typename T> inline constexpr int kStageBytes = STAGE_BYTES + (kHasScales<T> ? 2 * kScaleOperandBytes<T> : 0);
constexpr int NTHREADS = 256;
constexpr int KMAX = 16;
constexpr int WG_TARGET = 512;      // workgroups wanted per launch: two per CU of an MI355X
constexpr int MODE_TOPK = 0, MODE_RANK = 1, MODE_THRESH = 2, MODE_WIDE = 3;
constexpr int KWIDE = 256;          // MODE_WIDE (search_wide.hip): lists up to this k
// MODE_WIDE: the capacity of a (split, row) candidate buffer: >= k + one tile's columns, 64 lanes x 4 or 8 registers of the selecting wave
__host__ __device__ constexpr int wide_cap(int k) { return k <= 128 ? 256 : 512; }

template <typename T>
struct SearchArgs {
    int nq, ng, E;
    const T* Q;
    int ldq;
    const T* G;
    int ldg;
    int k, tiles, splits;
    const int32_t* gt;
    int gpr;
    float* thr;          // [nq] threshold score of the best ground-truth column (+inf: none)
    int32_t* gstar;      // [nq] its index (-1: none)
    int32_t* rank;
    float* part_val;     // [2 * splits][nq][k]; MODE_WIDE: the candidate buffers [splits][nq][wide_cap(k)], whose first k end as the split's sorted list
    int32_t* part_idx;
};

// MX-FP8 operands carry their scale arrays ([rows, E/32] bytes with a leading dimension) beside the element pointers
template <>
struct SearchArgs<mx8_t> {
    int nq, ng, E;
    const mx8_t* Q;
    int ldq;
    const mx8_t* G;
    int ldg;
    int k, tiles, splits;
    const int32_t* gt;
    int gpr;
    float* thr;
    int32_t* gstar;
    int32_t* rank;
    float* part_val;
    int32_t* part_idx;
    const uint8_t* Qs;
    int ldqs;
    const uint8_t* Gs;
    int ldgs;
};
// MX-FP4: the same, with E, ldq and ldg in BYTES (two elements each): the kernel's element is the byte
template <>
struct SearchArgs<mx4_t> {
    int nq, ng, E;
    const mx4_t* Q;
    int ldq;
    const mx4_t* G;
    int ldg;
    int k, tiles, splits;
    const int32_t* gt;
    int gpr;
    float* thr;
    int32_t* gstar;
    int32_t* rank;
    float* part_val;
    int32_t* part_idx;
    const uint8_t* Qs;
    int ldqs;
    const uint8_t* Gs;
    int ldgs;
};
struct SearchScales {      // what the host calls take for them (E8M0 bytes); unused by the other types
    const void* q; int ldq;
    const void* g; int ldg;
};

// (s, j) before (v, i) in the order value descending, then index descending
__device__ __forceinline__ bool beats(float s, int j, float v, int i) { return s > v || (s == v && j > i); }

// one lane inserts into a sorted list of k
typedef __attribute__((address_space(3))) volatile float lds_f32;
typedef __attribute__((address_space(3))) volatile int lds_i32;
__device__ __forceinline__ void list_insert(lds_f32* lv, lds_i32* li, int k, float s, int j) {
    if (!beats(s, j, lv[k - 1], li[k - 1])) return;
    int p = k - 1;
    while (p > 0) {
        const float pv = lv[p - 1];
        const int pi = li[p - 1];
        if (!beats(s, j, pv, pi)) break;
        lv[p] = pv;
        li[p] = pi;
        --p;
    }
    lv[p] = s;
    li[p] = j;
}

// ---- MODE_WIDE: a wave sorts 64 R (value, index) pairs in registers with a bitonic network over `beats` (a total order: the result is unique; the empty
// pairs (-inf, -1) are equal to each other only and come last).  Element i = lane * R + r: distances below R are exchanges between a lane's own registers
// (static indices: no scratch), the others a lane exchange (ds_bpermute: no LDS memory)
template <int R>
__device__ __forceinline__ void wide_pass(float (&v)[R], int (&x)[R], int lane, int k2)      // one merge level: blocks of k2, distances k2 / 2 .. 1
{
    constexpr int LOGR = R == 8 ? 3 : 2;
    static_assert(R == 4 || R == 8, "wide_pass: 4 or 8 elements per lane");
#pragma unroll 1
    for (int j = k2 >> 1; j >= R; j >>= 1) {
        const int lj = j / R;
        const bool lower = (lane & lj) == 0;
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const bool desc = ((lane * R + r) & k2) == 0;      // a descending block: its lower element keeps the better pair
            const float pv = __shfl_xor(v[r], lj, 64);
            const int px = __shfl_xor(x[r], lj, 64);
            const bool pb = beats(pv, px, v[r], x[r]);
            const bool take = lower == desc ? pb : !pb;
            v[r] = take ? pv : v[r];
            x[r] = take ? px : x[r];
        }
    }
#pragma unroll
    for (int jb = LOGR - 1; jb >= 0; --jb) {
        const int j = 1 << jb;
        if (j < k2) {
#pragma unroll
            for (int r = 0; r < R; ++r) {
                if ((r & j) == 0) {
                    const int r2 = r | j;
                    const bool desc = ((lane * R + r) & k2) == 0;
                    const bool b = beats(v[r2], x[r2], v[r], x[r]);
                    const bool sw = desc ? b : !b;
                    const float fv = v[r];
                    const int fx = x[r];
                    v[r] = sw ? v[r2] : fv;
                    x[r] = sw ? x[r2] : fx;
                    v[r2] = sw ? fv : v[r2];
                    x[r2] = sw ? fx : x[r2];
                }
            }
        }
    }
}
template <int R>
__device__ __forceinline__ void wide_sort(float (&v)[R], int (&x)[R], int lane)      // descending in `beats`
{
#pragma unroll 1
    for (int k2 = 2; k2 <= 64 * R; k2 <<= 1) wide_pass<R>(v, x, lane, k2);
}

// a wave brings the n candidates of a row down to its k best, sorted, in cv / ci [0, k) (a short list ends with (-inf, -1)) -> the k-th pair (tv, ti)
template <int R>
__device__ __forceinline__ void wide_select(float* cv, int32_t* ci, int n, int k, int lane, float& tv, int& ti)
{
    float v[R];
    int x[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const int i = lane * R + r;
        v[r] = i < n ? cv[i] : -INFINITY;
        x[r] = i < n ? ci[i] : -1;
    }
    wide_sort<R>(v, x, lane);
    float kv = -INFINITY;
    int ki = -1;
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const int i = lane * R + r;
        if (i < k) { cv[i] = v[r]; ci[i] = x[r]; }
        if (i == k - 1) { kv = v[r]; ki = x[r]; }
    }
    tv = __shfl(kv, (k - 1) / R, 64);
    ti = __shfl(ki, (k - 1) / R, 64);
}

template <typename T, int MODE>
__global__ __launch_bounds__(NTHREADS, 2) void search_kernel(SearchArgs<T> a)
{
    constexpr int EPC = Elem<T>::EPC;                      // elements per 16-byte piece
    constexpr int BK = ROW_BYTES / (int)sizeof(T);         // k-values per slab: two k steps of 4 pieces each (MX-FP8: one step of 8)
    constexpr int STAGE = kStageBytes<T>;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1;
    const int g = lane >> 4, r16 = lane & 15;
    const int m0 = blockIdx.x * BM;
    int t_begin = 0, t_end = a.gpr;      // MODE_THRESH: tile p = the p-th ground-truth row of each query row
    if constexpr (MODE != MODE_THRESH) {
        t_begin = (int)((long)blockIdx.y * a.tiles / a.splits);
        t_end = (int)((long)(blockIdx.y + 1) * a.tiles / a.splits);
    }
    const int nk = (a.E + BK - 1) / BK;
    const int ks_last = (a.E & (BK - 1)) ? 1 : 2;      // k steps of the last slab

    // ---- staging (gemm.hip): thread t, instruction i writes LDS byte i*4096 + t*16 of a tile; row = i*32 + t/8, logical chunk = (t%8) ^ ((row>>1)&7)
    const int srow = tid >> 3;
    const int schunk = (tid & 7) ^ (((wave & 1) << 2) | (lane >> 4));
    const T* qp[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) qp[i] = a.Q + (size_t)min(m0 + srow + 32 * i, a.nq - 1) * a.ldq;

    auto stage = [&](int tile, int kt, int buf) {
        char* base = smem + buf * STAGE + wave * 1024;
        int koff = kt * BK + schunk * EPC;
        if (koff >= a.E) koff -= BK / 2;      // the dead half of the last slab: staged from below E, never read
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(qp[i] + koff),
                                             (__attribute__((address_space(3))) void*)(base + i * 4096), 16, 0, 0);
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            int gr;
            if constexpr (MODE == MODE_THRESH) {
                const int q = m0 + srow + 32 * i;
                gr = q < a.nq ? a.gt[(size_t)q * a.gpr + tile] : -1;
                if ((unsigned)gr >= (unsigned)a.ng) gr = 0;
            } else {
                gr = min(tile * BN + srow + 32 * i, a.ng - 1);
            }
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(a.G + (size_t)gr * a.ldg + koff),
                                             (__attribute__((address_space(3))) void*)(base + TILE_BYTES + i * 4096), 16, 0, 0);
        }
        if constexpr (kHasScales<T>) {      // the slab's scales: lane = tile row (wave & 1) * 64 + lane of the queries (waves 0, 1) / the gallery (waves 2, 3)
            const int r = (wave & 1) * 64 + lane;
            const uint8_t* sp;
            if (wave < 2) {
                sp = a.Qs + (size_t)min(m0 + r, a.nq - 1) * a.ldqs;
            } else {
                int gr;
                if constexpr (MODE == MODE_THRESH) {
                    const int q = m0 + r;
                    gr = q < a.nq ? a.gt[(size_t)q * a.gpr + tile] : -1;
                    if ((unsigned)gr >= (unsigned)a.ng) gr = 0;
                } else {
                    gr = min(tile * BN + r, a.ng - 1);
                }
                sp = a.Gs + (size_t)gr * a.ldgs;
            }
            if constexpr (kIsMx4<T>) {      // 8 bytes per row: step 0's dword, then step 1's (a row has E / 16 scale bytes; past them: step 0's again)
                char* dst = smem + buf * STAGE + 2 * TILE_BYTES + (wave >> 1) * 2 * SCALE_BYTES + (wave & 1) * 256;
                const int s0 = kt * 8, s1 = s0 + 4 < (a.E >> 4) ? s0 + 4 : s0;
                __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(sp + s0),
                                                 (__attribute__((address_space(3))) void*)dst, 4, 0, 0);
                __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(sp + s1),
                                                 (__attribute__((address_space(3))) void*)(dst + SCALE_BYTES), 4, 0, 0);
            } else {
                __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(sp + kt * 4),
                                                 (__attribute__((address_space(3))) void*)(smem + buf * STAGE + 2 * TILE_BYTES + (wave >> 1) * SCALE_BYTES + (wave & 1) * 256), 4, 0, 0);
            }
        }
    };

    // ---- fragment read offsets: lane reads row (l&15) of a 16-row sub tile, logical chunk 4*ks + (l>>4)
    const int fsw = r16 >> 1;
    int foff[2];
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) foff[ks] = r16 * ROW_BYTES + (((ks << 2) | g) ^ fsw) * 16;
    const int a_frag_base = (wm * 64) * ROW_BYTES;               // query rows
    const int b_frag_base = TILE_BYTES + (wn * 64) * ROW_BYTES;  // gallery rows
    const int a_sc_base = 2 * TILE_BYTES + (wm * 64 + r16) * 4 + g;                // MX-FP8: the lane's scale byte of its first query / gallery row
    const int b_sc_base = 2 * TILE_BYTES + kScaleOperandBytes<T> + (wn * 64 + r16) * 4 + g;      // MX-FP4: + SCALE_BYTES for the slab's second step

    // ---- per-mode state.  A lane owns rows m0 + wm*64 + mi*16 + r16 (mi = 0..3) and, of each, columns wn*64 + ni*16 + 4g + 0..3 of the tile
    lds_f32* Lv = nullptr;      // MODE_TOPK: this wave's lists, [64 rows][k]
    lds_i32* Li = nullptr;
    int cnt[4] = {0, 0, 0, 0};         // MODE_RANK
    float tv[4];                       // MODE_RANK: thresholds; MODE_THRESH: best ground-truth score so far
    int ti[4];
#pragma unroll
    for (int mi = 0; mi < 4; ++mi) { tv[mi] = -INFINITY; ti[mi] = -1; }
    if constexpr (MODE == MODE_TOPK) {
        auto lists = (__attribute__((address_space(3))) char*)smem + 2 * STAGE + wave * (64 * a.k * 8);
        Lv = (lds_f32*)lists;
        Li = (lds_i32*)(lists + 64 * a.k * 4);
        for (int e = lane; e < 64 * a.k; e += 64) { Lv[e] = -INFINITY; Li[e] = -1; }
    }
    float* Wv = nullptr;        // MODE_WIDE: per tile row the k-th best pair so far (the threshold) and the fill of its candidate buffer
    int* Wi = nullptr;
    int* Wn = nullptr;
    if constexpr (MODE == MODE_WIDE) {
        Wv = reinterpret_cast<float*>(smem + 2 * STAGE);
        Wi = reinterpret_cast<int*>(smem + 2 * STAGE + BM * 4);
        Wn = reinterpret_cast<int*>(smem + 2 * STAGE + BM * 8);
        if (tid < BM) { Wv[tid] = -INFINITY; Wi[tid] = -1; Wn[tid] = 0; }      // seen by everyone after the first slab's barrier
    }
    if constexpr (MODE == MODE_RANK) {
#pragma unroll
        for (int mi = 0; mi < 4; ++mi) {
            const int row = m0 + wm * 64 + mi * 16 + r16;
            tv[mi] = row < a.nq ? a.thr[row] : INFINITY;
            ti[mi] = row < a.nq ? a.gstar[row] : -1;
        }
#pragma unroll
        for (int mi = 0; mi < 4; ++mi) asm volatile("" :: "v"(tv[mi]), "v"(ti[mi]));      // the loads are waited for here, not under the LDS-DMA
    }

    f32x4 acc[4][4];  // [n sub tile][m sub tile]
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

    int it = 0;
    if (t_begin < t_end) stage(t_begin, 0, 0);
    for (int tile = t_begin; tile < t_end; ++tile) {
        for (int kt = 0; kt < nk; ++kt, ++it) {
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // this wave's LDS-DMA of slab `it` has landed
            __syncthreads();                                  // ... and everyone's; buffer (it+1)&1 is free again
            if (kt + 1 < nk) stage(tile, kt + 1, (it + 1) & 1);
            else if (tile + 1 < t_end) stage(tile + 1, 0, (it + 1) & 1);
            const char* buf = smem + (it & 1) * STAGE;
            if constexpr (kIsMx8<T>) {
                Chunk fa[4][2], fb[4][2];
                int sa[4], sb[4];
#pragma unroll
                for (int i = 0; i < 4; ++i) {
#pragma unroll
                    for (int ks = 0; ks < 2; ++ks) {
                        fa[i][ks].u = *reinterpret_cast<const uint4*>(buf + a_frag_base + i * 16 * ROW_BYTES + foff[ks]);
                        fb[i][ks].u = *reinterpret_cast<const uint4*>(buf + b_frag_base + i * 16 * ROW_BYTES + foff[ks]);
                    }
                    sa[i] = *reinterpret_cast<const uint8_t*>(buf + a_sc_base + i * 64);      // rows 16 apart are 64 bytes apart
                    sb[i] = *reinterpret_cast<const uint8_t*>(buf + b_sc_base + i * 64);
                }
#pragma unroll
                for (int ni = 0; ni < 4; ++ni)
#pragma unroll
                    for (int mi = 0; mi < 4; ++mi)
                        mx8_mma(acc[ni][mi], mx8_operand(fb[ni][0], fb[ni][1]), mx8_operand(fa[mi][0], fa[mi][1]), 0, sb[ni], 0, sa[mi]);
                // hipcc sinks block-scaled instructions past barriers (gemm256_tile.h): an empty statement that "uses" the accumulators keeps them in their slab
#pragma unroll
                for (int ni = 0; ni < 4; ++ni) asm volatile("" : "+v"(acc[ni][0]), "+v"(acc[ni][1]), "+v"(acc[ni][2]), "+v"(acc[ni][3]));
            } else if constexpr (kIsMx4<T>) {
                const int nks = kt == nk - 1 ? ks_last : 2;
#pragma unroll
                for (int ks = 0; ks < 2; ++ks) {
                    if (ks < nks) {
                        Chunk fa[4], fb[4];
                        int sa[4], sb[4];
#pragma unroll
                        for (int i = 0; i < 4; ++i) {
                            fa[i].u = *reinterpret_cast<const uint4*>(buf + a_frag_base + i * 16 * ROW_BYTES + foff[ks]);
                            fb[i].u = *reinterpret_cast<const uint4*>(buf + b_frag_base + i * 16 * ROW_BYTES + foff[ks]);
                            sa[i] = *reinterpret_cast<const uint8_t*>(buf + a_sc_base + ks * SCALE_BYTES + i * 64);
                            sb[i] = *reinterpret_cast<const uint8_t*>(buf + b_sc_base + ks * SCALE_BYTES + i * 64);
                        }
#pragma unroll
                        for (int ni = 0; ni < 4; ++ni)
#pragma unroll
                            for (int mi = 0; mi < 4; ++mi) mx4_mma(acc[ni][mi], fb[ni], fa[mi], sb[ni], sa[mi]);
#pragma unroll
                        for (int ni = 0; ni < 4; ++ni) asm volatile("" : "+v"(acc[ni][0]), "+v"(acc[ni][1]), "+v"(acc[ni][2]), "+v"(acc[ni][3]));      // as above
                    }
                }
            } else {
                const int nks = kt == nk - 1 ? ks_last : 2;
#pragma unroll
                for (int ks = 0; ks < 2; ++ks) {
                    if (ks < nks) {
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
        }

        // ---- the tile's scores are in acc: lane holds s[row = .. + mi*16 + r16][col = col0 + ni*16 + 0..3]
        const int col0 = tile * BN + wn * 64 + 4 * g;
        if constexpr (MODE == MODE_TOPK) {
#pragma unroll
            for (int mi = 0; mi < 4; ++mi) {
                lds_f32* lv = Lv + (mi * 16 + r16) * a.k;
                lds_i32* li = Li + (mi * 16 + r16) * a.k;
                const float kv = lv[a.k - 1];
                const int ki = li[a.k - 1];
                unsigned mask = 0;
#pragma unroll
                for (int ni = 0; ni < 4; ++ni)
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const int col = col0 + ni * 16 + e;
                        if (col < a.ng && beats(acc[ni][mi][e], col, kv, ki)) mask |= 1u << (ni * 4 + e);
                    }
                if (__ballot(mask != 0) == 0) continue;
#pragma unroll
                for (int ni = 0; ni < 4; ++ni)
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const bool want = mask & (1u << (ni * 4 + e));
                        if (__ballot(want) == 0) continue;
                        // the four lanes of a row (g = 0..3) take turns; lanes of one turn own different rows
#pragma unroll 1
                        for (int gp = 0; gp < 4; ++gp) {
                            if (want && g == gp) list_insert(lv, li, a.k, acc[ni][mi][e], col0 + ni * 16 + e);
                            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                            __builtin_amdgcn_wave_barrier();
                            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
                        }
                    }
            }
        } else if constexpr (MODE == MODE_RANK) {
#pragma unroll
            for (int mi = 0; mi < 4; ++mi)
#pragma unroll
                for (int ni = 0; ni < 4; ++ni)
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const int col = col0 + ni * 16 + e;
                        cnt[mi] += (col < a.ng && col != ti[mi] && beats(acc[ni][mi][e], col, tv[mi], ti[mi])) ? 1 : 0;
                    }
        } else if constexpr (MODE == MODE_WIDE) {
            // a score that beats its row's threshold is appended to the row's candidate buffer of this split (slot from the LDS counter: the order in
            // the buffer is arbitrary, the selection's result is not); the two waves of a row share the buffer
            const int cap = wide_cap(a.k);
#pragma unroll
            for (int mi = 0; mi < 4; ++mi) {
                const int rl = wm * 64 + mi * 16 + r16;
                const bool rowok = m0 + rl < a.nq;
                const float kv = Wv[rl];
                const int ki = Wi[rl];
                unsigned mask = 0;
#pragma unroll
                for (int ni = 0; ni < 4; ++ni)
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const int col = col0 + ni * 16 + e;
                        if (rowok && col < a.ng && beats(acc[ni][mi][e], col, kv, ki)) mask |= 1u << (ni * 4 + e);
                    }
                if (__ballot(mask != 0) == 0) continue;
                const size_t cb = ((size_t)blockIdx.y * a.nq + (rowok ? m0 + rl : 0)) * cap;
#pragma unroll
                for (int ni = 0; ni < 4; ++ni)
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        if (mask & (1u << (ni * 4 + e))) {
                            const int slot = atomicAdd(&Wn[rl], 1);      // < cap: the fill was <= cap - BN before this tile
                            a.part_val[cb + slot] = acc[ni][mi][e];
                            a.part_idx[cb + slot] = col0 + ni * 16 + e;
                        }
                    }
            }
            __syncthreads();      // the tile's appends are complete and visible to the workgroup
            // wave w looks after tile rows 32 w ..: a buffer that the next tile could overflow, and every buffer after the last tile, is brought down to
            // its k best (sorted: the final one is the part the merge kernel reads), which also raises the threshold
            const bool last = tile + 1 == t_end;
#pragma unroll 1
            for (int rr = 0; rr < BM / 4; ++rr) {
                const int rl = wave * (BM / 4) + rr;
                if (m0 + rl >= a.nq) break;
                const int n = __builtin_amdgcn_readfirstlane(Wn[rl]);
                if (!last && n + BN <= cap) continue;
                const size_t cb = ((size_t)blockIdx.y * a.nq + m0 + rl) * cap;
                float sv;
                int si;
                if (cap == 256) wide_select<4>(a.part_val + cb, a.part_idx + cb, n, a.k, lane, sv, si);
                else wide_select<8>(a.part_val + cb, a.part_idx + cb, n, a.k, lane, sv, si);
                if (lane == 0) { Wv[rl] = sv; Wi[rl] = si; Wn[rl] = n < a.k ? n : a.k; }
            }
        } else if constexpr (MODE == MODE_THRESH) {
            // the diagonal of the tile: row == column  <=>  wm == wn, mi == ni, r16 == 4g + e
            if (wm == wn && g == (r16 >> 2)) {
                const int e = lane & 3;
#pragma unroll
                for (int mi = 0; mi < 4; ++mi) {
                    const f32x4 v = acc[mi][mi];
                    const float s = e == 0 ? v[0] : e == 1 ? v[1] : e == 2 ? v[2] : v[3];
                    const int row = m0 + wm * 64 + mi * 16 + r16;
                    const int gi = row < a.nq ? a.gt[(size_t)row * a.gpr + tile] : -1;
                    if ((unsigned)gi < (unsigned)a.ng && beats(s, gi, tv[mi], ti[mi])) { tv[mi] = s; ti[mi] = gi; }
                }
            }
        }
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
    }

    if constexpr (MODE == MODE_TOPK) {
        // this wave's lists -> part [blockIdx.y * 2 + wn][row][k]
        const size_t pbase = (size_t)(blockIdx.y * 2 + wn) * a.nq;
        for (int e = lane; e < 64 * a.k; e += 64) {
            const int row = m0 + wm * 64 + e / a.k;
            if (row < a.nq) {
                const size_t o = (pbase + row) * a.k + e % a.k;
                a.part_val[o] = Lv[e];
                a.part_idx[o] = Li[e];
            }
        }
    } else if constexpr (MODE == MODE_RANK) {
        int* wg = reinterpret_cast<int*>(smem);
        __syncthreads();      // every wave is done with the staging buffers
        if (tid < BM) wg[tid] = 0;
        __syncthreads();
#pragma unroll
        for (int mi = 0; mi < 4; ++mi) {
            int c = cnt[mi];
            c += __shfl_xor(c, 16, 64);
            c += __shfl_xor(c, 32, 64);
            if (g == 0) atomicAdd(&wg[wm * 64 + mi * 16 + r16], c);      // the two waves of a row
        }
        __syncthreads();
        if (tid < BM && m0 + tid < a.nq && wg[tid]) atomicAdd(a.rank + m0 + tid, wg[tid]);
    } else if constexpr (MODE == MODE_THRESH) {
        if (wm == wn && g == (r16 >> 2)) {
#pragma unroll
            for (int mi = 0; mi < 4; ++mi) {
                const int row = m0 + wm * 64 + mi * 16 + r16;
                if (row < a.nq) {
                    a.thr[row] = ti[mi] >= 0 ? tv[mi] : INFINITY;
                    a.gstar[row] = ti[mi];
                    a.rank[row] = ti[mi] >= 0 ? 0 : 0x7fffffff;      // lpi_retrieval_rank's value for a row without ground truth
                }
            }
        }
    }
}

// ------------------------------------------------------------------------------------------------ the host layer
// Every entry point of the family fills ONE SearchCall and hands it to search_topk<T, MODE> / search_rank<T> (below) or search_rerank<T> (search_rerank.hip);
// the typed ones choose T from a list (search_pick).  Each argument rule is a host predicate on the struct, written once, and sweep_args<T> is the only
// writer of the kernel argument.

// the arguments of one call; a field an entry point does not have keeps its default
struct SearchCall {
    int nq = 0, ng = 0, E = 0;                            // E in elements, whatever the type
    const void* Q = nullptr; int ldq = 0;
    const void* G = nullptr; int ldg = 0;
    SearchScales sc{};
    int k = 0, col_base = 0, accumulate = 0;              // the list forms (k, idx, val: the re-rank form too)
    int32_t* idx = nullptr; float* val = nullptr;
    const int32_t* gt = nullptr; int gt_per_row = 0; int32_t* rank = nullptr;      // the rank form
    const int32_t* cand = nullptr; int ldc = 0, kc = 0;   // the re-rank form
    void* ws = nullptr; long ws_bytes = 0; void* stream = nullptr;
};

// The sweep's grid is row blocks x splits, about WG_TARGET workgroups.  search_blocks is what the workspace functions size for: splits * row blocks = the
// largest multiple of the row blocks not above it, so blocks >= splits * row blocks, and it never shrinks when an argument grows (the split count itself falls
// as the row blocks rise)
inline long search_blocks(int nq, int ng) {
    const long rb = (nq + BM - 1) / BM, tiles = (ng + BN - 1) / BN;
    return tiles * rb < WG_TARGET - 1 + rb ? tiles * rb : WG_TARGET - 1 + rb;
}
inline int search_splits(int nq, int ng) { return (int)(search_blocks(nq, ng) / ((nq + BM - 1) / BM)); }      // min(tiles, ceil(WG_TARGET / row blocks))

// ---- the argument rules (host predicates: no HIP call)
// the envelope every call shares: E a multiple of half a slab (f32: 16, 2-byte: 32; MX-FP8: of a whole one, 128; MX-FP4: 128 elements, half a slab), rows of
// whole 16-byte pieces (MX-FP4: leading dimensions in bytes, a row has E / 2); MX-FP8 / MX-FP4: scale rows of whole dwords
template <typename T>
int search_check(const SearchCall& c)
{
    constexpr int EPC = Elem<T>::EPC, HALF = kHasScales<T> ? ROW_BYTES : ROW_BYTES / (int)sizeof(T) / 2;
    if (c.nq <= 0 || c.ng <= 0 || c.E <= 0 || (c.E & (HALF - 1)) || c.E > 1024) return LPI_EINVAL;
    const int row = kIsMx4<T> ? c.E / 2 : c.E;      // in the units of ldq / ldg
    if (c.ldq < row || c.ldg < row || (c.ldq & (EPC - 1)) || (c.ldg & (EPC - 1))) return LPI_EINVAL;
    if (!c.Q || !c.G || (((uintptr_t)c.Q | (uintptr_t)c.G) & 15)) return LPI_EINVAL;
    if constexpr (kHasScales<T>) {
        if (!c.sc.q || !c.sc.g || (((uintptr_t)c.sc.q | (uintptr_t)c.sc.g) & 3)) return LPI_EINVAL;
        if (c.sc.ldq < c.E / 32 || c.sc.ldg < c.E / 32 || (c.sc.ldq & 3) || (c.sc.ldg & 3)) return LPI_EINVAL;
    }
    return 0;
}
// a list of k <= kmax per query row, in idx / val; without `accumulate` the gallery fills it
inline bool list_ok(const SearchCall& c, int kmax) {
    return c.k >= 1 && c.k <= kmax && (c.accumulate || c.k <= c.ng) && c.col_base >= 0 && (long)c.col_base + c.ng <= 0x7fffffffL && c.idx && c.val;
}
inline bool rank_ok(const SearchCall& c) { return c.gt && c.gt_per_row > 0 && c.rank; }
// `need` = what the form's workspace function answers for the call
inline bool ws_ok(const SearchCall& c, long need) { return c.ws && !((uintptr_t)c.ws & 3) && c.ws_bytes >= need; }
inline bool rerank_ok(const SearchCall& c) {
    return c.kc >= 1 && c.kc <= KWIDE && c.k >= 1 && c.k <= c.kc && c.ldc >= c.kc && c.cand && c.idx && c.val &&
           !(((uintptr_t)c.cand | (uintptr_t)c.idx | (uintptr_t)c.val) & 3);
}

// the typed pick: f(Tag<T>) for the type of the list L (dispatch.h) whose code is dt; any other code is refused and calls nothing
typedef TypeList<Types<bf16_t>, Types<f16_t>> TwoByte;                          // search16.hip: LPI_F32 is forwarded to search.hip's entry points
typedef TypeList<Types<float>, Types<bf16_t>, Types<f16_t>> PlainTypes;         // search_wide.hip, search_rerank.hip
template <typename L, typename F> int search_pick(L, int dt, F f) { int rc = LPI_EINVAL; dispatch_types(L{}, [&](auto t) { rc = f(t); }, dt); return rc; }

// ---- the ONE writer of the kernel argument, for all three sweeps.  per_split = the pairs a gallery split leaves in the workspace per query row (the list
// forms); 0 = the rank form, whose workspace is thr | gstar
template <typename T>
SearchArgs<T> sweep_args(const SearchCall& c, int per_split = 0)
{
    SearchArgs<T> a{};
    a.nq = c.nq; a.ng = c.ng; a.E = kIsMx4<T> ? c.E / 2 : c.E;      // MX-FP4: the row length in bytes
    a.Q = (const T*)c.Q; a.ldq = c.ldq; a.G = (const T*)c.G; a.ldg = c.ldg;
    if constexpr (kHasScales<T>) { a.Qs = (const uint8_t*)c.sc.q; a.ldqs = c.sc.ldq; a.Gs = (const uint8_t*)c.sc.g; a.ldgs = c.sc.ldg; }
    a.tiles = (c.ng + BN - 1) / BN; a.splits = search_splits(c.nq, c.ng);
    if (per_split) { a.k = c.k; a.part_val = (float*)c.ws; a.part_idx = (int32_t*)c.ws + (size_t)a.splits * c.nq * per_split; }      // the indices behind the values
    else { a.gt = c.gt; a.gpr = c.gt_per_row; a.thr = (float*)c.ws; a.gstar = (int32_t*)c.ws + c.nq; a.rank = c.rank; }
    return a;
}

// ---- one sweep launch: `lds` bytes behind the staging buffers, of at most `lds_max` (the kernel's limit, raised once per device).  The static is one per
// kernel: this function is instantiated once per (T, MODE)
template <typename T, int MODE>
int sweep(const SearchArgs<T>& a, int splits, int lds_max, int lds, hipStream_t s)
{
    static LdsOnce once;
    auto kern = search_kernel<T, MODE>;
    if (int e = lpi_ensure_lds(once, (const void*)kern, 2 * kStageBytes<T> + lds_max)) return e;
    LPI_LAUNCH(kern, dim3((a.nq + BM - 1) / BM, splits), dim3(NTHREADS), 2 * kStageBytes<T> + lds, s, a);
    LPI_CHECK_LAST();
    return 0;
}

// what the narrow (MODE_TOPK) and the wide (MODE_WIDE: search_wide.hip has the design and the merge kernel) top-k call differ in
template <int MODE> struct ListMode {
    static constexpr bool WIDE = MODE == MODE_WIDE;
    static constexpr int KTOP = WIDE ? KWIDE : KMAX;
    static constexpr auto workspace = WIDE ? lpi_search_wide_workspace : lpi_search_workspace;
    static constexpr int per_split(int k) { return WIDE ? wide_cap(k) : 2 * k; }      // a candidate buffer | a sorted list per wave column
    static constexpr int lds(int k) { return WIDE ? BM * 12 : 4 * 64 * k * 8; }       // per tile row a threshold pair and a fill counter | every wave's lists
    static int merge(const SearchCall& c, int splits, const float* pv, const int32_t* pi, hipStream_t s) {
        return WIDE ? lpi_search_wide_merge(c.nq, c.k, splits, wide_cap(c.k), pv, pi, c.col_base, c.accumulate, c.idx, c.val, s)
                    : lpi_search_merge(c.nq, c.k, 2 * splits, pv, pi, c.col_base, c.accumulate, c.idx, c.val, s);
    }
};

// a top-k call: the sweep with the mode's epilogue, then the merge of the splits' lists (and, with accumulate, the held one) into idx / val
template <typename T, int MODE>
int search_topk(const SearchCall& c)
{
    typedef ListMode<MODE> M;
    if (int e = search_check<T>(c)) return e;
    if (!list_ok(c, M::KTOP) || !ws_ok(c, M::workspace(c.nq, c.ng, c.k))) return LPI_EINVAL;
    const SearchArgs<T> a = sweep_args<T>(c, M::per_split(c.k));
    if (int e = sweep<T, MODE>(a, a.splits, M::lds(M::KTOP), M::lds(c.k), (hipStream_t)c.stream)) return e;
    return M::merge(c, a.splits, a.part_val, a.part_idx, (hipStream_t)c.stream);
}

// a rank call: the gathered launch leaves the thresholds, the sweep counts what beats them
template <typename T>
int search_rank(const SearchCall& c)
{
    if (int e = search_check<T>(c)) return e;
    if (!rank_ok(c) || !ws_ok(c, lpi_search_workspace(c.nq, c.ng, 0))) return LPI_EINVAL;
    const SearchArgs<T> a = sweep_args<T>(c);
    if (int e = sweep<T, MODE_THRESH>(a, 1, 0, 0, (hipStream_t)c.stream)) return e;
    return sweep<T, MODE_RANK>(a, a.splits, 0, 0, (hipStream_t)c.stream);
}

}  // namespace
