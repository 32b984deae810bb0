// Attention with ONE query row per sample: the last block of a tower, where only the pooled token (CLS / EOT) is read by the
// heads (model.py:255, prompt_learner.py:61), so Q, the softmax row, the context row and their gradients exist for that row alone;
// K and V (and dK, dV) still cover every token of the sample.  Exact dead-row elimination of nn.MultiheadAttention
// (model.py:179-184), not an approximation.  HBM-bound: one pass over the sample's K and V (forward) / K, V, dK, dV (backward).
//
// One 4-wave workgroup per (sample, head), keys interleaved over the waves.  Scores: 16 lanes x 4 dims per key, 4 keys per wave
// instruction (each key row is one contiguous 128 B / 256 B read), 4-step xor reduction.  Softmax row in LDS; every wave reduces
// it for itself.  Context / dQ / dK / dV: lane = head dim, loop over keys, so every row access is one whole head row; the four
// partial context / dQ rows are summed through LDS in a fixed order.  No atomics: bitwise reproducible.
#include <algorithm>
#include "dispatch.h"

namespace {

constexpr int DH = 64;
constexpr int WPB = 4;   // waves per workgroup

__device__ __forceinline__ float reduce16(float v) {
    v += __shfl_xor(v, 1, 64);
    v += __shfl_xor(v, 2, 64);
    v += __shfl_xor(v, 4, 64);
    v += __shfl_xor(v, 8, 64);
    return v;
}

__device__ __forceinline__ float dot4(const f32x4& a, const f32x4& b) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2] + a[3] * b[3]; }

template <typename T>
__device__ __forceinline__ void attn_pooled_fwd_body(
    int bh, float* sm, int B, int Lmax, const int* __restrict__ rs, int H, int Lp, const T* __restrict__ q, int ldq, const T* __restrict__ qkv, int ld, const int* __restrict__ idx,
    T* __restrict__ ctx, int ldo, float* __restrict__ lse, int causal, int pre = 0)
{
    // pre > 0 (shared prefix, attention.hip: attn_fwd_body): key position j < pre is global row j, position j >= pre the sample's own row j - pre
    float* s = sm;                 // scores
    float* p = sm + Lp;            // exp(score - max)
    float* red = sm + 2 * Lp;      // [WPB][64] partial context rows
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int b = bh / H, h = bh - b * H, d = H * DH;
    const int row = idx ? idx[b] : 0;
    // ragged batch (rs = row starts): sample b owns rows rs[b] .. rs[b+1]-1 of qkv
    const size_t r0 = rs ? (size_t)rs[b] : (size_t)b * Lmax;
    const int L = rs ? rs[b + 1] - rs[b] : Lmax;
    const int nv = causal ? row + 1 : L;           // keys the query row may attend to
    const int kk = lane >> 4, g = lane & 15;
    const f32x4 q4 = Elem<T>::ld4(q + (size_t)b * ldq + h * DH + 4 * g);
    const T* kbase = qkv + d + h * DH;
    const T* vbase = kbase + d;
    const long seg = (long)r0 - pre;
    auto krow = [&](int j) -> size_t { return (size_t)(j < pre ? (long)j : (long)j + seg); };
    for (int j0 = wave * 4; j0 < nv; j0 += 4 * WPB) {
        const int j = j0 + kk;
        float v = 0.f;
        if (j < nv) v = dot4(q4, Elem<T>::ld4(kbase + krow(j) * ld + 4 * g));
        v = reduce16(v);
        if (g == 0 && j < nv) s[j] = v * 0.125f;   // 1/sqrt(64)
    }
    __syncthreads();
    float m = -INFINITY;                           // every wave reduces the whole row itself: no cross-wave exchange
    for (int j = lane; j < nv; j += WAVE) m = fmaxf(m, s[j]);
    m = wave_max(m);
    float sum = 0.f;
    for (int j = lane; j < nv; j += WAVE) sum += __expf(s[j] - m);
    sum = wave_sum(sum);
    for (int j = threadIdx.x; j < nv; j += WAVE * WPB) p[j] = __expf(s[j] - m);
    __syncthreads();
    float acc = 0.f;
#pragma unroll 8
    for (int j = wave; j < nv; j += WPB) acc += p[j] * Elem<T>::ld(vbase + krow(j) * ld + lane);
    red[wave * DH + lane] = acc;
    __syncthreads();
    if (wave == 0) {
        float t = 0.f;
#pragma unroll
        for (int w = 0; w < WPB; ++w) t += red[w * DH + lane];
        Elem<T>::st(ctx + (size_t)b * ldo + h * DH + lane, t / sum);
        if (lane == 0) lse[bh] = m + __logf(sum);
    }
}
template <typename T>
__global__ __launch_bounds__(WAVE * WPB) void attn_pooled_fwd_kernel(
    int B, int Lmax, const int* __restrict__ rs, int H, int Lp, const T* __restrict__ q, int ldq, const T* __restrict__ qkv, int ld, const int* __restrict__ idx,
    T* __restrict__ ctx, int ldo, float* __restrict__ lse, int causal, int pre)
{
    extern __shared__ float sm[];
    attn_pooled_fwd_body<T>(blockIdx.x, sm, B, Lmax, rs, H, Lp, q, ldq, qkv, ld, idx, ctx, ldo, lse, causal, pre);
}
// the two towers' pooled-row attention of the last block in ONE launch: workgroups [0, nb0) are problem 0's (sample, head) pairs
struct PoolFwdP { int B, Lmax, H, Lp, ldq, ld, ldo, causal; const int* rs; const void* q; const void* qkv; const int* idx; void* ctx; float* lse; int pre; };
template <typename T>
__global__ __launch_bounds__(WAVE * WPB) void attn_pooled_fwd_pair_kernel(PoolFwdP p0, PoolFwdP p1, int nb0)
{
    extern __shared__ float sm[];
    const bool z = (int)blockIdx.x >= nb0;
    const PoolFwdP& p = z ? p1 : p0;
    attn_pooled_fwd_body<T>(z ? blockIdx.x - nb0 : blockIdx.x, sm, p.B, p.Lmax, p.rs, p.H, p.Lp, (const T*)p.q, p.ldq, (const T*)p.qkv, p.ld, p.idx, (T*)p.ctx, p.ldo, p.lse,
                            p.causal, p.pre);
}

// TS: storage type of the SAVED q / qkv (fp16 after an f16-mode forward, else T); dctx, dq, dqkv are T.  All arithmetic is f32.
template <typename T, typename TS = T>
__device__ __forceinline__ void attn_pooled_bwd_body(
    int bh, float* sm, int B, int Lmax, const int* __restrict__ rs, int H, int Lp, const TS* __restrict__ q, int ldq, const TS* __restrict__ qkv, int ld, const int* __restrict__ idx,
    const T* __restrict__ dctx, int ldo, const float* __restrict__ lse, T* __restrict__ dq, int lddq, T* __restrict__ dqkv, int ldg, int causal, int pre = 0,
    float* __restrict__ part = nullptr)
{
    // pre > 0 (shared prefix): dK / dV of the shared keys go to part[b][key][dK (d) | dV (d)] as f32 (summed over the samples by lpi_shared_kv_reduce)
    float* p = sm;                 // softmax row
    float* dp = sm + Lp;           // dctx . V_j
    float* ds = sm + 2 * Lp;       // P_j (dP_j - delta) / 8
    float* red = sm + 3 * Lp;      // [WPB][64] partial dQ rows
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int b = bh / H, h = bh - b * H, d = H * DH;
    const int row = idx ? idx[b] : 0;
    const size_t r0 = rs ? (size_t)rs[b] : (size_t)b * Lmax;      // ragged batch: see the forward
    const int L = rs ? rs[b + 1] - rs[b] : Lmax;
    const int nv = causal ? row + 1 : L;
    const int kk = lane >> 4, g = lane & 15;
    const f32x4 q4 = Elem<TS>::ld4(q + (size_t)b * ldq + h * DH + 4 * g);
    const f32x4 o4 = Elem<T>::ld4(dctx + (size_t)b * ldo + h * DH + 4 * g);
    const TS* kbase = qkv + d + h * DH;
    const TS* vbase = kbase + d;
    const long seg = (long)r0 - pre;
    auto krow = [&](int j) -> size_t { return (size_t)(j < pre ? (long)j : (long)j + seg); };
    const float ls = lse[bh];
    for (int j0 = wave * 4; j0 < nv; j0 += 4 * WPB) {
        const int j = j0 + kk;
        float sc = 0.f, dv = 0.f;
        if (j < nv) {
            sc = dot4(q4, Elem<TS>::ld4(kbase + krow(j) * ld + 4 * g));
            dv = dot4(o4, Elem<TS>::ld4(vbase + krow(j) * ld + 4 * g));
        }
        sc = reduce16(sc);
        dv = reduce16(dv);
        if (g == 0 && j < nv) {
            p[j] = __expf(sc * 0.125f - ls);
            dp[j] = dv;
        }
    }
    __syncthreads();
    float delta = 0.f;
    for (int j = lane; j < nv; j += WAVE) delta += p[j] * dp[j];
    delta = wave_sum(delta);
    for (int j = threadIdx.x; j < nv; j += WAVE * WPB) ds[j] = p[j] * (dp[j] - delta) * 0.125f;
    __syncthreads();
    const float qd = Elem<TS>::ld(q + (size_t)b * ldq + h * DH + lane);
    const float od = Elem<T>::ld(dctx + (size_t)b * ldo + h * DH + lane);
    T* dk = dqkv + d + h * DH + lane;
    T* dv = dk + d;
    float* pk = part + ((size_t)b * pre) * 2 * d + h * DH + lane;      // used for j < pre only
    float acc = 0.f;
#pragma unroll 4
    for (int j = wave; j < nv; j += WPB) {
        const float dsj = ds[j];
        acc += dsj * Elem<TS>::ld(kbase + krow(j) * ld + lane);
        if (j < pre) {
            pk[(size_t)j * 2 * d] = dsj * qd;
            pk[(size_t)j * 2 * d + d] = p[j] * od;
        } else {
            Elem<T>::st(dk + krow(j) * ldg, dsj * qd);
            Elem<T>::st(dv + krow(j) * ldg, p[j] * od);
        }
    }
    for (int j = nv + wave; j < L + pre; j += WPB) {     // keys behind the causal mask get no gradient
        if (j < pre) {
            pk[(size_t)j * 2 * d] = 0.f;
            pk[(size_t)j * 2 * d + d] = 0.f;
        } else {
            Elem<T>::st(dk + krow(j) * ldg, 0.f);
            Elem<T>::st(dv + krow(j) * ldg, 0.f);
        }
    }
    red[wave * DH + lane] = acc;
    __syncthreads();
    if (wave == 0) {
        float t = 0.f;
#pragma unroll
        for (int w = 0; w < WPB; ++w) t += red[w * DH + lane];
        Elem<T>::st(dq + (size_t)b * lddq + h * DH + lane, t);
    }
}
template <typename T, typename TS = T>
__global__ __launch_bounds__(WAVE * WPB) void attn_pooled_bwd_kernel(
    int B, int Lmax, const int* __restrict__ rs, int H, int Lp, const TS* __restrict__ q, int ldq, const TS* __restrict__ qkv, int ld, const int* __restrict__ idx,
    const T* __restrict__ dctx, int ldo, const float* __restrict__ lse, T* __restrict__ dq, int lddq, T* __restrict__ dqkv, int ldg, int causal, int pre,
    float* __restrict__ part)
{
    extern __shared__ float sm[];
    attn_pooled_bwd_body<T, TS>(blockIdx.x, sm, B, Lmax, rs, H, Lp, q, ldq, qkv, ld, idx, dctx, ldo, lse, dq, lddq, dqkv, ldg, causal, pre, part);
}
struct PoolBwdP { int B, Lmax, H, Lp, ldq, ld, ldo, lddq, ldg, causal; const int* rs; const void* q; const void* qkv; const int* idx; const void* dctx; const float* lse;
                  void* dq; void* dqkv; int pre; float* part; };
template <typename T, typename TS = T>
__global__ __launch_bounds__(WAVE * WPB) void attn_pooled_bwd_pair_kernel(PoolBwdP p0, PoolBwdP p1, int nb0)
{
    extern __shared__ float sm[];
    const bool z = (int)blockIdx.x >= nb0;
    const PoolBwdP& p = z ? p1 : p0;
    attn_pooled_bwd_body<T, TS>(z ? blockIdx.x - nb0 : blockIdx.x, sm, p.B, p.Lmax, p.rs, p.H, p.Lp, (const TS*)p.q, p.ldq, (const TS*)p.qkv, p.ld, p.idx, (const T*)p.dctx,
                                p.ldo, p.lse, (T*)p.dq, p.lddq, (T*)p.dqkv, p.ldg, p.causal, p.pre, p.part);
}

// ---- the host layer: every form fills a lpi_attn_pooled_desc (one problem; the _pair forms bring two); one predicate and one launch per direction
typedef TypeList<Types<float>, Types<bf16_t>, Types<f16_t>> PooledFwdTypes;
// (gradients in and out, saved q / qkv): an f16-mode forward saved fp16, its gradients are bf16; the call's dtype names the SAVED type
typedef TypeList<Types<float, float>, Types<bf16_t, bf16_t>, Types<bf16_t, f16_t>> PooledBwdTypes;
inline int grad_dtype(int dtype) { return dtype == LPI_F16 ? LPI_BF16 : dtype; }

// LDS of a workgroup: `rows` score-sized rows of L rounded up to 64 floats + the waves' partial head rows
inline int pooled_lp(int L) { return (L + 63) / 64 * 64; }
inline size_t pooled_lds(int L, int rows) { return (size_t)(rows * pooled_lp(L) + WPB * DH) * sizeof(float); }
// the shared-prefix fields: none, or a causal ragged batch with its queries' positions, the prefix shorter than the longest sequence
inline bool pooled_shared_ok(const lpi_attn_pooled_desc& d) { return d.shared_rows == 0 || (d.shared_rows > 0 && d.causal && d.row_start && d.idx && d.shared_rows < d.L); }

// q and qkv are read four elements at a time (whole 16-byte units, 16-byte aligned); ctx is written one element per lane
bool pooled_fwd_ok(int dtype, const lpi_attn_pooled_desc& d) {
    const int esz = dtype == LPI_F32 ? 4 : 2;
    if (!d.q || !d.qkv || !d.ctx || !d.lse || d.B <= 0 || d.L <= 0 || d.H <= 0) return false;
    if (d.ldqkv < 3 * d.H * DH || d.ldq < d.H * DH || d.ldctx < d.H * DH || (d.ldqkv * esz) % 16 || (d.ldq * esz) % 16) return false;
    if (((uintptr_t)d.q | (uintptr_t)d.qkv) & 15) return false;
    return pooled_lds(d.L, 2) <= 64 * 1024 && pooled_shared_ok(d);
}
// the same for q, qkv and dctx; dq and dqkv are written one element per lane.  On a shared prefix dqkv and shared_dkv go through lpi_shared_kv_reduce after
// the launch (four elements per lane): its conditions are refused here, before any launch
bool pooled_bwd_ok(int dtype, const lpi_attn_pooled_desc& d) {
    const int esz = dtype == LPI_F32 ? 4 : 2;
    if (!d.q || !d.qkv || !d.dctx || !d.lse || !d.dq || !d.dqkv || d.B <= 0 || d.L <= 0 || d.H <= 0) return false;
    if (d.ldqkv < 3 * d.H * DH || d.lddqkv < 3 * d.H * DH || d.ldq < d.H * DH || d.lddctx < d.H * DH || d.lddq < d.H * DH) return false;
    if ((d.ldqkv * esz) % 16 || (d.ldq * esz) % 16 || (d.lddctx * esz) % 16) return false;
    if (((uintptr_t)d.q | (uintptr_t)d.qkv | (uintptr_t)d.dctx) & 15) return false;
    if (pooled_lds(d.L, 3) > 64 * 1024 || !pooled_shared_ok(d)) return false;
    return d.shared_rows == 0 || (d.shared_dkv && !(d.lddqkv & 3) && !((uintptr_t)d.shared_dkv & 15) && !((uintptr_t)d.dqkv & (dtype == LPI_F32 ? 15 : 7)));
}

// a single problem on a shared prefix is causal by rule: the kernel is handed 1, whatever non-zero value the descriptor holds
inline int causal_of(const lpi_attn_pooled_desc& d) { return d.shared_rows ? 1 : d.causal; }

int pooled_fwd(int dtype, const lpi_attn_pooled_desc& d, void* stream) {
    if (!pooled_fwd_ok(dtype, d)) return LPI_EINVAL;
    if (!dispatch_types(PooledFwdTypes{}, [&](auto t) {
            typedef type_of<decltype(t)> T;
            LPI_LAUNCH((attn_pooled_fwd_kernel<T>), dim3(d.B * d.H), dim3(WAVE * WPB), pooled_lds(d.L, 2), (hipStream_t)stream, d.B, d.L, d.row_start, d.H, pooled_lp(d.L),
                       (const T*)d.q, d.ldq, (const T*)d.qkv, d.ldqkv, d.idx, (T*)d.ctx, d.ldctx, d.lse, causal_of(d), d.shared_rows);
        }, dtype)) return LPI_ENOSYS;
    LPI_CHECK_LAST();
    return 0;
}

int pooled_bwd(int dtype, const lpi_attn_pooled_desc& d, void* stream) {
    if (!pooled_bwd_ok(dtype, d)) return LPI_EINVAL;
    if (!dispatch_types(PooledBwdTypes{}, [&](auto t, auto ts) {
            typedef type_of<decltype(t)> T;
            typedef type_of<decltype(ts)> TS;
            LPI_LAUNCH((attn_pooled_bwd_kernel<T, TS>), dim3(d.B * d.H), dim3(WAVE * WPB), pooled_lds(d.L, 3), (hipStream_t)stream, d.B, d.L, d.row_start, d.H, pooled_lp(d.L),
                       (const TS*)d.q, d.ldq, (const TS*)d.qkv, d.ldqkv, d.idx, (const T*)d.dctx, d.lddctx, d.lse, (T*)d.dq, d.lddq, (T*)d.dqkv, d.lddqkv, causal_of(d),
                       d.shared_rows, d.shared_rows ? d.shared_dkv : nullptr);
        }, grad_dtype(dtype), dtype)) return LPI_ENOSYS;
    LPI_CHECK_LAST();
    // shared prefix: no query sits on the shared rows here, so their dK / dV are the samples' sum alone (written, not added)
    return d.shared_rows ? lpi_shared_kv_reduce(dtype, d.B, d.shared_rows, d.H, d.shared_dkv, d.dqkv, d.lddqkv, 0, stream) : 0;
}

}  // namespace

extern "C" int lpi_attn_pooled_fwd_varlen(int dtype, int B, int L, const int32_t* row_start, int H, const void* q, int ldq, const void* qkv, int ld,
                                          const int* idx, void* ctx, int ldo, float* lse, int causal, void* stream)
{
    return pooled_fwd(dtype, lpi_attn_pooled_desc{.B = B, .L = L, .H = H, .row_start = row_start, .q = q, .ldq = ldq, .qkv = qkv, .ldqkv = ld, .idx = idx, .ctx = ctx,
                                                  .ldctx = ldo, .lse = lse, .causal = causal}, stream);
}

extern "C" int lpi_attn_pooled_bwd_varlen(int dtype, int B, int L, const int32_t* row_start, int H, const void* q, int ldq, const void* qkv, int ld,
                                          const int* idx, const void* dctx, int ldo, const float* lse, void* dq, int lddq, void* dqkv, int ldg,
                                          int causal, void* stream)
{
    return pooled_bwd(dtype, lpi_attn_pooled_desc{.B = B, .L = L, .H = H, .row_start = row_start, .q = q, .ldq = ldq, .qkv = qkv, .ldqkv = ld, .idx = idx,
                                                  .lse = const_cast<float*>(lse), .dctx = dctx, .lddctx = ldo, .dq = dq, .lddq = lddq, .dqkv = dqkv, .lddqkv = ldg,
                                                  .causal = causal}, stream);
}

// one problem through the descriptor form (the shared-prefix fields exist there only).  Without a shared prefix this is the _varlen form: shared_dkv is not looked at
extern "C" int lpi_attn_pooled_fwd_desc(int dtype, const lpi_attn_pooled_desc* d, void* stream) { return d ? pooled_fwd(dtype, *d, stream) : LPI_EINVAL; }
extern "C" int lpi_attn_pooled_bwd_desc(int dtype, const lpi_attn_pooled_desc* d, void* stream) { return d ? pooled_bwd(dtype, *d, stream) : LPI_EINVAL; }

// ---- the two towers' pooled attention in one launch (same kernels' bodies, bit for bit); desc[i]: the arguments of the _varlen entry points
extern "C" int lpi_attn_pooled_fwd_pair(int dtype, const lpi_attn_pooled_desc* d, void* stream)
{
    if (!d || !pooled_fwd_ok(dtype, d[0]) || !pooled_fwd_ok(dtype, d[1])) return LPI_EINVAL;
    PoolFwdP p[2];
    for (int i = 0; i < 2; ++i)
        p[i] = PoolFwdP{d[i].B, d[i].L, d[i].H, pooled_lp(d[i].L), d[i].ldq, d[i].ldqkv, d[i].ldctx, d[i].causal, d[i].row_start, d[i].q, d[i].qkv, d[i].idx, d[i].ctx, d[i].lse,
                        d[i].shared_rows};
    const int nb0 = p[0].B * p[0].H;
    const size_t lds = pooled_lds(std::max(d[0].L, d[1].L), 2);
    if (!dispatch_types(PooledFwdTypes{}, [&](auto t) {
            LPI_LAUNCH((attn_pooled_fwd_pair_kernel<type_of<decltype(t)>>), dim3(nb0 + p[1].B * p[1].H), dim3(WAVE * WPB), lds, (hipStream_t)stream, p[0], p[1], nb0);
        }, dtype)) return LPI_ENOSYS;
    LPI_CHECK_LAST();
    return 0;
}
extern "C" int lpi_attn_pooled_bwd_pair(int dtype, const lpi_attn_pooled_desc* d, void* stream)
{
    if (!d || !pooled_bwd_ok(dtype, d[0]) || !pooled_bwd_ok(dtype, d[1])) return LPI_EINVAL;
    PoolBwdP p[2];
    for (int i = 0; i < 2; ++i)
        p[i] = PoolBwdP{d[i].B, d[i].L, d[i].H, pooled_lp(d[i].L), d[i].ldq, d[i].ldqkv, d[i].lddctx, d[i].lddq, d[i].lddqkv, d[i].causal, d[i].row_start, d[i].q, d[i].qkv, d[i].idx,
                        d[i].dctx, d[i].lse, d[i].dq, d[i].dqkv, d[i].shared_rows, d[i].shared_dkv};
    const int nb0 = p[0].B * p[0].H;
    const size_t lds = pooled_lds(std::max(d[0].L, d[1].L), 3);
    if (!dispatch_types(PooledBwdTypes{}, [&](auto t, auto ts) {
            LPI_LAUNCH((attn_pooled_bwd_pair_kernel<type_of<decltype(t)>, type_of<decltype(ts)>>), dim3(nb0 + p[1].B * p[1].H), dim3(WAVE * WPB), lds, (hipStream_t)stream, p[0], p[1], nb0);
        }, grad_dtype(dtype), dtype)) return LPI_ENOSYS;
    LPI_CHECK_LAST();
    for (int i = 0; i < 2; ++i)      // shared prefix: as pooled_bwd
        if (d[i].shared_rows > 0)
            if (int e = lpi_shared_kv_reduce(dtype, d[i].B, d[i].shared_rows, d[i].H, d[i].shared_dkv, d[i].dqkv, d[i].lddqkv, 0, stream)) return e;
    return 0;
}

extern "C" int lpi_attn_pooled_fwd(int dtype, int B, int L, int H, const void* q, int ldq, const void* qkv, int ld, const int* idx,
                                   void* ctx, int ldo, float* lse, int causal, void* stream)
{
    return lpi_attn_pooled_fwd_varlen(dtype, B, L, nullptr, H, q, ldq, qkv, ld, idx, ctx, ldo, lse, causal, stream);
}
extern "C" int lpi_attn_pooled_bwd(int dtype, int B, int L, int H, const void* q, int ldq, const void* qkv, int ld, const int* idx,
                                   const void* dctx, int ldo, const float* lse, void* dq, int lddq, void* dqkv, int ldg, int causal,
                                   void* stream)
{
    return lpi_attn_pooled_bwd_varlen(dtype, B, L, nullptr, H, q, ldq, qkv, ld, idx, dctx, ldo, lse, dq, lddq, dqkv, ldg, causal, stream);
}
