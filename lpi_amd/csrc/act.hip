// erf-GELU as a row kernel behind a plain c_fc GEMM (EngineOptions.erf_gelu): g <- gelu(u) in place, aux <- gelu'(u) for the backward's LPI_EPI_DQUICKGELU
// epilogue, which multiplies by whatever derivative the forward saved.  No GEMM epilogue is touched: the QuickGELU instantiations of gemm256p.hip stay as they are.
#include "dispatch.h"
#include "gemm_epilogue.h"      // AuxT: the storage type of the saved derivative

#define S(stream) ((hipStream_t)(stream))

typedef __attribute__((ext_vector_type(4))) unsigned u32x4_;

// gelu(u) = u Phi(u) and gelu'(u) = Phi(u) + u phi(u) in f32.  Phi through erfc: 1 + erf cancels in the negative tail, erfc keeps its relative accuracy there.
// Any finite u gives finite values: u^2 may overflow to +inf, exp(-inf) = 0 and u * 0 = +-0; erfc saturates at 0 and 2.
__device__ __forceinline__ void gelu_erf_both(float u, float& g, float& dg) {
    const float cdf = 0.5f * erfcf(-u * 0.70710678118654752440f);
    g = u * cdf;      // one multiply: the same bits whether dg is wanted or not
    dg = cdf + u * (expf(-0.5f * u * u) * 0.39894228040143267794f);
}

// one 16-byte chunk of T (4 floats or 8 two-byte elements) as floats, and back
template <typename T> struct Chunk16;
template <> struct Chunk16<float> {
    static constexpr int N = 4;
    __device__ static __forceinline__ void load(const float* p, float (&v)[4]) {
        const f32x4 x = *reinterpret_cast<const f32x4*>(p);
        v[0] = x[0]; v[1] = x[1]; v[2] = x[2]; v[3] = x[3];
    }
    __device__ static __forceinline__ u32x4_ pack(const float* v) {
        return u32x4_{__float_as_uint(v[0]), __float_as_uint(v[1]), __float_as_uint(v[2]), __float_as_uint(v[3])};
    }
};
template <> struct Chunk16<bf16_t> {
    static constexpr int N = 8;
    __device__ static __forceinline__ void load(const bf16_t* p, float (&v)[8]) {
        const uint4 x = *reinterpret_cast<const uint4*>(p);
        const uint32_t w[4] = {x.x, x.y, x.z, x.w};
#pragma unroll
        for (int i = 0; i < 4; ++i) { v[2 * i] = __uint_as_float(w[i] << 16); v[2 * i + 1] = __uint_as_float(w[i] & 0xFFFF0000u); }
    }
    __device__ static __forceinline__ u32x4_ pack(const float* v) {
        return u32x4_{pack2_t<bf16_t>(v[0], v[1]), pack2_t<bf16_t>(v[2], v[3]), pack2_t<bf16_t>(v[4], v[5]), pack2_t<bf16_t>(v[6], v[7])};
    }
};
template <> struct Chunk16<f16_t> {
    static constexpr int N = 8;
    __device__ static __forceinline__ void load(const f16_t* p, float (&v)[8]) {
        Chunk c;
        c.u = *reinterpret_cast<const uint4*>(p);
#pragma unroll
        for (int i = 0; i < 8; ++i) v[i] = (float)c.hh[i];
    }
    __device__ static __forceinline__ u32x4_ pack(const float* v) {
        return u32x4_{pack2_t<f16_t>(v[0], v[1]), pack2_t<f16_t>(v[2], v[3]), pack2_t<f16_t>(v[4], v[5]), pack2_t<f16_t>(v[6], v[7])};
    }
};

// A workgroup walks groups of `rpg` whole rows (about 2048 chunks: eight per lane); a lane moves 16 bytes of g per step — EPC elements — and, with AUX, the
// same EPC elements of aux, 16 bytes as well (every built pair has an aux element as wide as g's).  Only chunks inside [rows, cols] are addressed: the ld
// gaps are never touched.  g is read by the next GEMM at once (plain store); aux a whole forward later (streaming store).
// Measured at 54 528 x 3 072: the f32 form runs at the row kernels' memory rate (5.4 TB/s); the 2-byte forms take the same time for half the
// bytes (2.9 - 3.7 TB/s) — eight erfcf (+ eight expf) per chunk hold them, not memory, and the one integer division per chunk is small beside those.
template <typename T, bool AUX>
__global__ __launch_bounds__(256) void gelu_erf_fwd_kernel(long rows, int cpr, int rpg, long ngroups, T* __restrict__ g, long ldg,
                                                            typename AuxT<T>::type* __restrict__ aux, long ldaux) {
    typedef typename AuxT<T>::type TA;
    constexpr int EPC = Chunk16<T>::N;
    static_assert(sizeof(T) * EPC == 16 && sizeof(TA) * EPC == 16, "16-byte chunks of g and of aux");
    for (long grp = blockIdx.x; grp < ngroups; grp += gridDim.x) {
        const long row0 = grp * rpg;
        const int nr = (int)(rows - row0 < rpg ? rows - row0 : rpg);
        const int n = nr * cpr;
        for (int k = threadIdx.x; k < n; k += 256) {
            const int r = k / cpr, c = (k - r * cpr) * EPC;
            T* pg = g + (size_t)(row0 + r) * ldg + c;
            float u[EPC], y[EPC], dy[EPC];
            Chunk16<T>::load(pg, u);
#pragma unroll
            for (int j = 0; j < EPC; ++j) gelu_erf_both(u[j], y[j], dy[j]);
            *reinterpret_cast<u32x4_*>(pg) = Chunk16<T>::pack(y);
            if constexpr (AUX) {
                TA* pa = aux + (size_t)(row0 + r) * ldaux + c;
                __builtin_nontemporal_store(Chunk16<TA>::pack(dy), reinterpret_cast<u32x4_*>(pa));
            }
        }
    }
}

extern "C" int lpi_gelu_erf_fwd(int dtype, int aux_dtype, long rows, int cols, void* g, long ldg, void* aux, long ldaux, void* stream) {
    if (!g || rows < 1 || cols < 8 || (cols & 7) || ldg < cols || (ldg & 7) || ((uintptr_t)g & 15)) return LPI_EINVAL;
    if (aux && (ldaux < cols || (ldaux & 7) || ((uintptr_t)aux & 15))) return LPI_EINVAL;
    typedef TypeList<Types<float, float>, Types<bf16_t, bf16_t>, Types<f16_t, bf16_t>> Pairs;
    if (!types_listed(Pairs{}, dtype, aux_dtype)) return LPI_EINVAL;
    const int cpr = cols / (dtype == LPI_F32 ? 4 : 8);               // 16-byte chunks per row
    const int rpg = cpr >= 2048 ? 1 : 2048 / cpr;                     // rows per group: nr * cpr <= max(cpr, 2048) fits an int
    const long ngroups = (rows + rpg - 1) / rpg;
    const long cap = (long)lpi_cu_count() * 16;                       // the kernel strides over the groups: a bounded grid for any row count
    const dim3 grid((unsigned)(ngroups < cap ? ngroups : cap)), block(256);
    dispatch_types(Pairs{}, [&](auto tg, auto) {
        typedef type_of<decltype(tg)> T; typedef typename AuxT<T>::type TA;
        if (aux) LPI_LAUNCH((gelu_erf_fwd_kernel<T, true>), grid, block, 0, S(stream), rows, cpr, rpg, ngroups, (T*)g, ldg, (TA*)aux, ldaux);
        else LPI_LAUNCH((gelu_erf_fwd_kernel<T, false>), grid, block, 0, S(stream), rows, cpr, rpg, ngroups, (T*)g, ldg, (TA*)nullptr, 0L);
    }, dtype, aux_dtype);
    LPI_CHECK_LAST();
    return 0;
}
