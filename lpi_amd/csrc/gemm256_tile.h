// One 256x256 output tile of the phased NT GEMM (see gemm256.hip for the schedule), as a device function so that the plain
// kernel and the tail-splitting kernel share it.
#pragma once
#ifndef LPI_TWO_PHASE
#define LPI_TWO_PHASE 1
#endif
#include "common.h"
#include "gemm_epilogue.h"
#include "mx8.h"

namespace t256 {

#ifndef EPI_UNROLL
#define EPI_UNROLL 4
#endif
constexpr int T256 = 256;
constexpr int ROWB = 128;                 // bytes per staged row
constexpr int HALF_BYTES = 128 * ROWB;    // 16 KiB
constexpr int BUF_BYTES = 4 * HALF_BYTES; // 64 KiB per K-tile
constexpr int NTHR = 512;
constexpr int LDS_BYTES = 128 * 1040;      // max(2 K-tile buffers = 131072, epilogue staging 128 rows x 1040 B = 133120)
// MX-FP8 operands (T = mx8_t): behind the two K-tile buffers, per buffer the K-tile's scale bytes, 256 A rows x 4 B then 256 B rows x 4 B.  The epilogue's
// staging area may cover them: it is written only after every wave's last scale read (the reads retire with the fragments' in each phase's lgkmcnt(0)).
constexpr int OFF_SC = 2 * BUF_BYTES, SC_BUF = 2 * T256 * 4;
constexpr int LDS_BYTES_MX8 = OFF_SC + 2 * SC_BUF;      // 135168
constexpr int OFF_A0 = 0, OFF_A1 = HALF_BYTES, OFF_B0 = 2 * HALF_BYTES, OFF_B1 = 3 * HALF_BYTES;


template <typename T, typename TC, int EPI, bool RES, bool SAVE_U>
__device__ __forceinline__ void tile(int m0, int n0, int K, const T* __restrict__ A, int lda, const T* __restrict__ B, int ldb,
                                     TC* __restrict__ C, int ldc, const float* __restrict__ bias, const float* __restrict__ residual, int ldr,
                                     typename AuxT<T>::type* __restrict__ aux, int ldaux, float alpha, char* smem, Mx8Side mx = Mx8Side{})
{
    constexpr int EPC = Elem<T>::EPC;
    constexpr int BK = ROWB / (int)sizeof(T);
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave >> 2, wn = wave & 3;

    // ---- staging: a half tile = 128 rows x 128 B = 2 LDS-DMA instructions of 512 lanes x 16 B ---------------------
    // thread t, instr i -> LDS byte i*8192 + t*16: row = i*64 + t/8, phys chunk = t%8, logical = phys ^ ((row>>1)&7)
    const int srow = tid >> 3;
    const int schunk = (tid & 7) ^ ((tid >> 4) & 7);
    const T* a_src = A + (size_t)(m0 + srow) * lda + schunk * EPC;
    const T* b_src = B + (size_t)(n0 + srow) * ldb + schunk * EPC;
    const size_t a_i = (size_t)64 * lda, b_i = (size_t)64 * ldb, a_h = (size_t)128 * lda, b_h = (size_t)128 * ldb;

    // LDS-DMA issued from inline asm: hipcc models the builtin as an LDS write and would put s_waitcnt vmcnt(0) in front of
    // every later ds_read, draining the queue each phase; in asm only the counted vmcnt below orders it (guide section 5.7).
    const unsigned lds_w = __builtin_amdgcn_readfirstlane((unsigned)(uintptr_t)(__attribute__((address_space(3))) char*)smem + wave * 1024);
    auto glds16 = [&](const T* src, unsigned lds_addr) {
        unsigned keep;
        asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off\n\ts_mov_b32 m0, %0"
                     : "=&s"(keep) : "v"(src), "s"(lds_addr) : "memory");
    };
    auto stage_half = [&](const T* src, size_t istep, int lds_off) {
        glds16(src, lds_w + lds_off);
        glds16(src + istep, lds_w + lds_off + 8192);
    };
    auto stage_A = [&](int kt, int h, int buf) { stage_half(a_src + (size_t)kt * BK + h * a_h, a_i, buf * BUF_BYTES + (h ? OFF_A1 : OFF_A0)); };
    auto stage_B = [&](int kt, int h, int buf) { stage_half(b_src + (size_t)kt * BK + h * b_h, b_i, buf * BUF_BYTES + (h ? OFF_B1 : OFF_B0)); };

    // MX-FP8 scales of a K-tile: 4 bytes per tile row = one dword per lane, waves 0-3 the 256 A rows, waves 4-7 the 256 B rows; ONE more LDS-DMA per wave
    // and K-tile, issued and counted with the A0 / B0 / B1 halves of that K-tile.  Rows of the [rows, K/32] arrays are 4-byte aligned (K % 128 == 0).
    const uint8_t* s_src = nullptr;
    unsigned lds_s = 0;
    if constexpr (kIsMx8<T>) {
        const int r = (wave & 3) * 64 + lane;
        s_src = wave < 4 ? mx.a_scales + (size_t)(m0 + r) * mx.ldas : mx.b_scales + (size_t)(n0 + r) * mx.ldbs;
        lds_s = lds_w - wave * 1024 + OFF_SC + wave * 256;
    }
    auto stage_S = [&](int kt, int buf) {
        if constexpr (kIsMx8<T>) {
            unsigned keep;
            asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dword %1, off\n\ts_mov_b32 m0, %0"
                         : "=&s"(keep) : "v"(s_src + kt * 4), "s"(lds_s + buf * SC_BUF) : "memory");
        }
    };
    constexpr int VM_RING = kIsMx8<T> ? 9 : 8;      // LDS-DMA instructions that may stay in flight at the ring's waits: four half tiles (+ one K-tile's scales)

    // ---- fragment offsets within a half tile ---------------------------------------------------------------------
    const int frow = lane & 15, fg = lane >> 4, fsw = frow >> 1;
    int foff[2];
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) foff[ks] = frow * ROWB + (((ks << 2) | fg) ^ fsw) * 16;
    const int a_base = (wm * 64) * ROWB;   // + mi*16 rows
    const int b_base = (wn * 32) * ROWB;   // + ni*16 rows

    Chunk fa[4][2], fb0[2][2], fb1[2][2];
    mx8_i32x8 xa[4], xb0[2], xb1[2];   // MX-FP8: a fragment pair [.][0], [.][1] as the one instruction's eight operand registers it is
    f32x4 acc[2][2][2][4];   // [nh][ni][mh][mi]
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b)
#pragma unroll
            for (int c = 0; c < 2; ++c)
#pragma unroll
                for (int d = 0; d < 4; ++d) acc[a][b][c][d] = f32x4{0.f, 0.f, 0.f, 0.f};

    auto read_A = [&](const char* half) {
#pragma unroll
        for (int mi = 0; mi < 4; ++mi)
#pragma unroll
            for (int ks = 0; ks < 2; ++ks) fa[mi][ks].u = *reinterpret_cast<const uint4*>(half + a_base + mi * 16 * ROWB + foff[ks]);
        if constexpr (kIsMx8<T>) {
#pragma unroll
            for (int mi = 0; mi < 4; ++mi) xa[mi] = mx8_operand(fa[mi][0], fa[mi][1]);
        }
    };
    auto read_B = [&](Chunk (&fb)[2][2], mx8_i32x8 (&xb)[2], const char* half) {
#pragma unroll
        for (int ni = 0; ni < 2; ++ni)
#pragma unroll
            for (int ks = 0; ks < 2; ++ks) fb[ni][ks].u = *reinterpret_cast<const uint4*>(half + b_base + ni * 16 * ROWB + foff[ks]);
        if constexpr (kIsMx8<T>) {
#pragma unroll
            for (int ni = 0; ni < 2; ++ni) xb[ni] = mx8_operand(fb[ni][0], fb[ni][1]);
        }
    };
    // bf16x3 (T = f32x3_t): a fragment's two f32 chunks [.][0], [.][1] are one 16x16x32 instruction's 8 k-values of this lane; split once per read, in
    // place, into [.][0] = hi and [.][1] = lo (after the phase's lgkmcnt(0)); the B fragments stay split across both phases of a K-tile.
    // MX-FP8: the scale byte this lane holds for an instruction is that of row (l & 15) of the 16-row sub tile, K block (l >> 4) (gemm_mx8.hip has the map).
    // All of a K-tile's are read in phase X, whose barrier frees the scale area for the K-tile after next like the A0 / B0 / B1 halves, and packed four to a
    // register — the instruction's opsel picks the byte: sa[mh] byte mi, sb byte 2 nh + ni (3 registers instead of 12: the kernel has none to spare).
    int sa[2], sb;
    // the lane's byte of the first A / B row it reads, buffer 0: ONE address register each (hidden from the compiler, which otherwise keeps an address per
    // read: the area lies beyond the 64 KiB a ds_read offset spans from the array's start); the rest is immediates
    unsigned sa_addr = 0, sb_addr = 0;
    if constexpr (kIsMx8<T>) {
        sa_addr = (unsigned)(uintptr_t)(__attribute__((address_space(3))) char*)smem + OFF_SC + (wm * 64 + frow) * 4 + fg;
        sb_addr = (unsigned)(uintptr_t)(__attribute__((address_space(3))) char*)smem + OFF_SC + T256 * 4 + (wn * 32 + frow) * 4 + fg;
        asm volatile("" : "+v"(sa_addr), "+v"(sb_addr));
    }
    auto lds_u8 = [](unsigned addr) { return (unsigned)*(const __attribute__((address_space(3))) uint8_t*)(uintptr_t)addr; };
    auto read_S = [&](int buf) {
        if constexpr (kIsMx8<T>) {
            unsigned w[3] = {0, 0, 0};
#pragma unroll
            for (int i = 0; i < 4; ++i) {      // rows 16 apart are 64 bytes apart, the halves 512
                w[0] |= lds_u8(sa_addr + buf * SC_BUF + i * 64) << (8 * i);
                w[1] |= lds_u8(sa_addr + buf * SC_BUF + 512 + i * 64) << (8 * i);
                w[2] |= lds_u8(sb_addr + buf * SC_BUF + (i >> 1) * 512 + (i & 1) * 64) << (8 * i);
            }
            sa[0] = (int)w[0]; sa[1] = (int)w[1]; sb = (int)w[2];
        }
    };
    auto split_A = [&]() {
        if constexpr (kIsX3<T>) {
#pragma unroll
            for (int mi = 0; mi < 4; ++mi) split_bf16x3(fa[mi][0], fa[mi][1]);
        }
    };
    auto split_B = [&](Chunk (&fb)[2][2]) {
        if constexpr (kIsX3<T>) {
#pragma unroll
            for (int ni = 0; ni < 2; ++ni) split_bf16x3(fb[ni][0], fb[ni][1]);
        }
    };
    auto mma_quadrant = [&](f32x4 (&c)[2][2][2][4], int nh, int mh, const Chunk (&fb)[2][2], const mx8_i32x8 (&xb)[2]) {
        __builtin_amdgcn_s_setprio(1);
        if constexpr (kIsX3<T>) {
#pragma unroll
            for (int t = 0; t < 3; ++t)      // hi.hi, hi.lo, lo.hi: (weight plane t >> 1, activation plane t & 1)
#pragma unroll
                for (int ni = 0; ni < 2; ++ni)
#pragma unroll
                    for (int mi = 0; mi < 4; ++mi) mma_chunk<bf16_t>(c[nh][ni][mh][mi], fb[ni][t >> 1], fa[mi][t & 1]);
        } else if constexpr (kIsMx8<T>) {
#pragma unroll
            for (int ni = 0; ni < 2; ++ni)
#pragma unroll
                for (int mi = 0; mi < 4; ++mi) mx8_mma(c[nh][ni][mh][mi], xb[ni], xa[mi], 2 * nh + ni, sb, mi, sa[mh]);
            // hipcc sinks these instructions, unlike the bf16 ones, out of their phase to the end of the K-tile, past the barriers, and then holds three phases'
            // fragments at once (150 registers spilled): an empty statement that "uses" the quadrant's accumulators keeps them here
            asm volatile("" : "+v"(c[nh][0][mh][0]), "+v"(c[nh][0][mh][1]), "+v"(c[nh][0][mh][2]), "+v"(c[nh][0][mh][3]),
                              "+v"(c[nh][1][mh][0]), "+v"(c[nh][1][mh][1]), "+v"(c[nh][1][mh][2]), "+v"(c[nh][1][mh][3]));
        } else {
#pragma unroll
            for (int ks = 0; ks < 2; ++ks)
#pragma unroll
                for (int ni = 0; ni < 2; ++ni)
#pragma unroll
                    for (int mi = 0; mi < 4; ++mi) mma_chunk<T>(c[nh][ni][mh][mi], fb[ni][ks], fa[mi][ks]);
        }
        __builtin_amdgcn_s_setprio(0);
    };
// lgkmcnt(0) BEFORE the barrier: with the two wave groups staggered by one barrier (below), the other group restages a half
// tile right after this barrier, so this group's ds_reads of it must already have completed (WAR).
#define PHASE_SYNC_IN()                                   \
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");    \
    __builtin_amdgcn_s_barrier();                         \
    __builtin_amdgcn_sched_barrier(0)
#define PHASE_SYNC_OUT()                                  \
    __builtin_amdgcn_sched_barrier(0);                    \
    __builtin_amdgcn_s_barrier();                         \
    asm volatile("" ::: "memory")

    const int nk = K / BK;   // even, >= 2 (checked on the host)
#if LPI_TWO_PHASE
    // Two phases per K-tile (32 MFMAs each, 4 barriers per K-tile instead of 8; four half tiles in flight instead of three).
    // X: quadrants (n0,m0),(n1,m0) from B0, B1, A0;   Y: quadrants (n1,m1),(n0,m1) from A1 (B fragments stay in registers).
    // LDS-DMA: A1(kt+1) is issued in X(kt) (its slot was last read in Y(kt-1)); A0, B0, B1 of kt+2 in Y(kt) (read in X(kt)).
    // Each wave waits for its own DMAs with a counted vmcnt BEFORE the phase's first barrier, so that with the one-barrier stagger
    // both groups' data is visible when the reading phase starts: X waits for A1(kt) (8 younger instructions may stay in flight),
    // Y for A0, B0, B1 of kt+1.
    stage_A(0, 0, 0); stage_B(0, 0, 0); stage_B(0, 1, 0); stage_S(0, 0); stage_A(0, 1, 0);
    stage_A(1, 0, 1); stage_B(1, 0, 1); stage_B(1, 1, 1); stage_S(1, 1);
    asm volatile("s_waitcnt vmcnt(%0)" :: "n"(VM_RING) : "memory");
    __builtin_amdgcn_s_barrier();
    if (wm == 1) __builtin_amdgcn_s_barrier();
    auto ktile = [&](int kt, const int BUF) {
        const char* buf = smem + BUF * BUF_BYTES;
        const bool more1 = kt + 1 < nk, more2 = kt + 2 < nk;
        // X
        read_B(fb0, xb0, buf + OFF_B0);
        read_B(fb1, xb1, buf + OFF_B1);
        __builtin_amdgcn_sched_barrier(0);
        read_A(buf + OFF_A0);
        read_S(BUF);
        if (more1) {
            stage_A(kt + 1, 1, BUF ^ 1);
            asm volatile("s_waitcnt vmcnt(%0)" :: "n"(VM_RING) : "memory");
        } else {
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        }
        PHASE_SYNC_IN();
        split_B(fb0); split_B(fb1); split_A();
        mma_quadrant(acc, 0, 0, fb0, xb0);
        mma_quadrant(acc, 1, 0, fb1, xb1);
        PHASE_SYNC_OUT();
        // Y
        read_A(buf + OFF_A1);
        if (more2) {
            stage_A(kt + 2, 0, BUF); stage_B(kt + 2, 0, BUF); stage_B(kt + 2, 1, BUF); stage_S(kt + 2, BUF);
            asm volatile("s_waitcnt vmcnt(%0)" :: "n"(VM_RING) : "memory");
        } else if (more1) {
            asm volatile("s_waitcnt vmcnt(2)" ::: "memory");
        } else {
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        }
        PHASE_SYNC_IN();
        split_A();
        mma_quadrant(acc, 1, 1, fb1, xb1);
        mma_quadrant(acc, 0, 1, fb0, xb0);
        PHASE_SYNC_OUT();
    };
#else
    static_assert(!kIsX3<T> && !kIsMx8<T>, "bf16x3 and MX-FP8 are built for the two-phase schedule only");
    // prologue: K-tile 0 (4 halves) -> buffer 0, first three halves of K-tile 1 -> buffer 1
    stage_A(0, 0, 0); stage_B(0, 0, 0); stage_B(0, 1, 0); stage_A(0, 1, 0);
    stage_A(1, 0, 1); stage_B(1, 0, 1); stage_B(1, 1, 1);
    asm volatile("s_waitcnt vmcnt(6)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    // Stagger: waves 4-7 (the SIMD partners of waves 0-3) run one barrier behind, so that while one group issues its
    // ds_reads / LDS-DMA the other group's MFMAs own the matrix pipe (MI355X_MICROARCH.md, two waves per SIMD, item 9).
    // Every wave must execute the same number of barriers: group 0 pays its extra one after the loop.
    if (wm == 1) __builtin_amdgcn_s_barrier();

    // one K-tile = 4 phases; BUF is a compile-time constant so every LDS address folds to base + immediate
    auto ktile = [&](int kt, const int BUF) {
        const char* buf = smem + BUF * BUF_BYTES;
        const bool more1 = kt + 1 < nk, more2 = kt + 2 < nk;
        // P1
        read_B(fb0, xb0, buf + OFF_B0);
        __builtin_amdgcn_sched_barrier(0);
        read_A(buf + OFF_A0);
        if (more1) stage_A(kt + 1, 1, BUF ^ 1);
        PHASE_SYNC_IN();
        mma_quadrant(acc, 0, 0, fb0, xb0);
        PHASE_SYNC_OUT();
        // P2
        read_B(fb1, xb1, buf + OFF_B1);
        if (more2) stage_A(kt + 2, 0, BUF);
        PHASE_SYNC_IN();
        mma_quadrant(acc, 1, 0, fb1, xb1);
        PHASE_SYNC_OUT();
        // P3
        read_A(buf + OFF_A1);
        if (more2) stage_B(kt + 2, 0, BUF);
        PHASE_SYNC_IN();
        mma_quadrant(acc, 1, 1, fb1, xb1);
        PHASE_SYNC_OUT();
        // P4
        if (more2) {
            stage_B(kt + 2, 1, BUF);
            asm volatile("s_waitcnt vmcnt(6)" ::: "memory");
        } else {
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        }
        PHASE_SYNC_IN();
        mma_quadrant(acc, 0, 1, fb0, xb0);
        PHASE_SYNC_OUT();
    };
#endif
    for (int kt = 0; kt < nk; kt += 2) {
        ktile(kt, 0);
        ktile(kt + 1, 1);
    }
#undef PHASE_SYNC_IN
#undef PHASE_SYNC_OUT
    if (wm == 0) __builtin_amdgcn_s_barrier();

    // ---- epilogue: through LDS, so that every global access is a whole contiguous tile row ----------------------------
    // Straight from the accumulators a store instruction would touch 16 rows x 64 B (half cache lines, 16 lines per
    // instruction): measured ~3 B/clk/CU, several times slower than the main loop for K = 768.  Instead the tile goes through
    // LDS in two passes of 128 rows (f32, row stride 1040 B = conflict-free ds_write_b128); each wave then owns 16 whole rows
    // per pass: one ds_read_b128 + one 1 KiB-contiguous residual/aux load + one contiguous store per row, bias held in registers.
    constexpr int ERS = 1040;   // epilogue LDS row stride in bytes: 256 f32 + 16 B pad
    const int lrow = lane & 15, lcol = (lane >> 4) << 2;
    const int ecol = n0 + lane * 4;
    f32x4 bv = f32x4{0.f, 0.f, 0.f, 0.f};
    if (bias) bv = *reinterpret_cast<const f32x4*>(bias + ecol);
#pragma unroll
    for (int mh = 0; mh < 2; ++mh) {
        if (mh) __builtin_amdgcn_s_barrier();   // pass 0's reads are done before pass 1 overwrites the staging area
#pragma unroll
        for (int nh = 0; nh < 2; ++nh)
#pragma unroll
            for (int ni = 0; ni < 2; ++ni)
#pragma unroll
                for (int mi = 0; mi < 4; ++mi)
                    *reinterpret_cast<f32x4*>(smem + (wm * 64 + mi * 16 + lrow) * ERS + (nh * 128 + wn * 32 + ni * 16 + lcol) * 4) = acc[nh][ni][mh][mi];
        __syncthreads();
        const int r0 = wave * 16;
#pragma unroll EPI_UNROLL
        for (int rr = 0; rr < 16; ++rr) {
            const f32x4 v = *reinterpret_cast<const f32x4*>(smem + (r0 + rr) * ERS + lane * 16);
            if constexpr (__is_same(TC, mx8_out_t)) {
                // MX output: the 8 lanes that hold 32 consecutive columns of the row are one block — the quantiser of mx8_quantize_kernel on the staged f32 row
                f32x4 y = v * alpha + bv;
                if constexpr (EPI == LPI_EPI_QUICKGELU) y = quick_gelu_x4(y);
                const int byte = mx8_scale_byte(mx8_max8(mx8_amax4(y)));
                const size_t row = m0 + mh * 128 + r0 + rr;
                *reinterpret_cast<uint32_t*>(reinterpret_cast<uint8_t*>(C) + row * ldc + ecol) = mx8_pack4(y, byte);
                if ((lane & 7) == 0) mx.c_scales[row * mx.ldcs + (ecol >> 5)] = (uint8_t)byte;
            } else {
                gemm_epilogue_store<T, TC, EPI, RES, SAVE_U>(v, m0 + mh * 128 + r0 + rr, ecol, C, ldc, bv, alpha, residual, ldr, aux, ldaux);
            }
        }
    }
}

}  // namespace t256
