/*
 * lpi_hip.h — C ABI of liblpi_hip.so: the MI355X (gfx950) kernels behind the LPI retrieval hot path.
 *
 * The reference (Kelvin-ywc/LPI, retrieval/) has no FFI of its own: its hot path is stock PyTorch modules
 * (SURVEY.md section 2d).  Each entry point below replaces the ATen arithmetic under one reference call site;
 * the citation after "replaces:" is the reference file:line (relative to /root/reference/retrieval/).
 * INTEGRATION.md shows the ctypes binding a maintainer adds on the reference side.
 *
 * Conventions
 *   - every pointer is DEVICE memory owned by the caller (torch); no hidden allocation, no host sync;
 *   - every call only enqueues work on `stream` (a hipStream_t passed as void*) and returns
 *     0 on success, a negative LPI_E* code on a rejected argument, or a positive hipError_t;
 *   - `dtype` selects the storage type of activations/weights fed to the matrix cores:
 *       LPI_F32  : f32 in, f32 accumulate (v_mfma_f32_16x16x4_f32)     — parity mode
 *       LPI_BF16 : bf16 in, f32 accumulate (v_mfma_f32_16x16x32_bf16) — throughput mode
 *       LPI_F32X3: f32 in, split into hi + lo bf16 in registers, three bf16 products, f32 accumulate — GEMMs of the f32 mode only
 *     the residual stream, LayerNorm statistics, losses and prompt factors are always f32;
 *   - token rows are batch-major: row(b, l) = b * L + l (the reference permutes to [L, B, d] for
 *     nn.MultiheadAttention, models/clip/model.py:253; the arithmetic is layout independent);
 *   - matrices handed to lpi_gemm_nt are padded by the caller: M % 128 == 0, N % 128 == 0,
 *     K % (128 / sizeof(element)) == 0, and EVERY leading dimension (lda, ldb, ldc, ldr, ldaux) a multiple of 16 bytes in its operand's
 *     own element type, every operand pointer (A, B, C, bias, residual, aux) 16-byte aligned — LPI_EINVAL before any launch otherwise
 *     (since 613; up to 612 ldc, an fp16 ldr, ldaux and the aux pointer were only held to 8 bytes, which the 16-byte stores and LDS-DMA
 *     loads of the persistent kernel's epilogues and the f32x4 accesses of an f32 C / aux do not honour: DESIGN.md section 4).
 *     lpi_gemm_nt_rows has one kernel, whose epilogue moves four elements per lane: lda, ldb 16 bytes; ldc, ldr, ldaux multiples of FOUR
 *     ELEMENTS (8 bytes for a 2-byte type, 16 for f32), aux aligned likewise.  The LN operand block's ldr and LPI_EPI_RES_ROWSTATS's ldaux
 *     count f32 entries: multiples of 4.  A leading dimension changes no arithmetic: a strided call gives the bits of the contiguous one, and
 *     nothing outside the [rows, cols] footprint of an operand is read into a result or written (tests/test_gemm_strides_gpu.py).
 *   - DEAD REGIONS.  A call is often handed more memory than it may use; what it does not use may hold anything, NaN included, and no
 *     live output depends on it (tests/test_dead_memory_gpu.py fills each of these with NaN and asks for the same bits):
 *       token rows behind the batch: rows >= B*L (ragged: >= row_start[B]) of qkv, ctx, dctx, x, mean, rstd — arenas are padded to 256 rows;
 *       ragged batches: the lse / delta entries l >= L_b of sample b, and ids[b, l >= L_b] of lpi_txt_embed_fwd_varlen;
 *       `delta` of every attention backward on entry, `scratch` of lpi_spool_attn_fwd on entry, and its second quarter and second half
 *         on entry to lpi_spool_attn_bwd;
 *       lpi_attn_pooled_*: columns 0..d of qkv (q arrives separately) and, with causal != 0, the K / V rows j > idx[b] of sample b;
 *       the LN operand block: entries M..ldr-1 of its mean and rstd segments; lpi_ln_stats_finalize: entries rows..ld-1 of every slot;
 *       kernels with a row map (row0 / P, or idx): every row of x, mean, rstd, dx0, src that the map does not name;
 *       padded matrices: rows and columns >= n of the logits of lpi_clip_loss_local / lpi_ce_rows_fwd_bwd, the columns between n_cols / E
 *         and the leading dimension of lpi_retrieval_rank, lpi_topk and lpi_l1_task_id.
 *     PRESERVED (never written): the rows of dx, dx_cast, dst, out_mean / out_rstd that a row map does not name; columns 0..d of the pooled
 *     backward's dqkv; rows of x0 behind row_start[B]; columns >= n and rows >= nloc (rows >= `rows`) of g, gt and dlogits.
 */
#ifndef LPI_HIP_H
#define LPI_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LPI_F32 0
#define LPI_BF16 1
#define LPI_F16 2          /* STORAGE type of the residual stream in bf16 mode (the reference's own activation type: it runs fp16 end to
                            * end, model.py:371-392); never an MFMA operand type.  Accepted where a parameter is named x_dtype, and as
                            * lpi_gemm_nt's c_dtype together with a residual of the same type. */

#define LPI_F32X3 4        /* lpi_gemm_nt / lpi_gemm_nt_grouped `dtype` only: f32 operands in memory (A, B, C, residual, aux all f32; c_dtype must be
                            * LPI_F32), multiplied as SPLIT bf16 ("bf16x3"): each operand element x becomes hi = RNE_bf16(x), lo = RNE_bf16(x - hi)
                            * in registers and a product is hi.hi + hi.lo + lo.hi on v_mfma_f32_16x16x32_bf16 with f32 accumulation (lo.lo dropped:
                            * about 2^-16 per product where f32 has 2^-24 and bf16 2^-8).  Epilogues LPI_EPI_NONE (+- bias, +- residual),
                            * LPI_EPI_QUICKGELU (+- aux) and LPI_EPI_DQUICKGELU; shapes as LPI_F32 (M, N % 128, K % 32); anything else is LPI_ENOSYS /
                            * LPI_EINVAL before any launch.  NaN / Inf operands are out of contract; a subnormal lo may flush.  Attributed to
                            * LPI_GEMM_K_X3.  lpi_gemm_nt_rows does not take it: few-row GEMMs stay exact f32. */

#define LPI_EINVAL (-22)   /* bad shape / alignment / null pointer */
#define LPI_ENOSYS (-38)   /* combination not built */

/* epilogue selectors of lpi_gemm_nt */
#define LPI_EPI_NONE 0        /* C = alpha*acc (+bias) (+residual)                                     */
#define LPI_EPI_QUICKGELU 1   /* u = acc+bias; C = u*sigmoid(1.702u) (model.py:163-165); aux (if given) = d/du[u*sigmoid(1.702u)] — the
                               * DERIVATIVE, evaluated here from the same sigmoid and saved for the backward                          */
#define LPI_EPI_DQUICKGELU 2  /* C = acc * aux, aux = the derivative the forward saved          (backward of the activation)          */
                              /* It multiplies by WHATEVER derivative the forward saved: QuickGELU's from the epilogues above, erf-GELU's from lpi_gelu_erf_fwd. */
#define LPI_EPI_LN 3          /* LayerNorm FOLDED into the GEMM: A is the LayerNorm's INPUT x, B = gamma o W (columns scaled), and
                               * C = rstd[row] * (acc - mean[row] * c1[col]) + bias[col] (alpha must be 1: LPI_EINVAL otherwise), c1[n] = sum_k B[n,k], bias = W beta + b — i.e.
                               * LN(x) W^T + b without ever writing LN(x) (model.py:172-177: ln_1 -> attn in_proj, ln_2 -> c_fc).  `residual`
                               * carries the LN operand block (f32): mean[ldr] | rstd[ldr] | c1[N] (ldr >= M, a multiple of 4). */
#define LPI_EPI_LN_QUICKGELU 4 /* ... followed by the QuickGELU epilogue (aux as for LPI_EPI_QUICKGELU).  Both: bf16 / f16 operands, shapes the
                               * persistent 256x256 kernel takes (LPI_ENOSYS otherwise: the caller runs LayerNorm + GEMM). */
#define LPI_EPI_RES_ROWSTATS 5 /* LPI_EPI_NONE on the fp16 residual stream (c_dtype LPI_F16, residual required), and the ROW STATISTICS of what it
                               * stores come out with it: `aux` is an f32 buffer of N/128 slots x 2 x ldaux (ldaux >= M, a multiple of 4) and
                               * aux[(2 j) ldaux + m] = sum, aux[(2 j + 1) ldaux + m] = sum of squares of the 128 stored (fp16-rounded) values
                               * C[m, 128 j .. 128 j + 127], summed in a fixed order.  lpi_ln_stats_finalize turns them into the mean / rstd the
                               * LayerNorm-fold epilogues of the NEXT GEMM read (model.py:172-177: x + attn(..) -> ln_2, x + mlp(..) -> the next
                               * block's ln_1), so no separate pass over the stream is needed.  Same shapes as the LN-fold epilogues. */

int lpi_version(void);   /* the C-ABI version: changes with every change of a signature or of an argument's meaning (bindings check it) */
/* number of kernels launched by this library since load (tests use it to prove the HIP path ran) */
uint64_t lpi_launch_count(void);

/* tuning knobs (speed only, never results):
 *   key 0 / 1  minimum number of 256x256 tiles for which lpi_gemm_nt uses the phased 256x256 kernel instead of the 128x128 one,
 *              for bf16 / f32 operands (defaults 1 / 1500; INT_MAX disables it);
 *   key 2      >= 0 (default 0): 2-byte-operand launches of the 256x256 kernel use its PERSISTENT form (a workgroup per CU walks its
 *              tiles; store-only epilogues: the next tile's first K-tile lands under the epilogue; epilogues that load a 2-byte
 *              residual / u tile: that tile comes to LDS by LDS-DMA; same results bit for bit); 2: store-only epilogues only;
 *              -1: one tile per workgroup everywhere;
 *   key 3      != 0 forces the two-pass attention backward where the fused single-pass kernel would be used (bf16, all four head
 *              matrices resident in LDS);
 *   key 4      row-tile group size of the 256x256 kernel's XCD-aware tile order (default 0 = 8; measured flat from 4 to 16);
 *   key 5      bf16 launches with at least 16 but fewer than this many 256x256 tiles use 256x128 tiles instead (twice the
 *              workgroups for launches that would leave the chip half empty; default 160, 0 disables it; same results bit for bit);
 *   key 6      != 0 (default): a 256x256 launch of 256k + rem tiles with rem <= 128 runs those rem tiles as 2*rem tiles of 256x128
 *              inside the same launch — one round of half tiles instead of a half-empty round (bf16; same results bit for bit);
 *   key 7      attention backward generation for 2-byte operands: 0 (default) the streamed single-pass kernel of attention4.hip where it
 *              applies and is faster (non-causal, 160 < L <= 224: the vision tower), the one-head-per-workgroup kernels of attention.hip
 *              elsewhere; 1 the kernels of attention.hip everywhere; 5 forces attention4.hip at every L it takes (same products, delta
 *              summed in another order: equal to rounding, not bit for bit).
 *   key 8      != 0: lpi_gemm_nt_grouped never groups (issues its problems one after the other; A/B switch, same bits).
 *   key 11     > 0: the streamed attention backward launches at most this many workgroups (tests: several heads per workgroup at small B H).
 *   key 12     A/B switches of the streamed attention backward (bit 0: K / V of the next head as one burst instead of spread over the head).
 *   key 13     != 0: the attention forward keeps padded (160-byte) K / V image rows where it would use the swizzled unpadded ones (Lp = 288; a TEST hook, same bits).
 *   key 14     1: the generic epilogue of the persistent GEMM everywhere (no half-width staging for store-only 2-byte outputs): a TEST hook, the bit-for-bit
 *              reference of the half-width staging (same bits).
 *   key 15     tile order of the persistent 256x256 GEMM for weights that do not fit an XCD's L2 next to the activation stream (round 5): 0 (default) = the
 *              N-tiles (an even number) of a weight above 3 MB are cut into two SLICES and the tiles run slice-major, so that each XCD keeps one slice
 *              resident instead of re-reading the whole weight every round; 2 / 3: that many slices wherever N divides; -1: off.  Same bits.
 *   key 9      > 0: minimum number of waves (<= 8) of a workgroup of the one-head attention kernels on RAGGED batches (the text tower: thousands of
 *              workgroups of a few dozen rows, bound by the latency of their staging loads; the waves beyond the row blocks only help to stage).  Same bits.
 *   key 10     reserved (0).  Returns LPI_EINVAL for a key outside 0..15. */
int lpi_set_tuning(int key, int value);
int lpi_get_tuning(int key);   /* current value of a knob (>= 0), LPI_EINVAL for a key outside 0..15 */

/* ---- a4: nn.Linear / in_proj / out_proj / c_fc / c_proj / conv1-as-matmul and every dgrad --------------
 * C[M,N] = epi(alpha * A[M,K] . B[N,K]^T + bias[N]) + residual[M,N]
 * replaces: models/clip/model.py:175-177 (c_fc, c_proj), :172,185 (nn.MultiheadAttention in/out proj),
 *           :215,228 (conv1 as per-patch matmul), :257 (x @ proj); prompt_learner.py:61 (@ text_projection);
 *           slinet.py:139 (logit_scale * I @ T^T); and their autograd dgrads (B = pre-transposed weight).
 * A, B: `dtype` elements.  C: `c_dtype` elements.  bias: f32 or NULL.  residual: f32 or NULL; with c_dtype == LPI_F16 (bf16
 * operands, LPI_EPI_NONE only) the residual is required and is fp16 like C — the fp16 residual stream.  aux: `dtype` or NULL. */
int lpi_gemm_nt(int dtype, int c_dtype, int M, int N, int K,
                const void* A, int lda, const void* B, int ldb, void* C, int ldc,
                const float* bias, const void* residual, int ldr,
                int epilogue, void* aux, int ldaux, float alpha, void* stream);

/* SEVERAL such GEMMs in one launch (a GROUPED launch): `count` problems of the same operand type, output type and epilogue kind
 * (residual / aux present in all of them or in none) — e.g. the vision tower's and the text tower's c_fc of the same layer
 * (models/clip/model.py:175-177 runs them as two nn.Linear calls of two independent towers).  With count == 2 and shapes the
 * persistent 256x256 kernel takes, the second problem's tiles follow the first's in one persistent launch: they fill the first
 * problem's partial last round of CUs and run at the large kernel's rate instead of as a small launch of their own.  Any other
 * combination is issued as `count` lpi_gemm_nt calls in order — the results are the same bits either way.  `descs` is HOST memory
 * (read during the call); the pointers inside are device memory.  The launches are attributed to kernel LPI_GEMM_K_256* when grouped
 * (lpi_gemm_last_kernel). */
typedef struct lpi_gemm_desc {
    int M, N, K;
    const void* A; int lda;
    const void* B; int ldb;
    void* C; int ldc;
    const float* bias;
    const void* residual; int ldr;
    void* aux; int ldaux;
} lpi_gemm_desc;
int lpi_gemm_nt_grouped(int dtype, int c_dtype, int epilogue, float alpha, int count, const lpi_gemm_desc* descs, void* stream);
/* 1 if the last lpi_gemm_nt_grouped call of this thread ran as ONE grouped launch, 0 if it fell back to separate launches */
int lpi_gemm_last_grouped(void);

/* 1 if lpi_gemm_nt / lpi_gemm_nt_grouped take the LayerNorm-fold epilogues (LPI_EPI_LN, LPI_EPI_LN_QUICKGELU) for this operand type and shape */
int lpi_gemm_ln_supported(int dtype, int M, int N, int K);
/* mean[m] = S / d, rstd[m] = 1 / sqrt(Q / d - mean^2 + eps) from the slot sums S, Q an LPI_EPI_RES_ROWSTATS GEMM left in `part` (d / 128 slots,
 * row stride ld): what nn.LayerNorm (model.py:154-160, biased variance, eps 1e-5) computes from the row.  `_pair`: the two towers' in one launch. */
int lpi_ln_stats_finalize(int rows, int d, const float* part, int ld, float eps, float* mean, float* rstd, void* stream);
/* Guard of the ONE-SWEEP row statistics (var = E[x^2] - mean^2 in f32: lpi_ln_stats_finalize(_pair), and the out_mean / out_rstd of lpi_vis_assemble_fwd,
 * lpi_txt_embed_fwd(_varlen), lpi_prompt_add(_varlen) and the PROMPT_ADD row job).  The form loses digits as (mean / std)^2 * 1e-7; LayerNorm itself
 * (model.py:154-160) does not.  `counter` (DEVICE int32; NULL = off, the default) and `flag` are remembered for the calling HOST THREAD: every later launch
 * of those kernels from this thread adds the number of rows with mean^2 > 64 var (8 deviations: the error is ~6e-6 there) to *counter, and the row that
 * takes it from 0 to 1 also stores 1 to *flag.  `flag` (optional) may be a word of PINNED HOST memory (hipHostMalloc / torch pin_memory: the library
 * resolves its device alias with hipPointerGetAttributes and returns LPI_EINVAL for memory the device cannot write): the host then reads its own word
 * whenever it likes — no copy, no event, no synchronisation — and switches to the two-sweep statistics pass (lpi_layernorm_fwd with y = NULL);
 * lpi_amd/engine.py does so from the next forward.  A speed knob's safety net: never changes a result by itself. */
int lpi_rowstat_guard(int32_t* counter, int32_t* flag);
int lpi_ln_stats_finalize_pair(int rows0, int d0, const float* part0, int ld0, float* mean0, float* rstd0,
                               int rows1, int d1, const float* part1, int ld1, float* mean1, float* rstd1, float eps, void* stream);

/* Few-row GEMM in ONE launch (csrc/gemm_rows.hip; round 6): `count` = 1 or 2 problems (the two towers' GEMM of the same op on the pooled rows of the last
 * block / the heads: model.py:172-177,185,257, prompt_learner.py:61 on B rows per tower, and their dgrads), same operand types and epilogue kind, epilogues
 * LPI_EPI_NONE (+ f32 residual) / LPI_EPI_QUICKGELU (+ aux = gelu'(u)) / LPI_EPI_DQUICKGELU as lpi_gemm_nt.  A workgroup owns a 32 x 32 output tile over the
 * whole K range (eight waves cut K, partial tiles meet in LDS in a fixed order): no scratch, no second launch, deterministic.  M, N multiples of 32, K a
 * multiple of 64 elements (32 for f32: whole 128-byte blocks), rows 16-byte aligned: lpi_gemm_nt_rows_supported says 1 for such a shape.  Replaces rounds 2-5's split-K partial + reduction launch pairs (lpi_gemm_nt_splitk*, gone from the ABI in 604): the same
 * sums in another f32 order, half the time (profiles/r06_experiments.md section 10).  Attributed to LPI_GEMM_K_ROWS. */
int lpi_gemm_nt_rows_supported(int dtype, int M, int N, int K);
int lpi_gemm_nt_rows(int dtype, int c_dtype, int epilogue, float alpha, int count, const lpi_gemm_desc* descs, void* stream);

/* ---- erf-GELU behind a plain c_fc GEMM (since 623)        replaces: nn.GELU() in the MLP of a checkpoint trained with it (OpenCLIP ViT-B/32, B/16, L/14) ----
 * IN PLACE: on entry g[rows, cols] (`dtype`, row stride ldg) holds the pre-activation u = c_fc output with its bias; on exit gelu(u) = u Phi(u).  aux (row
 * stride ldaux) receives gelu'(u) = Phi(u) + u phi(u), the tile LPI_EPI_DQUICKGELU multiplies by; aux == NULL: not wanted (ldaux is not looked at), and the
 * bits written to g are the same.  (dtype, aux_dtype) = (LPI_F32, LPI_F32) | (LPI_BF16, LPI_BF16) | (LPI_F16, LPI_BF16) — the GEMM epilogues' rule for the
 * saved derivative — anything else is LPI_EINVAL, with or without aux.  f32 arithmetic in registers: Phi(u) = erfc(-u / sqrt 2) / 2 (erfc, not 1 + erf: the
 * negative tail keeps its relative accuracy), phi(u) = exp(-u^2 / 2) / sqrt(2 pi).  Every finite u the type holds gives finite values (+-0, a square that
 * overflows, the f16 / bf16 / f32 maxima); NaN / Inf are out of contract.  A lane moves 16 bytes: cols a positive multiple of 8, ldg and ldaux >= cols and
 * multiples of 8 elements, g and aux 16-byte aligned, rows >= 1 — LPI_EINVAL before any launch otherwise.  Only the rows x cols elements are read or written;
 * the ld gaps are never touched.  One launch. */
int lpi_gelu_erf_fwd(int dtype, int aux_dtype, long rows, int cols, void* g, long ldg, void* aux, long ldaux, void* stream);

/* ---- a5: LayerNorm (fp32 statistics, eps 1e-5)            replaces: models/clip/model.py:154-160 ------
 * x_dtype: storage type of the residual stream x — LPI_F32, or LPI_F16 in bf16 mode (statistics and arithmetic are f32 either way).
 * fwd: y[r,:] = (x[r,:]-mean)*rstd*gamma+beta for r < rows; x `x_dtype` [rows,d] (row stride ldx), y `dtype`.
 * bwd: dx[r,:] (f32, in/out: residual-stream gradient) += LN'(dy[r,:]); optionally also writes a `cast_dtype`
 *      copy dx_cast (the next dgrad GEMM's operand).  dx == NULL: dx_cast itself is the in/out gradient stream (bf16 mode keeps
 *      no f32 copy).  dy is `dy_dtype`.  accumulate == 0: the gradient stream is WRITTEN (= LN'(dy)) instead of added to — the first
 *      backward kernel of a tower then needs no zero-fill of the [rows, d] stream.
 *
 * Leading dimensions and alignment of the row operations (this section, the pooled heads, the vision front end, lpi_row_jobs and the MX-FP8 rows below;
 * anything else is LPI_EINVAL before any launch — for a pair or a job list before the FIRST launch; each leading dimension is its own argument and may differ
 * from every other — tests/test_rowop_strides_gpu.py).  The rule is the widest access the kernels make to the operand (since 618; up to 617 the row kernels
 * only asked for leading dimensions in multiples of four elements):
 *   a [rows, d] operand with a row stride (x / ldx, y / ldy, dy / lddy, dx / lddx, dx_cast / ldcast, patch_emb / ldpe, cols / ldcols) is moved FOUR ELEMENTS at a
 *     time: d a multiple of 4 (<= 2048), ld >= d and a multiple of 4 elements, the pointer aligned to 4 elements (16 bytes f32, 8 bytes bf16 / f16).  dx == NULL /
 *     dx_cast == NULL: lddx / ldcast still a multiple of 4 (their size is not looked at).  Streams without a row stride of their own ([B L, d]: x, dx, dx_cast of
 *     lpi_pool_ln_*, x0, dx0, the x of lpi_prompt_add) take the same pointer rule;
 *   gamma, beta, cls, pos, prompt0 / prompt_l / ctx rows, dprompt, the f32 copy `out2` of POOL_LN_FWD: read or written as four floats, 16-byte aligned;
 *     mean, rstd, inv_norm, the statistics outputs: one float, no rule;
 *   the fp16-stream LayerNorms move 16 bytes per lane (a half wave per row) when d and every leading dimension of the call are multiples of 8 and x, y (dy, x,
 *     dx_cast with dx == NULL) are 16-byte aligned, and the four-element kernels otherwise: the leading dimension picks the kernel, the results are the same.  The
 *     statistics-only form (y == NULL), the fused pair launch and LN_BWD_ROWS_H16 have the 16-byte kernel only: those conditions are required;
 *   lpi_gather_batch_rows(_varlen): whole 16-byte units (cols, ld_src >= cols, ld_dst >= cols, both pointers); lpi_scatter_add_rows / SCATTER_ADD: the four-element rule
 *     above for src / ld_src and dst / ld_dst (up to 617 f32 rows were held to 8 bytes); lpi_transpose(2), lpi_copy_rows, lpi_ln_stats_finalize(_pair): one element per lane — lds >= cols, ldd >= rows (ld >= rows), any step;
 *   lpi_mx8_quantize / lpi_layernorm_mx8_fwd: ldx >= K (d) in multiples of 4, x aligned to 4 elements, ldq >= K in multiples of 4 with q 4-byte aligned, lds >=
 *     K / 32 in any step (one scale byte per store), gamma / beta 16-byte aligned — unchanged, each exactly as wide as its access. */
int lpi_layernorm_fwd(int dtype, int x_dtype, int rows, int d, const void* x, int ldx, const float* gamma, const float* beta,
                      void* y, int ldy, float* mean, float* rstd, void* stream);
int lpi_layernorm_bwd(int dy_dtype, int cast_dtype, int x_dtype, int rows, int d, const void* dy, int lddy,
                      const void* x, int ldx, const float* gamma, const float* mean, const float* rstd,
                      float* dx, int lddx, void* dx_cast, int ldcast, int accumulate, void* stream);
/* TWO LayerNorms in one launch — the vision and the text tower's LayerNorm of the same layer (two independent nn.LayerNorm calls of two
 * independent towers, model.py:154-160): the text tower's alone is a few-microsecond kernel that is mostly launch ramp.  `d` points to two
 * descriptors in HOST memory; with the bf16 / f16 operand types over the fp16 residual stream they run as one kernel, any other combination
 * as two lpi_layernorm_fwd / _bwd calls (same results either way). */
typedef struct lpi_ln_fwd_desc {
    int rows, d;
    const void* x; int ldx;
    const float* gamma; const float* beta;
    void* y; int ldy;
    float* mean; float* rstd;
} lpi_ln_fwd_desc;
typedef struct lpi_ln_bwd_desc {
    int rows, d;
    const void* dy; int lddy;
    const void* x; int ldx;
    const float* gamma; const float* mean; const float* rstd;
    float* dx; int lddx;
    void* dx_cast; int ldcast;
    int accumulate;
} lpi_ln_bwd_desc;
/* y = NULL (both problems of a pair): the row statistics only — mean / rstd are written, nothing else (fp16 stream; gamma / beta unused).  Used
 * with the LayerNorm-fold GEMM epilogues (LPI_EPI_LN), which apply the normalisation themselves; also accepted by lpi_layernorm_fwd. */
int lpi_layernorm_fwd_pair(int dtype, int x_dtype, const lpi_ln_fwd_desc* d, void* stream);
int lpi_layernorm_bwd_pair(int dy_dtype, int cast_dtype, int x_dtype, const lpi_ln_bwd_desc* d, void* stream);
/* The same backward for P rows per sample only (the first block: nothing upstream of the prompt slots is trainable, sprompt.py:230-237):
 * dy is compact [B*P, d]; x, mean/rstd and the gradient stream are the full [B*L, .] arrays, touched at rows b*L + row0 + p. */
int lpi_layernorm_bwd_rows(int dy_dtype, int cast_dtype, int x_dtype, int B, int L, int row0, int P, int d, const void* dy, int lddy,
                           const void* x, int ldx, const float* gamma, const float* mean, const float* rstd,
                           float* dx, int lddx, void* dx_cast, int ldcast, int accumulate, void* stream);
/* dst[(b*P + p), 0:cols] = src[(b*L + row0 + p), 0:cols] (`dtype` elements, 16-byte aligned rows): packs the prompt rows of a stream */
int lpi_gather_batch_rows(int dtype, int B, int L, int row0, int P, int cols, const void* src, int ld_src, void* dst, int ld_dst,
                          void* stream);

/* ---- a4: prompted multi-head attention, head_dim 64   replaces: models/clip/model.py:183-185 -----------
 * qkv: [B*L, 3*d] `dtype` (q | k | v, heads contiguous by 64).  ctx: [B*L, d] `dtype`.  lse: [B, H, L] f32.
 * softmax(q k^T / 8 + causal mask) v; causal != 0 applies the text tower's strict upper-triangular -inf mask
 * (model.py:347-353).  Backward recomputes P from lse; `delta` is [B,H,L] f32 SCRATCH: the kernels that make two passes over the scores
 * leave rowsum(dctx*ctx) there, the streamed single-pass backward (attention4.hip) keeps it in LDS and does not touch the buffer at L <= 224; at
 * 224 < L <= 288 (two key-window launches) its first launch leaves -rowsum(dctx*ctx)/8 there for the second.  The contents are unspecified after the call.
 * dqkv: [B*L, 3*d] `dtype`.  L <= 288: one workgroup per (sample, head) keeps the head's K and V in LDS (attention.hip, attention4.hip).  Round 6: NON-CAUSAL
 * UNIFORM sequences of 288 < L <= 1024 tokens (ViT-L/14@336px: 577 + prompts) run tiled over the keys with an online softmax (attn_long.hip, kernels in attn_walk.h: forward one
 * launch, backward two — dQ + delta, then dK / dV; the backward computes every row, `rows_needed` of the _prefix form is ignored there); causal or ragged
 * sequences of that length are refused with LPI_EINVAL.
 *
 * Alignment of the attention operands (every entry point of this section and of the _varlen / _prefix / _layout / _shared / pooled / spool forms below; anything
 * else is LPI_EINVAL before any launch; each leading dimension is its own argument and may differ from every other — tests/test_attn_strides_gpu.py).  The rule
 * is the widest access the kernels make to the operand: 16-byte row loads and stores for matrices, one element for what a lane stores alone.
 *   lpi_attn_fwd / _varlen / _shared / _pair (interleaved): ldqkv >= 3 H 64 and a whole number of 16-byte units; ldctx >= H 64 and a multiple of 8 ELEMENTS for
 *     every dtype (f32 too: stricter than its 16-byte stores need); qkv, ctx 16-byte aligned.
 *   lpi_attn_bwd / _varlen / _prefix / _shared: ldqkv, lddqkv >= 3 H 64, ldctx, lddctx >= H 64, each a whole number of 16-byte units; qkv, ctx, dctx, dqkv (and
 *     shared_dkv) 16-byte aligned.  A ctx that goes through both directions therefore takes ldctx in multiples of 8 elements.
 *   layout forms (lpi_attn_fwd_one / _pair with layout strides, lpi_attn_bwd_layout; 2-byte types): every leading dimension and layout stride >= 64 and a multiple
 *     of 8 elements; the same pointers 16-byte aligned.
 *   lpi_shared_kv_reduce: lddqkv >= 3 H 64 and a multiple of 4 elements; partial 16-byte aligned, dqkv 8-byte (2-byte types) / 16-byte (f32) aligned.
 *   lpi_attn_pooled_* (all forms): ldqkv >= 3 H 64, ldq, lddctx >= H 64, whole 16-byte units, q, qkv, dctx 16-byte aligned (read four elements at a time); ctx, dq
 *     and dqkv are stored one element at a time: ldctx, lddq >= H 64 and lddqkv >= 3 H 64 in ANY step, no pointer alignment beyond the element's.  With
 *     shared_rows > 0 (lpi_attn_pooled_bwd_desc / _bwd_pair) dqkv and shared_dkv go through lpi_shared_kv_reduce behind the pooled kernel, so that function's
 *     rule holds for them and is refused BEFORE that kernel: lddqkv a multiple of 4 elements, dqkv 8-byte (f32: 16-byte) aligned, shared_dkv 16-byte aligned
 *     (since 617; up to 616 such a call returned LPI_EINVAL from the reduce, after the pooled kernel had run).
 *   lpi_spool_attn_fwd / _bwd: ldx, ldw, ldq, lddctx >= d, ldwt >= 3 d, multiples of 8 elements, x, Wqkv, WqkvT, q, dctx 16-byte aligned; lddh >= d and a multiple
 *     of 4 elements, dh 8-byte aligned (8-byte stores); ctx and dq are stored one element at a time: ldctx, lddq >= d in any step.  scratch, gamma and beta are
 *     moved four floats at a time: 16-byte aligned (since 617; not checked up to 616).  bqkv, mean, rstd, lse: one float at a time.
 *   lse / delta: f32, written one element at a time, inside [B, H, L] ((B + 1) H L on a shared prefix) — never for the rows between L and the 32-row tile. */
int lpi_attn_fwd(int dtype, int B, int L, int H, const void* qkv, int ldqkv, void* ctx, int ldctx,
                 float* lse, int causal, void* stream);
int lpi_attn_bwd(int dtype, int B, int L, int H, const void* qkv, int ldqkv, const void* ctx, int ldctx,
                 const void* dctx, int lddctx, const float* lse, float* delta, void* dqkv, int lddqkv,
                 int causal, void* stream);
/* ---- Attention for heads that are NOT 64 wide (since 624; widths 88 and 104 since 625; lpi_amd/csrc/attn_hd.hip).  replaces: nn.MultiheadAttention of a vision
 * tower with width / heads != 64 (OpenCLIP ViT-H/14: 1280 = 16 heads of 80, ViT-g/14: 1408 = 16 of 88, ViT-bigG/14: 1664 = 16 of 104; the reference's
 * model.py:292 computes width // 64 and cannot build them).  The interleaved
 * layout of lpi_attn_fwd / lpi_attn_bwd with head_dim in place of 64 — qkv, dqkv [B*L, 3*H*head_dim], ctx, dctx [B*L, H*head_dim], lse, delta [B, H, L] f32 —,
 * softmax(q k^T head_dim^-0.5) v, NON-CAUSAL, UNIFORM sequences, at every 1 <= L <= 1024 in the key-walking form of attn_walk.h (forward one launch,
 * backward two: dQ + delta, then dK / dV; every row of dqkv is written; deterministic).  dtype as lpi_attn_fwd / lpi_attn_bwd at L > 288: LPI_F32, LPI_BF16,
 * LPI_F16 (backward: saved qkv / ctx fp16, dctx / dqkv bf16).
 * The rule (anything else is LPI_EINVAL before any launch): head_dim is 80, 88 or 104 (the widths that are built, by list: 64, 72, 96 are refused); B, L, H > 0,
 *   L <= 1024, B H <= 65535 (a grid extent);
 *   forward: ldqkv >= 3 H head_dim and a whole number of 16-byte units, ldctx >= H head_dim and a multiple of 8 ELEMENTS for every dtype; qkv, ctx 16-byte aligned;
 *   backward: ldqkv, lddqkv >= 3 H head_dim, ldctx, lddctx >= H head_dim, each a whole number of 16-byte units; qkv, ctx, dctx, dqkv 16-byte aligned;
 *   no pointer NULL (stream excepted).  No load or store touches an element outside the head_dim of its own (row, head) slice or a row >= B L (88 and 104 end in
 *   half a 16-column tile: the other half exists in registers and LDS only); lse / delta are written one element at a time inside [B, H, L].
 *   lpi_attn_hd_supported: 1 where (L, H, head_dim) is inside this rule, without a launch. */
int lpi_attn_hd_supported(int L, int H, int head_dim);
int lpi_attn_hd_fwd(int dtype, int B, int L, int H, int head_dim, const void* qkv, int ldqkv, void* ctx, int ldctx, float* lse, void* stream);
int lpi_attn_hd_bwd(int dtype, int B, int L, int H, int head_dim, const void* qkv, int ldqkv, const void* ctx, int ldctx, const void* dctx, int lddctx,
                    const float* lse, float* delta, void* dqkv, int lddqkv, void* stream);
/* The same attention for ONE query row per sample — token idx[b] (NULL: token 0) — used in the LAST block, whose output is read
 * at the pooled token only (model.py:255 CLS, prompt_learner.py:61 EOT): exact dead-row elimination.  q, ctx, dctx, dq: [B, d]
 * `dtype` (row b = sample b); K and V are read from columns d..3d of qkv [B*L, 3d]; lse: [B, H] f32.  causal != 0: keys <= idx[b].
 * bwd writes dK, dV into columns d..3d of dqkv for all L rows of every sample (zeros behind the mask); columns 0..d are untouched. */
int lpi_attn_pooled_fwd(int dtype, int B, int L, int H, const void* q, int ldq, const void* qkv, int ldqkv, const int32_t* idx,
                        void* ctx, int ldctx, float* lse, int causal, void* stream);
int lpi_attn_pooled_bwd(int dtype, int B, int L, int H, const void* q, int ldq, const void* qkv, int ldqkv, const int32_t* idx,
                        const void* dctx, int lddctx, const float* lse, void* dq, int lddq, void* dqkv, int lddqkv, int causal,
                        void* stream);

/* ---- RAGGED batches (`_varlen`): samples of different lengths packed back to back --------------------------------------------
 * The text tower is causal and read at the EOT token only (model.py:347-353, prompt_learner.py:61), so the token rows BEHIND a
 * sample's own EOT can reach neither its feature nor any gradient: the reference computes them (every caption is padded to 77
 * tokens, clip.py:185-221) and throws them away.  Here a batch may be packed: sample b owns rows row_start[b] .. row_start[b+1]-1 of
 * every [rows, *] array (row_start: B + 1 int32 on the device, ascending; L_b = row_start[b+1] - row_start[b] <= L).  `L` stays the
 * MAXIMUM length (launch geometry, the [B, H, L] layout of lse / delta, the [B, L] layout of ids).  row_start == NULL is exactly the
 * function without the suffix (row(b, l) = b*L + l).  Row-wise kernels (LayerNorm, GEMM) need no variant: they see sum_b L_b rows.
 * Kernels that take a per-sample token index `idx` (lpi_pool_ln_fwd/bwd, lpi_gather_rows, lpi_scatter_rows, lpi_scatter_add_rows)
 * accept L == 0, which makes idx[b] an ABSOLUTE row index (= row_start[b] + token). */
int lpi_attn_fwd_varlen(int dtype, int B, int L, const int32_t* row_start, int H, const void* qkv, int ldqkv, void* ctx, int ldctx,
                        float* lse, int causal, void* stream);
int lpi_attn_bwd_varlen(int dtype, int B, int L, const int32_t* row_start, int H, const void* qkv, int ldqkv, const void* ctx, int ldctx,
                        const void* dctx, int lddctx, const float* lse, float* delta, void* dqkv, int lddqkv,
                        int causal, void* stream);
/* TWO attention forwards in one launch — the vision and the text tower's of the same layer (two independent nn.MultiheadAttention calls,
 * model.py:183-185): the text tower's alone is a ~15 us chain of dependent memory round trips with the chip nearly idle.  `d`: two descriptors
 * in HOST memory (row_start may be NULL).  bf16 / f16 operands run as one kernel, f32 as two launches; same results either way. */
typedef struct lpi_attn_fwd_desc {
    int B, L, H;
    const int32_t* row_start;
    const void* qkv; int ldqkv;
    void* ctx; int ldctx;
    float* lse;
    int causal;
    int shared_rows;       /* 0, or the shared prefix of lpi_attn_fwd_shared (causal, row_start given) */
    /* LAYOUT (round 6; all 0 = the interleaved default above).  Element (row, head h, which in {q, k, v}, c) of qkv sits at row * ldqkv + h * qkv_hs +
     * which * qkv_vs + c, element (row, h, c) of ctx at row * ldctx + h * ctx_hs + c (elements; multiples of 8).  Head-BLOCKED planes [3 H][rows][64] /
     * [H][rows][64] — what the GEMMs write and read with a plane stride (lpi_gemm_nt_planes): ldqkv = ldctx = 64, qkv_hs = ctx_hs = rows * 64, qkv_vs =
     * H * rows * 64: a (sample, head) slice is one contiguous run.  2-byte types, uniform sequences (row_start = NULL, shared_rows = 0) only. */
    int qkv_hs, qkv_vs, ctx_hs;
} lpi_attn_fwd_desc;
int lpi_attn_fwd_pair(int dtype, const lpi_attn_fwd_desc* d, void* stream);
/* The same backward when only the FIRST `rows_needed` token rows of dqkv are wanted (the first block: nothing upstream of the prompt slots
 * 1 .. P is trainable, sprompt.py:230-237, so only dQ / dK / dV of rows < 1 + P are read): delta is produced for every row, the rows of dqkv
 * behind rows_needed MAY be left unwritten (the 2-byte kernels skip whole 32-row blocks behind it; rows_needed >= L is lpi_attn_bwd_varlen). */
int lpi_attn_bwd_prefix(int dtype, int B, int L, const int32_t* row_start, int rows_needed, int H, const void* qkv, int ldqkv, const void* ctx,
                        int ldctx, const void* dctx, int lddctx, const float* lse, float* delta, void* dqkv, int lddqkv, int causal,
                        void* stream);
/* The backward of an explicit LAYOUT (lpi_attn_fwd_desc): lay = {qkv_hs, qkv_vs, dqkv_hs, dqkv_vs, ctx_hs, dctx_hs} (elements, multiples of 8); 2-byte
 * types, non-causal, uniform sequences; rows_needed as lpi_attn_bwd_prefix (<= 0 or >= L: all rows).  Where the one-head-per-workgroup kernels run (short
 * sequences, tuning keys 3 / 7) ctx_hs and dctx_hs must be 64.  delta: [B, H, L] f32 scratch as above. */
int lpi_attn_bwd_layout(int dtype, int B, int L, int rows_needed, int H, const void* qkv, int ldqkv, const void* ctx, int ldctx, const void* dctx, int lddctx,
                        const float* lse, float* delta, void* dqkv, int lddqkv, const int32_t* lay /* HOST, 6 ints */, void* stream);
/* ONE forward in descriptor form: the single-problem call that takes the layout strides (all zero: lpi_attn_fwd_varlen / _shared) */
int lpi_attn_fwd_one(int dtype, const lpi_attn_fwd_desc* d, void* stream);
/* idx[b] stays the token index WITHIN sample b (the causal limit) */
int lpi_attn_pooled_fwd_varlen(int dtype, int B, int L, const int32_t* row_start, int H, const void* q, int ldq, const void* qkv, int ldqkv,
                               const int32_t* idx, void* ctx, int ldctx, float* lse, int causal, void* stream);
int lpi_attn_pooled_bwd_varlen(int dtype, int B, int L, const int32_t* row_start, int H, const void* q, int ldq, const void* qkv, int ldqkv,
                               const int32_t* idx, const void* dctx, int lddctx, const float* lse, void* dq, int lddq, void* dqkv,
                               int lddqkv, int causal, void* stream);
/* The two towers' pooled-row attention (last block) as ONE launch: d[i] = the arguments of lpi_attn_pooled_fwd_varlen / _bwd_varlen (fwd uses q, qkv, idx,
 * ctx, lse; bwd q, qkv, idx, dctx, lse, dq, dqkv).  Bit for bit the two single launches. */
typedef struct lpi_attn_pooled_desc {
    int B, L, H;
    const int32_t* row_start;
    const void* q; int ldq;
    const void* qkv; int ldqkv;
    const int32_t* idx;
    void* ctx; int ldctx;
    float* lse;
    const void* dctx; int lddctx;
    void* dq; int lddq;
    void* dqkv; int lddqkv;
    int causal;
    int shared_rows;       /* 0, or the shared prefix (below): idx[b] stays the query's POSITION in sample b's sequence, L the longest sequence */
    float* shared_dkv;     /* bwd with shared_rows > 0: f32 scratch [B, shared_rows, 2 H 64] */
} lpi_attn_pooled_desc;
int lpi_attn_pooled_fwd_pair(int dtype, const lpi_attn_pooled_desc* d /* [2] */, void* stream);
int lpi_attn_pooled_bwd_pair(int dtype, const lpi_attn_pooled_desc* d /* [2] */, void* stream);
/* ONE problem in descriptor form (the only single-problem form that takes the shared-prefix fields). */
int lpi_attn_pooled_fwd_desc(int dtype, const lpi_attn_pooled_desc* d, void* stream);
int lpi_attn_pooled_bwd_desc(int dtype, const lpi_attn_pooled_desc* d, void* stream);

/* ---- The LAST block's attention WITHOUT K and V (round 6; lpi_amd/csrc/attn_stream.hip).  replaces: models/clip/model.py:183-185 for the block whose output
 * only the pooled token reads (model.py:255).  With ONE live query per (sample, head), q_h . k_l / 8 = LN1(x_l) . (W_k,h^T q_h / 8) + const and
 * sum_l p_l v_l = W_v,h (sum_l p_l LN1(x_l)) + b_v,h: the block needs two passes over the sample's rows of the residual stream (LayerNorm applied on the fly from
 * the row statistics) instead of the [B L, 2 d] K / V projection, its dgrad and the single-query attention over them.  Exact algebra.
 *   w_dtype: LPI_BF16 | LPI_F16 = type of q [B, ldq], Wqkv [3 d, ldw] (in_proj weight: rows d..2d = W_k, 2d..3d = W_v), its transpose WqkvT [d, ldwt >= 3 d]
 *   and ctx [B, ldctx]; bqkv f32 [3 d];
 *   x: fp16 [B L, ldx], the block's input rows (uniform L per sample); mean / rstd f32 [B L]: ln_1's statistics of those rows; gamma / beta f32 [d]: ln_1's affine;
 *   scratch f32 [4 B H d] (the forward writes the first half, the backward reads its first quarter and writes the second half); lse f32 [B, H].
 *   Backward: dctx bf16 [B, lddctx] -> dq bf16 [B, lddq] (gradient of the pooled queries) and dh bf16 [B L, lddh] = d LN1(x_l) of EVERY row (the K / V path's
 *   gradient; the caller adds the pooled rows' query path as before); the backward's weight operands are the BF16 weight and its transpose whatever the
 *   forward's type was.  H <= 16 heads of 64, L <= 288: lpi_spool_attn_supported. */
int lpi_spool_attn_supported(int L, int H, int d);
int lpi_spool_attn_fwd(int w_dtype, int B, int L, int H, const void* q, int ldq, const void* Wqkv, int ldw, const void* WqkvT, int ldwt, const float* bqkv, const void* x, int ldx,
                       const float* mean, const float* rstd, const float* gamma, const float* beta, float* scratch, float* lse, void* ctx, int ldctx, void* stream);
int lpi_spool_attn_bwd(int B, int L, int H, const void* Wqkv /* bf16 */, int ldw, const void* WqkvT /* bf16 */, int ldwt, const void* x, int ldx, const float* mean,
                       const float* rstd, const float* gamma, float* scratch, const float* lse, const void* dctx, int lddctx, void* dq, int lddq, void* dh, int lddh,
                       void* stream);

/* ---- SHARED PREFIX of the text tower (round 5).  replaces nothing new: the same model.py:179-193, 347-353 and prompt_learner.py:155-163 arithmetic
 * on fewer rows.  In training every caption is [SOT][n_ctx context slots][caption tokens][EOT] and the context / deep prompts are broadcast over the
 * batch (slinet.py:119-130), so positions 0 .. n_ctx of ALL samples hold the same rows in every block: under the causal mask they attend only to each
 * other.  Layout: global rows [0, shared_rows) = those positions, stored ONCE; sample b owns rows row_start[b] .. row_start[b+1]-1 = its positions
 * shared_rows, shared_rows + 1, ... (row_start[0] = shared_rows); L = the longest sequence INCLUDING the shared positions; lse / delta hold
 * (B + 1) x H x L floats, sample index B being the shared sequence, indexed by OWN row.  Every row-wise op (LayerNorm, GEMMs) just sees fewer rows;
 * attention reads keys [shared rows | own rows].  The gradient that reaches the shared rows is the batch SUM (what lpi_rows_sum_over_batch produces
 * in the plain layout): dK / dV of the shared keys are summed over the samples in f32 in a fixed order (bitwise reproducible), so the prompt
 * gradients differ from the plain layout's only by the rounding of intermediate bf16 stores (f32: by the order of f32 sums).  All three operand types; f32
 * runs the two-pass backward kernels and ignores rows_needed. */
int lpi_txt_embed_fwd_shared(int x_dtype, int B, int L, const int32_t* row_start, int shared_rows /* = 1 + P */, int P, int d, const int64_t* ids,
                             const float* tok_emb, const float* pos, const float* ctx /* [P, d], broadcast */, void* x0, float* out_mean,
                             float* out_rstd, void* stream);
int lpi_attn_fwd_shared(int dtype, int B, int L, const int32_t* row_start, int shared_rows, int H, const void* qkv, int ldqkv, void* ctx, int ldctx,
                        float* lse, void* stream);
/* rows_needed counts POSITIONS (>= shared_rows); shared_dkv: f32 scratch [B, shared_rows, 2 H 64].  Runs the fused backward, then
 * lpi_shared_kv_reduce(accumulate = 1). */
int lpi_attn_bwd_shared(int dtype, int B, int L, const int32_t* row_start, int shared_rows, int rows_needed, int H, const void* qkv, int ldqkv,
                        const void* ctx, int ldctx, const void* dctx, int lddctx, const float* lse, float* delta, void* dqkv, int lddqkv,
                        float* shared_dkv, void* stream);
/* dqkv[key][H 64 .. 3 H 64) (+)= sum_b partial[b][key][0 .. 2 H 64) for key < shared_rows (the K and V columns of the shared rows). */
int lpi_shared_kv_reduce(int dtype, int B, int shared_rows, int H, const float* partial, void* dqkv, int lddqkv, int accumulate, void* stream);
int lpi_layernorm_bwd_rows_varlen(int dy_dtype, int cast_dtype, int x_dtype, int B, int L, const int32_t* row_start, int row0, int P, int d,
                                  const void* dy, int lddy, const void* x, int ldx, const float* gamma, const float* mean, const float* rstd,
                                  float* dx, int lddx, void* dx_cast, int ldcast, int accumulate, void* stream);
int lpi_gather_batch_rows_varlen(int dtype, int B, int L, const int32_t* row_start, int row0, int P, int cols, const void* src, int ld_src,
                                 void* dst, int ld_dst, void* stream);
int lpi_rows_sum_over_batch_varlen(int dtype, int B, int L, const int32_t* row_start, int row0, int P, int d, const void* dx, float* out,
                                   int accumulate, void* stream);
int lpi_prompt_add_varlen(int x_dtype, int B, int L, const int32_t* row_start, int P, int d, void* x, const float* prompt_l, long prompt_bstride,
                          float* out_mean, float* out_rstd, void* stream);
/* ids stays the padded [B, L] matrix (clip.tokenize's output); tokens l >= L_b of sample b are not embedded */
int lpi_txt_embed_fwd_varlen(int x_dtype, int B, int L, const int32_t* row_start, int P, int d, const int64_t* ids, const float* tok_emb,
                             const float* pos, const float* ctx, long ctx_bstride, void* x0, float* out_mean, float* out_rstd, void* stream);

/* ---- a1: DecomposedPrompt                          replaces: models/prompts/prompts.py:38-57 -----------
 * out[l,p,d] = scale/r * sum_r d1[l,r]*d2[p,r]*d3[d,r].  bwd: the three factor gradients from dout; scratch: Lyr*P*r floats. */
int lpi_prompt_cp_fwd(int Lyr, int P, int D, int r, const float* d1, const float* d2, const float* d3,
                      float scale, float* out, void* stream);
int lpi_prompt_cp_bwd(int Lyr, int P, int D, int r, const float* d1, const float* d2, const float* d3,
                      float scale, const float* dout, float* g1, float* g2, float* g3, int accumulate_g1,
                      float* scratch, void* stream);
/* Both prompt stacks of a DecomposedPrompt (visual and textual share dim_1_share, prompts.py:38-57) per call (round 4): the forward in ONE launch,
 * the backward in TWO (lpi_prompt_cp_bwd for the visual stack with g1 overwritten, then for the textual one with g1 accumulated: six launches).
 * The same arithmetic per value.  scratch: 2 * Lyr * P * r floats. */
int lpi_prompt_cp_fwd2(int Lyr, int P, int Dv, int Dt, int r, const float* d1, const float* d2v, const float* d2t, const float* d3v, const float* d3t,
                       float scale, float* outv, float* outt, void* stream);
int lpi_prompt_cp_bwd2(int Lyr, int P, int Dv, int Dt, int r, const float* d1, const float* d2v, const float* d2t, const float* d3v, const float* d3t,
                       float scale, const float* doutv, const float* doutt, float* g1, float* g2v, float* g2t, float* g3v, float* g3t, float* scratch,
                       void* stream);

/* ---- a3: vision front end                          replaces: models/clip/model.py:227-251 --------------
 * patchify: image [B,3,R,R] f32 -> cols [B*G*G (padded rows untouched), Kp] `dtype`, Kp >= 3*ps*ps zero padded.
 * assemble + ln_pre: x0[b] = LN([cls+pos0 ; prompts[b,0] (no pos) ; patch_emb[b]+pos1..]) -> x0 `x_dtype` [B*L,d];
 * prompt0: f32, element (b,p,:) at prompt0 + b*prompt_bstride + p*d (bstride 0 = broadcast, slinet.py:119).
 * bwd (dx0 is `dtype`: f32, or the bf16 gradient stream): applies LN' to rows 1..P of dx0 IN PLACE (dx0 is dead afterwards; the other rows' input gradients are
 *      not needed because the backbone is frozen), then dprompt[p,:] = sum_b dx0[b,1+p,:] (f32 [P,d]; the batch
 *      sum is the gradient of the training-time stride-0 broadcast, slinet.py:119).
 * out_mean / out_rstd (here, in lpi_txt_embed_fwd and in lpi_prompt_add; both or neither, NULL = not wanted): the LayerNorm statistics of every row
 *      these kernels WRITE, taken from the row as stored (a wave holds it) and written at the row's index in the stream — the statistics the NEXT
 *      LayerNorm needs (model.py:172: ln_1 of the block that reads the stream) without a pass over it; lpi_prompt_add overwrites the entries of the
 *      rows it rewrites, which a GEMM epilogue (LPI_EPI_RES_ROWSTATS) had filled from their old contents. */
int lpi_patchify(int dtype, int B, int R, int ps, const float* image, void* cols, int ldcols, void* stream);
/* The same im2col from UINT8 pixels [B,3,R,R] (what the decoder produces: PIL -> HWC bytes -> CHW) with the loader's ToTensor + Normalize
 * (utils/data.py:201-204: x / 255, (x - mean) / std) folded in through `lut` (f32 [3][256], DEVICE: lut[c][v] = the f32 value the host pipeline gives byte v
 * in channel c — filled by the caller with those very operations, so the columns equal lpi_patchify's on the normalised f32 image bit for bit).  A quarter
 * of the host-to-device bytes of the f32 batch (38.5 MB instead of 154 MB per 256 images).  Every geometry with R % ps == 0 (since 626; before, only ps and R multiples of 4): with ps and R multiples of 4 a kernel that reads four
 * pixels as one dword runs, and `image` must be 4-byte aligned (LPI_EINVAL otherwise, as before); every other geometry (ps = 14, 7, 6, ...) runs a kernel of
 * byte loads, which takes any image pointer.  Same columns, same zero padding of columns 3*ps*ps .. Kp, in f32, bf16 and f16. */
int lpi_patchify_u8(int dtype, int B, int R, int ps, const uint8_t* image, const float* lut, void* cols, int ldcols, void* stream);
int lpi_vis_assemble_fwd(int x_dtype, int B, int G2, int P, int d, const float* patch_emb, int ldpe, const float* cls,
                         const float* pos, const float* prompt0, long prompt_bstride,
                         const float* gamma, const float* beta, void* x0, float* mean, float* rstd, float* out_mean, float* out_rstd, void* stream);
int lpi_vis_assemble_bwd(int dtype, int B, int G2, int P, int d, void* dx0, const float* prompt0, long prompt_bstride,
                         const float* gamma, const float* mean, const float* rstd, float* dprompt, void* stream);
/* The position table at another patch grid (since 626; lpi_amd/csrc/posembed.hip): what a ViT library does when a checkpoint runs at a resolution other than
 * the one it was trained at.  src [1 + g_in*g_in, d] f32 (row 0 the class row, then the grid row-major; row stride lds), dst [1 + g_out*g_out, d] (stride ldd).
 * Row 0 is copied; the grid is resampled as torch.nn.functional.interpolate(x.reshape(1,g,g,d).permute(0,3,1,2), size=(g',g'), mode, align_corners=False,
 * antialias) does (OpenCLIP and timm use bicubic with antialias): separably, with float64 weights and sums and one rounding to f32.  g_out == g_in is a
 * bitwise copy in every mode, as in torch.  One launch; meant to be called once per engine.
 * 1 <= g_in, g_out <= 64; d a positive multiple of 4; lds, ldd >= d and multiples of 4; src, dst 16-byte aligned and not overlapping; filter one of the two
 * below, antialias 0 or 1: LPI_EINVAL before any launch otherwise.  Columns d .. ldd of dst are not written. */
#define LPI_POS_BICUBIC 0
#define LPI_POS_BILINEAR 1
int lpi_pos_embed_resample(int g_in, int g_out, int d, const float* src, long lds, float* dst, long ldd, int filter, int antialias, void* stream);

/* ---- a6/a7: text front end          replaces: models/clip/prompt_learner.py:52-53,128-163 --------------
 * x0[b,l] = (l in 1..P ? ctx[b,l-1] : tok_emb[ids[b,l]]) + pos[l]      (CLASS_TOKEN_POSITION == "end")
 * bwd: dctx[p,:] (+)= sum_b dx0[b,1+p,:] */
int lpi_txt_embed_fwd(int x_dtype, int B, int L, int P, int d, const int64_t* ids, const float* tok_emb, const float* pos,
                      const float* ctx, long ctx_bstride, void* x0, float* out_mean, float* out_rstd, void* stream);   /* x0 is `x_dtype` */
int lpi_rows_sum_over_batch(int dtype, int B, int L, int row0, int P, int d, const void* dx, float* out, int accumulate,
                            void* stream);   /* dx is `dtype` */

/* ---- F1: deep prompts                               replaces: models/clip/model.py:189-193 -------------
 * x[b, 1..P, :] += prompt_l[b?, p, :]   (in place on the `x_dtype` residual stream; prompt_l f32) */
int lpi_prompt_add(int x_dtype, int B, int L, int P, int d, void* x, const float* prompt_l, long prompt_bstride, float* out_mean, float* out_rstd,
                   void* stream);

/* ---- a3/a7/a2: pooled head     replaces: model.py:255-257, prompt_learner.py:57-61, slinet.py:122,133 --
 * pool_ln: y[b,:] = LN(x[b*L + idx[b], :]) (x `x_dtype`; idx NULL -> row 0 = CLS; else EOT position) -> y `dtype` [B,d]
 * pool_ln_bwd: dx (f32 [B*L,d], pre-zeroed) row idx[b] = LN'(dy[b]);
 * l2norm fwd/bwd on f32 [B,E]:  y = x/||x||. */
int lpi_pool_ln_fwd(int dtype, int x_dtype, int B, int L, int d, const void* x, const int32_t* idx, const float* gamma,
                    const float* beta, void* y, int ldy, float* mean, float* rstd, void* stream);
int lpi_pool_ln_bwd(int cast_dtype, int B, int L, int d, const float* dy, int lddy, const float* x,
                    const int32_t* idx, const float* gamma, const float* mean, const float* rstd,
                    float* dx, void* dx_cast, void* stream);
/* pooled-row gather (src `x_dtype` -> f32) / scatter (f32): dst[b] = src[b*L + idx[b]]  /  dst[b*L + idx[b]] = src[b] (+ `cast_dtype` copy; the other
 * rows of dst are the caller's, pre-zeroed).  Used to run the LAST block's MLP on the B pooled rows only: the heads read nothing
 * else of its output (model.py:255, prompt_learner.py:61), so this is exact dead-row elimination. */
int lpi_gather_rows(int x_dtype, int B, int L, int d, const void* src, const int32_t* idx, float* dst, void* stream);
int lpi_scatter_rows(int cast_dtype, int B, int L, int d, const float* src, const int32_t* idx, float* dst, void* dst_cast,
                     void* stream);
/* dst[b*L + idx[b], :] += src[b, :]  (`dtype` both; idx NULL: token 0) — adds the pooled rows' dQ contribution to d(LN1 output). */
int lpi_scatter_add_rows(int dtype, int B, int L, int d, const void* src, int ld_src, const int32_t* idx, void* dst, int ld_dst,
                         void* stream);
int lpi_l2norm_fwd(int B, int E, const float* x, int ldx, float* y, int ldy, float* inv_norm, void* stream);
int lpi_l2norm_bwd(int B, int E, const float* y, int ldy, const float* dy, int lddy, const float* inv_norm,
                   float* dx, int lddx, void* stream);
int lpi_eot_index(int B, int L, const int64_t* ids, int32_t* idx, void* stream);   /* ids.argmax(-1), prompt_learner.py:61 */

/* ---- several small row kernels of ONE dependency level in one launch (round 4) ------------------------------------------------------
 * The tail of a training step — the pooled rows of the last block, the heads, the L2 norms (model.py:255-257, prompt_learner.py:57-61,
 * slinet.py:122,133), the prompt rows (model.py:189-193, 240-248) — is a chain of few-microsecond launches on B or B*P rows, one per tower
 * and op.  lpi_row_jobs issues up to LPI_ROW_JOBS_MAX INDEPENDENT ones (the two towers' launch of the same op; independent ops of one tower) as
 * one launch: every job runs the body of its single-op kernel, so the results are bit for bit those of the entry point named below, and every
 * job is checked by that entry point's own argument predicate (csrc/rowops.hip: pool_ln_fwd_ok, l2norm_bwd_ok, scatter_add_ok, ... — one rule per op,
 * called from both; what a job form adds to it, such as out2, is written out in row_job_blocks).
 * Fields a job does not use are ignored.  dt_*: LPI_F32 / LPI_BF16 / LPI_F16.
 *   POOL_LN_FWD          lpi_pool_ln_fwd(dt_b, dt_a, B, L, d, a, idx, gamma, beta, out, ld_c, mean, rstd); out2 (optional) = the gathered row itself
 *                        as f32 [B, d] (lpi_gather_rows(dt_a, B, L, d, a, idx, out2))
 *   L2NORM_FWD           lpi_l2norm_fwd(B, d, a, ld_a, out, ld_c, mean [inv_norm])
 *   L2NORM_BWD           lpi_l2norm_bwd(B, d, a [y], ld_a, b [dy], ld_b, mean_in [inv_norm], out, ld_c); out2 (optional, dt_b = BF16) = the bf16
 *                        copy of out, same row stride (lpi_cast)
 *   POOL_LN_BWD          lpi_pool_ln_bwd(dt_b, B, L, d, a [dy], ld_a, b [x], idx, gamma, mean_in, rstd_in, out, out2 [cast copy or NULL])
 *   LN_BWD               lpi_layernorm_bwd(dt_a, dt_b, LPI_F32, B, d, a [dy], ld_a, b [x f32], ld_b, gamma, mean_in, rstd_in, out [dx or NULL], ld_c,
 *                        out2 [cast], ld_c, flag [accumulate])   with (dt_a, dt_b) = (BF16, BF16) or (F32, F32)
 *   SCATTER_ADD          lpi_scatter_add_rows(dt_a, B, L, d, a, ld_a, idx, out, ld_c)
 *   GATHER_BATCH_ROWS    lpi_gather_batch_rows_varlen with d = 16-byte chunks per row and ld_a / ld_c in 16-byte units: (B, L, row_start, row0, P, a, out)
 *   PROMPT_ADD           lpi_prompt_add_varlen(dt_a, B, L, row_start, P, d, out [x, in place], a [prompt_l], bstride, mean, rstd)
 *   LN_BWD_ROWS_H16      lpi_layernorm_bwd_rows_varlen(BF16, BF16, F16, B, L, row_start, row0, P, d, a [dy compact], ld_a, b [x], ld_b, gamma, mean_in,
 *                        rstd_in, NULL, 0, out2 [bf16 gradient stream], ld_c, flag [accumulate])   (the 16-byte half-wave kernel's alignment rules)
 *   VIS_PROMPT_ROWS_BWD  the LayerNorm part of lpi_vis_assemble_bwd: LN' on rows 1..P of out (dt_a, in place) with the rows of a (prompt0, bstride)   */
enum { LPI_ROWOP_POOL_LN_FWD = 1, LPI_ROWOP_L2NORM_FWD = 2, LPI_ROWOP_L2NORM_BWD = 3, LPI_ROWOP_POOL_LN_BWD = 4, LPI_ROWOP_LN_BWD = 5,
       LPI_ROWOP_SCATTER_ADD = 6, LPI_ROWOP_GATHER_BATCH_ROWS = 7, LPI_ROWOP_PROMPT_ADD = 8, LPI_ROWOP_LN_BWD_ROWS_H16 = 9,
       LPI_ROWOP_VIS_PROMPT_ROWS_BWD = 10 };
#define LPI_ROW_JOBS_MAX 4
typedef struct lpi_row_job {
    int op;
    int B, L, d;
    int P, row0;
    int dt_a, dt_b;
    int ld_a, ld_b, ld_c;
    int flag;
    long bstride;
    const void* a; const void* b;
    const int32_t* idx; const int32_t* row_start;
    const float* gamma; const float* beta; const float* mean_in; const float* rstd_in;
    void* out; void* out2;
    float* mean; float* rstd;
} lpi_row_job;
int lpi_row_jobs(int n, const lpi_row_job* jobs, void* stream);      /* jobs: HOST array, n <= LPI_ROW_JOBS_MAX */
typedef struct lpi_rows_sum_desc {
    int B, L, row0, P, d, accumulate;
    const int32_t* row_start;
    const void* dx; float* out;
} lpi_rows_sum_desc;
int lpi_rows_sum_over_batch_pair(int dtype, const lpi_rows_sum_desc* d /* [2] */, void* stream);

/* Leading dimensions and argument checks of the loss / prompt / k-means / ranking / interaction family (loss.hip, interact.hip: the sections a8, a9, a10, a11, a1,
 * "misc" ranking and f4 of this header; tests/test_loss_strides_gpu.py runs every entry point on offset, strided views with poisoned pads).  Every kernel of the
 * family moves ONE f32 (or int32) per lane: no pointer or leading dimension has an alignment rule beyond the element's own 4 bytes, odd leading dimensions are
 * legal.  All checks are made on the host BEFORE the first launch (since 619; up to 618 lpi_clip_loss_fwd_bwd looked at lddl after three launches): a refused call
 * (LPI_EINVAL) has launched nothing and written nothing.
 *   every leading dimension >= the width it strides: ld, lddl, ldg >= n (lddl only with dlogits, ldg only with g / gt); ldf, ldx >= E; the scores' ld >= n_cols;
 *     ldv, ldov, ldgv, lddv >= Dv and ldt, ldot, ldgt, lddt >= Dt (ten independent values: no two need be equal);
 *   every count > 0; r0 >= 0, nloc > 0, r0 + nloc <= n (with g / gt); label0 >= 0, label0 + rows <= n; row < T <= 32; 1 <= k <= n_cols (lpi_topk: ANY such k, a pass
 *     over the row per pick; the callers use k <= 16); r <= 16 (prompt CP) and Lyr P r, D r, 2 Lyr P within int (the CP kernels index with int; since 619);
 *     a one-thread-per-element grid (the CP forwards: Lyr P D, both widths summed for _fwd2; lpi_sgd_step: n; lpi_copy_rows: rows cols) within 2^31 - 1 workgroups of 256 (since 619);
 *     R <= 8, Dv, Dt <= 1024, 0 <= layer < Lyr (interaction; since 619 lpi_interact_workspace_floats refuses exactly what lpi_interact_fwd refuses);
 *     temp > 0; the alignment loss's LDS: 4 Lyr P + 2 Lyr^2 + 2 Lyr floats (lpi_align_loss_fwd_bwd; 2 Lyr P + ... for _fwd_bwd2) <= 64 KB;
 *   required pointers non-NULL.  Optional (NULL = not wanted): dlogits, g / gt (both or neither), lpi_sum_scaled's b, dist, mindist, center, val, dvis / dtxt (both
 *     or neither: since 619 lpi_align_loss_fwd_bwd refuses one without the other, as _fwd_bwd2 always did), dx_row (NULL, or row < 0: forward only — both spellings
 *     are accepted, a row >= 0 with dx_row = NULL computes the loss alone);
 *   lpi_ce_rows_fwd_bwd's dlogits may BE logits (the gradient overwrites the block, row by row by the wave that read it): then lddl must equal ld (since 619).
 * What the host CANNOT check, because the arrays are device memory — the caller's contract: gt[i, t] < n_cols (or < 0 = padding), cand[c] in [0, n),
 * labels[i] in [0, k) for lpi_kmeans_update (lpi_kmeans_assign accepts any stored value: it only compares), target entries 0 / 1 with at least one of each per row
 * (else the loss is NaN, as the reference's is); scratch / workspace sizes as stated at each call; dxv / dxt, g / gt, the output rows must not overlap their inputs. */
/* ---- a8: symmetric contrastive loss   replaces: loss/loss.py:75-87 (ClipLoss.forward), slinet.py:139-141
 * logits f32 [n_rows, n_cols] (ld), rows r0..r0+n_local-1 are this rank's pairs; square global matrix
 * (n_rows == n_cols == W*B).  loss[0] = (CE(logits,arange)+CE(logits^T,arange))/2 over ALL rows/cols;
 * dlogits (f32, same shape) = upstream * dloss/dlogits. */
int lpi_clip_loss_fwd_bwd(int n, const float* logits, int ld, float upstream, float* loss, float* dlogits,
                          int lddl, float* row_lse, float* col_lse, void* stream);
/* Data-parallel backward of the same loss (`local_loss=False` semantics of gather_features, sprompt.py:75-80): only the nloc rows
 * r0..r0+nloc of the global matrix belong to this rank.  g[i,j] = dL/dlogits[r0+i, j], gt[i,j] = dL/dlogits[j, r0+i] (both
 * [nloc, n] row-major, row stride ldg), from the row/column log-sum-exp vectors lpi_clip_loss_fwd_bwd left behind. */
int lpi_clip_loss_local_grad(int n, const float* logits, int ld, const float* row_lse, const float* col_lse, float upstream,
                             int r0, int nloc, float* g, float* gt, int ldg, void* stream);
/* lpi_clip_loss_fwd_bwd (dlogits = NULL) + lpi_clip_loss_local_grad as TWO launches instead of four (round 4): the two log-sum-exp vectors in one
 * launch, the loss value in the first workgroup of the local-gradient kernel.  g / gt NULL: the loss and the lse vectors only.  The same arithmetic
 * per value: bit for bit the four-launch results (loss/loss.py:75-87, sprompt.py:75-80). */
int lpi_clip_loss_local(int n, const float* logits, int ld, float upstream, int r0, int nloc, float* loss, float* row_lse, float* col_lse,
                        float* g, float* gt, int ldg, void* stream);
/* `local_loss=True` form of the same loss (sprompt.py:278-283 with loss/loss.py:62-73): row-wise cross-entropy of a [rows, n] block of
 * logits (this rank's images against ALL texts, or its texts against all images) whose row i has label label0 + i (= rank * B + i).
 * loss_rows[i] = logsumexp(logits[i, :]) - logits[i, label0 + i]; dlogits (optional; may be `logits` itself with lddl == ld: in place) = upstream * (softmax - onehot).
 * lpi_sum_scaled: out[0] = scale * sum(a[i] + b[i]) (b may be NULL), fixed order — the mean of the two row-loss vectors. */
int lpi_ce_rows_fwd_bwd(int rows, int n, const float* logits, int ld, int label0, float upstream, float* loss_rows, float* dlogits,
                        int lddl, void* stream);
int lpi_sum_scaled(int n, const float* a, const float* b, float scale, float* out, void* stream);
/* dst[r, 0:cols] = src[r, 0:cols], f32, row strides lds / ldd elements (packing / zero-padded operands; no framework copy kernels) */
int lpi_zero(void* ptr, long bytes, void* stream);   /* hipMemsetAsync(ptr, 0, bytes) on `stream` */
int lpi_copy_rows(int rows, int cols, const float* src, long lds, float* dst, long ldd, void* stream);
/* a11 task-id selection, replaces get_visual_task_id / get_textual_task_id (methods/sprompt.py:336-368):
 * sel[i] = argmin_t min_c sum_e |feat[i,e] - keys[t,c,e]|, keys [T, C, E] f32 (the KMeans centres of every task seen so far);
 * dist (optional) [n, T] receives the per-task minima. */
int lpi_l1_task_id(int n, int E, int T, int C, const float* feat, int ldf, const float* keys, int32_t* sel, float* dist,
                   void* stream);
/* ---- a10/f3: the task keys — KMeans(n_clusters=5, random_state=0).fit(features)   replaces: methods/sprompt.py:370-397 (clustering), round 4 -----------
 * The device parts of scikit-learn's fit (k-means++ seeding + Lloyd iterations, sklearn/cluster/_kmeans.py), driven by lpi_amd/kmeans.py, which keeps the
 * random draws (numpy RandomState) and the convergence logic on the host on vectors of n floats at most: the features X [n, E] f32 stay on the device.
 *   lpi_kmeans_sqdist   out[c, i] = |x_i - x_cand[c]|^2, c < nc (the distances of every point to candidate centres, which are points)
 *   lpi_kmeans_assign   labels[i] = argmin_c |x_i - centers[c]|^2 (first minimum; labels in / out), *changed = 1 if any label changed (never cleared here);
 *                       mindist (NULL = not wanted) [n]: that minimum — what scikit-learn's empty-cluster relocation ranks the points by
 *   lpi_kmeans_update   new_centers[c] = mean of the points labelled c (0 for an empty cluster), counts[c] = their number; fixed summation order
 *   lpi_kmeans_colstats colsum[e] = sum_i (x[i, e] - center[e]), colsq[e] = sum_i (x[i, e] - center[e])^2, center NULL = 0 (the tolerance mean_e var_i x[i, e] * tol:
 *                       column means from a first call, centred squares from a second — two passes, no cancellation) */
int lpi_kmeans_sqdist(int n, int E, int nc, const float* X, int ldx, const int32_t* cand, float* out, void* stream);
int lpi_kmeans_assign(int n, int E, int k, const float* X, int ldx, const float* centers, int32_t* labels, int32_t* changed, float* mindist, void* stream);
int lpi_kmeans_update(int n, int E, int k, const float* X, int ldx, const int32_t* labels, float* new_centers, float* counts, void* stream);
int lpi_kmeans_colstats(int n, int E, const float* X, int ldx, const float* center, float* colsum, float* colsq, void* stream);

/* a10 optimiser step, replaces optim.SGD(momentum, weight_decay).step() (methods/sprompt.py:253,311) on one flat f32 vector:
 * d = grad + wd*p; buf = first ? d : momentum*buf + d; p -= lr*buf. */
int lpi_sgd_step(long n, float* param, const float* grad, float* momentum_buf, float lr, float momentum, float weight_decay,
                 int first, void* stream);

/* ---- a8: alignment loss                                   replaces: models/slinet.py:143-158 ------------
 * v = mean_d(vis)/temp, t = mean_d(txt)/temp ([Lyr,P]); S = v t^T [Lyr,Lyr]; loss[0] = weight * ClipLoss(S);
 * dvis [Lyr,P,Dv], dtxt [Lyr,P,Dt] = dense gradients of loss[0] (both NULL: forward only). */
int lpi_align_loss_fwd_bwd(int Lyr, int P, int Dv, int Dt, const float* vis, const float* txt, float temp,
                           float weight, float* loss, float* dvis, float* dtxt, void* stream);
/* The same loss and gradients in TWO launches instead of three (round 4): the row means go to `scratch` (2 * Lyr * P floats), and every workgroup of the
 * second launch recomputes the Lyr x Lyr core from them and writes its own gradient row (workgroup 0 the loss).  Value for value lpi_align_loss_fwd_bwd. */
int lpi_align_loss_fwd_bwd2(int Lyr, int P, int Dv, int Dt, const float* vis, const float* txt, float temp, float weight, float* loss, float* dvis,
                            float* dtxt, float* scratch, void* stream);

/* ---- a9: task loss (nt_bxent over the tasks' flattened prompts)   replaces: loss/loss.py:6-33, models/slinet.py:167-183 ----
 * X f32 [T, D] (row t = prompts of task t, flattened), target int32 [T,T] (task_sim > 0.4), T <= 32.  loss[0] = weight * nt_bxent(X);
 * dx_row [D] = d loss / d X[row,:] (only the current task's prompts train; NULL or row < 0: forward only); accumulate != 0: ADDED to what dx_row
 * holds (the fused training step adds the task term onto the alignment gradient already sitting in the towers' prompt-gradient buffers).
 * scratch: 2*T*T floats. */
int lpi_nt_bxent_fwd_bwd(int T, int D, int row, const float* X, const int32_t* target, float temp, float weight,
                         float* loss, float* dx_row, int accumulate, float* scratch, void* stream);

/* ---- misc ---------------------------------------------------------------------------------------------- */
int lpi_cast(int src_dtype, int dst_dtype, long n, const void* src, void* dst, void* stream);
int lpi_transpose(int dtype, int rows, int cols, const void* src, int lds, void* dst, int ldd, void* stream);
/* two f32 transposes in one launch (the two feature matrices of the contrastive loss's gradient GEMMs) */
int lpi_transpose2(int dtype, int rows0, int cols0, const void* src0, int lds0, void* dst0, int ldd0,
                   int rows1, int cols1, const void* src1, int lds1, void* dst1, int ldd1, void* stream);
/* per-row descending rank of the best ground-truth column (itm_eval, methods/sprompt.py:558-599):
 * rank[i] = #{j : s[i,j] > s[i,gt] or (s[i,j] == s[i,gt] and j > gt)} minimised over gt in gt_list row i.
 * (np.argsort(score)[::-1] places later indices first among ties.) */
int lpi_retrieval_rank(int n_rows, int n_cols, const float* scores, int ld, const int32_t* gt, int gt_per_row,
                       int32_t* rank, void* stream);
/* idx [n_rows, k] (val [n_rows, k], NULL = not wanted): the k best columns of every row in that order (value descending, later index first among equal values,
 * -inf included); any 1 <= k <= n_cols. */
int lpi_topk(int n_rows, int n_cols, int k, const float* scores, int ld, int32_t* idx, float* val, void* stream);

/* ---- streamed search (search.hip, since 614): the two calls above without the score matrix.  s[i,j] = Q[i,:] . G[j,:] is computed tile by tile on the
 * matrix cores (exact f32 products, f32 accumulation, one fixed order over E per score) and consumed from the accumulators: memory is O(nq k), not
 * O(nq ng).  A score's bits depend on its two rows only: not on where the rows sit, on ng, or on how a gallery is cut into calls.
 * Q f32 [nq, E] (ldq), G f32 [ng, E] (ldg): nq, ng any positive number (edges are masked, the caller pads nothing), E a multiple of 16 and <= 1024,
 * ldq / ldg >= E and multiples of 4 (16-byte rows, as the GEMM family), Q and G 16-byte aligned, finite values.  Nothing outside the n x E elements
 * of an operand is read, nothing outside idx / val / rank / ws is written.  ws: lpi_search_workspace(nq, ng, k) bytes (k = 0: the rank form), a host
 * function that never shrinks when an argument grows; its contents need not survive between calls.  Anything outside the envelope, or a workspace
 * that is too small, is LPI_EINVAL before any launch.
 * lpi_search_topk: 1 <= k <= 16 (lpi_topk's range); idx / val [nq, k] in lpi_topk's order (value descending, then index descending); col_base >= 0 is
 *   added to the indices.  accumulate != 0: idx / val already hold such a list (entries with idx < 0 are empty) and it takes part: a gallery that is
 *   sharded or larger than the device is searched chunk by chunk, and the result is that of one call, bit for bit.  k <= ng unless accumulate (what the
 *   held list brings is the caller's statement; a list shorter than k ends with idx = -1, val = -inf).  val must not be NULL.  Two launches.
 * lpi_search_rank: rank [nq] as lpi_retrieval_rank over the gt list [nq, gt_per_row] (entries < 0 or >= ng are ignored; a row with none gets
 *   0x7fffffff as there): #{j != g* : s[i,j] > s[i,g*] or (s[i,j] == s[i,g*] and j > g*)} for g* = the row's ground-truth column that is largest in
 *   the order (score, then index) - equal to the minimum over the list because the count is monotone in that order.  The threshold score comes from a
 *   first launch of the same tile code over the gathered ground-truth rows, so duplicate gallery rows tie exactly and fall by index.  Two launches.
 *   After the call ws holds the thresholds: s[i,g*] f32 [nq] (+inf: none), then g* int32 [nq] (-1: none). */
long lpi_search_workspace(int nq, int ng, int k_or_0);
int lpi_search_topk(int nq, int ng, int E, const float* Q, int ldq, const float* G, int ldg, int k, int col_base, int accumulate,
                    int32_t* idx, float* val, void* ws, long ws_bytes, void* stream);
int lpi_search_rank(int nq, int ng, int E, const float* Q, int ldq, const float* G, int ldg, const int32_t* gt, int gt_per_row,
                    int32_t* rank, void* ws, long ws_bytes, void* stream);
/* The same two calls with the operand type as first argument (search16.hip, since 615).  dt = LPI_F32 forwards to the calls above: their envelope,
 * their bits.  dt = LPI_BF16 | LPI_F16: Q and G are 2-byte elements of that one type, read in place (no f32 copy is made).  The 2-byte envelope: E a
 * multiple of 32 and <= 1024, ldq / ldg >= E in elements and multiples of 8 (16-byte rows), Q and G 16-byte aligned, finite values; everything else
 * (nq, ng, k, col_base, accumulate, gt, idx, val, rank, ws and lpi_search_workspace, which does not depend on the type) as above.  val and the
 * thresholds left in ws are f32.  A score is the f32 accumulation, in one fixed order over E, of the exact products of the 2-byte values
 * (v_mfma_f32_16x16x32_bf16 / _f16), so every property above holds: a score's bits depend on its two rows only, a chunked search equals one call bit
 * for bit, duplicate rows tie exactly and fall by index, the rank threshold carries the sweep's bits.  Any other dt, LPI_F32X3 included, is
 * LPI_EINVAL before any launch. */
int lpi_search_topk_t(int dt, int nq, int ng, int E, const void* Q, int ldq, const void* G, int ldg, int k, int col_base, int accumulate,
                      int32_t* idx, float* val, void* ws, long ws_bytes, void* stream);
int lpi_search_rank_t(int dt, int nq, int ng, int E, const void* Q, int ldq, const void* G, int ldg, const int32_t* gt, int gt_per_row,
                      int32_t* rank, void* ws, long ws_bytes, void* stream);
/* The same two calls on MX-FP8 operands read in place (search_mx8.hip, since 616): Q / G are e4m3 bytes [n, ld] and q_scales / g_scales their E8M0
 * scale bytes [n, lds], one per 32 consecutive elements of a row: the project's MX format, THE FORMAT below (what lpi_mx8_quantize writes).  1.03 bytes
 * per gallery element.  s[i,j] is the f32 result of the chain of E / 128 block-scaled instructions (v_mfma_scale_f32_16x16x128_f8f6f4) over the two
 * rows, in one fixed order: its bits depend on its two rows (elements and scales) only, so a chunked search equals one call bit for bit, duplicate rows
 * (elements and scales alike) tie exactly and fall by index, and the rank threshold carries the sweep's bits.  val holds the scores of the QUANTISED
 * rows.  The instruction aligns the 128 scaled products of a step before it adds them: a score is within 8.6e-5 |q| . |g| of the exact product of the
 * dequantised rows (tests/test_search_mx8_gpu.py has the measured figure), and exact on data whose partial sums are exact.
 * Envelope: nq, ng > 0; E a multiple of 128 and <= 1024 (one instruction covers 128 k-values: there is no tail); ldq / ldg >= E and multiples of 16,
 * Q and G 16-byte aligned; ldqs / ldgs >= E / 32 and multiples of 4, the scale bases 4-byte aligned; no NULL operand or scale pointer; k, col_base,
 * accumulate, gt, idx, val, rank, ws and lpi_search_workspace (which does not depend on the type) as for the f32 calls.  Anything else is LPI_EINVAL
 * before any launch.  Nothing outside the n x E element bytes and the n x E / 32 scale bytes is read.  NaN element bytes (0x7F, 0xFF) and the scale
 * byte 0xFF are out of contract, like non-finite inputs above.  lpi_search_topk_t / lpi_search_rank_t keep refusing dt = LPI_MX8. */
int lpi_search_topk_mx8(int nq, int ng, int E, const void* Q, int ldq, const void* q_scales, int ldqs, const void* G, int ldg, const void* g_scales,
                        int ldgs, int k, int col_base, int accumulate, int32_t* idx, float* val, void* ws, long ws_bytes, void* stream);
int lpi_search_rank_mx8(int nq, int ng, int E, const void* Q, int ldq, const void* q_scales, int ldqs, const void* G, int ldg, const void* g_scales,
                        int ldgs, const int32_t* gt, int gt_per_row, int32_t* rank, void* ws, long ws_bytes, void* stream);
/* Wide lists (search_wide.hip, since 620): lpi_search_topk / _t / _mx8 with 1 <= k <= LPI_SEARCH_KWIDE = 256, in ONE sweep of the gallery.  Argument
 * lists, envelope per operand type (E and its multiple, leading dimensions, alignment, col_base, accumulate and its held list, k <= ng unless
 * accumulate, finite values), order (value descending, then index descending; a short list ends with idx = -1, val = -inf) and refusals (LPI_EINVAL
 * before any launch; lpi_search_topk_wide_t forwards dt = LPI_F32 and refuses LPI_MX8, LPI_F32X3 and anything else) are the narrow calls'.  The sweep
 * is the narrow calls' tile code with another epilogue: every score has the narrow calls' bits, so for k <= 16 the lists are the narrow calls' bit for
 * bit, a chunked search equals one call bit for bit, and duplicate rows tie exactly and fall by index.  Two launches per call, whatever k, nq and ng:
 * the sweep, which appends the scores that beat a per-row threshold (the row's k-th best so far) to a candidate buffer and brings a buffer down to its
 * k best when the next tile could overflow it, and the merge of the gallery splits' lists (with the held list when accumulating) into idx / val.
 * ws: lpi_search_wide_workspace(nq, ng, k) bytes, a host function (LPI_EINVAL outside nq, ng > 0, 1 <= k <= 256) that never shrinks when an argument
 * grows and is constant in ng from 65 536 on: per (gallery split, query row) one candidate buffer of 256 (k <= 128) or 512 (value, index) pairs, the
 * values of all buffers first, then the indices; its contents need not survive between calls.  (2048, 1 048 576, 256): 264 MiB, the score matrix
 * 8 GiB.  The narrow calls and lpi_search_workspace keep their range, k <= 16. */
#define LPI_SEARCH_KWIDE 256
long lpi_search_wide_workspace(int nq, int ng, int k);
int lpi_search_topk_wide(int nq, int ng, int E, const float* Q, int ldq, const float* G, int ldg, int k, int col_base, int accumulate,
                         int32_t* idx, float* val, void* ws, long ws_bytes, void* stream);
int lpi_search_topk_wide_t(int dt, int nq, int ng, int E, const void* Q, int ldq, const void* G, int ldg, int k, int col_base, int accumulate,
                           int32_t* idx, float* val, void* ws, long ws_bytes, void* stream);
int lpi_search_topk_wide_mx8(int nq, int ng, int E, const void* Q, int ldq, const void* q_scales, int ldqs, const void* G, int ldg,
                             const void* g_scales, int ldgs, int k, int col_base, int accumulate, int32_t* idx, float* val, void* ws, long ws_bytes,
                             void* stream);
/* Second stage of a two-stage search (search_rerank.hip, since 621): exact scores of a short candidate list per query row.  For query row i the
 * candidates are cand[i * ldc + 0 .. kc - 1], gallery row indices: what a coarse lpi_search_topk* call (2-byte or MX-FP8 operands, k a little above the
 * k wanted) left in idx, or several such lists side by side.  An entry outside [0, ng), negative ones (the padding of a short list) included, is
 * padding and never used as an address; an index that occurs several times in a row counts once.  The distinct valid candidates are scored against
 * Q[i, :] and the k best go to idx / val [nq, k] (contiguous rows of k) in lpi_topk's order, value descending, then index descending; unfilled slots
 * are (-1, -inf) and come last.  val has exactly the bits lpi_search_topk / lpi_search_topk_t of the same operand type returns for that (query row,
 * gallery row): the same matrix instruction and the same accumulator chain over E, so a coarse list that contains the f32 top k, re-ranked on the f32
 * rows, IS lpi_search_topk's f32 result, comparable with ==.  Envelope: the narrow call's for the operand type (nq, ng > 0; E <= 1024 and a multiple
 * of 16 for f32, of 32 for 2-byte operands; leading dimensions >= E and multiples of 16 bytes, Q / G 16-byte aligned), 1 <= kc <= LPI_SEARCH_KWIDE,
 * 1 <= k <= kc, ldc >= kc, no NULL pointer; cand is read only (it must not overlap idx / val), nothing of cand beyond kc entries per row and no
 * gallery row that is not listed is read.  Anything else is LPI_EINVAL before any launch.  No workspace: memory is the two outputs.  One launch per
 * call, whatever nq, kc and k.  lpi_search_rerank_t: dt = LPI_BF16 | LPI_F16 (2-byte Q / G of that one type, read in place); LPI_F32 forwards to
 * lpi_search_rerank; LPI_MX8 (the second stage exists for the better operand), LPI_F32X3 and anything else is LPI_EINVAL. */
int lpi_search_rerank(int nq, int ng, int E, const float* Q, int ldq, const float* G, int ldg, const int32_t* cand, int ldc, int kc, int k,
                      int32_t* idx, float* val, void* stream);
int lpi_search_rerank_t(int dt, int nq, int ng, int E, const void* Q, int ldq, const void* G, int ldg, const int32_t* cand, int ldc, int kc, int k,
                        int32_t* idx, float* val, void* stream);
/* The top-k calls on MX-FP4 operands read in place (search_mx4.hip, search_wide.hip, mx4_rows.hip; since 622): a COARSE operand for a two-stage search,
 * half a byte per gallery element plus the scales (0.53 bytes), four times the bf16 matrix rate.  Its lists are candidate lists for lpi_search_rerank
 * (scores are off by a few 1e-2 on unit rows), so there is no rank form and no re-rank form: lpi_search_topk_t, lpi_search_topk_wide_t,
 * lpi_search_rank_t and lpi_search_rerank_t refuse dt = LPI_MX4 exactly as they refuse LPI_MX8.
 * THE MX-FP4 FORMAT.  Codes: uint8 [n, E / 2], OCP e2m1 nibbles, a sign bit (8) and a magnitude code 0 .. 7 = {0, 0.5, 1, 1.5, 2, 3, 4, 6}; element 2 j of
 * a row is the LOW nibble of byte j, element 2 j + 1 the high one, so a row's bytes are the matrix instruction's operand bytes in K order and the search
 * reads them in place.  (Measured on an MI355X, tools/probe/mx4_map_probe.hip: a lane of v_mfma_scale_f32_16x16x128_f8f6f4 holds 32 consecutive K elements
 * in 16 bytes and the scale of exactly those; the instruction pairs nibble positions of its two operands, and a product of two operands packed alike
 * is the same in either nibble order, so the order is this format's choice.)  Scales: uint8 [n, E / 32], E8M0 (value 2^(byte - 127)), one per 32
 * consecutive elements.  Scale rule: for a block maximum amax with biased f32 exponent Eb, byte = max(Eb - 2, 0): the OCP rule e = floor(log2 amax) - 2.
 * Element rule: y 2^(127 - byte) (exact) rounded to nearest even on the e2m1 grid and saturating at +-6: values in (6, 8) become 6.  A zero or subnormal
 * amax gives byte 0.  Non-finite inputs and the scale byte 0xFF are out of contract, as for MX-FP8.  tests/mx4_emulate.py restates the format on the CPU.
 * lpi_mx4_quantize: rows of x (`x_dtype`: LPI_F32 | LPI_BF16 | LPI_F16, [rows, ldx], ldx >= K in multiples of 4, x aligned to 4 elements) -> q (codes
 *   [rows, ldq bytes], ldq >= K / 2 and a multiple of 4, q 4-byte aligned) + scales ([rows, lds >= K / 32], one byte per store), one launch, bit for bit
 *   the emulator.  rows > 0, K a positive multiple of 32, no NULL pointer.  Anything else is LPI_EINVAL before any launch.
 * lpi_search_topk_mx4 (1 <= k <= 16) / lpi_search_topk_wide_mx4 (1 <= k <= LPI_SEARCH_KWIDE): lpi_search_topk_mx8 / lpi_search_topk_wide_mx8 on such
 *   operands.  s[i,j] is the f32 result of the chain of E / 128 block-scaled instructions over the two rows in one fixed order: its bits depend on its two
 *   rows (codes and scales) only, so a chunked search equals one call bit for bit, the narrow and the wide call give the same bits for the same pair, and
 *   the order is lpi_topk's.  val holds the scores of the QUANTISED rows: within 8.6e-5 |q| . |g| of the exact product of the dequantised rows
 *   (tests/test_search_mx4_gpu.py has the measured figure), exact where the partial sums are exact.  Envelope: nq, ng > 0; E (in ELEMENTS) a multiple of
 *   128 and <= 1024; ldq / ldg in BYTES, >= E / 2 and multiples of 16, Q and G 16-byte aligned; ldqs / ldgs >= E / 32 and multiples of 4, the scale bases
 *   4-byte aligned; no NULL pointer; k, col_base, accumulate, idx, val, ws and lpi_search_workspace / lpi_search_wide_workspace as for the f32 calls.
 *   Anything else is LPI_EINVAL before any launch.  Nothing outside the n x E / 2 code bytes and the n x E / 32 scale bytes is read.  Two launches. */
#define LPI_MX4 5
int lpi_mx4_quantize(int x_dtype, int rows, int K, const void* x, int ldx, void* q, int ldq, void* scales, int lds, void* stream);
int lpi_search_topk_mx4(int nq, int ng, int E, const void* Q, int ldq, const void* q_scales, int ldqs, const void* G, int ldg, const void* g_scales,
                        int ldgs, int k, int col_base, int accumulate, int32_t* idx, float* val, void* ws, long ws_bytes, void* stream);
int lpi_search_topk_wide_mx4(int nq, int ng, int E, const void* Q, int ldq, const void* q_scales, int ldqs, const void* G, int ldg,
                             const void* g_scales, int ldgs, int k, int col_base, int accumulate, int32_t* idx, float* val, void* ws, long ws_bytes,
                             void* stream);

/* ---- a6 (host side): CLIP byte-level BPE      replaces: models/clip/simple_tokenizer.py:62-132, clip.py:185-221 ------
 * HOST functions (no GPU work, no stream).  create: `merges_utf8` is the decompressed text of bpe_simple_vocab_16e6.txt(.gz) —
 * third-party data that is not shipped with this library; returns NULL on a malformed table.  encode: pattern split + byte mapping
 * + pair merging of ONE cleaned, lower-cased UTF-8 string (cleaning — ftfy / html.unescape / whitespace — stays with the caller);
 * writes at most max_ids ids and returns the full count.  tokenize = clip.tokenize: row t of out [n, context_length] int64 is
 * SOT, ids, EOT, zero padding; returns 0, or t+1 for the first text that does not fit when truncate == 0 (clip.py:218 raises). */
/* ---- f4 (optional): low-rank cross-modal interaction of the prompt rows, "InteractModule" ------------------------------------------
 * replaces: InteractModule.forward (grounding/maskrcnn_benchmark/modeling/bert/modeling_bert.py:616-651; parameters :558-590) and its backward.
 * xv [N, Dv], xt [N, Dt] f32: the visual / textual prompt rows of the batch ([bs, P, D] flattened).  Per direction the rank-r CP weights
 * d1 [Lyr, R], d2 [Din + 1, R] (last row = bias), d3 [Dout, R]:  new = x M[:Din] + M[Din],  M[i, j] = mean_r d1[layer, r] d2[i, r] d3[j, r];
 * out_v = LayerNorm_v((1 - mix) xv + mix new_v), out_t likewise (mix = 0.1, eps = 1e-5 in the reference).  Dv, Dt <= 1024, R <= 8.
 * stat: [4, N] f32 (mean / rstd of the two LayerNorms).  The backward recomputes the forward; dxv / dxt are overwritten; `grads` receives
 *   [v2t: dd3 [Dt R] | dd2 [(Dv + 1) R] | dd1 row `layer` [R] | dgamma_t [Dt] | dbeta_t [Dt]] [t2v: dd3 [Dv R] | dd2 [(Dt + 1) R] | dd1 row [R] | dgamma_v [Dv] | dbeta_v [Dv]];
 * workspace: lpi_interact_workspace_floats(N, Dv, Dt, R) floats (per-workgroup partial sums, added in a fixed order). */
int lpi_interact_workspace_floats(int N, int Dv, int Dt, int R);
int lpi_interact_fwd(int N, int Dv, int Dt, int R, int Lyr, int layer, const float* xv, int ldv, const float* xt, int ldt,
                     const float* d1_v2t, const float* d2_v2t, const float* d3_v2t, const float* d1_t2v, const float* d2_t2v,
                     const float* d3_t2v, const float* gamma_v, const float* beta_v, const float* gamma_t, const float* beta_t, float mix,
                     float eps, float* out_v, int ldov, float* out_t, int ldot, float* stat, void* stream);
int lpi_interact_bwd(int N, int Dv, int Dt, int R, int Lyr, int layer, const float* xv, int ldv, const float* xt, int ldt,
                     const float* d1_v2t, const float* d2_v2t, const float* d3_v2t, const float* d1_t2v, const float* d2_t2v,
                     const float* d3_t2v, const float* gamma_v, const float* beta_v, const float* gamma_t, const float* beta_t, float mix,
                     float eps, const float* g_out_v, int ldgv, const float* g_out_t, int ldgt, float* dxv, int lddv, float* dxt, int lddt,
                     float* grads, float* workspace, void* stream);

/* ---- host side: batch assembly for the input pipeline      replaces: the DataLoader's default_collate (torch.stack of the decoded images) + the pageable
 * `images.cuda()` copy of methods/sprompt.py:166-167, 301.  HOST pointers, no stream: dst[i * bytes_each ..] = srcs[i][0 .. bytes_each) for i < n on
 * `threads` host threads (dst: the pinned staging buffer the H2D DMA reads; 154 MB of f32 pixels per 256-pair step).  lpi_amd/pipeline.py. */
int lpi_host_gather(void* dst, const void* const* srcs, int n, long bytes_each, int threads);
/* The ragged form (images of different sizes, pixel_format='decoded'): dst = srcs[0][0 .. bytes[0]) ++ srcs[1][0 .. bytes[1]) ++ ... packed without gaps,
 * on `threads` host threads.  bytes[i] >= 0.  Returns 0 or LPI_EINVAL. */
int lpi_host_gather_v(void* dst, const void* const* srcs, const long* bytes, int n, int threads);

/* ---- decoded pixels on the GPU (imageops.hip)      replaces: the host's crop / Resize (bilinear) / CenterCrop / RandomHorizontalFlip of the training and
 * evaluation transforms (lpi_amd/retrieval/utils/data.py) and the HWC -> CHW copy of pixel_format='u8'.
 * One descriptor per image: LPI_RESAMPLE_DESC int64 values {src_offset, w, h, x0, y0, x1, y1, rw, rh, ox, oy, flip}: the image is the w x h x 3 (HWC,
 * RGB) uint8 block at byte src_offset of `src`; its output is crop((x0, y0, x1, y1)).resize((rw, rh), FILTER), the window [ox, ox+S) x [oy, oy+S) of
 * that, mirrored left-right if flip = 1.  FILTER is one per call, a Pillow Image.Resampling value: LPI_FILTER_BILINEAR (the reference's retrieval
 * loader; what the entry points without _f use), LPI_FILTER_BICUBIC (CLIP's own preprocessing) or LPI_FILTER_BOX.  Any other value (0 NEAREST does
 * not go through ImagingResample; 1 LANCZOS and 5 HAMMING take their taps from the host's sin / cos, which the device's need not match in the last
 * bit) is LPI_EINVAL, returned before any copy or launch.
 * EXACTNESS: out is Pillow 12's ImagingResample for 8-bit channels, byte for byte: per axis scale = in/out (in = the CROP's size: the filter clamps at
 * the crop's edges), filterscale = max(scale, 1), support = fs * filterscale with the filter's support fs (BOX 0.5, BILINEAR 1, BICUBIC 2), center =
 * (xx + 0.5) * scale, xmin = max((int)(center - support + 0.5), 0), xmax = min((int)(center + support + 0.5), in) - xmin, taps f((x + xmin - center
 * + 0.5) * (1 / filterscale)) summed in tap order and divided by their sum, in double without FMA contraction, f the filter's function in Pillow's
 * association order — BILINEAR 1 - |x| below 1; BICUBIC (a = -0.5) ((a + 2) |x| - (a + 3)) |x| |x| + 1 below 1, (((|x| - 5) |x| + 8) |x| - 4) a
 * below 2; BOX 1 for -0.5 < x <= 0.5; else 0 — converted to 22-bit fixed point as (int)(+-0.5 + k * 2^22); the horizontal pass is rounded to a
 * uint8 intermediate (clamp((2^21 + sum) >> 22, 0, 255), both clamps live with bicubic's negative taps), then the vertical pass on it the same way —
 * or vertical first, then horizontal, where Pillow's Image.resize takes that order, whatever the filter: crop height > 100 * crop width and rh <
 * crop height.
 * Limits: 1 <= B <= 65535, 1 <= S <= LPI_RESAMPLE_MAX_SIZE, 1 <= w, h, rw, rh <= LPI_RESAMPLE_MAX_SIDE; the box non-empty inside the image, the window
 * inside the resized image, flip 0 or 1: anything else is LPI_EINVAL, returned before any launch. */
#define LPI_RESAMPLE_DESC 12
#define LPI_RESAMPLE_MAX_SIZE 1024
#define LPI_RESAMPLE_MAX_SIDE (1L << 24)
#define LPI_FILTER_BILINEAR 2
#define LPI_FILTER_BICUBIC 3
#define LPI_FILTER_BOX 4
/* *bytes = the workspace lpi_image_resample_u8 needs for these B HOST descriptors: the descriptor table (B * LPI_RESAMPLE_DESC * 8 bytes, rounded up to
 * 256) + B * S * (4 + KX + KY) * 4 bytes, KX / KY the largest per-image tap count ceil(fs * max(crop / resized, 1)) * 2 + 1 of each axis (fs = the
 * filter's support; 1 for the entry without _f, which is the LPI_FILTER_BILINEAR case).  0 or LPI_EINVAL (invalid descriptors or filter, as above). */
int lpi_image_resample_workspace(int B, int S, const long* desc, long* bytes);
int lpi_image_resample_workspace_f(int filter, int B, int S, const long* desc, long* bytes);
/* out[B,3,S,S] uint8 (CHW, contiguous) from the ragged sources in `src` (device, src_bytes bytes), on `stream`.  desc: the HOST descriptor table
 * [B][LPI_RESAMPLE_DESC], validated here (also against src_bytes) and then copied by this call into the head of the workspace, from where the kernels
 * read it (pageable desc: free to change once the call returns; pinned desc: unchanged until the stream has passed the copy).  ws: device workspace of
 * ws_bytes >= lpi_image_resample_workspace's.  One copy and two launches (tap tables, then the resample; a third for images resampled
 * vertical-first), the same for every filter.  A workspace sized for another filter that is too small is LPI_EINVAL, not a write past its end.
 * lpi_image_resample_u8 is lpi_image_resample_u8_f with LPI_FILTER_BILINEAR. */
int lpi_image_resample_u8(int B, int S, const long* desc, const void* src, long src_bytes, void* ws, long ws_bytes, void* out, void* stream);
int lpi_image_resample_u8_f(int filter, int B, int S, const long* desc, const void* src, long src_bytes, void* ws, long ws_bytes, void* out,
                            void* stream);

/* ---- baseline JPEG decoding on the GPU (jpeg.hip)      replaces: Image.open(f).convert("RGB") of the data transforms (pixel_format='jpeg',
 * lpi_amd/imageops.py).  The output of every file is np.asarray(Image.open(f).convert("RGB")) under Pillow 12 (libjpeg-turbo: islow IDCT, fancy
 * upsampling, its YCbCr tables), byte for byte.
 * THE ENVELOPE (decided from the headers, here only): SOF0 / SOF1, 8-bit samples, Huffman coding, one scan holding every component in the
 * frame's order (Ss 0, Se 63, Ah = Al = 0); 1 component, or 3 that libjpeg reads as YCbCr (a JFIF APP0, or no Adobe APP14 and ids other than 'R','G','B') with luma sampling 1x1,
 * 2x1 or 2x2 and chroma 1x1; any DQT precision, up to 4 tables of each kind, restart intervals; at most LPI_JPEG_MAX_PIXELS pixels and
 * LPI_JPEG_MAX_SCAN_BYTES bytes from the scan's start to the end of the file.  Anything else is the host's (Pillow's). */
#define LPI_JPEG_INFO 8
#define LPI_JPEG_MAX_PIXELS (1L << 28)
#define LPI_JPEG_MAX_SCAN_BYTES (1L << 27)
/* Host only (no GPU call): info[LPI_JPEG_INFO] = {inside the envelope (1) or not (0), width, height, components, luma H, luma V, restart interval,
 * offset of the entropy-coded data}.  A file that does not start with SOI is {0, 0, 0, ...}.  0, or LPI_EINVAL for a structural error of the headers
 * (truncated, a bad segment length, a scan that names an undefined table, a bad Huffman table, ...). */
int lpi_jpeg_info(const void* data, long nbytes, long* info);
/* *bytes = the device workspace lpi_jpeg_decode_u8 needs for the B files packed in the HOST buffer `host` (file i = bytes [offsets[i], offsets[i+1])).
 * 0, or LPI_EINVAL (a file outside the envelope or with a structural error). */
int lpi_jpeg_decode_workspace(int B, const void* host, const long* offsets, long* bytes);
/* Decodes the B files on `stream`: file i is bytes [offsets[i], offsets[i+1]) of both `host` (parsed here, before any launch) and `src` (its device
 * copy, src_bytes bytes); its h x w x 3 RGB output is written at byte out_off[i] (HOST array) of `out` (device, out_bytes).  status: device int[B],
 * 0 when image i decoded exactly its MCUs, else a nonzero mask (1 premature end of data, 2 invalid Huffman code, 4 coefficient index past 63, 8 block
 * count mismatch, 16 restart markers missing or out of order): the caller then decodes that file on the host.  ws: device workspace of ws_bytes >=
 * lpi_jpeg_decode_workspace's; this call copies the descriptors and tables into it.  One copy, one clear and four launches.  LPI_EINVAL before any launch
 * for a file outside the envelope, a structural error, an output outside `out`, or a workspace too small. */
int lpi_jpeg_decode_u8(int B, const void* host, const long* offsets, const void* src, long src_bytes, const long* out_off, void* out, long out_bytes,
                       int* status, void* ws, long ws_bytes, void* stream);

/* ---- progressive JPEG files in the same decoder: the _x entry points take a flags word.  flags = 0 is the calls above: the same verdicts, workspace
 * bytes, launches and output bytes.  Unknown flag bits are LPI_EINVAL before any copy or launch.
 * LPI_JPEG_PROGRESSIVE widens THE ENVELOPE by SOF2 files (8-bit, Huffman; the component, sampling, colour-space and size rules above unchanged;
 * LPI_JPEG_MAX_SCAN_BYTES counts from the first scan's start) whose scan script is complete and orderly:
 *   - DC scans Ss = Se = 0 with 1 to nc components, in the frame's order when interleaved; AC scans one component, 1 <= Ss <= Se <= 63; Al <= 13;
 *   - for every coefficient of every component the first scan that holds it has Ah = 0, each later one has Ah = the previous Al and Al = Ah - 1, the
 *     last one Al = 0; a component's AC scans come after its first DC scan; at the file's end all 64 coefficients of every component are fully
 *     refined (libjpeg-turbo only warns on other scripts and smooths the blocks of an incomplete one: Pillow's pixels are then not the IDCT of
 *     the coefficients, so those files stay the host's);
 *   - every scan uses the Huffman tables and the restart interval in force at its SOS (DHT and DRI between scans are allowed, DQT is not);
 *   - at most LPI_JPEG_MAX_SCANS scans (Pillow's own files have 10, or 6 for grayscale).
 * The parser walks the whole file (every SOS, the entropy-coded bytes up to the next marker other than FF00 / RSTn).  A file that ends inside a scan
 * after a complete script is inside the envelope; its status is then nonzero.  One batch may mix baseline and progressive files.  The status bits
 * keep their meaning (2 also: a refinement symbol of a size other than 1).  For B files with S progressive scans in R rounds (scans that touch the
 * same coefficients of a component run in file order, in different rounds): two copies, one clear and 5 + R launches; 4 when S = 0. */
#define LPI_JPEG_PROGRESSIVE 1
#define LPI_JPEG_MAX_SCANS 32
/* lpi_jpeg_info_x fills LPI_JPEG_INFO_X fields: the LPI_JPEG_INFO of lpi_jpeg_info, then {the frame is SOF2 and was parsed as such (only with
 * LPI_JPEG_PROGRESSIVE), its scans inside the envelope (1 for a baseline file whose SOS was reached, else 0)}. */
#define LPI_JPEG_INFO_X 10
/* LPI_JPEG_LAYOUTS widens the frame rule of THE ENVELOPE for SOF0 / SOF1 files (one scan in the frame's order, 8-bit, Huffman and the size limits
 * as above): 1, 3 or 4 components; the first sampled 1x1, 2x1, 2x2, 1x2 (4:4:0), 4x1 (4:1:1) or 1x4, every other component 1x1; any colour marking
 * libjpeg accepts.  Three components: a JFIF APP0 says YCbCr; else an Adobe APP14 says RGB (transform 0) or YCbCr (any other value); else the ids
 * 'R','G','B' say RGB, any others YCbCr.  Four components: an Adobe APP14 with a transform other than 0 says YCCK, anything else CMYK; the output is
 * Pillow's convert("RGB") of its (inverted) CMYK image.  A four-component scan names up to four DC and four AC tables.  Upsampling as libjpeg-turbo's:
 * the triangle filter for 2x1, 2x2 and 1x2, replication for 4x1 and 1x4.  Other factors (3x1, 4x2, 2x4, ...), a later component that is not 1x1
 * and ratios that are not whole stay the host's.  lpi_jpeg_info_x then reports the first component's H and V for four-component files too.
 * A LIMIT OF THIS DECODER, not of the format: SOF2 files keep the frame rule above with LPI_JPEG_PROGRESSIVE | LPI_JPEG_LAYOUTS; the two flags
 * combine in one batch, but a progressive CMYK or 4:4:0 file is the host's.
 * A batch without a four-component file: the same workspace bytes, copies and launches as without the flag; with one: one more copy and one more
 * launch (the Huffman kernel's four-component instantiation).
 * The value is 4: flags 2 and 3 have been LPI_EINVAL since the flags word exists and callers rely on that, so bit 1 is never given a meaning. */
#define LPI_JPEG_LAYOUTS 4
#define LPI_JPEG_FLAGS (LPI_JPEG_PROGRESSIVE | LPI_JPEG_LAYOUTS) /* every valid bit */
int lpi_jpeg_info_x(int flags, const void* data, long nbytes, long* info);
int lpi_jpeg_decode_workspace_x(int flags, int B, const void* host, const long* offsets, long* bytes);
int lpi_jpeg_decode_u8_x(int flags, int B, const void* host, const long* offsets, const void* src, long src_bytes, const long* out_off, void* out,
                         long out_bytes, int* status, void* ws, long ws_bytes, void* stream);

void* lpi_bpe_create(const char* merges_utf8, long nbytes);
void lpi_bpe_destroy(void* handle);
int lpi_bpe_encode(void* handle, const char* text_utf8, int32_t* ids, int max_ids);
int lpi_bpe_tokenize(void* handle, const char* const* texts, int n, int context_length, int truncate, int64_t* out);

/* Which kernel the calling thread's last lpi_gemm_nt / lpi_gemm_nt_rows launched (-1: none yet): measurement tools attribute a
 * launch to a kernel with this instead of re-deriving the dispatch rules. */
#define LPI_GEMM_K_128 0        /* gemm_nt_kernel, 128x128 tiles                                  */
#define LPI_GEMM_K_256 1        /* gemm256_kernel, 256x256 tiles                                  */
#define LPI_GEMM_K_256_TAIL 2   /* gemm256_tail_kernel: 256x256 tiles, short last round as halves */
#define LPI_GEMM_K_256X128 3    /* gemm256x128_kernel                                             */
#define LPI_GEMM_K_ROWS 4       /* gemm_rows_kernel: few-row GEMM, 32x32 tiles over the whole K   */
#define LPI_GEMM_K_MX8 5        /* gemm_mx8_kernel: MX-FP8 operands, 128x128 tiles (lpi_gemm_nt_mx8) */
#define LPI_GEMM_K_X3 6         /* gemm_nt_kernel / gemm256_kernel on split-bf16 operands (LPI_F32X3) */
#define LPI_GEMM_K_MX8_256 7    /* gemm256_mx8_kernel: MX-FP8 operands, phased 256x256 tiles (lpi_gemm_nt_mx8_256) */
int lpi_gemm_last_kernel(void);

/* ---- MX-FP8 forward (csrc/gemm_mx8.hip, csrc/mx8_rows.hip): the four block GEMMs of the no-grad forwards on the block-scaled FP8 matrix instruction ----
 * replaces (EngineOptions.mx8_forward, train=False only): models/clip/model.py:172-177 (ln_1 -> in_proj, out_proj, ln_2 -> c_fc -> QuickGELU -> c_proj).
 * THE FORMAT.  Elements: OCP e4m3fn bytes (torch.float8_e4m3fn; not MI300X's fnuz), round to nearest even, subnormals kept.  Scales: one E8M0 byte
 * (value 2^(byte - 127)) per 32 consecutive K elements, stored [rows, K/32] row-major with a leading dimension.  Block scale: for the block maximum amax
 * the exponent is e = floor(log2 amax) - 8, raised by one if amax 2^-e > 448, clamped to [-127, 127]; byte = e + 127; element = y 2^-e rounded.  No
 * element ever saturates (a deliberate departure from the OCP floor rule): |deq - y| <= max(2^-4 |y|, 2^-10 S) with S the block's scale.  An all-zero
 * block is byte 0 and zero elements.  NaN / Inf inputs are out of contract.
 * LPI_MX8 as lpi_gemm_nt_mx8's c_dtype: C is e4m3 bytes [M, ldc] and c_scales [M, ldcs >= N/32] receives the scales along N. */
#define LPI_MX8 3
/* 1 if lpi_gemm_nt_mx8 takes the shape (M, N, K positive multiples of 128), else 0.  Host only: no GPU call. */
int lpi_gemm_mx8_ok(int M, int N, int K);
/* C[M,N] = epi(alpha * A[M,K] . B[N,K]^T + bias) (+ residual), A / B e4m3 with scales a_scales [M, ldas] / b_scales [N, ldbs] (ld* multiples of 4, 4-byte
 * aligned), f32 accumulation.  c_dtype LPI_F32 | LPI_BF16 | LPI_F16 | LPI_MX8.  Epilogues LPI_EPI_NONE and LPI_EPI_QUICKGELU (no aux); residual (LPI_EPI_NONE
 * only) has C's type: fp16 with LPI_F16, f32 with LPI_F32 (LPI_ENOSYS with bf16, LPI_EINVAL with LPI_MX8).  bias f32 or NULL.  LPI_EINVAL before any launch
 * for any other shape, a NULL scale pointer of an MX operand or output, or a misaligned argument.  Attributed to LPI_GEMM_K_MX8. */
int lpi_gemm_nt_mx8(int c_dtype, int M, int N, int K, const void* A, int lda, const void* a_scales, int ldas, const void* B, int ldb,
                    const void* b_scales, int ldbs, void* C, int ldc, void* c_scales, int ldcs, const float* bias, const void* residual, int ldr,
                    int epilogue, float alpha, void* stream);
/* 1 if lpi_gemm_nt_mx8_256 takes the shape: M, N positive multiples of 256 and K a positive multiple of 256 (an even number >= 2 of K-tiles of 128 elements),
 * else 0.  Host only: no GPU call. */
int lpi_gemm_mx8_256_ok(int M, int N, int K);
/* lpi_gemm_nt_mx8 on the phased 256x256 tile (csrc/gemm256_tile.h on one-byte elements: LDS-DMA ring with counted waits, the scale bytes by LDS-DMA beside
 * the elements): the same arguments, meaning, epilogues, outputs and refusals, and the SAME BITS — each output element is the same sequence of block-scaled
 * instructions over K.  LPI_EINVAL before any launch for a shape lpi_gemm_mx8_256_ok refuses.  One launch, one tile per workgroup, attributed to
 * LPI_GEMM_K_MX8_256.  lpi_gemm_nt_mx8 itself always runs the 128x128 kernel. */
int lpi_gemm_nt_mx8_256(int c_dtype, int M, int N, int K, const void* A, int lda, const void* a_scales, int ldas, const void* B, int ldb,
                        const void* b_scales, int ldbs, void* C, int ldc, void* c_scales, int ldcs, const float* bias, const void* residual, int ldr,
                        int epilogue, float alpha, void* stream);
/* rows of x (`x_dtype`: LPI_F32 | LPI_BF16 | LPI_F16, [rows, ldx]) -> q (e4m3 [rows, ldq]) + scales ([rows, lds >= K/32]); K a multiple of 32. */
int lpi_mx8_quantize(int x_dtype, int rows, int K, const void* x, int ldx, void* q, int ldq, void* scales, int lds, void* stream);
/* LayerNorm (f32 two-sweep statistics in registers, eps 1e-5, affine in f32) of the rows of the residual stream x (`x_dtype`: LPI_F16 | LPI_F32) written
 * straight as MX-FP8: LN(x) never exists in a 2-byte type.  d a multiple of 32, <= 1024.  mean / rstd (f32 [rows]) are optional outputs (NULL: not written). */
int lpi_layernorm_mx8_fwd(int x_dtype, int rows, int d, const void* x, int ldx, const float* gamma, const float* beta, void* q, int ldq,
                          void* scales, int lds, float* mean, float* rstd, void* stream);


#ifdef __cplusplus
}
#endif
#endif /* LPI_HIP_H */
