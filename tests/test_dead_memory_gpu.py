"""No kernel reads dead memory into a live value.

The speed of this code base comes from skipping work: pooled rows only, prompt rows only, ragged and shared-prefix batches, 32-row tiles over
lengths such as 213, arenas padded to 256 rows and reused for smaller batches.  Each leaves memory a kernel is handed but must not use
(include/lpi_hip.h, "Dead regions").  Every case here runs twice through tests/poison.py — zeros, then NaN, in the dead regions — and requires
bit-identical live outputs, untouched preserved regions, no NaN, and the f64 CPU reference of the operation at the bar the kernel's own test in
tests/test_kernels_gpu.py uses (F32 2e-5, BF16 2e-2 and that file's f16 bars; each bar below names its source).  Token-row buffers are allocated
as the engine allocates them, rows rounded up to 256, so that "behind the last sample" exists inside the allocation: poison never leaves an
allocation, no index is out of range, and a wrong kernel fails an assertion instead of faulting.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import poison as P  # noqa: E402
from lpi_amd import _lib, engine as E, synth  # noqa: E402
from lpi_amd._lib import BF16, F16, F32, call  # noqa: E402

DEV = "cuda:0"
TD = {F32: torch.float32, BF16: torch.bfloat16, F16: torch.float16}
GD = {F32: torch.float32, BF16: torch.bfloat16, F16: torch.bfloat16}      # gradients of the f16 mode are bf16 (test_attention_f16_forward_bf16_backward)
TOL = {F32: 2e-5, BF16: 2e-2}                                             # tests/test_kernels_gpu.py: TOL
NAME = {F32: "f32", BF16: "bf16", F16: "f16"}


def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g) * scale


def pad256(n):
    return (n + 255) // 256 * 256


def stream():
    return torch.cuda.current_stream().cuda_stream


def run(case, label):
    return P.two_arms(case, label, sync=torch.cuda.synchronize)


def rows_in(n, rows):
    """bool [n]: True at `rows`"""
    m = torch.zeros(n, dtype=torch.bool)
    m[torch.as_tensor(rows, dtype=torch.long)] = True
    return m


def padded(ref, rows):
    """a [M, ...] reference inside `rows` rows (the rest is never compared)"""
    out = torch.zeros((rows,) + tuple(ref.shape[1:]), dtype=torch.float64)
    out[:ref.shape[0]] = ref
    return out


def attn_ref(qkv, B, L, H, causal):
    """tests/test_kernels_gpu.py: attn_ref"""
    d = H * 64
    q, k, v = qkv.double().reshape(B, L, 3, H, 64).permute(2, 0, 3, 1, 4)
    s = (q * 0.125) @ k.transpose(-1, -2)
    if causal:
        s = s + torch.full((L, L), float("-inf"), dtype=torch.float64).triu_(1)
    p = torch.softmax(s, -1)
    return (p @ v).transpose(1, 2).reshape(B * L, d), torch.logsumexp(s, -1)


# ------------------------------------------------------------------------------------------------ full attention, uniform batches
# one shape per kernel path: short one-head kernels | causal | streamed single-pass backward of the 2-byte types | two key windows, swizzled
# images, Lp 288 | the smallest long-sequence shape (attn_long.hip).  B = 2: sample 0's tail block is followed by live rows, sample 1's by poison.
@pytest.mark.parametrize("dt", [F32, BF16, F16])
@pytest.mark.parametrize("B,L,H,causal", [(2, 21, 2, 0), (2, 77, 2, 1), (2, 213, 2, 0), (1, 273, 2, 0), (1, 289, 1, 0)])
def test_full_attention_reads_no_row_behind_the_batch(dt, B, L, H, causal):
    d, M = H * 64, B * L
    Mp = pad256(M)
    qkv = rnd(Mp, 3 * d, seed=11).to(TD[dt])
    dctx = rnd(Mp, d, seed=12).to(GD[dt])
    qr = qkv[:M].double().requires_grad_(True)
    oref, lref = attn_ref(qr, B, L, H, causal)
    oref.backward(dctx[:M].double())
    oref, lref, gref = padded(oref.detach(), Mp), lref.detach(), padded(qr.grad, Mp)
    live = torch.arange(Mp) < M
    long_ = L > 288
    # test_attention_fwd_bwd (F32, BF16), test_attention_f16_forward_bf16_backward (F16), test_attention_long_sequences_fwd_bwd (L > 288: bf16's bars for f16 too)
    ctol = {F32: 2e-5, BF16: 2e-2, F16: 2e-2 if long_ else 3e-3}[dt]
    ltol = {F32: 1e-5, BF16: 2e-2, F16: 2e-2 if long_ else 3e-3}[dt]
    gtol = 5e-5 if dt == F32 else 4e-2

    def case(arm):
        q, dc = qkv.to(DEV), dctx.to(DEV)
        ctx = torch.zeros(Mp, d, device=DEV, dtype=TD[dt])
        lse = torch.zeros(B, H, L, device=DEV)
        arm.dead(q, ~live), arm.dead(ctx, ~live), arm.dead(dc, ~live)
        call("lpi_attn_fwd", dt, B, L, H, q, 3 * d, ctx, d, lse, causal, stream())
        arm.out("ctx", ctx, live, oref, ctol)
        arm.out("lse", lse, None, lref, ltol)
        dqkv = torch.zeros(Mp, 3 * d, device=DEV, dtype=GD[dt])
        delta = torch.zeros(B, H, L, device=DEV)
        arm.dead(delta)                                      # scratch: "the contents are unspecified"
        arm.dead(ctx, ~live, count=False)                    # whatever the forward left behind the batch is dead to the backward too
        call("lpi_attn_bwd", dt, B, L, H, q, 3 * d, ctx, d, dc, d, lse, delta, dqkv, 3 * d, causal, stream())
        for name, sl in (("dq", slice(0, d)), ("dk", slice(d, 2 * d)), ("dv", slice(2 * d, 3 * d))):
            arm.out(name, dqkv[:, sl], live, gref[:, sl], gtol)

    run(case, f"attn_fwd/bwd {NAME[dt]} B={B} L={L} H={H} causal={causal}")


# ------------------------------------------------------------------------------------------------ ragged causal batches
RAGGED = [59, 17, 32, 5]


@pytest.mark.parametrize("dt", [F32, BF16, F16])
def test_ragged_attention_reads_nothing_behind_a_sample(dt):
    """lpi_attn_fwd_varlen / _bwd_varlen / lpi_attn_bwd_prefix: rows >= row_start[B], the lse entries l >= L_b (poisoned between the forward and the
    backward) and delta are dead.  The prefix form (rows_needed = 17) is compared at rows < 17 of every sample: the header lets the rest stay unwritten."""
    B, Lmax, H, causal, need = 4, 59, 2, 1, 17
    d = H * 64
    lens = torch.tensor(RAGGED)
    rs = torch.cat([torch.zeros(1, dtype=torch.long), lens.cumsum(0)])
    M = int(rs[-1])
    Mp = pad256(M)
    qkv = rnd(Mp, 3 * d, seed=31).to(TD[dt])
    dctx = rnd(Mp, d, seed=32).to(GD[dt])
    oref, gref = torch.zeros(Mp, d, dtype=torch.float64), torch.zeros(Mp, 3 * d, dtype=torch.float64)
    lref = torch.zeros(B, H, Lmax, dtype=torch.float64)
    for b in range(B):
        r0, L = int(rs[b]), int(lens[b])
        qr = qkv[r0:r0 + L].double().requires_grad_(True)
        o, l_ = attn_ref(qr, 1, L, H, causal)
        o.backward(dctx[r0:r0 + L].double())
        oref[r0:r0 + L], gref[r0:r0 + L], lref[b, :, :L] = o.detach(), qr.grad, l_.detach()[0]
    live = torch.arange(Mp) < M
    lse_dead = (torch.arange(Lmax)[None, None, :] >= lens[:, None, None]).expand(B, H, Lmax)
    # test_attention_varlen_fwd_bwd: tol, the lse bar, gtol — per sample, as there
    ctol = {F32: 2e-5, BF16: 2e-2, F16: 3e-3}[dt]
    ltol = 1e-5 if dt == F32 else 2e-2
    gtol = {F32: 5e-5, BF16: 4e-2, F16: 4e-2}[dt]

    def case(arm):
        q, dc, rs_d = qkv.to(DEV), dctx.to(DEV), rs.int().to(DEV)
        ctx = torch.zeros(Mp, d, device=DEV, dtype=TD[dt])
        lse = torch.zeros(B, H, Lmax, device=DEV)
        arm.dead(q, ~live), arm.dead(ctx, ~live), arm.dead(dc, ~live)
        call("lpi_attn_fwd_varlen", dt, B, Lmax, rs_d, H, q, 3 * d, ctx, d, lse, causal, stream())
        for b in range(B):
            own = rows_in(Mp, range(int(rs[b]), int(rs[b + 1])))
            arm.out(f"ctx[{b}]", ctx, own, oref, ctol)
            arm.out(f"lse[{b}]", lse[b], ~lse_dead[b], lref[b], ltol)
        arm.dead(lse, lse_dead)
        arm.dead(ctx, ~live, count=False)
        dqkv, part = torch.zeros(Mp, 3 * d, device=DEV, dtype=GD[dt]), torch.zeros(Mp, 3 * d, device=DEV, dtype=GD[dt])
        delta, delta_p = torch.zeros(B, H, Lmax, device=DEV), torch.zeros(B, H, Lmax, device=DEV)
        arm.dead(delta), arm.dead(delta_p)
        call("lpi_attn_bwd_varlen", dt, B, Lmax, rs_d, H, q, 3 * d, ctx, d, dc, d, lse, delta, dqkv, 3 * d, causal, stream())
        call("lpi_attn_bwd_prefix", dt, B, Lmax, rs_d, need, H, q, 3 * d, ctx, d, dc, d, lse, delta_p, part, 3 * d, causal, stream())
        for b in range(B):
            r0, L = int(rs[b]), int(lens[b])
            arm.out(f"dqkv[{b}]", dqkv, rows_in(Mp, range(r0, r0 + L)), gref, gtol)
            arm.out(f"prefix dqkv[{b}]", part, rows_in(Mp, range(r0, r0 + min(L, need))), gref, gtol)

    run(case, f"attn varlen fwd/bwd/prefix {NAME[dt]} lengths {RAGGED}")


# ------------------------------------------------------------------------------------------------ pooled-row attention
class _Pooled:
    """One lpi_attn_pooled_fwd / _bwd problem: q arrives separately, so columns 0..d of qkv are dead; under the causal mask so are the K / V rows
    j > idx[b]; dqkv starts as NaN, must come back with zeros behind the mask, and its columns 0..d are preserved."""

    def __init__(self, dt, B, L, H, causal, idx, seed):
        self.dt, self.B, self.L, self.H, self.causal = dt, B, L, H, causal
        d = self.d = H * 64
        M = self.M = B * L
        Mp = self.Mp = pad256(M)
        self.idx = torch.tensor(idx if idx is not None else [0] * B, dtype=torch.int32)
        self.has_idx = idx is not None
        rows = torch.arange(B) * L + self.idx.long()
        self.qkv = rnd(Mp, 3 * d, seed=seed).to(TD[dt])
        self.dctx = rnd(B, d, seed=seed + 1).to(GD[dt])
        self.q_rows = self.qkv[rows, :d].contiguous()
        qr = self.qkv[:M].double().requires_grad_(True)
        oref, lref = attn_ref(qr, B, L, H, causal)
        dfull = torch.zeros(M, d, dtype=torch.float64)
        dfull[rows] = self.dctx.double()
        oref.backward(dfull)
        self.oref, self.lref = oref.detach()[rows], lref.detach()[torch.arange(B), :, self.idx.long()]
        self.dq_ref, self.g_ref = qr.grad[rows, :d], padded(qr.grad, Mp)
        dead = torch.zeros(Mp, 3 * d, dtype=torch.bool)
        dead[:, :d] = True
        dead[M:] = True
        if causal:
            for b in range(B):
                dead[b * L + int(self.idx[b]) + 1:(b + 1) * L] = True
        self.dead = dead
        self.live = torch.arange(Mp) < M
        self.qcols = torch.zeros(Mp, 3 * d, dtype=torch.bool)
        self.qcols[:, :d] = True

    def buffers(self, arm, tag):
        d, B, dt = self.d, self.B, self.dt
        t = dict(B=B, L=self.L, H=self.H, row_start=None, q=self.q_rows.to(DEV), ldq=d, qkv=self.qkv.to(DEV), ldqkv=3 * d,
                 idx=self.idx.to(DEV) if self.has_idx else None, ctx=torch.zeros(B, d, device=DEV, dtype=TD[dt]), ldctx=d,
                 lse=torch.zeros(B, self.H, device=DEV), dctx=self.dctx.to(DEV), lddctx=d, dq=torch.zeros(B, d, device=DEV, dtype=GD[dt]), lddq=d,
                 dqkv=torch.full((self.Mp, 3 * d), float("nan"), device=DEV, dtype=GD[dt]), lddqkv=3 * d, causal=self.causal, shared_rows=0, shared_dkv=None)
        arm.dead(t["qkv"], self.dead)
        arm.preserve(tag + "dqkv[:, :d]", t["dqkv"], self.qcols)
        return t

    def outs(self, arm, t, tag):
        dt, d = self.dt, self.d
        # test_attention_pooled_row_fwd_bwd (F32, BF16); test_layernorm_f16_output_and_pooled_attention_f16 (F16: no lse bar there — bits only)
        arm.out(tag + "ctx", t["ctx"], None, self.oref, {F32: 2e-5, BF16: 2e-2, F16: 3e-3}[dt])
        arm.out(tag + "lse", t["lse"], None, *((None, None) if dt == F16 else (self.lref, 1e-5 if dt == F32 else 2e-2)))
        gtol = 5e-5 if dt == F32 else 4e-2
        arm.out(tag + "dq", t["dq"], None, self.dq_ref, gtol)
        arm.out(tag + "dk", t["dqkv"][:, d:2 * d], self.live, self.g_ref[:, d:2 * d], gtol)
        arm.out(tag + "dv", t["dqkv"][:, 2 * d:], self.live, self.g_ref[:, 2 * d:], gtol)


POOLED = [(3, 77, 2, 1, [0, 40, 76]), (2, 21, 2, 0, None)]


@pytest.mark.parametrize("dt", [F32, BF16, F16])
@pytest.mark.parametrize("B,L,H,causal,idx", POOLED)
def test_pooled_attention_reads_neither_q_columns_nor_masked_keys(dt, B, L, H, causal, idx):
    pr = _Pooled(dt, B, L, H, causal, idx, seed=21)

    def case(arm):
        t = pr.buffers(arm, "")
        call("lpi_attn_pooled_fwd", dt, B, L, H, t["q"], t["ldq"], t["qkv"], t["ldqkv"], t["idx"], t["ctx"], t["ldctx"], t["lse"], causal, stream())
        call("lpi_attn_pooled_bwd", dt, B, L, H, t["q"], t["ldq"], t["qkv"], t["ldqkv"], t["idx"], t["dctx"], t["lddctx"], t["lse"], t["dq"], t["lddq"],
             t["dqkv"], t["lddqkv"], causal, stream())
        pr.outs(arm, t, "")

    run(case, f"attn_pooled fwd/bwd {NAME[dt]} B={B} L={L} H={H} causal={causal}")


def test_pooled_attention_pair_launch_reads_neither_q_columns_nor_masked_keys():
    """The BF16 cases once more through lpi_attn_pooled_fwd_pair / _bwd_pair (the two towers' last block as one launch)."""
    prs = [_Pooled(BF16, B, L, H, causal, idx, seed=21 + 10 * i) for i, (B, L, H, causal, idx) in enumerate(POOLED)]

    def case(arm):
        ts = [pr.buffers(arm, f"[{i}] ") for i, pr in enumerate(prs)]
        _lib.attn_pooled_pair(BF16, ts[0], ts[1], stream())
        _lib.attn_pooled_pair(BF16, ts[0], ts[1], stream(), backward=True)
        for i, pr in enumerate(prs):
            pr.outs(arm, ts[i], f"[{i}] ")

    run(case, "attn_pooled pair fwd/bwd bf16")


# ------------------------------------------------------------------------------------------------ the last block without K and V
@pytest.mark.parametrize("dtname", ["bf16", "f16"])
def test_last_block_from_the_stream_reads_no_dead_scratch_or_row(dtname):
    """lpi_spool_attn_fwd / _bwd at B = 2, L = 21, H = 2, d = 128 (head_dim is 64, so d = 64 H: the smallest shape with two heads).  Dead: all of `scratch`
    before the forward; after it the parts the backward is documented not to read (its second quarter and its second half); rows >= B L of x, mean, rstd.
    The f64 reference and the bars are those of tests/test_round6_gpu.py::test_last_block_attention_from_the_stream_against_f64."""
    B, L, H = 2, 21, 2
    d, M = 64 * H, B * L
    Mp = pad256(M)
    dt, tdt = (BF16, torch.bfloat16) if dtname == "bf16" else (F16, torch.float16)
    assert _lib.load().lpi_spool_attn_supported(L, H, d) == 1
    g = torch.Generator().manual_seed(B * 1000 + L)
    x = (torch.randn(Mp, d, generator=g) * 1.3 + 0.4 * torch.randn(Mp, 1, generator=g)).half()
    gamma = 1.0 + 0.1 * torch.randn(d, generator=g)
    beta = 0.05 * torch.randn(d, generator=g)
    W = (torch.randn(3 * d, d, generator=g) * d ** -0.5).to(tdt)
    bq = 0.02 * torch.randn(3 * d, generator=g)
    q = torch.randn(B, d, generator=g).to(tdt)
    dctx = torch.randn(B, d, generator=g).bfloat16()
    x64 = x.double()
    mean = x64.mean(1)
    rstd = 1.0 / (x64.var(1, unbiased=False) + 1e-5).sqrt()
    h = ((x64 - mean[:, None]) * rstd[:, None] * gamma.double() + beta.double())[:M].clone().requires_grad_(True)       # LN1(x_l)
    qr = q.double().requires_grad_(True)
    Wd, bd = W.double(), bq.double()
    k = (h @ Wd[d:2 * d].t() + bd[d:2 * d]).view(B, L, H, 64)
    v = (h @ Wd[2 * d:].t() + bd[2 * d:]).view(B, L, H, 64)
    s = torch.einsum("bhc,blhc->bhl", qr.view(B, H, 64), k) / 8.0
    ctx_ref = torch.einsum("bhl,blhc->bhc", torch.softmax(s, dim=-1), v).reshape(B, d)
    (ctx_ref * dctx.double()).sum().backward()
    live = torch.arange(Mp) < M
    n = B * H * d

    def case(arm):
        xd, md, rd = x.to(DEV), mean.float().to(DEV), rstd.float().to(DEV)
        arm.dead(xd, ~live), arm.dead(md, ~live), arm.dead(rd, ~live)
        scratch = torch.zeros(4 * n, device=DEV)
        arm.dead(scratch)
        lse = torch.zeros(B, H, device=DEV)
        ctx = torch.zeros(B, d, device=DEV, dtype=tdt)
        Wdv, bdv, gd, bd_ = W.to(DEV), bq.to(DEV), gamma.to(DEV), beta.to(DEV)
        call("lpi_spool_attn_fwd", dt, B, L, H, q.to(DEV), d, Wdv, d, Wdv.t().contiguous(), 3 * d, bdv, xd, d, md, rd, gd, bd_, scratch, lse, ctx, d, stream())
        arm.out("ctx", ctx, None, ctx_ref.detach(), 1e-2)
        arm.out("lse", lse)
        arm.dead(scratch[n:], None, count=False)              # the backward reads the first quarter only
        dq = torch.zeros(B, d, device=DEV, dtype=torch.bfloat16)
        dh = torch.full((Mp, d), float("nan"), device=DEV, dtype=torch.bfloat16)
        Wb = Wdv.bfloat16()
        call("lpi_spool_attn_bwd", B, L, H, Wb, d, Wb.t().contiguous(), 3 * d, xd, d, md, rd, gd, scratch, lse, dctx.to(DEV), d, dq, d, dh, d, stream())
        arm.out("dq", dq, None, qr.grad, 1.5e-2)
        arm.out("dh", dh, live, padded(h.grad, Mp), 1.5e-2)

    run(case, f"spool_attn fwd/bwd {dtname} B={B} L={L} H={H}")


# ------------------------------------------------------------------------------------------------ LayerNorm operand blocks
def gelu_grad_ref(u):
    sg = torch.sigmoid(1.702 * u)
    return sg * (1 + 1.702 * u * (1 - sg))


@pytest.mark.parametrize("cdt", [BF16, F16])
def test_layernorm_fold_gemm_reads_no_entry_behind_m_of_its_operand_block(cdt):
    """LPI_EPI_LN / LPI_EPI_LN_QUICKGELU with ldr = M + 4 at the smallest shape lpi_gemm_ln_supported accepts: entries M .. ldr - 1 of the mean and the
    rstd segment of the block are dead.  Operands and bars: test_gemm_layernorm_fold_epilogues / _ln_fold_operands."""
    M, N, K = 256, 256, 128
    sup = _lib.load().lpi_gemm_ln_supported
    assert sup(F16, M, N, K) == 1 and sup(F16, M - 128, N, K) == 0 and sup(F16, M, N - 128, K) == 0 and sup(F16, M, N, K - 64) == 0
    ctd = TD[cdt]
    tol = 6e-3 if cdt == BF16 else 1.5e-3
    ldr = M + 4
    x = rnd(M, K, seed=1) + 0.7 * rnd(M, 1, seed=2)
    x[:, 3] *= 20.0
    x = x.half()
    w = rnd(N, K, seed=3, scale=0.05)
    b, gamma, beta = rnd(N, seed=4), 1.0 + 0.3 * rnd(K, seed=5), 0.2 * rnd(K, seed=6)
    xd = x.double()
    mu, var = xd.mean(1, keepdim=True), xd.var(1, unbiased=False, keepdim=True)
    ref = ((xd - mu) / torch.sqrt(var + 1e-5) * gamma.double() + beta.double()) @ w.double().t() + b.double()
    wl = (w.double() * gamma.double()[None, :]).half()
    blk0 = torch.zeros(2 * ldr + N)
    blk0[:M], blk0[ldr:ldr + M], blk0[2 * ldr:] = mu[:, 0].float(), (1.0 / torch.sqrt(var[:, 0] + 1e-5)).float(), wl.double().sum(1).float()
    c2 = (w.double() @ beta.double() + b.double()).float()
    dead = torch.zeros(2 * ldr + N, dtype=torch.bool)
    dead[M:ldr] = True
    dead[ldr + M:2 * ldr] = True

    def case(arm):
        blk = arm.dead(blk0.to(DEV), dead)
        a, bw, bias = x.to(DEV), wl.to(DEV), c2.to(DEV)
        c, g = torch.zeros(M, N, dtype=ctd, device=DEV), torch.zeros(M, N, dtype=ctd, device=DEV)
        aux = torch.zeros(M, N, dtype=torch.bfloat16, device=DEV)
        call("lpi_gemm_nt", F16, cdt, M, N, K, a, K, bw, K, c, N, bias, blk, ldr, E.EPI_LN, None, 0, 1.0, stream())
        call("lpi_gemm_nt", F16, cdt, M, N, K, a, K, bw, K, g, N, bias, blk, ldr, E.EPI_LN_QUICKGELU, aux, N, 1.0, stream())
        arm.out("LN", c, None, ref, tol)
        arm.out("LN_QUICKGELU", g, None, ref * torch.sigmoid(1.702 * ref), tol)
        arm.out("LN_QUICKGELU aux", aux, None, gelu_grad_ref(ref), 6e-3)

    assert run(case, f"gemm EPI_LN / EPI_LN_QUICKGELU c={NAME[cdt]} ldr=M+4") == 8


def test_ln_stats_finalize_reads_no_slot_tail():
    """lpi_ln_stats_finalize with ld = rows + 4: the tail of every slot is dead.  Bars: test_gemm_residual_epilogue_with_row_statistics (mean to 1e-5
    absolute, rstd x std to 2e-5)."""
    rows, d = 37, 384
    ld, ns = rows + 4, d // 128
    x = (rnd(rows, d, seed=3) * 3 + 0.7).half().double()
    xs = x.view(rows, ns, 128)
    part0 = torch.zeros(2 * ns, ld)
    part0[:, :rows] = torch.stack([xs.sum(-1).t(), (xs * xs).sum(-1).t()], 1).reshape(2 * ns, rows).float()
    dead = torch.zeros(2 * ns, ld, dtype=torch.bool)
    dead[:, rows:] = True
    std = x.std(1, unbiased=False).clamp_min(1e-3)

    def case(arm):
        part = arm.dead(part0.to(DEV), dead)
        mean, rstd = torch.zeros(rows, device=DEV), torch.zeros(rows, device=DEV)
        call("lpi_ln_stats_finalize", rows, d, part, ld, 1e-5, mean, rstd, stream())
        arm.out("mean", mean, None, x.mean(1), 1e-5, err=lambda got, ref: float((got.double() - ref).abs().max()))
        arm.out("rstd", rstd, None, 1.0 / std, 2e-5, err=lambda got, ref: float((got.double() / ref - 1).abs().max()))

    assert run(case, "ln_stats_finalize ld=rows+4") == 2 * ns * 4


# ------------------------------------------------------------------------------------------------ row kernels with a row map
# B = 3 samples of L = 11 tokens inside a 256-row arena; the prompt rows b L + 1 + p (row0 = 1, P = 4) or the pooled rows b L + idx[b].  d = 520 gives
# three 256-column chunks, the last holding 8 columns; it is a multiple of 8, so the 16-byte half-wave kernels take it too.
RB, RL, ROW0, RP = 3, 11, 1, 4
RMP = pad256(RB * RL)
MAPPED = [b * RL + ROW0 + p for b in range(RB) for p in range(RP)]
IDX = [0, 7, 10]
POOLROWS = [b * RL + IDX[b] for b in range(RB)]
MROWS, PROWS = rows_in(RMP, MAPPED), rows_in(RMP, POOLROWS)
ROW_D = [128, 520]


def in_rows(ref, rows, like_rows=RMP):
    """a compact [len(rows), ...] reference scattered to its rows of a [like_rows, ...] array"""
    out = torch.zeros((like_rows,) + tuple(ref.shape[1:]), dtype=torch.float64)
    out[torch.as_tensor(rows)] = ref.double()
    return out


def row_stats(x64):
    return x64.mean(1).float(), (1.0 / (x64.var(1, unbiased=False) + 1e-5).sqrt()).float()


def ln_bwd_ref(x64, gamma, dy64):
    xr = x64.clone().requires_grad_(True)
    torch.nn.functional.layer_norm(xr, (x64.shape[1],), gamma.double(), None, 1e-5).backward(dy64)
    return xr.grad


def abs_err(got, ref):
    return float((got.double() - ref).abs().max())


def ratio_err(got, ref):
    return float((got.double() / ref - 1).abs().max())


# Every piece builds its buffers, marks the dead / preserved regions through `arm`, and returns (single, job, collect): the call through the entry point
# of its own, the same work as an lpi_row_job (None where lpi_row_jobs has no such op), and the registration of its live outputs.
def piece_ln_bwd_rows(arm, d, dy_dt, cast_dt, x_dt, with_dx, tag=""):
    x = (rnd(RMP, d, seed=5) * 2 + 0.3).to(TD[x_dt])
    gam = 1 + 0.1 * rnd(d, seed=6)
    dy = rnd(RB * RP, d, seed=8).to(TD[dy_dt])
    dx0, cast0 = rnd(RMP, d, seed=9), rnd(RMP, d, seed=10).to(TD[cast_dt])
    mean, rstd = row_stats(x.double())
    g = ln_bwd_ref(x[MAPPED].double(), gam, dy.double())
    ref = in_rows((dx0 if with_dx else cast0)[MAPPED].double() + g, MAPPED)
    xd, md, rd = x.to(DEV), mean.to(DEV), rstd.to(DEV)
    arm.dead(xd, ~MROWS), arm.dead(md, ~MROWS), arm.dead(rd, ~MROWS)
    dx = arm.preserve(tag + "dx", dx0.to(DEV), ~MROWS) if with_dx else None
    cast = arm.preserve(tag + "dx_cast", cast0.to(DEV), ~MROWS)
    dyd, gd = dy.to(DEV), gam.to(DEV)

    def single():
        call("lpi_layernorm_bwd_rows", dy_dt, cast_dt, x_dt, RB, RL, ROW0, RP, d, dyd, d, xd, d, gd, md, rd, dx, d, cast, d, 1, stream())

    job = None
    if (dy_dt, cast_dt, x_dt, with_dx) == (BF16, BF16, F16, False):
        job = _lib.row_job(_lib.ROWOP_LN_BWD_ROWS_H16, B=RB, L=RL, row0=ROW0, P=RP, d=d, a=dyd, ld_a=d, b=xd, ld_b=d, gamma=gd, mean_in=md, rstd_in=rd,
                           out2=cast, ld_c=d, flag=1)

    def collect():
        if with_dx:      # test_layernorm_fwd_bwd: the f32 stream to 2e-5, its cast copy to TOL
            arm.out(tag + "dx", dx, MROWS, ref, 2e-5)
            arm.out(tag + "dx_cast", cast, MROWS, ref, TOL[cast_dt])
        else:            # test_layernorm_bwd_bf16_gradient_stream / test_fp16_residual_stream_kernels: the bf16 stream to 1e-2
            arm.out(tag + "dx_cast", cast, MROWS, ref, 1e-2 if cast_dt == BF16 else TOL[cast_dt])
    return single, job, collect


def piece_gather_batch_rows(arm, d, dt, tag=""):
    src = rnd(RMP, d, seed=13).to(TD[dt])
    sd = arm.dead(src.to(DEV), ~MROWS)
    dst = torch.full((RB * RP, d), float("nan"), device=DEV, dtype=TD[dt])
    ch = d * (4 if dt == F32 else 2) // 16

    def single():
        call("lpi_gather_batch_rows", dt, RB, RL, ROW0, RP, d, sd, d, dst, d, stream())
    job = _lib.row_job(_lib.ROWOP_GATHER_BATCH_ROWS, B=RB, L=RL, row0=ROW0, P=RP, d=ch, a=sd, ld_a=ch, out=dst, ld_c=ch)
    return single, job, lambda: arm.out(tag + "dst", dst, None, src[MAPPED].double(), 0)      # a copy: test_row_kernels_varlen asks for equality


def piece_rows_sum(arm, d, dt, tag=""):
    dx = rnd(RMP, d, seed=14).to(TD[dt])
    dxd = arm.dead(dx.to(DEV), ~MROWS)
    out = torch.full((RP, d), float("nan"), device=DEV)

    def single():
        call("lpi_rows_sum_over_batch", dt, RB, RL, ROW0, RP, d, dxd, out, 0, stream())
    return single, None, lambda: arm.out(tag + "out", out, None, dx[MAPPED].double().view(RB, RP, d).sum(0), TOL[dt])


def piece_vis_assemble_bwd(arm, d, dt, tag=""):
    G2 = RL - 1 - RP
    pr = rnd(RP, d, seed=15) * 2 + 0.3
    gam = 1 + 0.1 * rnd(d, seed=16)
    dx0 = rnd(RMP, d, seed=17).to(TD[dt])
    xrows = pr.repeat(RB, 1).double()                      # the LayerNorm input of row (b, 1 + p) is prompt0[p]
    m, r = row_stats(xrows)
    mean, rstd = torch.zeros(RMP), torch.zeros(RMP)
    mean[MAPPED], rstd[MAPPED] = m, r
    g = ln_bwd_ref(xrows, gam, dx0[MAPPED].double())
    dxd, md, rd = dx0.to(DEV), mean.to(DEV), rstd.to(DEV)
    arm.dead(dxd, ~MROWS), arm.dead(md, ~MROWS), arm.dead(rd, ~MROWS)
    dpr = torch.full((RP, d), float("nan"), device=DEV)
    prd, gd = pr.to(DEV), gam.to(DEV)

    def single():
        call("lpi_vis_assemble_bwd", dt, RB, G2, RP, d, dxd, prd, 0, gd, md, rd, dpr, stream())

    def collect():
        arm.out(tag + "dx0", dxd, MROWS, in_rows(g, MAPPED), TOL[dt])
        arm.out(tag + "dprompt", dpr, None, g.view(RB, RP, d).sum(0), TOL[dt])
    return single, None, collect


def piece_prompt_add(arm, d, xdt, tag=""):
    x = rnd(RMP, d, seed=18).to(TD[xdt])
    pr = rnd(RP, d, seed=19)
    want = (x[MAPPED].float() + pr.repeat(RB, 1)).to(TD[xdt])      # test_fp16_residual_stream_kernels: the f32 sum, stored — equality
    m, r = row_stats(want.double())
    xd = arm.dead(x.to(DEV), ~MROWS)
    om, orr = arm.preserve(tag + "out_mean", torch.zeros(RMP, device=DEV), ~MROWS), arm.preserve(tag + "out_rstd", torch.zeros(RMP, device=DEV), ~MROWS)
    prd = pr.to(DEV)

    def single():
        call("lpi_prompt_add", xdt, RB, RL, RP, d, xd, prd, 0, om, orr, stream())
    job = _lib.row_job(_lib.ROWOP_PROMPT_ADD, B=RB, L=RL, P=RP, d=d, dt_a=xdt, out=xd, a=prd, bstride=0, mean=om, rstd=orr)

    def collect():
        arm.out(tag + "x", xd, MROWS, in_rows(want, MAPPED), 0)
        # test_row_kernels_leave_the_layernorm_statistics_of_the_rows_they_write: close() — 2e-6 of max(1, |mean|), rstd to 2e-6 relative
        arm.out(tag + "out_mean", om, MROWS, in_rows(m, MAPPED), 2e-6, err=lambda a, b: abs_err(a, b) / max(1.0, float(b.abs().max())))
        arm.out(tag + "out_rstd", orr, MROWS, in_rows(r, MAPPED), 2e-6, err=ratio_err)
    return single, job, collect


def piece_pool_ln_fwd(arm, d, dt, xdt, tag=""):
    x = (rnd(RMP, d, seed=20) * 3 + 0.5).to(TD[xdt])
    gam, bet = 1 + 0.1 * rnd(d, seed=21), 0.05 * rnd(d, seed=22)
    xp = x[POOLROWS].double()
    ref = torch.nn.functional.layer_norm(xp, (d,), gam.double(), bet.double(), 1e-5)
    m, r = row_stats(xp)
    xd = arm.dead(x.to(DEV), ~PROWS)
    y = torch.full((RB, d), float("nan"), device=DEV, dtype=TD[dt])
    raw = torch.full((RB, d), float("nan"), device=DEV)
    st = torch.zeros(2, RB, device=DEV)
    idx, gd, bd = torch.tensor(IDX, dtype=torch.int32, device=DEV), gam.to(DEV), bet.to(DEV)

    def single():
        call("lpi_pool_ln_fwd", dt, xdt, RB, RL, d, xd, idx, gd, bd, y, d, st[0], st[1], stream())
        call("lpi_gather_rows", xdt, RB, RL, d, xd, idx, raw, stream())
    job = _lib.row_job(_lib.ROWOP_POOL_LN_FWD, B=RB, L=RL, d=d, dt_a=xdt, dt_b=dt, a=xd, idx=idx, gamma=gd, beta=bd, out=y, ld_c=d, mean=st[0], rstd=st[1], out2=raw)

    def collect():
        # F32: test_attention_pooled_varlen_and_absolute_row_index (2e-5); BF16 over the fp16 stream: test_fp16_residual_stream_kernels (8e-3, statistics 1e-5);
        # F16: test_layernorm_f16_output_and_pooled_attention_f16 (2e-3)
        arm.out(tag + "y", y, None, ref, {F32: 2e-5, BF16: 8e-3, F16: 2e-3}[dt])
        arm.out(tag + "mean", st[0], None, m.double(), 1e-5)
        arm.out(tag + "rstd", st[1], None, r.double(), 1e-5)
        arm.out(tag + "gathered rows", raw, None, xp, 0)      # test_fp16_residual_stream_kernels: equality
    return single, job, collect


def piece_pool_ln_bwd(arm, d, cast_dt, tag=""):
    x = rnd(RMP, d, seed=23) * 2 + 0.3
    gam = 1 + 0.1 * rnd(d, seed=24)
    dy = rnd(RB, d, seed=25)
    xp = x[POOLROWS].double()
    m, r = row_stats(xp)
    ref = in_rows(ln_bwd_ref(xp, gam, dy.double()), POOLROWS)
    xd = arm.dead(x.to(DEV), ~PROWS)
    dx = arm.preserve(tag + "dx", torch.zeros(RMP, d, device=DEV), ~PROWS)
    cast = arm.preserve(tag + "dx_cast", torch.zeros(RMP, d, device=DEV, dtype=TD[cast_dt]), ~PROWS)
    idx, gd, dyd, md, rd = torch.tensor(IDX, dtype=torch.int32, device=DEV), gam.to(DEV), dy.to(DEV), m.to(DEV), r.to(DEV)

    def single():
        call("lpi_pool_ln_bwd", cast_dt, RB, RL, d, dyd, d, xd, idx, gd, md, rd, dx, cast, stream())
    job = _lib.row_job(_lib.ROWOP_POOL_LN_BWD, B=RB, L=RL, d=d, dt_b=cast_dt, a=dyd, ld_a=d, b=xd, idx=idx, gamma=gd, mean_in=md, rstd_in=rd, out=dx, out2=cast)

    def collect():      # test_layernorm_fwd_bwd: the f32 gradient to 2e-5, its cast copy to TOL
        arm.out(tag + "dx", dx, PROWS, ref, 2e-5)
        arm.out(tag + "dx_cast", cast, PROWS, ref, TOL[cast_dt])
    return single, job, collect


def piece_scatter_rows(arm, d, cast_dt, tag=""):
    src = rnd(RB, d, seed=26)
    dst = arm.preserve(tag + "dst", torch.zeros(RMP, d, device=DEV), ~PROWS)
    cast = arm.preserve(tag + "dst_cast", torch.zeros(RMP, d, device=DEV, dtype=TD[cast_dt]), ~PROWS)
    # the scatter has no dead input of its own: the source rows of the gather beside it are the poisoned region of this piece
    g_src = rnd(RMP, d, seed=27).half()
    gd = arm.dead(g_src.to(DEV), ~PROWS)
    got = torch.full((RB, d), float("nan"), device=DEV)
    idx, sd = torch.tensor(IDX, dtype=torch.int32, device=DEV), src.to(DEV)

    def single():
        call("lpi_scatter_rows", cast_dt, RB, RL, d, sd, idx, dst, cast, stream())
        call("lpi_gather_rows", F16, RB, RL, d, gd, idx, got, stream())

    def collect():
        arm.out(tag + "dst", dst, PROWS, in_rows(src, POOLROWS), 0)
        arm.out(tag + "dst_cast", cast, PROWS, in_rows(src, POOLROWS), 0 if cast_dt == F32 else 8e-3)      # test_scatter_add_rows: bf16 rounding, 8e-3
        arm.out(tag + "gathered", got, None, g_src[POOLROWS].double(), 0)
    return single, None, collect


def piece_scatter_add_rows(arm, d, dt, tag=""):
    dst0 = rnd(RMP, d, seed=31).to(TD[dt])
    src = rnd(RB, d, seed=32).to(TD[dt])
    dst = arm.preserve(tag + "dst", dst0.to(DEV), ~PROWS)
    g_src = rnd(RMP, d, seed=33)
    gd = arm.dead(g_src.to(DEV), ~PROWS)                     # (as in piece_scatter_rows: the f32 gather's source rows carry the poison)
    got = torch.full((RB, d), float("nan"), device=DEV)
    idx, sd = torch.tensor(IDX, dtype=torch.int32, device=DEV), src.to(DEV)

    def single():
        call("lpi_scatter_add_rows", dt, RB, RL, d, sd, d, idx, dst, d, stream())
        call("lpi_gather_rows", F32, RB, RL, d, gd, idx, got, stream())
    job = _lib.row_job(_lib.ROWOP_SCATTER_ADD, B=RB, L=RL, d=d, dt_a=dt, a=sd, ld_a=d, idx=idx, out=dst, ld_c=d)

    def collect():      # test_scatter_add_rows: 1e-6 / 8e-3
        arm.out(tag + "dst", dst, PROWS, in_rows(dst0[POOLROWS].double() + src.double(), POOLROWS), 1e-6 if dt == F32 else 8e-3)
        arm.out(tag + "gathered", got, None, g_src[POOLROWS].double(), 0)
    return single, job, collect


# every (dy, cast, x, f32 stream kept) combination ln_bwd_impl dispatches (csrc/rowops.hip): the 16-byte half-wave kernel needs dx == NULL
LN_BWD_COMBOS = [(BF16, BF16, F16, False), (BF16, BF16, F16, True), (F32, F32, F32, True), (F32, BF16, F32, True), (BF16, BF16, F32, True), (BF16, F32, F32, True)]


@pytest.mark.parametrize("d", ROW_D)
@pytest.mark.parametrize("dy_dt,cast_dt,x_dt,with_dx", LN_BWD_COMBOS)
def test_layernorm_bwd_rows_touches_the_mapped_rows_only(d, dy_dt, cast_dt, x_dt, with_dx):
    def case(arm):
        single, _, collect = piece_ln_bwd_rows(arm, d, dy_dt, cast_dt, x_dt, with_dx)
        single()
        collect()
    run(case, f"layernorm_bwd_rows dy={NAME[dy_dt]} cast={NAME[cast_dt]} x={NAME[x_dt]} dx={'f32' if with_dx else 'NULL'} d={d}")


ROW_PIECES = {
    "gather_batch_rows f32": (piece_gather_batch_rows, F32), "gather_batch_rows bf16": (piece_gather_batch_rows, BF16),
    "rows_sum_over_batch f32": (piece_rows_sum, F32), "rows_sum_over_batch bf16": (piece_rows_sum, BF16),      # the header: dx is f32 or bf16
    "vis_assemble_bwd f32": (piece_vis_assemble_bwd, F32), "vis_assemble_bwd bf16": (piece_vis_assemble_bwd, BF16),      # dx0 is f32, or the bf16 gradient stream
    "prompt_add f32": (piece_prompt_add, F32), "prompt_add f16": (piece_prompt_add, F16),      # x_dtype: f32 or the fp16 stream
    "pool_ln_fwd f32<-f32 + gather_rows": (piece_pool_ln_fwd, F32, F32), "pool_ln_fwd bf16<-f16 + gather_rows": (piece_pool_ln_fwd, BF16, F16),
    "pool_ln_fwd f16<-f16 + gather_rows": (piece_pool_ln_fwd, F16, F16),
    "pool_ln_bwd cast f32": (piece_pool_ln_bwd, F32), "pool_ln_bwd cast bf16": (piece_pool_ln_bwd, BF16),
    "scatter_rows cast f32 + gather_rows": (piece_scatter_rows, F32), "scatter_rows cast bf16 + gather_rows": (piece_scatter_rows, BF16),
    "scatter_add_rows f32 + gather_rows": (piece_scatter_add_rows, F32), "scatter_add_rows bf16 + gather_rows": (piece_scatter_add_rows, BF16),
}


@pytest.mark.parametrize("d", ROW_D)
@pytest.mark.parametrize("name", list(ROW_PIECES))
def test_row_kernels_touch_the_mapped_rows_only(d, name):
    fn, *types = ROW_PIECES[name]

    def case(arm):
        single, _, collect = fn(arm, d, *types)
        single()
        collect()
    run(case, f"{name} d={d}")


@pytest.mark.parametrize("d", ROW_D)
def test_one_row_jobs_launch_of_four_gives_the_same_verdicts(d):
    """LN_BWD_ROWS_H16, GATHER_BATCH_ROWS, PROMPT_ADD and POOL_LN_FWD (with the gathered row) as ONE lpi_row_jobs launch."""
    def case(arm):
        pieces = [piece_ln_bwd_rows(arm, d, BF16, BF16, F16, False, "ln_bwd_rows_h16 "), piece_gather_batch_rows(arm, d, BF16, "gather_batch_rows "),
                  piece_prompt_add(arm, d, F16, "prompt_add "), piece_pool_ln_fwd(arm, d, BF16, F16, "pool_ln_fwd ")]
        n0 = _lib.launch_count()
        _lib.row_jobs([p[1] for p in pieces], stream())
        assert _lib.launch_count() == n0 + 1
        for p in pieces:
            p[2]()
    run(case, f"row_jobs x4 d={d}")


# ------------------------------------------------------------------------------------------------ text front end
@pytest.mark.parametrize("xdt", [F32, F16])      # x_dtype: f32 or the fp16 stream (txt_embed_launch refuses anything else)
def test_text_embedding_reads_no_token_behind_a_caption(xdt):
    """lpi_txt_embed_fwd_varlen: ids stays the padded [B, L] matrix; ids[b, l >= L_b] are not embedded — arm B holds ANOTHER token id there, in range."""
    B, Lmax, Pn, d, V = 4, 59, 4, 128, 50
    lens = torch.tensor(RAGGED)
    rs = torch.cat([torch.zeros(1, dtype=torch.long), lens.cumsum(0)])
    M = int(rs[-1])
    Mp = pad256(M)
    ids = torch.randint(0, V, (B, Lmax), generator=torch.Generator().manual_seed(7))
    tok, pos, ctx = rnd(V, d, seed=8), rnd(Lmax, d, seed=9), rnd(Pn, d, seed=10)
    dead = torch.arange(Lmax)[None, :] >= lens[:, None]
    want = torch.zeros(Mp, d)
    for b in range(B):
        for l_ in range(int(lens[b])):
            want[int(rs[b]) + l_] = (ctx[l_ - 1] if 1 <= l_ <= Pn else tok[ids[b, l_]]) + pos[l_]
    want = want.to(TD[xdt])
    m, r = row_stats(want[:M].double())
    live = torch.arange(Mp) < M

    def case(arm):
        idd = arm.dead_index(ids.to(DEV), dead, V)
        x0 = arm.preserve("x0", torch.zeros(Mp, d, device=DEV, dtype=TD[xdt]), ~live)
        om, orr = arm.preserve("out_mean", torch.zeros(Mp, device=DEV), ~live), arm.preserve("out_rstd", torch.zeros(Mp, device=DEV), ~live)
        call("lpi_txt_embed_fwd_varlen", xdt, B, Lmax, rs.int().to(DEV), Pn, d, idd, tok.to(DEV), pos.to(DEV), ctx.to(DEV), 0, x0, om, orr, stream())
        arm.out("x0", x0, live, want.double(), 0)      # test_row_kernels_varlen: equality with the f32 sum as stored
        arm.out("out_mean", om, live, padded(m.double(), Mp), 2e-6, err=lambda a, b: abs_err(a, b) / max(1.0, float(b.abs().max())))
        arm.out("out_rstd", orr, live, padded(r.double(), Mp) + (~live).double(), 2e-6, err=ratio_err)

    assert run(case, f"txt_embed_fwd_varlen x={NAME[xdt]} lengths {RAGGED}") == int(dead.sum())


# ------------------------------------------------------------------------------------------------ losses and retrieval
LN_, LPAD = 130, 256      # logits with n = 130 inside a [256, 256] buffer


def _logits():
    lg = torch.zeros(LPAD, LPAD)
    lg[:LN_, :LN_] = rnd(LN_, LN_, seed=41) * 3
    dead = torch.ones(LPAD, LPAD, dtype=torch.bool)
    dead[:LN_, :LN_] = False
    return lg, dead


def test_clip_loss_local_reads_inside_n_and_writes_inside_its_block():
    """lpi_clip_loss_local with r0 = 64, nloc = 5: rows and columns >= n of the logits are dead; columns >= n and rows >= nloc of g / gt are preserved
    (engine.clip_loss_fwd_bwd feeds them to a padded GEMM and relies on them staying zero).  Bars: test_clip_loss (loss 1e-5, gradients 5e-5)."""
    r0, nloc = 64, 5
    lg, dead = _logits()
    l64 = lg[:LN_, :LN_].double().requires_grad_(True)
    lab = torch.arange(LN_)
    ref = (torch.nn.functional.cross_entropy(l64, lab) + torch.nn.functional.cross_entropy(l64.t(), lab)) / 2
    ref.backward()
    G = l64.grad
    block = torch.zeros(LPAD, LPAD, dtype=torch.bool)
    block[:nloc, :LN_] = True
    gref, gtref = torch.zeros(LPAD, LPAD, dtype=torch.float64), torch.zeros(LPAD, LPAD, dtype=torch.float64)
    gref[:nloc, :LN_], gtref[:nloc, :LN_] = G[r0:r0 + nloc], G[:, r0:r0 + nloc].t()
    inside = torch.arange(LPAD) < LN_

    def case(arm):
        lgd = arm.dead(lg.to(DEV), dead)
        g, gt = arm.preserve("g", torch.zeros(LPAD, LPAD, device=DEV), ~block), arm.preserve("gt", torch.zeros(LPAD, LPAD, device=DEV), ~block)
        loss, lse = torch.zeros(1, device=DEV), torch.zeros(2, LPAD, device=DEV)
        call("lpi_clip_loss_local", LN_, lgd, LPAD, 1.0, r0, nloc, loss, lse[0], lse[1], g, gt, LPAD, stream())
        arm.out("loss", loss, None, ref.detach().reshape(1), 1e-5, err=lambda a, b: abs_err(a, b) / max(1.0, float(b.abs().max())))
        arm.out("row_lse", lse[0], inside), arm.out("col_lse", lse[1], inside)
        arm.out("g", g, block, gref, 5e-5), arm.out("gt", gt, block, gtref, 5e-5)

    run(case, "clip_loss_local n=130 in [256, 256] r0=64 nloc=5")


def test_ce_rows_reads_inside_n_and_writes_inside_its_block():
    """lpi_ce_rows_fwd_bwd with rows = 5, label0 = 64.  Bars: test_clip_loss_modes_of_gather_features (loss 2e-5, gradients 2e-4)."""
    rows, label0, up = 5, 64, 0.1
    lg, _ = _logits()
    dead = torch.ones(LPAD, LPAD, dtype=torch.bool)
    dead[:rows, :LN_] = False
    l64 = lg[:rows, :LN_].double()
    lab = torch.arange(rows) + label0
    lref = torch.logsumexp(l64, 1) - l64[torch.arange(rows), lab]
    dref = torch.zeros(LPAD, LPAD, dtype=torch.float64)
    dref[:rows, :LN_] = up * (torch.softmax(l64, 1) - torch.nn.functional.one_hot(lab, LN_).double())

    def case(arm):
        lgd = arm.dead(lg.to(DEV), dead)
        dl = arm.preserve("dlogits", torch.zeros(LPAD, LPAD, device=DEV), dead)
        lr = torch.zeros(rows, device=DEV)
        call("lpi_ce_rows_fwd_bwd", rows, LN_, lgd, LPAD, label0, up, lr, dl, LPAD, stream())
        arm.out("loss_rows", lr, None, lref, 2e-5)
        arm.out("dlogits", dl, ~dead, dref, 2e-4)

    run(case, "ce_rows_fwd_bwd n=130 in [256, 256] rows=5 label0=64")


def test_retrieval_rank_topk_and_task_id_read_no_gap_column():
    """lpi_retrieval_rank and lpi_topk with ld = n_cols + 5, lpi_l1_task_id with ldf = E + 4: the gap columns are dead.  References and bars:
    test_retrieval_rank_and_topk (equality with numpy's stable argsort), test_l1_task_id_kernel (distances to 1e-3)."""
    n_img, n_txt = 37, 91
    ld = n_txt + 5
    s = torch.zeros(n_img, ld)
    s[:, :n_txt] = rnd(n_img, n_txt, seed=3)
    s[3, 10] = s[3, 20]
    gap = torch.zeros(n_img, ld, dtype=torch.bool)
    gap[:, n_txt:] = True
    gt = torch.stack([torch.arange(n_img) * 2, torch.arange(n_img) * 2 + 1], 1).int()
    order = [np.argsort(s[i, :n_txt].numpy(), kind="stable")[::-1] for i in range(n_img)]
    rank_ref = torch.tensor([min(int(np.where(order[i] == j)[0][0]) for j in gt[i].tolist()) for i in range(n_img)])
    idx_ref = torch.from_numpy(np.stack([o[:5] for o in order]).copy())
    n, E_, T, C = 37, 128, 4, 5
    ldf = E_ + 4
    f = torch.zeros(n, ldf)
    f[:, :E_] = rnd(n, E_, seed=5)
    fgap = torch.zeros(n, ldf, dtype=torch.bool)
    fgap[:, E_:] = True
    keys = rnd(T, C, E_, seed=6)
    keys[2, 1] = f[3, :E_]
    dist_ref = torch.stack([torch.stack([(f[:, :E_].double() - c.double()).abs().sum(1) for c in keys[t]]).min(0)[0] for t in range(T)]).t()

    def case(arm):
        sd = arm.dead(s.to(DEV), gap)
        rank = torch.zeros(n_img, dtype=torch.int32, device=DEV)
        call("lpi_retrieval_rank", n_img, n_txt, sd, ld, gt.to(DEV), 2, rank, stream())
        idx, val = torch.zeros(n_img, 5, dtype=torch.int32, device=DEV), torch.zeros(n_img, 5, device=DEV)
        call("lpi_topk", n_img, n_txt, 5, sd, ld, idx, val, stream())
        arm.out("rank", rank, None, rank_ref, 0), arm.out("topk idx", idx, None, idx_ref, 0)
        arm.out("topk val", val, None, torch.gather(s.double(), 1, idx_ref.long()), 0)
        fd = arm.dead(f.to(DEV), fgap)
        sel, dist = torch.zeros(n, dtype=torch.int32, device=DEV), torch.zeros(n, T, device=DEV)
        call("lpi_l1_task_id", n, E_, T, C, fd, ldf, keys.to(DEV), sel, dist, stream())
        arm.out("task dist", dist, None, dist_ref, 1e-3, err=abs_err)
        arm.out("task sel", sel)

    assert run(case, "retrieval_rank / topk ld=n_cols+5, l1_task_id ldf=E+4") == n_img * 5 + n * 4


# ------------------------------------------------------------------------------------------------ the engine's own claim
# How Tower.workspace's buffers are poisoned behind the bound batch (M rows, B samples, L tokens; shapes are those of the ARENA, which was allocated for
# the larger batch).  Every tensor of an arena must appear in exactly one group: a buffer added to the arena has to be classified here.
ARENA_MP_ROWS = ["x", "xmid", "qkv", "ctx", "u", "h", "g", "dx", "dh", "dctx", "dqkv", "dxT"]                                   # [Mp, *]: rows [M, Mp)
ARENA_BP_ROWS = ["c_xmid", "c_h", "c_g", "c_u", "c_xout", "c_q", "c_ctx", "c_xin", "c_dx", "c_dxT", "c_dh", "c_dctx", "c_dq"]    # [Bp, *]: rows [B, Bp)
ARENA_BP_COLS = ["c_stat", "c_stat1"]                                                                                              # [2, Bp]: entries [B, Bp)
ARENA_FLAT = {      # flat per-sample storage: everything past what the bound batch addresses
    "lse": lambda B, L, H, d, pre: (B + (1 if pre else 0)) * H * L, "delta": lambda B, L, H, d, pre: (B + (1 if pre else 0)) * H * L,
    "c_lse": lambda B, L, H, d, pre: B * H, "sp_lse": lambda B, L, H, d, pre: B * H, "sp_scratch": lambda B, L, H, d, pre: 4 * B * H * d,
    "shared_dkv": lambda B, L, H, d, pre: B * pre * 2 * d,
}
ARENA_PROMPT_ROWS = ["p_dqkv", "p_dh"]      # the first block's packed prompt rows, "up to 32 prompt rows per sample": rows [32 B, end)
ARENA_VIEWS = {"du": "a view of g in the gradient type", "c_du": "a view of c_g in the gradient type", "stat": "views into lnblk's mean / rstd segments"}
ARENA_FRONT = "front"      # the vision front end's own buffers: cols / pe [rows of B G2 patches, *]: rows [B G2, end); stat [2, Mp]: entries [M, Mp)
# no stale region: the bound batch's own row starts / pooled rows (a PackedIds' tensors), and the prompt gradient [Lyr, P, d] (live in every row)
ARENA_NOT_STORAGE = {"rs", "pool_abs", "dprompts"}
# buffers left out by name because the engine itself rewrites the region in every step: none.
ARENA_LEFT_OUT = {}


def _poison_arena(tower, B, M, L, pre, n_patches):
    """NaN behind the bound batch in every buffer of the tower's training arena; returns the number of elements poisoned."""
    (ws,) = [w for (bcap, train), w in tower._ws.items() if train]
    H, d = tower.spec.heads, tower.spec.width
    n = 0
    known = set(ARENA_MP_ROWS) | set(ARENA_BP_ROWS) | set(ARENA_BP_COLS) | set(ARENA_FLAT) | set(ARENA_PROMPT_ROWS) | set(ARENA_VIEWS) | ARENA_NOT_STORAGE | \
        set(ARENA_LEFT_OUT) | {"rstat", "lnblk", ARENA_FRONT}
    for key, val in ws.items():
        tensors = [t for t in (val if isinstance(val, (list, tuple)) else val.values() if isinstance(val, dict) else [val]) if torch.is_tensor(t) or isinstance(t, tuple)]
        if not tensors:
            continue
        assert key in known, f"arena buffer {key!r} is not classified (tests/test_dead_memory_gpu.py: ARENA_*)"
        if key == ARENA_FRONT:
            assert set(val) == {"cols", "pe", "stat"}, sorted(val)
            patches = B * n_patches
            n += P.fill_nan(val["cols"], torch.arange(val["cols"].shape[0]) >= patches) + P.fill_nan(val["pe"], torch.arange(val["pe"].shape[0]) >= patches)
            n += P.fill_nan(val["stat"][:, M:])
            continue
        for t in tensors:
            if key in ARENA_MP_ROWS:
                n += P.fill_nan(t, torch.arange(t.shape[0]) >= M)
            elif key in ARENA_BP_ROWS:
                n += P.fill_nan(t, torch.arange(t.shape[0]) >= B)
            elif key in ARENA_PROMPT_ROWS:
                n += P.fill_nan(t, torch.arange(t.shape[0]) >= 32 * B)
            elif key in ARENA_BP_COLS:
                n += P.fill_nan(t[:, B:])
            elif key == "rstat":
                n += P.fill_nan(t[:, M:])
            elif key == "lnblk":      # mean[Mp] | rstd[Mp] | c1 ...: the statistics behind the batch, never the c1 tail
                Mp = (t.shape[1] - 4 * d) // 3
                n += P.fill_nan(t[:, M:Mp]) + P.fill_nan(t[:, Mp + M:2 * Mp])
            elif key in ARENA_FLAT:
                n += P.fill_nan(t.view(-1)[ARENA_FLAT[key](B, L, H, d, pre):]) if t.numel() > ARENA_FLAT[key](B, L, H, d, pre) else 0
    return n


@pytest.mark.parametrize("dtype", ["f32", "bf16", "f16"])
def test_a_smaller_batch_reads_nothing_stale_from_the_arena_of_a_larger_one(dtype):
    """Tower.workspace: "rows past the bound batch ... no kernel reads into a live row".  A 4-sample step, NaN in everything the engine calls stale for the
    3-sample batch that follows, the 3-sample step: every output and factor gradient bit for bit those of the same sequence without poison and of a fresh
    encoder."""
    from lpi_amd.engine import DualEncoder
    from lpi_amd.step import train_step
    cfg = synth.TINY
    ids = synth.token_ids(4)

    def step(enc, n):
        fac = {k: torch.from_numpy(v).to(DEV).requires_grad_(True) for k, v in synth.prompt_factors(9, 16, cfg.vision_width, cfg.transformer_width).items()}
        img = torch.from_numpy(synth.images(4, cfg.image_resolution)[:n].copy()).to(DEV)
        out = train_step(enc, img, torch.from_numpy(ids[:n].copy()).to(DEV), fac, 2)
        torch.cuda.synchronize()
        res = {k: v.detach().clone() for k, v in out.items() if torch.is_tensor(v)}
        res.update({"grad." + k: fac[k].grad.clone() for k in synth.PROMPT_NAMES})
        return res

    def make():
        return DualEncoder(cfg, synth.clip_state_dict(cfg), dtype=dtype, device=DEV)

    plain = make()
    step(plain, 4)
    want = step(plain, 3)
    bound = {}
    for name, tower in (("vis", plain.vis), ("txt", plain.txt)):
        (ws,) = [w for (bcap, train), w in tower._ws.items() if train]
        assert ws["B"] == 3 and ws["x"][0].shape[0] >= 4 * ws["L"]      # the 3-sample batch ran in the 4-sample arena
        bound[name] = (ws["B"], ws["M"], ws["L"], ws.get("pre", 0))
    enc = make()
    step(enc, 4)
    n = sum(_poison_arena(tower, *bound[name], cfg.n_patches) for name, tower in (("vis", enc.vis), ("txt", enc.txt)))
    print(f"POISON engine {dtype}: {n} stale arena elements poisoned (bound batches: {bound})")
    assert n > 0
    got = step(enc, 3)
    fresh = step(make(), 3)
    assert want.keys() == got.keys() == fresh.keys() and any(k.startswith("grad.") for k in got)
    for k in want:
        assert not bool(torch.isnan(want[k].float()).any()), k
        assert P.same_bits(got[k], want[k]), f"{k}: the 3-sample step read stale arena memory into a live value"
        assert P.same_bits(got[k], fresh[k]), f"{k}: differs from a fresh encoder"
