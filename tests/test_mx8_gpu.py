"""MX-FP8 kernels on a real MI355X (csrc/gemm_mx8.hip, csrc/mx8_rows.hip) against the CPU restatement of the format (tests/mx8_emulate.py):
the quantiser bit for bit; the GEMM bit for bit on integer data whose f32 sums are exact in any order (this is the test of the operand lane map, the
scale bytes and the C write), and on quantised Gaussian operands against the f64 product of the DEQUANTISED operands; the epilogues; LayerNorm -> MX;
the rejections."""
import pytest
import torch

pytestmark = pytest.mark.gpu

import mx8_emulate as MX  # noqa: E402
from lpi_amd import _lib  # noqa: E402
from lpi_amd._lib import BF16, F16, F32, MX8, call  # noqa: E402
from lpi_amd.engine import EPI_NONE, EPI_QUICKGELU, mx8_quantize  # noqa: E402

DEV = "cuda:0"
SHAPES = [(128, 128, 128), (128, 256, 256), (256, 384, 768), (384, 128, 3072)]
# GEMM on random quantised operands against the f64 product of the dequantised operands, max |got - ref| / max |ref|.  Measured on MI355X over SHAPES:
# 1.75e-5, 2.15e-5, 1.48e-5, 1.42e-5 — not f32 round-off (1e-7): the matrix pipe aligns the scaled products of an instruction to a common exponent before
# it adds them (about 2^-16 of the largest), while integer data stays exact (test_gemm_exact).  Bar = 4 x the measured maximum (the cap is 1e-3).
RANDOM_BAR = 8.6e-5
BF16_BAR = 2e-2      # tests/test_kernels_gpu.py


def relerr(got, ref):
    got, ref = got.double().cpu(), ref.double().cpu()
    return float((got - ref).abs().max() / (ref.abs().max() + 1e-30))


def stream():
    return torch.cuda.current_stream().cuda_stream


def rnd(*shape, seed=0, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale


def gemm_mx8(cdt, a, as_, b, bs, c, cs=None, bias=None, residual=None, epi=EPI_NONE, alpha=1.0):
    M, K = a.shape
    N = b.shape[0]
    call("lpi_gemm_nt_mx8", cdt, M, N, K, a, a.stride(0), as_, as_.stride(0), b, b.stride(0), bs, bs.stride(0), c, c.stride(0), cs,
         cs.stride(0) if cs is not None else 0, bias, residual, residual.stride(0) if residual is not None else 0, epi, float(alpha), stream())


def special_rows(rows, K, seed):
    """Gaussian rows with a per-row gain, and: an x40 outlier channel, an all-zero block, a block of subnormal-range values, blocks whose maximum sits just
    above / exactly at 448 2^e (the bump-by-one branch and its edge)."""
    x = rnd(rows, K, seed=seed) * torch.exp(rnd(rows, 1, seed=seed + 1))
    x[:, 5] *= 40.0
    x[3, 64:96] = 0.0
    x[7, 32:64] = rnd(32, seed=seed + 2) * 2.0 ** -140
    x[9, 0:32] = rnd(32, seed=seed + 3).clamp(-1, 1) * 100.0
    x[9, 4] = 449.0
    x[10, 0:32] = x[9, 0:32]
    x[10, 4] = 448.0
    x[11, 32:64] = x[9, 0:32] * 2.0 ** -20
    x[11, 36] = 1.7539062 * 2.0 ** -12      # 449 / 256 scaled: mantissa just above 0.875 * 2
    return x


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("rows,K", [(128, 128), (128, 3072), (384, 768)])
def test_quantize_bit_for_bit(rows, K, dtype):
    x = special_rows(rows, K, seed=rows + K).to(dtype)
    q, s = mx8_quantize(x.to(DEV))
    qr, sr = MX.quantize(x)
    assert torch.equal(s.cpu(), sr)
    assert torch.equal(q.cpu(), qr)


def integer_operands(M, N, K, seed):
    """e4m3 bytes of integers in [-8, 8] and per-block scales from {1, 2, 4} (A) and {1/2, 1, 2} (B): asymmetric, every row and K block different; every
    partial sum is a multiple of 1/2 below 2^22, so f32 accumulation is exact in any order."""
    g = torch.Generator().manual_seed(seed)
    a = torch.randint(-8, 9, (M, K), generator=g).float()
    b = torch.randint(-8, 9, (N, K), generator=g).float()
    a[:, 0] = (torch.arange(M) % 17 - 8).float()      # no two rows alike even by chance
    b[:, 1] = (torch.arange(N) % 13 - 6).float()
    as_ = (127 + torch.randint(0, 3, (M, K // 32), generator=g)).to(torch.uint8)
    bs = (126 + torch.randint(0, 3, (N, K // 32), generator=g)).to(torch.uint8)
    aq, bq = a.to(torch.float8_e4m3fn).view(torch.uint8), b.to(torch.float8_e4m3fn).view(torch.uint8)
    ref = MX.dequantize(aq, as_) @ MX.dequantize(bq, bs).t()
    assert float(ref.abs().max()) < 2 ** 22
    return aq, as_, bq, bs, ref


@pytest.mark.parametrize("M,N,K", SHAPES)
def test_gemm_exact(M, N, K):
    aq, as_, bq, bs, ref = integer_operands(M, N, K, seed=K)
    c = torch.full((M, N), -1.0, device=DEV)
    n0 = _lib.launch_count()
    gemm_mx8(F32, aq.to(DEV), as_.to(DEV), bq.to(DEV), bs.to(DEV), c)
    assert _lib.launch_count() == n0 + 1 and _lib.load().lpi_gemm_last_kernel() == _lib.GEMM_K_MX8
    assert torch.equal(c.cpu().double(), ref)


def random_operands(M, N, K, seed, bscale=1.0):
    a, b = rnd(M, K, seed=seed) * torch.exp(rnd(M, 1, seed=seed + 1)), rnd(N, K, seed=seed + 2, scale=bscale)
    aq, as_ = MX.quantize(a)
    bq, bs = MX.quantize(b)
    return aq, as_, bq, bs, MX.dequantize(aq, as_) @ MX.dequantize(bq, bs).t()


@pytest.mark.parametrize("M,N,K", SHAPES)
def test_gemm_random(M, N, K):
    aq, as_, bq, bs, ref = random_operands(M, N, K, seed=K + 1)
    c = torch.zeros(M, N, device=DEV)
    gemm_mx8(F32, aq.to(DEV), as_.to(DEV), bq.to(DEV), bs.to(DEV), c)
    err = relerr(c, ref)
    print(f"mx8 gemm random ({M},{N},{K}): relerr {err:.3e}")
    assert err < RANDOM_BAR


def test_gemm_epilogues():
    M, N, K = 256, 384, 768
    aq, as_, bq, bs, prod = random_operands(M, N, K, seed=5, bscale=0.05)
    bias, res = rnd(N, seed=6), rnd(M, N, seed=7)
    dev = [t.to(DEV) for t in (aq, as_, bq, bs)]
    # bias + alpha (f32 out), and an f32 residual
    c = torch.zeros(M, N, device=DEV)
    gemm_mx8(F32, *dev, c, bias=bias.to(DEV), alpha=0.5)
    assert relerr(c, 0.5 * prod + bias.double()) < RANDOM_BAR
    gemm_mx8(F32, *dev, c, bias=bias.to(DEV), residual=res.to(DEV))
    assert relerr(c, prod + bias.double() + res.double()) < RANDOM_BAR
    # fp16 residual with fp16 output (the residual stream); bf16 output (qkv)
    r16 = res.half()
    c16 = torch.zeros(M, N, device=DEV, dtype=torch.float16)
    gemm_mx8(F16, *dev, c16, bias=bias.to(DEV), residual=r16.to(DEV))
    assert relerr(c16, prod + bias.double() + r16.double()) < 2.0 ** -11 + RANDOM_BAR      # fp16 rounding of the stored value: 2^-11 of at most the maximum
    cb = torch.zeros(M, N, device=DEV, dtype=torch.bfloat16)
    gemm_mx8(BF16, *dev, cb, bias=bias.to(DEV))
    assert relerr(cb, prod + bias.double()) < BF16_BAR
    # QuickGELU to bf16
    u = prod + bias.double()
    act = u * torch.sigmoid(1.702 * u)
    gemm_mx8(BF16, *dev, cb, bias=bias.to(DEV), epi=EPI_QUICKGELU)
    assert relerr(cb, act) < BF16_BAR
    # QuickGELU to MX: the element bound against the f64 activation, widened by the f32 bar of the GEMM for u itself (|d act / du| <= 1.1) and by the
    # epilogue's sigmoid (v_exp / v_rcp: 1 ulp each)
    cq = torch.zeros(M, N, device=DEV, dtype=torch.uint8)
    cs = torch.zeros(M, N // 32, device=DEV, dtype=torch.uint8)
    gemm_mx8(MX8, *dev, cq, cs, bias=bias.to(DEV), epi=EPI_QUICKGELU)
    widen = torch.full_like(act, 1.1 * RANDOM_BAR * float(u.abs().max())) + 4e-7 * act.abs()
    assert MX.bound_violations(act, cq, cs, widen=widen) == 0
    assert int((cs.cpu() == 0).sum()) == 0      # every block was written


def test_gemm_mx8_output_exact():
    """LPI_EPI_NONE to MX on the integer data: bytes and scales bitwise against the emulator applied to the exact product."""
    M, N, K = 256, 384, 768
    aq, as_, bq, bs, ref = integer_operands(M, N, K, seed=11)
    cq = torch.zeros(M, N, device=DEV, dtype=torch.uint8)
    cs = torch.zeros(M, N // 32, device=DEV, dtype=torch.uint8)
    gemm_mx8(MX8, aq.to(DEV), as_.to(DEV), bq.to(DEV), bs.to(DEV), cq, cs)
    qr, sr = MX.quantize(ref.float())      # exact: integers / halves below 2^22
    assert torch.equal(cs.cpu(), sr)
    assert torch.equal(cq.cpu(), qr)


@pytest.mark.parametrize("rows,d", [(256, 128), (128, 768)])
def test_layernorm_mx8(rows, d):
    x = (rnd(rows, d, seed=d) * torch.exp(0.5 * rnd(rows, 1, seed=d + 1)) + rnd(rows, 1, seed=d + 2)).half()
    x[::7, 3] *= 40.0      # rows with an x40 outlier
    gamma, beta = 1.0 + 0.2 * rnd(d, seed=3), 0.1 * rnd(d, seed=4)
    q = torch.zeros(rows, d, device=DEV, dtype=torch.uint8)
    s = torch.zeros(rows, d // 32, device=DEV, dtype=torch.uint8)
    mean, rstd = torch.zeros(rows, device=DEV), torch.zeros(rows, device=DEV)
    call("lpi_layernorm_mx8_fwd", F16, rows, d, x.to(DEV), d, gamma.to(DEV), beta.to(DEV), q, d, s, d // 32, mean, rstd, stream())
    xd = x.double()
    mu, var = xd.mean(dim=1, keepdim=True), xd.var(dim=1, unbiased=False, keepdim=True)
    rs = 1.0 / torch.sqrt(var + 1e-5)
    y = (xd - mu) * rs * gamma.double() + beta.double()
    assert relerr(mean, mu[:, 0]) < 1e-5 and relerr(rstd, rs[:, 0]) < 1e-5
    assert MX.bound_violations(y, q, s, widen=2e-6 * y.abs()) == 0
    # mean / rstd are optional
    q2, s2 = torch.zeros_like(q), torch.zeros_like(s)
    call("lpi_layernorm_mx8_fwd", F16, rows, d, x.to(DEV), d, gamma.to(DEV), beta.to(DEV), q2, d, s2, d // 32, None, None, stream())
    assert torch.equal(q2, q) and torch.equal(s2, s)


def test_rejections_launch_nothing():
    lib = _lib.load()
    z = lambda *sh: torch.zeros(*sh, device=DEV, dtype=torch.uint8)  # noqa: E731
    a, as_, b, bs = z(256, 256), z(256, 8), z(256, 256), z(256, 8)
    c = torch.zeros(256, 256, device=DEV)
    st = stream()
    n0 = _lib.launch_count()

    def rc(cdt, M, N, K, A, As, B, Bs, C, Cs):
        p = lambda t: None if t is None else t.data_ptr()  # noqa: E731
        return lib.lpi_gemm_nt_mx8(cdt, M, N, K, p(A), 256, p(As), 8, p(B), 256, p(Bs), 8, p(C), 256, p(Cs), 8, None, None, 0, EPI_NONE, 1.0, st)

    assert rc(F32, 256, 256, 64, a, as_, b, bs, c, None) == -22       # K not a multiple of 128
    assert rc(F32, 100, 256, 256, a, as_, b, bs, c, None) == -22      # M
    assert rc(F32, 256, 200, 256, a, as_, b, bs, c, None) == -22      # N
    assert rc(F32, 256, 256, 256, a, None, b, bs, c, None) == -22     # NULL scales of an MX operand
    assert rc(F32, 256, 256, 256, a, as_, b, None, c, None) == -22
    assert rc(MX8, 256, 256, 256, a, as_, b, bs, z(256, 256), None) == -22      # ... of an MX output
    assert rc(7, 256, 256, 256, a, as_, b, bs, c, None) == -22
    assert lib.lpi_mx8_quantize(F32, 128, 100, c.data_ptr(), 256, a.data_ptr(), 256, as_.data_ptr(), 8, st) == -22
    assert lib.lpi_mx8_quantize(F32, 128, 256, c.data_ptr(), 256, a.data_ptr(), 256, None, 8, st) == -22
    assert lib.lpi_layernorm_mx8_fwd(F16, 128, 100, c.data_ptr(), 256, c.data_ptr(), c.data_ptr(), a.data_ptr(), 256, as_.data_ptr(), 8, None, None, st) == -22
    assert _lib.launch_count() == n0
