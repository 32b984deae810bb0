"""CPU restatement of the split-bf16 ("bf16x3") GEMM arithmetic of LPI_F32X3 (include/lpi_hip.h) in torch: what every GPU test of
the bf16x3 kernels is held to.

An f32 operand element x becomes hi = RNE_bf16(x) and lo = RNE_bf16(x - float(hi)); the subtraction is exact in f32 (hi agrees with x in its leading 8
bits).  torch's float32 -> bfloat16 cast rounds to nearest even, as v_cvt_pk_bf16_f32 does.  A product a.b is hi_a hi_b + hi_a lo_b + lo_a hi_b; lo_a lo_b
is dropped.  The emulator sums the three terms in f64, so it carries the operand error of the format and no accumulation error."""
import torch


def split(x: torch.Tensor):
    """x (f32) -> (hi, lo) as bfloat16 tensors of the same shape."""
    x = x.detach().to("cpu", torch.float32)
    hi = x.to(torch.bfloat16)
    lo = (x - hi.to(torch.float32)).to(torch.bfloat16)
    return hi, lo


def gemm_x3(a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    """a [M, K], b [N, K] (f32) -> hi_a hi_b^T + hi_a lo_b^T + lo_a hi_b^T in f64 ([M, N])."""
    ah, al = (t.double() for t in split(a))
    bh, bl = (t.double() for t in split(b))
    return ah @ bh.t() + ah @ bl.t() + al @ bh.t()


def abs_product(a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    """(|A| |B|^T) in f64: the scale of the elementwise error bounds."""
    return a.detach().cpu().double().abs() @ b.detach().cpu().double().abs().t()


def rows(n: int, K: int, seed: int, outlier: bool = True) -> torch.Tensor:
    """Seeded Gaussian rows with a per-row log-normal gain and (outlier) one x40 channel: the generator of the accuracy tests."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n, K, generator=g) * torch.exp(torch.randn(n, 1, generator=g))
    if outlier:
        x[:, 5 % K] *= 40.0
    return x


def integer_operands(M: int, N: int, K: int, seed: int, swap: bool = False, narrow_max: int = 0):
    """Integer operands on which bf16x3 is EXACT and every partial sum of any summation order is an integer below 2^24: |a| < 2^16 (hi + lo holds 16
    significant bits: lo is exact), |b| <= narrow_max <= 2^8 (b = hi, lo = 0), so the dropped lo.lo term is zero; magnitudes are drawn so that
    sum_k |a||b| < 2^24 (narrow_max = 0: the largest value up to 2^8 that leaves a 11 bits or more; a small one leaves room for the full 16 bits).  Rows are distinct.  swap: the wide operand is b.  -> (a, b) f32."""
    g = torch.Generator().manual_seed(seed)
    if narrow_max <= 0:
        narrow_max = max(1, min(256, (2 ** 24 - 1) // (K * 2048)))
    wide_max = min(65535, (2 ** 24 - 1) // (K * narrow_max))
    wide = torch.randint(-wide_max, wide_max + 1, (M if not swap else N, K), generator=g).float()
    narrow = torch.randint(-narrow_max, narrow_max + 1, (N if not swap else M, K), generator=g).float()
    wide[:, 0] = (torch.arange(wide.shape[0]) % 251 - 125).float()
    narrow[:, 1 % K] = (torch.arange(narrow.shape[0]) % (2 * narrow_max - 1) - narrow_max + 1).float().clamp(-120, 120)
    a, b = (narrow, wide) if swap else (wide, narrow)
    assert float(abs_product(a, b).max()) < 2 ** 24
    return a, b
