"""CPU restatement of the project's MX-FP8 format (include/lpi_hip.h) in torch: what every GPU test of the MX kernels is held to.

Elements are OCP e4m3fn (torch.float8_e4m3fn), rounded to nearest even with subnormals kept; one E8M0 scale byte (2^(byte - 127)) per 32 consecutive
elements of the last dimension.  For a block maximum amax = m 2^x (frexp: m in [0.5, 1)) the scale exponent is e = floor(log2 amax) - 8 = x - 9, raised by
one if amax 2^-e = 512 m > 448, clamped to [-127, 127]; an all-zero block is byte 0.  The elements are y 2^-e (exact) cast to e4m3fn; none saturates."""
import torch

BLOCK = 32
E4M3_MAX = 448.0


def quantize(y: torch.Tensor):
    """y [..., K] (any float type; K a multiple of 32) -> (elements uint8 [..., K] holding e4m3fn bytes, scale bytes uint8 [..., K/32])."""
    y = y.detach().to("cpu", torch.float32)
    K = y.shape[-1]
    assert K % BLOCK == 0
    blk = y.reshape(*y.shape[:-1], K // BLOCK, BLOCK)
    amax = blk.abs().amax(dim=-1)
    m, x = torch.frexp(amax)
    e = x.to(torch.int32) - 9 + (m > 0.875).to(torch.int32)
    e = e.clamp(-127, 127)
    e = torch.where(amax == 0, torch.full_like(e, -127), e)
    scaled = torch.ldexp(blk.double(), (-e).unsqueeze(-1).double()).float()      # y 2^-e: exact in f64, exact in f32 wherever it matters (>= 2^-10)
    assert float(scaled.abs().max()) <= E4M3_MAX
    q = scaled.to(torch.float8_e4m3fn).view(torch.uint8).reshape(y.shape)
    return q, (e + 127).to(torch.uint8)


def dequantize(q: torch.Tensor, s: torch.Tensor) -> torch.Tensor:
    """(element bytes [..., K], scale bytes [..., K/32]) -> f64 values."""
    q, s = q.detach().cpu(), s.detach().cpu()
    v = q.contiguous().view(torch.float8_e4m3fn).to(torch.float32).double()
    sc = torch.ldexp(torch.ones((), dtype=torch.float64), s.to(torch.float64) - 127.0)
    return (v.reshape(*q.shape[:-1], -1, BLOCK) * sc.unsqueeze(-1)).reshape(q.shape)


def scale_values(s: torch.Tensor) -> torch.Tensor:
    """E8M0 bytes -> f64 scale values 2^(byte - 127)."""
    return torch.ldexp(torch.ones((), dtype=torch.float64), s.detach().cpu().to(torch.float64) - 127.0)


def bound_violations(y: torch.Tensor, q: torch.Tensor, s: torch.Tensor, widen=None) -> int:
    """Number of elements outside |deq - y| <= max(2^-4 |y|, 2^-10 S) (+ widen, a tensor like y), S the block's scale."""
    y = y.detach().cpu().double()
    deq = dequantize(q, s)
    S = scale_values(s).unsqueeze(-1).expand(*s.shape, BLOCK).reshape(y.shape)
    bound = torch.maximum(y.abs() * 2.0 ** -4, S * 2.0 ** -10)
    if widen is not None:
        bound = bound + widen.detach().cpu().double()
    return int(((deq - y).abs() > bound).sum())
