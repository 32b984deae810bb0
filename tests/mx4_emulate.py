"""CPU restatement of the project's MX-FP4 format (include/lpi_hip.h) in torch, from the f32 bits: the definition every GPU test of the
MX-FP4 kernels is held to.

Codes are OCP e2m1 nibbles: bit 3 the sign, bits 0..2 the magnitude code of GRID = (0, 0.5, 1, 1.5, 2, 3, 4, 6).  Nibble order: element 2 j of a row is the
LOW nibble of byte j, element 2 j + 1 the high one.  (The probe tools/probe/mx4_map_probe.hip showed on an MI355X that a lane of the block-scaled matrix
instruction holds 32 consecutive K elements in 16 bytes, that nibble positions of the two operands pair with each other, and that a product of two operands
packed alike is the same in either order: the order is the format's choice, and this is it.)  One E8M0 scale byte (2^(byte - 127)) per 32 consecutive
elements of the last dimension: for a block maximum amax with biased f32 exponent Eb, byte = max(Eb - 2, 0), the OCP rule e = floor(log2 amax) - 2; a zero or
subnormal amax gives byte 0.  An element is y 2^(127 - byte) (exact), rounded to nearest even on the grid and saturating at +-6: values in (6, 8) become 6.
The sign is the sign BIT of y (a negative value that rounds to zero is code 8).  Non-finite inputs are out of contract."""
import torch

BLOCK = 32
GRID = (0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0)
LOW_NIBBLE_FIRST = True      # element 2 j in the low nibble of byte j


def scale_bytes(y: torch.Tensor) -> torch.Tensor:
    """y [..., K] f32 -> the E8M0 byte of every 32-block, uint8 [..., K/32], from the bits of the block maximum."""
    blk = y.reshape(*y.shape[:-1], y.shape[-1] // BLOCK, BLOCK)
    eb = (blk.abs().amax(dim=-1).contiguous().view(torch.int32) >> 23) & 0xFF
    return (eb - 2).clamp(min=0).to(torch.uint8)


def encode(v: torch.Tensor, negative: torch.Tensor) -> torch.Tensor:
    """scaled values (f64, |v| < 8) and their sign bits -> e2m1 codes, uint8 of the same shape.  In [0, 2) the grid's step is 0.5, in [2, 4) 1, in [4, 8) 2,
    and an even count of steps is a code with an even mantissa bit: torch.round (ties to even) of the value in steps is the grid's round to nearest even."""
    a = v.abs()
    c = torch.where(a < 2, torch.round(a * 2), torch.where(a < 4, torch.round(a) + 2, (torch.round(a / 2) + 4).clamp(max=7)))
    return c.to(torch.uint8) | (negative.to(torch.uint8) << 3)


def pack(codes: torch.Tensor) -> torch.Tensor:
    """codes uint8 [..., K] (one per element, 0 .. 15) -> bytes uint8 [..., K/2]."""
    lo, hi = (codes[..., 0::2], codes[..., 1::2]) if LOW_NIBBLE_FIRST else (codes[..., 1::2], codes[..., 0::2])
    return (lo | (hi << 4)).contiguous()


def unpack(q: torch.Tensor) -> torch.Tensor:
    """bytes uint8 [..., K/2] -> codes uint8 [..., K]."""
    lo, hi = q & 15, q >> 4
    pair = (lo, hi) if LOW_NIBBLE_FIRST else (hi, lo)
    return torch.stack(pair, dim=-1).reshape(*q.shape[:-1], 2 * q.shape[-1])


def quantize(y: torch.Tensor):
    """y [..., K] (any float type; K a multiple of 32) -> (code bytes uint8 [..., K/2], scale bytes uint8 [..., K/32])."""
    y = y.detach().to("cpu", torch.float32).contiguous()
    K = y.shape[-1]
    assert K % BLOCK == 0
    s = scale_bytes(y)
    blk = y.reshape(*y.shape[:-1], K // BLOCK, BLOCK)
    scaled = torch.ldexp(blk.double(), (127 - s.to(torch.int32)).unsqueeze(-1).double())      # exact in f64
    assert float(scaled.abs().max()) < 8
    negative = (y.view(torch.int32) < 0).reshape(blk.shape)
    return pack(encode(scaled, negative).reshape(y.shape)), s


def decode(codes: torch.Tensor) -> torch.Tensor:
    """codes uint8 (one per element) -> f64 grid values."""
    mag = torch.tensor(GRID, dtype=torch.float64)[(codes & 7).long()]
    return torch.where((codes & 8) != 0, -mag, mag)


def scale_values(s: torch.Tensor) -> torch.Tensor:
    """E8M0 bytes -> f64 scale values 2^(byte - 127)."""
    return torch.ldexp(torch.ones((), dtype=torch.float64), s.detach().cpu().to(torch.float64) - 127.0)


def dequantize(q: torch.Tensor, s: torch.Tensor) -> torch.Tensor:
    """(code bytes [..., K/2], scale bytes [..., K/32]) -> f64 values [..., K]."""
    q, s = q.detach().cpu(), s.detach().cpu()
    v = decode(unpack(q))
    return (v.reshape(*v.shape[:-1], -1, BLOCK) * scale_values(s).unsqueeze(-1)).reshape(v.shape)
