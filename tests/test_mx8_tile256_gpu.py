"""lpi_gemm_nt_mx8_256 (MX-FP8 operands on the phased 256x256 tile: csrc/gemm256_tile.h on one-byte elements) on a real MI355X: bit for bit the 128x128
kernel (lpi_gemm_nt_mx8) on the same buffers for every combination the entry point takes, integer-exact against the CPU restatement of the format
(tests/mx8_emulate.py) independently of that kernel, one launch of the right kind per call, and the rejections.

Every leading dimension is larger than its row and every output has rows beyond M; pad columns and rows are pre-filled with a canary and must come back
untouched.  Shapes: the smallest at which the tile can go wrong — two K-tiles (prologue and one ring turn only), six K-tiles with two column tiles, two row
tiles, and 24 K-tiles (the ring wrapping many times)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

import mx8_emulate as MX  # noqa: E402
from lpi_amd import _lib  # noqa: E402
from lpi_amd._lib import BF16, F16, F32, MX8, call  # noqa: E402
from lpi_amd.engine import EPI_NONE, EPI_QUICKGELU  # noqa: E402

DEV = "cuda:0"
SHAPES = [(256, 256, 256), (256, 512, 768), (512, 256, 1024), (512, 768, 3072)]
ROWS_BEYOND = 8      # rows of every output beyond M
CANARY = {torch.float32: -7.25, torch.bfloat16: -7.25, torch.float16: -7.25, torch.uint8: 0xA5}
# (name, c_dtype, torch type of C, bias, residual, epilogue)
COMBOS = [
    ("f32", F32, torch.float32, False, False, EPI_NONE),
    ("bf16+bias", BF16, torch.bfloat16, True, False, EPI_NONE),
    ("f16+res", F16, torch.float16, True, True, EPI_NONE),
    ("bf16+gelu", BF16, torch.bfloat16, True, False, EPI_QUICKGELU),
    ("mx+gelu", MX8, torch.uint8, True, False, EPI_QUICKGELU),
    ("f32+res", F32, torch.float32, False, True, EPI_NONE),
]


def stream():
    return torch.cuda.current_stream().cuda_stream


def padded(t, ld, fill=0):
    """t [R, C] inside a [R, ld] buffer (ld > C): a view with row stride ld; the pad columns hold `fill`."""
    buf = torch.full((t.shape[0], ld), fill, dtype=t.dtype)
    buf[:, :t.shape[1]] = t
    return buf.to(DEV)[:, :t.shape[1]]


def scale_bytes(rows, blocks, lo, g):
    """Random E8M0 bytes in [lo, lo + 12) with no two neighbouring K blocks of a row alike: a scale routed to the wrong block or row changes the result."""
    s = torch.randint(0, 12, (rows, blocks), generator=g)
    for b in range(1, blocks):
        same = s[:, b] == s[:, b - 1]
        s[same, b] = (s[same, b] + 1 + torch.randint(0, 10, (int(same.sum()),), generator=g)) % 12
    assert bool((s[:, 1:] != s[:, :-1]).all())
    return (lo + s).to(torch.uint8)


_OPERANDS = {}


def operands(M, N, K):
    """Random e4m3 bytes (the two NaN codes replaced) and per-block scales 2^-16 .. 2^-5 for A, 2^-14 .. 2^-3 for B: |a b| <= 448^2 2^-8 per product, so the
    f32 sums stay below 2^10 K — finite, and in practice (a few hundred at K = 3072) inside fp16's range; bias and residual O(1).  Built once per shape, on the device, never written."""
    if (M, N, K) not in _OPERANDS:
        g = torch.Generator().manual_seed(M + 3 * N + 7 * K)

        def elems(rows):
            q = torch.randint(0, 256, (rows, K), generator=g).to(torch.uint8)
            q[(q & 0x7F) == 0x7F] = 0x3A
            return q
        aq, bq = elems(M), elems(N)
        as_, bs = scale_bytes(M, K // 32, 127 - 16, g), scale_bytes(N, K // 32, 127 - 14, g)
        res = torch.randn(M, N, generator=g)
        _OPERANDS[(M, N, K)] = {
            "a": padded(aq, K + 16, 0x38), "as": padded(as_, K // 32 + 4, 140), "b": padded(bq, K + 32, 0x38), "bs": padded(bs, K // 32 + 8, 140),
            "bias": torch.randn(N, generator=g).to(DEV), "res32": padded(res, N + 8), "res16": padded(res.half(), N + 8),
        }
    return _OPERANDS[(M, N, K)]


def outputs(M, N, ctype):
    """C [M + ROWS_BEYOND, ldc > N] and, for an MX output, its scales [M + ROWS_BEYOND, ldcs > N / 32], canary-filled."""
    c = torch.full((M + ROWS_BEYOND, N + 16), CANARY[ctype], dtype=ctype, device=DEV)
    cs = torch.full((M + ROWS_BEYOND, N // 32 + 3), CANARY[torch.uint8], dtype=torch.uint8, device=DEV) if ctype == torch.uint8 else None
    return c, cs


def run(name, op, M, N, K, cdt, c, cs, bias, residual, epi, alpha=1.0):
    call(name, cdt, M, N, K, op["a"], op["a"].stride(0), op["as"], op["as"].stride(0), op["b"], op["b"].stride(0), op["bs"], op["bs"].stride(0), c,
         c.stride(0), cs, cs.stride(0) if cs is not None else 0, bias, residual, residual.stride(0) if residual is not None else 0, epi, float(alpha), stream())


def bits(t):
    return t.cpu().view({1: torch.uint8, 2: torch.int16, 4: torch.int32}[t.element_size()])


def canary_intact(t, rows, cols):
    ref = torch.full_like(t, CANARY[t.dtype])
    return torch.equal(bits(t[rows:]), bits(ref[rows:])) and torch.equal(bits(t[:, cols:]), bits(ref[:, cols:]))


@pytest.mark.parametrize("combo", COMBOS, ids=[c[0] for c in COMBOS])
@pytest.mark.parametrize("M,N,K", SHAPES)
def test_bit_for_bit_the_128x128_kernel(M, N, K, combo):
    _, cdt, ctype, with_bias, with_res, epi = combo
    op = operands(M, N, K)
    bias = op["bias"] if with_bias else None
    residual = (op["res16"] if ctype == torch.float16 else op["res32"]) if with_res else None
    lib = _lib.load()
    got = {}
    for name, kind in (("lpi_gemm_nt_mx8", _lib.GEMM_K_MX8), ("lpi_gemm_nt_mx8_256", _lib.GEMM_K_MX8_256)):
        c, cs = outputs(M, N, ctype)
        n0 = _lib.launch_count()
        run(name, op, M, N, K, cdt, c, cs, bias, residual, epi)
        assert _lib.launch_count() == n0 + 1 and lib.lpi_gemm_last_kernel() == kind      # one launch, attributed to its kernel
        torch.cuda.synchronize()
        assert canary_intact(c, M, N) and (cs is None or canary_intact(cs, M, N // 32)), name
        got[name] = (c, cs)
    (c0, s0), (c1, s1) = got["lpi_gemm_nt_mx8"], got["lpi_gemm_nt_mx8_256"]
    if ctype != torch.uint8:
        assert bool(torch.isfinite(c0[:M, :N].float()).all())
    assert not torch.equal(bits(c0[:M, :N]), bits(torch.full_like(c0[:M, :N], CANARY[ctype])))      # written at all
    assert torch.equal(bits(c1), bits(c0))
    if cs is not None:
        assert torch.equal(s1.cpu(), s0.cpu())


def test_alpha_is_applied_alike():
    """alpha != 1 through the f32 and the MX store code: the same bits as the 128x128 kernel."""
    M, N, K = 256, 512, 768
    op = operands(M, N, K)
    for cdt, ctype, epi in ((F32, torch.float32, EPI_NONE), (MX8, torch.uint8, EPI_QUICKGELU)):
        out = []
        for name in ("lpi_gemm_nt_mx8", "lpi_gemm_nt_mx8_256"):
            c, cs = outputs(M, N, ctype)
            run(name, op, M, N, K, cdt, c, cs, op["bias"], None, epi, alpha=0.375)
            out.append((c, cs))
        assert torch.equal(bits(out[0][0]), bits(out[1][0]))
        if ctype == torch.uint8:
            assert torch.equal(out[0][1].cpu(), out[1][1].cpu())


def integer_operands(M, N, K, seed):
    """e4m3 bytes of integers in [-8, 8] and per-block scales from {1, 2, 4} (A) and {1/2, 1, 2} (B), every row and K block different: every partial sum is
    a multiple of 1/2 below 2^22, so f32 accumulation is exact in any order (the operands of tests/test_mx8_gpu.py)."""
    g = torch.Generator().manual_seed(seed)
    a = torch.randint(-8, 9, (M, K), generator=g).float()
    b = torch.randint(-8, 9, (N, K), generator=g).float()
    a[:, 0] = (torch.arange(M) % 17 - 8).float()
    b[:, 1] = (torch.arange(N) % 13 - 6).float()
    as_ = (127 + torch.randint(0, 3, (M, K // 32), generator=g)).to(torch.uint8)
    bs = (126 + torch.randint(0, 3, (N, K // 32), generator=g)).to(torch.uint8)
    aq, bq = a.to(torch.float8_e4m3fn).view(torch.uint8), b.to(torch.float8_e4m3fn).view(torch.uint8)
    ref = MX.dequantize(aq, as_) @ MX.dequantize(bq, bs).t()
    assert float(ref.abs().max()) < 2 ** 22
    return aq, as_, bq, bs, ref


@pytest.mark.parametrize("M,N,K", [SHAPES[0], SHAPES[3]])
def test_integer_exact_against_the_emulator(M, N, K):
    aq, as_, bq, bs, ref = integer_operands(M, N, K, seed=K + 1)
    op = {"a": padded(aq, K + 16), "as": padded(as_, K // 32 + 4), "b": padded(bq, K + 16), "bs": padded(bs, K // 32 + 4)}
    c, _ = outputs(M, N, torch.float32)
    run("lpi_gemm_nt_mx8_256", op, M, N, K, F32, c, None, None, None, EPI_NONE)
    assert canary_intact(c, M, N)
    assert torch.equal(c[:M, :N].cpu().double(), ref)
    # the MX store code on the exact product: bytes and scales are the emulator's quantiser's
    cq, cs = outputs(M, N, torch.uint8)
    run("lpi_gemm_nt_mx8_256", op, M, N, K, MX8, cq, cs, None, None, EPI_NONE)
    qr, sr = MX.quantize(ref.float())
    assert canary_intact(cq, M, N) and canary_intact(cs, M, N // 32)
    assert torch.equal(cs[:M, :N // 32].cpu(), sr) and torch.equal(cq[:M, :N].cpu(), qr)


def test_rejections_launch_nothing():
    lib = _lib.load()
    z = lambda *sh: torch.zeros(*sh, device=DEV, dtype=torch.uint8)  # noqa: E731
    a, as_, b, bs = z(512, 512), z(512, 16), z(512, 512), z(512, 16)
    c, c16, cb = torch.zeros(512, 512, device=DEV), torch.zeros(512, 512, device=DEV, dtype=torch.float16), torch.zeros(512, 512, device=DEV, dtype=torch.bfloat16)
    st = stream()
    n0 = _lib.launch_count()

    def rc(fn, cdt, M, N, K, A, As, B, Bs, C, Cs, R=None):
        p = lambda t: None if t is None else t.data_ptr()  # noqa: E731
        return fn(cdt, M, N, K, p(A), 512, p(As), 16, p(B), 512, p(Bs), 16, p(C), 512, p(Cs), 16, None, p(R), 512 if R is not None else 0, EPI_NONE, 1.0, st)

    g = lib.lpi_gemm_nt_mx8_256
    assert rc(g, F32, 128, 256, 256, a, as_, b, bs, c, None) == -22       # M a multiple of 128 only
    assert rc(g, F32, 256, 384, 256, a, as_, b, bs, c, None) == -22       # N
    assert rc(g, F32, 256, 256, 128, a, as_, b, bs, c, None) == -22       # one K-tile
    assert rc(g, F32, 256, 256, 384, a, as_, b, bs, c, None) == -22       # an odd number of K-tiles
    assert rc(g, F32, 256, 256, 256, a, None, b, bs, c, None) == -22      # NULL scales of an MX operand
    assert rc(g, F32, 256, 256, 256, a, as_, b, None, c, None) == -22
    assert rc(g, MX8, 256, 256, 256, a, as_, b, bs, z(512, 512), None) == -22               # ... of an MX output
    assert rc(g, MX8, 256, 256, 256, a, as_, b, bs, z(512, 512), z(512, 16), R=c) == -22    # MX output with a residual
    assert rc(g, F32, 256, 256, 256, a[:, 4:], as_, b, bs, c, None) == -22                  # a misaligned operand
    # bf16 output with a residual: the 128x128 entry point's code
    code = rc(lib.lpi_gemm_nt_mx8, BF16, 256, 256, 256, a, as_, b, bs, cb, None, R=c16)
    assert code != 0 and rc(g, BF16, 256, 256, 256, a, as_, b, bs, cb, None, R=c16) == code
    assert _lib.launch_count() == n0
