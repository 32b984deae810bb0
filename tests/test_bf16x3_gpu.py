"""Split-bf16 (bf16x3) GEMMs on a real MI355X: lpi_gemm_nt / lpi_gemm_nt_grouped with the operand code LPI_F32X3 (csrc/gemm.hip, csrc/gemm256_tile.h)
against the CPU restatement of the arithmetic (tests/bf16x3_emulate.py): bit for bit on integer operands whose every partial sum is exact (the test of the
fragment map and of the three terms: a dropped or doubled cross term, or a k-permutation that differs between the operands, fails there), on general data
against the f64 product of the ORIGINAL operands, the epilogues against the exact f32 kernel, the kernel attribution and the refusals."""
import pytest
import torch

pytestmark = pytest.mark.gpu

import bf16x3_emulate as X3  # noqa: E402
from lpi_amd import _lib  # noqa: E402
from lpi_amd._lib import BF16, EPI_DQUICKGELU, EPI_NONE, EPI_QUICKGELU, F16, F32, F32X3, GEMM_K_X3, call  # noqa: E402

DEV = "cuda:0"
# 128x128 kernel: one K-tile (prologue only); an odd number of K-tiles (both buffers); several tiles and the XCD remap
SHAPES_128 = [(128, 128, 32), (128, 128, 96), (256, 384, 160)]
# phased 256x256 kernel (tuning key 1 = 1): the minimum (K / 32 even and >= 2); two tiles; twelve tiles and 24 K-tiles
SHAPES_256 = [(256, 256, 64), (512, 256, 128), (512, 768, 768)]
ALL = [(s, False) for s in SHAPES_128] + [(s, True) for s in SHAPES_256]
IDS = [f"{m}x{n}x{k}{'-k256' if big else ''}" for (m, n, k), big in ALL]
U16 = 2.0 ** -16


def stream():
    return torch.cuda.current_stream().cuda_stream


class key1:
    """Tuning key 1 (minimum number of 256x256 tiles for which 4-byte operands take the phased 256x256 kernel) set to 1 inside the block, restored after."""

    def __init__(self, on):
        self.on = on

    def __enter__(self):
        lib = _lib.load()
        self.old = lib.lpi_get_tuning(1)
        if self.on:
            assert lib.lpi_set_tuning(1, 1) == 0

    def __exit__(self, *exc):
        assert _lib.load().lpi_set_tuning(1, self.old) == 0


def gemm(dt, a, b, c, bias=None, residual=None, epi=EPI_NONE, aux=None, alpha=1.0, cdt=F32):
    M, K = a.shape
    N = b.shape[0]
    call("lpi_gemm_nt", dt, cdt, M, N, K, a, a.stride(0), b, b.stride(0), c, c.stride(0), bias, residual, residual.stride(0) if residual is not None else 0,
         epi, aux, aux.stride(0) if aux is not None else 0, float(alpha), stream())


def run_x3(a, b, big, **kw):
    """One LPI_F32X3 launch of a [M, K] . b [N, K]^T; asserts one launch, attributed to the bf16x3 kernels.  -> C on the host (f64)."""
    c = torch.full((a.shape[0], b.shape[0]), -1.0, device=DEV)
    n0 = _lib.launch_count()
    with key1(big):
        gemm(F32X3, a.to(DEV), b.to(DEV), c, **kw)
    assert _lib.launch_count() == n0 + 1
    assert _lib.load().lpi_gemm_last_kernel() == GEMM_K_X3      # a build that quietly runs the f32 kernel fails here
    return c.cpu().double()


@pytest.mark.parametrize("swap", [False, True])
@pytest.mark.parametrize("shape,big", ALL, ids=IDS)
def test_integer_operands_bit_for_bit(shape, big, swap):
    M, N, K = shape
    a, b = X3.integer_operands(M, N, K, seed=M + N + K, swap=swap)
    ref = X3.gemm_x3(a, b)
    assert torch.equal(ref, a.double() @ b.double().t())
    assert torch.equal(run_x3(a, b, big), ref)


def test_full_16_bits_bit_for_bit():
    """|a| up to 2^16 - 1 against |b| <= 7 at K = 32: hi and lo carry 8 bits each."""
    for swap in (False, True):
        a, b = X3.integer_operands(128, 128, 32, seed=5, swap=swap, narrow_max=7)
        assert torch.equal(run_x3(a, b, False), X3.gemm_x3(a, b))


_MEASURED = {}


def measure(key, a, b, big):
    """Computed once per key: the f64 product of the operands, (|A||B|^T), the bf16x3 output, and the accumulation allowance measured on the spot from the
    PARENT's kernel: LPI_BF16 on the bf16-rounded copy of the same operands (bf16-exact: its only error is the matrix pipe's f32 accumulation) against
    the f64 product of that copy, relative to (|A||B|^T) of the copy, times 2.  The bf16 kernel's K is a multiple of 64: its operands are padded with
    zero columns, which add nothing to any sum."""
    if key not in _MEASURED:
        (M, K), N = a.shape, b.shape[0]
        ref, scale = a.double() @ b.double().t(), X3.abs_product(a, b)
        got = run_x3(a, b, big)
        ab, bb = a.to(torch.bfloat16), b.to(torch.bfloat16)
        Kp = (K + 63) // 64 * 64
        pad = lambda t: torch.nn.functional.pad(t, (0, Kp - K)).contiguous().to(DEV)  # noqa: E731
        cb = torch.zeros(M, N, device=DEV)
        gemm(BF16, pad(ab), pad(bb), cb)
        cb = cb.cpu().double()
        refb = ab.double() @ bb.double().t()
        allowance = 2.0 * float(((cb - refb).abs() / X3.abs_product(ab, bb)).max())
        _MEASURED[key] = dict(a=a, b=b, ref=ref, scale=scale, got=got, cb=cb, allowance=allowance)
    return _MEASURED[key]


def general(shape, big):
    """Gaussian rows with per-row log-normal gains and a x40 outlier channel (the generator of the host tests)."""
    M, N, K = shape
    return measure((shape, big), X3.rows(M, K, seed=K), X3.rows(N, K, seed=K + 1), big)


@pytest.mark.parametrize("shape,big", ALL, ids=IDS)
def test_general_data_against_f64(shape, big):
    """Measured on MI355X (max error / max |ref|; worst |err| / (|A||B|^T)): see DESIGN.md section 4, "bf16x3 GEMMs"."""
    g = general(shape, big)
    err = (g["got"] - g["ref"]).abs()
    errb = (g["cb"] - g["ref"]).abs()
    print(f"bf16x3 {shape} big={big}: max err / max |ref| {float(err.max() / g['ref'].abs().max()):.3e}, worst err / (|A||B|^T) {float((err / g['scale']).max()):.3e} "
          f"(bar {3 * U16 + g['allowance']:.3e}, allowance {g['allowance']:.3e}); LPI_BF16 on the rounded operands: max err {float(errb.max()):.3e} = "
          f"{float(errb.max() / err.max()):.0f} x")
    assert bool((err <= (3 * U16 + g["allowance"]) * g["scale"]).all())
    assert float(err.max()) <= float(errb.max()) / 32.0


EPI_SHAPE = (256, 384, 160)


@pytest.mark.parametrize("case", ["bias", "residual", "bias_residual", "quickgelu_saved", "quickgelu", "dquickgelu"])
def test_epilogues_against_the_f32_kernel(case):
    """Operands: plain Gaussian activations against weights of deviation 0.05, so that u = A.B^T + bias is of order one (where QuickGELU bends) and the
    bar, about 4.7e-5 of (|A||B|^T) ~ 5, stays three orders above what both arms share: the f32 rounding of the epilogue's own arithmetic (2^-24 |C|)."""
    M, N, K = EPI_SHAPE
    gen = torch.Generator().manual_seed(11)
    g = measure("epilogue", torch.randn(M, K, generator=gen), torch.randn(N, K, generator=gen) * 0.05, False)
    a, b = g["a"].to(DEV), g["b"].to(DEV)
    bias = torch.randn(N, generator=gen).to(DEV) if case in ("bias", "bias_residual", "quickgelu_saved", "quickgelu") else None
    res = torch.randn(M, N, generator=gen).to(DEV) if case in ("residual", "bias_residual") else None
    epi = {"quickgelu_saved": EPI_QUICKGELU, "quickgelu": EPI_QUICKGELU, "dquickgelu": EPI_DQUICKGELU}.get(case, EPI_NONE)
    scale = g["scale"]
    outs = []
    for dt in (F32, F32X3):
        c = torch.full((M, N), -1.0, device=DEV)
        aux = None
        if case == "quickgelu_saved":
            aux = torch.full((M, N), -1.0, device=DEV)
        elif case == "dquickgelu":
            aux = (torch.rand(M, N, generator=torch.Generator().manual_seed(12)) * 2 - 1).to(DEV)      # a stand-in for gelu'(u), |aux| <= 1
        n0 = _lib.launch_count()
        gemm(dt, a, b, c, bias=bias, residual=res, epi=epi, aux=aux)
        assert _lib.launch_count() == n0 + 1
        assert (_lib.load().lpi_gemm_last_kernel() == GEMM_K_X3) == (dt == F32X3)
        outs.append((c.cpu().double(), aux.cpu().double() if case == "quickgelu_saved" else None))
    bar = (3 * U16 + g["allowance"]) * scale
    diff = (outs[1][0] - outs[0][0]).abs()
    print(f"bf16x3 epilogue {case}: worst |x3 - f32| / bar {float((diff / bar).max()):.3f}")
    assert float(diff.max()) > 0      # not the f32 kernel's bits
    assert bool((diff <= bar).all())
    if case == "quickgelu_saved":
        assert bool(((outs[1][1] - outs[0][1]).abs() <= bar).all())


def test_grouped_entry_issues_the_descriptors_one_by_one():
    probs, refs = [], []
    for M, N, K in ((256, 384, 160), (128, 128, 96)):
        a, b = X3.integer_operands(M, N, K, seed=K)
        probs.append(dict(M=M, N=N, K=K, a=a.to(DEV), b=b.to(DEV), c=torch.full((M, N), -1.0, device=DEV)))
        refs.append(X3.gemm_x3(a, b))
    n0 = _lib.launch_count()
    grouped = _lib.gemm_grouped(F32X3, F32, EPI_NONE, 1.0, probs, stream())
    assert grouped is False and _lib.launch_count() == n0 + 2
    assert _lib.load().lpi_gemm_last_kernel() == GEMM_K_X3
    for p, r in zip(probs, refs):
        assert torch.equal(p["c"].cpu().double(), r)


def test_refusals_launch_nothing():
    lib = _lib.load()
    z = lambda *sh, dtype=torch.float32: torch.zeros(*sh, device=DEV, dtype=dtype)  # noqa: E731
    a, b, c, c16 = z(256, 256), z(256, 256), z(256, 256), z(256, 256, dtype=torch.bfloat16)
    st = stream()
    p = lambda t: None if t is None else t.data_ptr()  # noqa: E731
    n0 = _lib.launch_count()

    def rc(cdt, M, N, K, C, epi=EPI_NONE, aux=None):
        return lib.lpi_gemm_nt(F32X3, cdt, M, N, K, p(a), 256, p(b), 256, p(C), 256, None, None, 0, epi, p(aux), 256, 1.0, st)

    assert rc(BF16, 256, 256, 256, c16) in (-22, -38)      # c_dtype other than f32
    assert rc(F16, 256, 256, 256, c16) in (-22, -38)
    assert rc(F32, 256, 256, 48, c) == -22                 # K % 32
    assert rc(F32, 192, 256, 256, c) == -22                # M % 128
    assert rc(F32, 256, 192, 256, c) == -22                # N % 128
    assert rc(F32, 256, 256, 256, c, epi=_lib.EPI_LN) in (-22, -38)      # an epilogue the f32 mode does not use
    assert rc(F32, 256, 256, 256, c, epi=EPI_DQUICKGELU) == -22          # gelu' without its aux
    with pytest.raises(_lib.LpiError):                     # the few-row entry does not take the code: those GEMMs stay exact f32
        _lib.gemm_rows(F32X3, F32, EPI_NONE, 1.0, [dict(M=256, N=256, K=256, a=a, b=b, c=c)], st)
    with pytest.raises(_lib.LpiError):
        _lib.gemm_grouped(F32X3, BF16, EPI_NONE, 1.0, [dict(M=256, N=256, K=256, a=a, b=b, c=c16)], st)
    assert _lib.launch_count() == n0
    assert rc(F32, 256, 256, 256, c) == 0 and _lib.launch_count() == n0 + 1      # the same arguments, accepted
