"""Split-bf16 (bf16x3) GEMMs of the f32 mode, host side: the CPU restatement of the arithmetic (tests/bf16x3_emulate.py, the yardstick of the GPU tests)
against its algebraic bounds; the engine option; header, binding and ABI number; the build metadata of the new kernel instantiations.  CPU only."""
import dataclasses
import os
import re
import shutil
import subprocess

import pytest
import torch

import bf16x3_emulate as X3  # noqa: E402
from lpi_amd import _lib  # noqa: E402

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LLVM = "/opt/rocm/lib/llvm/bin"
U16 = 2.0 ** -16


def split_cases():
    x = X3.rows(64, 768, seed=0, outlier=False)
    out = X3.rows(64, 768, seed=0)
    p2 = torch.ldexp(torch.ones(64, 768), torch.arange(-60, 4).float()[:, None].expand(64, 768).contiguous()) * torch.tensor([1.0, -1.0]).repeat(384)
    zeros = x.clone()
    zeros[3] = 0.0
    zeros[:, 7] = 0.0
    return {"gaussian": x, "outlier": out, "powers_of_two": p2, "zeros": zeros}


@pytest.mark.parametrize("name", ["gaussian", "outlier", "powers_of_two", "zeros"])
def test_split_reproduces_x_to_2_pow_minus_16(name):
    x = split_cases()[name]
    hi, lo = X3.split(x)
    assert hi.dtype == torch.bfloat16 and lo.dtype == torch.bfloat16 and hi.shape == x.shape
    err = (hi.double() + lo.double() - x.double()).abs()
    assert bool((err <= U16 * x.double().abs()).all())
    # |x - hi| <= 2^-9 |x| (8 significant bits, round to nearest), and lo rounds that again: 2^-9 * 2^-9 would do; the format's promise is 2^-16
    assert bool(((x.double() - hi.double()).abs() <= 2.0 ** -8 * x.double().abs()).all())
    if name == "powers_of_two":
        assert torch.equal(hi.float(), x) and int((lo.float() != 0).sum()) == 0
    if name == "zeros":
        assert float(hi[3].float().abs().max()) == 0.0 and float(lo[:, 7].float().abs().max()) == 0.0


@pytest.mark.parametrize("swap", [False, True])
@pytest.mark.parametrize("K,narrow_max", [(32, 7), (32, 256), (160, 0), (768, 0), (3072, 0)])
def test_integer_operands_are_exact(K, narrow_max, swap):
    a, b = X3.integer_operands(48, 40, K, seed=K, swap=swap, narrow_max=narrow_max)
    if narrow_max == 7:
        assert float((b if swap else a).abs().max()) > 2 ** 15      # the full 16 bits of hi + lo
    wide = b if swap else a
    assert float(wide.abs().max()) < 2 ** 16 and float((b if not swap else a).abs().max()) <= 2 ** 8
    assert int((X3.split(wide)[1].float() != 0).sum()) > 0      # the lo plane is in play: a dropped cross term would show
    assert torch.equal(X3.gemm_x3(a, b), a.double() @ b.double().t())


@pytest.mark.parametrize("K", [32, 768, 3072])
@pytest.mark.parametrize("outlier", [False, True])
def test_emulator_obeys_the_algebraic_bound(K, outlier):
    a, b = X3.rows(64, K, seed=K, outlier=outlier), X3.rows(48, K, seed=K + 1, outlier=outlier)
    ref = a.double() @ b.double().t()
    got = X3.gemm_x3(a, b)
    scale = X3.abs_product(a, b)
    ratio = float(((got - ref).abs() / scale).max())
    print(f"bf16x3 emulator K={K} outlier={outlier}: worst |err| / (|A||B|^T) = 2^{torch.log2(torch.tensor(ratio)).item():.2f}, "
          f"max err / max |ref| = {float((got - ref).abs().max() / ref.abs().max()):.2e}")
    assert bool(((got - ref).abs() <= 3 * U16 * scale).all())


def test_engine_option():
    from lpi_amd import synth
    from lpi_amd.engine import DualEncoder, EngineOptions
    assert "gemm_bf16x3" in {f.name for f in dataclasses.fields(EngineOptions)}
    assert EngineOptions().gemm_bf16x3 is False
    opt = EngineOptions(gemm_bf16x3=True)
    assert opt.gemm_bf16x3 is True and EngineOptions.from_env(gemm_bf16x3=True) == opt
    for dtype in ("bf16", "f16"):
        with pytest.raises(ValueError, match="gemm_bf16x3"):
            opt.check_dtype(dtype)
    opt.check_dtype("f32")
    EngineOptions().check_dtype("bf16")
    # refused before anything touches the GPU (this test runs without one: the device check would raise LpiError first)
    with pytest.raises(ValueError, match="gemm_bf16x3"):
        DualEncoder(synth.TINY, {}, dtype="bf16", device="cuda:0", options=opt)


def test_engine_sends_the_code_only_to_lpi_gemm_nt(monkeypatch):
    """engine.gemm with the operand code F32X3: a few-row shape goes to lpi_gemm_nt_rows as F32, any other to lpi_gemm_nt as F32X3; F32 is the parent's call."""
    from lpi_amd import engine as E
    seen = []
    monkeypatch.setattr(E, "call", lambda name, *args: seen.append((name, args[0])))
    monkeypatch.setattr(E._lib, "gemm_rows", lambda dt, *args: seen.append(("rows", dt)))
    monkeypatch.setattr(E, "_stream", lambda: 0)
    t = lambda r, c: torch.zeros(r, c)  # noqa: E731
    for dt in (E.F32X3, E.F32):
        E.gemm(dt, t(256, 128), t(128, 128), t(256, 128), 256, 128, 128)          # few rows
        E.gemm(dt, t(768, 128), t(128, 128), t(768, 128), 768, 128, 128)          # more than 512 rows
    assert seen == [("rows", _lib.F32), ("lpi_gemm_nt", _lib.F32X3), ("rows", _lib.F32), ("lpi_gemm_nt", _lib.F32)]
    assert E._gemm_code(E.F32, E.EngineOptions(gemm_bf16x3=True)) == _lib.F32X3
    assert E._gemm_code(E.F32, E.EngineOptions()) == _lib.F32


def test_header_binding_and_abi_agree():
    hdr = open(os.path.join(REPO, "include", "lpi_hip.h")).read()
    define = lambda name: int(re.search(r"#define %s (\d+)" % name, hdr).group(1))  # noqa: E731
    assert define("LPI_F32X3") == _lib.F32X3 == 4
    assert define("LPI_GEMM_K_X3") == _lib.GEMM_K_X3 == 6
    assert len({define(n) for n in ("LPI_F32", "LPI_BF16", "LPI_F16", "LPI_MX8", "LPI_F32X3")}) == 5
    api = open(os.path.join(REPO, "lpi_amd", "csrc", "api.hip")).read()
    assert int(re.search(r"#define LPI_ABI_VERSION (\d+)", api).group(1)) == _lib.EXPECTED_ABI >= 611
    assert _lib.load().lpi_version() == _lib.EXPECTED_ABI


@pytest.mark.parametrize("unit,kernel", [("gemm", "gemm_nt_kernel"), ("gemm256", "gemm256_kernel")])
def test_bf16x3_kernels_do_not_spill(tmp_path, unit, kernel):
    """A scratch reload's vmcnt(0) would drain the K loop's LDS-DMA (tests/test_no_spills.py): .private_segment_fixed_size == 0 for the five epilogue
    instantiations of each kernel on the f32x3_t element tag."""
    src = os.path.join(REPO, "lpi_amd", "csrc", "build", unit + ".o")
    if not os.path.exists(src) or not os.path.exists(os.path.join(LLVM, "llvm-objdump")):
        pytest.skip(f"{unit}.o not built (run __graft_entry__.build()) or llvm-objdump not available")
    obj = shutil.copy(src, tmp_path / (unit + ".o"))
    subprocess.run([os.path.join(LLVM, "llvm-objdump"), "--offloading", str(obj)], check=True, capture_output=True, cwd=tmp_path)
    dev = [p for p in os.listdir(tmp_path) if "amdgcn" in p]
    assert dev
    notes = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "--notes", str(tmp_path / dev[0])], check=True, capture_output=True, text=True).stdout
    ks = {}
    for blk in notes.split("- .agpr_count:")[1:]:
        name, size = re.search(r"\.name:\s+(\S+)", blk), re.search(r"\.private_segment_fixed_size:\s+(\d+)", blk)
        if name and size and kernel in name.group(1) and "f32x3_t" in name.group(1):
            ks[name.group(1)] = int(size.group(1))
    assert len(ks) == 5
    assert {k: v for k, v in ks.items() if v} == {}
