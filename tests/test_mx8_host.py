"""MX-FP8 forward, host side: the CPU restatement of the format (tests/mx8_emulate.py, the yardstick of every GPU test of the MX kernels) against the
element bound and hand-written e4m3 cases; the shape predicate; the engine option; the build metadata of the MX GEMM kernels.  CPU only."""
import dataclasses
import os
import re
import shutil
import subprocess

import pytest
import torch

import mx8_emulate as MX  # noqa: E402
from lpi_amd import _lib  # noqa: E402

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LLVM = "/opt/rocm/lib/llvm/bin"


def gaussian_rows(rows=64, K=768, seed=0):
    """Seeded Gaussian rows with a per-row log-normal gain."""
    g = torch.Generator().manual_seed(seed)
    return torch.randn(rows, K, generator=g) * torch.exp(2.0 * torch.randn(rows, 1, generator=g))


def bound_cases():
    x = gaussian_rows()
    out = x.clone()
    out[:, 5] *= 40.0                                     # one x40 outlier channel
    zero = x.clone()
    zero[3, 64:96] = 0.0                                  # an all-zero block
    sub = x.clone()
    sub[7, 32:64] = torch.randn(32, generator=torch.Generator().manual_seed(1)) * 2.0 ** -140      # a block of f32-subnormal-range values
    return {"gaussian": x, "outlier": out, "zero_block": zero, "subnormal_block": sub}


@pytest.mark.parametrize("name", ["gaussian", "outlier", "zero_block", "subnormal_block"])
def test_emulator_obeys_the_element_bound(name):
    y = bound_cases()[name]
    q, s = MX.quantize(y)
    assert q.dtype == torch.uint8 and s.dtype == torch.uint8 and q.shape == y.shape and s.shape == (y.shape[0], y.shape[1] // 32)
    assert MX.bound_violations(y, q, s) == 0
    if name == "zero_block":
        assert int(s[3, 2]) == 0 and int(q[3, 64:96].max()) == 0
    if name == "subnormal_block":
        assert int(s[7, 1]) == 0      # e clamped to -127


def test_emulator_never_saturates_and_uses_the_top_binade():
    y = gaussian_rows(seed=3)
    q, s = MX.quantize(y)
    v = q.view(torch.float8_e4m3fn).float().abs().reshape(y.shape[0], -1, 32).amax(dim=-1)
    assert float(v.max()) <= 448.0 and float(v.min()) >= 224.0      # block maximum lands in (224, 448]: the bump-by-one rule, nothing clamps


def test_emulator_rounding_cases():
    # a block whose maximum is 256 has scale 2^0: the elements are rounded as they stand.  e4m3 has a step of 2 in [16, 32): ties go to the even mantissa
    y = torch.zeros(1, 32)
    y[0, 0] = 256.0
    y[0, 1:5] = torch.tensor([17.0, 19.0, 21.0, 23.0])
    y[0, 5] = 2.0 ** -10            # half the smallest subnormal (2^-9): a tie, to zero
    y[0, 6] = 2.0 ** -10 * 1.5      # above the tie: to the smallest subnormal
    y[0, 7] = -17.0
    q, s = MX.quantize(y)
    assert int(s[0, 0]) == 127
    d = MX.dequantize(q, s)[0]
    assert d[:8].tolist() == [256.0, 16.0, 20.0, 20.0, 24.0, 0.0, 2.0 ** -9, -16.0]
    # amax just above 448 2^e: the exponent is raised by one (449 -> scale 2, 224.5 -> 224); at 448 exactly it is not
    y = torch.zeros(2, 32)
    y[0, 0], y[1, 0] = 449.0, 448.0
    q, s = MX.quantize(y)
    assert s[:, 0].tolist() == [128, 127]
    assert MX.dequantize(q, s)[:, 0].tolist() == [448.0, 448.0]


def test_gemm_mx8_ok_is_a_host_predicate():
    lib = _lib.load()
    for d, rows in ((768, 50432), (512, 8192), (1024, 131584), (768, 16384)):      # ViT-B/16 and ViT-L/14: vision and text towers, padded row counts
        for N, K in ((3 * d, d), (d, d), (4 * d, d), (d, 4 * d)):
            assert lib.lpi_gemm_mx8_ok(rows, N, K) == 1
    assert lib.lpi_gemm_mx8_ok(256, 768, 64) == 0
    assert lib.lpi_gemm_mx8_ok(100, 768, 768) == 0
    assert lib.lpi_gemm_mx8_ok(256, 768, 588) == 0      # the patch embedding's K, un-padded
    assert lib.lpi_gemm_mx8_ok(0, 128, 128) == 0


def test_engine_option():
    from lpi_amd import synth
    from lpi_amd.engine import DualEncoder, EngineOptions
    assert "mx8_forward" in {f.name for f in dataclasses.fields(EngineOptions)}
    assert EngineOptions().mx8_forward is False
    assert EngineOptions.from_env(mx8_forward=True).mx8_forward is True
    assert EngineOptions.from_env(mx8_forward=True) == EngineOptions(mx8_forward=True)
    # refused with the f32 parity mode before anything touches the GPU (this test runs without one: the device check would raise LpiError first)
    with pytest.raises(ValueError, match="mx8_forward"):
        DualEncoder(synth.TINY, {}, dtype="f32", device="cuda:0", options=EngineOptions(mx8_forward=True))


def test_mx8_gemm_kernels_do_not_spill(tmp_path):
    """A scratch reload's vmcnt(0) would drain the K loop's LDS-DMA (tests/test_no_spills.py): .private_segment_fixed_size == 0 for every gemm_mx8 kernel."""
    src = os.path.join(REPO, "lpi_amd", "csrc", "build", "gemm_mx8.o")
    if not os.path.exists(src) or not os.path.exists(os.path.join(LLVM, "llvm-objdump")):
        pytest.skip("gemm_mx8.o not built (run __graft_entry__.build()) or llvm-objdump not available")
    obj = shutil.copy(src, tmp_path / "gemm_mx8.o")
    subprocess.run([os.path.join(LLVM, "llvm-objdump"), "--offloading", str(obj)], check=True, capture_output=True, cwd=tmp_path)
    dev = [p for p in os.listdir(tmp_path) if "amdgcn" in p]
    assert dev
    notes = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "--notes", str(tmp_path / dev[0])], check=True, capture_output=True, text=True).stdout
    ks = {}
    for blk in notes.split("- .agpr_count:")[1:]:
        name, size = re.search(r"\.name:\s+(\S+)", blk), re.search(r"\.private_segment_fixed_size:\s+(\d+)", blk)
        if name and size and "gemm_mx8_kernel" in name.group(1):
            ks[name.group(1)] = int(size.group(1))
    assert len(ks) >= 10
    assert {k: v for k, v in ks.items() if v} == {}
