"""lpi_gemm_nt_mx8_256 without a GPU: the host predicate on a table of shapes, the EngineOptions switch, and no scratch in the new kernels (the K-tile
ring keeps LDS-DMA in flight behind counted waits: a scratch reload's vmcnt(0) would drain it — tests/test_no_spills.py)."""
import dataclasses
import os
import re
import shutil
import subprocess

import pytest

from lpi_amd import _lib

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LLVM = "/opt/rocm/lib/llvm/bin"


def test_gemm_mx8_256_ok_is_a_host_predicate():
    ok = _lib.load().lpi_gemm_mx8_256_ok
    # ViT-B/16 at 256 pairs: the vision tower's 54 528 = 213 x 256 rows, every block GEMM; ViT-L/14 (width 1024) likewise
    for rows, d in ((54528, 768), (19712, 512), (131584, 1024)):
        for N, K in ((3 * d, d), (d, d), (4 * d, d), (d, 4 * d)):
            assert ok(rows, N, K) == 1, (rows, N, K)
    table = {
        (256, 256, 256): 1, (512, 768, 3072): 1, (256, 256, 512): 1,
        (128, 256, 256): 0, (384, 256, 256): 0,      # M a multiple of 128 only
        (256, 384, 256): 0, (256, 128, 256): 0,      # N
        (256, 256, 128): 0,                          # one K-tile
        (256, 256, 384): 0, (256, 256, 640): 0,      # an odd number of K-tiles
        (256, 256, 192): 0, (256, 256, 288): 0,      # K not whole K-tiles
        (0, 256, 256): 0, (256, 0, 256): 0, (256, 256, 0): 0, (-256, 256, 256): 0,
        (50432, 768, 768): 1, (50560, 768, 768): 0,  # 197 x 256 rows; 395 x 128 rows: the 128x128 kernel's shape only
    }
    for shape, want in table.items():
        assert ok(*shape) == want, shape
        if want:
            assert _lib.load().lpi_gemm_mx8_ok(*shape) == 1      # whatever the 256x256 tile takes, the 128x128 kernel takes too


def test_binding_and_abi():
    assert "lpi_gemm_nt_mx8_256" in _lib.SIGNATURES and _lib.SIGNATURES["lpi_gemm_nt_mx8_256"] == _lib.SIGNATURES["lpi_gemm_nt_mx8"]
    assert _lib.GEMM_K_MX8_256 == _lib.GEMM_K_X3 + 1
    assert _lib.load().lpi_version() % 1000000 == _lib.EXPECTED_ABI >= 612
    hdr = open(os.path.join(REPO, "include", "lpi_hip.h")).read()
    assert re.search(r"#define LPI_GEMM_K_MX8_256 %d\b" % _lib.GEMM_K_MX8_256, hdr)


def test_engine_option():
    from lpi_amd.engine import EngineOptions
    assert "mx8_tile256" in {f.name for f in dataclasses.fields(EngineOptions)}
    assert EngineOptions().mx8_tile256 is True and EngineOptions().mx8_forward is False      # no default changes: the path needs mx8_forward
    assert EngineOptions.from_env(mx8_forward=True, mx8_tile256=False) == EngineOptions(mx8_forward=True, mx8_tile256=False)


def test_mx8_tile256_kernels_do_not_spill(tmp_path):
    """.private_segment_fixed_size == 0 for every gemm256_mx8_kernel instantiation, and 135 168 bytes of LDS fit the 160 KiB of a CU."""
    src = os.path.join(REPO, "lpi_amd", "csrc", "build", "gemm256.o")
    if not os.path.exists(src) or not os.path.exists(os.path.join(LLVM, "llvm-objdump")):
        pytest.skip("gemm256.o not built (run __graft_entry__.build()) or llvm-objdump not available")
    obj = shutil.copy(src, tmp_path / "gemm256.o")
    subprocess.run([os.path.join(LLVM, "llvm-objdump"), "--offloading", str(obj)], check=True, capture_output=True, cwd=tmp_path)
    dev = [p for p in os.listdir(tmp_path) if "amdgcn" in p]
    assert dev
    notes = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "--notes", str(tmp_path / dev[0])], check=True, capture_output=True, text=True).stdout
    ks = {}
    for blk in notes.split("- .agpr_count:")[1:]:
        name, size = re.search(r"\.name:\s+(\S+)", blk), re.search(r"\.private_segment_fixed_size:\s+(\d+)", blk)
        if name and size and "gemm256_mx8_kernel" in name.group(1):
            ks[name.group(1)] = (int(size.group(1)), int(re.search(r"\.vgpr_spill_count:\s+(\d+)", blk).group(1)))
    assert len(ks) == 10      # f32 x {none, residual, gelu}, bf16 x {none, gelu}, f16 x {none, residual, gelu}, MX x {none, gelu}
    assert {k: v for k, v in ks.items() if v != (0, 0)} == {}
