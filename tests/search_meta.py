"""What the host tests of the streamed search (tests/test_search*_host.py) share: the public header without its comments, a declaration's ctypes
signature, and the per-kernel metadata of an object file's gfx950 code object."""
import os
import re
import shutil
import subprocess

from lpi_amd import _lib

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LLVM = "/opt/rocm/lib/llvm/bin"
EINVAL = -22
A = 1 << 20      # an aligned non-NULL address that is never dereferenced: the cases that pass it are refused on the host
_CTYPE = {"int": _lib._I, "long": _lib._L}


def header():
    """include/lpi_hip.h without its comments"""
    with open(os.path.join(REPO, "include", "lpi_hip.h")) as f:
        return re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)


def params(hdr, name):
    """(return type, ctypes argument types) of the declaration of `name` in the header text"""
    m = re.search(r"\b(int|long)\s+%s\s*\(([^)]*)\)\s*;" % name, hdr)
    assert m, name
    return m.group(1), [_lib._P if "*" in p else _CTYPE[p.split()[0]] for p in (q.strip() for q in m.group(2).split(","))]


def abi_version():
    """LPI_ABI_VERSION of csrc/api.hip"""
    with open(os.path.join(REPO, "lpi_amd", "csrc", "api.hip")) as f:
        return int(re.search(r"#define LPI_ABI_VERSION (\d+)", f.read()).group(1))


def have_objects(*names):
    """are these objects of lpi_amd/csrc/build and llvm-objdump there?"""
    return all(os.path.exists(obj_path(n)) for n in names) and os.path.exists(os.path.join(LLVM, "llvm-objdump"))


def obj_path(name):
    return os.path.join(REPO, "lpi_amd", "csrc", "build", name)


def kernels(obj, tmp_path):
    """{kernel name: (.private_segment_fixed_size, .vgpr_spill_count, .sgpr_spill_count)} of the gfx950 code object of an object file (the notes of
    llvm-readelf, parsed as tests/test_no_spills.py does); unbundled in a directory of its own under tmp_path"""
    d = tmp_path / os.path.basename(obj).replace(".", "_")
    d.mkdir()
    copy = shutil.copy(obj, d / os.path.basename(obj))
    subprocess.run([os.path.join(LLVM, "llvm-objdump"), "--offloading", str(copy)], check=True, capture_output=True, cwd=d)
    dev = [p for p in os.listdir(d) if "amdgcn" in p and p.startswith(os.path.basename(obj))]
    assert dev
    notes = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "--notes", str(d / dev[0])], check=True, capture_output=True, text=True).stdout
    ks = {}
    for blk in notes.split("- .agpr_count:")[1:]:
        name, size = re.search(r"\.name:\s+(\S+)", blk), re.search(r"\.private_segment_fixed_size:\s+(\d+)", blk)
        if name and size:
            ks[name.group(1)] = (int(size.group(1)), int(re.search(r"\.vgpr_spill_count:\s+(\d+)", blk).group(1)),
                                 int(re.search(r"\.sgpr_spill_count:\s+(\d+)", blk).group(1)))
    return ks
