"""The streamed search on 2-byte operands (csrc/search16.hip, search_tile.h; lpi_amd.search `operands`) without a GPU: header, binding and ABI number of the
typed entry points; every refusal of the 2-byte and of the forwarded f32 envelope before any launch (NULL or never-dereferenced operands: a launch
would fault, a refusal returns); no scratch in the six new kernels; the plugin's eval_search_operands key and the wrapper's keyword."""
import json
import os
import re

import pytest

import search_meta as M
from lpi_amd import _lib
from search_meta import A, EINVAL, REPO

_I, _P, _L = _lib._I, _lib._P, _lib._L


def test_header_binding_and_abi():
    want = {
        "lpi_search_topk_t": ("int", [_I, _I, _I, _I, _P, _I, _P, _I, _I, _I, _I, _P, _P, _P, _L, _P]),
        "lpi_search_rank_t": ("int", [_I, _I, _I, _I, _P, _I, _P, _I, _P, _I, _P, _P, _L, _P]),
    }
    hdr = M.header()
    for name, (ret, argtypes) in want.items():
        assert _lib.SIGNATURES[name] == argtypes, name
        assert M.params(hdr, name) == (ret, argtypes), name
    assert M.abi_version() == _lib.EXPECTED_ABI >= 615
    lib = _lib.load()
    assert lib.lpi_version() == _lib.EXPECTED_ABI
    assert (_lib.F32, _lib.BF16, _lib.F16, _lib.F32X3) == (0, 1, 2, 4)      # the codes of include/lpi_hip.h the cases below pass as `dt`


def _calls(lib, dt):
    def topk(nq=300, ng=4133, E=512, Q=A, ldq=None, G=A, ldg=None, k=10, col_base=0, acc=0, idx=A, val=A, ws=A, ws_bytes=None):
        ldq, ldg = E if ldq is None else ldq, E if ldg is None else ldg
        if ws_bytes is None:
            ws_bytes = max(1, lib.lpi_search_workspace(max(nq, 1), max(ng, 1), min(max(k, 1), 16)))
        return lib.lpi_search_topk_t(dt, nq, ng, E, Q, ldq, G, ldg, k, col_base, acc, idx, val, ws, ws_bytes, None)

    def rank(nq=300, ng=4133, E=512, Q=A, ldq=None, G=A, ldg=None, gt=A, gpr=5, out=A, ws=A, ws_bytes=None):
        ldq, ldg = E if ldq is None else ldq, E if ldg is None else ldg
        if ws_bytes is None:
            ws_bytes = max(1, lib.lpi_search_workspace(max(nq, 1), max(ng, 1), 0))
        return lib.lpi_search_rank_t(dt, nq, ng, E, Q, ldq, G, ldg, gt, gpr, out, ws, ws_bytes, None)

    return topk, rank


def _refused(lib, dt, shared):
    """`shared`: refusals of the operand envelope, both calls, with the given and with NULL pointers; then the refusals of k, col_base, idx, val, gt,
    rank, ws and ws_bytes that tests/test_search_host.py lists for the f32 entry points."""
    topk, rank = _calls(lib, dt)
    for kw in shared:
        none = dict(kw, **{p: None for p in ("Q", "G", "ws") if p not in kw})      # the refusals of shape hold with NULL operands too
        assert topk(**kw) == EINVAL, (dt, "topk", kw)
        assert rank(**kw) == EINVAL, (dt, "rank", kw)
        assert topk(**none, idx=None, val=None) == EINVAL and rank(**none, gt=None, out=None) == EINVAL, (dt, kw)
    for kw in (dict(k=0), dict(k=-1), dict(k=17), dict(k=16, ng=15), dict(col_base=-1), dict(col_base=2**31 - 100), dict(idx=None), dict(val=None),
               dict(ws_bytes=lib.lpi_search_workspace(300, 4133, 10) - 1), dict(ws_bytes=0)):
        assert topk(**kw) == EINVAL, (dt, kw)
    for kw in (dict(gt=None), dict(gpr=0), dict(gpr=-2), dict(out=None), dict(ws_bytes=8 * 300 - 1), dict(ws_bytes=0)):
        assert rank(**kw) == EINVAL, (dt, kw)


def test_every_refusal_returns_before_any_launch():
    lib = _lib.load()
    before = _lib.launch_count()
    common = [dict(nq=0), dict(nq=-3), dict(ng=0), dict(ng=-1), dict(Q=None), dict(G=None), dict(ws=None), dict(ws=A + 2)]
    for dt in (_lib.BF16, _lib.F16):      # E a multiple of 32, <= 1024; 16-byte rows = leading dimensions in multiples of 8 elements
        _refused(lib, dt, common + [dict(E=E) for E in (0, 16, 48, 72, 1056, 2048)]
                 + [dict(ldq=512 - 8), dict(ldq=512 + 4), dict(ldg=512 + 1), dict(ldg=512 - 8), dict(ldg=512 + 4),
                    dict(Q=A + 8), dict(G=A + 8), dict(Q=A + 2)])
    # LPI_F32 forwards: the f32 envelope (E a multiple of 16, leading dimensions in multiples of 4)
    _refused(lib, _lib.F32, common + [dict(E=E) for E in (0, 8, 24, 520, 1040, 2048)]
             + [dict(ldq=496), dict(ldg=496), dict(ldq=514), dict(ldg=513), dict(ldq=515), dict(Q=A + 4), dict(G=A + 8)])
    for dt in (_lib.F32X3, -1, 99, 3):     # not an operand type of the search: refused even where everything else is in the envelope
        topk, rank = _calls(lib, dt)
        assert topk() == EINVAL and rank() == EINVAL, dt
        assert topk(Q=None, G=None, ws=None, idx=None, val=None) == EINVAL and rank(Q=None, G=None, ws=None, gt=None, out=None) == EINVAL, dt
    assert _lib.launch_count() == before


def test_search16_kernels_use_no_scratch(tmp_path):
    """search16.o holds exactly the six 2-byte tile kernels (three modes x bf16, f16; the merge kernel is search.o's, not duplicated), none with
    scratch or spills; search.o still holds its three tile kernels and the one merge kernel."""
    if not M.have_objects("search16.o"):
        pytest.skip("search16.o not built (run __graft_entry__.build()) or llvm-objdump not available")
    ks = M.kernels(M.obj_path("search16.o"), tmp_path)
    assert len(ks) == 6 and all("search_kernel" in k for k in ks), sorted(ks)
    # Itanium mangling of the first template argument: t = unsigned short (bf16_t), DF16_ = _Float16 (f16_t); Li<MODE>E
    assert sorted(re.search(r"search_kernelI(t|DF16_)Li(\d)E", k).groups() for k in ks) == sorted((t, m) for t in ("t", "DF16_") for m in "012"), sorted(ks)
    assert {k: v for k, v in ks.items() if v != (0, 0, 0)} == {}
    ks = M.kernels(M.obj_path("search.o"), tmp_path)
    assert len([k for k in ks if "search_kernel" in k]) == 3 and len([k for k in ks if "search_merge_kernel" in k]) == 1, sorted(ks)
    assert {k: v for k, v in ks.items() if v != (0, 0, 0)} == {}


def test_eval_search_operands_key_is_validated_at_construction():
    from lpi_amd.retrieval.methods import sprompt
    assert sprompt._eval_search_operands({}) == "f32"      # the default does not change
    assert sprompt._eval_search_operands({"eval_scores": "streamed"}) == "f32"
    assert sprompt._eval_search_operands({"eval_scores": "matrix", "eval_search_operands": "f32"}) == "f32"
    for ops in ("bf16", "f16"):
        assert sprompt._eval_search_operands({"eval_scores": "streamed", "eval_search_operands": ops}) == ops
    args = json.load(open(os.path.join(REPO, "lpi_amd", "retrieval", "configs", "lpi", "coco_lpi.json")))
    assert "eval_search_operands" not in args
    for bad in ("fp8", "", None, 1, "BF16", "f32x3"):
        with pytest.raises(ValueError, match="eval_search_operands"):
            sprompt.SPrompts(dict(args, eval_scores="streamed", eval_search_operands=bad))      # raised before the network is built
    for ops in ("bf16", "f16"):
        with pytest.raises(ValueError, match="eval_search_operands"):
            sprompt.SPrompts(dict(args, eval_search_operands=ops))                              # eval_scores defaults to 'matrix'
        with pytest.raises(ValueError, match="eval_search_operands"):
            sprompt.SPrompts(dict(args, eval_scores="matrix", eval_search_operands=ops))


def test_operands_keyword_is_checked_before_anything_else():
    """An unknown operand type raises before the tensors are looked at: None is no tensor, and no device is touched."""
    from lpi_amd import search
    before = _lib.launch_count()
    for bad in ("fp8", "F16", "", 16, "f32x3"):
        with pytest.raises(ValueError, match="operands"):
            search.topk(None, None, 10, operands=bad)
        with pytest.raises(ValueError, match="operands"):
            search.gt_rank(None, None, None, operands=bad)
    assert _lib.launch_count() == before
