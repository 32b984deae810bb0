"""The streamed search on MX-FP8 operands (csrc/search_mx8.hip, search_tile.h; lpi_amd.search `operands="mx8"`, Mx8Rows) without a GPU: header, binding and
ABI number of the two entry points; every refusal of the envelope before any launch (NULL or never-dereferenced operands: a launch would fault, a refusal
returns); exactly three tile kernels in search_mx8.o, none with scratch or spills; the plugin's eval_search_operands key, the wrapper's keyword and
Mx8Rows' validation."""
import json
import os
import re

import pytest
import torch

import search_meta as M
from lpi_amd import _lib
from search_meta import A, EINVAL, REPO

_I, _P, _L = _lib._I, _lib._P, _lib._L


def test_header_binding_and_abi():
    want = {
        "lpi_search_topk_mx8": ("int", [_I, _I, _I, _P, _I, _P, _I, _P, _I, _P, _I, _I, _I, _I, _P, _P, _P, _L, _P]),
        "lpi_search_rank_mx8": ("int", [_I, _I, _I, _P, _I, _P, _I, _P, _I, _P, _I, _P, _I, _P, _P, _L, _P]),
    }
    hdr = M.header()
    for name, (ret, argtypes) in want.items():
        assert _lib.SIGNATURES[name] == argtypes, name
        assert M.params(hdr, name) == (ret, argtypes), name
    assert M.abi_version() == _lib.EXPECTED_ABI >= 616
    lib = _lib.load()
    assert lib.lpi_version() == _lib.EXPECTED_ABI
    assert hasattr(lib, "lpi_search_topk_mx8") and hasattr(lib, "lpi_search_rank_mx8")


def _calls(lib):
    def fill(E, kw):
        for ld, dflt in (("ldq", E), ("ldg", E), ("ldqs", E // 32), ("ldgs", E // 32)):
            if kw[ld] is None:
                kw[ld] = dflt
        return kw

    def topk(nq=300, ng=4133, E=512, Q=A, ldq=None, Qs=A, ldqs=None, G=A, ldg=None, Gs=A, ldgs=None, k=10, col_base=0, acc=0, idx=A, val=A, ws=A,
             ws_bytes=None):
        ld = fill(E, dict(ldq=ldq, ldg=ldg, ldqs=ldqs, ldgs=ldgs))
        if ws_bytes is None:
            ws_bytes = max(1, lib.lpi_search_workspace(max(nq, 1), max(ng, 1), min(max(k, 1), 16)))
        return lib.lpi_search_topk_mx8(nq, ng, E, Q, ld["ldq"], Qs, ld["ldqs"], G, ld["ldg"], Gs, ld["ldgs"], k, col_base, acc, idx, val, ws, ws_bytes, None)

    def rank(nq=300, ng=4133, E=512, Q=A, ldq=None, Qs=A, ldqs=None, G=A, ldg=None, Gs=A, ldgs=None, gt=A, gpr=5, out=A, ws=A, ws_bytes=None):
        ld = fill(E, dict(ldq=ldq, ldg=ldg, ldqs=ldqs, ldgs=ldgs))
        if ws_bytes is None:
            ws_bytes = max(1, lib.lpi_search_workspace(max(nq, 1), max(ng, 1), 0))
        return lib.lpi_search_rank_mx8(nq, ng, E, Q, ld["ldq"], Qs, ld["ldqs"], G, ld["ldg"], Gs, ld["ldgs"], gt, gpr, out, ws, ws_bytes, None)

    return topk, rank


def test_every_refusal_returns_before_any_launch():
    lib = _lib.load()
    before = _lib.launch_count()
    topk, rank = _calls(lib)
    shared = ([dict(nq=0), dict(nq=-3), dict(ng=0), dict(ng=-1), dict(ws=None), dict(ws=A + 2)]
              + [dict(E=E) for E in (0, 32, 64, 96, 160, 1152)]                                          # E a multiple of 128, <= 1024
              + [dict(ldq=512 - 16), dict(ldg=512 - 16), dict(ldq=512 + 8), dict(ldg=512 + 8), dict(ldq=512 + 1), dict(ldg=512 + 4)]      # >= E, multiples of 16
              + [dict(ldqs=16 - 4), dict(ldgs=16 - 4), dict(ldqs=16 + 2), dict(ldgs=16 + 2), dict(ldqs=16 + 1), dict(ldgs=16 + 3)]        # >= E / 32, multiples of 4
              + [dict(Q=A + 8), dict(G=A + 8), dict(Qs=A + 2), dict(Gs=A + 2)]                           # 16-byte / 4-byte aligned bases
              + [dict(Q=None), dict(Qs=None), dict(G=None), dict(Gs=None)])                              # no NULL operand or scale pointer
    for kw in shared:
        none = dict(kw, **{p: None for p in ("Q", "Qs", "G", "Gs", "ws") if p not in kw})      # the refusals of shape hold with NULL operands too
        assert topk(**kw) == EINVAL, ("topk", kw)
        assert rank(**kw) == EINVAL, ("rank", kw)
        assert topk(**none, idx=None, val=None) == EINVAL and rank(**none, gt=None, out=None) == EINVAL, kw
    # the list tests/test_search_host.py has for the f32 entry points
    for kw in (dict(k=0), dict(k=-1), dict(k=17), dict(k=16, ng=15), dict(col_base=-1), dict(col_base=2**31 - 100), dict(idx=None), dict(val=None),
               dict(ws_bytes=lib.lpi_search_workspace(300, 4133, 10) - 1), dict(ws_bytes=0)):
        assert topk(**kw) == EINVAL, kw
    for kw in (dict(gt=None), dict(gpr=0), dict(gpr=-2), dict(out=None), dict(ws_bytes=8 * 300 - 1), dict(ws_bytes=0)):
        assert rank(**kw) == EINVAL, kw
    # the typed entry points keep refusing the MX code: the MX form needs the scale pointers
    assert lib.lpi_search_topk_t(_lib.MX8, 300, 4133, 512, A, 512, A, 512, 10, 0, 0, A, A, A, lib.lpi_search_workspace(300, 4133, 10), None) == EINVAL
    assert lib.lpi_search_rank_t(_lib.MX8, 300, 4133, 512, A, 512, A, 512, A, 5, A, A, lib.lpi_search_workspace(300, 4133, 0), None) == EINVAL
    assert _lib.launch_count() == before


def test_search_mx8_kernels_use_no_scratch(tmp_path):
    """search_mx8.o holds exactly the three MX tile kernels (top-k, rank, threshold; the merge kernel is search.o's, not duplicated), none with scratch or
    spills."""
    if not M.have_objects("search_mx8.o"):
        pytest.skip("search_mx8.o not built (run __graft_entry__.build()) or llvm-objdump not available")
    ks = M.kernels(M.obj_path("search_mx8.o"), tmp_path)
    assert len(ks) == 3 and all("search_kernel" in k for k in ks), sorted(ks)
    assert sorted(re.search(r"search_kernelI5mx8_tLi(\d)E", k).group(1) for k in ks) == ["0", "1", "2"], sorted(ks)
    assert not [k for k in ks if "merge" in k]
    assert {k: v for k, v in ks.items() if v != (0, 0, 0)} == {}


def test_eval_search_operands_accepts_mx8_with_streamed_only():
    from lpi_amd.retrieval.methods import sprompt
    assert sprompt._eval_search_operands({"eval_scores": "streamed", "eval_search_operands": "mx8"}) == "mx8"
    assert sprompt._eval_search_operands({}) == "f32" and sprompt._eval_search_operands({"eval_scores": "streamed"}) == "f32"      # defaults unchanged
    args = json.load(open(os.path.join(REPO, "lpi_amd", "retrieval", "configs", "lpi", "coco_lpi.json")))
    with pytest.raises(ValueError, match="eval_search_operands"):
        sprompt.SPrompts(dict(args, eval_search_operands="mx8"))                              # eval_scores defaults to 'matrix'
    with pytest.raises(ValueError, match="eval_search_operands"):
        sprompt.SPrompts(dict(args, eval_scores="matrix", eval_search_operands="mx8"))
    for bad in ("MX8", "mxfp8", "fp8"):
        with pytest.raises(ValueError, match="eval_search_operands"):
            sprompt.SPrompts(dict(args, eval_scores="streamed", eval_search_operands=bad))


def _rows(n=8, E=256):
    return torch.zeros(n, E, dtype=torch.uint8), torch.zeros(n, E // 32 if E % 128 == 0 else 4 * ((E // 32 + 3) // 4), dtype=torch.uint8)[:, :E // 32]


def test_operands_mx8_passes_the_name_check_and_mx8rows_is_validated():
    """"mx8" is a known operand name: what raises next is the operand itself (None is no tensor), not the name check; an Mx8Rows goes with "mx8" only; the
    class refuses what the kernels cannot read in place.  All on CPU tensors, no launch."""
    from lpi_amd import search
    before = _lib.launch_count()
    assert search._operands("mx8") == "mx8"
    with pytest.raises(Exception) as ei:
        search.topk(None, None, 10, operands="mx8")
    assert "unknown operands" not in str(ei.value)
    with pytest.raises(Exception) as ei:
        search.gt_rank(None, None, None, operands="mx8")
    assert "unknown operands" not in str(ei.value)
    for bad in ("fp8", "MX8", "mxfp8"):
        with pytest.raises(ValueError, match="unknown operands"):
            search.topk(None, None, 10, operands=bad)

    c, s = _rows()
    r = search.Mx8Rows(c, s)
    assert tuple(r.shape) == (8, 256) and r.nbytes == 8 * 256 + 8 * 8 and len(r) == 8
    with pytest.raises(AttributeError):
        r.codes = c
    v = r[2:5]
    assert tuple(v.shape) == (3, 256) and v.codes.data_ptr() == c[2:5].data_ptr() and v.scales.data_ptr() == s[2:5].data_ptr()      # views
    with pytest.raises(TypeError):
        r[::2]
    for ops in (None, "f32", "bf16", "f16"):
        with pytest.raises(ValueError, match="Mx8Rows"):
            search.topk(r, r, 1, operands=ops)
        with pytest.raises(ValueError, match="Mx8Rows"):
            search.gt_rank(torch.zeros(8, 256), r, torch.zeros(8, dtype=torch.int32), operands=ops)
    wide_c, wide_s = torch.zeros(8, 256 + 16, dtype=torch.uint8), torch.zeros(8, 8 + 4, dtype=torch.uint8)
    search.Mx8Rows(wide_c[:, :256], wide_s[:, :8])                                     # strided rows are fine: 16-byte / 4-byte row strides
    bad = [
        (c.float(), s), (c, s.to(torch.int8)),                                          # dtype
        (c[0], s), (c, s[0]), (c[None], s),                                             # dims
        (c, s[:, :7]), (c[:4], s), (c[:, :250], s), (torch.zeros(8, 0, dtype=torch.uint8), torch.zeros(8, 0, dtype=torch.uint8)),      # shapes
        (torch.zeros(8, 512, dtype=torch.uint8)[:, ::2], s),                            # inner stride
        (torch.zeros(8, 256 + 8, dtype=torch.uint8)[:, :256], s),                       # row stride of the codes not 16 bytes
        (c, torch.zeros(8, 8 + 2, dtype=torch.uint8)[:, :8]),                           # row stride of the scales not 4 bytes
        (torch.zeros(8 * 256 + 8, dtype=torch.uint8)[8:].view(8, 256), s),              # base of the codes
        (c, torch.zeros(8 * 8 + 2, dtype=torch.uint8)[2:].view(8, 8)),                  # base of the scales
        (c.numpy(), s),                                                                 # not a tensor
    ]
    for cc, ss in bad:
        with pytest.raises(ValueError, match="Mx8Rows"):
            search.Mx8Rows(cc, ss)
    e384 = search.Mx8Rows(*_rows(4, 384))      # E = 384 is fine for the class and for the search ...
    with pytest.raises(ValueError, match="128"):
        search.topk(search.Mx8Rows(*_rows(4, 160)), search.Mx8Rows(*_rows(4, 160)), 1, operands="mx8")      # ... E = 160 for the class only
    assert tuple(e384.shape) == (4, 384)
    assert _lib.launch_count() == before
