"""The wide streamed search (csrc/search_wide.hip: top-k lists up to k = 256 in one sweep) without a GPU: header, binding and ABI number; the workspace
function; every refusal of the envelope before any launch (NULL device pointers: a launch would fault, a refusal returns); no scratch in the new
kernels; what lpi_amd.search.topk refuses before it touches the device."""
import re

import pytest

import search_meta as M
from lpi_amd import _lib, search
from search_meta import EINVAL
from search_meta import params as _params

_I, _P, _L = _lib._I, _lib._P, _lib._L
PAIRS = {"lpi_search_topk_wide": "lpi_search_topk", "lpi_search_topk_wide_t": "lpi_search_topk_t", "lpi_search_topk_wide_mx8": "lpi_search_topk_mx8"}


def test_header_binding_and_abi():
    hdr = M.header()
    for wide, narrow in PAIRS.items():
        assert _params(hdr, wide) == _params(hdr, narrow) == ("int", _lib.SIGNATURES[narrow]), wide
        assert _lib.SIGNATURES[wide] == _lib.SIGNATURES[narrow], wide
        assert hasattr(_lib.load(), wide)
    assert _params(hdr, "lpi_search_wide_workspace") == ("long", [_I, _I, _I]) and _lib.SIGNATURES["lpi_search_wide_workspace"] == [_I, _I, _I]
    assert _lib._RESTYPES["lpi_search_wide_workspace"] is _L
    assert re.search(r"#define\s+LPI_SEARCH_KWIDE\s+256\b", hdr)
    assert M.abi_version() == _lib.EXPECTED_ABI >= 617
    assert _lib.load().lpi_version() == _lib.EXPECTED_ABI


def test_workspace_is_positive_monotone_and_saturates():
    ws = _lib.load().lpi_search_wide_workspace
    nqs = (1, 5, 127, 128, 129, 300, 2048, 5000, 25000, 123287)
    ngs = (1, 16, 127, 129, 4133, 25000, 65536, 70001, 616767)      # ng = 1 with k > 1 is a legal workspace question: the accumulating call takes it
    ks = (1, 16, 17, 100, 256)
    for k in ks:
        table = [[ws(nq, ng, k) for ng in ngs] for nq in nqs]
        for a, row in enumerate(table):
            for b, v in enumerate(row):
                assert v > 0, (nqs[a], ngs[b], k)
                assert b == 0 or v >= row[b - 1], ("ng", nqs[a], ngs[b], k)
                assert a == 0 or v >= table[a - 1][b], ("nq", nqs[a], ngs[b], k)
            assert row[ngs.index(65536)] == row[-1] == ws(nqs[a], 2**31 - 1, k), ("the split count has saturated", nqs[a], k)
    for nq in nqs:
        for ng in ngs:
            sizes = [ws(nq, ng, k) for k in range(1, 257)]
            assert sizes == sorted(sizes), (nq, ng)
    assert 0 < ws(2048, 1048576, 256) < 2048 * 1048576 * 4 // 8      # below an eighth of the score matrix's 8 GiB
    for bad in ((0, 5, 1), (5, 0, 1), (-1, 5, 1), (5, -1, 1), (5, 5, 0), (5, 5, -1), (5, 5, 257)):
        assert ws(*bad) == EINVAL, bad
    narrow = _lib.load().lpi_search_workspace
    assert narrow(5, 5, 17) == EINVAL and narrow(300, 4133, 16) > 0      # the narrow range is what it was


def test_every_refusal_returns_before_any_launch():
    """Shapes and strides outside each entry point's envelope with NULL operands: LPI_EINVAL comes back and nothing was launched.  Then a valid envelope
    with each required pointer missing, misaligned operands, k outside 1..256 or above ng, col_base, a workspace one byte short, a bad dt."""
    lib = _lib.load()
    before = _lib.launch_count()
    A = 1 << 20      # an aligned non-NULL address that is never dereferenced: every case below is refused on the host
    wsf = lib.lpi_search_wide_workspace

    def call(form, nq=300, ng=4133, E=512, Q=A, ldq=None, G=A, ldg=None, k=100, col_base=0, acc=0, idx=A, val=A, ws=A, ws_bytes=None, dt=_lib.BF16,
             Qs=A, ldqs=None, Gs=A, ldgs=None):
        ldq, ldg = E if ldq is None else ldq, E if ldg is None else ldg
        if ws_bytes is None:
            ws_bytes = max(1, wsf(max(nq, 1), max(ng, 1), min(max(k, 1), 256)))
        tail = (k, col_base, acc, idx, val, ws, ws_bytes, None)
        if form == "f32":
            return lib.lpi_search_topk_wide(nq, ng, E, Q, ldq, G, ldg, *tail)
        if form == "t":
            return lib.lpi_search_topk_wide_t(dt, nq, ng, E, Q, ldq, G, ldg, *tail)
        ldqs, ldgs = (E // 32 if ldqs is None else ldqs), (E // 32 if ldgs is None else ldgs)
        return lib.lpi_search_topk_wide_mx8(nq, ng, E, Q, ldq, Qs, ldqs, G, ldg, Gs, ldgs, *tail)

    shapes = [dict(nq=0), dict(nq=-3), dict(ng=0), dict(ng=-1), dict(E=0), dict(E=8), dict(E=1040), dict(E=2048), dict(ldq=496), dict(ldg=496),
              dict(Q=None), dict(G=None), dict(Q=A + 4), dict(G=A + 8), dict(ws=None), dict(ws=A + 2)]
    per_form = {"f32": [dict(E=24), dict(E=520), dict(ldq=514), dict(ldg=513), dict(ldq=515)],
                "t": [dict(E=16), dict(E=48), dict(E=528), dict(ldq=516), dict(ldg=514), dict(ldq=513)],
                "mx8": [dict(E=32), dict(E=64), dict(E=192), dict(E=576), dict(ldq=520), dict(ldg=528 - 8), dict(Qs=None), dict(Gs=None), dict(Qs=A + 2),
                        dict(Gs=A + 1), dict(ldqs=12), dict(ldgs=12), dict(ldqs=18), dict(ldgs=17)]}
    for form, extra in per_form.items():
        for kw in shapes + extra:
            none = dict(kw, **{p: None for p in ("Q", "G", "ws") if p not in kw})      # the refusals of shape hold with NULL operands too
            assert call(form, **kw) == EINVAL, (form, kw)
            if not any(p in kw for p in ("Qs", "Gs")):
                assert call(form, **none, idx=None, val=None) == EINVAL, (form, kw)
        for kw in (dict(k=0), dict(k=-1), dict(k=257), dict(k=256, ng=255), dict(col_base=-1), dict(col_base=2**31 - 100), dict(idx=None),
                   dict(val=None), dict(ws_bytes=wsf(300, 4133, 100) - 1), dict(ws_bytes=0)):
            assert call(form, **kw) == EINVAL, (form, kw)
    for dt in (_lib.MX8, _lib.F32X3, -1, 99):
        assert call("t", dt=dt) == EINVAL, dt
    assert call("t", dt=_lib.F32, E=24) == EINVAL and call("t", dt=_lib.F32, Q=None) == EINVAL      # forwarded to the f32 form: its envelope
    for form in per_form:      # the narrow calls keep refusing k = 17
        assert {"f32": lib.lpi_search_topk(300, 4133, 512, A, 512, A, 512, 17, 0, 0, A, A, A, 1 << 40, None),
                "t": lib.lpi_search_topk_t(_lib.BF16, 300, 4133, 512, A, 512, A, 512, 17, 0, 0, A, A, A, 1 << 40, None),
                "mx8": lib.lpi_search_topk_mx8(300, 4133, 512, A, 512, A, 16, A, 512, A, 16, 17, 0, 0, A, A, A, 1 << 40, None)}[form] == EINVAL
    assert _lib.launch_count() == before


def test_wide_kernels_use_no_scratch(tmp_path):
    """.private_segment_fixed_size == 0 and no VGPR spill for every kernel of search_wide.hip: four sweeps (f32, bf16, f16, MX-FP8) and one merge."""
    if not M.have_objects("search_wide.o"):
        pytest.skip("search_wide.o not built (run __graft_entry__.build()) or llvm-objdump not available")
    ks = M.kernels(M.obj_path("search_wide.o"), tmp_path)
    assert len([k for k in ks if "search_kernel" in k]) == 4 and len([k for k in ks if "search_wide_merge_kernel" in k]) == 1 and len(ks) == 5, sorted(ks)
    assert {k: v for k, v in ks.items() if v[:2] != (0, 0)} == {}


def test_python_surface_refuses_before_the_device():
    import torch
    before = _lib.launch_count()
    with pytest.raises(ValueError, match="unknown operands"):
        search.topk(None, None, 100, operands="fp4")
    rows = search.Mx8Rows(torch.zeros(4, 128, dtype=torch.uint8), torch.zeros(4, 4, dtype=torch.uint8))
    for operands in (None, "bf16"):
        with pytest.raises(ValueError, match="Mx8Rows operand is searched with"):
            search.topk(rows, rows, 100, operands=operands)
    assert _lib.launch_count() == before
