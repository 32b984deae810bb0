"""The streamed search (csrc/search.hip, lpi_amd/search.py) without a GPU: header, binding and ABI number; the workspace function; every refusal of the
envelope before any launch (NULL device pointers: a launch would fault, a refusal returns); no scratch in the new kernels; the plugin's eval_scores key."""
import json
import os

import pytest

import search_meta as M
from lpi_amd import _lib
from search_meta import EINVAL, REPO

_I, _P, _L = _lib._I, _lib._P, _lib._L


def test_header_binding_and_abi():
    want = {
        "lpi_search_workspace": ("long", [_I, _I, _I]),
        "lpi_search_topk": ("int", [_I, _I, _I, _P, _I, _P, _I, _I, _I, _I, _P, _P, _P, _L, _P]),
        "lpi_search_rank": ("int", [_I, _I, _I, _P, _I, _P, _I, _P, _I, _P, _P, _L, _P]),
    }
    hdr = M.header()
    for name, (ret, argtypes) in want.items():
        assert _lib.SIGNATURES[name] == argtypes, name
        assert M.params(hdr, name) == (ret, argtypes), name
    assert _lib._RESTYPES["lpi_search_workspace"] is _L
    assert M.abi_version() == _lib.EXPECTED_ABI >= 614
    assert _lib.load().lpi_version() == _lib.EXPECTED_ABI


def test_workspace_is_positive_and_monotone():
    ws = _lib.load().lpi_search_workspace
    nqs = (1, 5, 127, 128, 129, 300, 2048, 5000, 25000, 123287)
    ngs = (1, 16, 127, 129, 4133, 25000, 65536, 70001, 616767)
    for k in (0, 1, 5, 10, 16):
        table = [[ws(nq, ng, k) for ng in ngs] for nq in nqs]
        for a, row in enumerate(table):
            for b, v in enumerate(row):
                assert v > 0, (nqs[a], ngs[b], k)
                assert b == 0 or v >= row[b - 1], ("ng", nqs[a], ngs[b], k)
                assert a == 0 or v >= table[a - 1][b], ("nq", nqs[a], ngs[b], k)
    for nq in nqs:
        for ng in ngs:
            sizes = [ws(nq, ng, k) for k in range(1, 17)]
            assert sizes == sorted(sizes), (nq, ng)
    assert ws(5000, 25000, 0) == 8 * 5000      # the rank form: a threshold and an index per query row
    assert ws(2048, 65536, 16) < 2048 * 65536 * 4 // 8      # nowhere near the matrix
    for bad in ((0, 5, 1), (5, 0, 1), (-1, 5, 1), (5, 5, -1), (5, 5, 17)):
        assert ws(*bad) == EINVAL, bad


def test_every_refusal_returns_before_any_launch():
    """Shapes and strides outside the envelope with NULL operands: LPI_EINVAL comes back and nothing was launched.  Then a valid envelope with each
    required pointer missing, misaligned operands, and a workspace one byte short."""
    lib = _lib.load()
    before = _lib.launch_count()
    A = 1 << 20      # an aligned non-NULL address that is never dereferenced: every case below is refused on the host

    def topk(nq=300, ng=4133, E=512, Q=A, ldq=None, G=A, ldg=None, k=10, col_base=0, acc=0, idx=A, val=A, ws=A, ws_bytes=None):
        ldq, ldg = E if ldq is None else ldq, E if ldg is None else ldg
        if ws_bytes is None:
            ws_bytes = max(1, lib.lpi_search_workspace(max(nq, 1), max(ng, 1), min(max(k, 1), 16)))
        return lib.lpi_search_topk(nq, ng, E, Q, ldq, G, ldg, k, col_base, acc, idx, val, ws, ws_bytes, None)

    def rank(nq=300, ng=4133, E=512, Q=A, ldq=None, G=A, ldg=None, gt=A, gpr=5, out=A, ws=A, ws_bytes=None):
        ldq, ldg = E if ldq is None else ldq, E if ldg is None else ldg
        if ws_bytes is None:
            ws_bytes = max(1, lib.lpi_search_workspace(max(nq, 1), max(ng, 1), 0))
        return lib.lpi_search_rank(nq, ng, E, Q, ldq, G, ldg, gt, gpr, out, ws, ws_bytes, None)

    shared = [dict(nq=0), dict(nq=-3), dict(ng=0), dict(ng=-1), dict(E=0), dict(E=8), dict(E=24), dict(E=520), dict(E=1040), dict(E=2048),
              dict(ldq=496), dict(ldg=496), dict(ldq=514), dict(ldg=513), dict(ldq=515),
              dict(Q=None), dict(G=None), dict(Q=A + 4), dict(G=A + 8), dict(ws=None), dict(ws=A + 2)]
    for kw in shared:
        none = dict(kw, **{p: None for p in ("Q", "G", "ws") if p not in kw})      # the refusals of shape hold with NULL operands too
        assert topk(**kw) == EINVAL, ("topk", kw)
        assert rank(**kw) == EINVAL, ("rank", kw)
        assert topk(**none, idx=None, val=None) == EINVAL and rank(**none, gt=None, out=None) == EINVAL, kw
    for kw in (dict(k=0), dict(k=-1), dict(k=17), dict(k=16, ng=15), dict(col_base=-1), dict(col_base=2**31 - 100), dict(idx=None), dict(val=None),
               dict(ws_bytes=lib.lpi_search_workspace(300, 4133, 10) - 1), dict(ws_bytes=0)):
        assert topk(**kw) == EINVAL, kw
    for kw in (dict(gt=None), dict(gpr=0), dict(gpr=-2), dict(out=None), dict(ws_bytes=8 * 300 - 1), dict(ws_bytes=0)):
        assert rank(**kw) == EINVAL, kw
    assert _lib.launch_count() == before


def test_search_kernels_use_no_scratch(tmp_path):
    """.private_segment_fixed_size == 0 for every kernel of search.hip (a scratch reload's vmcnt(0) would drain the staged tile in flight; parsed as
    tests/test_no_spills.py does)."""
    if not M.have_objects("search.o"):
        pytest.skip("search.o not built (run __graft_entry__.build()) or llvm-objdump not available")
    ks = M.kernels(M.obj_path("search.o"), tmp_path)
    assert len([k for k in ks if "search_kernel" in k]) == 3 and len([k for k in ks if "search_merge_kernel" in k]) == 1, sorted(ks)
    assert {k: v for k, v in ks.items() if v[:2] != (0, 0)} == {}


def test_eval_scores_key_is_validated_at_construction():
    from lpi_amd.retrieval.methods import sprompt
    assert sprompt._eval_scores({}) == "matrix"      # the default does not change
    assert sprompt._eval_scores({"eval_scores": "streamed"}) == "streamed"
    args = json.load(open(os.path.join(REPO, "lpi_amd", "retrieval", "configs", "lpi", "coco_lpi.json")))
    assert "eval_scores" not in args
    for bad in ("stream", "", None, 1, "Matrix"):
        with pytest.raises(ValueError, match="eval_scores"):
            sprompt.SPrompts(dict(args, eval_scores=bad))      # raised before the network is built: nothing touches a device
