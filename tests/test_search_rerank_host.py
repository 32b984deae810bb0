"""The second stage of the streamed search (csrc/search_rerank.hip: exact scores of a candidate list per query row) without a GPU: header, binding and ABI
number of the two entry points; every refusal of the envelope before any launch (NULL or never-dereferenced addresses: a launch would fault, a refusal
returns); no scratch in the kernels; what lpi_amd.search.rerank / topk_reranked refuse before they touch the device."""
import pytest

import search_meta as M
from lpi_amd import _lib, search
from search_meta import EINVAL

_I, _P = _lib._I, _lib._P


def _params(hdr, name):
    ret, argtypes = M.params(hdr, name)
    assert ret == "int", name
    return argtypes


def test_header_binding_and_abi():
    hdr = M.header()
    f32 = [_I, _I, _I, _P, _I, _P, _I, _P, _I, _I, _I, _P, _P, _P]      # nq ng E Q ldq G ldg cand ldc kc k idx val stream
    assert _params(hdr, "lpi_search_rerank") == _lib.SIGNATURES["lpi_search_rerank"] == f32
    assert _params(hdr, "lpi_search_rerank_t") == _lib.SIGNATURES["lpi_search_rerank_t"] == [_I] + f32
    for name in ("lpi_search_rerank", "lpi_search_rerank_t"):
        assert hasattr(_lib.load(), name) and name not in _lib._RESTYPES
    assert M.abi_version() == _lib.EXPECTED_ABI > 620
    assert _lib.load().lpi_version() == _lib.EXPECTED_ABI


def test_every_refusal_returns_before_any_launch():
    lib = _lib.load()
    before = _lib.launch_count()
    A = 1 << 20      # an aligned non-NULL address that is never dereferenced: every case below is refused on the host

    def call(form, nq=300, ng=4133, E=512, Q=A, ldq=None, G=A, ldg=None, cand=A, ldc=None, kc=100, k=10, idx=A, val=A, dt=_lib.BF16):
        ldq, ldg, ldc = E if ldq is None else ldq, E if ldg is None else ldg, kc if ldc is None else ldc
        args = (nq, ng, E, Q, ldq, G, ldg, cand, ldc, kc, k, idx, val, None)
        return lib.lpi_search_rerank(*args) if form == "f32" else lib.lpi_search_rerank_t(dt, *args)

    shared = [dict(nq=0), dict(nq=-3), dict(ng=0), dict(ng=-1), dict(E=0), dict(E=8), dict(E=1040), dict(E=2048), dict(ldq=496), dict(ldg=496),
              dict(Q=A + 4), dict(G=A + 8), dict(Q=None), dict(G=None), dict(cand=None), dict(idx=None), dict(val=None),
              dict(kc=0), dict(kc=-1), dict(kc=257, k=10), dict(k=0), dict(k=-1), dict(k=101), dict(kc=1, k=2), dict(kc=256, k=257), dict(ldc=99),
              dict(kc=256, k=256, ldc=255)]
    per_form = {"f32": [dict(E=24), dict(E=520), dict(ldq=514), dict(ldg=513), dict(ldq=515)],
                "t": [dict(E=16), dict(E=48), dict(E=528), dict(ldq=516), dict(ldg=514), dict(ldq=513)]}
    for form, extra in per_form.items():
        assert call(form, Q=None, G=None, cand=None, idx=None, val=None, nq=0) == EINVAL
        for kw in shared + extra:
            assert call(form, **kw) == EINVAL, (form, kw)
            none = dict(kw, **{p: None for p in ("Q", "G", "cand", "idx", "val") if p not in kw})      # the refusals hold with NULL operands too
            assert call(form, **none) == EINVAL, (form, kw)
    for dt in (_lib.F16,):
        assert call("t", dt=dt, E=48) == EINVAL and call("t", dt=dt, k=101) == EINVAL
    for dt in (_lib.MX8, _lib.F32X3, -1, 99):
        assert call("t", dt=dt) == EINVAL, dt
    assert call("t", dt=_lib.F32, E=24) == EINVAL and call("t", dt=_lib.F32, Q=None) == EINVAL      # forwarded to the f32 form: its envelope
    assert call("t", dt=_lib.F32, E=48, Q=None) == EINVAL      # E = 48 is inside the f32 envelope: the NULL pointer is what is refused
    assert _lib.launch_count() == before


def test_rerank_kernels_use_no_scratch(tmp_path):
    """.private_segment_fixed_size == 0 and no VGPR spill for every kernel of search_rerank.hip: one per operand type (f32, bf16, f16)."""
    if not M.have_objects("search_rerank.o"):
        pytest.skip("search_rerank.o not built (run __graft_entry__.build()) or llvm-objdump not available")
    ks = M.kernels(M.obj_path("search_rerank.o"), tmp_path)
    assert len(ks) == 3 and all("search_rerank_kernel" in k for k in ks), sorted(ks)
    assert {k: v for k, v in ks.items() if v[:2] != (0, 0)} == {}


def test_python_surface_refuses_before_the_device():
    import torch
    before = _lib.launch_count()
    q, g = torch.zeros(4, 128), torch.zeros(300, 128)
    cand = torch.zeros(4, 20, dtype=torch.int32)
    rows = search.Mx8Rows(torch.zeros(300, 128, dtype=torch.uint8), torch.zeros(300, 4, dtype=torch.uint8))
    with pytest.raises(ValueError, match="not a re-rank type"):
        search.rerank(q, g, cand, operands="mx8")
    with pytest.raises(ValueError, match="not a re-rank type"):
        search.rerank(q, rows, cand)
    with pytest.raises(ValueError, match="not a re-rank type"):
        search.rerank(search.Mx8Rows(rows.codes[:4], rows.scales[:4]), g, cand, operands="bf16")
    with pytest.raises(ValueError, match="unknown operands"):
        search.rerank(q, g, cand, operands="fp4")
    with pytest.raises(ValueError, match="<= k <= kc"):
        search.rerank(q, g, cand, 21)
    with pytest.raises(ValueError, match="<= k <= kc"):
        search.rerank(q, g, cand, 0)
    with pytest.raises(ValueError, match="candidates per row"):
        search.rerank(q, g, torch.zeros(4, 257, dtype=torch.int32))
    with pytest.raises(ValueError, match="candidates per row"):
        search.rerank(q, g, torch.zeros(4, 0, dtype=torch.int32))
    with pytest.raises(ValueError, match="cand has 5 rows"):
        search.rerank(q, g, torch.zeros(5, 20, dtype=torch.int32))
    with pytest.raises(ValueError, match="integer tensor"):
        search.rerank(q, g, torch.zeros(4, 20))
    with pytest.raises(ValueError, match="features"):
        search.rerank(q, torch.zeros(300, 64), cand)
    for kw in (dict(candidates=9), dict(candidates=257), dict(candidates=0)):
        with pytest.raises(ValueError, match="<= candidates <="):
            search.topk_reranked(q, g, 10, **kw)
    with pytest.raises(ValueError, match="<= candidates <="):
        search.topk_reranked(q, g[:15], 10, candidates=16)      # more candidates than gallery rows
    with pytest.raises(ValueError, match="<= candidates <="):
        search.topk_reranked(q, g[:8], 10)                      # the default is clipped to ng, which is below k
    with pytest.raises(ValueError, match="not \"mx8\""):
        search.topk_reranked(q, g, 10, operands="mx8")
    with pytest.raises(ValueError, match="unknown operands"):
        search.topk_reranked(q, g, 10, coarse="fp4")
    assert _lib.launch_count() == before
