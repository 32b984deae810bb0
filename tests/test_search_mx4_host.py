"""The streamed search on MX-FP4 operands (csrc/search_mx4.hip, mx4_rows.hip, search_tile.h; lpi_amd.search `operands="mx4"`, Mx4Rows, quantize_mx4) without
a GPU: the emulator's own rules (tests/mx4_emulate.py is the format's definition); header, binding and ABI number of the three entry points; every refusal
of their envelopes before any launch (aligned addresses that are never dereferenced: a launch would fault, a refusal returns); the kernels of
search_mx4.o and mx4_rows.o, none with scratch or spills beyond the family's; Mx4Rows' validation and the wrapper's refusals (MX-FP4 is a coarse top-k
type: no rank form, no re-rank form, not a plugin value); the default candidate counts of topk_reranked."""
import re

import numpy as np
import pytest
import torch

import mx4_emulate as MX4
import search_meta as M
from lpi_amd import _lib
from search_meta import A, EINVAL

_I, _P, _L = _lib._I, _lib._P, _lib._L


# ---------------------------------------------------------------------------------------------------------------- the emulator
def _q1(values, amax=4.0):
    """one block whose first elements are `values` and whose maximum is `amax` (4.0: biased exponent 129, byte 127, scale 1) -> the elements' codes"""
    y = torch.zeros(32)
    y[:len(values)] = torch.tensor(values, dtype=torch.float32)
    y[31] = amax
    q, s = MX4.quantize(y[None])
    return MX4.unpack(q)[0, :len(values)].tolist(), int(s[0, 0])


def test_emulator_codes_rounding_saturation_and_zero_block():
    # every code decodes to its grid value, the sign bit is bit 3
    got = MX4.decode(torch.arange(16, dtype=torch.uint8)).tolist()
    assert got == [0, 0.5, 1, 1.5, 2, 3, 4, 6, -0.0, -0.5, -1, -1.5, -2, -3, -4, -6]
    # the grid is a fixed point, with scale 1 (amax 4 -> Eb 129 -> byte 127)
    codes, byte = _q1([0, 0.5, 1, 1.5, 2, 3, 4, -0.5, -1, -1.5, -2, -3, -4])
    assert byte == 127 and codes == [0, 1, 2, 3, 4, 5, 6, 9, 10, 11, 12, 13, 14]
    # round to nearest EVEN at every midpoint: 0.25 -> 0, 0.75 -> 1, 1.25 -> 1, 1.75 -> 2, 2.5 -> 2, 3.5 -> 4 (and 5 -> 4 below, where amax allows it)
    codes, _ = _q1([0.25, 0.75, 1.25, 1.75, 2.5, 3.5, -0.25, -0.75, -2.5, -3.5])
    assert codes == [0, 2, 2, 4, 4, 6, 8, 10, 12, 14]
    # just off the midpoints: to the nearer neighbour
    codes, _ = _q1([0.2500001, 0.7499999, 2.4999998, 2.5000002, 3.4999998])
    assert codes == [1, 1, 4, 5, 5]
    # amax in [4, 8) has byte 127 too: 5 is the midpoint of 4 and 6 -> 4 (even); (6, 8) saturates to 6; 7 would round to 8: 6
    for amax, want in ((5.0, 6), (5.0000005, 7), (6.0, 7), (6.5, 7), (7.0, 7), (7.9999995, 7)):
        codes, byte = _q1([amax, -amax], amax)
        assert byte == 127 and codes == [want, want | 8], amax
    # the scale rule: byte = Eb - 2 = floor(log2 amax) + 125; a zero block is byte 0 and zero codes; a subnormal maximum too; tiny normal maxima clamp at 0
    for amax, want in ((1.0, 125), (1.9999999, 125), (2.0, 126), (0.75, 124), (2.0 ** -100, 25), (2.0 ** 100, 225), (2.0 ** -125, 0), (2.0 ** -126, 0)):
        assert _q1([], amax)[1] == want, amax
    q, s = MX4.quantize(torch.zeros(2, 64))
    assert int(s.max()) == 0 and int(q.max()) == 0
    q, s = MX4.quantize(torch.full((1, 32), 2.0 ** -140))
    assert int(s.max()) == 0 and int(q.max()) == 0                      # 2^-140 2^127 = 2^-13: rounds to zero
    # nibble order: element 2 j is the low nibble of byte j
    y = torch.zeros(1, 32)
    y[0, 0], y[0, 1], y[0, 31] = 1.0, -2.0, 4.0
    q, _ = MX4.quantize(y)
    assert int(q[0, 0]) == (12 << 4 | 2) and int(q[0, 15]) == 6 << 4
    # dequantize inverts quantize on representable rows, blocks scaled separately
    gen = torch.Generator().manual_seed(3)
    codes = torch.randint(0, 16, (7, 96), generator=gen).to(torch.uint8)
    codes[:, 31::32] = 7                                                # the block maximum is 6: byte = scale byte below, nothing saturates or shifts
    sb = torch.randint(100, 150, (7, 3), generator=gen).to(torch.uint8)
    vals = (MX4.decode(codes).reshape(7, 3, 32) * MX4.scale_values(sb)[..., None]).reshape(7, 96)
    q, s = MX4.quantize(vals.float())
    assert torch.equal(s, sb) and torch.equal(MX4.dequantize(q, s), vals)
    assert torch.equal(MX4.unpack(q) & 7, codes & 7)


def test_integer_reference_has_ties_at_every_list_length():
    """From the reference alone: at (300, 4133, 512), the seed tests/test_search_mx4_gpu.py uses, at least half the rows have equal scores at positions k - 1
    and k for every k tested there, so the integer test does test the tie order (index descending) at every list length."""
    from mx4_cases import int_case, tie_shares
    _, _, _, _, s, order = int_case(300, 4133, 512, 300 * 1000 + 512)
    shares = tie_shares(s, order)
    print(shares)
    assert sorted(shares) == [1, 16, 17, 100, 256] and min(shares.values()) >= 0.5, shares
    assert len(np.unique(s)) > 100      # and the scores are not all alike


# ---------------------------------------------------------------------------------------------------------------- header, binding, ABI
def test_header_binding_and_abi():
    topk = [_I, _I, _I, _P, _I, _P, _I, _P, _I, _P, _I, _I, _I, _I, _P, _P, _P, _L, _P]
    want = {"lpi_search_topk_mx4": topk, "lpi_search_topk_wide_mx4": topk, "lpi_mx4_quantize": [_I, _I, _I, _P, _I, _P, _I, _P, _I, _P]}
    hdr = M.header()
    for name, argtypes in want.items():
        assert _lib.SIGNATURES[name] == argtypes, name
        assert _lib.SIGNATURES[name.replace("mx4", "mx8")] == argtypes, name                     # the MX-FP8 calls' signatures
        assert M.params(hdr, name) == ("int", argtypes), name
    assert re.search(r"#define LPI_MX4 (\d+)", hdr).group(1) == str(_lib.MX4)
    assert _lib.MX4 not in (_lib.F32, _lib.BF16, _lib.F16, _lib.MX8, _lib.F32X3)
    assert M.abi_version() == _lib.EXPECTED_ABI >= 622
    lib = _lib.load()
    assert lib.lpi_version() == _lib.EXPECTED_ABI
    assert all(hasattr(lib, n) for n in want)
    assert not hasattr(lib, "lpi_search_rank_mx4")


# ---------------------------------------------------------------------------------------------------------------- C-ABI refusals
def _topk_call(lib, wide):
    fn = lib.lpi_search_topk_wide_mx4 if wide else lib.lpi_search_topk_mx4
    wsfn = lib.lpi_search_wide_workspace if wide else lib.lpi_search_workspace
    kmax = 256 if wide else 16

    def topk(nq=300, ng=4133, E=512, Q=A, ldq=None, Qs=A, ldqs=None, G=A, ldg=None, Gs=A, ldgs=None, k=10, col_base=0, acc=0, idx=A, val=A, ws=A,
             ws_bytes=None):
        ldq, ldg = (E // 2 if v is None else v for v in (ldq, ldg))
        ldqs, ldgs = (E // 32 if v is None else v for v in (ldqs, ldgs))
        if ws_bytes is None:
            ws_bytes = max(1, wsfn(max(nq, 1), max(ng, 1), min(max(k, 1), kmax)))
        return fn(nq, ng, E, Q, ldq, Qs, ldqs, G, ldg, Gs, ldgs, k, col_base, acc, idx, val, ws, ws_bytes, None)

    return topk, wsfn, kmax


@pytest.mark.parametrize("wide", [False, True])
def test_every_search_refusal_returns_before_any_launch(wide):
    lib = _lib.load()
    before = _lib.launch_count()
    topk, wsfn, kmax = _topk_call(lib, wide)
    cases = ([dict(nq=0), dict(nq=-3), dict(ng=0), dict(ng=-1), dict(ws=None), dict(ws=A + 2)]
             + [dict(E=E) for E in (0, -128, 32, 64, 96, 160, 192, 320, 1152, 2048)]                     # E (elements) a multiple of 128, <= 1024
             + [dict(ldq=256 - 16), dict(ldg=256 - 16), dict(ldq=256 + 8), dict(ldg=256 + 8), dict(ldq=256 + 1), dict(ldg=256 + 4)]      # bytes: >= E / 2, multiples of 16
             + [dict(ldqs=16 - 4), dict(ldgs=16 - 4), dict(ldqs=16 + 2), dict(ldgs=16 + 2), dict(ldqs=16 + 1), dict(ldgs=16 + 3)]        # >= E / 32, multiples of 4
             + [dict(Q=A + 8), dict(G=A + 8), dict(Q=A + 4), dict(Qs=A + 2), dict(Gs=A + 2), dict(Gs=A + 1)]      # 16-byte / 4-byte aligned bases
             + [dict(Q=None), dict(Qs=None), dict(G=None), dict(Gs=None)]                                # no NULL operand or scale pointer
             + [dict(k=0), dict(k=-1), dict(k=kmax + 1), dict(k=kmax, ng=kmax - 1), dict(col_base=-1), dict(col_base=2**31 - 100), dict(idx=None),
                dict(val=None), dict(ws_bytes=wsfn(300, 4133, 10) - 1), dict(ws_bytes=0)])
    for kw in cases:
        assert topk(**kw) == EINVAL, kw
        none = dict(kw, **{p: None for p in ("Q", "Qs", "G", "Gs", "ws", "idx", "val") if p not in kw})      # the refusals hold with NULL pointers too
        assert topk(**none) == EINVAL, kw
    assert _lib.launch_count() == before


def test_quantize_refusals_return_before_any_launch():
    lib = _lib.load()
    before = _lib.launch_count()

    def quant(dt=_lib.F32, rows=8, K=256, x=A, ldx=None, q=A, ldq=None, sc=A, lds=None):
        return lib.lpi_mx4_quantize(dt, rows, K, x, K if ldx is None else ldx, q, K // 2 if ldq is None else ldq, sc, K // 32 if lds is None else lds, None)

    for kw in ([dict(rows=0), dict(rows=-1), dict(K=0), dict(K=-32), dict(K=16), dict(K=48), dict(K=250), dict(x=None), dict(q=None), dict(sc=None)]
               + [dict(ldx=252), dict(ldx=258), dict(ldq=124), dict(ldq=130), dict(ldq=129), dict(lds=7)]      # ldx >= K in 4s; ldq >= K / 2 in 4s; lds >= K / 32
               + [dict(q=A + 2), dict(q=A + 1), dict(x=A + 8), dict(x=A + 4, dt=_lib.BF16), dict(x=A + 4, dt=_lib.F16), dict(x=A + 2, dt=_lib.BF16)]
               + [dict(dt=_lib.MX8), dict(dt=_lib.MX4), dict(dt=_lib.F32X3), dict(dt=-1), dict(dt=17)]):
        assert quant(**kw) == EINVAL, kw
    assert _lib.launch_count() == before


def test_typed_entry_points_refuse_the_mx4_code():
    """lpi_search_topk_t, lpi_search_topk_wide_t, lpi_search_rank_t and lpi_search_rerank_t refuse LPI_MX4 exactly as they refuse LPI_MX8."""
    lib = _lib.load()
    before = _lib.launch_count()
    for dt in (_lib.MX4, _lib.MX8):
        assert lib.lpi_search_topk_t(dt, 300, 4133, 512, A, 512, A, 512, 10, 0, 0, A, A, A, lib.lpi_search_workspace(300, 4133, 10), None) == EINVAL
        assert lib.lpi_search_topk_wide_t(dt, 300, 4133, 512, A, 512, A, 512, 100, 0, 0, A, A, A, lib.lpi_search_wide_workspace(300, 4133, 100), None) == EINVAL
        assert lib.lpi_search_rank_t(dt, 300, 4133, 512, A, 512, A, 512, A, 5, A, A, lib.lpi_search_workspace(300, 4133, 0), None) == EINVAL
        assert lib.lpi_search_rerank_t(dt, 300, 4133, 512, A, 512, A, 512, A, 40, 40, 10, A, A, None) == EINVAL
    assert _lib.launch_count() == before


# ---------------------------------------------------------------------------------------------------------------- the objects
def test_mx4_kernels_use_no_scratch(tmp_path):
    """search_mx4.o holds exactly the two MX-FP4 tile kernels (narrow top-k = mode 0, wide = mode 3; no rank or threshold form, and neither merge kernel:
    they are search.o's and search_wide.o's); mx4_rows.o the three quantisers.  No kernel has a private segment or a VGPR spill.  The narrow sweep and the
    quantisers spill no SGPR either; the wide sweep parks SGPRs in VGPR lanes (no memory), as every wide sweep of search_wide.o does: DESIGN.md has the
    table."""
    names = ("search_mx4.o", "mx4_rows.o", "search_wide.o")
    if not M.have_objects(*names):
        pytest.skip("the objects are not built (run __graft_entry__.build()) or llvm-objdump is not available")
    objs = [M.obj_path(n) for n in names]
    ks = M.kernels(objs[0], tmp_path)
    assert len(ks) == 2 and all("search_kernel" in k for k in ks), sorted(ks)
    assert sorted(re.search(r"search_kernelI5mx4_tLi(\d)E", k).group(1) for k in ks) == ["0", "3"], sorted(ks)
    assert all(v[:2] == (0, 0) for v in ks.values()), ks
    assert [v for k, v in ks.items() if "Li0E" in k] == [(0, 0, 0)], ks
    rows = M.kernels(objs[1], tmp_path)
    assert len(rows) == 3 and all("mx4_quantize_kernel" in k for k in rows), sorted(rows)
    assert set(rows.values()) == {(0, 0, 0)}, rows
    assert not [k for k in M.kernels(objs[2], tmp_path) if "mx4" in k]      # search_wide.o keeps its five kernels


# ---------------------------------------------------------------------------------------------------------------- Mx4Rows and the wrapper
def _rows(n=8, E=256):
    return torch.zeros(n, E // 2, dtype=torch.uint8), torch.zeros(n, 4 * ((E // 32 + 3) // 4), dtype=torch.uint8)[:, :E // 32]


def test_mx4rows_is_validated():
    from lpi_amd import search
    before = _lib.launch_count()
    c, s = _rows()
    r = search.Mx4Rows(c, s)
    assert tuple(r.shape) == (8, 256) and r.nbytes == 8 * 128 + 8 * 8 and len(r) == 8 and r.device == c.device
    with pytest.raises(AttributeError):
        r.codes = c
    with pytest.raises(AttributeError):
        r.other = 1
    v = r[2:5]
    assert isinstance(v, search.Mx4Rows) and tuple(v.shape) == (3, 256)
    assert v.codes.data_ptr() == c[2:5].data_ptr() and v.scales.data_ptr() == s[2:5].data_ptr()      # views
    assert r[3:].nbytes == 5 * 128 + 5 * 8
    with pytest.raises(TypeError):
        r[::2]
    with pytest.raises(TypeError):
        r[1]
    wide_c, wide_s = torch.zeros(8, 128 + 16, dtype=torch.uint8), torch.zeros(8, 8 + 4, dtype=torch.uint8)
    w = search.Mx4Rows(wide_c[:, :128], wide_s[:, :8])                                 # strided rows are fine: 16-byte / 4-byte row strides
    assert w.nbytes == r.nbytes                                                         # gaps are not counted
    bad = [
        (c.float(), s), (c, s.to(torch.int8)),                                          # dtype
        (c[0], s), (c, s[0]), (c[None], s),                                             # dims
        (c, s[:, :7]), (c[:4], s), (c[:, :120], s), (c, torch.zeros(8, 4, dtype=torch.uint8)),      # shapes: scales [n, E / 32] with E = 2 x the code bytes
        (torch.zeros(8, 0, dtype=torch.uint8), torch.zeros(8, 0, dtype=torch.uint8)),
        (torch.zeros(8, 256, dtype=torch.uint8)[:, ::2], s),                            # inner stride
        (torch.zeros(8, 128 + 8, dtype=torch.uint8)[:, :128], s),                       # row stride of the codes not 16 bytes
        (c, torch.zeros(8, 8 + 2, dtype=torch.uint8)[:, :8]),                           # row stride of the scales not 4 bytes
        (torch.zeros(8 * 128 + 8, dtype=torch.uint8)[8:].view(8, 128), s),              # base of the codes
        (c, torch.zeros(8 * 8 + 2, dtype=torch.uint8)[2:].view(8, 8)),                  # base of the scales
        (c.numpy(), s),                                                                 # not a tensor
    ]
    for cc, ss in bad:
        with pytest.raises(ValueError, match="Mx4Rows"):
            search.Mx4Rows(cc, ss)
    assert tuple(search.Mx4Rows(*_rows(4, 384)).shape) == (4, 384)
    assert _lib.launch_count() == before


def test_wrapper_refusals():
    """All on CPU tensors: every refusal comes before any launch."""
    from lpi_amd import search
    from lpi_amd.retrieval.methods import sprompt
    before = _lib.launch_count()
    assert search._operands("mx4") == "mx4"
    r4 = search.Mx4Rows(*_rows())
    r8 = search.Mx8Rows(torch.zeros(8, 256, dtype=torch.uint8), torch.zeros(8, 8, dtype=torch.uint8))
    f = torch.zeros(8, 256)
    gt = torch.zeros(8, dtype=torch.int32)
    cand = torch.zeros(8, 4, dtype=torch.int32)
    # "mx4" passes the name check: what raises next is the operand itself (None is no tensor)
    with pytest.raises(Exception) as ei:
        search.topk(None, None, 10, operands="mx4")
    assert "unknown operands" not in str(ei.value)
    # "fp4" and friends stay unknown, and the message lists the names
    for bad in ("fp4", "MX4", "mxfp4", "e2m1"):
        with pytest.raises(ValueError, match=r"unknown operands .*f32 \| bf16 \| f16 \| mx8 \| mx4"):
            search.topk(f, f, 1, operands=bad)
        with pytest.raises(ValueError, match="unknown operands"):
            search.topk_reranked(f, f, 1, coarse=bad)
    # an Mx4Rows goes with "mx4" only, an Mx8Rows never with "mx4"
    for ops in (None, "f32", "bf16", "f16", "mx8"):
        with pytest.raises(ValueError, match="Mx4Rows"):
            search.topk(r4, r4, 1, operands=ops)
        with pytest.raises(ValueError, match="Mx4Rows"):
            search.topk(f, r4, 1, operands=ops)
    for q, g in ((r8, r8), (r4, r8), (r8, r4), (f, r8)):
        with pytest.raises(ValueError, match="Mx8Rows"):
            search.topk(q, g, 1, operands="mx4")
    with pytest.raises(ValueError, match="Mx4Rows"):
        search.topk(r4, r8, 1, operands="mx8")
    # no rank form
    for q, g, ops in ((f, f, "mx4"), (r4, r4, "mx4"), (f, r4, None), (r4, f, "bf16"), (r4, r4, "mx8")):
        with pytest.raises(ValueError):
            search.gt_rank(q, g, gt, operands=ops)
    # no re-rank form; the message keeps its words
    for q, g, ops in ((f, f, "mx4"), (r4, f, None), (f, r4, None), (f, r4, "bf16")):
        with pytest.raises(ValueError, match="not a re-rank type"):
            search.rerank(q, g, cand, operands=ops)
    with pytest.raises(ValueError, match="not a re-rank type"):
        search.rerank(f, f, cand, operands="mx8")
    for ops in ("mx4", "mx8"):
        with pytest.raises(ValueError, match="re-rank operands"):
            search.topk_reranked(f, f, 1, coarse="mx4", operands=ops)
    # E: a multiple of 128
    for E in (64, 160, 192):
        with pytest.raises(ValueError, match="128"):
            search.topk(search.Mx4Rows(*_rows(4, E)), search.Mx4Rows(*_rows(4, E)), 1, operands="mx4")
    with pytest.raises(ValueError, match="features"):
        search.topk(search.Mx4Rows(*_rows(4, 128)), search.Mx4Rows(*_rows(4, 256)), 1, operands="mx4")
    # the plugin's key does not know it
    with pytest.raises(ValueError, match="eval_search_operands"):
        sprompt._eval_search_operands({"eval_scores": "streamed", "eval_search_operands": "mx4"})
    assert sprompt._eval_search_operands({"eval_scores": "streamed", "eval_search_operands": "mx8"}) == "mx8"
    assert _lib.launch_count() == before


def test_default_candidate_counts(monkeypatch):
    """coarse="mx4": min(ng, 256, max(16 k, 128)); the other coarse types keep min(ng, 256, max(4 k, 32)); an explicit count is used as given."""
    from lpi_amd import search
    seen = []

    class Stop(Exception):
        pass

    def fake_topk(cq, cg, candidates, *, operands=None, **kw):
        seen.append((operands, candidates))
        raise Stop

    monkeypatch.setattr(search, "topk", fake_topk)
    f = torch.zeros(3, 128)

    def default(coarse, ng, k, **kw):
        with pytest.raises(Stop):
            search.topk_reranked(f, torch.zeros(ng, 128), k, coarse=coarse, **kw)
        return seen[-1]

    assert default("mx4", 5000, 1) == ("mx4", 128)
    assert default("mx4", 5000, 8) == ("mx4", 128)
    assert default("mx4", 5000, 10) == ("mx4", 160)
    assert default("mx4", 5000, 16) == ("mx4", 256)
    assert default("mx4", 5000, 100) == ("mx4", 256)
    assert default("mx4", 100, 10) == ("mx4", 100)
    assert default("mx4", 5000, 10, candidates=16) == ("mx4", 16)
    for coarse in ("mx8", "bf16", "f16"):
        assert default(coarse, 5000, 1) == (coarse, 32)
        assert default(coarse, 5000, 10) == (coarse, 40)
        assert default(coarse, 5000, 100) == (coarse, 256)
        assert default(coarse, 20, 10) == (coarse, 20)
    with pytest.raises(ValueError, match="candidates"):
        search.topk_reranked(f, torch.zeros(5000, 128), 10, coarse="mx4", candidates=9)
    with pytest.raises(ValueError, match="candidates"):
        search.topk_reranked(f, torch.zeros(5000, 128), 10, coarse="mx4", candidates=257)
