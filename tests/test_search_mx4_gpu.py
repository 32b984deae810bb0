"""lpi_mx4_quantize, lpi_search_topk_mx4 and lpi_search_topk_wide_mx4 (csrc/mx4_rows.hip, search_mx4.hip) on a real MI355X, held to the CPU restatement of the
MX-FP4 format (tests/mx4_emulate.py): the quantiser bit for bit; integer data with per-block scales where every summation order agrees (ties included: the
test of the operand lane map, the nibble and scale bytes, the two k steps of a slab, the shortened last slab, the edges and the order); float data
against the f64 product of the DEQUANTISED operands under a measured tolerance capped by the project's bar for the block-scaled instruction; narrow
against wide and chunked against whole, bit for bit; strided operands with poisoned gaps and guarded outputs; the two-stage search end to end, where the
reference alone shows that the coarse lists must hold the f32 top 10; and the Python wrapper (an Mx4Rows is read in place)."""
import functools

import numpy as np
import pytest
import torch

import mx4_emulate as MX4
from mx4_cases import KS, int_case as _int_case, tie_shares
from lpi_amd import _lib

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CANARY_I, CANARY_F = -0x5A5A5A5B, -12345.5
KNARROW = 16
SHAPES = [(1, 17, 128), (5, 40, 256), (127, 129, 384), (300, 4133, 512), (130, 300, 1024)]


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _ws_bytes(nq, ng, k, wide):
    lib = _lib.load()
    n = int(lib.lpi_search_wide_workspace(nq, ng, k) if wide else lib.lpi_search_workspace(nq, ng, k))
    assert n > 0
    return n


def c_topk(Q, Qs, G, Gs, k, wide, col_base=0, into=None):
    """the C call on code tensors [n, E / 2] and scale tensors [n, E / 32] (any row strides)"""
    nq, ng, E = Q.shape[0], G.shape[0], 2 * Q.shape[1]
    if into is None:
        idx = torch.empty(nq, k, dtype=torch.int32, device=DEV)
        val = torch.empty(nq, k, dtype=torch.float32, device=DEV)
    else:
        idx, val = into
    n = _ws_bytes(nq, ng, k, wide)
    ws = torch.empty(n, dtype=torch.uint8, device=DEV)
    _lib.call("lpi_search_topk_wide_mx4" if wide else "lpi_search_topk_mx4", nq, ng, E, Q, Q.stride(0), Qs, Qs.stride(0), G, G.stride(0), Gs, Gs.stride(0),
              k, col_base, 0 if into is None else 1, idx, val, ws, n, _stream())
    return idx, val


def _bits(t):
    return t.view(torch.int32)


# ---------------------------------------------------------------------------------------------------------------- 1. the quantiser
def _quant_input(rows, K, dtype):
    gen = torch.Generator().manual_seed(9 + rows)
    x = torch.randn(rows, K, generator=gen) * torch.exp(2 * torch.randn(rows, 1, generator=gen))
    mid = torch.tensor([0.25, 0.75, 1.25, 1.75, 2.5, 3.5, 5.0, 7.0, 6.5, 6.0, 4.0, 3.0, -0.25, -0.75, -1.25, -1.75, -2.5, -3.5, -5.0, -7.0, 0.0, -0.0, 0.125,
                        -0.125, 0.375, 1.0, 1.5, 2.0, 0.5, 7.75, -7.75, 4.5])
    x[0, :32] = mid                                   # every midpoint of the grid and the saturating range, block maximum 7.75: scale 1
    if K >= 64:
        x[1, :32] = mid * 2.0 ** -9                   # the same with another scale
        x[2, 32:64] = 0                               # a zero block: byte 0
    return x.to(dtype)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16])
@pytest.mark.parametrize("rows,K", [(300, 512), (5, 32)])
def test_quantize_mx4_is_the_emulator_bit_for_bit(rows, K, dtype):
    from lpi_amd import search
    x = _quant_input(rows, K, dtype)
    n0 = _lib.launch_count()
    r = search.quantize_mx4(x.to(DEV))
    assert _lib.launch_count() == n0 + 1      # one lpi_mx4_quantize launch
    qr, sr = MX4.quantize(x)
    assert isinstance(r, search.Mx4Rows) and tuple(r.shape) == (rows, K) and r.nbytes == rows * K // 2 + rows * K // 32
    assert torch.equal(r.scales.cpu(), sr)
    assert torch.equal(r.codes.cpu(), qr)
    if K >= 64:
        assert int(sr[2, 1]) == 0 and int(qr[2, 16:32].max()) == 0 and int(sr[0, 0]) == 127


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16])
def test_quantize_mx4_strided_rows_and_canaries(dtype):
    """a row-strided view with NaN in the gaps and in a row past the end; strided outputs whose gaps, and guards before and behind, keep their canaries"""
    rows, K, guard = 37, 96, 64
    ldx, ldq, lds = K + 8, K // 2 + 12, K // 32 + 3
    x = _quant_input(rows, K, dtype)
    xw = torch.full((rows + 1, ldx), float("nan"), dtype=dtype)
    xw[:rows, :K] = x
    xw = xw.to(DEV)
    qbuf = torch.full((guard + rows * ldq + guard,), 0xA5, dtype=torch.uint8, device=DEV)
    sbuf = torch.full((guard + rows * lds + guard,), 0xA5, dtype=torch.uint8, device=DEV)
    n0 = _lib.launch_count()
    _lib.call("lpi_mx4_quantize", {torch.float32: _lib.F32, torch.float16: _lib.F16}[dtype], rows, K, xw, ldx, qbuf[guard:], ldq, sbuf[guard:], lds, _stream())
    assert _lib.launch_count() == n0 + 1
    qr, sr = MX4.quantize(x)
    for buf, ld, w, ref in ((qbuf, ldq, K // 2, qr), (sbuf, lds, K // 32, sr)):
        buf = buf.cpu()
        assert (buf[:guard] == 0xA5).all() and (buf[guard + rows * ld:] == 0xA5).all()
        body = buf[guard:guard + rows * ld].view(rows, ld)
        assert torch.equal(body[:, :w], ref)
        assert (body[:, w:] == 0xA5).all()


# ---------------------------------------------------------------------------------------------------------------- 2. integer-exact, with ties
@pytest.mark.parametrize("nq,ng,E", SHAPES)
def test_integer_scores_exact_with_ties(nq, ng, E):
    qc, qs, gc, gs, s, order = _int_case(nq, ng, E, nq * 1000 + E)
    if (nq, ng) == (300, 4133):      # the premise, from the reference alone (tests/test_search_mx4_host.py checks it without a GPU): ties across every list's end
        assert min(tie_shares(s, order).values()) >= 0.5
    Q, Qs, G, Gs = (t.to(DEV) for t in (qc, qs, gc, gs))
    done = set()
    for k, wide in KS:
        k = min(k, ng)
        if (k, wide) in done:
            continue
        done.add((k, wide))
        idx, val = c_topk(Q, Qs, G, Gs, k, wide)
        want = order[:, :k]
        assert np.array_equal(idx.cpu().numpy(), want), (k, wide, "idx")
        assert np.array_equal(val.cpu().numpy(), np.take_along_axis(s, want, 1).astype(np.float32)), (k, wide, "val")


# ---------------------------------------------------------------------------------------------------------------- 3. float data
NQ, NG, E_F = 300, 4133, 512
# |val - s64| <= TOL * A with s64 = the f64 product of the DEQUANTISED operands and A = |q| . |g| of them.  As for MX-FP8 (tests/test_search_mx8_gpu.py) TOL is
# measured: 2 x the first measured maximum over all returned entries, and it must stay under the project's bar for this instruction, RANDOM_BAR = 8.6e-5.
# First measured maximum on an MI355X, over the top 1, 16, 17, 100 and 256 of 300 rows: MEASURED = 0, every returned score IS the f64 product.  That is
# the format, not luck: a product of two e2m1 values is a multiple of 1/4 of at most 36, and on unit rows of 512 features every block maximum lies within a
# few binades, so all products of a score are multiples of one power of two some 14 bits below their sum's bound: the instruction's alignment of the 128
# products of a step drops nothing and the f32 chain is exact (MX-FP8's 8-bit products with wider exponents are not: 1.4e-5).  So TOL = 0 and this test
# is an exact test on real quantised data, next to test 2's on integers; a dropped, doubled or mis-scaled 32-block would move a score by about 2e-2 A.
RANDOM_BAR = 8.6e-5
MEASURED = 0.0
TOL = 2 * MEASURED
PLANTS = 10


@functools.lru_cache(maxsize=None)
def floats():
    """Unit rows (seed 2025).  Every query has PLANTS planted neighbours, gallery rows a q + sqrt(1 - a^2) n with a in [0.6, 0.8] and n a unit noise row:
    their f32 scores are about a, while random unit rows of 512 features score |s| < 0.25.  Quantised on the host by the emulator."""
    rng = np.random.default_rng(2025)
    q = rng.standard_normal((NQ, E_F))
    g = rng.standard_normal((NG, E_F))
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    g /= np.linalg.norm(g, axis=1, keepdims=True)
    plant = rng.permutation(NG)[:NQ * PLANTS].reshape(NQ, PLANTS)
    a = rng.uniform(0.6, 0.8, size=(NQ, PLANTS))
    g[plant] = a[..., None] * q[:, None, :] + np.sqrt(1 - a * a)[..., None] * g[plant]
    g /= np.linalg.norm(g, axis=1, keepdims=True)
    q, g = q.astype(np.float32), g.astype(np.float32)
    qc, qs = MX4.quantize(torch.from_numpy(q))
    gc, gs = MX4.quantize(torch.from_numpy(g))
    q64, g64 = MX4.dequantize(qc, qs).numpy(), MX4.dequantize(gc, gs).numpy()
    planted = np.zeros((NQ, NG), dtype=bool)
    np.put_along_axis(planted, plant, True, 1)
    return dict(q=q, g=g, plant=plant, planted=planted, s64=q64 @ g64.T, A=np.abs(q64) @ np.abs(g64).T, qc=qc, qs=qs, gc=gc, gs=gs)


@functools.lru_cache(maxsize=None)
def floats_dev():
    f = floats()
    return tuple(f[n].to(DEV) for n in ("qc", "qs", "gc", "gs"))


def test_float_scores_against_f64():
    f, tol = floats(), TOL
    assert tol <= RANDOM_BAR
    s64, A = f["s64"], f["A"]
    srt = -np.sort(-s64, axis=1)
    Q, Qs, G, Gs = floats_dev()
    worst = 0.0
    for k, wide in KS:
        idx, val = (t.cpu().numpy() for t in c_topk(Q, Qs, G, Gs, k, wide))
        picked = np.take_along_axis(s64, idx.astype(np.int64), 1)
        rel = np.abs(val - picked) / np.take_along_axis(A, idx.astype(np.int64), 1)
        worst = max(worst, float(rel.max()))
        print(f"mx4 top-{k} ({'wide' if wide else 'narrow'}): max |val - s64| / A = {rel.max():.4e} (tol {tol:.4e}, bar {RANDOM_BAR:.4e}; max A {A.max():.5f})")
        assert (np.diff(val, axis=1) <= 0).all()
        assert all(len(set(r)) == k for r in idx.tolist())
        assert idx.min() >= 0 and idx.max() < NG
        assert (rel <= tol).all()
        assert (picked >= srt[:, k - 1:k] - 2 * tol * A.max(1, keepdims=True)).all()      # nothing better than the list's last was left out
    print(f"mx4: max over all lists {worst:.4e}")


# ---------------------------------------------------------------------------------------------------------------- 4. the same bits
def test_narrow_and_wide_agree_bit_for_bit():
    Q, Qs, G, Gs = floats_dev()
    for k in (1, 10, 16):
        i1, v1 = c_topk(Q, Qs, G, Gs, k, False)
        i2, v2 = c_topk(Q, Qs, G, Gs, k, True)
        assert torch.equal(i1, i2) and torch.equal(_bits(v1), _bits(v2)), k


@pytest.mark.parametrize("k", [16, 100])
def test_chunked_gallery_equals_one_call(k):
    """Were this to fail while test 2 passes, the instruction's result would depend on something other than its two rows: a finding, not a tolerance."""
    from lpi_amd import search
    Q, Qs, G, Gs = floats_dev()
    q, g = search.Mx4Rows(Q, Qs), search.Mx4Rows(G, Gs)
    idx1, val1 = search.topk(q, g, k, operands="mx4")
    assert torch.equal(idx1, c_topk(Q, Qs, G, Gs, k, k > KNARROW)[0])
    for cuts in (((0, 1500), (1500, 1517), (1517, NG)),      # three uneven chunks, the middle one 17 rows
                 ((1517, NG), (0, 1500), (1500, 1517))):     # in another order: the order of the lists is total
        into = None
        for a, b in cuts:      # the first chunk of either order has more than k rows; later ones are merged into the held list
            chunk = g[a:b]
            assert chunk.codes.data_ptr() == G[a:b].data_ptr()      # a view
            into = search.topk(q, chunk, k, col_base=a, into=into, operands="mx4")
        assert torch.equal(into[0], idx1)
        assert torch.equal(_bits(into[1]), _bits(val1))      # bit for bit


# ---------------------------------------------------------------------------------------------------------------- 5. reads and writes
@pytest.mark.parametrize("nq,ng,E", [(127, 129, 384), (130, 300, 1024)])
def test_strided_operands_poisoned_gaps_guarded_outputs(nq, ng, E):
    """0xFF (the code pair -6, -6 and the NaN scale) in every gap of every row and in three whole rows past n, of codes and scales alike; canaries around
    idx, val and the workspace; two launches per call, narrow and wide."""
    guard = 64
    ldq, ldg, ldqs, ldgs = E // 2 + 16, E // 2 + 32, E // 32 + 4, E // 32 + 8
    qc, qs, gc, gs, _, _ = _int_case(nq, ng, E, 11)
    Qc, Qsc, Gc, Gsc = qc.to(DEV), qs.to(DEV), gc.to(DEV), gs.to(DEV)
    Qw = torch.full((nq + 3, ldq), 0xFF, device=DEV, dtype=torch.uint8)
    Gw = torch.full((ng + 3, ldg), 0xFF, device=DEV, dtype=torch.uint8)
    Qsw = torch.full((nq + 3, ldqs), 0xFF, device=DEV, dtype=torch.uint8)
    Gsw = torch.full((ng + 3, ldgs), 0xFF, device=DEV, dtype=torch.uint8)
    Qw[:nq, :E // 2], Gw[:ng, :E // 2], Qsw[:nq, :E // 32], Gsw[:ng, :E // 32] = Qc, Gc, Qsc, Gsc
    for k, wide in ((5, False), (40, True)):
        idx0, val0 = c_topk(Qc, Qsc, Gc, Gsc, k, wide)
        wsn = _ws_bytes(nq, ng, k, wide)
        ibuf = torch.full((guard + nq * k + guard,), CANARY_I, dtype=torch.int32, device=DEV)
        vbuf = torch.full((guard + nq * k + guard,), CANARY_F, dtype=torch.float32, device=DEV)
        wbuf = torch.full((guard + wsn // 4 + guard,), CANARY_I, dtype=torch.int32, device=DEV)
        idx, val = ibuf[guard:guard + nq * k], vbuf[guard:guard + nq * k]
        n0 = _lib.launch_count()
        _lib.call("lpi_search_topk_wide_mx4" if wide else "lpi_search_topk_mx4", nq, ng, E, Qw, ldq, Qsw, ldqs, Gw, ldg, Gsw, ldgs, k, 0, 0, idx, val,
                  wbuf[guard:], wsn, _stream())
        assert _lib.launch_count() == n0 + 2, wide      # the sweep and the merge
        for b, n in ((ibuf, nq * k), (wbuf, wsn // 4)):
            assert (b[:guard] == CANARY_I).all() and (b[guard + n:] == CANARY_I).all(), wide
        assert (vbuf[:guard] == CANARY_F).all() and (vbuf[guard + nq * k:] == CANARY_F).all(), wide
        assert not torch.isnan(val).any()
        assert torch.equal(idx.view(nq, k), idx0) and torch.equal(_bits(val.view(nq, k)), _bits(val0)), wide


# ---------------------------------------------------------------------------------------------------------------- 6. two stages end to end
def test_two_stages_recover_the_f32_lists():
    from lpi_amd import search
    f, k = floats(), PLANTS
    # before any GPU call, from the reference alone: in the emulator's MX-FP4 scores every planted neighbour beats every other row by more than twice the
    # kernel's tolerance, so the coarse top `candidates` (>= 10) of the GPU must hold all ten
    s4, planted = f["s64"], f["planted"]
    gap = np.where(planted, s4, np.inf).min(1) - np.where(planted, -np.inf, s4).max(1)
    print(f"planted - unplanted, MX-FP4 scores: min gap {gap.min():.4f}; 2 TOL max A = {2 * TOL * f['A'].max():.3e}")
    assert (gap > 2 * TOL * f["A"].max()).all()
    s32 = f["q"].astype(np.float64) @ f["g"].astype(np.float64).T
    assert (np.where(planted, s32, np.inf).min(1) - np.where(planted, -np.inf, s32).max(1) > 0.2).all()      # and they are the f32 top 10 by a wide margin
    q, g = torch.from_numpy(f["q"]).to(DEV), torch.from_numpy(f["g"]).to(DEV)
    idx0, val0 = search.topk(q, g, k)
    assert np.array_equal(np.sort(idx0.cpu().numpy(), 1), np.sort(f["plant"], 1))

    def same(got):
        assert torch.equal(got[0], idx0) and torch.equal(_bits(got[1]), _bits(val0))

    n0 = _lib.launch_count()
    same(search.topk_reranked(q, g, k, coarse="mx4"))                                   # the default: 160 candidates, the wide coarse kernel
    assert _lib.launch_count() == n0 + 5      # two quantisers, sweep, merge, re-rank
    same(search.topk_reranked(q, g, k, coarse="mx4", candidates=16))                    # the narrow coarse kernel
    Q, Qs, G, Gs = floats_dev()
    hq, hg = search.Mx4Rows(Q, Qs), search.Mx4Rows(G, Gs)
    n0 = _lib.launch_count()
    same(search.topk_reranked(q, g, k, coarse="mx4", coarse_queries=hq, coarse_gallery=hg))
    assert _lib.launch_count() == n0 + 3      # held operands: nothing is quantised
    gq = search.quantize_mx4(g)
    assert torch.equal(gq.codes.cpu(), f["gc"]) and torch.equal(gq.scales.cpu(), f["gs"])      # what the wrapper quantises is what the host did
    into = None
    for a, b in ((0, 1500), (1500, 1700), (1700, NG)):                                  # a chunked coarse gallery, then one re-rank on the whole f32 gallery
        into = search.topk(hq, hg[a:b], 64, col_base=a, into=into, operands="mx4")
    same(search.rerank(q, g, into[0], k))


# ---------------------------------------------------------------------------------------------------------------- 7. the Python wrapper
def test_wrapper_reads_mx4_rows_in_place():
    from lpi_amd import search
    nq, ng, E, k = 2048, 65536, 512, 10
    gen = torch.Generator(device=DEV).manual_seed(1)
    Qf = torch.randn(nq, E, device=DEV, generator=gen)
    Gf = torch.randn(ng, E, device=DEV, generator=gen)
    Q, G = search.quantize_mx4(Qf), search.quantize_mx4(Gf)
    assert isinstance(G, search.Mx4Rows) and tuple(G.shape) == (ng, E) and G.nbytes == ng * E // 2 + ng * E // 32
    ptrs = (Q.codes.data_ptr(), Q.scales.data_ptr(), G.codes.data_ptr(), G.scales.data_ptr())
    search._WS.clear()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    n0 = _lib.launch_count()
    idx, val = search.topk(Q, G, k, operands="mx4")
    assert _lib.launch_count() == n0 + 2      # held operands: the sweep and the merge, nothing quantised
    torch.cuda.synchronize()
    grown = torch.cuda.max_memory_allocated() - base
    ws = int(_lib.load().lpi_search_workspace(nq, ng, k))
    # three allocations (workspace, idx, val), each rounded up to the allocator's 512-byte granule: no copy of the gallery (17.8 MB), nor of the queries
    bound = ws + 2 * nq * k * 4 + 3 * 512
    print(f"search.topk[mx4] {nq} x {ng} x {E}: peak growth {grown} bytes (workspace {ws}); the gallery is {G.nbytes} bytes")
    assert grown <= bound < G.nbytes
    assert ptrs == (Q.codes.data_ptr(), Q.scales.data_ptr(), G.codes.data_ptr(), G.scales.data_ptr())
    # the answer is right on a sample of rows (f64 on the host, dequantised operands), within test 3's tolerance
    rows = [0, 1, 1027, 2047]
    q64, g64 = MX4.dequantize(Q.codes[rows], Q.scales[rows]).numpy(), MX4.dequantize(G.codes, G.scales).numpy()
    s64, A = q64 @ g64.T, np.abs(q64) @ np.abs(g64).T
    ii = idx[rows].cpu().numpy().astype(np.int64)
    picked = np.take_along_axis(s64, ii, 1)
    assert (np.abs(val[rows].cpu().numpy() - picked) <= TOL * np.take_along_axis(A, ii, 1)).all()
    assert (np.abs(picked - -np.sort(-s64, axis=1)[:, :k]) <= 2 * TOL * A.max(1, keepdims=True)).all()
    # a float operand is quantised exactly once per call: the bits of quantising it first
    n0 = _lib.launch_count()
    i2, v2 = search.topk(Qf, G, k, operands="mx4")
    assert _lib.launch_count() == n0 + 3
    assert torch.equal(i2, idx) and torch.equal(_bits(v2), _bits(val))
    n0 = _lib.launch_count()
    i3, v3 = search.topk(Qf, Gf, 40, operands="mx4")      # both float, the wide call
    assert _lib.launch_count() == n0 + 4
    assert torch.equal(i3[:, :k], idx) and torch.equal(_bits(v3[:, :k]), _bits(val))
    with pytest.raises(ValueError, match="Mx4Rows"):
        search.topk(Q, G, k)
    with pytest.raises(ValueError):
        search.gt_rank(Q, G, idx[:, 3].contiguous(), operands="mx4")
    with pytest.raises(ValueError, match="not a re-rank type"):
        search.rerank(Qf, G, idx)
