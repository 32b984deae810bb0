"""lpi_search_topk_mx8 / lpi_search_rank_mx8 (csrc/search_mx8.hip) on a real MI355X, through the C ABI, held to the CPU restatement of the MX format
(tests/mx8_emulate.py): integer data with per-block scales where every summation order agrees (ties included: the test of the operand lane map, the scale
bytes, the edges and the order), float data against the f64 product of the DEQUANTISED operands under a measured tolerance capped by the project's bar for
the block-scaled instruction, duplicate gallery rows, chunked galleries, strided operands with poisoned gaps and guarded outputs, and the Python wrapper
(an Mx8Rows gallery is read in place; quantize_mx8 is the emulator bit for bit)."""
import functools

import numpy as np
import pytest
import torch

import mx8_emulate as MX
from lpi_amd import _lib

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NONE = 0x7fffffff
CANARY_I, CANARY_F = -0x5A5A5A5B, -12345.5


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _ws(nq, ng, k):
    n = int(_lib.load().lpi_search_workspace(nq, ng, k))
    assert n > 0
    return torch.empty(n, dtype=torch.uint8, device=DEV), n


def c_topk(Q, Qs, G, Gs, k, col_base=0, into=None):
    nq, ng, E = Q.shape[0], G.shape[0], Q.shape[1]
    if into is None:
        idx = torch.empty(nq, k, dtype=torch.int32, device=DEV)
        val = torch.empty(nq, k, dtype=torch.float32, device=DEV)
    else:
        idx, val = into
    ws, n = _ws(nq, ng, k)
    _lib.call("lpi_search_topk_mx8", nq, ng, E, Q, Q.stride(0), Qs, Qs.stride(0), G, G.stride(0), Gs, Gs.stride(0), k, col_base, 0 if into is None else 1,
              idx, val, ws, n, _stream())
    return idx, val


def c_rank(Q, Qs, G, Gs, gt, want_thr=False):
    nq, ng, E = Q.shape[0], G.shape[0], Q.shape[1]
    gt = gt.reshape(nq, -1).contiguous()
    rank = torch.empty(nq, dtype=torch.int32, device=DEV)
    ws, n = _ws(nq, ng, 0)
    _lib.call("lpi_search_rank_mx8", nq, ng, E, Q, Q.stride(0), Qs, Qs.stride(0), G, G.stride(0), Gs, Gs.stride(0), gt, gt.shape[1], rank, ws, n, _stream())
    if want_thr:      # include/lpi_hip.h: after the call ws = threshold scores f32 [nq] | g* int32 [nq]
        return rank, ws[:4 * nq].view(torch.float32).clone(), ws[4 * nq:8 * nq].view(torch.int32).clone()
    return rank


def _bits(t):
    return t.view(torch.int32)


# ---------------------------------------------------------------------------------------------------------------- 1. integer-exact
@functools.lru_cache(maxsize=None)
def _int_case(nq, ng, E, lim, seed):
    """e4m3 bytes of integers in -lim..lim (exact in e4m3) and a random scale byte per (row, block) from {127, 128, 129} (queries: 1, 2, 4) and
    {126, 127, 128} (gallery: 1/2, 1, 2), the domain tests/test_mx8_gpu.py::test_gemm_exact shows exact on the hardware: every partial sum is a multiple of
    1/2 far below 2^22, so every summation order gives the same f32.  Reference: the f64 product of the dequantised operands.  Computed once per shape."""
    gen = torch.Generator().manual_seed(seed)
    q = torch.randint(-lim, lim + 1, (nq, E), generator=gen).float()
    g = torch.randint(-lim, lim + 1, (ng, E), generator=gen).float()
    qs = (127 + torch.randint(0, 3, (nq, E // 32), generator=gen)).to(torch.uint8)
    gs = (126 + torch.randint(0, 3, (ng, E // 32), generator=gen)).to(torch.uint8)
    qc, gc = q.to(torch.float8_e4m3fn).view(torch.uint8), g.to(torch.float8_e4m3fn).view(torch.uint8)
    s = (MX.dequantize(qc, qs) @ MX.dequantize(gc, gs).t()).numpy()
    assert np.abs(s).max() < 2 ** 22 and np.array_equal(s * 2, np.round(s * 2))
    key = np.round(s * 2).astype(np.int64) * ng + np.arange(ng, dtype=np.int64)[None, :]      # monotone in (value, then index): a row's keys are distinct
    order = np.argsort(-key, axis=1, kind="stable")
    gts = {}
    rng = np.random.default_rng(7)
    for gpr in (1, 5):
        gt = rng.integers(0, ng, size=(nq, gpr)).astype(np.int32)
        gt[rng.random((nq, gpr)) < 0.2] = -1                 # padding, whole rows included
        ref = np.full(nq, NONE, dtype=np.int64)
        for i in range(nq):
            v = gt[i][gt[i] >= 0]
            if len(v):
                ref[i] = int((key[i] > key[i, v].max()).sum())
        gts[gpr] = (gt, ref)
    return qc, qs, gc, gs, s, order, gts


# (1, 16, 128): the smallest everything; (127, 129, 256): two slabs, ragged edges; (129, 127, 512): two row blocks; (300, 4133, 512) on -1..1: several
# splits of several tiles, ties; (5, 9001, 1024): the longest rows, one tile per split
@pytest.mark.parametrize("nq,ng,E,lim", [(1, 16, 128, 8), (127, 129, 256, 8), (129, 127, 512, 8), (300, 4133, 512, 1), (5, 9001, 1024, 8)])
def test_integer_scores_exact_with_ties(nq, ng, E, lim):
    qc, qs, gc, gs, s, order, gts = _int_case(nq, ng, E, lim, nq * 1000 + E)
    if (nq, ng) == (300, 4133):      # the premise, from the reference alone: most rows have a tie inside their top 17 (82 % with -1..1, 3 % with -8..8)
        top = np.take_along_axis(s, order[:, :17], 1)
        assert (np.diff(top, axis=1) == 0).any(1).mean() > 0.5
    Q, Qs, G, Gs = (t.to(DEV) for t in (qc, qs, gc, gs))
    for k in (1, 5, 16):
        idx, val = c_topk(Q, Qs, G, Gs, k)
        want = order[:, :k]
        assert np.array_equal(idx.cpu().numpy(), want), (k, "idx")
        assert np.array_equal(val.cpu().numpy(), np.take_along_axis(s, want, 1).astype(np.float32)), (k, "val")
    for gpr, (gt, ref) in gts.items():
        rank = c_rank(Q, Qs, G, Gs, torch.from_numpy(gt).to(DEV))
        assert np.array_equal(rank.cpu().numpy().astype(np.int64), ref), gpr


# ---------------------------------------------------------------------------------------------------------------- 2.-4. float data
NQ, NG, E_F = 300, 4133, 512
# |val - s64| <= TOL * A with s64 = the f64 product of the DEQUANTISED operands and A = |q| . |g| of them.  The block-scaled instruction aligns the 128 scaled
# products of a step to a common exponent before it adds them (tests/test_mx8_gpu.py records 1.4 - 2.2e-5 of max |ref| for the GEMM), so f32 round-off
# reasoning does not apply and TOL is measured: 2 x the first measured maximum over all returned entries (top-16 of 300 rows; the margin covers data
# dependence, as tests/test_search16_gpu.py's), and it must stay under the project's own bar for this instruction, RANDOM_BAR = 8.6e-5, applied to A
# (A >= max |ref|: no tighter than the GEMM's bar).  A dropped or doubled 32-block moves a score by about 1.7e-2 A on these rows (6e-2 A on planted ones):
# test 1 is the definitive check of that, the bar still catches it.  First measured maximum on an MI355X: MEASURED below.
RANDOM_BAR = 8.6e-5
MEASURED = 1.4234e-05
TOL = 2 * MEASURED


@functools.lru_cache(maxsize=None)
def floats():
    """tests/test_search16_gpu.py::floats' construction (seed 2024, unit rows) with the ground truth planted on 3 of every 4 rows, quantised on the host by
    the emulator."""
    rng = np.random.default_rng(2024)
    q = rng.standard_normal((NQ, E_F)).astype(np.float32)
    g = rng.standard_normal((NG, E_F)).astype(np.float32)
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    gt = np.empty(NQ, dtype=np.int32)
    planted = np.arange(NQ) % 4 != 3
    gt[planted] = 13 + 18 * np.arange(int(planted.sum()))                  # 13, 31, ...: room for the copies of test 3 around each
    free = np.setdiff1d(np.arange(NG), np.concatenate([gt[planted] + d for d in (-5, 0, 7, 11)]))
    gt[~planted] = rng.choice(free, size=int((~planted).sum()), replace=False)
    g[gt[planted]] = q[planted] + 1e-3 * rng.standard_normal((int(planted.sum()), E_F)).astype(np.float32)
    g /= np.linalg.norm(g, axis=1, keepdims=True)
    qc, qs = MX.quantize(torch.from_numpy(q))
    gc, gs = MX.quantize(torch.from_numpy(g))
    q64, g64 = MX.dequantize(qc, qs).numpy(), MX.dequantize(gc, gs).numpy()
    return dict(gt=gt, planted=planted, s64=q64 @ g64.T, A=np.abs(q64) @ np.abs(g64).T, gc=gc, gs=gs, Q=qc.to(DEV), Qs=qs.to(DEV), G=gc.to(DEV),
                Gs=gs.to(DEV), GT=torch.from_numpy(gt).to(DEV))


def test_float_scores_against_f64():
    f, tol = floats(), TOL
    assert tol <= RANDOM_BAR
    s64, A, gt = f["s64"], f["A"], f["gt"]
    rows = np.arange(NQ)
    # a score's kernel value lies in s64 -+ tol A: column j surely beats the ground truth / may beat it
    slack = tol * (A + A[rows, gt][:, None])
    gv = s64[rows, gt][:, None]
    lo = (s64 - gv > slack).sum(1)
    hi = (s64 - gv >= -slack).sum(1) - 1                     # j != g*
    assert (lo == hi).mean() >= 0.5                          # premise, from the reference alone: at least half the intervals are one point
    srt = -np.sort(-s64, axis=1)
    for k in (16, 5, 1):
        idx, val = (t.cpu().numpy() for t in c_topk(f["Q"], f["Qs"], f["G"], f["Gs"], k))
        picked = np.take_along_axis(s64, idx.astype(np.int64), 1)
        rel = np.abs(val - picked) / np.take_along_axis(A, idx.astype(np.int64), 1)
        print(f"mx8 top-{k}: max |val - s64| / A = {rel.max():.4e} (tol {tol:.4e}, bar {RANDOM_BAR:.4e}; max A {A.max():.5f})")
        assert (np.diff(val, axis=1) <= 0).all()
        assert all(len(set(r)) == k for r in idx.tolist())
        assert idx.min() >= 0 and idx.max() < NG
        assert (rel <= tol).all()
        assert (picked >= srt[:, k - 1:k] - 2 * tol * A.max(1, keepdims=True)).all()
    rank = c_rank(f["Q"], f["Qs"], f["G"], f["Gs"], f["GT"]).cpu().numpy()
    print(f"mx8 rank: {int((lo == hi).sum())} one-point intervals of {NQ}; widest {int((hi - lo).max())}")
    assert ((rank >= lo) & (rank <= hi)).all()


def test_duplicate_gallery_rows_fall_by_index():
    f = floats()
    c2, s2 = f["gc"].clone(), f["gs"].clone()
    rows = np.nonzero(f["planted"])[0]
    larger = np.zeros(NQ, dtype=np.int64)
    for n, i in enumerate(rows):
        j = int(f["gt"][i])
        c2[j - 5], s2[j - 5] = c2[j], s2[j]                  # a copy (elements and scales) at a smaller index: it sorts after the original
        for d in (7, 11)[:n % 3]:                            # 0, 1 or 2 copies at larger indices: they sort before it
            c2[j + d], s2[j + d] = c2[j], s2[j]
        larger[i] = n % 3
    r1 = c_rank(f["Q"], f["Qs"], f["G"], f["Gs"], f["GT"]).cpu().numpy().astype(np.int64)
    r2 = c_rank(f["Q"], f["Qs"], c2.to(DEV), s2.to(DEV), f["GT"]).cpu().numpy().astype(np.int64)
    assert np.array_equal(r2[rows], r1[rows] + larger[rows])
    assert set(larger[rows]) == {0, 1, 2}


@pytest.mark.parametrize("data", ["float", "int"])
def test_chunked_gallery_and_consistency(data):
    """Were this to fail while test 1 passes, the instruction's result would depend on something other than its two rows: a finding, not a tolerance."""
    if data == "float":
        f = floats()
        Q, Qs, G, Gs, GT = f["Q"], f["Qs"], f["G"], f["Gs"], f["GT"]
    else:
        qc, qs, gc, gs, _, _, _ = _int_case(NQ, NG, E_F, 8, 5)
        Q, Qs, G, Gs = (t.to(DEV) for t in (qc, qs, gc, gs))
        GT = torch.from_numpy(np.random.default_rng(3).integers(0, NG, size=NQ).astype(np.int32)).to(DEV)
    k = 16
    idx1, val1 = c_topk(Q, Qs, G, Gs, k)
    if data == "int":      # random ground truth is rarely among the 16 best of 4 133: every other row's becomes its third best
        GT = torch.where(torch.arange(NQ, device=DEV) % 2 == 0, idx1[:, 2], GT)
    for cuts in (((0, 1500), (1500, 1517), (1517, NG)),      # three uneven chunks, the middle one 17 rows
                 ((1517, NG), (0, 1500), (1500, 1517))):     # in another order: the order of the lists is total
        into = None
        for a, b in cuts:
            into = c_topk(Q, Qs, G[a:b], Gs[a:b], k, col_base=a, into=into)
        assert torch.equal(into[0], idx1)
        assert torch.equal(_bits(into[1]), _bits(val1))      # bit for bit
    rank, thr, gstar = c_rank(Q, Qs, G, Gs, GT, want_thr=True)
    assert torch.equal(gstar, GT)
    hit = idx1 == GT[:, None]
    assert torch.equal(rank < k, hit.any(1))
    rows, pos = hit.nonzero(as_tuple=True)
    assert len(rows) > 0
    assert torch.equal(_bits(val1[rows, pos]), _bits(thr[rows]))      # the threshold launch computes the sweep's bits
    assert torch.equal(pos.to(torch.int32), rank[rows])               # and the rank is the position in the list


# ---------------------------------------------------------------------------------------------------------------- 5. bounds
@pytest.mark.parametrize("nq,ng,E", [(127, 129, 256), (129, 300, 512)])
def test_strided_operands_poisoned_gaps_guarded_outputs(nq, ng, E):
    k, gpr, guard = 5, 2, 64
    ldq, ldg, ldqs, ldgs = E + 16, E + 32, E // 32 + 4, E // 32 + 8
    qc, qs, gc, gs, _, _, _ = _int_case(nq, ng, E, 8, 11)
    gt = np.random.default_rng(11).integers(0, ng, size=(nq, gpr)).astype(np.int32)
    Qc, Qsc, Gc, Gsc, GT = qc.to(DEV), qs.to(DEV), gc.to(DEV), gs.to(DEV), torch.from_numpy(gt).to(DEV)
    idx0, val0 = c_topk(Qc, Qsc, Gc, Gsc, k)
    rank0 = c_rank(Qc, Qsc, Gc, Gsc, GT)
    # NaN element bytes (0x7F) in the gaps of every row and in three whole rows past n; the NaN scale byte (0xFF) likewise
    Qw = torch.full((nq + 3, ldq), 0x7F, device=DEV, dtype=torch.uint8)
    Gw = torch.full((ng + 3, ldg), 0x7F, device=DEV, dtype=torch.uint8)
    Qsw = torch.full((nq + 3, ldqs), 0xFF, device=DEV, dtype=torch.uint8)
    Gsw = torch.full((ng + 3, ldgs), 0xFF, device=DEV, dtype=torch.uint8)
    Qw[:nq, :E], Gw[:ng, :E], Qsw[:nq, :E // 32], Gsw[:ng, :E // 32] = Qc, Gc, Qsc, Gsc
    ws_t, ws_r = int(_lib.load().lpi_search_workspace(nq, ng, k)), int(_lib.load().lpi_search_workspace(nq, ng, 0))
    ibuf = torch.full((guard + nq * k + guard,), CANARY_I, dtype=torch.int32, device=DEV)
    vbuf = torch.full((guard + nq * k + guard,), CANARY_F, dtype=torch.float32, device=DEV)
    rbuf = torch.full((guard + nq + guard,), CANARY_I, dtype=torch.int32, device=DEV)
    wbuf = torch.full((guard + max(ws_t, ws_r) // 4 + guard,), CANARY_I, dtype=torch.int32, device=DEV)
    idx, val, rank = ibuf[guard:guard + nq * k], vbuf[guard:guard + nq * k], rbuf[guard:guard + nq]
    s = _stream()
    _lib.call("lpi_search_topk_mx8", nq, ng, E, Qw, ldq, Qsw, ldqs, Gw, ldg, Gsw, ldgs, k, 0, 0, idx, val, wbuf[guard:], ws_t, s)
    for b, n in ((ibuf, nq * k), (rbuf, 0), (wbuf, ws_t // 4)):
        assert (b[:guard] == CANARY_I).all() and (b[guard + n:] == CANARY_I).all()
    assert (vbuf[:guard] == CANARY_F).all() and (vbuf[guard + nq * k:] == CANARY_F).all()
    assert torch.equal(idx.view(nq, k), idx0) and torch.equal(_bits(val.view(nq, k)), _bits(val0))
    wbuf.fill_(CANARY_I)
    _lib.call("lpi_search_rank_mx8", nq, ng, E, Qw, ldq, Qsw, ldqs, Gw, ldg, Gsw, ldgs, GT, gpr, rank, wbuf[guard:], ws_r, s)
    assert (rbuf[:guard] == CANARY_I).all() and (rbuf[guard + nq:] == CANARY_I).all()
    assert (wbuf[:guard] == CANARY_I).all() and (wbuf[guard + ws_r // 4:] == CANARY_I).all()
    assert (ibuf[:guard] == CANARY_I).all() and (ibuf[guard + nq * k:] == CANARY_I).all()
    assert torch.equal(rank, rank0)
    assert not torch.isnan(val).any()


# ---------------------------------------------------------------------------------------------------------------- 6. the Python wrapper
def test_wrapper_reads_mx8_rows_in_place():
    from lpi_amd import search
    nq, ng, E, k = 2048, 65536, 512, 10
    gen = torch.Generator(device=DEV).manual_seed(1)
    Qf = torch.randn(nq, E, device=DEV, generator=gen)
    Q = search.quantize_mx8(Qf)
    G = search.quantize_mx8(torch.randn(ng, E, device=DEV, generator=gen))
    assert isinstance(G, search.Mx8Rows) and tuple(G.shape) == (ng, E) and G.nbytes == ng * E + ng * E // 32
    search._WS.clear()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    idx, val = search.topk(Q, G, k, operands="mx8")
    torch.cuda.synchronize()
    grown = torch.cuda.max_memory_allocated() - base
    ws = int(_lib.load().lpi_search_workspace(nq, ng, k))
    # three allocations (workspace, idx, val), each rounded up to the allocator's 512-byte granule: no copy of the gallery (33.5 MB), nor of the queries
    bound = ws + 2 * nq * k * 4 + 3 * 512
    print(f"search.topk[mx8] {nq} x {ng} x {E}: peak growth {grown} bytes (workspace {ws}); the gallery is {G.nbytes} bytes")
    assert grown <= bound < ng * E
    # the answer is right on a sample of rows (f64 on the host, dequantised operands), within test 2's tolerance
    rows = [0, 1, 1027, 2047]
    q64, g64 = MX.dequantize(Q.codes[rows], Q.scales[rows]).numpy(), MX.dequantize(G.codes, G.scales).numpy()
    s64, A = q64 @ g64.T, np.abs(q64) @ np.abs(g64).T
    ii = idx[rows].cpu().numpy().astype(np.int64)
    picked = np.take_along_axis(s64, ii, 1)
    assert (np.abs(val[rows].cpu().numpy() - picked) <= TOL * np.take_along_axis(A, ii, 1)).all()
    assert (np.abs(picked - -np.sort(-s64, axis=1)[:, :k]) <= 2 * TOL * A.max(1, keepdims=True)).all()
    # a float query with an Mx8Rows gallery is quantised once: the bits of quantising it first
    i2, v2 = search.topk(Qf, G, k, operands="mx8")
    assert torch.equal(i2, idx) and torch.equal(_bits(v2), _bits(val))
    # a gallery searched in chunks (row slices are views) gives one call's result
    into = None
    for a, b in ((0, 30000), (30000, ng)):
        into = search.topk(Q, G[a:b], k, col_base=a, into=into, operands="mx8")
    assert torch.equal(into[0], idx) and torch.equal(_bits(into[1]), _bits(val))
    r = search.gt_rank(Q, G, idx[:, 3].contiguous(), operands="mx8")
    assert torch.equal(r, torch.full_like(r, 3))      # the fourth of the list has rank 3: the list's order is the rank's
    with pytest.raises(ValueError, match="Mx8Rows"):
        search.topk(Q, G, k)
    with pytest.raises(ValueError, match="Mx8Rows"):
        search.gt_rank(Qf, G, idx[:, 3].contiguous(), operands="bf16")


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_quantize_mx8_is_the_emulator_bit_for_bit(dtype):
    from lpi_amd import search
    x = (torch.randn(300, 512, generator=torch.Generator().manual_seed(9)) * torch.exp(torch.randn(300, 1, generator=torch.Generator().manual_seed(10)))).to(dtype)
    n0 = _lib.launch_count()
    r = search.quantize_mx8(x.to(DEV))
    assert _lib.launch_count() == n0 + 1      # one lpi_mx8_quantize launch
    qr, sr = MX.quantize(x)
    assert torch.equal(r.codes.cpu(), qr) and torch.equal(r.scales.cpu(), sr)
