"""lpi_search_topk_t / lpi_search_rank_t (csrc/search16.hip) on a real MI355X, through the C ABI, for bf16 and f16 operands: integer data where every
summation order agrees (ties included) and where the 2-byte, the f32 and the forwarded-f32 results are one, float data against f64 under a measured
tolerance capped by E * 2^-23, duplicate gallery rows, chunked galleries, strided operands with poisoned gaps and guarded outputs, and the Python wrapper
(no copy of a 2-byte gallery; the default path is the f32 one)."""
import functools

import numpy as np
import pytest
import torch

from lpi_amd import _lib

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NONE = 0x7fffffff
CANARY_I, CANARY_F = -0x5A5A5A5B, -12345.5
OPS = {"bf16": (_lib.BF16, torch.bfloat16), "f16": (_lib.F16, torch.float16)}
both = pytest.mark.parametrize("op", sorted(OPS))


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _ws(nq, ng, k):
    n = int(_lib.load().lpi_search_workspace(nq, ng, k))
    assert n > 0
    return torch.empty(n, dtype=torch.uint8, device=DEV), n


def c_topk(dt, Q, G, k, col_base=0, into=None):
    """dt = None: lpi_search_topk (the f32 entry point); else lpi_search_topk_t with that code."""
    nq, ng, E = Q.shape[0], G.shape[0], Q.shape[1]
    if into is None:
        idx = torch.empty(nq, k, dtype=torch.int32, device=DEV)
        val = torch.empty(nq, k, dtype=torch.float32, device=DEV)
    else:
        idx, val = into
    ws, n = _ws(nq, ng, k)
    name, lead = ("lpi_search_topk", ()) if dt is None else ("lpi_search_topk_t", (dt,))
    _lib.call(name, *lead, nq, ng, E, Q, Q.stride(0), G, G.stride(0), k, col_base, 0 if into is None else 1, idx, val, ws, n, _stream())
    return idx, val


def c_rank(dt, Q, G, gt, want_thr=False):
    nq, ng, E = Q.shape[0], G.shape[0], Q.shape[1]
    gt = gt.reshape(nq, -1).contiguous()
    rank = torch.empty(nq, dtype=torch.int32, device=DEV)
    ws, n = _ws(nq, ng, 0)
    name, lead = ("lpi_search_rank", ()) if dt is None else ("lpi_search_rank_t", (dt,))
    _lib.call(name, *lead, nq, ng, E, Q, Q.stride(0), G, G.stride(0), gt, gt.shape[1], rank, ws, n, _stream())
    if want_thr:      # include/lpi_hip.h: after the call ws = threshold scores f32 [nq] | g* int32 [nq]
        return rank, ws[:4 * nq].view(torch.float32).clone(), ws[4 * nq:8 * nq].view(torch.int32).clone()
    return rank


def _bits(t):
    return t.view(torch.int32)


# ---------------------------------------------------------------------------------------------------------------- 1. integer-exact
@functools.lru_cache(maxsize=None)
def _int_case(nq, ng, E, seed):
    """Values in -3..3 are exact in bf16 and f16; |s| <= 9 E < 2^24, so every summation order gives the same f32.  Computed once per shape."""
    rng = np.random.default_rng(seed)
    q = rng.integers(-3, 4, size=(nq, E)).astype(np.int64)
    g = rng.integers(-3, 4, size=(ng, E)).astype(np.int64)
    s = q @ g.T
    key = s * ng + np.arange(ng, dtype=np.int64)[None, :]    # monotone in (value, then index): all keys of a row are distinct
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
    return q, g, s, order, gts


# (1, 16, 32): the smallest everything; (127, 129, 96): the E % 64 == 32 tail, two slabs, ragged edges; (129, 127, 512): two row blocks;
# (300, 4133, 512): several splits of several tiles; (5, 9001, 1024): the longest rows, one tile per split
@both
@pytest.mark.parametrize("nq,ng,E", [(1, 16, 32), (127, 129, 96), (129, 127, 512), (300, 4133, 512), (5, 9001, 1024)])
def test_integer_scores_exact_with_ties(op, nq, ng, E):
    dt, tdt = OPS[op]
    q, g, s, order, gts = _int_case(nq, ng, E, nq * 1000 + E)
    if (nq, ng) == (300, 4133):      # the premise: most rows have a tie inside their top 17
        top = np.take_along_axis(s, order[:, :17], 1)
        assert (np.diff(top, axis=1) == 0).any(1).mean() > 0.5
    Qf, Gf = torch.from_numpy(q.astype(np.float32)).to(DEV), torch.from_numpy(g.astype(np.float32)).to(DEV)
    Q, G = Qf.to(tdt), Gf.to(tdt)
    assert torch.equal(Q.float(), Qf) and torch.equal(G.float(), Gf)
    for k in (1, 5, 16):
        idx, val = c_topk(dt, Q, G, k)
        want = order[:, :k]
        assert np.array_equal(idx.cpu().numpy(), want), (k, "idx")
        assert np.array_equal(val.cpu().numpy(), np.take_along_axis(s, want, 1).astype(np.float32)), (k, "val")
        for other in (None, _lib.F32):      # the f32 entry point, and LPI_F32 through the typed one: the same bits
            i2, v2 = c_topk(other, Qf, Gf, k)
            assert torch.equal(i2, idx) and torch.equal(_bits(v2), _bits(val)), (k, other)
    for gpr, (gt, ref) in gts.items():
        GT = torch.from_numpy(gt).to(DEV)
        rank = c_rank(dt, Q, G, GT)
        assert np.array_equal(rank.cpu().numpy().astype(np.int64), ref), gpr
        for other in (None, _lib.F32):
            assert torch.equal(c_rank(other, Qf, Gf, GT), rank), (gpr, other)


# ---------------------------------------------------------------------------------------------------------------- 2.-4. float data
NQ, NG, E_F = 300, 4133, 512
# |val - s64| <= TOL * A with A = |q| . |g| (f64), s64 = the f64 product of the ROUNDED values.  The products of two 2-byte values are exact in f32 (16-bit
# significands for bf16, 22-bit for f16) and at most E - 1 additions lose at most one ulp each, rounding or truncating, so TOL <= CAP = E * 2^-23 whatever
# the instruction's inner summation is; a value above CAP would mean a slab dropped or read twice.  How v_mfma_f32_16x16x32_{bf16,f16} sums its 32
# products is not documented, so TOL is measured: 2 x the first measured maximum over all returned entries (top-16 of 300 rows; the margin covers data
# dependence).  First measured maxima on an MI355X: MEASURED below, 3.07e-7 for bf16 and 3.09e-7 for f16 = 1/199 of CAP (6.10e-5); an f32 matrix product
# of the same rounded values on a CPU is as far from s64 (3.1e-7 / 5.1e-7).
CAP = E_F * 2.0 ** -23
MEASURED = {"bf16": 3.0736e-07, "f16": 3.0896e-07}
TOL = {op: 2 * m for op, m in MEASURED.items()}


@functools.lru_cache(maxsize=None)
def floats(op):
    """tests/test_search_gpu.py::floats (seed 2024, half the ground truths planted), then rounded to the operand type."""
    tdt = OPS[op][1]
    rng = np.random.default_rng(2024)
    q = rng.standard_normal((NQ, E_F)).astype(np.float32)
    g = rng.standard_normal((NG, E_F)).astype(np.float32)
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    gt = np.empty(NQ, dtype=np.int32)
    planted = np.arange(NQ) % 2 == 0
    gt[planted] = 13 + 27 * (np.arange(NQ)[planted] // 2)                  # 13, 40, ...: room for the copies of test 3 around each
    free = np.setdiff1d(np.arange(NG), np.concatenate([gt[planted] + d for d in (-5, 0, 7, 11)]))
    gt[~planted] = rng.choice(free, size=int((~planted).sum()), replace=False)
    g[gt[planted]] = q[planted] + 1e-3 * rng.standard_normal((int(planted.sum()), E_F)).astype(np.float32)
    g /= np.linalg.norm(g, axis=1, keepdims=True)
    Qh, Gh = torch.from_numpy(q.astype(np.float32)).to(tdt), torch.from_numpy(g.astype(np.float32)).to(tdt)      # rounded on the host, RNE
    q64, g64 = Qh.double().numpy(), Gh.double().numpy()
    return dict(gt=gt, planted=planted, s64=q64 @ g64.T, A=np.abs(q64) @ np.abs(g64).T, Gh=Gh, Q=Qh.to(DEV), G=Gh.to(DEV),
                GT=torch.from_numpy(gt).to(DEV))


@both
def test_float_scores_against_f64(op):
    dt, f, tol = OPS[op][0], floats(op), TOL[op]
    assert tol <= CAP
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
        idx, val = (t.cpu().numpy() for t in c_topk(dt, f["Q"], f["G"], k))
        picked = np.take_along_axis(s64, idx.astype(np.int64), 1)
        rel = np.abs(val - picked) / np.take_along_axis(A, idx.astype(np.int64), 1)
        print(f"{op} top-{k}: max |val - s64| / A = {rel.max():.4e} (tol {tol:.4e}, cap E 2^-23 = {CAP:.4e}; max A {A.max():.5f})")
        assert (np.diff(val, axis=1) <= 0).all()
        assert all(len(set(r)) == k for r in idx.tolist())
        assert idx.min() >= 0 and idx.max() < NG
        assert (rel <= tol).all()
        assert (picked >= srt[:, k - 1:k] - 2 * tol * A.max(1, keepdims=True)).all()
    rank = c_rank(dt, f["Q"], f["G"], f["GT"]).cpu().numpy()
    print(f"{op} rank: {int((lo == hi).sum())} one-point intervals of {NQ}; widest {int((hi - lo).max())}")
    assert ((rank >= lo) & (rank <= hi)).all()


@both
def test_duplicate_gallery_rows_fall_by_index(op):
    dt, f = OPS[op][0], floats(op)
    g2 = f["Gh"].clone()
    rows = np.nonzero(f["planted"])[0]
    larger = np.zeros(NQ, dtype=np.int64)
    for n, i in enumerate(rows):
        j = int(f["gt"][i])
        g2[j - 5] = g2[j]                                    # a copy at a smaller index: it sorts after the original
        for d in (7, 11)[:n % 3]:                            # 0, 1 or 2 copies at larger indices: they sort before it
            g2[j + d] = g2[j]
        larger[i] = n % 3
    r1 = c_rank(dt, f["Q"], f["G"], f["GT"]).cpu().numpy().astype(np.int64)
    r2 = c_rank(dt, f["Q"], g2.to(DEV), f["GT"]).cpu().numpy().astype(np.int64)
    assert np.array_equal(r2[rows], r1[rows] + larger[rows])
    assert set(larger[rows]) == {0, 1, 2}


@both
@pytest.mark.parametrize("data", ["float", "int"])
def test_chunked_gallery_and_consistency(op, data):
    dt, tdt = OPS[op]
    if data == "float":
        f = floats(op)
        Q, G, GT = f["Q"], f["G"], f["GT"]
    else:
        q, g, _, _, _ = _int_case(NQ, NG, E_F, 5)
        Q, G = torch.from_numpy(q.astype(np.float32)).to(DEV).to(tdt), torch.from_numpy(g.astype(np.float32)).to(DEV).to(tdt)
        GT = torch.from_numpy(np.random.default_rng(3).integers(0, NG, size=NQ).astype(np.int32)).to(DEV)
    k = 16
    idx1, val1 = c_topk(dt, Q, G, k)
    if data == "int":      # random ground truth is rarely among the 16 best of 4 133: every other row's becomes its third best
        GT = torch.where(torch.arange(NQ, device=DEV) % 2 == 0, idx1[:, 2], GT)
    for cuts in (((0, 1500), (1500, 1517), (1517, NG)),      # three uneven chunks, the middle one 17 rows
                 ((1517, NG), (0, 1500), (1500, 1517))):     # in another order: the order of the lists is total
        into = None
        for a, b in cuts:
            into = c_topk(dt, Q, G[a:b], k, col_base=a, into=into)
        assert torch.equal(into[0], idx1)
        assert torch.equal(_bits(into[1]), _bits(val1))      # bit for bit
    rank, thr, gstar = c_rank(dt, Q, G, GT, want_thr=True)
    assert torch.equal(gstar, GT)
    hit = idx1 == GT[:, None]
    assert torch.equal(rank < k, hit.any(1))
    rows, pos = hit.nonzero(as_tuple=True)
    assert len(rows) > 0
    assert torch.equal(_bits(val1[rows, pos]), _bits(thr[rows]))      # the threshold launch computes the sweep's bits
    assert torch.equal(pos.to(torch.int32), rank[rows])               # and the rank is the position in the list


# ---------------------------------------------------------------------------------------------------------------- 5. bounds
@both
@pytest.mark.parametrize("nq,ng,E", [(127, 129, 96), (129, 300, 512)])
def test_strided_operands_poisoned_gaps_guarded_outputs(op, nq, ng, E):
    dt, tdt = OPS[op]
    k, gpr, guard = 5, 2, 64
    ldq, ldg = E + 8, E + 16
    rng = np.random.default_rng(11)
    q = rng.integers(-3, 4, size=(nq, E)).astype(np.float32)
    g = rng.integers(-3, 4, size=(ng, E)).astype(np.float32)
    gt = rng.integers(0, ng, size=(nq, gpr)).astype(np.int32)
    Qc, Gc, GT = torch.from_numpy(q).to(DEV).to(tdt), torch.from_numpy(g).to(DEV).to(tdt), torch.from_numpy(gt).to(DEV)
    idx0, val0 = c_topk(dt, Qc, Gc, k)
    rank0 = c_rank(dt, Qc, Gc, GT)
    # NaN in the gaps of every row and in whole rows past n
    Qs = torch.full((nq + 3, ldq), float("nan"), device=DEV, dtype=tdt)
    Gs = torch.full((ng + 3, ldg), float("nan"), device=DEV, dtype=tdt)
    Qs[:nq, :E] = Qc
    Gs[:ng, :E] = Gc
    ws_t, ws_r = int(_lib.load().lpi_search_workspace(nq, ng, k)), int(_lib.load().lpi_search_workspace(nq, ng, 0))
    ibuf = torch.full((guard + nq * k + guard,), CANARY_I, dtype=torch.int32, device=DEV)
    vbuf = torch.full((guard + nq * k + guard,), CANARY_F, dtype=torch.float32, device=DEV)
    rbuf = torch.full((guard + nq + guard,), CANARY_I, dtype=torch.int32, device=DEV)
    wbuf = torch.full((guard + max(ws_t, ws_r) // 4 + guard,), CANARY_I, dtype=torch.int32, device=DEV)
    idx, val, rank = ibuf[guard:guard + nq * k], vbuf[guard:guard + nq * k], rbuf[guard:guard + nq]
    s = _stream()
    _lib.call("lpi_search_topk_t", dt, nq, ng, E, Qs, ldq, Gs, ldg, k, 0, 0, idx, val, wbuf[guard:], ws_t, s)
    for b, n in ((ibuf, nq * k), (rbuf, 0), (wbuf, ws_t // 4)):
        assert (b[:guard] == CANARY_I).all() and (b[guard + n:] == CANARY_I).all()
    assert (vbuf[:guard] == CANARY_F).all() and (vbuf[guard + nq * k:] == CANARY_F).all()
    assert torch.equal(idx.view(nq, k), idx0) and torch.equal(_bits(val.view(nq, k)), _bits(val0))
    wbuf.fill_(CANARY_I)
    _lib.call("lpi_search_rank_t", dt, nq, ng, E, Qs, ldq, Gs, ldg, GT, gpr, rank, wbuf[guard:], ws_r, s)
    assert (rbuf[:guard] == CANARY_I).all() and (rbuf[guard + nq:] == CANARY_I).all()
    assert (wbuf[:guard] == CANARY_I).all() and (wbuf[guard + ws_r // 4:] == CANARY_I).all()
    assert (ibuf[:guard] == CANARY_I).all() and (ibuf[guard + nq * k:] == CANARY_I).all()
    assert torch.equal(rank, rank0)
    assert not torch.isnan(val).any()


# ---------------------------------------------------------------------------------------------------------------- 6. the Python wrapper
@both
def test_wrapper_reads_2byte_operands_in_place(op):
    from lpi_amd import search
    tdt = OPS[op][1]
    nq, ng, E, k = 2048, 65536, 512, 10
    gen = torch.Generator(device=DEV).manual_seed(1)
    Q = torch.randn(nq, E, device=DEV, generator=gen).to(tdt)
    G = torch.randn(ng, E, device=DEV, generator=gen).to(tdt)
    search._WS.clear()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    idx, val = search.topk(Q, G, k, operands=op)
    torch.cuda.synchronize()
    grown = torch.cuda.max_memory_allocated() - base
    ws = int(_lib.load().lpi_search_workspace(nq, ng, k))
    # three allocations (workspace, idx, val), each rounded up to the allocator's 512-byte granule: no copy of the gallery (64 MB), nor of the queries
    bound = ws + 2 * nq * k * 4 + 3 * 512
    print(f"search.topk[{op}] {nq} x {ng} x {E}: peak growth {grown} bytes (workspace {ws}); the gallery is {ng * E * 2} bytes")
    assert grown <= bound < ng * E * 2
    # the answer is right on a sample of rows (f64 on the host), within test 2's tolerance at these rows' lengths, both sides
    rows = [0, 1, 1027, 2047]
    q64, g64 = Q[rows].double().cpu().numpy(), G.double().cpu().numpy()
    s64, A = q64 @ g64.T, np.abs(q64) @ np.abs(g64).T
    ii = idx[rows].cpu().numpy().astype(np.int64)
    picked = np.take_along_axis(s64, ii, 1)
    assert (np.abs(val[rows].cpu().numpy() - picked) <= TOL[op] * np.take_along_axis(A, ii, 1)).all()
    assert (np.abs(picked - -np.sort(-s64, axis=1)[:, :k]) <= 2 * TOL[op] * A.max(1, keepdims=True)).all()
    # operands=None on the same 2-byte tensors is the old path: an f32 copy searched by the f32 kernels, bit for bit
    i0, v0 = search.topk(Q, G, k)
    i1, v1 = search.topk(Q.float(), G.float(), k)
    assert torch.equal(i0, i1) and torch.equal(_bits(v0), _bits(v1))
    # a gallery that is a view: row stride E + 8 is read in place, a transposed one is made contiguous once; both give the contiguous one's result
    wide = torch.zeros(ng, E + 8, device=DEV, dtype=tdt)
    wide[:, :E] = G
    for view in (wide[:, :E], G.t().contiguous().t()):
        assert not view.is_contiguous()
        i2, v2 = search.topk(Q, view, k, operands=op)
        assert torch.equal(i2, idx) and torch.equal(_bits(v2), _bits(val))
    r = search.gt_rank(Q, G, idx[:, 3].contiguous(), operands=op)
    assert torch.equal(r, torch.full_like(r, 3))      # the fourth of the list has rank 3: the list's order is the rank's
