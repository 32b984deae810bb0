"""lpi_search_topk / lpi_search_rank (csrc/search.hip) on a real MI355X, through the C ABI: integer data where every summation order agrees (ties
included, nothing excluded), float data against f64 under the worst-case dot-product bound, duplicate gallery rows, chunked galleries, strided operands
with poisoned gaps and guarded outputs, and the memory the Python wrapper takes."""
import numpy as np
import pytest
import torch

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


def c_topk(Q, G, k, nq=None, ng=None, E=None, col_base=0, into=None):
    nq, ng, E = nq or Q.shape[0], ng or G.shape[0], E or Q.shape[1]
    if into is None:
        idx = torch.empty(nq, k, dtype=torch.int32, device=DEV)
        val = torch.empty(nq, k, dtype=torch.float32, device=DEV)
    else:
        idx, val = into
    ws, n = _ws(nq, ng, k)
    _lib.call("lpi_search_topk", nq, ng, E, Q, Q.stride(0), G, G.stride(0), k, col_base, 0 if into is None else 1, idx, val, ws, n, _stream())
    return idx, val


def c_rank(Q, G, gt, nq=None, ng=None, E=None, want_thr=False):
    nq, ng, E = nq or Q.shape[0], ng or G.shape[0], E or Q.shape[1]
    gt = gt.reshape(nq, -1).contiguous()
    rank = torch.empty(nq, dtype=torch.int32, device=DEV)
    ws, n = _ws(nq, ng, 0)
    _lib.call("lpi_search_rank", nq, ng, E, Q, Q.stride(0), G, G.stride(0), gt, gt.shape[1], rank, ws, n, _stream())
    if want_thr:      # include/lpi_hip.h: after the call ws = threshold scores f32 [nq] | g* int32 [nq]
        return rank, ws[:4 * nq].view(torch.float32).clone(), ws[4 * nq:8 * nq].view(torch.int32).clone()
    return rank


# ---------------------------------------------------------------------------------------------------------------- 1. integer-exact
def _int_case(nq, ng, E, seed):
    rng = np.random.default_rng(seed)
    q = rng.integers(-3, 4, size=(nq, E)).astype(np.int64)
    g = rng.integers(-3, 4, size=(ng, E)).astype(np.int64)
    s = q @ g.T                                              # |s| <= 9 E: exact in f32 in every summation order
    key = s * ng + np.arange(ng, dtype=np.int64)[None, :]    # monotone in (value, then index): all keys of a row are distinct
    order = np.argsort(-key, axis=1, kind="stable")
    return q, g, s, key, order


@pytest.mark.parametrize("nq,ng,E", [(1, 16, 16), (127, 129, 48), (129, 127, 512), (300, 4133, 512), (5, 70001, 1024)])
def test_integer_scores_exact_with_ties(nq, ng, E):
    q, g, s, key, order = _int_case(nq, ng, E, seed=nq * 1000 + E)
    if (nq, ng) == (300, 4133):      # the premise: most rows have a tie inside their top 17
        top = np.take_along_axis(s, order[:, :17], 1)
        assert (np.diff(top, axis=1) == 0).any(1).mean() > 0.5
    Q = torch.from_numpy(q.astype(np.float32)).to(DEV)
    G = torch.from_numpy(g.astype(np.float32)).to(DEV)
    for k in (1, 5, 16):
        idx, val = c_topk(Q, G, k)
        want = order[:, :k]
        assert np.array_equal(idx.cpu().numpy(), want), (k, "idx")
        assert np.array_equal(val.cpu().numpy(), np.take_along_axis(s, want, 1).astype(np.float32)), (k, "val")
    rng = np.random.default_rng(7)
    for gpr in (1, 5):
        gt = rng.integers(0, ng, size=(nq, gpr)).astype(np.int32)
        gt[rng.random((nq, gpr)) < 0.2] = -1                 # padding, whole rows included
        ref = np.full(nq, NONE, dtype=np.int64)
        for i in range(nq):
            v = gt[i][gt[i] >= 0]
            if len(v):
                ref[i] = int((key[i] > key[i, v].max()).sum())
        rank = c_rank(Q, G, torch.from_numpy(gt).to(DEV))
        assert np.array_equal(rank.cpu().numpy().astype(np.int64), ref), gpr


# ---------------------------------------------------------------------------------------------------------------- 2.-4. float data
NQ, NG, E_F = 300, 4133, 512
TOL = E_F * 2.0 ** -24      # |fl(q . g) - q . g| <= gamma_E sum |q_i g_i| <= gamma_E for unit vectors


@pytest.fixture(scope="module")
def floats():
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
    q, g = q.astype(np.float32), g.astype(np.float32)
    s64 = q.astype(np.float64) @ g.astype(np.float64).T
    return dict(q=q, g=g, gt=gt, planted=planted, s64=s64, Q=torch.from_numpy(q).to(DEV), G=torch.from_numpy(g).to(DEV),
                GT=torch.from_numpy(gt).to(DEV))


def test_float_scores_against_f64(floats):
    s64, gt = floats["s64"], floats["gt"]
    gv = s64[np.arange(NQ), gt]
    lo = (s64 > (gv + 2 * TOL)[:, None]).sum(1)
    hi = (s64 >= (gv - 2 * TOL)[:, None]).sum(1) - 1         # j != g*
    assert (lo == hi).mean() >= 0.5                          # premise, from the reference alone: at least half the intervals are one point
    rank = c_rank(floats["Q"], floats["G"], floats["GT"]).cpu().numpy()
    print(f"rank: {int((lo == hi).sum())} one-point intervals of {NQ}; widest {int((hi - lo).max())}")
    assert ((rank >= lo) & (rank <= hi)).all()
    srt = -np.sort(-s64, axis=1)
    for k in (1, 5, 16):
        idx, val = (t.cpu().numpy() for t in c_topk(floats["Q"], floats["G"], k))
        assert (np.diff(val, axis=1) <= 0).all()
        picked = np.take_along_axis(s64, idx.astype(np.int64), 1)
        print(f"top-{k}: max |val - s64| = {np.abs(val - picked).max():.3e} (tol {TOL:.3e})")
        assert (np.abs(val - picked) <= TOL).all()
        assert (picked >= srt[:, k - 1:k] - 2 * TOL).all()
        assert all(len(set(r)) == k for r in idx.tolist())
        assert idx.min() >= 0 and idx.max() < NG


def test_duplicate_gallery_rows_fall_by_index(floats):
    g2 = floats["g"].copy()
    rows = np.nonzero(floats["planted"])[0]
    larger = np.zeros(NQ, dtype=np.int64)
    for n, i in enumerate(rows):
        j = int(floats["gt"][i])
        g2[j - 5] = g2[j]                                    # a copy at a smaller index: it sorts after the original
        for d in (7, 11)[:n % 3]:                            # 0, 1 or 2 copies at larger indices: they sort before it
            g2[j + d] = g2[j]
        larger[i] = n % 3
    r1 = c_rank(floats["Q"], floats["G"], floats["GT"]).cpu().numpy().astype(np.int64)
    r2 = c_rank(floats["Q"], torch.from_numpy(g2).to(DEV), floats["GT"]).cpu().numpy().astype(np.int64)
    assert np.array_equal(r2[rows], r1[rows] + larger[rows])
    assert set(larger[rows]) == {0, 1, 2}


@pytest.mark.parametrize("data", ["float", "int"])
def test_chunked_gallery_and_consistency(floats, data):
    if data == "float":
        Q, G, GT = floats["Q"], floats["G"], floats["GT"]
    else:
        q, g, _, _, _ = _int_case(NQ, NG, E_F, seed=5)
        Q, G = torch.from_numpy(q.astype(np.float32)).to(DEV), torch.from_numpy(g.astype(np.float32)).to(DEV)
        GT = torch.from_numpy(np.random.default_rng(3).integers(0, NG, size=NQ).astype(np.int32)).to(DEV)
    k = 16
    idx1, val1 = c_topk(Q, G, k)
    if data == "int":      # random ground truth is rarely among the 16 best of 4 133: every other row's becomes its third best
        GT = torch.where(torch.arange(NQ, device=DEV) % 2 == 0, idx1[:, 2], GT)
    cuts = [0, 1500, 1517, NG]                               # three uneven chunks, the middle one 17 rows
    into = None
    for a, b in zip(cuts[:-1], cuts[1:]):
        into = c_topk(Q, G[a:b], k, col_base=a, into=into)
    assert torch.equal(into[0], idx1)
    assert torch.equal(into[1].view(torch.int32), val1.view(torch.int32))      # bit for bit
    # the chunks in another order give the same list too (the order is total)
    into = None
    for a, b in ((1517, NG), (0, 1500), (1500, 1517)):
        into = c_topk(Q, G[a:b], k, col_base=a, into=into)
    assert torch.equal(into[0], idx1) and torch.equal(into[1].view(torch.int32), val1.view(torch.int32))
    rank, thr, gstar = c_rank(Q, G, GT, want_thr=True)
    assert torch.equal(gstar, GT)
    hit = idx1 == GT[:, None]
    assert torch.equal(rank < k, hit.any(1))
    rows, pos = hit.nonzero(as_tuple=True)
    assert len(rows) > 0
    assert torch.equal(val1[rows, pos].view(torch.int32), thr[rows].view(torch.int32))      # the threshold launch computes the sweep's bits
    assert torch.equal(pos.to(torch.int32), rank[rows])                                       # and the rank is the position in the list


# ---------------------------------------------------------------------------------------------------------------- 5. bounds
@pytest.mark.parametrize("nq,ng,E", [(127, 129, 48), (129, 300, 512)])
def test_strided_operands_poisoned_gaps_guarded_outputs(nq, ng, E):
    k, gpr, guard = 5, 2, 64
    rng = np.random.default_rng(11)
    q = rng.integers(-3, 4, size=(nq, E)).astype(np.float32)
    g = rng.integers(-3, 4, size=(ng, E)).astype(np.float32)
    gt = rng.integers(0, ng, size=(nq, gpr)).astype(np.int32)
    Qc, Gc, GT = torch.from_numpy(q).to(DEV), torch.from_numpy(g).to(DEV), torch.from_numpy(gt).to(DEV)
    idx0, val0 = c_topk(Qc, Gc, k)
    rank0 = c_rank(Qc, Gc, GT)
    # NaN in the gaps of every row and in whole rows past n
    Qs = torch.full((nq + 3, E + 4), float("nan"), device=DEV)
    Gs = torch.full((ng + 3, E + 8), float("nan"), device=DEV)
    Qs[:nq, :E] = Qc
    Gs[:ng, :E] = Gc
    ws_t, ws_r = int(_lib.load().lpi_search_workspace(nq, ng, k)), int(_lib.load().lpi_search_workspace(nq, ng, 0))
    ibuf = torch.full((guard + nq * k + guard,), CANARY_I, dtype=torch.int32, device=DEV)
    vbuf = torch.full((guard + nq * k + guard,), CANARY_F, dtype=torch.float32, device=DEV)
    rbuf = torch.full((guard + nq + guard,), CANARY_I, dtype=torch.int32, device=DEV)
    wbuf = torch.full((guard + max(ws_t, ws_r) // 4 + guard,), CANARY_I, dtype=torch.int32, device=DEV)
    idx, val, rank = ibuf[guard:guard + nq * k], vbuf[guard:guard + nq * k], rbuf[guard:guard + nq]
    s = _stream()
    _lib.call("lpi_search_topk", nq, ng, E, Qs, E + 4, Gs, E + 8, k, 0, 0, idx, val, wbuf[guard:], ws_t, s)
    for b, n in ((ibuf, nq * k), (rbuf, 0), (wbuf, ws_t // 4)):
        if n:
            assert (b[:guard] == CANARY_I).all() and (b[guard + n:] == CANARY_I).all()
    assert (vbuf[:guard] == CANARY_F).all() and (vbuf[guard + nq * k:] == CANARY_F).all()
    assert torch.equal(idx.view(nq, k), idx0) and torch.equal(val.view(nq, k).view(torch.int32), val0.view(torch.int32))
    wbuf.fill_(CANARY_I)
    _lib.call("lpi_search_rank", nq, ng, E, Qs, E + 4, Gs, E + 8, GT, gpr, rank, wbuf[guard:], ws_r, s)
    assert (rbuf[:guard] == CANARY_I).all() and (rbuf[guard + nq:] == CANARY_I).all()
    assert (wbuf[:guard] == CANARY_I).all() and (wbuf[guard + ws_r // 4:] == CANARY_I).all()
    assert torch.equal(rank, rank0)
    assert not torch.isnan(val).any()


# ---------------------------------------------------------------------------------------------------------------- 6. memory
def test_topk_memory_is_workspace_plus_outputs():
    from lpi_amd import search
    nq, ng, E, k = 2048, 65536, 512, 10
    gen = torch.Generator(device=DEV).manual_seed(1)
    Q = torch.randn(nq, E, device=DEV, generator=gen)
    G = torch.randn(ng, E, device=DEV, generator=gen)
    search._WS.clear()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    idx, val = search.topk(Q, G, k)
    torch.cuda.synchronize()
    grown = torch.cuda.max_memory_allocated() - base
    ws = int(_lib.load().lpi_search_workspace(nq, ng, k))
    # three allocations (workspace, idx, val), each rounded up to the allocator's 512-byte granule
    bound = ws + 2 * nq * k * 4 + 3 * 512
    print(f"search.topk {nq} x {ng} x {E}: peak growth {grown} bytes (workspace {ws}); the score matrix would be {nq * ng * 4}")
    assert grown <= bound < nq * ng * 4 // 8
    # and the answer is right on a sample of rows (f64 on the host)
    rows = [0, 1, 1027, 2047]
    s64 = Q[rows].double().cpu().numpy() @ G.double().cpu().numpy().T
    picked = np.take_along_axis(s64, idx[rows].cpu().numpy().astype(np.int64), 1)
    atol = 2 * E * 2.0 ** -24 * float(Q[rows].norm(dim=1).max() * G.norm(dim=1).max())      # the dot-product bound at these rows' lengths, both sides
    assert np.allclose(picked, -np.sort(-s64, axis=1)[:, :k], rtol=0, atol=atol)
