"""lpi_search_topk_wide / _wide_t / _wide_mx8 (csrc/search_wide.hip) on a real MI355X, through the C ABI: lists up to k = 256 in one sweep.  Integer
data where every summation order agrees (ties across the cut included), monotone galleries (every column beats the threshold), float data against f64,
the narrow path's bits, chunked galleries, duplicates, strided operands with poisoned gaps and guarded outputs, the launch count and the memory the
Python wrapper takes."""
import numpy as np
import pytest
import torch

from lpi_amd import _lib, search

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CANARY_I, CANARY_F = -0x5A5A5A5B, -12345.5
KINDS = ("f32", "bf16", "f16", "mx8")
_DT = {"bf16": (_lib.BF16, torch.bfloat16), "f16": (_lib.F16, torch.float16)}


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _ws_bytes(nq, ng, k, wide):
    n = int(getattr(_lib.load(), "lpi_search_wide_workspace" if wide else "lpi_search_workspace")(nq, ng, k))
    assert n > 0
    return n


def _operand(kind, x):
    """float32 numpy [n, E] -> what the entry point of `kind` reads: a tensor, or (codes, scales) with every scale byte 127 (small integers: exact)."""
    t = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(DEV)
    if kind == "f32":
        return t
    if kind == "mx8":
        codes = t.to(torch.float8_e4m3fn).view(torch.uint8).contiguous()
        return codes, torch.full((t.shape[0], t.shape[1] // 32), 127, dtype=torch.uint8, device=DEV)
    return t.to(_DT[kind][1])


def _rows(op, a, b):
    return (op[0][a:b], op[1][a:b]) if isinstance(op, tuple) else op[a:b]


def c_topk(kind, Q, G, k, *, wide=True, col_base=0, into=None, nq=None, ng=None, E=None, out=None, ws=None):
    first = Q[0] if isinstance(Q, tuple) else Q
    nq, E = nq or first.shape[0], E or first.shape[1]
    ng = ng or (G[0] if isinstance(G, tuple) else G).shape[0]
    if out is not None:
        idx, val = out
    elif into is None:
        idx = torch.empty(nq, k, dtype=torch.int32, device=DEV)
        val = torch.empty(nq, k, dtype=torch.float32, device=DEV)
    else:
        idx, val = into
    n = _ws_bytes(nq, ng, k, wide)
    if ws is None:
        ws = torch.empty(n, dtype=torch.uint8, device=DEV)
    w = "_wide" if wide else ""
    tail = (k, col_base, 0 if into is None else 1, idx, val, ws, n, _stream())
    if kind == "f32":
        _lib.call(f"lpi_search_topk{w}", nq, ng, E, Q, Q.stride(0), G, G.stride(0), *tail)
    elif kind == "mx8":
        _lib.call(f"lpi_search_topk{w}_mx8", nq, ng, E, Q[0], Q[0].stride(0), Q[1], Q[1].stride(0), G[0], G[0].stride(0), G[1], G[1].stride(0), *tail)
    else:
        _lib.call(f"lpi_search_topk{w}_t", _DT[kind][0], nq, ng, E, Q, Q.stride(0), G, G.stride(0), *tail)
    return idx, val


def _np(pair):
    return pair[0].cpu().numpy(), pair[1].cpu().numpy()


def _bits(v):
    return np.ascontiguousarray(v).view(np.int32)


# ---------------------------------------------------------------------------------------------------------------- 1. integer-exact
def _int_case(nq, ng, E, seed):
    rng = np.random.default_rng(seed)
    q = rng.integers(-3, 4, size=(nq, E)).astype(np.int64)
    g = rng.integers(-3, 4, size=(ng, E)).astype(np.int64)
    s = q @ g.T                                              # |s| <= 9 E: exact in f32 in every summation order
    key = s * ng + np.arange(ng, dtype=np.int64)[None, :]    # monotone in (value, then index): all keys of a row are distinct
    order = np.argsort(-key, axis=1, kind="stable")
    return q, g, s, key, order


INT_CASES = [(1, 17, 16, (17,)), (127, 129, 48, (17, 128, 129)), (129, 300, 512, (17, 256)), (300, 4133, 512, (17, 100, 256)),
             (5, 70001, 1024, (256,))]


@pytest.mark.parametrize("nq,ng,E,ks", INT_CASES)
def test_integer_scores_exact_with_ties(nq, ng, E, ks):
    q, g, s, key, order = _int_case(nq, ng, E, seed=nq * 1000 + E)
    if (nq, ng) == (300, 4133):      # the premise, from the host arrays alone: index order across the cut decides more than half the rows
        for k in (100, 256):
            assert (s[np.arange(nq), order[:, k - 1]] == s[np.arange(nq), order[:, k]]).mean() > 0.5, k
    for kind in KINDS:
        if kind == "mx8" and E % 128:
            continue
        if kind in ("bf16", "f16") and E % 32:
            continue
        Q, G = _operand(kind, q), _operand(kind, g)
        for k in ks:
            idx, val = _np(c_topk(kind, Q, G, k))
            want = order[:, :k]
            assert np.array_equal(idx, want), (kind, k, "idx")
            assert np.array_equal(val, np.take_along_axis(s, want, 1).astype(np.float32)), (kind, k, "val")


# ---------------------------------------------------------------------------------------------------------------- 2. monotone galleries
@pytest.mark.parametrize("permuted", [False, True])
def test_monotone_gallery_threshold_pressure(permuted):
    nq, ng, E = 130, 4133, 16
    g = np.zeros((ng, E), dtype=np.float32)
    g[:, 0] = np.arange(ng) // 3
    q = np.zeros((nq, E), dtype=np.float32)
    q[:, 0] = np.where(np.arange(nq) % 2 == 0, 1.0, -1.0)
    if permuted:
        g = g[np.random.default_rng(11).permutation(ng)]
    s = (q[:, :1].astype(np.int64) * g[:, 0].astype(np.int64)[None, :])
    order = np.argsort(-(s * ng + np.arange(ng, dtype=np.int64)[None, :]), axis=1, kind="stable")
    Q, G = _operand("f32", q), _operand("f32", g)
    for k in (17, 256):
        idx, val = _np(c_topk("f32", Q, G, k))
        assert np.array_equal(idx, order[:, :k]), k
        assert np.array_equal(val, np.take_along_axis(s, order[:, :k], 1).astype(np.float32)), k


# ---------------------------------------------------------------------------------------------------------------- 3.-6. float data
NQ, NG, E_F = 300, 4133, 512
TOL = E_F * 2.0 ** -24      # |fl(q . g) - q . g| <= gamma_E sum |q_i g_i| <= gamma_E for unit vectors


@pytest.fixture(scope="module")
def floats():
    rng = np.random.default_rng(2024)
    q = rng.standard_normal((NQ, E_F)).astype(np.float32)
    g = rng.standard_normal((NG, E_F)).astype(np.float32)
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    g /= np.linalg.norm(g, axis=1, keepdims=True)
    q, g = q.astype(np.float32), g.astype(np.float32)
    ops = {"f32": (_operand("f32", q), _operand("f32", g)), "bf16": (_operand("bf16", q), _operand("bf16", g)),
           "f16": (_operand("f16", q), _operand("f16", g))}
    mq, mg = search.quantize_mx8(ops["f32"][0]), search.quantize_mx8(ops["f32"][1])
    ops["mx8"] = ((mq.codes, mq.scales), (mg.codes, mg.scales))
    return dict(q=q, g=g, s64=q.astype(np.float64) @ g.astype(np.float64).T, ops=ops)


def test_float_scores_against_f64(floats):
    s64 = floats["s64"]
    srt = -np.sort(-s64, axis=1)
    Q, G = floats["ops"]["f32"]
    for k in (17, 100, 256):
        idx, val = _np(c_topk("f32", Q, G, k))
        assert (np.diff(val, axis=1) <= 0).all()
        picked = np.take_along_axis(s64, idx.astype(np.int64), 1)
        print(f"top-{k}: max |val - s64| = {np.abs(val - picked).max():.3e} (tol {TOL:.3e})")
        assert (np.abs(val - picked) <= TOL).all()
        assert (picked >= srt[:, k - 1:k] - 2 * TOL).all()
        assert all(len(set(r)) == k for r in idx.tolist())
        assert idx.min() >= 0 and idx.max() < NG


# bf16 / f16 / MX-FP8 against the f64 product of the rounded / dequantised rows, relative to A = |q| . |g|^T, with the bounds of
# tests/test_search16_gpu.py and tests/test_search_mx8_gpu.py (twice the figure measured there on the same unit Gaussian rows)
TOL_REL = {"bf16": 2 * 3.0736e-07, "f16": 2 * 3.0896e-07, "mx8": 2 * 1.4234e-05}


@pytest.mark.parametrize("kind", ["bf16", "f16", "mx8"])
def test_rounded_operands_against_f64(floats, kind):
    Q, G = floats["ops"][kind]
    if kind == "mx8":
        import mx8_emulate as MX
        q64, g64 = (MX.dequantize(c.cpu(), sc.cpu().contiguous()).double().numpy() for c, sc in (Q, G))
    else:
        q64, g64 = Q.double().cpu().numpy(), G.double().cpu().numpy()
    s64, A, tol = q64 @ g64.T, np.abs(q64) @ np.abs(g64).T, TOL_REL[kind]
    srt = -np.sort(-s64, axis=1)
    for k in (17, 100, 256):
        idx, val = _np(c_topk(kind, Q, G, k))
        picked = np.take_along_axis(s64, idx.astype(np.int64), 1)
        rel = np.abs(val - picked) / np.take_along_axis(A, idx.astype(np.int64), 1)
        print(f"{kind} top-{k}: max |val - s64| / A = {rel.max():.4e} (tol {tol:.4e}; max A {A.max():.5f})")
        assert (np.diff(val, axis=1) <= 0).all()
        assert all(len(set(r)) == k for r in idx.tolist())
        assert idx.min() >= 0 and idx.max() < NG
        assert (rel <= tol).all()
        assert (picked >= srt[:, k - 1:k] - 2 * tol * A.max(1, keepdims=True)).all()


@pytest.mark.parametrize("kind", KINDS)
def test_same_bits_as_the_narrow_path(floats, kind):
    Q, G = floats["ops"][kind]
    ni, nv = _np(c_topk(kind, Q, G, 16, wide=False))
    for k in (16, 17, 256):
        idx, val = _np(c_topk(kind, Q, G, k))
        assert np.array_equal(idx[:, :16], ni), (kind, k)
        assert np.array_equal(_bits(val[:, :16]), _bits(nv)), (kind, k)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("k", [17, 256])
def test_chunked_gallery_equals_one_call(floats, kind, k):
    Q, G = floats["ops"][kind]
    one = _np(c_topk(kind, Q, G, k))
    cuts = [0, 1500, 1517, NG]
    spans = list(zip(cuts[:-1], cuts[1:]))
    empty = lambda: (torch.full((NQ, k), -1, dtype=torch.int32, device=DEV), torch.full((NQ, k), -np.inf, dtype=torch.float32, device=DEV))
    for order, prefill in ((spans, False), ([spans[2], spans[0], spans[1]], False), ([spans[1], spans[0], spans[2]], True)):
        held = empty() if prefill else None      # the 17-row chunk first: fewer rows than k = 256 is legal only when accumulating
        for a, b in order:
            held = c_topk(kind, Q, _rows(G, a, b), k, col_base=a, into=held)
        got = _np(held)
        assert np.array_equal(got[0], one[0]), (kind, k, order)
        assert np.array_equal(_bits(got[1]), _bits(one[1])), (kind, k, order)


def test_chunked_integer_data_equals_one_call():
    q, g, s, key, order = _int_case(300, 4133, 512, seed=300512)
    Q, G = _operand("f32", q), _operand("f32", g)
    for k in (17, 256):
        held = None
        for a, b in ((1517, 4133), (0, 1500), (1500, 1517)):
            held = c_topk("f32", Q, G[a:b], k, col_base=a, into=held)
        idx, val = _np(held)
        assert np.array_equal(idx, order[:, :k]), k
        assert np.array_equal(val, np.take_along_axis(s, order[:, :k], 1).astype(np.float32)), k


def test_duplicate_gallery_rows_fall_by_index(floats):
    q, g2 = floats["q"], floats["g"].copy()
    rows = np.arange(0, NQ, 2)
    home = 13 + 27 * (rows // 2)
    larger = np.zeros(NQ, dtype=np.int64)
    for n, (i, j) in enumerate(zip(rows, home)):
        g2[j] = q[i]                                         # the planted best row of query row i
        g2[j - 5] = g2[j]                                    # a copy at a smaller index: it sorts after the original
        for d in (7, 11)[:n % 3]:                            # 0, 1 or 2 copies at larger indices: they sort before it
            g2[j + d] = g2[j]
        larger[i] = n % 3
    idx, val = _np(c_topk("f32", floats["ops"]["f32"][0], _operand("f32", g2), 100))
    for i, j in zip(rows, home):
        want = [j + d for d in (11, 7)[2 - larger[i]:]] + [j, j - 5]
        assert idx[i, :len(want)].tolist() == want, i
        assert len(set(_bits(val[i, :len(want)]).tolist())) == 1, i


# ---------------------------------------------------------------------------------------------------------------- 7. bounds
@pytest.mark.parametrize("nq,ng,E,k", [(127, 129, 48, 100), (129, 300, 512, 256)])
def test_strided_operands_poisoned_gaps_guarded_outputs(nq, ng, E, k):
    rng = np.random.default_rng(nq + ng)
    q = rng.standard_normal((nq, E)).astype(np.float32)
    g = rng.standard_normal((ng, E)).astype(np.float32)
    Q, G = _operand("f32", q), _operand("f32", g)
    want = _np(c_topk("f32", Q, G, k))

    def strided(t, ld, extra):      # NaN in every gap and in whole rows past n
        buf = torch.full((t.shape[0] + extra, ld), float("nan"), dtype=torch.float32, device=DEV)
        buf[:t.shape[0], :E] = t
        return buf

    Qs, Gs = strided(Q, E + 12, 3), strided(G, E + 4, 5)
    GUARD = 64
    ib = torch.full((nq * k + 2 * GUARD,), CANARY_I, dtype=torch.int32, device=DEV)
    vb = torch.full((nq * k + 2 * GUARD,), CANARY_F, dtype=torch.float32, device=DEV)
    n = _ws_bytes(nq, ng, k, True)
    wb = torch.full((n + 512,), 0xA5, dtype=torch.uint8, device=DEV)
    out = (ib[GUARD:GUARD + nq * k].view(nq, k), vb[GUARD:GUARD + nq * k].view(nq, k))
    got = _np(c_topk("f32", Qs, Gs, k, nq=nq, ng=ng, E=E, out=out, ws=wb[256:256 + n]))
    assert np.array_equal(got[0], want[0]) and np.array_equal(_bits(got[1]), _bits(want[1]))
    assert not np.isnan(got[1]).any()
    for buf, c in ((ib, CANARY_I), (vb, CANARY_F)):
        assert (buf[:GUARD] == c).all() and (buf[-GUARD:] == c).all()
    assert (wb[:256] == 0xA5).all() and (wb[-256:] == 0xA5).all()


@pytest.mark.parametrize("nq,ng,E,k", [(127, 129, 128, 100), (129, 300, 512, 256)])      # E = 48 is outside the MX-FP8 envelope: its smallest E instead
def test_strided_mx8_operands_poisoned_gaps_guarded_outputs(nq, ng, E, k):
    q, g, s, key, order = _int_case(nq, ng, E, seed=nq * 1000 + E)
    (Qc, Qs), (Gc, Gs) = _operand("mx8", q), _operand("mx8", g)
    want = _np(c_topk("mx8", (Qc, Qs), (Gc, Gs), k))
    assert np.array_equal(want[0], order[:, :k])
    ldq, ldg, ldqs, ldgs = E + 16, E + 32, E // 32 + 4, E // 32 + 8
    # NaN element bytes (0x7F) in the gaps of every row and in three whole rows past n; the NaN scale byte (0xFF) likewise
    Qw = torch.full((nq + 3, ldq), 0x7F, device=DEV, dtype=torch.uint8)
    Gw = torch.full((ng + 3, ldg), 0x7F, device=DEV, dtype=torch.uint8)
    Qsw = torch.full((nq + 3, ldqs), 0xFF, device=DEV, dtype=torch.uint8)
    Gsw = torch.full((ng + 3, ldgs), 0xFF, device=DEV, dtype=torch.uint8)
    Qw[:nq, :E], Gw[:ng, :E], Qsw[:nq, :E // 32], Gsw[:ng, :E // 32] = Qc, Gc, Qs, Gs
    GUARD = 64
    ib = torch.full((nq * k + 2 * GUARD,), CANARY_I, dtype=torch.int32, device=DEV)
    vb = torch.full((nq * k + 2 * GUARD,), CANARY_F, dtype=torch.float32, device=DEV)
    n = _ws_bytes(nq, ng, k, True)
    wb = torch.full((n + 512,), 0xA5, dtype=torch.uint8, device=DEV)
    out = (ib[GUARD:GUARD + nq * k].view(nq, k), vb[GUARD:GUARD + nq * k].view(nq, k))
    got = _np(c_topk("mx8", (Qw, Qsw), (Gw, Gsw), k, nq=nq, ng=ng, E=E, out=out, ws=wb[256:256 + n]))
    assert np.array_equal(got[0], want[0]) and np.array_equal(_bits(got[1]), _bits(want[1]))
    assert not np.isnan(got[1]).any()
    for buf, c in ((ib, CANARY_I), (vb, CANARY_F)):
        assert (buf[:GUARD] == c).all() and (buf[-GUARD:] == c).all()
    assert (wb[:256] == 0xA5).all() and (wb[-256:] == 0xA5).all()


# ---------------------------------------------------------------------------------------------------------------- 8. launch count
def test_launch_count_does_not_depend_on_k_or_ng():
    rng = np.random.default_rng(5)
    Q = _operand("f32", rng.standard_normal((5, 64)))
    counts = []
    for ng, k in ((300, 17), (70001, 256)):
        G = _operand("f32", rng.standard_normal((ng, 64)))
        before = _lib.launch_count()
        c_topk("f32", Q, G, k)
        counts.append(_lib.launch_count() - before)
    assert counts[0] == counts[1] == 2, counts


# ---------------------------------------------------------------------------------------------------------------- 9. Python and memory
def _requested():
    """(current, peak) of the bytes the allocator was ASKED for: unlike the allocated bytes they do not depend on which cached block serves a request
    (a free block up to 1 MiB larger than a request is handed out whole, and what earlier tests left behind decides whether there is one)."""
    st = torch.cuda.memory_stats()
    return st["requested_bytes.all.current"], st["requested_bytes.all.peak"]


def test_wrapper_wide_memory_and_values():
    nq, ng, E, k = 256, 65536, 512, 256
    gen = torch.Generator(device="cpu").manual_seed(9)
    Q = torch.randn(nq, E, generator=gen).to(DEV)
    G = torch.randn(ng, E, generator=gen).to(DEV)
    search._WS.clear()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    base, rbase = torch.cuda.memory_allocated(), _requested()[0]
    idx, val = search.topk(Q, G, k)
    torch.cuda.synchronize()
    grown, asked = torch.cuda.max_memory_allocated() - base, _requested()[1] - rbase
    need = _ws_bytes(nq, ng, k, True) + 2 * nq * k * 4
    print(f"wide top-{k}: peak growth {grown} bytes, asked for {asked}, workspace + outputs {need}, score matrix {nq * ng * 4}")
    assert asked == need      # the workspace and the two outputs, nothing else
    assert grown <= need + 3 * (2 << 20)      # three allocations; the allocator's coarsest granule is 2 MiB (requests above 10 MiB)
    for i in (0, 77, 128, 255):
        s = Q[i].double().cpu().numpy() @ G.double().cpu().numpy().T
        ref = np.argsort(-s, kind="stable")[:k]
        got = idx[i].cpu().numpy()
        tol = 2 * E * 2.0 ** -24 * float(Q[i].norm()) * float(G.norm(dim=1).max())
        assert (s[got] >= s[ref[-1]] - tol).all() and len(set(got.tolist())) == k
        assert np.abs(val[i].cpu().numpy() - s[got]).max() <= tol
    # 2-byte and MX-FP8 operands are read in place, and the wrapper gives the C-ABI call's lists
    Qb, Gb = Q.bfloat16(), G[:4133].bfloat16()
    mq, mg = search.quantize_mx8(Q), search.quantize_mx8(G[:4133])
    for kind, args, ops in (("bf16", (Qb, Gb), (Qb, Gb)), ("mx8", (mq, mg), ((mq.codes, mq.scales), (mg.codes, mg.scales)))):
        search.topk(*args, 100, operands=kind)      # the workspace is in place
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        rbase = _requested()[0]
        pi, pv = search.topk(*args, 100, operands=kind)
        torch.cuda.synchronize()
        asked = _requested()[1] - rbase
        print(f"wide top-100 [{kind}]: asked for {asked} bytes; the gallery is {4133 * E * (2 if kind == 'bf16' else 1)} bytes or more")
        assert asked == 2 * nq * 100 * 4, kind      # the outputs only: no copy of an operand, no second workspace
        ci, cv = c_topk(kind, *ops, 100)
        assert torch.equal(pi, ci) and torch.equal(pv.view(torch.int32), cv.view(torch.int32)), kind
    # the narrow path allocates what it allocated: lpi_search_workspace and the two outputs
    search._WS.clear()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    rbase = _requested()[0]
    search.topk(Q, G[:4133], 10)
    torch.cuda.synchronize()
    asked, n10 = _requested()[1] - rbase, _ws_bytes(nq, 4133, 10, False)
    print(f"narrow top-10: asked for {asked} bytes, lpi_search_workspace + outputs {n10 + 2 * nq * 10 * 4}")
    assert asked == n10 + 2 * nq * 10 * 4
