"""lpi_search_rerank / _rerank_t (csrc/search_rerank.hip) and lpi_amd.search.rerank / topk_reranked on a real MI355X: integer data where every summation
order agrees (ties across the cut included), the sweep's bits on float data, scores against f64, padding and repeated candidates, strided operands with
poisoned gaps and guarded outputs, the launch count, the two stages end to end against the f32 search, and what the Python wrapper allocates."""
import numpy as np
import pytest
import torch

from lpi_amd import _lib, search

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CANARY_I, CANARY_F = -0x5A5A5A5B, -12345.5
KINDS = ("f32", "bf16", "f16")
_DT = {"f32": (_lib.F32, torch.float32), "bf16": (_lib.BF16, torch.bfloat16), "f16": (_lib.F16, torch.float16)}
NONE = np.iinfo(np.int64).min      # the key of an empty slot


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _operand(kind, x):
    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(DEV).to(_DT[kind][1])


def _cand(c):
    return torch.from_numpy(np.ascontiguousarray(c, dtype=np.int32)).to(DEV)


def c_rerank(kind, Q, G, cand, k, *, nq=None, ng=None, E=None, kc=None, out=None):
    """The C ABI call: the f32 form for f32, the typed form otherwise.  Sizes default to the tensors' shapes (strided views pass their own)."""
    nq, E = nq or Q.shape[0], E or Q.shape[1]
    ng, kc = ng or G.shape[0], kc or cand.shape[1]
    if out is None:
        out = (torch.empty(nq, k, dtype=torch.int32, device=DEV), torch.empty(nq, k, dtype=torch.float32, device=DEV))
    args = (nq, ng, E, Q, Q.stride(0), G, G.stride(0), cand, cand.stride(0), kc, k, out[0], out[1], _stream())
    if kind == "f32":
        _lib.call("lpi_search_rerank", *args)
    else:
        _lib.call("lpi_search_rerank_t", _DT[kind][0], *args)
    return out


def _np(pair):
    return pair[0].cpu().numpy(), pair[1].cpu().numpy()


def _bits(v):
    return np.ascontiguousarray(v).view(np.int32)


def _same(a, b):
    return torch.equal(a[0], b[0]) and torch.equal(a[1].view(torch.int32), b[1].view(torch.int32))


def _expected(s, cand, k):
    """Integer scores s [nq, ng] (int64), candidates [nq, kc] (int64, any values) -> (idx [nq, k], val f32 [nq, k]): the distinct valid candidates by
    (score descending, index descending), then (-1, -inf).  key = score * ng + index is monotone in that order and distinct for distinct indices."""
    ng = s.shape[1]
    valid = (cand >= 0) & (cand < ng)
    cc = np.where(valid, cand, 0)
    key = np.where(valid, np.take_along_axis(s, cc, 1) * ng + cc, NONE)
    key = -np.sort(-key.astype(np.float64), axis=1)      # |key| < 2^53: exact as f64, and -NONE does not overflow there
    dup = np.zeros(key.shape, dtype=bool)
    dup[:, 1:] = key[:, 1:] == key[:, :-1]
    key = -np.sort(-np.where(dup, float(NONE), key), axis=1)[:, :k]
    empty = key == float(NONE)
    ki = np.where(empty, 0, key).astype(np.int64)
    idx = np.where(empty, -1, ki % ng).astype(np.int32)
    val = np.where(empty, -np.inf, (ki // ng).astype(np.float64)).astype(np.float32)
    return idx, val, empty


# ---------------------------------------------------------------------------------------------------------------- 1. integer-exact
def _int_case(nq, ng, E, seed):
    """Entries in {-1, 0, 1}: exact in f32, bf16 and f16, every partial sum an integer below 2^11, so every summation order gives the same f32.  The
    narrow range (a score's deviation is about 0.67 sqrt(E)) makes equal scores among a row's candidates common: the index order decides the cut."""
    rng = np.random.default_rng(seed)
    q = rng.integers(-1, 2, size=(nq, E)).astype(np.int64)
    g = rng.integers(-1, 2, size=(ng, E)).astype(np.int64)
    s = (q.astype(np.float64) @ g.astype(np.float64).T).astype(np.int64)      # exact: |s| <= E
    return q, g, s


SHAPES = [(1, 17, 16), (5, 40, 48), (127, 129, 512), (300, 4133, 512), (130, 300, 1024)]      # E = 16 / 48 become 32 / 96 for the 2-byte types
KCS = (1, 16, 17, 100, 255, 256)


def _e_of(kind, E):
    return E if kind == "f32" else {16: 32, 48: 96}.get(E, E)


def _ks(kc):
    return sorted({1, (kc + 1) // 2, kc})


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("nq,ng,E", SHAPES)
def test_integer_scores_exact_with_ties(nq, ng, E, kind):
    E = _e_of(kind, E)
    q, g, s = _int_case(nq, ng, E, seed=nq * 1000 + E)
    rng = np.random.default_rng(nq + ng)
    cases = []
    for kc in sorted({min(kc, ng) for kc in KCS}):
        cand = rng.integers(0, ng, size=(nq, kc)).astype(np.int64)      # with replacement: repeated indices occur
        cases.append((kc, cand, {k: _expected(s, cand, k) for k in _ks(kc)}))
    if (nq, ng) == (300, 4133):      # the premise, from the host arrays alone: in most rows index order decides who makes the cut
        for kc, cand, want in cases:
            if kc >= 100:
                k = (kc + 1) // 2
                wi, wv, _ = _expected(s, cand, k + 1)
                tied = (wv[:, k - 1] == wv[:, k]) & (wi[:, k] >= 0)
                print(f"kc = {kc}, k = {k}: equal scores at positions k - 1 and k in {tied.mean():.3f} of the rows")
                assert tied.mean() >= 0.5, (kc, k)
    Q, G = _operand(kind, q), _operand(kind, g)
    for kc, cand, want in cases:
        C = _cand(cand)
        for k, (wi, wv, _) in want.items():
            idx, val = _np(c_rerank(kind, Q, G, C, k))
            assert np.array_equal(idx, wi), (kind, kc, k, "idx")
            assert np.array_equal(_bits(val), _bits(wv)), (kind, kc, k, "val")


# ---------------------------------------------------------------------------------------------------------------- 2., 3. float data
NQ, NG, E_F = 300, 4133, 512
TOL = E_F * 2.0 ** -24      # |fl(q . g) - q . g| <= gamma_E sum |q_i g_i| <= gamma_E for unit vectors (tests/test_search_wide_gpu.py)
TOL_REL = {"bf16": 2 * 3.0736e-07, "f16": 2 * 3.0896e-07}      # that file's bounds for the 2-byte types, relative to |q| . |g|


def _unit_rows(rng, n, E):
    x = rng.standard_normal((n, E)).astype(np.float32)
    return (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float32)


@pytest.fixture(scope="module")
def floats():
    rng = np.random.default_rng(2025)
    q, g = _unit_rows(rng, NQ, E_F), _unit_rows(rng, NG, E_F)
    ops = {kind: (_operand(kind, q), _operand(kind, g)) for kind in KINDS}
    wide = {kind: search.topk(*ops[kind], 256, operands=kind) for kind in KINDS}
    return dict(ops=ops, wide=wide, rng=np.random.default_rng(77))


@pytest.mark.parametrize("kind", KINDS)
def test_permuted_wide_list_comes_back_bit_for_bit(floats, kind):
    Q, G = floats["ops"][kind]
    wide = floats["wide"][kind]
    perm = torch.from_numpy(np.argsort(floats["rng"].random((NQ, 256)), axis=1)).to(DEV)
    cand = torch.gather(wide[0], 1, perm).contiguous()
    assert not torch.equal(cand, wide[0])
    assert _same(search.rerank(Q, G, cand, operands=kind), wide), kind
    assert _same(c_rerank(kind, Q, G, cand, 256), wide), kind
    got = search.rerank(Q, G, cand, 100, operands=kind)
    assert _same(got, (wide[0][:, :100].contiguous(), wide[1][:, :100].contiguous())), kind


@pytest.mark.parametrize("kind", KINDS)
def test_narrow_list_among_random_others(floats, kind):
    Q, G = floats["ops"][kind]
    narrow = search.topk(Q, G, 16, operands=kind)
    rng = floats["rng"]
    others = torch.from_numpy(rng.integers(0, NG, size=(NQ, 84)).astype(np.int32)).to(DEV)
    perm = torch.from_numpy(np.argsort(rng.random((NQ, 100)), axis=1)).to(DEV)
    cand = torch.gather(torch.cat([narrow[0], others], 1), 1, perm).contiguous()
    idx, val = search.rerank(Q, G, cand, 100, operands=kind)
    assert _same((idx[:, :16].contiguous(), val[:, :16].contiguous()), narrow), kind


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", ["unit", "half-slab"])
def test_every_score_is_the_one_row_search(floats, kind, shape):
    """val of a returned entry == the val a one-row topk over gallery[idx : idx + 1] gives for the pair: 64 sampled entries."""
    rng = floats["rng"]
    if shape == "unit":
        Q, G = floats["ops"][kind]
        cand = torch.from_numpy(rng.integers(0, NG, size=(NQ, 100)).astype(np.int32)).to(DEV)
    else:      # E % BK == BK / 2: the shortened last slab
        E = _e_of(kind, 48)
        Q, G = _operand(kind, _unit_rows(rng, 5, E)), _operand(kind, _unit_rows(rng, 40, E))
        cand = torch.from_numpy(rng.integers(0, 40, size=(5, 40)).astype(np.int32)).to(DEV)
    idx, val = search.rerank(Q, G, cand, operands=kind)
    hi, hv = _np((idx, val))
    filled = np.argwhere(hi >= 0)
    for i, p in filled[rng.choice(len(filled), size=64, replace=False)]:
        j = int(hi[i, p])
        oi, ov = search.topk(Q[i:i + 1], G[j:j + 1], 1, operands=kind)
        assert int(oi[0, 0]) == 0
        assert _bits(ov.cpu().numpy())[0, 0] == _bits(hv)[i, p], (kind, shape, i, p, j)


@pytest.mark.parametrize("kind", KINDS)
def test_scores_against_f64(floats, kind):
    Q, G = floats["ops"][kind]
    q64, g64 = Q.double().cpu().numpy(), G.double().cpu().numpy()      # the rows as the kernel reads them (rounded for the 2-byte types)
    cand = floats["rng"].integers(0, NG, size=(NQ, 256))
    idx, val = _np(search.rerank(Q, G, _cand(cand), operands=kind))
    wi = np.where(idx >= 0, idx, 0).astype(np.int64)
    s64 = np.take_along_axis(q64 @ g64.T, wi, 1)
    if kind == "f32":
        err, tol = np.abs(val - s64), TOL
    else:
        err, tol = np.abs(val - s64) / np.take_along_axis(np.abs(q64) @ np.abs(g64).T, wi, 1), TOL_REL[kind]
    err = np.where(idx >= 0, err, 0.0)
    print(f"{kind}: max error {err.max():.4e} (tol {tol:.4e})")
    assert (idx >= 0).sum() == sum(len(set(r)) for r in cand.tolist())
    assert (err <= tol).all()
    assert (val[:, 1:] <= val[:, :-1]).all() and np.isneginf(val[idx < 0]).all()      # descending, the empty slots (-inf) last


# ---------------------------------------------------------------------------------------------------------------- 4. padding and duplicates
@pytest.mark.parametrize("kind", KINDS)
def test_padding_and_repeated_candidates(kind):
    nq, ng, kc, k = 7, 40, 24, 12
    E = _e_of(kind, 48)
    q, g, s = _int_case(nq, ng, E, seed=4)
    rng = np.random.default_rng(44)
    pads = np.array([-1, ng, ng + 7, 2 ** 31 - 1, -2 ** 31, -5])
    cand = np.empty((nq, kc), dtype=np.int64)
    cand[0] = rng.permutation(np.concatenate([pads, [3, 9, 9, 17, 3, 39, 21, 9], rng.integers(1, ng, 10)]))      # everything mixed
    cand[1] = rng.choice(pads, kc)                                                                               # all padding
    cand[2] = rng.permutation(np.concatenate([[5, 7, 11, 13, 29] * 3, rng.choice(pads, kc - 15)]))               # 5 distinct valid entries < k
    cand[3] = 23                                                                                                 # one index kc times
    cand[4] = rng.integers(1, ng, kc)
    cand[5] = np.concatenate([np.full(kc - 3, -1), [2, 38, 2]])                                                  # the valid ones last
    cand[6] = np.concatenate([np.arange(1, 13), np.arange(1, 13)])                                               # exactly k distinct, each twice
    assert not (cand == 0).any()      # row 0 stands in for padding: it stays unlisted, and is NaN below
    wi, wv, empty = _expected(s, cand, k)
    assert empty[1].all() and empty[2].sum() == k - 5 and empty[3].sum() == k - 1 and not empty[6].any()
    Q, C = _operand(kind, q), _cand(cand)
    got = _np(c_rerank(kind, Q, _operand(kind, g), C, k))
    assert np.array_equal(got[0], wi) and np.array_equal(_bits(got[1]), _bits(wv)), kind
    listed = np.unique(cand[(cand >= 0) & (cand < ng)])
    gn = g.astype(np.float32)
    gn[np.setdiff1d(np.arange(ng), listed)] = np.nan
    assert np.isnan(gn[0]).all() and np.isnan(gn).any(axis=1).sum() == ng - len(listed) > 0
    poisoned = _np(c_rerank(kind, Q, _operand(kind, gn), C, k))
    assert np.array_equal(poisoned[0], wi) and np.array_equal(_bits(poisoned[1]), _bits(wv)), kind
    full = _np(c_rerank(kind, Q, _operand(kind, gn), C, kc))      # k = kc: the fill reaches the end of the row
    fi, fv, _ = _expected(s, cand, kc)
    assert np.array_equal(full[0], fi) and np.array_equal(_bits(full[1]), _bits(fv)), kind


# ---------------------------------------------------------------------------------------------------------------- 5. bounds
@pytest.mark.parametrize("kind", ["f32", "bf16"])
@pytest.mark.parametrize("nq,ng,E,kc,k", [(5, 40, 48, 17, 9), (130, 300, 1024, 256, 256), (127, 129, 512, 100, 100)])
def test_strided_operands_poisoned_gaps_guarded_outputs(nq, ng, E, kc, k, kind):
    E = _e_of(kind, E)
    rng = np.random.default_rng(nq + ng)
    dtype = _DT[kind][1]
    Q, G = _operand(kind, _unit_rows(rng, nq, E)), _operand(kind, _unit_rows(rng, ng, E))
    cand = rng.integers(0, ng, size=(nq, kc)).astype(np.int32)
    cand[:, ::7] = -1
    C = _cand(cand)
    want = c_rerank(kind, Q, G, C, k)

    def strided(t, ld, extra):      # NaN in every gap and in whole rows past n
        buf = torch.full((t.shape[0] + extra, ld), float("nan"), dtype=dtype, device=DEV)
        buf[:t.shape[0], :E] = t
        return buf

    Qs, Gs = strided(Q, E + 24, 3), strided(G, E + 8, 5)
    ldc = kc + 5
    junk = torch.tensor([2 ** 30, 1, -7, ng, 2], dtype=torch.int32, device=DEV)
    Cw = junk.repeat((nq + 2) * ldc // 5 + 1)[:(nq + 2) * ldc].view(nq + 2, ldc).clone()
    Cw[:nq, :kc] = C      # the gaps and the rows past nq: out-of-range junk, and in-range junk that a read past kc would turn into candidates
    GUARD = 64
    ib = torch.full((nq * k + 2 * GUARD,), CANARY_I, dtype=torch.int32, device=DEV)
    vb = torch.full((nq * k + 2 * GUARD,), CANARY_F, dtype=torch.float32, device=DEV)
    out = (ib[GUARD:GUARD + nq * k].view(nq, k), vb[GUARD:GUARD + nq * k].view(nq, k))
    got = c_rerank(kind, Qs, Gs, Cw, k, nq=nq, ng=ng, E=E, kc=kc, out=out)
    assert _same(got, want)
    assert not torch.isnan(got[1]).any()
    for buf, c in ((ib, CANARY_I), (vb, CANARY_F)):
        assert (buf[:GUARD] == c).all() and (buf[-GUARD:] == c).all()
    # the Python wrapper reads the same views in place
    assert _same(search.rerank(Qs[:nq, :E], Gs[:ng, :E], Cw[:nq, :kc], k, operands=kind), want)


# ---------------------------------------------------------------------------------------------------------------- 6. launch count
def test_one_launch_per_call():
    rng = np.random.default_rng(6)
    Q, G = _operand("f32", _unit_rows(rng, 130, 64)), _operand("f32", _unit_rows(rng, 300, 64))
    for kind in KINDS:
        Qk, Gk = Q.to(_DT[kind][1]), G.to(_DT[kind][1])
        for kc, k in ((1, 1), (100, 10), (256, 256)):
            C = _cand(rng.integers(0, 300, size=(130, kc)))
            before = _lib.launch_count()
            c_rerank(kind, Qk, Gk, C, k)
            assert _lib.launch_count() - before == 1, (kind, kc, k)


# ---------------------------------------------------------------------------------------------------------------- 7. two stages end to end
def test_two_stages_equal_the_f32_search():
    import mx8_emulate as MX
    nq, ng, E, k = 300, 4133, 512, 10
    rng = np.random.default_rng(7)
    q, g = _unit_rows(rng, nq, E).astype(np.float64), _unit_rows(rng, ng, E).astype(np.float64)
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    homes = rng.permutation(ng)[:nq * k].reshape(nq, k)      # distinct gallery rows: k per query
    cos = np.linspace(0.50, 0.86, k)
    for i in range(nq):
        u = rng.standard_normal((k, E))
        u -= (u @ q[i])[:, None] * q[i][None, :]
        u /= np.linalg.norm(u, axis=1, keepdims=True)
        g[homes[i]] = cos[:, None] * q[i][None, :] + np.sqrt(1 - cos ** 2)[:, None] * u
    q32, g32 = q.astype(np.float32), g.astype(np.float32)
    # the premise, on the host: the planted rows stay ahead of every other row through the MX-FP8 rounding of both operands
    s64 = q32.astype(np.float64) @ g32.astype(np.float64).T
    planted = np.zeros((nq, ng), dtype=bool)
    np.put_along_axis(planted, homes, True, 1)
    gap = float(np.where(planted, s64, np.inf).min() - np.where(planted, -np.inf, s64).max())
    deq = [MX.dequantize(*MX.quantize(torch.from_numpy(x))).double().numpy() for x in (q32, g32)]
    dev = float(np.abs(deq[0] @ deq[1].T - s64).max())
    print(f"gap {gap:.4f}, dev {dev:.5f}")
    assert gap > 2 * dev + 2 * 8.6e-5

    Q, G = torch.from_numpy(q32).to(DEV), torch.from_numpy(g32).to(DEV)
    want = search.topk(Q, G, k, operands="f32")
    assert np.array_equal(np.sort(want[0].cpu().numpy(), axis=1), np.sort(homes, axis=1))
    for coarse in ("mx8", "bf16"):
        assert _same(search.topk_reranked(Q, G, k, coarse=coarse, candidates=20), want), coarse
        assert _same(search.topk_reranked(Q, G, k, coarse=coarse), want), coarse      # the default: 40 candidates, the wide kernels
    held = search.quantize_mx8(G)
    assert _same(search.topk_reranked(Q, G, k, coarse="mx8", candidates=20, coarse_gallery=held), want)
    assert _same(search.topk_reranked(Q, G, k, coarse="mx8", candidates=20, coarse_gallery=held, coarse_queries=search.quantize_mx8(Q)), want)
    assert _same(search.topk_reranked(Q, G, k, coarse="bf16", candidates=16, coarse_gallery=G.bfloat16()), want)
    # a coarse gallery searched in chunks, then one re-rank on the whole exact gallery
    lists = None
    for a, b in ((0, 1500), (1500, 1517), (1517, ng)):
        lists = search.topk(Q, held[a:b], 20, col_base=a, into=lists, operands="mx8")
    assert _same(search.rerank(Q, G, lists[0], k), want)


# ---------------------------------------------------------------------------------------------------------------- 8. the wrapper
def _requested():
    """(current, peak) of the bytes the allocator was ASKED for (tests/test_search_wide_gpu.py): they do not depend on which cached block serves a request."""
    st = torch.cuda.memory_stats()
    return st["requested_bytes.all.current"], st["requested_bytes.all.peak"]


def test_wrapper_converts_cand_once_and_reads_operands_in_place():
    nq, ng, E, kc, k = 256, 4133, 512, 100, 10
    gen = torch.Generator(device="cpu").manual_seed(8)
    Q, G = torch.randn(nq, E, generator=gen).to(DEV), torch.randn(ng, E, generator=gen).to(DEV)
    cand64 = torch.randint(0, ng, (nq, kc), generator=gen)
    cand64[:, 3] = -1
    cand64[:, 5] = 2 ** 32 + 17      # would be index 17 if it were truncated to 32 bits: it is padding
    cand64[:, 7] = ng
    c32 = torch.where((cand64 < 0) | (cand64 >= ng), torch.full_like(cand64, -1), cand64).to(torch.int32).to(DEV)
    want = search.rerank(Q, G, c32, k)
    assert _same(want, c_rerank("f32", Q, G, c32, k))
    for other in (cand64, cand64.to(DEV), c32.cpu(), c32.t().contiguous().t()):      # int64 on the host / the device, int32 on the host, a column-major one
        got = search.rerank(Q, G, other, k)
        assert got[0].dtype == torch.int32 and _same(got, want)
    Qb, Gb = Q.bfloat16(), G.bfloat16()
    wantb = c_rerank("bf16", Qb, Gb, c32, k)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    rbase = _requested()[0]
    got = search.rerank(Qb, Gb, c32, k, operands="bf16")
    torch.cuda.synchronize()
    asked = _requested()[1] - rbase
    print(f"rerank [bf16]: asked for {asked} bytes; the gallery is {ng * E * 2} bytes")
    assert asked == 2 * nq * k * 4      # the outputs only: no copy of an operand or of cand, no workspace
    assert _same(got, wantb)
