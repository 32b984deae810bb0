"""The GEMM family held to its five leading dimensions and its write bounds on a real MI355X: lpi_gemm_nt, lpi_gemm_nt_grouped and lpi_gemm_nt_rows on the
128x128, one-tile 256x256, persistent 256x256 (half-width staging, LDS-DMA side tiles, LN-fold and row-statistics epilogues), 256x128, hybrid-tail and 32x32
few-row kernels.

Every case runs its call twice under the same tuning keys: the STRIDED arm on tests/strided.py views (offset base pointers, lda / ldb / ldc / ldr / ldaux all
different from each other and from the widths, NaN in every pad), the TIGHT arm on contiguous copies of the same values.  Asserted in each case:
  * lpi_gemm_last_kernel() names the kernel the case is meant to reach, in both arms;
  * every output of the strided arm equals the tight arm's bit for bit (a leading dimension changes no arithmetic and no summation order);
  * no pad of any operand, inputs included, changed, and every output element was written;
  * the tight arm meets the f64 CPU reference at the bar of the kernel's existing test (TOL of test_kernels_gpu.py, 2e-3 / 1e-3 for f16 outputs / f16 operands
    into f32, 6e-3 for the LN fold's bf16 outputs, the bf16x3 bar of test_bf16x3_gpu.py against the exact f32 kernel).
A kernel that indexes the residual with ldc, the saved gelu' tile with ldr or the A panel with K reads NaN or writes a pad; every arena of a case is sized by
strided.arena_bytes from the case's largest row count, leading dimension and element size, so such a kernel fails an assertion and never leaves an allocation.

Leading dimensions: "tier1" = K + 32, K + 64, N + 8, N + 16, N + 24 elements with a 16-byte base offset; "min16" = the smallest steps the argument checks accept
(one, two, three 16-byte units per operand type); "engine" = the last block's own shape, the right two thirds of a [rows, 1.5 x width] buffer
(lpi_amd/engine.py: C = qkv[:, d:], A = dqkv[:, d:], B = wqt[:, d:]).  What the checks refuse (8-byte row ends: DESIGN.md section 4) is tested to launch nothing.
"""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

import bf16x3_emulate as X3  # noqa: E402
import strided as S  # noqa: E402
from lpi_amd import _lib  # noqa: E402
from lpi_amd._lib import (BF16, EPI_DQUICKGELU, EPI_LN, EPI_LN_QUICKGELU, EPI_NONE, EPI_QUICKGELU, EPI_RES_ROWSTATS, F16, F32, F32X3, GEMM_K_128, GEMM_K_256,  # noqa: E402
                          GEMM_K_256_TAIL, GEMM_K_256X128, GEMM_K_ROWS, GEMM_K_X3, call)
from poison import relerr, same_bits  # noqa: E402

DEV = "cuda:0"
TD = {F32: torch.float32, F32X3: torch.float32, BF16: torch.bfloat16, F16: torch.float16}
AUX_TD = {F32: torch.float32, F32X3: torch.float32, BF16: torch.bfloat16, F16: torch.bfloat16}      # gemm_epilogue.h, AuxT
TOL = {F32: 2e-5, BF16: 2e-2}      # tests/test_kernels_gpu.py
U16 = 2.0 ** -16
DEFAULT_KEYS = {0: 1, 1: 1500, 2: 0, 5: 160, 6: 1, 8: 0, 14: 0}
ONE_TILE = {0: 1, 1: 1, 5: 0, 2: -1}
PERSISTENT = {0: 1, 5: 0, 2: 0}
BIG = (11008, 1536, 128)      # 258 tiles of 256x256: more tiles than CUs, a last round of two

#            epilogue, bias, alpha, residual, aux ("out": the QuickGELU epilogue saves gelu'(u); "in": the backward multiplies by it)
KINDS = {"plain": (EPI_NONE, False, 1.0, False, None), "bias_alpha": (EPI_NONE, True, 0.5, False, None), "res": (EPI_NONE, True, 1.0, True, None),
         "gelu": (EPI_QUICKGELU, True, 1.0, False, None), "gelu_aux": (EPI_QUICKGELU, True, 1.0, False, "out"), "dgelu": (EPI_DQUICKGELU, False, 1.0, False, "in")}


def stream():
    return torch.cuda.current_stream().cuda_stream


def esz(td):
    return 4 if td == torch.float32 else 2


def gelu_grad_ref(u):
    sg = torch.sigmoid(1.702 * u)
    return sg * (1 + 1.702 * u * (1 - sg))


class tuning:
    """Tuning keys set inside the block, every one of them restored after it (also when the block raises)."""

    def __init__(self, keys):
        self.keys = dict(keys)

    def __enter__(self):
        lib = _lib.load()
        self.old = {k: lib.lpi_get_tuning(k) for k in self.keys}
        for k, v in self.keys.items():
            assert lib.lpi_set_tuning(k, v) == 0

    def __exit__(self, *exc):
        for k, v in self.old.items():
            assert _lib.load().lpi_set_tuning(k, v) == 0


@functools.lru_cache(maxsize=6)
def data(dt, M, N, K, seed=0):
    """Operands as stored (rounded to their types) on the CPU and the f64 product A.B^T of those: computed once per shape, shared by the cases, never written."""
    g = torch.Generator().manual_seed(1000 * seed + M + N + K)
    td = TD[dt]
    a = torch.randn(M, K, generator=g).to(td)
    b = (torch.randn(N, K, generator=g) * 0.05).to(td)
    d = dict(a=a, b=b, bias=torch.randn(N, generator=g), res32=torch.randn(M, N, generator=g), res16=(torch.randn(M, N, generator=g) * 4).half(),
             aux_in=(torch.rand(M, N, generator=g) * 2 - 1).to(AUX_TD[dt]), ab=a.double() @ b.double().t())      # a stand-in for gelu'(u), |aux| <= 1
    return d


def make_lds(ldset, N, K, tds):
    """-> {lda, ldb, ldc, ldr, ldaux, a0, b0, c0, r0, x0} in elements; tds = element types of (A / B, C, residual, aux)."""
    ta, tc, tr, tx = tds
    u = lambda td: 16 // esz(td)      # noqa: E731  elements per 16 bytes
    if ldset == "tier1":
        return dict(lda=K + 32, ldb=K + 64, ldc=N + 8, ldr=N + 16, ldaux=N + 24, a0=u(ta), b0=u(ta), c0=u(tc), r0=u(tr), x0=u(tx))
    if ldset == "min16":
        return dict(lda=K + u(ta), ldb=K + 2 * u(ta), ldc=N + u(tc), ldr=N + 3 * u(tr), ldaux=N + 2 * u(tx), a0=u(ta), b0=u(ta), c0=u(tc), r0=u(tr), x0=u(tx))
    assert ldset == "engine"
    return dict(lda=3 * K // 2, ldb=3 * K // 2, ldc=3 * N // 2, ldr=3 * N // 2, ldaux=3 * N // 2, a0=K // 2, b0=K // 2, c0=N // 2, r0=N // 2, x0=N // 2)


def build(dt, cdt, M, N, K, kind, L, d):
    """The operands of one arm as strided.Records; L = make_lds(...) for the strided arm, None for the tight one."""
    epi, use_bias, alpha, use_res, aux = KINDS[kind]
    ta, tc, tr, tx = TD[dt], TD[cdt], (torch.float16 if cdt == F16 else torch.float32), AUX_TD[dt]
    used = [(M, ta, "lda", "a0"), (N, ta, "ldb", "b0"), (M, tc, "ldc", "c0")] + ([(M, tr, "ldr", "r0")] if use_res else []) + ([(M, tx, "ldaux", "x0")] if aux else [])
    nbytes = 0 if L is None else S.arena_bytes(max(r for r, _, _, _ in used), max(L[k] for _, _, k, _ in used), max(esz(t) for _, t, _, _ in used),
                                               max(L[o] for _, _, _, o in used))

    def op(rows, cols, td, ld, off, fill):
        if L is None:
            return S.operand(rows, cols, cols, td, 0, rows * cols, fill, DEV)
        return S.operand(rows, cols, L[ld], td, L[off], nbytes // esz(td), fill, DEV)

    ops = dict(A=op(M, K, ta, "lda", "a0", d["a"]), B=op(N, K, ta, "ldb", "b0", d["b"]), C=op(M, N, tc, "ldc", "c0", None))
    if use_res:
        ops["R"] = op(M, N, tr, "ldr", "r0", d["res16"] if cdt == F16 else d["res32"])
    if aux:
        ops["X"] = op(M, N, tx, "ldaux", "x0", None if aux == "out" else d["aux_in"])
    return ops


def launch_nt(dt, cdt, M, N, K, kind, ops, bias):
    epi, use_bias, alpha, use_res, aux = KINDS[kind]
    r, x = ops.get("R"), ops.get("X")
    n0 = _lib.launch_count()
    call("lpi_gemm_nt", dt, cdt, M, N, K, ops["A"].t, ops["A"].t.stride(0), ops["B"].t, ops["B"].t.stride(0), ops["C"].t, ops["C"].t.stride(0),
         bias if use_bias else None, r.t if r else None, r.t.stride(0) if r else 0, epi, x.t if x else None, x.t.stride(0) if x else 0, alpha, stream())
    assert _lib.launch_count() == n0 + 1
    return int(_lib.load().lpi_gemm_last_kernel())


def outputs(ops):
    return [k for k, o in ops.items() if o.output]


def check_arms(label, strided_ops, tight_ops):
    """Pads, written outputs, and the strided arm's outputs bit for bit the tight arm's."""
    torch.cuda.synchronize()
    for ops in (strided_ops, tight_ops):
        for k, o in ops.items():
            S.check_pads(f"{label} {k}", o)
        for k in outputs(ops):
            S.check_written(f"{label} {k}", ops[k])
    assert outputs(strided_ops) == outputs(tight_ops) and outputs(tight_ops)
    for k in outputs(tight_ops):
        s, t = (o.arena[o.inside] for o in (strided_ops[k], tight_ops[k]))      # the footprints' values, row by row
        assert not bool(torch.isnan(t.float()).any()), f"{label} {k}: NaN in the tight arm"
        assert same_bits(s, t), f"{label} {k}: the strided arm differs from the tight arm in {int((S.bits(s) != S.bits(t)).sum())} of {t.numel()} values"


def bar(dt, cdt, name):
    """The bar of the kernel's existing test for output `name` ("C" or "X") of a (dt, cdt) GEMM."""
    if dt == F32:
        return TOL[F32]
    if dt == BF16:
        return 2e-3 if (cdt == F16 and name == "C") else TOL[BF16]      # test_gemm_256x128_tiles_for_half_empty_launches: the fp16 residual stream
    assert dt == F16      # test_gemm_f16_operands_all_epilogues
    return TOL[BF16] if name == "X" else (2e-3 if cdt == F16 else 1e-3)


def references(kind, cdt, d):
    """f64 references of the outputs of one kind, from the operands as stored."""
    epi, use_bias, alpha, use_res, aux = KINDS[kind]
    u = alpha * d["ab"] + (d["bias"].double() if use_bias else 0.0)
    if epi == EPI_QUICKGELU:
        out = {"C": u * torch.sigmoid(1.702 * u)}
        if aux:
            out["X"] = gelu_grad_ref(u)
        return out
    if epi == EPI_DQUICKGELU:
        return {"C": u * d["aux_in"].double()}
    return {"C": u + ((d["res16"] if cdt == F16 else d["res32"]).double() if use_res else 0.0)}


@functools.lru_cache(maxsize=4)
def x3_bar(M, N, K):
    """test_bf16x3_gpu.py's bar: (3 x 2^-16 + allowance) x (|A||B|^T), the accumulation allowance measured from the LPI_BF16 kernel on the bf16-rounded copies."""
    d = data(F32X3, M, N, K)
    ab, bb = d["a"].bfloat16(), d["b"].bfloat16()
    Kp = (K + 63) // 64 * 64
    pad = lambda t: torch.nn.functional.pad(t, (0, Kp - K)).contiguous().to(DEV)  # noqa: E731
    cb = torch.zeros(M, N, device=DEV)
    with tuning(DEFAULT_KEYS):
        call("lpi_gemm_nt", BF16, F32, M, N, Kp, pad(ab), Kp, pad(bb), Kp, cb, N, None, None, 0, EPI_NONE, None, 0, 1.0, stream())
    allowance = 2.0 * float(((cb.cpu().double() - ab.double() @ bb.double().t()).abs() / X3.abs_product(ab, bb)).max())
    return (3 * U16 + allowance) * X3.abs_product(d["a"], d["b"])


def nt_case(dt, cdt, shape, kind, ldset, kernel, keys):
    M, N, K = shape
    d = data(dt, M, N, K)
    bias = d["bias"].to(DEV)
    tds = (TD[dt], TD[cdt], torch.float16 if cdt == F16 else torch.float32, AUX_TD[dt])
    label = f"{dt}->{cdt} {shape} {kind} {ldset}"
    with tuning({**DEFAULT_KEYS, **keys}):
        st = build(dt, cdt, M, N, K, kind, make_lds(ldset, N, K, tds), d)
        ti = build(dt, cdt, M, N, K, kind, None, d)
        assert launch_nt(dt, cdt, M, N, K, kind, st, bias) == kernel, label
        assert launch_nt(dt, cdt, M, N, K, kind, ti, bias) == kernel, label
        check_arms(label, st, ti)
        if dt == F32X3:      # against the exact f32 kernel on the same operands, as test_bf16x3_gpu.py::test_epilogues_against_the_f32_kernel
            ex = build(F32, cdt, M, N, K, kind, None, d)
            assert launch_nt(F32, cdt, M, N, K, kind, ex, bias) in (GEMM_K_128, GEMM_K_256)
            torch.cuda.synchronize()
            for k in outputs(ti):
                diff = (ti[k].t.cpu().double() - ex[k].t.cpu().double()).abs()
                print(f"{label} {k}: worst |x3 - f32| / bar {float((diff / x3_bar(M, N, K)).max()):.3f}")
                assert float(diff.max()) > 0 and bool((diff <= x3_bar(M, N, K)).all()), (label, k)
            return
    for k, ref in references(kind, cdt, d).items():
        e = relerr(ti[k].t, ref)
        print(f"{label} {k}: error {e:.3e} (bar {bar(dt, cdt, k):g})")
        assert e < bar(dt, cdt, k), (label, k, e)


ALL_KINDS = ["plain", "bias_alpha", "res", "gelu", "gelu_aux", "dgelu"]
TYPES_KINDS = [(F32, F32, ALL_KINDS), (F32X3, F32, ALL_KINDS), (BF16, BF16, ALL_KINDS), (BF16, F32, ["bias_alpha", "res"]), (BF16, F16, ["res"]),
               (F16, F16, ["bias_alpha", "res", "gelu", "gelu_aux"]), (F16, F32, ["res"])]
NAME = {F32: "f32", F32X3: "x3", BF16: "bf16", F16: "f16"}


def nt_params(type_kinds, ldsets_extra):
    """tier1 for every (types, kind); the other ld sets for the kinds that use the most operands."""
    out = []
    for dt, cdt, kinds in type_kinds:
        for kind in kinds:
            out.append(pytest.param(dt, cdt, kind, "tier1", id=f"{NAME[dt]}-{NAME[cdt]}-{kind}-tier1"))
        for ldset in ldsets_extra:
            for kind in [k for k in ("plain", "res", "gelu_aux", "dgelu") if k in kinds]:
                out.append(pytest.param(dt, cdt, kind, ldset, id=f"{NAME[dt]}-{NAME[cdt]}-{kind}-{ldset}"))
    return out


@pytest.mark.parametrize("dt,cdt,kind,ldset", nt_params(TYPES_KINDS, ["min16", "engine"]))
def test_gemm128(dt, cdt, kind, ldset):
    """128x128 kernel: N is no multiple of 256."""
    four = dt in (F32, F32X3)
    nt_case(dt, cdt, (384, 128, 64 if four else 128), kind, ldset, GEMM_K_X3 if dt == F32X3 else GEMM_K_128, {})


@pytest.mark.parametrize("dt,cdt,kind,ldset", nt_params(TYPES_KINDS, ["engine"]))
def test_gemm256_one_tile_per_workgroup(dt, cdt, kind, ldset):
    nt_case(dt, cdt, (768, 512, 128), kind, ldset, GEMM_K_X3 if dt == F32X3 else GEMM_K_256, ONE_TILE)


PERSISTENT_TYPES = [(BF16, BF16, ["plain", "bias_alpha", "res", "gelu", "gelu_aux", "dgelu"]), (BF16, F16, ["res"]), (BF16, F32, ["plain", "res"]),
                    (F16, F16, ["plain", "bias_alpha", "res", "gelu_aux"]), (F16, F32, ["res"])]


@pytest.mark.parametrize("dt,cdt,kind,ldset", nt_params(PERSISTENT_TYPES, ["min16", "engine"]))
def test_gemm256_persistent(dt, cdt, kind, ldset):
    """Persistent 256x256 kernel, six tiles: "plain" = the half-width staging with its 16-byte row stores, an fp16 residual and the saved gelu' come to LDS as
    LDS-DMA side tiles (ldr / ldaux in the DMA's addresses), an f32 residual stays on the one-tile kernel."""
    nt_case(dt, cdt, (768, 512, 128), kind, ldset, GEMM_K_256, PERSISTENT)


@pytest.mark.parametrize("ldset", ["tier1", "min16", "engine"])
@pytest.mark.parametrize("dt", [BF16, F16], ids=["bf16", "f16"])
def test_gemm256_persistent_generic_store_only_epilogue(dt, ldset):
    """Key 14 = 1: the same store-only GEMM through the generic epilogue (8-byte stores) instead of the half-width staging."""
    nt_case(dt, dt, (768, 512, 128), "plain", ldset, GEMM_K_256, {**PERSISTENT, 14: 1})


@pytest.mark.parametrize("kind,cdt", [("plain", BF16), ("res", F16)])
def test_gemm256_persistent_more_tiles_than_cus(kind, cdt):
    """258 tiles on 256 CUs with the hybrid round off (key 6 = 0): workgroups walk on to a second tile, whose operands are re-addressed from the leading dimensions."""
    nt_case(BF16, cdt, BIG, kind, "tier1", GEMM_K_256, {**PERSISTENT, 6: 0})


@pytest.mark.parametrize("kind,cdt,ldset", [("bias_alpha", BF16, "tier1"), ("res", F16, "tier1"), ("bias_alpha", F32, "tier1"), ("gelu_aux", BF16, "tier1"), ("dgelu", BF16, "tier1"),
                                            ("res", F16, "engine"), ("gelu_aux", BF16, "min16")])
def test_gemm256x128(kind, cdt, ldset):
    """16 tiles of 256x256 under the default keys -> the 256x128 kernel; the epilogues of test_gemm_256x128_tiles_for_half_empty_launches."""
    nt_case(BF16, cdt, (4096, 256, 128), kind, ldset, GEMM_K_256X128, {})


@pytest.mark.parametrize("key2", [0, -1])
@pytest.mark.parametrize("kind,cdt,ldset", [("plain", BF16, "tier1"), ("res", F16, "tier1"), ("gelu_aux", BF16, "tier1"), ("dgelu", BF16, "tier1"), ("res", F16, "engine")])
def test_gemm_hybrid_tail_round(kind, cdt, ldset, key2):
    """258 tiles: the last two run as four 256x128 half tiles inside the launch, persistent (key 2 = 0) and one tile per workgroup (key 2 = -1)."""
    nt_case(BF16, cdt, BIG, kind, ldset, GEMM_K_256_TAIL, {0: 1, 5: 0, 2: key2, 6: 1})


# ---- LN-fold and row-statistics epilogues (persistent kernel only) ---------------------------------------------------------------------------------------------

def ln_block(M, N, ldr, mean, rstd, c1, nbytes):
    """The LN operand block mean[ldr] | rstd[ldr] | c1[N] as a strided.Record (4 floats into its arena); entries M..ldr-1 are pads.  nbytes 0: tight (ldr = M)."""
    idx = torch.cat([torch.arange(M), ldr + torch.arange(M), 2 * ldr + torch.arange(N)]) + (4 if nbytes else 0)
    fill = None if mean is None else torch.cat([mean, rstd, c1]).float()
    return S.region(idx, torch.float32, nbytes // 4 if nbytes else 2 * M + N, fill, DEV)


def ln_data(dt, M, N, K, seed):
    """The recipe of test_kernels_gpu.py::_ln_fold_operands (rows with a mean and a large channel) at a small shape; the reference from the operands as stored."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(M, K, generator=g) + 0.7 * torch.randn(M, 1, generator=g)
    x[:, 3] *= 20.0
    x = x.to(TD[dt])
    w = torch.randn(N, K, generator=g) * 0.05
    b, gamma, beta = torch.randn(N, generator=g), 1.0 + 0.3 * torch.randn(K, generator=g), 0.2 * torch.randn(K, generator=g)
    wl = (w.double() * gamma.double()[None, :]).to(TD[dt])
    return x, wl, (w.double() @ beta.double() + b.double()).float()


def ln_reference(x, wl, c2):
    xd = x.double()
    mu, var = xd.mean(1, keepdim=True), xd.var(1, unbiased=False, keepdim=True)
    rstd = 1.0 / torch.sqrt(var + 1e-5)
    c1 = wl.double().sum(1).float()
    ref = rstd * (xd @ wl.double().t() - mu * c1.double()[None, :]) + c2.double()
    return mu[:, 0].float(), rstd[:, 0].float(), c1, ref


@pytest.mark.parametrize("ldset", ["tier1", "engine"])
@pytest.mark.parametrize("epi,aux", [(EPI_LN, False), (EPI_LN_QUICKGELU, False), (EPI_LN_QUICKGELU, True)], ids=["ln", "ln_gelu", "ln_gelu_aux"])
@pytest.mark.parametrize("dt", [BF16, F16], ids=["bf16", "f16"])
def test_gemm_layernorm_fold(dt, epi, aux, ldset):
    """LPI_EPI_LN / LPI_EPI_LN_QUICKGELU, bf16 output: ldr = M + 4 strides the LN block's vectors (the entries between M and ldr hold NaN), on top of padded
    lda / ldb / ldc / ldaux.  Bars of test_gemm_layernorm_fold_epilogues: 6e-3 for the bf16 output and for the saved gelu'."""
    M, N, K = 768, 512, 128
    x, wl, c2 = ln_data(dt, M, N, K, seed=7)
    mean, rstd, c1, ref = ln_reference(x, wl, c2)
    bias = c2.to(DEV)
    L = make_lds(ldset, N, K, (TD[dt], torch.bfloat16, torch.float32, torch.bfloat16))
    ldr = M + 4
    nbytes = S.arena_bytes(max(M, N), max(L["lda"], L["ldb"], L["ldc"], L["ldaux"], ldr), 4, max(L["a0"], L["c0"], L["x0"], 4))
    assert nbytes >= (4 + 2 * ldr + N) * 4
    arms = []
    with tuning({**DEFAULT_KEYS, **PERSISTENT}):
        for strided in (True, False):
            if strided:
                ops = dict(A=S.operand(M, K, L["lda"], TD[dt], L["a0"], nbytes // 2, x, DEV), B=S.operand(N, K, L["ldb"], TD[dt], L["b0"], nbytes // 2, wl, DEV),
                           C=S.operand(M, N, L["ldc"], torch.bfloat16, L["c0"], nbytes // 2, None, DEV), R=ln_block(M, N, ldr, mean, rstd, c1, nbytes))
                if aux:
                    ops["X"] = S.operand(M, N, L["ldaux"], torch.bfloat16, L["x0"], nbytes // 2, None, DEV)
            else:
                ops = dict(A=S.operand(M, K, K, TD[dt], 0, M * K, x, DEV), B=S.operand(N, K, K, TD[dt], 0, N * K, wl, DEV),
                           C=S.operand(M, N, N, torch.bfloat16, 0, M * N, None, DEV), R=ln_block(M, N, M, mean, rstd, c1, 0))
                if aux:
                    ops["X"] = S.operand(M, N, N, torch.bfloat16, 0, M * N, None, DEV)
            X = ops.get("X")
            n0 = _lib.launch_count()
            call("lpi_gemm_nt", dt, BF16, M, N, K, ops["A"].t, ops["A"].t.stride(0), ops["B"].t, ops["B"].t.stride(0), ops["C"].t, ops["C"].t.stride(0), bias,
                 ops["R"].t[4:] if strided else ops["R"].t, ldr if strided else M, epi, X.t if X else None, X.t.stride(0) if X else 0, 1.0, stream())
            assert _lib.launch_count() == n0 + 1 and _lib.load().lpi_gemm_last_kernel() == GEMM_K_256
            arms.append(ops)
    check_arms(f"LN {dt} {epi} {ldset}", *arms)
    ti = arms[1]
    want = ref if epi == EPI_LN else ref * torch.sigmoid(1.702 * ref)
    e = relerr(ti["C"].t, want)
    print(f"LN fold dt {dt} epi {epi}: error {e:.3e} (bar 6e-3)")
    assert e < 6e-3
    if aux:
        assert relerr(ti["X"].t, gelu_grad_ref(ref)) < 6e-3


def slot_stats(c):
    """f64 slot sums of the stored values, laid out as the LPI_EPI_RES_ROWSTATS aux buffer (test_kernels_gpu.py::_slot_stats)."""
    x = c.double().cpu()
    M, N = x.shape
    xs = x.view(M, N // 128, 128)
    return torch.stack([xs.sum(-1).t(), (xs * xs).sum(-1).t()], 1).reshape(2 * (N // 128), M)


@pytest.mark.parametrize("dt", [BF16, F16], ids=["bf16", "f16"])
def test_gemm_row_statistics_chained_into_the_layernorm_fold(dt):
    """LPI_EPI_RES_ROWSTATS (768, 256, 128) with ldaux = M + 8 on the slot buffer, lpi_ln_stats_finalize into an LN block of ldr = M + 4, then LPI_EPI_LN
    (768, 512, 256) whose A operand is the first GEMM's strided fp16 output: both GEMMs bit for bit their contiguous arms, the slot sums within 2e-6 of the f64 sums
    of the stored values (test_gemm_residual_epilogue_with_row_statistics), the chain within 6e-3 of LayerNorm(x) W^T + b of the stored x."""
    M, N1, K1, N2 = 768, 256, 128, 512
    td = TD[dt]
    d = data(dt, M, N1, K1, seed=3)
    g = torch.Generator().manual_seed(17)
    w2 = (torch.randn(N2, N1, generator=g) * 0.05).half()      # the LN GEMM's operands are fp16 (the stream's type)
    bias1, bias2 = d["bias"].to(DEV), torch.randn(N2, generator=g).to(DEV)
    c1 = w2.double().sum(1).float()
    res = (d["res16"] * 0.75 + 0.7).half()      # rows with a mean
    ldr, ldaux, slots = M + 4, M + 8, 2 * (N1 // 128)
    L1 = make_lds("tier1", N1, K1, (td, torch.float16, torch.float16, torch.float32))
    L2 = make_lds("tier1", N2, N1, (torch.float16, torch.bfloat16, torch.float32, torch.bfloat16))
    nbytes = S.arena_bytes(max(M, N1, N2), max(L1["lda"], L1["ldb"], L1["ldc"], L1["ldr"], L2["ldb"], L2["ldc"], ldr, ldaux), 4, 8)
    arms = []
    with tuning({**DEFAULT_KEYS, **PERSISTENT}):
        for strided in (True, False):
            def op(rows, cols, tdx, ld, off, fill):
                return S.operand(rows, cols, ld, tdx, off, nbytes // esz(tdx), fill, DEV) if strided else S.operand(rows, cols, cols, tdx, 0, rows * cols, fill, DEV)
            ops = dict(A=op(M, K1, td, L1["lda"], L1["a0"], d["a"]), B=op(N1, K1, td, L1["ldb"], L1["b0"], d["b"]), C=op(M, N1, torch.float16, L1["ldc"], L1["c0"], None),
                       R=op(M, N1, torch.float16, L1["ldr"], L1["r0"], res), SLOTS=op(slots, M, torch.float32, ldaux, 4, None),
                       B2=op(N2, N1, torch.float16, L2["ldb"], L2["b0"], w2), C2=op(M, N2, torch.bfloat16, L2["ldc"], L2["c0"], None))
            ld_blk = ldr if strided else M
            blk = ln_block(M, N2, ld_blk, None, None, None, nbytes if strided else 0)      # an output of lpi_ln_stats_finalize, c1 filled in below
            off = 4 if strided else 0
            blk.t[off + 2 * ld_blk:off + 2 * ld_blk + N2] = c1.to(DEV)
            call("lpi_gemm_nt", dt, F16, M, N1, K1, ops["A"].t, ops["A"].t.stride(0), ops["B"].t, ops["B"].t.stride(0), ops["C"].t, ops["C"].t.stride(0), bias1,
                 ops["R"].t, ops["R"].t.stride(0), EPI_RES_ROWSTATS, ops["SLOTS"].t, ops["SLOTS"].t.stride(0), 1.0, stream())
            assert _lib.load().lpi_gemm_last_kernel() == GEMM_K_256
            call("lpi_ln_stats_finalize", M, N1, ops["SLOTS"].t, ops["SLOTS"].t.stride(0), 1e-5, blk.t[off:], blk.t[off + ld_blk:], stream())
            call("lpi_gemm_nt", F16, BF16, M, N2, N1, ops["C"].t, ops["C"].t.stride(0), ops["B2"].t, ops["B2"].t.stride(0), ops["C2"].t, ops["C2"].t.stride(0), bias2,
                 blk.t[off:], ld_blk, EPI_LN, None, 0, 1.0, stream())
            assert _lib.load().lpi_gemm_last_kernel() == GEMM_K_256
            ops["BLK"] = blk
            arms.append(ops)
    check_arms(f"ROWSTATS -> LN {dt}", *arms)
    ti = arms[1]
    x = ti["C"].t.cpu()
    assert relerr(x, d["ab"] + d["bias"].double() + res.double()) < 2e-3
    want = slot_stats(x)
    assert float((ti["SLOTS"].t.double().cpu() - want).abs().max()) <= 2e-6 * float(want.abs().max())
    _, _, _, ref = ln_reference(x, w2, bias2.cpu())
    e = relerr(ti["C2"].t, ref)
    print(f"ROWSTATS -> LN dt {dt}: error {e:.3e} (bar 6e-3)")
    assert e < 6e-3


# ---- grouped launches ------------------------------------------------------------------------------------------------------------------------------------------------

GROUP = ((16384, 1024, 128), (4096, 512, 128))      # 256 + 32 tiles: the smallest pair that lpi_gemm_nt_grouped groups (a round of tiles, two K-tiles)


@pytest.mark.parametrize("kind,cdt,ldset", [("plain", BF16, "tier1"), ("res", F16, "tier1"), ("gelu_aux", BF16, "tier1"), ("dgelu", BF16, "tier1"), ("res", F16, "engine")])
def test_gemm_grouped(kind, cdt, ldset):
    """Two problems in one persistent launch, all ten leading dimensions distinct (tier1; "engine": both problems as column blocks of 1.5 x wider buffers);
    the fallback (key 8 = 1: two launches) gives the same bits."""
    epi, use_bias, alpha, use_res, aux = KINDS[kind]
    tds = (torch.bfloat16, TD[cdt], torch.float16 if cdt == F16 else torch.float32, torch.bfloat16)
    ds = [data(BF16, *s) for s in GROUP]
    Ls = [make_lds(ldset, s[1], s[2], tds) for s in GROUP]
    lds10 = [L[k] for L in Ls for k in ("lda", "ldb", "ldc", "ldr", "ldaux")]
    if ldset == "tier1":
        Ls[1] = {k: (v + 40 if k.startswith("ld") else v) for k, v in Ls[1].items()}      # 40 elements = 80 bytes more than anything of problem 0
        lds10 = [L[k] for L in Ls for k in ("lda", "ldb", "ldc", "ldr", "ldaux")]
        assert len(set(lds10)) == 10, lds10
    # one arena size for BOTH problems' operands: the larger problem's rows against the largest leading dimension of either
    nbytes = S.arena_bytes(max(s[0] for s in GROUP), max(lds10), max(esz(t) for t in tds), max(v for L in Ls for k, v in L.items() if not k.startswith("ld")))

    def arm(strided, key8):
        probs, recs = [], []
        for (M, N, K), d, L in zip(GROUP, ds, Ls):
            def op(rows, cols, tdx, ld, off, fill):
                return S.operand(rows, cols, L[ld], tdx, L[off], nbytes // esz(tdx), fill, DEV) if strided else S.operand(rows, cols, cols, tdx, 0, rows * cols, fill, DEV)
            ops = dict(A=op(M, K, tds[0], "lda", "a0", d["a"]), B=op(N, K, tds[0], "ldb", "b0", d["b"]), C=op(M, N, tds[1], "ldc", "c0", None))
            if use_res:
                ops["R"] = op(M, N, tds[2], "ldr", "r0", d["res16"] if cdt == F16 else d["res32"])
            if aux:
                ops["X"] = op(M, N, tds[3], "ldaux", "x0", None if aux == "out" else d["aux_in"])
            recs.append(ops)
            probs.append(dict(M=M, N=N, K=K, a=ops["A"].t, b=ops["B"].t, c=ops["C"].t, bias=d["bias"].to(DEV) if use_bias else None,
                              residual=ops["R"].t if use_res else None, aux=ops["X"].t if aux else None))
        n0 = _lib.launch_count()
        with tuning({**DEFAULT_KEYS, 8: key8}):
            grouped = _lib.gemm_grouped(BF16, cdt, epi, alpha, probs, stream())
        assert grouped == (key8 == 0) and _lib.launch_count() - n0 == (1 if grouped else 2)
        # grouped: the persistent kernel (288 tiles: with a hybrid last round where the chip has 256 CUs); the fallback's last launch is the second problem
        # alone, 32 tiles of 256x256 -> the 256x128 kernel
        assert _lib.load().lpi_gemm_last_kernel() in ((GEMM_K_256, GEMM_K_256_TAIL) if grouped else (GEMM_K_256X128,))
        return recs
    st, ti, fb = arm(True, 0), arm(False, 0), arm(True, 1)
    for i in range(2):
        check_arms(f"grouped {kind} problem {i}", st[i], ti[i])
        check_arms(f"grouped {kind} problem {i}, fallback", fb[i], ti[i])
        for k, ref in references(kind, cdt, ds[i]).items():
            assert relerr(ti[i][k].t, ref) < bar(BF16, cdt, k), (kind, i, k)


# ---- the few-row 32x32 kernel -------------------------------------------------------------------------------------------------------------------------------------

ROWS_SHAPES = {F32: ((32, 32, 32), (96, 160, 224)), BF16: ((32, 32, 64), (96, 160, 448)), F16: ((32, 32, 64), (96, 160, 448))}


def rows_lds(ldset, N, K, tds, bump):
    """tier1 / min16 as make_lds; "min8": the four-element row steps lpi_gemm_nt_rows takes for C / residual / aux (8 bytes for a 2-byte type).  bump: the
    second problem of a pair gets other leading dimensions than the first."""
    if ldset == "min8":
        L = dict(lda=K + 16 // esz(tds[0]), ldb=K + 32 // esz(tds[0]), ldc=N + 4, ldr=N + 12, ldaux=N + 8, a0=16 // esz(tds[0]), b0=16 // esz(tds[0]), c0=16 // esz(tds[1]),
                 r0=16 // esz(tds[2]), x0=16 // esz(tds[3]))
    else:
        L = make_lds(ldset, N, K, tds)
    return {k: (v + bump if k.startswith("ld") else v) for k, v in L.items()}


def rows_params():
    out = []
    for dt in (F32, BF16, F16):
        for count in (1, 2):
            for kind, c32 in (("res", True), ("gelu_aux", False), ("dgelu", False)) + ((("res", False),) if dt == F16 else ()):
                for ldset in ("tier1",) + (("min8",) if (dt != F32 and not c32) else ("min16",)) + (("engine",) if count == 2 else ()):
                    out.append(pytest.param(dt, count, kind, c32, ldset, id=f"{NAME[dt]}-{count}-{kind}-{'f32out' if c32 else 'out'}-{ldset}"))
    return out


@pytest.mark.parametrize("dt,count,kind,c32,ldset", rows_params())
def test_gemm_rows(dt, count, kind, c32, ldset):
    """lpi_gemm_nt_rows, one problem and a pair whose two problems have different leading dimensions: NONE + residual (f32 into an f32 C; fp16 into an fp16 C),
    QUICKGELU + aux, DQUICKGELU.  "min8": ldc / ldr / ldaux = N + 4 / 12 / 8 elements of a 2-byte type — the kernel moves four elements per lane."""
    epi, use_bias, alpha, use_res, aux = KINDS[kind]
    cdt = F32 if c32 else dt
    tds = (TD[dt], TD[cdt], torch.float16 if cdt == F16 else torch.float32, AUX_TD[dt])
    shapes = ROWS_SHAPES[dt] if count == 2 else (ROWS_SHAPES[dt][1],)
    if count == 1 and ldset == "tier1":
        shapes = (ROWS_SHAPES[dt][0],)
    ds = [data(dt, *s) for s in shapes]
    Ls = [rows_lds(ldset, s[1], s[2], tds, 32 * i) for i, s in enumerate(shapes)]
    nbytes = S.arena_bytes(max(max(s[0], s[1]) for s in shapes), max(v for L in Ls for k, v in L.items() if k.startswith("ld")), max(esz(t) for t in tds),
                           max(v for L in Ls for k, v in L.items() if not k.startswith("ld")))
    arms = []
    for strided in (True, False):
        probs, recs = [], []
        for (M, N, K), d, L in zip(shapes, ds, Ls):
            def op(rows, cols, tdx, ld, off, fill):
                return S.operand(rows, cols, L[ld], tdx, L[off], nbytes // esz(tdx), fill, DEV) if strided else S.operand(rows, cols, cols, tdx, 0, rows * cols, fill, DEV)
            ops = dict(A=op(M, K, tds[0], "lda", "a0", d["a"]), B=op(N, K, tds[0], "ldb", "b0", d["b"]), C=op(M, N, tds[1], "ldc", "c0", None))
            if use_res:
                ops["R"] = op(M, N, tds[2], "ldr", "r0", d["res16"] if cdt == F16 else d["res32"])
            if aux:
                ops["X"] = op(M, N, tds[3], "ldaux", "x0", None if aux == "out" else d["aux_in"])
            recs.append(ops)
            probs.append(dict(M=M, N=N, K=K, a=ops["A"].t, b=ops["B"].t, c=ops["C"].t, bias=d["bias"].to(DEV) if use_bias else None,
                              residual=ops["R"].t if use_res else None, aux=ops["X"].t if aux else None))
        n0 = _lib.launch_count()
        _lib.gemm_rows(dt, cdt, epi, alpha, probs, stream())
        assert _lib.launch_count() == n0 + 1 and _lib.load().lpi_gemm_last_kernel() == GEMM_K_ROWS
        arms.append(recs)
    tol = TOL[BF16] if dt == F16 else TOL[dt]      # test_gemm_rows_all_epilogues
    for i in range(len(shapes)):
        check_arms(f"rows {dt} {kind} problem {i}", arms[0][i], arms[1][i])
        for k, ref in references(kind, cdt, ds[i]).items():
            assert relerr(arms[1][i][k].t, ref) < tol, (kind, i, k)


# ---- what the argument checks refuse -------------------------------------------------------------------------------------------------------------------------------

def test_row_ends_that_are_not_16_bytes_are_refused_before_any_launch():
    """lpi_gemm_nt / lpi_gemm_nt_grouped: ldc, ldr, ldaux that are multiples of 8 but not of 16 bytes, and an aux pointer that is: LPI_EINVAL, nothing launched
    (the persistent kernel's 16-byte row stores and LDS-DMA side-tile loads, and the f32x4 accesses of an f32 C / aux, need them: DESIGN.md section 4).
    lpi_gemm_nt_rows: the same for its f32 C and f32 aux; a 2-byte C at N + 4 runs (test_gemm_rows, min8)."""
    lib = _lib.load()
    M, N, K = 768, 512, 128
    z = lambda n, td: torch.zeros(n, device=DEV, dtype=td)  # noqa: E731
    big = (M + 1) * (N + 64)
    a16, b16, c16, x16, r16 = z(M * K, torch.bfloat16), z(N * K, torch.bfloat16), z(big, torch.bfloat16), z(big, torch.bfloat16), z(big, torch.float16)
    a32, c32, x32 = z(M * K, torch.float32), z(big, torch.float32), z(big, torch.float32)
    p = lambda t: None if t is None else t.data_ptr()  # noqa: E731
    st = stream()

    def nt(dt, cdt, A, B, C, ldc, res=None, ldr=0, epi=EPI_NONE, aux=None, ldaux=0, aux_off=0):
        return lib.lpi_gemm_nt(dt, cdt, M, N, K, p(A), K, p(B), K, p(C), ldc, None, p(res), ldr, epi, (p(aux) + aux_off) if aux is not None else None, ldaux, 1.0, st)

    n0 = _lib.launch_count()
    for keys in ({}, ONE_TILE, PERSISTENT):      # the refusal does not depend on the kernel the dispatcher would choose
        with tuning({**DEFAULT_KEYS, **keys}):
            assert nt(BF16, BF16, a16, b16, c16, N + 4) == -22                                         # a bf16 C row that ends on 8 bytes
            assert nt(BF16, F16, a16, b16, r16, N, res=r16, ldr=N + 4) == -22                          # the fp16 residual
            assert nt(BF16, BF16, a16, b16, c16, N, epi=EPI_DQUICKGELU, aux=x16, ldaux=N + 4) == -22   # the saved gelu'
            assert nt(BF16, BF16, a16, b16, c16, N, epi=EPI_QUICKGELU, aux=x16, ldaux=N, aux_off=8) == -22
            assert nt(BF16, F32, a16, b16, c32, N + 2) == -22                                          # an f32 C row that ends on 8 bytes
            assert nt(F32, F32, a32, a32, c32, N, epi=EPI_QUICKGELU, aux=x32, ldaux=N + 2) == -22
    assert _lib.launch_count() == n0
    view = lambda t, ld: t[:M * ld].view(M, ld)[:, :N]  # noqa: E731
    with pytest.raises(_lib.LpiError):
        _lib.gemm_grouped(BF16, BF16, EPI_NONE, 1.0, [dict(M=M, N=N, K=K, a=a16.view(M, K), b=b16.view(N, K), c=view(c16, N + 4))] * 2, st)
    with pytest.raises(_lib.LpiError):      # few-row kernel: an f32 C needs whole f32x4 rows
        _lib.gemm_rows(BF16, F32, EPI_NONE, 1.0, [dict(M=M, N=N, K=K, a=a16.view(M, K), b=b16.view(N, K), c=view(c32, N + 2))], st)
    with pytest.raises(_lib.LpiError):
        _lib.gemm_rows(F32, F32, EPI_QUICKGELU, 1.0, [dict(M=M, N=N, K=K, a=a32.view(M, K), b=a32.view(M, K)[:N], c=view(c32, N), aux=view(x32, N + 2))], st)
    assert _lib.launch_count() == n0
    assert nt(BF16, BF16, a16, b16, c16, N + 8) == 0 and _lib.launch_count() == n0 + 1      # 16-byte row ends: accepted
