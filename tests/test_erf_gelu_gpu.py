"""erf-GELU on the GPU: lpi_gelu_erf_fwd (csrc/act.hip) against f64, its write bounds and refusals, and EngineOptions.erf_gelu through the engine — f32 against
the oracle with nn.GELU patched in (the test that cannot pass on a QuickGELU engine: tests/test_erf_gelu_host.py holds the premise), the 2-byte modes against
that f32 engine and against their own unfolded arm, the train=False forwards, and the option off (the parent's launch count, reproducible bits).

Bars.  2-byte outputs: one unit in the last place of the output type at |ref|, the smallest subnormal as the floor — the f32 evaluation error is below a
hundredth of such a unit (host test), so only a value next to a rounding boundary may land on the neighbouring number.  f32 outputs: 4 times the error of the
float32 CPU restatement of the same formulas (gelu_ref.restatement_error: 165 units of 2^-24 |ref| for gelu, 306 for gelu'), measured on the same inputs.
Measured on the MI355X ("erf-GELU"): f32 167 units for gelu and 245 for gelu' (bars 660 / 1224); 2-byte outputs 0.50 units."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import gelu_ref  # noqa: E402
import strided  # noqa: E402
from poison import same_bits  # noqa: E402
from lpi_amd import _lib, synth  # noqa: E402
from lpi_amd import engine as E  # noqa: E402
from lpi_amd.engine import DualEncoder, EngineOptions  # noqa: E402
from lpi_amd.step import train_step  # noqa: E402
from test_model_gpu import GRADS, check, maxerr, run_hip  # noqa: E402

DEV = "cuda:0"
CODE = {torch.float32: _lib.F32, torch.bfloat16: _lib.BF16, torch.float16: _lib.F16}
AUX = {torch.float32: torch.float32, torch.bfloat16: torch.bfloat16, torch.float16: torch.bfloat16}      # AuxT of csrc/gemm_epilogue.h
ROWS, COLS = (1, 5, 130), (8, 136, 512)
EINVAL = -22

_KERNEL_REF = {}


def kernel_case(dtype):
    """The input vector of a type (specials first, so that the smallest shape holds them; then the grid and the samples in a fixed shuffled order) and its f64
    reference, computed once and shared."""
    if dtype not in _KERNEL_REF:
        u = gelu_ref.kernel_inputs(dtype)
        n_special = 6 if dtype == torch.float32 else 4
        rest = u[:-n_special][torch.randperm(u.numel() - n_special, generator=torch.Generator().manual_seed(1))]
        u = torch.cat([u[-n_special:], rest])
        _KERNEL_REF[dtype] = (u,) + gelu_ref.gelu_f64(u)
    return _KERNEL_REF[dtype]


def fill_for(dtype, rows, cols, shift=0):
    """[rows, cols] inputs: the input vector cycled (the 130 x 512 shape holds all of it several times), and the matching f64 references."""
    u, rg, rdg = kernel_case(dtype)
    idx = (torch.arange(rows * cols) + shift) % u.numel()
    return u[idx].view(rows, cols), rg[idx].view(rows, cols), rdg[idx].view(rows, cols)


def run_kernel(dtype, rows, cols, ld, with_aux, col0=0, shift=0):
    """One call on strided views in arenas of one size (strided.py's safety rule); returns (g record, aux record or None, references)."""
    vals, rg, rdg = fill_for(dtype, rows, cols, shift)
    nbytes = strided.arena_bytes(max(ROWS), max(COLS) + 8, 4, 8)      # ONE byte size for every arena of every case: the largest shape in the widest type
    esz = lambda t: torch.empty(0, dtype=t).element_size()  # noqa: E731
    g = strided.in_out(strided.operand(rows, cols, ld, dtype, col0, nbytes // esz(dtype), fill=vals, device=DEV))
    aux = strided.operand(rows, cols, ld, AUX[dtype], col0, nbytes // esz(AUX[dtype]), device=DEV) if with_aux else None
    n0 = _lib.launch_count()
    _lib.call("lpi_gelu_erf_fwd", CODE[dtype], CODE[AUX[dtype]], rows, cols, g.t, ld, aux.t if with_aux else None, ld if with_aux else 0,
              torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert _lib.launch_count() == n0 + 1
    strided.check_pads("g", g)
    if with_aux:
        strided.check_pads("aux", aux)
        strided.check_written("aux", aux)
    return g, aux, rg, rdg


def hold(name, got, ref, dtype, f32_bar, worst):
    got, ref = got.detach().cpu(), ref
    assert bool(torch.isfinite(got).all()), name
    if dtype == torch.float32:
        e = gelu_ref.err_units(got, ref)
        worst[name] = max(worst.get(name, 0.0), e)
        assert e <= f32_bar, (name, e, f32_bar)
    else:
        e = float(((got.double() - ref).abs() / gelu_ref.ulp(ref, dtype)).max())
        worst[name] = max(worst.get(name, 0.0), e)
        assert e <= 1.0, (name, e)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16], ids=["f32", "bf16", "f16"])
def test_kernel_against_f64(dtype):
    """(a) every shape x leading dimension, with aux and without: values against f64 at the bars of the module docstring, the g bits the same either way."""
    eg, edg = gelu_ref.restatement_error(torch.float32)
    worst = {}
    for rows in ROWS:
        for cols in COLS:
            for ld in (cols, cols + 8):
                g1, aux, rg, rdg = run_kernel(dtype, rows, cols, ld, True)
                g0, _, _, _ = run_kernel(dtype, rows, cols, ld, False)
                assert same_bits(g1.t, g0.t), (rows, cols, ld)
                hold("gelu", g1.t, rg, dtype, gelu_ref.F32_BAR_FACTOR * eg, worst)
                hold("gelu'", aux.t, rdg, AUX[dtype], gelu_ref.F32_BAR_FACTOR * edg, worst)
    print(f"lpi_gelu_erf_fwd {dtype}: largest error {worst} ({'units of 2^-24 |ref|; the host restatement has %.1f / %.1f' % (eg, edg) if dtype == torch.float32 else 'units in the last place of the output type'})")


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16], ids=["f32", "bf16", "f16"])
def test_kernel_write_bounds(dtype):
    """(b) views that start 8 elements into their allocations, with ld = cols + 8: the ld gaps and everything before and behind both footprints keep their bits
    (strided.check_pads inside run_kernel), every aux element is written, and the values are those of the contiguous call."""
    for rows, cols in ((5, 136), (130, 8), (130, 512)):
        g, aux, _, _ = run_kernel(dtype, rows, cols, cols + 8, True, col0=8, shift=3)
        gc, auxc, _, _ = run_kernel(dtype, rows, cols, cols, True, shift=3)
        assert same_bits(g.t, gc.t) and same_bits(aux.t, auxc.t)
        g0, _, _, _ = run_kernel(dtype, rows, cols, cols + 8, False, col0=8, shift=3)
        assert same_bits(g0.t, gc.t)


def test_kernel_refusals():
    """(c) LPI_EINVAL before any launch."""
    lib = _lib.load()
    F32, BF16, F16 = _lib.F32, _lib.BF16, _lib.F16
    buf, abuf = torch.zeros(8 * 64 + 16, device=DEV), torch.zeros(8 * 64 + 16, device=DEV)
    g, a = buf.data_ptr(), abuf.data_ptr()
    assert g % 16 == 0 and a % 16 == 0
    s = torch.cuda.current_stream().cuda_stream
    n0 = _lib.launch_count()
    bad = {"cols = 12": (F32, F32, 4, 12, g, 16, a, 16), "ldg < cols": (F32, F32, 4, 16, g, 8, a, 16), "ldaux < cols": (F32, F32, 4, 16, g, 16, a, 8),
           "ldg not a multiple of 8": (F32, F32, 4, 16, g, 20, a, 24), "ldaux not a multiple of 8": (F32, F32, 4, 16, g, 24, a, 20),
           "g offset by 2 bytes": (BF16, BF16, 4, 16, g + 2, 16, a, 16), "aux offset by 2 bytes": (BF16, BF16, 4, 16, g, 16, a + 2, 16),
           "rows = 0": (F32, F32, 0, 16, g, 16, a, 16), "g NULL": (F32, F32, 4, 16, None, 16, a, 16)}
    for d in (F32, BF16, F16):
        for x in (F32, BF16, F16):
            if (d, x) not in ((F32, F32), (BF16, BF16), (F16, BF16)):
                bad[f"type pair ({d}, {x})"] = (d, x, 4, 16, g, 16, a, 16)
                bad[f"type pair ({d}, {x}) without aux"] = (d, x, 4, 16, g, 16, None, 0)
    for name, args in bad.items():
        assert lib.lpi_gelu_erf_fwd(*args, s) == EINVAL, name
    torch.cuda.synchronize()
    assert _lib.launch_count() == n0
    assert not bool(buf.any()) and not bool(abuf.any())
    assert lib.lpi_gelu_erf_fwd(F32, F32, 4, 16, g, 16, a, 16, s) == 0 and _lib.launch_count() == n0 + 1      # the legal neighbour of every case above
    torch.cuda.synchronize()


# ------------------------------------------------------------------ engine
_ERF_REF = {}


def erf_ref(monkeypatch, depth):
    """The f64 oracle with nn.GELU on TINY, 4 pairs: computed once per depth, under the patch."""
    O = gelu_ref.erf_oracle(monkeypatch)
    if depth not in _ERF_REF:
        cfg = synth.TINY
        fac = synth.prompt_factors(9, 16, cfg.vision_width, cfg.transformer_width)
        _ERF_REF[depth] = O.train_step(O.Oracle(cfg, synth.clip_state_dict(cfg), torch.float64), synth.images(4, cfg.image_resolution), synth.token_ids(4), fac, depth=depth)
    return _ERF_REF[depth]


_F32_ARM = {}


def f32_arm(depth, ids):
    """The f32 engine with erf_gelu=True on TINY, 4 pairs: the 2-byte modes' reference, run once per depth."""
    if depth not in _F32_ARM:
        _F32_ARM[depth] = run_hip(synth.TINY, "f32", 4, ids, depth, erf_gelu=True)[0]
    return _F32_ARM[depth]


@pytest.mark.parametrize("pooled_last", [True, False], ids=["pooled_last", "full_last"])
@pytest.mark.parametrize("depth", [1, 2])
def test_f32_engine_vs_oracle_with_nn_gelu(monkeypatch, depth, pooled_last):
    """(d) the bars of test_model_gpu.py::test_tiny_f32_vs_golden_and_oracle against the f64 oracle, which a QuickGELU engine misses by 16x .. 590x
    (tests/test_erf_gelu_host.py).  pooled_last=True runs the `cfc` site of the last block, False the `fc` site in every block."""
    ref = erf_ref(monkeypatch, depth)
    n0 = _lib.launch_count()
    res, _ = run_hip(synth.TINY, "f32", 4, synth.token_ids(4), depth, erf_gelu=True, pooled_last=pooled_last)
    print("erf_gelu f32 vs the f64 oracle:", {k: f"{maxerr(res[k], ref[k]):.2e}" for k in ("img_f", "txt_f", "logits")}, "launches", _lib.launch_count() - n0)
    check(res, ref, tol=2e-5, gtol=2e-4)


def test_bf16_mode_vs_the_f32_engine(golden):
    """(e) arm 1, bf16: the config and bars of test_model_gpu.py::test_tiny_bf16_close_to_oracle, erf_gelu=True in both arms."""
    ids = golden("tiny_d1")["token_ids"]
    ref = f32_arm(1, ids)
    res, _ = run_hip(synth.TINY, "bf16", 4, ids, 1, erf_gelu=True)
    print("erf_gelu bf16 vs f32:", {k: f"{maxerr(res[k], ref[k]):.2e}" for k in ("img_f", "txt_f", "logits")})
    for k in ("img_f", "txt_f"):
        assert maxerr(res[k], ref[k]) < 2e-2, (k, maxerr(res[k], ref[k]))
    assert maxerr(res["logits"], ref["logits"]) < 0.25
    for k in GRADS:
        assert maxerr(res[k], ref[k]) <= 0.08 * np.abs(ref[k]).max() + 1e-4, k


def test_f16_mode_vs_the_f32_engine(golden):
    """(e) arm 1, f16: the config and bars of test_model_gpu.py::test_tiny_f16_close_to_oracle, erf_gelu=True in both arms."""
    ids = golden("tiny_d2_patched")["token_ids"]
    ref = f32_arm(2, ids)
    res, _ = run_hip(synth.TINY, "f16", 4, ids, 2, erf_gelu=True)
    print("erf_gelu f16 vs f32:", {k: f"{maxerr(res[k], ref[k]):.2e}" for k in ("img_f", "txt_f", "logits")})
    for k in ("img_f", "txt_f"):
        assert maxerr(res[k], ref[k]) < 4e-3, (k, maxerr(res[k], ref[k]))
    assert maxerr(res["logits"], ref["logits"]) < 0.06
    for k in GRADS:
        assert maxerr(res[k], ref[k]) <= 0.08 * np.abs(ref[k]).max() + 1e-4, k


@pytest.mark.parametrize("dtype", ["bf16", "f16"])
def test_folded_c_fc_agrees_with_the_unfolded_one(monkeypatch, dtype):
    """(e) arm 2: LayerNorm folded into c_fc (LPI_EPI_LN, then the activation kernel) against LayerNorm as its own kernel, erf_gelu=True in both arms.  The fold
    needs N = 2 d, 3 d and 4 d in whole 256-column tiles (lpi_gemm_ln_supported), i.e. a width that is a multiple of 256: synth.TINY14's vision tower (256) is
    the smallest — its text tower (128) takes the unfolded pair in both arms — and the row count does not matter (arenas are padded to 256 rows), so the batch
    is 2, the smallest with a contrastive term.  Bars: those of test_model_gpu.py::test_layernorm_fold_levels_agree_and_do_not_lose_accuracy between fold
    levels (features 3e-3 bf16 / 6e-4 f16, factor-gradient cosine 0.995), like it with the two-sweep statistics in both arms.  That the folded GEMM really
    ran — LPI_EPI_LN at N = 4 d on the persistent 256 x 256 kernel — is asserted from lpi_gemm_last_kernel.  The spies sit on the three functions through which
    the engine launches a tower GEMM — gemm() (one problem), _lib.gemm_grouped (the towers' pair in one launch) and _lib.gemm_rows (few-row GEMMs, alone or
    paired) — so "no QuickGELU epilogue ran" covers the paired launches of the lock-stepped towers too."""
    cfg = synth.TINY14
    ids = synth.token_ids(2)
    seen = []
    real = E.gemm

    def spy(dt, a, b, c, M, N, K, **kw):
        real(dt, a, b, c, M, N, K, **kw)
        seen.append((kw.get("epi", E.EPI_NONE), N, K, int(_lib.load().lpi_gemm_last_kernel())))

    epis = []      # the epilogue of EVERY GEMM launch: the grouped and the few-row entry points take it as their third argument
    real_grouped, real_rows = _lib.gemm_grouped, _lib.gemm_rows

    def spy_grouped(dt, cdt, epi, *rest):
        epis.append(("grouped", epi))
        return real_grouped(dt, cdt, epi, *rest)

    def spy_rows(dt, cdt, epi, *rest):
        epis.append(("rows", epi))
        return real_rows(dt, cdt, epi, *rest)

    res = {}
    for level in (0, 2):
        monkeypatch.setattr(E, "gemm", spy)
        monkeypatch.setattr(_lib, "gemm_grouped", spy_grouped)
        monkeypatch.setattr(_lib, "gemm_rows", spy_rows)
        del seen[:], epis[:]
        res[level], _ = run_hip(cfg, dtype, 2, ids, 2, erf_gelu=True, ln_fold=level, rowstats=0)
        monkeypatch.setattr(E, "gemm", real)
        monkeypatch.setattr(_lib, "gemm_grouped", real_grouped)
        monkeypatch.setattr(_lib, "gemm_rows", real_rows)
        assert any(k == "rows" for k, _ in epis), "the few-row GEMMs (the pooled c_fc among them) did not pass the spy"
        assert not [e for e in epis if e[1] in (E.EPI_QUICKGELU, E.EPI_LN_QUICKGELU)], ("a QuickGELU epilogue ran with erf_gelu=True", epis)
        assert any(e[1] == E.EPI_DQUICKGELU for e in epis) or any(s[0] == E.EPI_DQUICKGELU for s in seen)      # the unchanged backward reads the saved derivative
        folded = [s for s in seen if s[0] == E.EPI_LN and s[1] == 4 * cfg.vision_width and s[2] == cfg.vision_width]
        assert not [s for s in seen if s[0] in (E.EPI_QUICKGELU, E.EPI_LN_QUICKGELU)], "a QuickGELU epilogue ran with erf_gelu=True"
        if level == 0:
            assert not folded
        else:
            assert folded and all(s[3] in (_lib.GEMM_K_256, _lib.GEMM_K_256_TAIL) for s in folded), seen
    d_feat = max(maxerr(res[2]["img_f"], res[0]["img_f"]), maxerr(res[2]["txt_f"], res[0]["txt_f"]))
    cos = lambda a, b: float((a * b).sum() / np.sqrt((a * a).sum() * (b * b).sum()))  # noqa: E731
    print(f"erf_gelu {dtype} fold 2 vs 0: features differ by {d_feat:.2e}; gradient cosines", {k: round(cos(res[2][k], res[0][k]), 5) for k in GRADS})
    assert d_feat <= (3e-3 if dtype == "bf16" else 6e-4)
    for k in GRADS:
        assert cos(res[2][k], res[0][k]) > 0.995, k


def _eval_inputs(golden):
    from lpi_amd.engine import prompt_cp_fwd
    cfg = synth.TINY
    g = golden("tiny_eval")
    img = torch.from_numpy(synth.images(6, 32, seed=synth.IMAGE_SEED + 7)).to(DEV)
    ids = torch.from_numpy(g["token_ids"]).to(DEV)
    allf = [synth.prompt_factors(9, 16, cfg.vision_width, cfg.transformer_width, task=t) for t in range(12)]
    vis_all, txt_all = [], []
    for fnp in allf:
        f = {k: torch.from_numpy(v).to(DEV) for k, v in fnp.items()}
        vis_all.append(prompt_cp_fwd(f["dim_1_share"], f["dim_2_visual"], f["dim_3_visual"]))
        txt_all.append(prompt_cp_fwd(f["dim_1_share"], f["dim_2_textual"], f["dim_3_textual"]))
    vis_sel = torch.stack(vis_all)[torch.from_numpy(g["sel_v"]).to(DEV)]
    txt_sel = torch.stack(txt_all)[torch.from_numpy(g["sel_t"]).to(DEV)]
    return g, img, ids, allf, vis_sel, txt_sel


def _four_interfaces(enc, img, ids, vis_sel, txt_sel, train):
    """extract_vector, visual_interface, extract_textual_vector, textual_interface as the plugin calls the engine (test_model_gpu.py::test_eval_interfaces_f32)."""
    with torch.no_grad():
        out = {"extract_vector": enc.encode_image(img, None, train=train).clone(), "visual_interface": enc.encode_image(img, vis_sel, train=train).clone(),
               "extract_textual_vector": enc.encode_text(ids, None, train=train).clone(), "textual_interface": enc.encode_text(ids, txt_sel, train=train).clone()}
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("dtype", ["f32", "bf16", "f16"])
def test_no_grad_forwards(monkeypatch, golden, dtype):
    """(f) the four evaluation interfaces with the option on: the bits of the training forward's features wherever the QuickGELU engine has that property
    (the forward that saves gelu' and the one that does not must round alike) — on the parent that is all four interfaces in all three modes, which is
    asserted, so the property is checked 4 times per mode — and in f32 the oracle with nn.GELU at 1e-4, the bar of test_model_gpu.py::test_eval_interfaces_f32."""
    cfg = synth.TINY
    g, img, ids, allf, vis_sel, txt_sel = _eval_inputs(golden)
    sd = synth.clip_state_dict(cfg)
    quick = DualEncoder(cfg, sd, dtype=dtype, device=DEV)
    q_eval, q_train = (_four_interfaces(quick, img, ids, vis_sel, txt_sel, t) for t in (False, True))
    del quick
    erf = DualEncoder(cfg, sd, dtype=dtype, device=DEV, options=EngineOptions(erf_gelu=True))
    n0 = _lib.launch_count()
    e_eval, e_train = (_four_interfaces(erf, img, ids, vis_sel, txt_sel, t) for t in (False, True))
    assert _lib.launch_count() > n0
    held = 0
    for k in e_eval:
        assert not same_bits(e_eval[k], q_eval[k]), k      # the option changes the features
        if same_bits(q_eval[k], q_train[k]):
            held += 1
            assert same_bits(e_eval[k], e_train[k]), (dtype, k, maxerr(e_eval[k].cpu().numpy(), e_train[k].cpu().numpy()))
    print(f"erf_gelu {dtype}: train=False features equal the training forward's bit for bit on {held} of 4 interfaces (those where the QuickGELU engine's do)")
    assert held == 4, (dtype, held)      # the QuickGELU engine has the property on every interface in every mode (measured on the parent's device code)
    if dtype == "f32":
        O = gelu_ref.erf_oracle(monkeypatch)
        orc = O.Oracle(cfg, sd, torch.float64)
        allf_t = [{k: torch.from_numpy(v).double() for k, v in f.items()} for f in allf]
        icpu, idc = img.cpu(), ids.cpu()
        with torch.no_grad():
            ref = {"extract_vector": orc.extract_vector(icpu), "visual_interface": orc.visual_interface(icpu, torch.from_numpy(g["sel_v"]), allf_t),
                   "extract_textual_vector": orc.extract_textual_vector(idc), "textual_interface": orc.textual_interface(idc, torch.from_numpy(g["sel_t"]), allf_t)}
        for k in ref:
            assert maxerr(e_eval[k].cpu().numpy(), ref[k].numpy()) < 1e-4, (k, maxerr(e_eval[k].cpu().numpy(), ref[k].numpy()))


# launches of ONE train_step of a fresh default engine on TINY, 4 pairs, depth 2 — counted on the build of the parent commit (before act.hip existed)
PARENT_LAUNCHES = {"f32": 91, "bf16": 70, "f16": 68}


@pytest.mark.parametrize("dtype", ["f32", "bf16", "f16"])
def test_option_off_is_the_parent(dtype):
    """(g) a default engine issues the parent's number of launches and gives reproducible bits; with the option on the forward has one more launch per tower
    and block (4 on TINY), the backward none."""
    cfg = synth.TINY
    sd = synth.clip_state_dict(cfg)
    img = torch.from_numpy(synth.images(4, cfg.image_resolution)).to(DEV)
    ids = torch.from_numpy(synth.token_ids(4)).to(DEV)

    def step(options):
        enc = DualEncoder(cfg, sd, dtype=dtype, device=DEV, options=options)
        fac = {k: torch.from_numpy(v).to(DEV).requires_grad_(True) for k, v in synth.prompt_factors(9, 16, cfg.vision_width, cfg.transformer_width).items()}
        torch.cuda.synchronize()
        n0 = _lib.launch_count()
        out = train_step(enc, img, ids, fac, 2)
        torch.cuda.synchronize()
        n = _lib.launch_count() - n0
        return n, [out["img_f"].clone(), out["txt_f"].clone(), out["base_loss"].clone(), out["alignment_loss"].clone()] + [fac[k].grad.clone() for k in synth.PROMPT_NAMES]

    n_a, a = step(None)
    n_b, b = step(EngineOptions())
    n_on, on = step(EngineOptions(erf_gelu=True))
    print(f"launches of a TINY train_step, {dtype}: default {n_a}, erf_gelu {n_on}")
    assert n_a == n_b == PARENT_LAUNCHES[dtype]
    assert all(same_bits(x, y) for x, y in zip(a, b))
    assert n_on == n_a + 4
    assert not same_bits(on[0], a[0])
