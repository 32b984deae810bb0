"""Attention for 88- and 104-wide heads on a real MI355X (csrc/attn_hd88.hip, attn_hd104.hip behind lpi_attn_hd_fwd / _bwd) and the engine, the configs and the
plugin on top of it (OpenCLIP ViT-g/14: 16 heads of 88, MLP 6144; ViT-bigG/14: 16 heads of 104, MLP 8192).  The form of tests/test_attn_hd_gpu.py with the head
width a parameter: kernels against f64 autograd on the rounded inputs with the key-walking family's own bars; the last EIGHT columns — the live half of the last
16-column tile; bit-exact independence of heads and samples; padded leading dimensions with NaN in every gap and canaries around every output; the engine at
the two models' widths against the f64 oracle (the reference cannot build them: model.py:292), once with nn.GELU; the plugin."""
import json
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import attn_hdx_cases as X  # noqa: E402
import gelu_ref  # noqa: E402
import strided as S  # noqa: E402
from lpi_amd import _lib, synth  # noqa: E402
from lpi_amd._lib import call  # noqa: E402
from poison import same_bits  # noqa: E402
from test_attn_hd_gpu import GRADS, check, cos, inputs, maxerr, oracle, weights  # noqa: E402

DEV = "cuda:0"
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODES = ["f32", "bf16", "f16"]
WIDTHS = list(X.WIDTHS)


def stream():
    return torch.cuda.current_stream().cuda_stream


def run_dense(HD, mode, B, L, H, qkv, dctx, count=False):
    """forward + backward on contiguous device copies -> (ctx, lse, delta, dqkv); ctx and dqkv pre-filled with 7.0 so that an unwritten row or column shows"""
    dt, td, tg = X.MODES[mode]
    d = H * HD
    qd, dd = qkv.to(DEV), dctx.to(DEV)
    ctx = torch.full((B * L, d), 7.0, device=DEV, dtype=td)
    lse = torch.zeros(B, H, L, device=DEV)
    n0 = _lib.launch_count()
    call("lpi_attn_hd_fwd", dt, B, L, H, HD, qd, 3 * d, ctx, d, lse, stream())
    n1 = _lib.launch_count()
    dqkv = torch.full((B * L, 3 * d), 7.0, device=DEV, dtype=tg)
    delta = torch.zeros(B, H, L, device=DEV)
    call("lpi_attn_hd_bwd", dt, B, L, H, HD, qd, 3 * d, ctx, d, dd, d, lse, delta, dqkv, 3 * d, stream())
    if count:      # launches per call: one for the forward, two for the backward, as the long family has
        assert (n1 - n0, _lib.launch_count() - n1) == (1, 2)
    torch.cuda.synchronize()
    return ctx, lse, delta, dqkv


def hold(HD, mode, H, outs, ref, label):
    e = X.errors(HD, mode, H, *outs, ref)
    bar = X.bars(mode)
    print(f"ATTN_HD{HD} {label} {mode}: " + "  ".join(f"{k} {v:.3e} (bar {bar[k]:g})" for k, v in e.items()))
    for k, v in e.items():
        assert v < bar[k], (HD, label, mode, k, v, bar[k])


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("B,L,H", X.SHAPES)
@pytest.mark.parametrize("HD", WIDTHS)
def test_fwd_bwd_against_f64_autograd(HD, B, L, H, mode):
    """Every block edge of a 16-, 32-, 64- or 128-row tiling from both sides, the real towers' lengths and the envelope's end; a dominant late key (L >= 8) forces
    the running-max rescale.  The key-walking family's own bars, unchanged."""
    ref = X.case(HD, B, L, H, "late", mode)
    outs = run_dense(HD, mode, B, L, H, ref["qkv"], ref["dctx"], count=True)
    for t in outs:
        assert bool(torch.isfinite(t.float()).all())
    hold(HD, mode, H, outs, ref, f"late ({B}, {L}, {H})")


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("B,L,H", X.TAIL8_SHAPES)
@pytest.mark.parametrize("HD", WIDTHS)
def test_the_last_eight_columns_count(HD, B, L, H, mode):
    """q, k, v, dctx zero in the columns 0 .. HD - 9 of every head and random in the last eight: a kernel that drops, mis-pads or mis-masks the half tile returns a
    uniform softmax (lse = log L) and zero ctx, which the same bars catch grossly — the premises asserted first, on the CPU reference alone."""
    ref = X.case(HD, B, L, H, "tail8", mode)
    X.tail8_premises(ref, L)
    outs = run_dense(HD, mode, B, L, H, ref["qkv"], ref["dctx"])
    hold(HD, mode, H, outs, ref, f"tail8 ({B}, {L}, {H})")


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("B,L,H", [(2, 129, 2), (1, 273, 2)])
@pytest.mark.parametrize("HD", WIDTHS)
def test_heads_and_samples_are_independent_bit_for_bit(HD, B, L, H, mode):
    """Head 1's columns of qkv and dctx replaced by other finite data of magnitude 1e4: head 0's ctx, lse, delta, dq, dk, dv keep their bits (a half-tile load or
    store that strays into the neighbouring head's columns, or padding taken from them, would not); the same for sample 1 against sample 0; two identical calls
    give identical bits."""
    _, td, tg = X.MODES[mode]
    ref = X.case(HD, B, L, H, "late", mode)
    d = H * HD
    base = run_dense(HD, mode, B, L, H, ref["qkv"], ref["dctx"])
    again = run_dense(HD, mode, B, L, H, ref["qkv"], ref["dctx"])
    for a, b in zip(base, again):
        assert same_bits(a, b)
    h0_qkv, h0 = X.head_cols(HD, H, 0).to(DEV), X.head_cols(HD, H, 0, 1).to(DEV)

    def head0(outs):
        ctx, lse, delta, dqkv = outs
        return ctx[:, h0], lse[:, 0], delta[:, 0], dqkv[:, h0_qkv]

    qkv2, dctx2 = ref["qkv"].clone(), ref["dctx"].clone()
    h1_qkv, h1 = X.head_cols(HD, H, 1), X.head_cols(HD, H, 1, 1)
    qkv2[:, h1_qkv] = (X.rnd(B * L, 3 * HD, seed=21).sign() * 1e4).to(td)
    dctx2[:, h1] = (X.rnd(B * L, HD, seed=22).sign() * 1e4).to(tg)
    assert bool(torch.isfinite(qkv2.float()).all()) and float(qkv2.float().abs().max()) > 9e3
    other = run_dense(HD, mode, B, L, H, qkv2, dctx2)
    for name, a, b in zip(("ctx", "lse", "delta", "dqkv"), head0(base), head0(other)):
        assert a.numel() > 0 and torch.equal(a, b), ("head", name)
    if B > 1:
        qkv3, dctx3 = ref["qkv"].clone(), ref["dctx"].clone()
        qkv3[L:] = (X.rnd(B * L - L, 3 * d, seed=23).sign() * 1e4).to(td)
        dctx3[L:] = (X.rnd(B * L - L, d, seed=24).sign() * 1e4).to(tg)
        other = run_dense(HD, mode, B, L, H, qkv3, dctx3)
        for name, a, b in zip(("ctx", "lse", "delta", "dqkv"), base, other):
            rows = slice(0, 1) if name in ("lse", "delta") else slice(0, L)
            assert torch.equal(a[rows], b[rows]), ("sample", name)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("pad", [8, 24])
@pytest.mark.parametrize("HD", WIDTHS)
def test_padded_leading_dimensions_and_write_bounds(HD, pad, mode):
    """Every leading dimension padded by `pad` elements (each operand with its own), NaN in every gap, in front of every operand and in three rows behind B L
    (the last row's tail included); UNWRITTEN NaNs in the outputs — a column the half tile's guard left out shows —, canaries (the arenas' pads) around them
    and around lse and delta — a store of the dead half shows.  Outputs finite, equal to the dense call's bits, every pad intact, every input untouched."""
    B, L, H = 2, 129, 2
    dt, td, tg = X.MODES[mode]
    ref = X.case(HD, B, L, H, "late", mode)
    d, rows = H * HD, B * L
    dense = run_dense(HD, mode, B, L, H, ref["qkv"], ref["dctx"])
    ld_qkv, ld_ctx, ld_dctx, ld_dqkv = 3 * d + pad, d + pad, d + 2 * pad, 3 * d + 3 * pad      # four different strides
    col0 = 16
    nbytes = S.arena_bytes(rows + 3, ld_dqkv, 4, col0)      # one arena size for every operand of the case (strided.py: the safety rule)
    elems = lambda t: nbytes // torch.empty(0, dtype=t).element_size()  # noqa: E731
    qkv = S.operand(rows, 3 * d, ld_qkv, td, col0, elems(td), ref["qkv"], DEV)
    ctx = S.operand(rows, d, ld_ctx, td, col0, elems(td), None, DEV)
    dctx = S.operand(rows, d, ld_dctx, tg, col0, elems(tg), ref["dctx"], DEV)
    dqkv = S.operand(rows, 3 * d, ld_dqkv, tg, col0, elems(tg), None, DEV)
    n = B * H * L
    lse = S.region(torch.arange(64, 64 + n), torch.float32, elems(torch.float32), None, DEV)
    delta = S.region(torch.arange(64, 64 + n), torch.float32, elems(torch.float32), None, DEV)
    call("lpi_attn_hd_fwd", dt, B, L, H, HD, qkv.t, ld_qkv, ctx.t, ld_ctx, lse.t[64:], stream())
    torch.cuda.synchronize()
    S.check_written("ctx", ctx), S.check_written("lse", lse)
    for name, rec in (("qkv", qkv), ("ctx", ctx), ("lse", lse)):
        S.check_pads(name, rec)
    # the backward reads the forward's ctx and lse: inputs from here on
    ctx.before, lse.before = S.bits(ctx.arena).clone(), S.bits(lse.arena).clone()
    ctx.output = lse.output = False
    call("lpi_attn_hd_bwd", dt, B, L, H, HD, qkv.t, ld_qkv, ctx.t, ld_ctx, dctx.t, ld_dctx, lse.t[64:], delta.t[64:], dqkv.t, ld_dqkv, stream())
    torch.cuda.synchronize()
    S.check_written("dqkv", dqkv), S.check_written("delta", delta)
    for name, rec in (("qkv", qkv), ("ctx", ctx), ("dctx", dctx), ("lse", lse), ("delta", delta), ("dqkv", dqkv)):
        S.check_pads(name, rec)
    got = (ctx.t.contiguous(), lse.t[64:64 + n].view(B, H, L), delta.t[64:64 + n].view(B, H, L), dqkv.t.contiguous())
    for name, a, b in zip(("ctx", "lse", "delta", "dqkv"), got, dense):
        assert bool(torch.isfinite(a.float()).all()), name
        assert same_bits(a, b), name


# ---------------------------------------------------------------------------------------------------------------------------------- engine
SHAPE = {"g14-widths": (88, 6144), "bigG14-widths": (104, 8192)}


def run_engine(cfg, dtype, batch, depth, r, lockstep=True, eval_too=False, erf_gelu=False):
    from lpi_amd.engine import DualEncoder, EngineOptions
    from lpi_amd.step import train_step
    enc = DualEncoder(cfg, weights(cfg), dtype=dtype, device=DEV, options=EngineOptions.from_env(erf_gelu=True) if erf_gelu else None)
    hd, f = SHAPE[cfg.name]
    assert enc.vis.hd == hd and enc.txt.hd == 64 and not enc.vis.pooled_last and enc.txt.pooled_last
    assert enc.vis.spec.mlp_width == f and enc.txt.spec.mlp_width == 4 * cfg.transformer_width
    img_np, ids, fac_np = inputs(cfg, batch, r)
    fac = {k: torch.from_numpy(v).to(DEV).requires_grad_(True) for k, v in fac_np.items()}
    img, idt = torch.from_numpy(img_np).to(DEV), torch.from_numpy(ids).to(DEV)
    n0 = _lib.launch_count()
    out = train_step(enc, img, idt, fac, depth, lockstep=lockstep)
    torch.cuda.synchronize()
    assert _lib.launch_count() > n0
    res = {k: v.cpu().numpy() for k, v in out.items()}
    res["logits"] = (enc.logit_scale_exp * out["img_f"] @ out["txt_f"].t()).cpu().numpy()
    for k in synth.PROMPT_NAMES:
        res["grad." + k] = fac[k].grad.cpu().numpy()
    if eval_too:      # the no-grad forwards (train=False) on the same prompts
        with torch.no_grad():
            res["img_f_eval"] = enc.encode_image(img, out["vis_prompt"], depth, train=False).cpu().numpy()
            res["txt_f_eval"] = enc.encode_text(idt, out["txt_prompt"], depth, train=False).cpu().numpy()
    return res


def hold_engine(cfg, batch, depth, r, label, lockstep_arm):
    """tests/test_attn_hd_gpu.py::hold_engine: the project's bars, set at d = 1280, unchanged — f32 tol 2e-5, gtol 2e-4; bf16 / f16 features < 2e-2, gradient
    cosine > 0.99; train=False features at the same bars.  The measured errors are printed first."""
    ref = oracle(cfg, batch, depth, r)
    res = run_engine(cfg, "f32", batch, depth, r, eval_too=True)
    print(f"ATTN_HDX engine {label} f32: " + "  ".join(f"{k} {maxerr(res[k], ref[k]):.3e}" for k in ("img_f", "txt_f", "logits"))
          + "  worst grad err / scale " + f"{max(maxerr(res[k], ref[k]) / np.abs(ref[k]).max() for k in GRADS):.3e}")
    check(res, ref, tol=2e-5, gtol=2e-4)
    for k in ("img_f", "txt_f"):
        assert maxerr(res[k + "_eval"], ref[k]) <= 2e-5, (k, "train=False")
    if lockstep_arm:
        for mode in ("f32", "bf16"):
            a = res if mode == "f32" else run_engine(cfg, mode, batch, depth, r)
            b = run_engine(cfg, mode, batch, depth, r, lockstep=False)
            for k in ["img_f", "txt_f"] + GRADS:
                assert np.array_equal(a[k], b[k]), (mode, k, "lock step against one tower after the other")
    for mode in ("bf16", "f16"):
        r16 = run_engine(cfg, mode, batch, depth, r, eval_too=True)
        print(f"ATTN_HDX engine {label} {mode}: " + "  ".join(f"{k} {maxerr(r16[k], ref[k]):.3e}" for k in ("img_f", "txt_f"))
              + "  min cosine " + f"{min(cos(r16[k], ref[k]) for k in GRADS):.5f}")
        for k in ("img_f", "txt_f"):
            assert maxerr(r16[k], ref[k]) < 2e-2, (mode, k, maxerr(r16[k], ref[k]))
            assert maxerr(r16[k + "_eval"], ref[k]) < 2e-2, (mode, k, "train=False")
        for k in GRADS:
            assert cos(r16[k], ref[k]) > 0.99, (mode, k, cos(r16[k], ref[k]))


@pytest.mark.parametrize("depth", [1, 2])
def test_engine_g14_widths_against_the_oracle(depth):
    """g14-widths (vision 1408 = 16 heads of 88 with an MLP of 6144, text 1024 = 16 heads of 64, E = 1024; 4 patches + CLS, 2 + 2 layers), 2 pairs, r 4: the test
    that finds a row kernel, few-row GEMM or LN-fold predicate that does not take d = 1408 (a multiple of 128, not of 256) or f = 6144 != 4 d.  At depth 2 also
    the towers in lock step against one after the other: the same bits."""
    hold_engine(synth.CONFIGS["g14-widths"], 2, depth, 4, f"g14-widths depth {depth}", lockstep_arm=depth == 2)


def test_engine_bigg14_widths_against_the_oracle():
    """bigG14-widths: vision 1664 = 16 heads of 104 with an MLP of 8192, text 1280 = 20 heads of 64, E = 1280; 2 pairs, depth 2, r 4."""
    hold_engine(synth.CONFIGS["bigG14-widths"], 2, 2, 4, "bigG14-widths", lockstep_arm=False)


def test_engine_g14_widths_with_nn_gelu(monkeypatch):
    """These checkpoints were trained with nn.GELU: erf_gelu=True on g14-widths in f32 against the f64 oracle with its activation patched to the erf form
    (tests/gelu_ref.py, the arm of tests/test_erf_gelu_gpu.py), at the same f32 bars."""
    cfg = synth.CONFIGS["g14-widths"]
    quick = oracle(cfg, 2, 2, 4)      # the QuickGELU oracle (shared, cached) BEFORE the patch
    O = gelu_ref.erf_oracle(monkeypatch)
    img, ids, fac_np = inputs(cfg, 2, 4)
    ref = O.train_step(O.Oracle(cfg, weights(cfg), torch.float64), img, ids, fac_np, depth=2)
    assert maxerr(ref["img_f"], quick["img_f"]) > 10 * 2e-5      # the two activations differ by more than ten times the bar: a QuickGELU engine cannot pass
    res = run_engine(cfg, "f32", 2, 2, 4, erf_gelu=True)
    print("ATTN_HDX engine g14-widths erf_gelu f32: " + "  ".join(f"{k} {maxerr(res[k], ref[k]):.3e}" for k in ("img_f", "txt_f", "logits")))
    check(res, ref, tol=2e-5, gtol=2e-4)


def test_plugin_synthetic_weights_and_state_dict_with_the_config_key():
    """SliNet with backbonename g14-widths: one train_step, then extract_vector — with the synthetic weights and with the same state dict handed over as
    clip_state_dict + vision_head_width 88 under a name the package does not know (the MLP width comes from the shapes).  Equal bits."""
    from lpi_amd.retrieval.models.slinet import SliNet
    cfg = synth.CONFIGS["g14-widths"]
    args = json.load(open(os.path.join(REPO, "lpi_amd", "retrieval", "configs", "lpi", "coco_lpi.json")))
    args.update(backbonename="g14-widths", visual_dim=1408, textual_dim=1024, device=[torch.device(DEV)], compute_dtype="bf16", batch_size=4, epochs=1, num_workers=0)
    img = torch.from_numpy(synth.images(4, cfg.image_resolution)).to(DEV)
    ids = torch.from_numpy(synth.token_ids(4))
    got = []
    for over in ({}, {"clip_state_dict": weights(cfg), "backbonename": "my-g14", "vision_head_width": 88}):
        net = SliNet(dict(args, **over)).to(DEV)
        assert net.clip_cfg.vision_heads == 16 and net.clip_cfg.vision_mlp == 6144
        for t in range(len(net.prompts)):
            for k, v in synth.prompt_factors(9, 16, 1408, 1024, task=t).items():
                getattr(net.prompts[t], k).data = torch.from_numpy(v.copy()).to(DEV)
        net.numtask = 1
        net.train()
        for n, p in net.named_parameters():
            p.requires_grad_("prompts.0." in n)
            p.grad = None
        n0 = _lib.launch_count()
        out = net.train_step(img, ids)
        net.eval()
        with torch.no_grad():
            vec = net.extract_vector(img)
        torch.cuda.synchronize()
        assert _lib.launch_count() - n0 > 30
        assert bool(torch.isfinite(vec).all()) and vec.shape == (4, cfg.embed_dim)
        got.append([out["image_features"], out["text_features"], vec] + [getattr(net.prompts[0], k).grad for k in synth.PROMPT_NAMES])
    for a, b in zip(*got):
        assert torch.equal(a, b)
