"""Attention for 80-wide heads on a real MI355X (csrc/attn_hd.hip: lpi_attn_hd_fwd / _bwd) and the engine, the configs and the plugin on top of it (OpenCLIP
ViT-H/14's vision tower: 16 heads of 80).  Kernels against f64 autograd on the rounded inputs with the key-walking family's own bars; the last 16 columns; bit-exact
independence of heads and samples; padded leading dimensions with NaN in every gap and canaries around every output; the engine at tinyH80 and at ViT-H/14's
widths against the f64 oracle (the reference cannot build this model: model.py:292); the plugin with synthetic weights and with a state dict + vision_head_width."""
import json
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import attn_hd_cases as C  # noqa: E402
import strided as S  # noqa: E402
from lpi_amd import _lib, synth  # noqa: E402
from lpi_amd._lib import call  # noqa: E402
from poison import same_bits  # noqa: E402

DEV = "cuda:0"
HD = C.HD
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def stream():
    return torch.cuda.current_stream().cuda_stream


def run_dense(mode, B, L, H, qkv, dctx, count=False):
    """forward + backward on contiguous device copies -> (ctx, lse, delta, dqkv); dqkv pre-filled with 7.0 so that an unwritten row shows"""
    dt, td, tg = C.MODES[mode]
    d = H * HD
    qd, dd = qkv.to(DEV), dctx.to(DEV)
    ctx = torch.zeros(B * L, d, device=DEV, dtype=td)
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


def hold(mode, H, outs, ref, label):
    e = C.errors(mode, H, *outs, ref)
    bar = C.bars(mode)
    print(f"ATTN_HD {label} {mode}: " + "  ".join(f"{k} {v:.3e} (bar {bar[k]:g})" for k, v in e.items()))
    for k, v in e.items():
        assert v < bar[k], (label, mode, k, v, bar[k])


@pytest.mark.parametrize("mode", ["f32", "bf16", "f16"])
@pytest.mark.parametrize("B,L,H", C.SHAPES)
def test_fwd_bwd_against_f64_autograd(mode, B, L, H):
    """Every block edge of a 16-, 32-, 64- or 128-row tiling from both sides, the real towers' lengths and the envelope's end; a dominant late key (L >= 8) forces
    the running-max rescale.  The key-walking family's own bars, unchanged."""
    ref = C.case(B, L, H, "late", mode)
    outs = run_dense(mode, B, L, H, ref["qkv"], ref["dctx"], count=True)
    for t in outs:
        assert bool(torch.isfinite(t.float()).all())
    hold(mode, H, outs, ref, f"late ({B}, {L}, {H})")


@pytest.mark.parametrize("mode", ["f32", "bf16", "f16"])
@pytest.mark.parametrize("B,L,H", [(2, 17, 2), (2, 129, 2), (1, 273, 2)])
def test_the_upper_sixteen_columns_count(mode, B, L, H):
    """q, k, v, dctx zero in the columns 0 .. 63 of every head and random in 64 .. 79: a kernel that drops or mis-pads the last 16 columns returns a uniform
    softmax (lse = log L) and zero ctx, which the same bars catch grossly — asserted first, on the CPU reference alone: the scores of every query spread over the
    keys by more than 1 and lse lies more than 1 off the uniform softmax's log L."""
    ref = C.case(B, L, H, "upper", mode)
    s = ref["scores"]
    assert float((s.max(-1).values - s.min(-1).values).min()) > 1.0
    assert float((ref["lse"] - C.uniform_lse(L)).abs().max()) > 1.0
    assert float(ref["ctx"].abs().max()) > 0.5
    outs = run_dense(mode, B, L, H, ref["qkv"], ref["dctx"])
    hold(mode, H, outs, ref, f"upper ({B}, {L}, {H})")


@pytest.mark.parametrize("mode", ["f32", "bf16", "f16"])
@pytest.mark.parametrize("B,L,H", [(2, 129, 2), (1, 273, 2)])
def test_heads_and_samples_are_independent_bit_for_bit(mode, B, L, H):
    """Head 1's columns of qkv and dctx replaced by other finite data of magnitude 1e4: head 0's ctx, lse, delta, dq, dk, dv keep their bits (a load that strays
    into the neighbouring head's columns, or padding taken from them, would not); the same for sample 1 against sample 0; two identical calls give identical bits."""
    _, td, tg = C.MODES[mode]
    ref = C.case(B, L, H, "late", mode)
    d = H * HD
    base = run_dense(mode, B, L, H, ref["qkv"], ref["dctx"])
    again = run_dense(mode, B, L, H, ref["qkv"], ref["dctx"])
    for a, b in zip(base, again):
        assert same_bits(a, b)
    h0_qkv, h0 = C.head_cols(H, 0).to(DEV), C.head_cols(H, 0, 1).to(DEV)

    def head0(outs):
        ctx, lse, delta, dqkv = outs
        return ctx[:, h0], lse[:, 0], delta[:, 0], dqkv[:, h0_qkv]

    qkv2, dctx2 = ref["qkv"].clone(), ref["dctx"].clone()
    h1_qkv, h1 = C.head_cols(H, 1), C.head_cols(H, 1, 1)
    qkv2[:, h1_qkv] = (C.rnd(B * L, 3 * HD, seed=21).sign() * 1e4).to(td)
    dctx2[:, h1] = (C.rnd(B * L, HD, seed=22).sign() * 1e4).to(tg)
    assert bool(torch.isfinite(qkv2.float()).all()) and float(qkv2.float().abs().max()) > 9e3
    other = run_dense(mode, B, L, H, qkv2, dctx2)
    for name, a, b in zip(("ctx", "lse", "delta", "dqkv"), head0(base), head0(other)):
        assert a.numel() > 0 and torch.equal(a, b), ("head", name)
    if B > 1:
        qkv3, dctx3 = ref["qkv"].clone(), ref["dctx"].clone()
        qkv3[L:] = (C.rnd(B * L - L, 3 * d, seed=23).sign() * 1e4).to(td)
        dctx3[L:] = (C.rnd(B * L - L, d, seed=24).sign() * 1e4).to(tg)
        other = run_dense(mode, B, L, H, qkv3, dctx3)
        for name, a, b in zip(("ctx", "lse", "delta", "dqkv"), base, other):
            rows = slice(0, 1) if name in ("lse", "delta") else slice(0, L)
            assert torch.equal(a[rows], b[rows]), ("sample", name)


@pytest.mark.parametrize("mode", ["f32", "bf16", "f16"])
@pytest.mark.parametrize("pad", [8, 24])
def test_padded_leading_dimensions_and_write_bounds(mode, pad):
    """Every leading dimension padded by `pad` elements (each operand with its own), NaN in every gap, in front of every operand and in three rows behind B L
    (the last row's tail included); UNWRITTEN NaNs in the outputs, canaries (the arenas' pads) around them and around lse and delta.  Outputs finite, equal to the
    dense call's bits, every pad intact, every input untouched."""
    B, L, H = 2, 129, 2
    dt, td, tg = C.MODES[mode]
    ref = C.case(B, L, H, "late", mode)
    d, rows = H * HD, B * L
    dense = run_dense(mode, B, L, H, ref["qkv"], ref["dctx"])
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
GRADS = ["grad." + n for n in synth.PROMPT_NAMES]
_ORACLE, _WEIGHTS = {}, {}


def weights(cfg):
    if cfg.name not in _WEIGHTS:
        _WEIGHTS[cfg.name] = synth.clip_state_dict(cfg)
    return _WEIGHTS[cfg.name]


def maxerr(a, b):
    return float(np.abs(np.asarray(a, dtype=np.float64) - np.asarray(b, dtype=np.float64)).max())


def cos(a, b):
    return float((a * b).sum() / np.sqrt((a * a).sum() * (b * b).sum()))


def check(res, ref, tol, gtol, gabs=1e-7):
    """tests/test_model_gpu.py::check"""
    for k in ("img_f", "txt_f", "logits", "base_loss", "alignment_loss"):
        assert maxerr(res[k], ref[k]) <= tol, (k, maxerr(res[k], ref[k]))
    for k in ("vis_prompt", "txt_prompt"):
        n = ref[k].shape[0]
        assert maxerr(res[k][:n], ref[k]) <= 1e-6, k
    for k in GRADS:
        e = maxerr(res[k], ref[k])
        scale = np.abs(ref[k]).max()
        assert e <= gtol * scale + gabs, (k, e, scale)


def inputs(cfg, batch, r):
    fac_np = synth.prompt_factors(9, 16, cfg.vision_width, cfg.transformer_width, r=r)
    return synth.images(batch, cfg.image_resolution), synth.token_ids(batch), fac_np


def oracle(cfg, batch, depth, r):
    """the f64 oracle's train step, once per (config, batch, depth, rank)"""
    key = (cfg.name, batch, depth, r)
    if key not in _ORACLE:
        from oracle import lpi_oracle as O
        img, ids, fac_np = inputs(cfg, batch, r)
        _ORACLE[key] = O.train_step(O.Oracle(cfg, weights(cfg), torch.float64), img, ids, fac_np, depth=depth)
    return _ORACLE[key]


def run_engine(cfg, dtype, batch, depth, r, lockstep=True, eval_too=False):
    from lpi_amd.engine import DualEncoder
    from lpi_amd.step import train_step
    enc = DualEncoder(cfg, weights(cfg), dtype=dtype, device=DEV)
    assert enc.vis.hd == 80 and enc.txt.hd == 64 and not enc.vis.pooled_last and enc.txt.pooled_last
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
    ref = oracle(cfg, batch, depth, r)
    res = run_engine(cfg, "f32", batch, depth, r, eval_too=True)
    print(f"ATTN_HD engine {label} f32: " + "  ".join(f"{k} {maxerr(res[k], ref[k]):.3e}" for k in ("img_f", "txt_f", "logits")))
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
        print(f"ATTN_HD engine {label} {mode}: " + "  ".join(f"{k} {maxerr(r16[k], ref[k]):.3e}" for k in ("img_f", "txt_f"))
              + "  min cosine " + f"{min(cos(r16[k], ref[k]) for k in GRADS):.5f}")
        for k in ("img_f", "txt_f"):
            assert maxerr(r16[k], ref[k]) < 2e-2, (mode, k, maxerr(r16[k], ref[k]))
            assert maxerr(r16[k + "_eval"], ref[k]) < 2e-2, (mode, k, "train=False")
        for k in GRADS:
            assert cos(r16[k], ref[k]) > 0.99, (mode, k, cos(r16[k], ref[k]))


@pytest.mark.parametrize("depth", [1, 2])
def test_engine_tiny_h80_against_the_oracle(depth):
    """tinyH80 (vision 640 = 8 heads of 80, text 128 = 2 heads of 64), 4 pairs: f32 at the bars of test_long_sequence_tower_vs_oracle, bf16 / f16 at theirs; the
    train=False features at the same bars; the towers in lock step (last blocks of different forms: full + gather against pooled) and one after the other give
    the same bits."""
    hold_engine(synth.CONFIGS["tinyH80"], 4, depth, 4, f"tinyH80 depth {depth}", lockstep_arm=True)


def test_engine_vit_h14_widths_against_the_oracle():
    """H14-shallow: ViT-H/14's widths (d = 1280, E = 1024, text 1024), patch and resolution with 2 + 2 layers; 2 pairs, depth 2, r 4 — the test that finds a row
    kernel or few-row GEMM that does not take d = 1280 or E = 1024."""
    hold_engine(synth.CONFIGS["H14-shallow"], 2, 2, 4, "H14-shallow", lockstep_arm=False)


def test_plugin_synthetic_weights_and_state_dict_with_the_config_key():
    """SliNet with backbonename tinyH80: one train_step, then extract_vector — with the synthetic weights and with the same state dict handed over as
    clip_state_dict + vision_head_width 80 under a name the package does not know (a state dict alone would be read as 10 heads of 64).  Equal bits."""
    from lpi_amd.retrieval.models.slinet import SliNet
    cfg = synth.CONFIGS["tinyH80"]
    args = json.load(open(os.path.join(REPO, "lpi_amd", "retrieval", "configs", "lpi", "coco_lpi.json")))
    args.update(backbonename="tinyH80", visual_dim=640, textual_dim=128, device=[torch.device(DEV)], compute_dtype="bf16", batch_size=4, epochs=1, num_workers=0)
    img = torch.from_numpy(synth.images(4, cfg.image_resolution)).to(DEV)
    ids = torch.from_numpy(synth.token_ids(4))
    got = []
    for over in ({}, {"clip_state_dict": synth.clip_state_dict(cfg), "backbonename": "my-h80", "vision_head_width": 80}):
        net = SliNet(dict(args, **over)).to(DEV)
        assert net.clip_cfg.vision_heads == 8
        for t in range(len(net.prompts)):
            for k, v in synth.prompt_factors(9, 16, 640, 128, task=t).items():
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
