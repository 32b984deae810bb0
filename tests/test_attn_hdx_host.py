"""Attention for 88- and 104-wide heads (csrc/attn_hd88.hip, attn_hd104.hip behind lpi_attn_hd_fwd / _bwd; OpenCLIP ViT-g/14 and ViT-bigG/14) and the MLP width
as a property of the tower, without a GPU: lpi_attn_hd_supported and every refusal of the envelope at the new widths before any launch (aligned addresses that
are never dereferenced: a launch would fault, a refusal returns); nine kernels per object, no scratch, no spill; the four configs, the MLP-width fields, the
loader's inference of them, unchanged synthetic weights of the old configs; the plugin; the `tail8` arm's premises; and the yardstick itself — the oracle's
attention at head widths 88 and 104 and its block with a 6144-wide MLP against plain torch."""
import hashlib
import json
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import attn_hdx_cases as X  # noqa: E402
from lpi_amd import _lib, checkpoint, synth  # noqa: E402
from test_attn_hd_host import EINVAL, A, _check_walk_kernels  # noqa: E402

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _fwd(hd, dt=_lib.BF16, B=2, L=273, H=16, qkv=A, ldqkv=None, ctx=A, ldctx=None, lse=A):
    ldqkv, ldctx = 3 * H * hd if ldqkv is None else ldqkv, H * hd if ldctx is None else ldctx
    return _lib.load().lpi_attn_hd_fwd(dt, B, L, H, hd, qkv, ldqkv, ctx, ldctx, lse, None)


def _bwd(hd, dt=_lib.BF16, B=2, L=273, H=16, qkv=A, ldqkv=None, ctx=A, ldctx=None, dctx=A, lddctx=None, lse=A, delta=A, dqkv=A, lddqkv=None):
    ldqkv, lddqkv = (3 * H * hd if v is None else v for v in (ldqkv, lddqkv))
    ldctx, lddctx = (H * hd if v is None else v for v in (ldctx, lddctx))
    return _lib.load().lpi_attn_hd_bwd(dt, B, L, H, hd, qkv, ldqkv, ctx, ldctx, dctx, lddctx, lse, delta, dqkv, lddqkv, None)


def test_abi_number():
    assert _lib.EXPECTED_ABI >= 625 and _lib.load().lpi_version() == _lib.EXPECTED_ABI


def test_supported_at_the_new_widths_and_nowhere_else():
    """1 for 88 and 104 at L in {1, 288, 289, 1024}, 0 at 1025; 0 for 64, 72, 96, 112, 0 and -88 (72 is 8 mod 16 too: the widths are a list, not a rule), where
    both entry points refuse a call whose every other argument is valid, and nothing is launched."""
    lib = _lib.load()
    before = _lib.launch_count()
    for hd in X.WIDTHS:
        for H in (1, 16):
            for L in (1, 288, 289, 1024):
                assert lib.lpi_attn_hd_supported(L, H, hd) == 1, (L, H, hd)
            assert lib.lpi_attn_hd_supported(1025, H, hd) == 0
            assert _fwd(hd, L=1025, H=H) == EINVAL and _bwd(hd, L=1025, H=H) == EINVAL
        assert lib.lpi_attn_hd_supported(0, 16, hd) == 0 and lib.lpi_attn_hd_supported(273, 0, hd) == 0
    for hd in (64, 72, 96, 112, 0, -88):
        for L in (1, 273, 1024):
            assert lib.lpi_attn_hd_supported(L, 16, hd) == 0, (L, hd)
            assert _fwd(hd, L=L) == EINVAL and _bwd(hd, L=L) == EINVAL, (L, hd)
            assert _fwd(hd, L=L, ldqkv=3 * 16 * 104, ldctx=16 * 104) == EINVAL      # generous leading dimensions do not make the width acceptable
            assert _bwd(hd, L=L, ldqkv=3 * 16 * 104, lddqkv=3 * 16 * 104, ldctx=16 * 104, lddctx=16 * 104) == EINVAL
    assert _lib.launch_count() == before


@pytest.mark.parametrize("hd", X.WIDTHS)
def test_every_refusal_returns_before_any_launch(hd):
    """test_attn_hd_host.py's list with H * hd in place of H * 80: the leading dimensions are held to the head width of the call."""
    before = _lib.launch_count()
    d = 16 * hd
    shape = [dict(L=0), dict(L=1025), dict(L=-1), dict(B=0), dict(B=-2), dict(H=0), dict(H=-1), dict(B=4096, H=16), dict(dt=_lib.MX8), dict(dt=_lib.F32X3),
             dict(dt=-1), dict(dt=99)]
    fwd = shape + [dict(qkv=A + 8), dict(qkv=A + 2), dict(ctx=A + 8), dict(qkv=None), dict(ctx=None), dict(lse=None),
                   dict(ldqkv=3 * d - 8), dict(ldqkv=3 * d + 4), dict(ldqkv=3 * d + 1), dict(ldctx=d - 8), dict(ldctx=d + 4), dict(ldctx=d + 1),
                   dict(ldqkv=3 * 16 * 80), dict(ldctx=16 * 80),      # what an 80-wide call of the same H takes
                   dict(dt=_lib.F32, ldctx=d + 4),      # a whole number of 16-byte units in f32, but not a multiple of 8 elements
                   dict(dt=_lib.F32, ldqkv=3 * d + 2)]
    bwd = shape + [dict(qkv=A + 8), dict(ctx=A + 4), dict(dctx=A + 8), dict(dqkv=A + 8), dict(qkv=None), dict(ctx=None), dict(dctx=None), dict(lse=None),
                   dict(delta=None), dict(dqkv=None), dict(ldqkv=3 * d - 8), dict(ldqkv=3 * d + 4), dict(lddqkv=3 * d - 8), dict(lddqkv=3 * d + 1),
                   dict(ldctx=d - 8), dict(ldctx=d + 4), dict(lddctx=d - 8), dict(lddctx=d + 3), dict(lddqkv=3 * 16 * 80), dict(lddctx=16 * 80),
                   dict(dt=_lib.F32, lddctx=d + 2), dict(dt=_lib.F32, ldqkv=3 * d + 1)]
    ptrs = {_fwd: ("qkv", "ctx", "lse"), _bwd: ("qkv", "ctx", "dctx", "lse", "delta", "dqkv")}
    for fn, cases in ((_fwd, fwd), (_bwd, bwd)):
        for kw in cases:
            assert fn(hd, **kw) == EINVAL, (fn.__name__, kw)
            none = dict(kw, **{p: None for p in ptrs[fn] if p not in kw})      # the refusals hold with NULL operands too
            assert fn(hd, **none) == EINVAL, (fn.__name__, kw)
    assert _lib.launch_count() == before


@pytest.mark.parametrize("hd", X.WIDTHS)
def test_kernels_use_no_scratch(tmp_path, hd):
    """attn_hd88.o / attn_hd104.o: nine kernels each (3 forward, 3 dQ, 3 dK / dV), every one instantiated at that width only, private segment 0, no VGPR spill."""
    _check_walk_kernels(tmp_path, "attn_hd%d.o" % hd, hd)


# ------------------------------------------------------------------------------------------------------------------------------ configuration
def test_the_four_configs():
    g, b, gw, bw = (synth.CONFIGS[n] for n in ("ViT-g/14", "ViT-bigG/14", "g14-widths", "bigG14-widths"))
    assert g.as_clip_args() == (1024, 224, 40, 1408, 14, 77, 49408, 1024, 16, 24) and b.as_clip_args() == (1280, 224, 48, 1664, 14, 77, 49408, 1280, 20, 32)
    assert gw.as_clip_args() == (1024, 28, 2, 1408, 14, 77, 49408, 1024, 16, 2) and bw.as_clip_args() == (1280, 28, 2, 1664, 14, 77, 49408, 1280, 20, 2)
    for c, hd, f in ((g, 88, 6144), (gw, 88, 6144), (b, 104, 8192), (bw, 104, 8192)):
        assert (c.vision_head_width, c.vision_heads, c.vision_mlp_width, c.vision_mlp, c.transformer_mlp_width) == (hd, 16, f, f, None)
        assert c.transformer_mlp == 4 * c.transformer_width and c.transformer_width // c.transformer_heads == 64 and len(c.as_clip_args()) == 10
    assert 1 + g.n_patches == 257 and 1 + gw.n_patches == 5 and 1 + bw.n_patches == 5
    for name in ("tiny", "tinyH80", "ViT-H/14", "ViT-L/14"):      # the default: 4 x width, recorded as None
        c = synth.CONFIGS[name]
        assert c.vision_mlp_width is None and c.transformer_mlp_width is None and c.vision_mlp == 4 * c.vision_width and c.transformer_mlp == 4 * c.transformer_width


def test_mlp_width_validation():
    base = ("a", 128, 32, 2, 128, 16, 77, 49408, 128, 2, 2)
    assert synth.ClipConfig(*base, vision_mlp_width=640).vision_mlp == 640 and synth.ClipConfig(*base, transformer_mlp_width=384).transformer_mlp == 384
    for bad in (0, -128, 100, 6144 + 64, 512.0, True):
        with pytest.raises(ValueError, match="MLP width"):
            synth.ClipConfig(*base, vision_mlp_width=bad)
        with pytest.raises(ValueError, match="MLP width"):
            synth.ClipConfig(*base, transformer_mlp_width=bad)
    with pytest.raises(TypeError):      # keyword fields: the eleven positional arguments stay what they were
        synth.ClipConfig(*base, 640)
    a, b = synth.ClipConfig(*base), synth.ClipConfig(*base, vision_mlp_width=640)
    assert a.as_clip_args() == b.as_clip_args() and not checkpoint.same_architecture(a, b)
    assert checkpoint.same_architecture(a, synth.ClipConfig(*base, vision_mlp_width=512, transformer_mlp_width=512))      # 4 x width said explicitly
    assert not checkpoint.same_architecture(a, synth.ClipConfig(*base, transformer_mlp_width=384))


def test_infer_config_recovers_the_mlp_widths():
    for name, hd, f in (("g14-widths", 88, 6144), ("bigG14-widths", 104, 8192)):
        cfg = synth.CONFIGS[name]
        sd = synth.clip_state_dict(cfg)
        assert tuple(sd["visual.transformer.resblocks.1.mlp.c_fc.weight"].shape) == (f, cfg.vision_width)
        assert tuple(sd["visual.transformer.resblocks.1.mlp.c_proj.weight"].shape) == (cfg.vision_width, f)
        assert tuple(sd["transformer.resblocks.0.mlp.c_fc.weight"].shape) == (4 * cfg.transformer_width, cfg.transformer_width)
        got = checkpoint.infer_config(sd, "some-checkpoint", vision_head_width=hd)      # the MLP width is in the shapes; the head width is not
        assert (got.vision_mlp_width, got.transformer_mlp_width, got.vision_heads) == (f, None, 16) and checkpoint.same_architecture(got, cfg)
        assert checkpoint.infer_config(sd, name) == cfg      # a known name's head width
        assert checkpoint.infer_config(sd, "some-checkpoint").vision_mlp == f
    tiny = synth.clip_state_dict(synth.TINY)
    got = checkpoint.infer_config(tiny, "tiny")
    assert got == synth.TINY and got.vision_mlp == 512 and got.transformer_mlp == 512 and got.vision_mlp_width is None


# sha256 over the sorted (name, dtype, shape, bytes) of synth.clip_state_dict(cfg), recorded on the commit before the MLP-width fields: the generator is keyed by
# tensor name, so a default shape that moved would change these
PARENT_WEIGHTS = {"tiny": "cacf8b180fbc3ed5e269db2b3c7ddbe796796ce3ef8b800c884b4590c588cccf",
                  "tinyH80": "99911abb36f46daf6c5bca1a13ca3f2223006c76fc1c327322c6e479fca344b6"}


def test_old_configs_keep_their_synthetic_weights():
    for name, want in PARENT_WEIGHTS.items():
        sd = synth.clip_state_dict(synth.CONFIGS[name])
        h = hashlib.sha256()
        for k in sorted(sd):
            h.update(k.encode()), h.update(str(sd[k].dtype).encode()), h.update(str(tuple(sd[k].shape)).encode()), h.update(sd[k].tobytes())
        assert h.hexdigest() == want, name


def _args(**over):
    args = json.load(open(os.path.join(REPO, "lpi_amd", "retrieval", "configs", "lpi", "coco_lpi.json")))
    args.update(device=[torch.device("cpu")], backbonename="g14-widths", visual_dim=1408, textual_dim=1024)
    args.update(over)
    return args


def test_plugin_takes_the_widths_and_refuses_the_streamed_search_beyond_1024():
    from lpi_amd.retrieval.models.slinet import SliNet
    cfg = synth.CONFIGS["g14-widths"]
    sd = synth.clip_state_dict(cfg)
    assert SliNet(_args()).clip_cfg == cfg
    net = SliNet(_args(clip_state_dict=sd, backbonename="my-g14", vision_head_width=88))      # an unknown name: head width from the key, MLP width from the shapes
    assert net.clip_cfg.vision_heads == 16 and net.clip_cfg.vision_mlp == 6144 and checkpoint.same_architecture(net.clip_cfg, cfg) and net.feature_dim == 1024
    with pytest.raises(checkpoint.CheckpointError, match="head width"):      # 1408 = 22 x 64: a state dict alone is read as heads of 64, and 60 does not divide it
        SliNet(_args(clip_state_dict=sd, backbonename="my-g14", vision_head_width=60))
    assert SliNet(_args(eval_scores="streamed")).clip_cfg == cfg      # E = 1024: inside the streamed search's envelope
    big = dict(backbonename="bigG14-widths", visual_dim=1664, textual_dim=1280)
    assert SliNet(_args(**big)).clip_cfg.embed_dim == 1280      # the default, 'matrix', works
    assert SliNet(_args(eval_scores="matrix", **big)).clip_cfg.vision_mlp == 8192
    with pytest.raises(ValueError, match="streamed.*1024.*1280"):
        SliNet(_args(eval_scores="streamed", **big))


def test_engine_refuses_weights_that_disagree_with_the_config():
    """The MLP width is read from the tower's spec and checked against c_fc's shape before anything is put on a device."""
    from lpi_amd.engine import Tower, TowerSpec
    cfg = synth.CONFIGS["tiny"]
    assert TowerSpec(128, 2, 2, False).mlp_width == 512 and TowerSpec(1408, 16, 2, False, 6144).mlp_width == 6144
    with pytest.raises(ValueError, match="MLP of 640"):
        Tower(synth.clip_state_dict(cfg), "visual.transformer.", TowerSpec(128, 2, 2, False, 640), _lib.F32, "cpu")


# ------------------------------------------------------------------------------------------------------------------------------ the tail8 arm
@pytest.mark.parametrize("mode", ["f32", "bf16", "f16"])
@pytest.mark.parametrize("B,L,H", X.TAIL8_SHAPES)
@pytest.mark.parametrize("hd", X.WIDTHS)
def test_tail8_premises_hold_on_the_reference(hd, B, L, H, mode):
    """On the f64 reference alone: the inputs live in the last eight columns of every head, and they decide the result (score spread, lse off log L, ctx)."""
    ref = X.case(hd, B, L, H, "tail8", mode)
    q = ref["qkv"].float().view(B * L, 3 * H, hd)
    assert float(q[:, :, :hd - 8].abs().max()) == 0.0 and float(q[:, :, hd - 8:].abs().min()) > 0.0
    assert float(ref["dctx"].float().view(B * L, H, hd)[:, :, :hd - 8].abs().max()) == 0.0
    X.tail8_premises(ref, L)


# ------------------------------------------------------------------------------------------------------------------------------ the yardstick
@pytest.mark.parametrize("d,heads,hd", [(176, 2, 88), (1408, 16, 88), (208, 2, 104), (1664, 16, 104)])
def test_oracle_attention_at_the_new_head_widths(d, heads, hd):
    """The oracle's attention() at heads of 88 and 104, non-causal, f64, equals torch.nn.functional.multi_head_attention_forward with the same weights to 1e-12."""
    from oracle import lpi_oracle as O
    g = torch.Generator().manual_seed(5)
    B, L = 2, 7
    x = torch.randn(B, L, d, generator=g, dtype=torch.float64)
    w_in, b_in = torch.randn(3 * d, d, generator=g, dtype=torch.float64) * d ** -0.5, torch.randn(3 * d, generator=g, dtype=torch.float64) * 0.1
    w_out, b_out = torch.randn(d, d, generator=g, dtype=torch.float64) * d ** -0.5, torch.randn(d, generator=g, dtype=torch.float64) * 0.1
    assert d // heads == hd
    got = O.attention(x, w_in, b_in, w_out, b_out, heads, False)
    ref, _ = torch.nn.functional.multi_head_attention_forward(x.transpose(0, 1), x.transpose(0, 1), x.transpose(0, 1), d, heads, w_in, b_in, None, None, False, 0.0,
                                                              w_out, b_out, need_weights=False)
    assert got.shape == (B, L, d)
    assert float((got - ref.transpose(0, 1)).abs().max()) < 1e-12


def test_oracle_block_with_a_6144_wide_mlp():
    """The oracle's res_block takes the MLP's shape from the weights: g14-widths' first vision block (1408 -> 6144 -> 1408, 16 heads of 88) in f64 against
    nn.MultiheadAttention + nn.LayerNorm + two nn.Linear around QuickGELU, built from the same tensors."""
    from oracle import lpi_oracle as O
    cfg = synth.CONFIGS["g14-widths"]
    pre = "visual.transformer.resblocks.0."
    W = {k: torch.from_numpy(v).double() for k, v in synth.clip_state_dict(cfg).items() if k.startswith(pre)}
    d, f = cfg.vision_width, cfg.vision_mlp
    assert tuple(W[pre + "mlp.c_fc.weight"].shape) == (f, d) == (6144, 1408)
    x = torch.randn(2, 5, d, generator=torch.Generator().manual_seed(6), dtype=torch.float64)
    got = O.res_block(x, W, pre, cfg.vision_heads, False)
    nn = torch.nn
    attn = nn.MultiheadAttention(d, cfg.vision_heads, batch_first=True, dtype=torch.float64)
    ln1, ln2, fc, proj = nn.LayerNorm(d, dtype=torch.float64), nn.LayerNorm(d, dtype=torch.float64), nn.Linear(d, f, dtype=torch.float64), nn.Linear(f, d, dtype=torch.float64)
    with torch.no_grad():
        attn.in_proj_weight.copy_(W[pre + "attn.in_proj_weight"]), attn.in_proj_bias.copy_(W[pre + "attn.in_proj_bias"])
        attn.out_proj.weight.copy_(W[pre + "attn.out_proj.weight"]), attn.out_proj.bias.copy_(W[pre + "attn.out_proj.bias"])
        for m, n in ((ln1, "ln_1"), (ln2, "ln_2"), (fc, "mlp.c_fc"), (proj, "mlp.c_proj")):
            m.weight.copy_(W[pre + n + ".weight"]), m.bias.copy_(W[pre + n + ".bias"])
        h = ln1(x)
        y = x + attn(h, h, h, need_weights=False)[0]
        u = fc(ln2(y))
        ref = y + proj(u * torch.sigmoid(1.702 * u))
    assert got.shape == ref.shape and float((got - ref).abs().max()) < 1e-11 * max(1.0, float(ref.abs().max()))
