"""Attention for 80-wide heads (csrc/attn_hd.hip; OpenCLIP ViT-H/14's vision tower) without a GPU: header, binding and ABI number of the three entry points; every
refusal of the envelope before any launch (NULL or never-dereferenced addresses: a launch would fault, a refusal returns); lpi_attn_hd_supported against the
refusals; no scratch and no spill in the nine kernels; the config field, the checkpoint loader's and the plugin's head-width argument; the engine option that does
not combine with such a tower; and the yardstick itself — the oracle's attention at head widths other than 64 against torch's multi_head_attention_forward."""
import ctypes
import json
import os
import re
import shutil
import subprocess

import pytest
import torch

from lpi_amd import _lib, checkpoint, synth

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LLVM = "/opt/rocm/lib/llvm/bin"
EINVAL = -22
_I, _P = _lib._I, _lib._P
NAMES = ("lpi_attn_hd_supported", "lpi_attn_hd_fwd", "lpi_attn_hd_bwd")


def _header():
    txt = open(os.path.join(REPO, "include", "lpi_hip.h")).read()
    return re.sub(r"/\*.*?\*/", "", txt, flags=re.S)


def _params(hdr, name):
    m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, hdr)
    assert m, name
    return [_P if "*" in p else {"int": _I}[p.split()[0]] for p in (q.strip() for q in m.group(1).split(","))]


def test_header_binding_and_abi():
    hdr = _header()
    fwd = [_I, _I, _I, _I, _I, _P, _I, _P, _I, _P, _P]      # dtype B L H head_dim qkv ldqkv ctx ldctx lse stream
    bwd = [_I, _I, _I, _I, _I, _P, _I, _P, _I, _P, _I, _P, _P, _P, _I, _P]      # ... ctx ldctx dctx lddctx lse delta dqkv lddqkv stream
    assert _params(hdr, "lpi_attn_hd_supported") == _lib.SIGNATURES["lpi_attn_hd_supported"] == [_I, _I, _I]
    assert _params(hdr, "lpi_attn_hd_fwd") == _lib.SIGNATURES["lpi_attn_hd_fwd"] == fwd
    assert _params(hdr, "lpi_attn_hd_bwd") == _lib.SIGNATURES["lpi_attn_hd_bwd"] == bwd
    api = open(os.path.join(REPO, "lpi_amd", "csrc", "api.hip")).read()
    assert int(re.search(r"#define LPI_ABI_VERSION (\d+)", api).group(1)) == _lib.EXPECTED_ABI >= 624
    assert _lib.load().lpi_version() == _lib.EXPECTED_ABI


def test_the_three_symbols_are_exported():
    lib = _lib.load()
    for name in NAMES:
        assert hasattr(lib, name) and name not in _lib._RESTYPES
    raw = ctypes.CDLL(_lib.LIB_PATH)      # the dynamic symbol table itself, past the binding's own bookkeeping
    for name in NAMES:
        assert getattr(raw, name) is not None


A = 1 << 20      # an aligned non-NULL address that is never dereferenced: every case below is refused on the host


def _fwd(dt=_lib.BF16, B=2, L=273, H=16, hd=80, qkv=A, ldqkv=None, ctx=A, ldctx=None, lse=A):
    ldqkv, ldctx = 3 * H * 80 if ldqkv is None else ldqkv, H * 80 if ldctx is None else ldctx
    return _lib.load().lpi_attn_hd_fwd(dt, B, L, H, hd, qkv, ldqkv, ctx, ldctx, lse, None)


def _bwd(dt=_lib.BF16, B=2, L=273, H=16, hd=80, qkv=A, ldqkv=None, ctx=A, ldctx=None, dctx=A, lddctx=None, lse=A, delta=A, dqkv=A, lddqkv=None):
    ldqkv, lddqkv = (3 * H * 80 if v is None else v for v in (ldqkv, lddqkv))
    ldctx, lddctx = (H * 80 if v is None else v for v in (ldctx, lddctx))
    return _lib.load().lpi_attn_hd_bwd(dt, B, L, H, hd, qkv, ldqkv, ctx, ldctx, dctx, lddctx, lse, delta, dqkv, lddqkv, None)


def test_every_refusal_returns_before_any_launch():
    before = _lib.launch_count()
    d = 16 * 80
    shape = [dict(hd=64), dict(hd=72), dict(hd=96), dict(hd=0), dict(hd=-80), dict(L=0), dict(L=1025), dict(L=-1), dict(B=0), dict(B=-2), dict(H=0), dict(H=-1),
             dict(B=4096, H=16), dict(dt=_lib.MX8), dict(dt=_lib.F32X3), dict(dt=-1), dict(dt=99)]
    fwd = shape + [dict(qkv=A + 8), dict(qkv=A + 2), dict(ctx=A + 8), dict(qkv=None), dict(ctx=None), dict(lse=None),
                   dict(ldqkv=3 * d - 8), dict(ldqkv=3 * d + 4), dict(ldqkv=3 * d + 1), dict(ldctx=d - 8), dict(ldctx=d + 4), dict(ldctx=d + 1),
                   dict(dt=_lib.F32, ldctx=d + 4),      # a whole number of 16-byte units in f32, but not a multiple of 8 elements
                   dict(dt=_lib.F32, ldqkv=3 * d + 2)]
    bwd = shape + [dict(qkv=A + 8), dict(ctx=A + 4), dict(dctx=A + 8), dict(dqkv=A + 8), dict(qkv=None), dict(ctx=None), dict(dctx=None), dict(lse=None),
                   dict(delta=None), dict(dqkv=None), dict(ldqkv=3 * d - 8), dict(ldqkv=3 * d + 4), dict(lddqkv=3 * d - 8), dict(lddqkv=3 * d + 1),
                   dict(ldctx=d - 8), dict(ldctx=d + 4), dict(lddctx=d - 8), dict(lddctx=d + 3), dict(dt=_lib.F32, lddctx=d + 2), dict(dt=_lib.F32, ldqkv=3 * d + 1)]
    ptrs = {_fwd: ("qkv", "ctx", "lse"), _bwd: ("qkv", "ctx", "dctx", "lse", "delta", "dqkv")}
    for fn, cases in ((_fwd, fwd), (_bwd, bwd)):
        for kw in cases:
            assert fn(**kw) == EINVAL, (fn.__name__, kw)
            none = dict(kw, **{p: None for p in ptrs[fn] if p not in kw})      # the refusals hold with NULL operands too
            assert fn(**none) == EINVAL, (fn.__name__, kw)
    assert _lib.launch_count() == before


def test_supported_agrees_with_the_refusals():
    """lpi_attn_hd_supported over L x H x head width: 1 exactly inside the envelope; wherever it says 0, both entry points refuse a call whose every other
    argument is valid (aligned non-NULL addresses, never dereferenced), and nothing is launched."""
    lib = _lib.load()
    before = _lib.launch_count()
    for L in (1, 288, 289, 1024, 1025):
        for H in (1, 16):
            for hd in (64, 80, 96):
                ok = lib.lpi_attn_hd_supported(L, H, hd)
                assert ok == (1 if (hd == 80 and L <= 1024) else 0), (L, H, hd)
                if not ok:
                    assert _fwd(L=L, H=H, hd=hd) == EINVAL and _bwd(L=L, H=H, hd=hd) == EINVAL, (L, H, hd)
    assert lib.lpi_attn_hd_supported(0, 16, 80) == 0 and lib.lpi_attn_hd_supported(273, 0, 80) == 0 and lib.lpi_attn_hd_supported(273, 16, 0) == 0
    assert _lib.launch_count() == before


def _check_walk_kernels(tmp_path, obj_name, width):
    """(private segment, VGPR spill) == (0, 0) for the nine kernels of csrc/build/<obj_name>: forward x (f32, bf16, f16), backward dQ and backward dK / dV x (f32,
    bf16, fp16-saved with bf16 gradients), each an instantiation of attn_walk.h at the one head width `width`."""
    src = os.path.join(REPO, "lpi_amd", "csrc", "build", obj_name)
    if not os.path.exists(src) or not os.path.exists(os.path.join(LLVM, "llvm-objdump")):
        pytest.skip(obj_name + " not built (run __graft_entry__.build()) or llvm-objdump not available")
    obj = shutil.copy(src, tmp_path / obj_name)
    subprocess.run([os.path.join(LLVM, "llvm-objdump"), "--offloading", str(obj)], check=True, capture_output=True, cwd=tmp_path)
    dev = [p for p in os.listdir(tmp_path) if "amdgcn" in p]
    assert dev
    notes = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "--notes", str(tmp_path / dev[0])], check=True, capture_output=True, text=True).stdout
    ks = {}
    for blk in notes.split("- .agpr_count:")[1:]:
        name, size = re.search(r"\.name:\s+(\S+)", blk), re.search(r"\.private_segment_fixed_size:\s+(\d+)", blk)
        if name and size:
            ks[name.group(1)] = (int(size.group(1)), int(re.search(r"\.vgpr_spill_count:\s+(\d+)", blk).group(1)))
    assert len(ks) == 9, sorted(ks)
    for kind, n in (("attn_walk_fwd_kernel", 3), ("attn_walk_bwd_dq_kernel", 3), ("attn_walk_bwd_dkv_kernel", 3)):
        assert sum(kind in k for k in ks) == n, (kind, sorted(ks))
    assert all("Li%dE" % width in k for k in ks), sorted(ks)      # the head width is a template argument; one instantiation per object
    assert {k: v for k, v in ks.items() if v != (0, 0)} == {}


def test_attn_hd_kernels_use_no_scratch(tmp_path):
    """.private_segment_fixed_size == 0 and no VGPR spill for every kernel of attn_hd.hip: nine, each instantiated at head width 80 only."""
    _check_walk_kernels(tmp_path, "attn_hd.o", 80)


def test_attn_long_kernels_use_no_scratch(tmp_path):
    """The same for attn_long.hip, the family's instantiation at head width 64."""
    _check_walk_kernels(tmp_path, "attn_long.o", 64)


# ------------------------------------------------------------------------------------------------------------------------------ configuration
# as_clip_args() of every config that existed before the head-width field: the ten arguments of the reference's CLIP.__init__, unchanged
OLD_ARGS = {
    "ViT-B/16": (512, 224, 12, 768, 16, 77, 49408, 512, 8, 12),
    "ViT-L/14": (768, 224, 24, 1024, 14, 77, 49408, 768, 12, 12),
    "ViT-L/14@336px": (768, 336, 24, 1024, 14, 77, 49408, 768, 12, 12),
    "ViT-B/32": (512, 224, 12, 768, 32, 77, 49408, 512, 8, 12),
    "tiny": (128, 32, 2, 128, 16, 77, 49408, 128, 2, 2),
    "tiny14": (128, 28, 2, 256, 14, 77, 49408, 128, 2, 2),
    "tinyLong": (128, 80, 2, 128, 4, 77, 49408, 128, 2, 2),
}


def test_config_field():
    h14 = synth.CONFIGS["ViT-H/14"]
    assert h14.vision_heads == 16 and h14.vision_head_width == 80 and h14.transformer_heads == 16 and h14.transformer_width // h14.transformer_heads == 64
    assert h14.as_clip_args() == (1024, 224, 32, 1280, 14, 77, 49408, 1024, 16, 24)
    assert 1 + h14.n_patches == 257
    for name, args in OLD_ARGS.items():
        c = synth.CONFIGS[name]
        assert c.as_clip_args() == args and len(c.as_clip_args()) == 10 and c.vision_head_width == 64 and c.vision_heads == c.vision_width // 64
    for name in ("ViT-H/14", "tinyH80", "H14-shallow"):
        assert len(synth.CONFIGS[name].as_clip_args()) == 10
    t = synth.CONFIGS["tinyH80"]
    assert (t.vision_width, t.vision_heads, t.vision_layers, t.n_patches, t.transformer_width, t.transformer_heads, t.embed_dim) == (640, 8, 2, 4, 128, 2, 128)
    s = synth.CONFIGS["H14-shallow"]
    assert s.as_clip_args() == (1024, 224, 2, 1280, 14, 77, 49408, 1024, 16, 2) and s.vision_heads == 16
    w64 = synth.ClipConfig("a", 128, 32, 2, 640, 16, 77, 49408, 128, 2, 2)
    w80 = synth.ClipConfig("a", 128, 32, 2, 640, 16, 77, 49408, 128, 2, 2, vision_head_width=80)
    assert w64.vision_heads == 10 and w80.vision_heads == 8 and w64.as_clip_args() == w80.as_clip_args()
    assert not checkpoint.same_architecture(w64, w80) and checkpoint.same_architecture(w80, t) and checkpoint.same_architecture(w64, w64)
    for bad in (7, 0, -80, 1280):
        with pytest.raises(ValueError, match="head width"):
            synth.ClipConfig("a", 128, 32, 2, 640, 16, 77, 49408, 128, 2, 2, vision_head_width=bad)
    with pytest.raises(TypeError):      # a keyword field: the eleven positional arguments stay what they were
        synth.ClipConfig("a", 128, 32, 2, 640, 16, 77, 49408, 128, 2, 2, 80)


def test_infer_config_head_width():
    sd = synth.clip_state_dict(synth.CONFIGS["tinyH80"])
    assert checkpoint.infer_config(sd, "some-checkpoint").vision_heads == 10      # a state dict does not say: build_model's width // 64
    assert checkpoint.infer_config(sd, "some-checkpoint", vision_head_width=80).vision_heads == 8
    assert checkpoint.infer_config(sd, "tinyH80").vision_heads == 8      # a known name's width
    assert checkpoint.infer_config(sd, "tinyH80", vision_head_width=64).vision_heads == 10      # the argument wins; the plugin then refuses the disagreement
    for bad in (7, 0, -80, 96):
        with pytest.raises(checkpoint.CheckpointError, match="head width"):
            checkpoint.infer_config(sd, "some-checkpoint", vision_head_width=bad)
    tiny = synth.clip_state_dict(synth.TINY)
    assert checkpoint.infer_config(tiny, "tiny") == synth.TINY and checkpoint.infer_config(tiny, "x").vision_head_width == 64


def _args(**over):
    args = json.load(open(os.path.join(REPO, "lpi_amd", "retrieval", "configs", "lpi", "coco_lpi.json")))
    args.update(device=[torch.device("cpu")], backbonename="tinyH80", visual_dim=640, textual_dim=128)
    args.update(over)
    return args


def test_plugin_head_width_key():
    from lpi_amd.retrieval.models.slinet import SliNet
    sd = synth.clip_state_dict(synth.CONFIGS["tinyH80"])
    assert SliNet(_args()).clip_cfg.vision_heads == 8
    assert SliNet(_args(vision_head_width=80)).clip_cfg.vision_heads == 8
    assert SliNet(_args(clip_state_dict=sd)).clip_cfg.vision_heads == 8      # the known name's width
    assert SliNet(_args(clip_state_dict=sd, vision_head_width=80)).clip_cfg.vision_heads == 8
    net = SliNet(_args(clip_state_dict=sd, backbonename="my-h80", vision_head_width=80))
    assert net.clip_cfg.vision_heads == 8 and checkpoint.same_architecture(net.clip_cfg, synth.CONFIGS["tinyH80"])
    assert SliNet(_args(clip_state_dict=sd, backbonename="my-h80")).clip_cfg.vision_heads == 10
    with pytest.raises(ValueError, match="names .* vision heads of 80"):      # the key disagrees with the known backbone
        SliNet(_args(clip_state_dict=sd, vision_head_width=64))
    with pytest.raises(ValueError, match="names vision heads of 80"):
        SliNet(_args(vision_head_width=64))
    with pytest.raises(ValueError, match="names .* vision heads of 64"):
        SliNet(_args(backbonename="tiny", visual_dim=128, clip_state_dict=synth.clip_state_dict(synth.TINY), vision_head_width=32))
    with pytest.raises(ValueError, match="integer"):
        SliNet(_args(vision_head_width="80"))
    with pytest.raises(checkpoint.CheckpointError, match="head width"):
        SliNet(_args(clip_state_dict=sd, backbonename="my-h80", vision_head_width=7))
    with pytest.raises(ValueError, match="visual_dim"):      # checked against the backbone as before
        SliNet(_args(visual_dim=1280))


def test_mx8_forward_refuses_such_a_tower_at_construction():
    from lpi_amd.engine import DualEncoder, EngineOptions
    cfg = synth.CONFIGS["tinyH80"]
    with pytest.raises(ValueError, match="mx8_forward does not combine with vision heads of 80"):      # before anything touches a GPU
        DualEncoder(cfg, {}, dtype="bf16", device="cuda:0", options=EngineOptions(mx8_forward=True))


# ------------------------------------------------------------------------------------------------------------------------------ the yardstick
@pytest.mark.parametrize("d,heads", [(160, 2), (640, 8)])
def test_oracle_attention_at_other_head_widths(d, heads):
    """The oracle is pinned by reference fixtures at head width 64 only, and is the yardstick for ViT-H/14: its attention() at heads of 80, non-causal, f64,
    equals torch.nn.functional.multi_head_attention_forward with the same weights to 1e-12."""
    from oracle import lpi_oracle as O
    g = torch.Generator().manual_seed(5)
    B, L = 2, 7
    x = torch.randn(B, L, d, generator=g, dtype=torch.float64)
    w_in, b_in = torch.randn(3 * d, d, generator=g, dtype=torch.float64) * d ** -0.5, torch.randn(3 * d, generator=g, dtype=torch.float64) * 0.1
    w_out, b_out = torch.randn(d, d, generator=g, dtype=torch.float64) * d ** -0.5, torch.randn(d, generator=g, dtype=torch.float64) * 0.1
    assert d // heads == 80
    got = O.attention(x, w_in, b_in, w_out, b_out, heads, False)
    ref, _ = torch.nn.functional.multi_head_attention_forward(x.transpose(0, 1), x.transpose(0, 1), x.transpose(0, 1), d, heads, w_in, b_in, None, None, False, 0.0,
                                                              w_out, b_out, need_weights=False)
    assert got.shape == (B, L, d)
    assert float((got - ref.transpose(0, 1)).abs().max()) < 1e-12
