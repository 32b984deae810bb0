"""The vision front end at patch 14 and at other input resolutions, without a GPU: lpi_pos_embed_resample's header, binding, ABI number and every refusal of
its envelope before any launch (made-up addresses: a launch would fault, a refusal returns); lpi_patchify_u8 takes the geometries whose patch size or resolution
is no multiple of 4 and keeps its other refusals; ClipConfig.at_resolution; EngineOptions.pos_embed; the plugin's config keys image_resolution and
pos_embed_interpolation with their construction-time refusals; and that nothing changes for a config without the new keys."""
import json
import os
import re

import pytest
import torch

from lpi_amd import _lib, synth

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = -22
_I, _L, _P = _lib._I, _lib._L, _lib._P
A = 0x7E0000000000      # aligned made-up addresses, 16 MiB apart: never dereferenced by the host layer
A2 = A + 0x1000000
A3 = A + 0x2000000


# ---------------------------------------------------------------------------------------------------------------------------------- the C ABI
def test_header_binding_and_abi():
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "lpi_hip.h")).read(), flags=re.S)
    m = re.search(r"\bint\s+lpi_pos_embed_resample\s*\(([^)]*)\)\s*;", hdr)
    assert m
    params = [_P if "*" in p else {"int": _I, "long": _L}[p.split()[0]] for p in (q.strip() for q in m.group(1).split(","))]
    assert params == _lib.SIGNATURES["lpi_pos_embed_resample"] == [_I, _I, _I, _P, _L, _P, _L, _I, _I, _P]
    assert re.search(r"#define LPI_POS_BICUBIC 0\b", hdr) and re.search(r"#define LPI_POS_BILINEAR 1\b", hdr)
    api = open(os.path.join(REPO, "lpi_amd", "csrc", "api.hip")).read()
    assert int(re.search(r"#define LPI_ABI_VERSION (\d+)", api).group(1)) == _lib.EXPECTED_ABI >= 626
    assert _lib.load().lpi_version() == _lib.EXPECTED_ABI
    assert "posembed" in open(os.path.join(REPO, "lpi_amd", "csrc", "build.sh")).read()


def _resample(g_in=7, g_out=12, d=128, src=A, lds=None, dst=A2, ldd=None, filter=0, antialias=1):
    return _lib.load().lpi_pos_embed_resample(g_in, g_out, d, src, d if lds is None else lds, dst, d if ldd is None else ldd, filter, antialias, None)


def test_pos_embed_resample_refuses_before_any_launch():
    before = _lib.launch_count()
    cases = [dict(g_in=v) for v in (0, -1, 65)] + [dict(g_out=v) for v in (0, -1, 65)] + [dict(d=0), dict(d=6), dict(d=-4)]
    cases += [dict(lds=124), dict(lds=130), dict(lds=129), dict(ldd=124), dict(ldd=130), dict(ldd=131), dict(lds=0), dict(ldd=-128)]
    cases += [dict(src=A + 4), dict(dst=A2 + 4), dict(src=A + 8), dict(dst=A2 + 8), dict(src=None), dict(dst=None)]
    cases += [dict(filter=2), dict(filter=-1), dict(antialias=2), dict(antialias=-1)]
    src_bytes = (7 * 7 * 128 + 128) * 4
    cases += [dict(dst=A),                            # dst is src
              dict(dst=A + 16),                       # dst inside src
              dict(dst=A + src_bytes - 16),           # dst starts in src's last row
              dict(src=A2 + 16, dst=A2 - 64),         # src inside dst
              dict(g_in=14, g_out=14, dst=A + 512)]   # the copy does not take overlapping tables either
    for kw in cases:
        assert _resample(**kw) == EINVAL, kw
    assert _lib.launch_count() == before


def _device_present():
    return torch.cuda.device_count() != 0


def test_pos_embed_resample_accepts_the_envelopes_corners():
    """Accepted argument lists count one launch.  Without a device the launch then fails in the runtime (a positive HIP code, never LPI_EINVAL) and nothing is
    dereferenced; with one, the same lists run on real tensors."""
    for g_in, g_out, d, pad in ((1, 1, 4, 0), (1, 64, 4, 4), (64, 1, 8, 0), (64, 64, 128, 8), (16, 24, 1024, 0)):
        if _device_present():
            src = torch.zeros(1 + g_in * g_in, d + pad, device="cuda:0")
            dst = torch.zeros(1 + g_out * g_out, d + pad, device="cuda:0")
            ps, pd = src.data_ptr(), dst.data_ptr()
        else:
            ps, pd = A, A2
        for filt in (0, 1):
            for aa in (0, 1):
                n0 = _lib.launch_count()
                rc = _lib.load().lpi_pos_embed_resample(g_in, g_out, d, ps, d + pad, pd, d + pad, filt, aa, None)
                assert _lib.launch_count() - n0 == 1, (g_in, g_out, d, filt, aa)
                assert rc == 0 if _device_present() else rc > 0, (g_in, g_out, d, filt, aa, rc)
        if _device_present():
            torch.cuda.synchronize()
    # adjacent tables do not overlap
    if not _device_present():
        n0 = _lib.launch_count()
        assert _resample(dst=A + (7 * 7 * 128 + 128) * 4) > 0 and _lib.launch_count() - n0 == 1


def _kp(ps, dt):
    K, bk = 3 * ps * ps, 32 if dt == _lib.F32 else 64
    return (K + bk - 1) // bk * bk


def _patchify_u8(dt=_lib.F32, B=2, R=28, ps=14, image=A, lut=A2, cols=A3, ld=None):
    return _lib.load().lpi_patchify_u8(dt, B, R, ps, image, lut, cols, _kp(ps, dt) if ld is None else ld, None)


def test_patchify_u8_keeps_its_refusals_at_every_geometry():
    before = _lib.launch_count()
    for R, ps in ((28, 14), (42, 14), (32, 16)):
        kp = _kp(ps, _lib.F32)
        for kw in (dict(R=R + 1), dict(R=R - 1), dict(ps=0), dict(ps=-ps), dict(B=0), dict(B=-1), dict(image=None), dict(lut=None), dict(cols=None),
                   dict(ld=kp - 4), dict(ld=kp + 2), dict(ld=0), dict(cols=A3 + 4), dict(dt=-1), dict(dt=_lib.F32X3)):
            assert _patchify_u8(**dict(dict(R=R, ps=ps), **kw)) == EINVAL, (R, ps, kw)
    for dt in (_lib.BF16, _lib.F16):
        assert _patchify_u8(dt=dt, ld=_kp(14, dt) - 4) == EINVAL and _patchify_u8(dt=dt, cols=A3 + 2) == EINVAL
    # the dword kernel's geometries (ps and R multiples of 4) keep its rule on the image pointer
    for off in (1, 2, 3):
        assert _patchify_u8(R=32, ps=16, image=A + off) == EINVAL, off
    assert _lib.launch_count() == before


def test_patchify_u8_takes_patch_14():
    """(R, ps) = (28, 14) and (42, 14), refused before (LPI_EINVAL: ps and R had to be multiples of 4), are launched — with any image pointer."""
    lib = _lib.load()
    for R, ps in ((28, 14), (42, 14), (30, 6), (35, 7)):
        for dt, td in ((_lib.F32, torch.float32), (_lib.BF16, torch.bfloat16), (_lib.F16, torch.float16)):
            for off in (0, 1):
                B, G, kp = 2, R // ps, _kp(ps, dt)
                if _device_present():
                    img = torch.zeros(B * 3 * R * R + 1, dtype=torch.uint8, device="cuda:0")
                    lut, cols = torch.zeros(768, device="cuda:0"), torch.zeros(B * G * G, kp, dtype=td, device="cuda:0")
                    pi, pl, pc = img.data_ptr() + off, lut.data_ptr(), cols.data_ptr()
                else:
                    pi, pl, pc = A + off, A2, A3
                n0 = _lib.launch_count()
                rc = lib.lpi_patchify_u8(dt, B, R, ps, pi, pl, pc, kp, None)
                assert rc != EINVAL and _lib.launch_count() - n0 == 1, (R, ps, dt, off, rc)
                assert rc == 0 if _device_present() else rc > 0, (R, ps, dt, off, rc)
                if _device_present():
                    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------------------------------------- config and options
def test_at_resolution():
    c = synth.TINY.at_resolution(48)
    assert c.image_resolution == 48 and c.n_patches == 9 and c.name == "tiny"
    assert c == synth.ClipConfig("tiny", 128, 48, 2, 128, 16, 77, 49408, 128, 2, 2)
    assert synth.TINY.at_resolution(32) == synth.TINY and synth.TINY.image_resolution == 32
    h = synth.VIT_H14.at_resolution(378)
    assert h.n_patches == 729 and h.vision_head_width == 80 and h.as_clip_args()[1] == 378
    assert synth.VIT_L14.at_resolution(336) == synth.ClipConfig("ViT-L/14", 768, 336, 24, 1024, 14, 77, 49408, 768, 12, 12)
    for bad in (0, -16, 40, 33, 16.0, "48", None, True):
        with pytest.raises(ValueError, match="multiple of the patch size"):
            synth.TINY.at_resolution(bad)


def test_engine_option_pos_embed():
    from lpi_amd.engine import EngineOptions
    assert EngineOptions().pos_embed is None
    for m in ("bicubic", "bicubic_aa", "bilinear"):
        assert EngineOptions(pos_embed=m).pos_embed == m
        assert EngineOptions.from_env(pos_embed=m).pos_embed == m
    for bad in ("nearest", "", "BICUBIC", 1, True, ("bicubic",)):
        with pytest.raises(ValueError, match="pos_embed"):
            EngineOptions(pos_embed=bad)


def test_engine_refuses_another_grid_before_the_gpu():
    """A table of another grid with pos_embed=None, and a table that is no 1 + g * g rows: ValueError before the device is looked at (device 'cpu' would be the
    next refusal) and before any launch."""
    from lpi_amd.engine import DualEncoder, EngineOptions
    sd = synth.clip_state_dict(synth.TINY)
    before = _lib.launch_count()
    with pytest.raises(ValueError, match=r"2 x 2.*3 x 3"):
        DualEncoder(synth.TINY.at_resolution(48), sd, device="cpu", options=EngineOptions())
    bad = dict(sd)
    bad["visual.positional_embedding"] = sd["visual.positional_embedding"][:4]
    for opt in (EngineOptions(), EngineOptions(pos_embed="bicubic_aa")):
        with pytest.raises(ValueError, match="4 rows"):
            DualEncoder(synth.TINY, bad, device="cpu", options=opt)
    assert _lib.launch_count() == before


# ---------------------------------------------------------------------------------------------------------------------------------- plugin
def _shipped():
    return json.load(open(os.path.join(REPO, "lpi_amd", "retrieval", "configs", "lpi", "coco_lpi.json")))


def _args(**over):
    args = _shipped()
    args.update(device=[torch.device("cpu")], backbonename="tiny", visual_dim=128, textual_dim=128)
    args.update(over)
    return args


def test_plugin_resolution_keys():
    from lpi_amd.retrieval.models.slinet import SliNet
    net = SliNet(_args(image_resolution=48))
    assert net.clip_cfg.n_patches == 9 and net.clip_cfg == synth.TINY.at_resolution(48) and net.pos_embed == "bicubic_aa"
    assert SliNet(_args(image_resolution=64, pos_embed_interpolation="bilinear")).pos_embed == "bilinear"
    same = SliNet(_args(image_resolution=32, pos_embed_interpolation="bicubic"))
    assert same.clip_cfg == synth.TINY and same.pos_embed is None      # the checkpoint's own resolution: nothing to resample
    # the module state keeps the checkpoint's table: 1 + 2 * 2 rows
    assert tuple(net.clip_model.state_dict()["visual.positional_embedding"].shape) == (5, 128)
    # a state dict under an unknown name: the resolution comes from its table, the key moves it
    sd = synth.clip_state_dict(synth.TINY)
    assert SliNet(_args(clip_state_dict=sd, backbonename="mine", image_resolution=80)).clip_cfg.n_patches == 25


def test_plugin_refuses_at_construction():
    from lpi_amd.retrieval.models.slinet import SliNet
    P = _shipped()["prompt_length"]
    for bad in (40, 33, 0, -16):
        with pytest.raises(ValueError, match="multiple of the patch size"):
            SliNet(_args(image_resolution=bad))
    for bad in (48.0, "48", True, [48], None):
        with pytest.raises(ValueError, match="image_resolution must be an integer"):
            SliNet(_args(image_resolution=bad))
    # 1 + prompt_length + g * g <= 1024
    g = 1
    while 1 + P + (g + 1) ** 2 <= 1024:
        g += 1
    assert SliNet(_args(image_resolution=16 * g)).clip_cfg.n_patches == g * g
    with pytest.raises(ValueError, match="limit is 1024"):
        SliNet(_args(image_resolution=16 * (g + 1)))
    for bad in ("nearest", "bicubic-aa", "", 3, True, ["bicubic"]):
        with pytest.raises(ValueError, match="pos_embed_interpolation"):
            SliNet(_args(image_resolution=48, pos_embed_interpolation=bad))
        with pytest.raises(ValueError, match="pos_embed_interpolation"):
            SliNet(_args(pos_embed_interpolation=bad))
    with pytest.raises(ValueError, match="must agree"):
        SliNet(_args(image_resolution=48, pos_embed_interpolation="bilinear", engine_options={"pos_embed": "bicubic"}))
    # the refusals that were there stay
    with pytest.raises(ValueError, match="visual_dim"):
        SliNet(_args(image_resolution=48, visual_dim=256))
    with pytest.raises(ValueError, match="activation"):
        SliNet(_args(image_resolution=48, activation="relu"))


def test_without_the_keys_nothing_changes():
    from lpi_amd.retrieval.models.slinet import SliNet
    from lpi_amd.retrieval.utils.data import preprocess_options
    shipped = _shipped()
    assert "image_resolution" not in shipped and "pos_embed_interpolation" not in shipped
    assert preprocess_options(shipped) is None
    assert preprocess_options(_args()) is None
    net = SliNet(_args())
    assert net.clip_cfg == synth.TINY and net.clip_cfg is synth.CONFIGS["tiny"] and net.pos_embed is None
    assert SliNet(_args(backbonename="tiny14", visual_dim=256)).clip_cfg is synth.TINY14
    assert synth.CONFIGS[shipped["backbonename"]].image_resolution == 224
    ref = {"interpolation": "bilinear", "normalize": "imagenet", "eval_resize": 256, "size": 224}
    assert preprocess_options(dict(shipped, preprocess="reference")) == ref
    assert preprocess_options(dict(shipped, preprocess="reference"), 336) == ref
    assert preprocess_options(dict(shipped, preprocess="clip"), 336) == {"interpolation": "bicubic", "normalize": "clip", "eval_resize": 336, "size": 336}
    assert preprocess_options(dict(shipped, eval_resize=300)) == dict(ref, eval_resize=300)


def test_preprocess_follows_the_resolution_key():
    from lpi_amd.retrieval.utils.data import preprocess_options
    shipped = _shipped()
    ref = {"interpolation": "bilinear", "normalize": "imagenet"}
    assert preprocess_options(dict(shipped, image_resolution=336), 336) == dict(ref, size=336, eval_resize=384)
    assert preprocess_options(dict(shipped, image_resolution=384, preprocess="reference"), 384) == dict(ref, size=384, eval_resize=439)
    assert preprocess_options(dict(shipped, image_resolution=224), 224) == dict(ref, size=224, eval_resize=256)
    assert preprocess_options(dict(shipped, image_resolution=336, eval_resize=400), 336) == dict(ref, size=336, eval_resize=400)
    with pytest.raises(ValueError, match="smaller than"):
        preprocess_options(dict(shipped, image_resolution=336, eval_resize=256), 336)
    assert preprocess_options(dict(shipped, image_resolution=336, preprocess="clip"), 336) == {"interpolation": "bicubic", "normalize": "clip", "eval_resize": 336,
                                                                                                "size": 336}
