"""The vision front end at patch 14 and at other input resolutions on a real MI355X: lpi_patchify_u8 at geometries whose patch size or resolution is no
multiple of 4 (bit for bit lpi_patchify on the host-normalised image), the engine and the plugin loop on uint8 pixels at patch 14, lpi_pos_embed_resample against
torch.nn.functional.interpolate in float64, the engine at another resolution than its position table's against the oracle, and the plugin's image_resolution key."""
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from lpi_amd import _lib, synth  # noqa: E402
from lpi_amd._lib import BF16, F16, F32, call  # noqa: E402

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RET = os.path.join(REPO, "lpi_amd", "retrieval")
DEV = torch.device("cuda:0")
TD = {F32: torch.float32, BF16: torch.bfloat16, F16: torch.float16}
GRADS = ["grad." + n for n in synth.PROMPT_NAMES]
_WEIGHTS = {}


def weights(cfg):
    if cfg.name not in _WEIGHTS:
        _WEIGHTS[cfg.name] = synth.clip_state_dict(cfg)
    return _WEIGHTS[cfg.name]


def stream():
    return torch.cuda.current_stream().cuda_stream


def bits(t):
    return t.view(torch.int32 if t.element_size() == 4 else torch.int16)


def plugin_args(**over):
    args = json.load(open(os.path.join(RET, "configs", "lpi", "coco_lpi.json")))
    args.update(backbonename="tiny", visual_dim=128, textual_dim=128, device=[DEV], compute_dtype="f32", batch_size=4, epochs=1, num_workers=0)
    args.update(over)
    return args


def set_factors(net, dv, dt):
    for t in range(len(net.prompts)):
        for k, v in synth.prompt_factors(9, 16, dv, dt, task=t).items():
            getattr(net.prompts[t], k).data = torch.from_numpy(v.copy()).to(DEV)


# ---------------------------------------------------------------------------------------------------------------------------------- 1. u8 columns
def _columns(R, ps, dt, off, B=3):
    """(lpi_patchify on the host-normalised image, lpi_patchify_u8 on the bytes `off` bytes into their buffer, launches of the latter)"""
    from lpi_amd.engine import make_pixel_lut
    from lpi_amd.retrieval.utils.data import normalise_u8
    g = torch.Generator().manual_seed(R * 100 + ps)
    u8 = torch.randint(0, 256, (B, 3, R, R), generator=g, dtype=torch.uint8)
    buf = torch.zeros(u8.numel() + 16, dtype=torch.uint8, device=DEV)
    buf[off:off + u8.numel()] = u8.reshape(-1).to(DEV)
    img = buf[off:off + u8.numel()].view(B, 3, R, R)
    assert img.data_ptr() % 16 == off
    G, K, bk = R // ps, 3 * ps * ps, 128 // TD[dt].itemsize
    kp = (K + bk - 1) // bk * bk
    c0 = torch.zeros(B * G * G, kp, dtype=TD[dt], device=DEV)
    c1 = torch.full((B * G * G, kp), 7.0, dtype=TD[dt], device=DEV)      # a missed pad column shows
    call("lpi_patchify", dt, B, R, ps, normalise_u8(u8).to(DEV), c0, kp, stream())
    n0 = _lib.launch_count()
    call("lpi_patchify_u8", dt, B, R, ps, img, make_pixel_lut().to(DEV), c1, kp, stream())
    n = _lib.launch_count() - n0
    torch.cuda.synchronize()
    if K < kp:
        assert not bits(c0[:, K:]).any()
    return c0, c1, n


@pytest.mark.parametrize("R,ps", [(28, 14), (42, 14), (14, 14), (35, 7), (30, 6)])
def test_u8_columns_at_any_patch_size(R, ps):
    """Geometries the dword kernel cannot take, three images (more than one block at (42, 14)): the columns of lpi_patchify_u8 equal lpi_patchify's on
    normalise_u8(u8) as integers in f32, bf16 and f16, the pad columns K .. Kp are zero — and the same from an image pointer one byte off."""
    for dt in (F32, BF16, F16):
        for off in ((0, 1) if dt == BF16 else (0,)):
            c0, c1, n = _columns(R, ps, dt, off)
            assert n == 1
            assert torch.equal(bits(c0), bits(c1)), (R, ps, dt, off)


@pytest.mark.parametrize("R,ps,dts", [(32, 16, (F32, BF16, F16)), (224, 16, (BF16,))])
def test_u8_columns_of_the_dword_geometries_are_unchanged(R, ps, dts):
    """ps and R multiples of 4: one launch and the same bits as ever (tests/test_round5_gpu.py holds the same cases)."""
    for dt in dts:
        c0, c1, n = _columns(R, ps, dt, 0)
        assert n == 1
        assert torch.equal(bits(c0), bits(c1)), (R, ps, dt)


# ---------------------------------------------------------------------------------------------------------------------------------- 2. u8 engine and plugin
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_tiny14_features_from_uint8_pixels(dtype):
    from lpi_amd.engine import DualEncoder
    from lpi_amd.retrieval.utils.data import normalise_u8
    cfg = synth.TINY14
    enc = DualEncoder(cfg, weights(cfg), dtype=dtype, device=DEV)
    u8 = torch.randint(0, 256, (5, 3, 28, 28), generator=torch.Generator().manual_seed(14), dtype=torch.uint8)
    with torch.no_grad():
        fa = enc.encode_image(u8.to(DEV)).clone()
        fb = enc.encode_image(normalise_u8(u8).to(DEV)).clone()
    assert torch.isfinite(fa).all() and torch.equal(fa, fb)


def _train_tiny14(loader, epochs=2, **over):
    from lpi_amd.retrieval.methods.sprompt import SPrompts
    m = SPrompts(plugin_args(backbonename="tiny14", visual_dim=256, epochs=epochs, **over))
    net = m._network.to(DEV)
    set_factors(net, 256, 128)
    net.numtask = 1
    opt, sch = m._setup_training()
    for ep in range(epochs):
        m.train_epoch(loader, opt, ep)
        sch.step()
    torch.cuda.synchronize()
    return m, {k: getattr(net.prompts[0], k).detach().clone() for k in synth.PROMPT_NAMES}


def test_tiny14_plugin_loop_on_uint8_pixels():
    """SPrompts on tiny14 (patch 14: LpiError on the first batch before) trains to the same parameters with pixel_format 'u8' as with 'f32' on the same pixels:
    the arm tests/test_round5_gpu.py runs for tiny."""
    from lpi_amd.retrieval.utils.data import normalise_u8
    g = torch.Generator().manual_seed(15)
    ids = torch.from_numpy(synth.token_ids(8, seed=5))
    px = torch.randint(0, 256, (8, 3, 28, 28), generator=g, dtype=torch.uint8)
    got = []
    for fmt in ("u8", "f32"):
        im = px if fmt == "u8" else normalise_u8(px)
        loader = [(im[:4], ids[:4], 0, 0), ([im[j] for j in range(4, 8)], ids[4:], 0, 0)]
        m, params = _train_tiny14(loader)
        got.append(params)
        if fmt == "u8":
            assert m._pipeline._stage[0].dtype == torch.uint8 and m._pipeline._dev[0].dtype == torch.uint8
    start = synth.prompt_factors(9, 16, 256, 128, task=0)
    assert any(not np.array_equal(got[0][k].cpu().numpy(), start[k]) for k in synth.PROMPT_NAMES), "the loop trained nothing"
    for k in synth.PROMPT_NAMES:
        assert torch.equal(got[0][k], got[1][k]), k


def test_tiny14_two_steps_on_decoded_pixels():
    """pixel_format 'decoded' (crop / resize / flip on the GPU, then lpi_patchify_u8) at patch 14: two steps on DecodedBatches against two steps on the uint8
    pixels the same batches decode to."""
    from lpi_amd import imageops
    from lpi_amd.retrieval.utils import data as D
    torch.manual_seed(16)
    ds = D.SyntheticCoco(8, [0], 28, seed=3, pixel_format="decoded")
    items = [ds[i] for i in range(8)]      # the crop draws happen here, once
    dec = [D.collate_decoded(items[j:j + 4]) for j in (0, 4)]
    assert all(isinstance(b[0], D.DecodedBatch) for b in dec)
    u8 = [[imageops.resample_decoded(b[0], device=DEV).cpu()] + list(b[1:]) for b in dec]
    assert u8[0][0].dtype == torch.uint8 and tuple(u8[0][0].shape) == (4, 3, 28, 28)
    _, a = _train_tiny14(u8, epochs=1)
    _, b = _train_tiny14(dec, epochs=1)
    for k in synth.PROMPT_NAMES:
        assert torch.equal(a[k], b[k]), k


# ---------------------------------------------------------------------------------------------------------------------------------- 3. the resample kernel
MODES = [("bicubic", 0, 0), ("bicubic", 0, 1), ("bilinear", 1, 0), ("bilinear", 1, 1)]      # torch's mode, filter, antialias


def torch_resize(x, g_in, g_out, mode, antialias, dtype):
    """[1 + g_in^2, d] -> [1 + g_out^2, d] in `dtype` on the CPU: the recipe of OpenCLIP's and timm's resize_pos_embed."""
    t = x.to(dtype)
    grid = t[1:].reshape(1, g_in, g_in, -1).permute(0, 3, 1, 2)
    out = F.interpolate(grid, size=(g_out, g_out), mode=mode, align_corners=False, antialias=bool(antialias))
    return torch.cat([t[:1], out.permute(0, 2, 3, 1).reshape(g_out * g_out, -1)])


def kernel_resize(x, g_in, g_out, filt, aa, pad=0, fill=0.0):
    d = x.shape[1]
    src = torch.full((x.shape[0], d + pad), 3.0, device=DEV)
    src[:, :d] = x.to(DEV)
    dst = torch.full((1 + g_out * g_out, d + pad), fill, device=DEV)
    n0 = _lib.launch_count()
    call("lpi_pos_embed_resample", g_in, g_out, d, src, src.stride(0), dst, dst.stride(0), filt, aa, stream())
    assert _lib.launch_count() - n0 == 1
    torch.cuda.synchronize()
    return dst.cpu()


def hold_resample(x, g_in, g_out, label):
    amax = float(x.abs().max())
    for mode, filt, aa in MODES:
        r64 = torch_resize(x, g_in, g_out, mode, aa, torch.float64)
        e32 = float((torch_resize(x, g_in, g_out, mode, aa, torch.float32).double() - r64).abs().max())
        got = kernel_resize(x, g_in, g_out, filt, aa)
        err = float((got.double() - r64).abs().max())
        bar = max(2 * e32, 4 * 2.0 ** -24 * amax)
        print(f"POS_EMBED {label} {g_in}->{g_out} {mode}{' aa' if aa else ''}: kernel err {err:.3e}  torch f32 err {e32:.3e}  bar {bar:.3e}  "
              f"(2^-24 max|x| = {2.0 ** -24 * amax:.3e})")
        assert torch.equal(bits(got[0]), bits(x[0])), (mode, aa, "row 0 is a copy")
        assert err <= bar, (g_in, g_out, mode, aa, err, bar)
        if g_in == g_out:
            assert torch.equal(bits(got), bits(x)), (mode, aa, "equal grids are a copy")
        # padded leading dimensions: the same bits, and the pad columns of dst untouched
        padded = kernel_resize(x, g_in, g_out, filt, aa, pad=8, fill=7.0)
        assert torch.equal(bits(padded[:, :x.shape[1]]), bits(got)), (mode, aa, "lds / ldd = d + 8")
        assert torch.equal(padded[:, x.shape[1]:], torch.full((padded.shape[0], 8), 7.0)), (mode, aa, "pad columns of dst")


@pytest.mark.parametrize("g_in,g_out", [(2, 3), (3, 2), (2, 24), (7, 12), (16, 31), (20, 10), (16, 7), (14, 14)])
def test_pos_embed_resample_against_torch(g_in, g_out):
    """Bar per case: max(2 e32, 4 * 2^-24 max|x|) with e32 = max |torch f32 - torch f64| of that very case — torch's own single-precision error on the same
    grid, and the kernel gets twice it.  (The kernel sums in float64 and rounds once: half an ulp of the result.)"""
    g = torch.Generator().manual_seed(1000 * g_in + g_out)
    x = 0.05 * torch.randn(1 + g_in * g_in, 128, generator=g)
    hold_resample(x, g_in, g_out, "randn")


def test_pos_embed_resample_with_outliers():
    g = torch.Generator().manual_seed(7)
    x = 0.05 * torch.randn(1 + 49, 128, generator=g)
    x[1 + 3 * 7 + 2] = 1e4 * (2.0 * torch.randint(0, 2, (128,), generator=g) - 1.0)      # one grid row of +-1e4
    hold_resample(x, 7, 12, "outliers")
    hold_resample(x, 7, 4, "outliers")


# ---------------------------------------------------------------------------------------------------------------------------------- 4. the engine at another resolution
TORCH_MODE = {"bicubic": ("bicubic", 0), "bicubic_aa": ("bicubic", 1), "bilinear": ("bilinear", 0)}


def resized_weights(cfg, r, mode):
    """(cfg at r, the state dict with the table torch resized in float64, cast to f32)"""
    sd = dict(weights(cfg))
    new = cfg.at_resolution(r)
    g_in, g_out = cfg.image_resolution // cfg.vision_patch_size, r // cfg.vision_patch_size
    tab = torch.as_tensor(np.asarray(sd["visual.positional_embedding"])).float()
    tmode, aa = TORCH_MODE[mode]
    out = torch_resize(tab, g_in, g_out, tmode, aa, torch.float64).float()
    sd["visual.positional_embedding"] = out if torch.is_tensor(weights(cfg)["visual.positional_embedding"]) else out.numpy()
    return new, sd


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


def run_engine(cfg, sd, dtype, mode, img, ids, fac_np, depth):
    from lpi_amd.engine import DualEncoder, EngineOptions
    from lpi_amd.step import train_step
    n0 = _lib.launch_count()
    enc = DualEncoder(cfg, sd, dtype=dtype, device=DEV, options=EngineOptions(pos_embed=mode))
    built = _lib.launch_count() - n0
    fac = {k: torch.from_numpy(v).to(DEV).requires_grad_(True) for k, v in fac_np.items()}
    out = train_step(enc, img.to(DEV), torch.from_numpy(ids).to(DEV), fac, depth)
    torch.cuda.synchronize()
    res = {k: v.cpu().numpy() for k, v in out.items()}
    res["logits"] = (enc.logit_scale_exp * out["img_f"] @ out["txt_f"].t()).cpu().numpy()
    for k in synth.PROMPT_NAMES:
        res["grad." + k] = fac[k].grad.cpu().numpy()
    return enc, res, built


@pytest.mark.parametrize("name,r,mode,u8", [("tiny", 48, "bicubic_aa", False), ("tiny", 64, "bilinear", False), ("tiny14", 42, "bicubic_aa", True),
                                            ("tinyLong", 40, "bicubic_aa", False), ("tiny", 384, "bicubic", False)])
def test_engine_at_another_resolution_against_the_oracle(name, r, mode, u8):
    """cfg' = cfg.at_resolution(r), 2 pairs, depth 2: the oracle in f32 on a state dict whose table torch resized (float64, cast to f32) against the engine that
    was handed the ORIGINAL state dict and EngineOptions(pos_embed=mode), on one train_step.  The project's bars, unchanged: f32 features 2e-5 and gradients 2e-4
    relative; bf16 features < 2e-2, gradient cosine > 0.99.  tiny14 runs on uint8 pixels (the general lpi_patchify_u8 kernel and the resampled table together);
    tiny at 384 has 1 + 16 + 576 = 593 vision tokens (csrc/attn_long.hip)."""
    from oracle import lpi_oracle as O
    from lpi_amd.retrieval.utils.data import normalise_u8
    cfg = synth.CONFIGS[name]
    new, sd_resized = resized_weights(cfg, r, mode)
    depth, batch = 2, 2
    fac_np = synth.prompt_factors(9, 16, cfg.vision_width, cfg.transformer_width, r=4)
    ids = synth.token_ids(batch)
    if u8:
        px = torch.randint(0, 256, (batch, 3, r, r), generator=torch.Generator().manual_seed(r), dtype=torch.uint8)
        img_ref, img = normalise_u8(px).numpy(), px
    else:
        img_ref = synth.images(batch, r)
        img = torch.from_numpy(img_ref)
    ref = O.train_step(O.Oracle(new, sd_resized), img_ref, ids, fac_np, depth=depth)
    enc, res, built = run_engine(new, weights(cfg), "f32", mode, img, ids, fac_np, depth)
    assert tuple(enc.vpos.shape) == (1 + new.n_patches, cfg.vision_width)
    tab_err = maxerr(enc.vpos.cpu().numpy(), np.asarray(sd_resized["visual.positional_embedding"]))
    print(f"FRONT {name} {cfg.image_resolution}->{r} {mode} f32: table {tab_err:.3e}  " + "  ".join(f"{k} {maxerr(res[k], ref[k]):.3e}" for k in ("img_f", "txt_f", "logits"))
          + "  worst grad err / scale " + f"{max(maxerr(res[k], ref[k]) / np.abs(ref[k]).max() for k in GRADS):.3e}")
    check(res, ref, tol=2e-5, gtol=2e-4)
    _, r16, _ = run_engine(new, weights(cfg), "bf16", mode, img, ids, fac_np, depth)
    print(f"FRONT {name} {cfg.image_resolution}->{r} {mode} bf16: " + "  ".join(f"{k} {maxerr(r16[k], ref[k]):.3e}" for k in ("img_f", "txt_f"))
          + "  min cosine " + f"{min(cos(r16[k], ref[k]) for k in GRADS):.5f}")
    for k in ("img_f", "txt_f"):
        assert maxerr(r16[k], ref[k]) < 2e-2, (k, maxerr(r16[k], ref[k]))
    for k in GRADS:
        assert cos(r16[k], ref[k]) > 0.99, (k, cos(r16[k], ref[k]))


def test_same_resolution_is_untouched_and_a_mismatch_is_refused():
    """The table's own grid: any pos_embed gives the bits and the construction-time launch count of pos_embed=None, and vpos is the table as it came.  Another
    grid with pos_embed=None: ValueError naming both grids, and no launch."""
    from lpi_amd.engine import DualEncoder, EngineOptions
    cfg = synth.TINY
    sd = weights(cfg)
    img = torch.from_numpy(synth.images(3, cfg.image_resolution)).to(DEV)
    feats, built = [], []
    for mode in (None, "bicubic", "bicubic_aa", "bilinear"):
        n0 = _lib.launch_count()
        enc = DualEncoder(cfg, sd, dtype="f32", device=DEV, options=EngineOptions(pos_embed=mode))
        torch.cuda.synchronize()
        built.append(_lib.launch_count() - n0)
        assert np.array_equal(enc.vpos.cpu().numpy(), np.asarray(sd["visual.positional_embedding"], dtype=np.float32))
        with torch.no_grad():
            feats.append(enc.encode_image(img).clone())
    assert built == [built[0]] * 4, built
    assert all(torch.equal(feats[0], f) for f in feats[1:])
    n0 = _lib.launch_count()
    with pytest.raises(ValueError, match=r"2 x 2.*3 x 3"):
        DualEncoder(cfg.at_resolution(48), sd, dtype="f32", device=DEV, options=EngineOptions())
    with pytest.raises(ValueError, match=r"2 x 2.*1 x 1"):      # a table longer than the config needs: was read silently wrong
        DualEncoder(cfg.at_resolution(16), sd, dtype="f32", device=DEV)
    assert _lib.launch_count() == n0


# ---------------------------------------------------------------------------------------------------------------------------------- 5. the plugin
def test_plugin_at_another_resolution():
    """backbonename tiny with image_resolution 48 on the synthetic datasets (which follow clip_cfg.image_resolution): one epoch trains, and extract_vector on 48 px
    images equals a DualEncoder built by hand with at_resolution(48) and pos_embed='bicubic_aa', bit for bit."""
    from torch.utils.data import DataLoader
    from lpi_amd.engine import DualEncoder, EngineOptions
    from lpi_amd.retrieval.methods.sprompt import SPrompts
    from lpi_amd.retrieval.utils.data import collate_keep_images
    m = SPrompts(plugin_args(image_resolution=48, dataset_impl="synthetic", synthetic_train_size=8))
    net = m._network.to(DEV)
    assert net.clip_cfg.n_patches == 9 and net.engine.opt.pos_embed == "bicubic_aa" and tuple(net.engine.vpos.shape) == (10, 128)
    set_factors(net, 128, 128)
    net.numtask = 1
    m._cur_task, m.cur_id = [0], 0
    train, _ = m._datasets(0)
    assert tuple(train[0][0].shape) == (3, 48, 48)
    opt, _ = m._setup_training()
    before = {k: getattr(net.prompts[0], k).detach().clone() for k in synth.PROMPT_NAMES}
    steps = []
    m.train_epoch(DataLoader(train, batch_size=4, shuffle=False, num_workers=0, collate_fn=collate_keep_images), opt, 0, None,
                  lambda i, b, out: steps.append(tuple(b.images.shape)) and False)
    torch.cuda.synchronize()
    assert steps == [(4, 3, 48, 48)] * 2
    assert any(not torch.equal(before[k], getattr(net.prompts[0], k).detach()) for k in synth.PROMPT_NAMES)
    img = torch.from_numpy(synth.images(5, 48)).to(DEV)
    with torch.no_grad():
        got = net.extract_vector(img).clone()
    hand = DualEncoder(synth.TINY.at_resolution(48), weights(synth.TINY), dtype="f32", device=DEV, options=EngineOptions.from_env(pos_embed="bicubic_aa"))
    with torch.no_grad():
        want = hand.encode_image(img).clone()
    assert torch.isfinite(got).all() and torch.equal(got, want)
    assert tuple(net.state_dict()["clip_model.visual.positional_embedding"].shape) == (5, 128)      # the module state keeps the checkpoint's table
