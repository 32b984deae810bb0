"""The resampling filters of the decoded pixel formats, host side: the numpy restatement of Pillow's filtered resample (tests/pil_resample_filters.py,
the yardstick of lpi_image_resample_u8_f) against Pillow itself for BICUBIC and BOX, byte for byte; the signed-tap sums against int32; the
datasets under CLIP's own preprocessing against Pillow calls spelled out; the filter on items and batches; CLIP's normalisation table.  CPU only."""
import ctypes
import io
import json
import pickle
import types

import numpy as np
import pytest
import torch

PIL = pytest.importorskip("PIL")
from PIL import Image  # noqa: E402

import pil_resample as R  # noqa: E402
import pil_resample_filters as F  # noqa: E402
from lpi_amd import _lib, imageops  # noqa: E402
from lpi_amd.retrieval.utils import data as D  # noqa: E402

PIL_FILTER = {"bilinear": Image.BILINEAR, "bicubic": Image.BICUBIC, "box": Image.BOX}
NEW = ("bicubic", "box")


def resize_cases(n, seed):
    """(w, h, ow, oh): random sizes, 1-px sources and outputs, 20x+ downscales, 8x+ upscales, extreme aspect ratios (the generator of
    tests/test_image_decoded_host.py)."""
    rng = np.random.default_rng(seed)
    fixed = [(1, 1, 7, 5), (1, 40, 224, 224), (37, 1, 224, 3), (4480, 30, 224, 30), (30, 4600, 29, 224), (28, 28, 224, 224), (13, 17, 120, 140),
             (2000, 12, 50, 300), (12, 2000, 300, 50), (640, 480, 1, 1), (5000, 8, 224, 224), (224, 224, 224, 224), (3, 2, 2, 3),
             (10, 3071, 11, 180), (2, 225, 219, 191), (13, 1300, 74, 184), (20, 2202, 50, 21), (300, 31000, 256, 224)]
    out = list(fixed)
    while len(out) < n:
        w, h = (int(v) for v in rng.integers(1, 700, 2))
        ow, oh = (int(v) for v in rng.integers(1, 700, 2))
        out.append((w, h, ow, oh))
    return out


def checkerboard(w, h, cell):
    """0 / 255 squares of `cell` pixels, the three channels in different phases: bicubic overshoots below 0 and above 255 at every edge."""
    y, x = np.mgrid[0:h, 0:w]
    return np.stack([(((x // cell) + (y // cell) + c) % 2) * 255 for c in range(3)], axis=2).astype(np.uint8)


def test_constants_are_pillows():
    assert (F.BILINEAR, F.BICUBIC, F.BOX) == (int(Image.BILINEAR), int(Image.BICUBIC), int(Image.BOX)) == (2, 3, 4)
    assert imageops.FILTERS == F.NAMES and set(D.INTERPOLATIONS) == set(F.NAMES)


@pytest.mark.parametrize("name", NEW)
def test_restatement_equals_pillow_on_random_bytes(name):
    rng = np.random.default_rng(1)
    cases = resize_cases(110, 2)
    assert len(cases) == 110
    assert any(w >= 20 * ow for w, h, ow, oh in cases) and any(ow >= 8 * w for w, h, ow, oh in cases)
    assert any(w == 1 or h == 1 for w, h, ow, oh in cases) and any(ow == 1 and oh == 1 for w, h, ow, oh in cases)
    assert any(h > 100 * w for w, h, ow, oh in cases) and any(R.vertical_first(w, h, oh) for w, h, ow, oh in cases)
    for w, h, ow, oh in cases:
        src = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
        ref = np.asarray(Image.fromarray(src).resize((ow, oh), PIL_FILTER[name]))
        assert np.array_equal(F.resize(F.NAMES[name], src, ow, oh), ref), (name, w, h, ow, oh)


@pytest.mark.parametrize("name", NEW)
def test_restatement_equals_pillow_on_checkerboards(name):
    """0 / 255 checkerboards over the whole size list: bicubic's negative taps drive sums below 0 and above 255 * 2^22, so both clamps of the
    intermediate and of the output are live (asserted for bicubic: the unclamped restatement differs)."""
    clamps = 0
    for i, (w, h, ow, oh) in enumerate(resize_cases(110, 2)):
        src = checkerboard(w, h, 1 + i % 3)
        ref = np.asarray(Image.fromarray(src).resize((ow, oh), PIL_FILTER[name]))
        got = F.resize(F.NAMES[name], src, ow, oh)
        assert np.array_equal(got, ref), (name, w, h, ow, oh)
        if name == "bicubic" and ow > w and w > 3 and not R.vertical_first(w, h, oh):
            xmin, k = F.coeffs(F.BICUBIC, w, ow)
            row = src[0, :, 0].astype(np.int64)
            s = (1 << 21) + sum(row[np.minimum(xmin + t, w - 1)] * k[:, t] for t in range(k.shape[1]))
            clamps += int((s < 0).any()) + int(((s >> 22) > 255).any())
    assert name != "bicubic" or clamps > 20


def test_bilinear_restatement_equals_the_bilinear_only_one():
    rng = np.random.default_rng(7)
    for w, h, ow, oh in resize_cases(60, 2):
        src = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
        assert np.array_equal(F.resize(F.BILINEAR, src, ow, oh), R.resize(src, ow, oh)), (w, h, ow, oh)
        xa, ka = F.coeffs(F.BILINEAR, w, ow)
        xb, kb = R.coeffs(w, ow)
        assert np.array_equal(xa, xb) and np.array_equal(ka, kb)


@pytest.mark.parametrize("name", ("bilinear",) + NEW)
def test_every_partial_sum_fits_int32(name):
    """csrc/imageops.hip, "Signed taps": with T = sum |tap| of an output position, every partial sum over any subset of its taps lies within
    2^21 + 255 * T of zero, so any chunking of the vertical accumulation stays inside int32 while 255 * T + 2^21 < 2^31.  Asserted here for every
    position (clamped edges included) of every in, out <= 64 pair, of dense ratio sweeps at larger sizes and of the size list."""
    f = F.NAMES[name]
    worst = 0
    pairs = [(i, o) for i in range(1, 65) for o in range(1, 65)]
    pairs += [(i, 97) for i in range(97, 400)] + [(1000, o) for o in range(300, 1001, 7)] + [(i, 224) for i in range(1, 2300, 13)]
    pairs += [(w, ow) for w, h, ow, oh in resize_cases(110, 2)] + [(h, oh) for w, h, ow, oh in resize_cases(110, 2)]
    for i, o in pairs:
        k = F.coeffs(f, i, o)[1]
        t = int(np.abs(k).sum(axis=1).max())
        assert 255 * t + (1 << 21) < (1 << 31), (name, i, o, t / (1 << 22))
        if name != "bicubic":                       # no negative taps: 2^22 plus at most half a unit of rounding per tap
            assert t <= (1 << 22) + k.shape[1] // 2 + 1, (name, i, o, t)
        worst = max(worst, t)
    print(f"{name}: largest sum |tap| = {worst / (1 << 22):.4f} * 2^22")
    assert worst >= (1 << 22) - 64                  # the taps of a position sum to 2^22 up to their roundings


@pytest.mark.parametrize("name", NEW)
def test_descriptors_through_pillow_and_the_restatement(name):
    """train_crop_params (crop + flip) and test_crop_params with resize == size (CLIP's Resize(n) + CenterCrop(n): a window of the resized image)
    through Pillow (apply_descriptor(..., interpolation=)) and through the restatement give the transforms' 'u8' bytes, same draws."""
    rng = np.random.default_rng(3)
    f = F.NAMES[name]
    flips = set()
    for i, (w, h) in enumerate([(640, 480), (480, 640), (100, 900), (900, 64), (224, 224), (1, 50), (300, 2), (257, 26000)]):
        a = rng.integers(0, 256, (h, w, 3), dtype=np.uint8) if i % 2 else checkerboard(w, h, 2)
        img = Image.fromarray(a)
        for rep in range(3):
            torch.manual_seed(100 * i + rep)
            want = D.train_transform(img, pixel_format="u8", interpolation=name)
            after = torch.get_rng_state()
            torch.manual_seed(100 * i + rep)
            desc = D.train_crop_params(w, h, 224)
            assert torch.equal(torch.get_rng_state(), after)
            flips.add(desc[8])
            x0, y0, x1, y1 = desc[:4]
            pil = img.crop((x0, y0, x1, y1)).resize((224, 224), PIL_FILTER[name])
            pil = pil.transpose(Image.FLIP_LEFT_RIGHT) if desc[8] else pil
            assert np.array_equal(np.asarray(pil).transpose(2, 0, 1), want.numpy())
            assert torch.equal(D._to_u8_chw(D.apply_descriptor(img, desc, 224, interpolation=name)), want)
            assert np.array_equal(F.apply(f, a, desc, 224), want.numpy())
        for resize in (224, 256):
            want = D.test_transform(img, resize, 224, pixel_format="u8", interpolation=name)
            desc = D.test_crop_params(w, h, resize, 224)
            assert desc[8] == 0 and desc[:4] == (0, 0, w, h) and min(desc[4:6]) == resize
            assert np.array_equal(F.apply(f, a, desc, 224), want.numpy()), (w, h, resize)
    assert flips == {0, 1}


# ------------------------------------------------------------------------------------------------ the datasets
@pytest.fixture(scope="module")
def coco(tmp_path_factory):
    root = tmp_path_factory.mktemp("coco_filters")
    rng = np.random.default_rng(4)
    train, val = [], []
    for i, (w, h) in enumerate([(320, 240), (240, 320), (500, 375), (64, 48), (96, 96), (70, 200)]):
        a = rng.integers(0, 256, size=(h // 8 + 1, w // 8 + 1, 3), dtype=np.uint8)
        Image.fromarray(a).resize((w, h), Image.NEAREST).save(root / f"im{i}.jpg", quality=92)
        train.append({"image": f"im{i}.jpg", "caption": f"a photo of thing {i}", "category": 11, "image_id": f"coco_{i}"})
        val.append({"image": f"im{i}.jpg", "caption": [f"first {i}", f"second {i}"], "category": 11, "image_id": i})
    (root / "train.json").write_text(json.dumps(train))
    (root / "val.json").write_text(json.dumps(val))
    return root


def clip_datasets(coco, pixel_format, n_px, **over):
    """The datasets SPrompts builds for a config with preprocess = 'clip' and a model of resolution n_px."""
    from lpi_amd.retrieval.methods import sprompt as S
    m = S.SPrompts.__new__(S.SPrompts)
    m.args = {"image_root": str(coco), "annotation_train_root": str(coco / "train.json"), "annotation_val_root": str(coco / "val.json"),
              "pixel_format": pixel_format, "preprocess": "clip", **over}
    m._network = types.SimpleNamespace(clip_cfg=types.SimpleNamespace(image_resolution=n_px))
    return S.SPrompts._datasets(m, 0)


def clip_transform_eval(img, n_px):
    """models/clip/clip.py:71-78 of the reference (_transform) in Pillow calls: Resize(n_px, BICUBIC) of the shorter side, CenterCrop(n_px)."""
    w, h = img.size
    nw, nh = (n_px, int(n_px * h / w)) if w <= h else (int(n_px * w / h), n_px)
    img = img.resize((nw, nh), Image.BICUBIC)
    left, top = int(round((nw - n_px) / 2.0)), int(round((nh - n_px) / 2.0))
    return img.crop((left, top, left + n_px, top + n_px))


def clip_normalise(img):
    """ToTensor + Normalize((0.48145466, 0.4578275, 0.40821073), (0.26862954, 0.26130258, 0.27577711)) in float32 numpy."""
    a = np.asarray(img, dtype=np.uint8).astype(np.float32).transpose(2, 0, 1) / np.float32(255.0)
    mean = np.array([0.48145466, 0.4578275, 0.40821073], dtype=np.float32).reshape(3, 1, 1)
    std = np.array([0.26862954, 0.26130258, 0.27577711], dtype=np.float32).reshape(3, 1, 1)
    return (a - mean) / std


@pytest.mark.parametrize("n_px", [64, 224])
def test_clip_preprocessing_items_equal_pillow_calls(coco, n_px):
    assert D.CLIP_MEAN == (0.48145466, 0.4578275, 0.40821073) and D.CLIP_STD == (0.26862954, 0.26130258, 0.27577711)
    tr8, ev8 = clip_datasets(coco, "u8", n_px)
    tr32, ev32 = clip_datasets(coco, "f32", n_px)
    for i in range(len(ev8)):
        img = Image.open(coco / f"im{i}.jpg").convert("RGB")
        want = clip_transform_eval(img, n_px)
        assert np.array_equal(ev8[i][0].numpy(), np.asarray(want).transpose(2, 0, 1)), i
        got = ev32[i][0]
        assert got.dtype == torch.float32 and tuple(got.shape) == (3, n_px, n_px)
        assert np.abs(got.numpy() - clip_normalise(want)).max() < 1e-6, i
        assert torch.equal(got, D.normalise_u8(ev8[i][0], D.CLIP_MEAN, D.CLIP_STD))
        # the training form: RandomResizedCrop(n_px) + flip with the bicubic filter, CLIP's statistics
        torch.manual_seed(50 + i)
        a8 = tr8[i][0]
        torch.manual_seed(50 + i)
        a32 = tr32[i][0]
        torch.manual_seed(50 + i)
        x0, y0, x1, y1, rw, rh, ox, oy, flip = D.train_crop_params(img.size[0], img.size[1], n_px)
        pil = img.crop((x0, y0, x1, y1)).resize((n_px, n_px), Image.BICUBIC)
        pil = pil.transpose(Image.FLIP_LEFT_RIGHT) if flip else pil
        assert np.array_equal(a8.numpy(), np.asarray(pil).transpose(2, 0, 1)), i
        assert np.abs(a32.numpy() - clip_normalise(pil)).max() < 1e-6, i


def test_decoded_and_jpeg_items_carry_the_filter(coco):
    for fmt, collate in (("decoded", D.collate_decoded), ("jpeg", D.collate_encoded)):
        tr, ev = clip_datasets(coco, fmt, 64)
        assert tr.interpolation == ev.interpolation == "bicubic" and tr.normalize == ev.normalize == "clip"
        torch.manual_seed(1)
        items = [tr[i] for i in range(4)] + [(ev[i][0], "x", 0, 0) for i in range(2)]
        assert all(it[0].filter == "bicubic" and it[0].size == 64 for it in items)
        assert pickle.loads(pickle.dumps(items[0][0])).filter == "bicubic"
        batch = collate(items)[0]
        assert batch.filter == "bicubic" and len(batch) == 6
        again = pickle.loads(pickle.dumps(batch))
        assert again.filter == "bicubic" and torch.equal(again.params, batch.params)
        # the evaluation geometry is CLIP's: the shorter side resized to 64, the centre window
        w, h = Image.open(coco / "im5.jpg").size
        assert tuple(ev[5][0].params) == D.test_crop_params(w, h, 64, 64)
        # the reference preprocessing stays what it was, and the two do not mix in one batch
        plain = D.Coco(image_root=str(coco), ann_file=str(coco / "train.json"), tasks=[0], pixel_format=fmt, size=64)
        assert plain[0][0].filter == "bilinear" and collate([plain[0], plain[1]])[0].filter == "bilinear"
        with pytest.raises(ValueError, match="filter"):
            collate([items[0], plain[1]])
    for cls, args in ((D.DecodedBatch, ([], torch.zeros((0, 9), dtype=torch.int64), 8)),
                      (D.EncodedBatch, (torch.zeros(0, dtype=torch.uint8), torch.zeros(1, dtype=torch.int64), torch.zeros((0, 9), dtype=torch.int64),
                                        torch.zeros((0, 2), dtype=torch.int64), 8))):
        assert cls(*args).filter == "bilinear" and cls(*args, filter="box").filter == "box"
        with pytest.raises(ValueError):
            cls(*args, filter="lanczos")
    with pytest.raises(ValueError):
        D.Coco(image_root=str(coco), ann_file=str(coco / "train.json"), interpolation="nearest")
    with pytest.raises(ValueError):
        D.CocoEval(image_root=str(coco), ann_file=str(coco / "val.json"), normalize="laion")


def test_preprocess_config_keys(coco):
    assert D.preprocess_options({}) is None and D.engine_pixel_norm({}) is None
    assert D.preprocess_options({"preprocess": "reference"}, 224) == {"interpolation": "bilinear", "normalize": "imagenet", "eval_resize": 256,
                                                                      "size": 224}
    assert D.preprocess_options({"preprocess": "clip"}, 336) == {"interpolation": "bicubic", "normalize": "clip", "eval_resize": 336, "size": 336}
    assert D.preprocess_options({"preprocess": "clip", "eval_resize": 400, "interpolation": "box"}, 336)["eval_resize"] == 400
    assert D.engine_pixel_norm({"preprocess": "clip"}, 224) == "clip"
    assert D.engine_pixel_norm({"preprocess": "clip", "engine_options": {"pixel_norm": "clip", "ln_fold": 1}}, 224) == "clip"
    for bad in ({"preprocess": "openai"}, {"interpolation": "lanczos"}, {"normalize": "laion"}, {"eval_resize": 100}):
        with pytest.raises(ValueError):
            D.preprocess_options(bad, 224)
    # the datasets normalise 'f32' items, the engine every other format: different statistics for the two are an error
    for bad in ({"preprocess": "clip", "engine_options": {"pixel_norm": "imagenet"}}, {"normalize": "imagenet", "engine_options": {"pixel_norm": "clip"}},
                {"engine_options": {"pixel_norm": "clip"}}):
        with pytest.raises(ValueError, match="pixel_norm"):
            D.engine_pixel_norm(bad, 224)
    # the reference preprocessing by name builds what no key at all builds
    tr, ev = clip_datasets(coco, "u8", 224, preprocess="reference")
    base = D.CocoEval(image_root=str(coco), ann_file=str(coco / "val.json"), tasks=[0], pixel_format="u8")
    assert torch.equal(ev[2][0], base[2][0]) and tr.interpolation == "bilinear"


def test_clip_pixel_lut_equals_the_host_normalisation_bit_for_bit():
    from lpi_amd import engine as E
    assert E.PIXEL_NORMS["clip"] == (D.CLIP_MEAN, D.CLIP_STD) and E.PIXEL_NORMS["imagenet"] == (None, None)
    lut = E.make_pixel_lut(D.CLIP_MEAN, D.CLIP_STD)
    ramp = np.arange(256, dtype=np.uint8).reshape(16, 16, 1).repeat(3, axis=2)            # HWC: every byte value in every channel
    host = D._to_normalised_tensor(Image.fromarray(ramp), D.CLIP_MEAN, D.CLIP_STD)
    assert torch.equal(lut.view(3, 16, 16), host)
    assert torch.equal(E.make_pixel_lut(), E.make_pixel_lut(D.IMAGENET_MEAN, D.IMAGENET_STD))
    assert not torch.equal(lut, E.make_pixel_lut())
    assert E.EngineOptions().pixel_norm == "imagenet" and E.EngineOptions().pixel_stats() == (None, None)
    assert E.EngineOptions(pixel_norm="clip").pixel_stats() == (D.CLIP_MEAN, D.CLIP_STD)
    pair = E.EngineOptions.from_env(pixel_norm=[[0.5, 0.5, 0.5], [0.25, 0.25, 0.25]])
    assert pair.pixel_stats() == ((0.5, 0.5, 0.5), (0.25, 0.25, 0.25)) and hash(pair) is not None
    for bad in ("laion", 3, [[0.5, 0.5], [1, 1, 1]]):
        with pytest.raises(ValueError):
            E.EngineOptions(pixel_norm=bad)


def test_workspace_entry_takes_the_filter():
    """lpi_image_resample_workspace_f is host code: the bilinear case equals the entry without _f, bicubic needs the taps of twice the support, and
    every filter value outside {2, 3, 4} is LPI_EINVAL."""
    lib = _lib.load()
    desc = np.array([[0, 640, 480, 10, 20, 610, 470, 224, 224, 0, 0, 1], [0, 64, 48, 0, 0, 64, 48, 256, 341, 16, 58, 0]], dtype=np.int64)
    out = ctypes.c_long(0)

    def ws(code):
        out.value = -1
        rc = lib.lpi_image_resample_workspace_f(code, 2, 224, desc.ctypes.data, ctypes.addressof(out))
        return rc, out.value
    assert lib.lpi_image_resample_workspace(2, 224, desc.ctypes.data, ctypes.addressof(out)) == 0
    old = out.value

    def expect(fs):
        kx = max(int(np.ceil(fs * max(600 / 224, 1.0))), int(np.ceil(fs * 1.0))) * 2 + 1
        ky = max(int(np.ceil(fs * max(450 / 224, 1.0))), int(np.ceil(fs * 1.0))) * 2 + 1
        return 256 + 2 * 224 * (4 + kx + ky) * 4
    assert ws(2) == (0, old) and old == expect(1.0) == imageops.workspace_bytes(desc, 224) == imageops.workspace_bytes(desc, 224, "bilinear")
    assert ws(3) == (0, expect(2.0)) and expect(2.0) > old and imageops.workspace_bytes(desc, 224, "bicubic") == expect(2.0)
    assert ws(4) == (0, expect(0.5)) and imageops.workspace_bytes(desc, 224, "box") == expect(0.5)
    for code in (0, 1, 5, 6, -1, 7, 100):
        assert ws(code) == (-22, -1), code
    for name in ("nearest", "lanczos", "hamming", None, 3):
        with pytest.raises(ValueError):
            imageops.workspace_bytes(desc, 224, name)
