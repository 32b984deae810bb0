"""The resampling filters on a real MI355X: lpi_image_resample_u8_f (through the C ABI and lpi_amd.imageops) for BICUBIC and BOX against the numpy
restatement of Pillow's filtered resample (tests/pil_resample_filters.py) and Pillow itself, byte for byte; the BILINEAR case against the entry
points without _f; refusals; the four pixel formats under CLIP's own preprocessing; features under pixel_norm='clip'; BatchPipeline with a bicubic
batch."""
import json
import types

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import jpeg_cases as C  # noqa: E402
import pil_resample as R  # noqa: E402
import pil_resample_filters as F  # noqa: E402
from lpi_amd import _lib, imageops, synth  # noqa: E402
from lpi_amd.retrieval.utils import data as D  # noqa: E402

DEV = torch.device("cuda:0")
try:
    from PIL import Image
except ImportError:         # the restatement (pinned to Pillow by the CPU suite) is the yardstick then
    Image = None
NEW = ("bicubic", "box")


def batch_of(items, size, name):
    """[(HWC uint8 array, descriptor)] -> DecodedBatch."""
    return D.DecodedBatch([torch.from_numpy(np.ascontiguousarray(a)) for a, _ in items], torch.tensor([list(d) for _, d in items], dtype=torch.int64),
                          size, filter=name)


def check(items, size, name):
    got = imageops.resample_decoded(batch_of(items, size, name), device=DEV).cpu()
    assert got.shape == (len(items), 3, size, size) and got.dtype == torch.uint8 and got.is_contiguous()
    for i, (a, d) in enumerate(items):
        want = F.apply(F.NAMES[name], a, d, size)
        assert np.array_equal(got[i].numpy(), want), (name, i, a.shape, d)
        if Image is not None:
            pil = D._to_u8_chw(D.apply_descriptor(Image.fromarray(a), d, size, interpolation=name)).numpy()
            assert np.array_equal(want, pil), (name, i, a.shape, d)


def checkerboard(w, h, cell):
    y, x = np.mgrid[0:h, 0:w]
    return np.stack([(((x // cell) + (y // cell) + c) % 2) * 255 for c in range(3)], axis=2).astype(np.uint8)


def random_items(rng, n, size, lo=8, hi=700):
    """Ragged sources (every fourth a 0 / 255 checkerboard), train crops with and without flip, and centre windows of Resize(size) (CLIP's form) and
    of Resize(size * 8 // 7)."""
    items = []
    for i in range(n):
        w, h = (int(v) for v in rng.integers(lo, hi, 2))
        a = checkerboard(w, h, 1 + i % 5) if i % 4 == 3 else rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
        if i % 3 == 2 and min(w, h) * size // 224 >= 1:
            d = D.test_crop_params(w, h, size if i % 2 else size * 8 // 7, size)
        else:
            d = D.train_crop_params(w, h, size)
        if i % 2 and d[8] == 0 and i % 3 != 2:
            d = d[:8] + (1,)
        items.append((a, d))
    return items


@pytest.mark.parametrize("name", NEW)
@pytest.mark.parametrize("size", [7, 224, 336])
def test_kernel_equals_pillow_on_random_descriptors(size, name):
    torch.manual_seed(size)
    rng = np.random.default_rng(size)
    items = random_items(rng, 48, size)
    assert {d[8] for _, d in items} == {0, 1} and any(d[6] or d[7] for _, d in items)
    check(items, size, name)                           # one ragged batch
    check(items[3:4], size, name)                      # B = 1, a checkerboard


@pytest.mark.parametrize("name", NEW)
def test_kernel_extremes(name):
    """20x+ downscales, 8x+ upscales (checkerboards: bicubic's overshoot at both clamps), 1-px-wide sources, a source wider than 4096 px, crops
    Pillow resizes vertical-first mixed into a normal batch, a 1-px output."""
    rng = np.random.default_rng(5)
    px = lambda w, h: rng.integers(0, 256, (h, w, 3), dtype=np.uint8)  # noqa: E731
    S = 224
    items = [
        (px(4600, 4700), (0, 0, 4600, 4700, S, S, 0, 0, 0)),            # 20.5x / 21x downscale
        (checkerboard(5000, 300, 3), (100, 20, 4700, 260, S, S, 0, 0, 1)),   # wider than 4096, 20x horizontally
        (checkerboard(60, 50, 1), (10, 5, 38, 33, S, S, 0, 0, 0)),      # 8x upscale of 1-px squares
        (px(60, 50), (10, 5, 38, 33, S, S, 0, 0, 1)),
        (px(1, 300), (0, 0, 1, 300, S, S, 0, 0, 1)),                    # 1 px wide
        (px(1, 300), D.test_crop_params(1, 300, S, S)),                 # 1 px wide, CLIP's eval geometry (224 x 67200)
        (px(257, 26000), D.test_crop_params(257, 26000, S, S)),         # > 100 x taller than wide, shrunk: Pillow's vertical-first order
        (checkerboard(20, 2202, 2), (0, 0, 20, 2202, S, S, 0, 0, 1)),   # vertical-first
        (px(30, 4600), (0, 0, 30, 4600, 230, S, 3, 0, 0)),              # vertical-first with a window
        (px(4097, 64), D.test_crop_params(4097, 64, 256, S)),
        (px(224, 224), (0, 0, 224, 224, S, S, 0, 0, 0)),                # same size: the identity for all three filters
    ]
    assert R.vertical_first(257, 26000, items[6][1][5]) and R.vertical_first(20, 2202, S) and R.vertical_first(30, 4600, S)
    check(items, S, name)
    for it in items[5:9]:
        check([it], S, name)
    one = px(7, 5)
    check([(one, (0, 0, 7, 5, 1, 1, 0, 0, 0)), (px(640, 480), (0, 0, 640, 480, 1, 1, 0, 0, 1))], 1, name)


@pytest.mark.parametrize("name", NEW)
def test_kernel_batch_of_256(name):
    torch.manual_seed(256)
    rng = np.random.default_rng(256)
    check(random_items(rng, 256, 224, 64, 480), 224, name)


def raw_call(lib, entry, code, desc, src, ws, ws_bytes, out, size):
    s = torch.cuda.current_stream().cuda_stream
    head = () if code is None else (code,)
    return getattr(lib, entry)(*head, int(desc.shape[0]), size, desc.ctypes.data, src.data_ptr(), src.numel(), ws.data_ptr(), ws_bytes, out.data_ptr(), s)


def test_bilinear_through_the_new_entry_equals_the_old_entry():
    import ctypes
    lib = _lib.load()
    torch.manual_seed(3)
    rng = np.random.default_rng(3)
    items = random_items(rng, 40, 224) + [(rng.integers(0, 256, (2202, 20, 3), dtype=np.uint8), (0, 0, 20, 2202, 224, 224, 0, 0, 1))]
    batch = batch_of(items, 224, "bilinear")
    desc, nbytes = imageops.descriptors(batch)
    a, b = ctypes.c_long(0), ctypes.c_long(0)
    assert lib.lpi_image_resample_workspace(len(items), 224, desc.ctypes.data, ctypes.addressof(a)) == 0
    assert lib.lpi_image_resample_workspace_f(F.BILINEAR, len(items), 224, desc.ctypes.data, ctypes.addressof(b)) == 0
    assert a.value == b.value > 0
    src = torch.cat([torch.from_numpy(x).reshape(-1) for x, _ in items]).to(DEV)
    outs = []
    for entry, code in (("lpi_image_resample_u8", None), ("lpi_image_resample_u8_f", F.BILINEAR)):
        ws = torch.empty(a.value, dtype=torch.uint8, device=DEV)
        out = torch.zeros((len(items), 3, 224, 224), dtype=torch.uint8, device=DEV)
        n0 = _lib.launch_count()
        assert raw_call(lib, entry, code, desc, src, ws, a.value, out, 224) == 0
        torch.cuda.synchronize()
        assert _lib.launch_count() == n0 + 3           # tap tables, the resample, the vertical-first image
        outs.append(out.cpu())
    assert torch.equal(outs[0], outs[1])
    for i, (x, d) in enumerate(items):
        assert np.array_equal(outs[0][i].numpy(), R.apply(x, d, 224)), i


def test_refusals_come_before_any_copy_or_launch():
    """Every filter value outside {2, 3, 4} and a workspace sized for another filter are LPI_EINVAL with the launch count unchanged and the output
    and the workspace untouched."""
    lib = _lib.load()
    src = torch.zeros(480 * 640 * 3, dtype=torch.uint8, device=DEV)
    desc = np.array([[0, 640, 480, 0, 0, 640, 480, 224, 224, 0, 0, 0]], dtype=np.int64)
    small, large = imageops.workspace_bytes(desc, 224, "bilinear"), imageops.workspace_bytes(desc, 224, "bicubic")
    assert small < large
    ws = torch.full((large,), 7, dtype=torch.uint8, device=DEV)
    out = torch.full((3 * 224 * 224,), 9, dtype=torch.uint8, device=DEV)
    n0 = _lib.launch_count()
    for code in (0, 1, 5, 6, -1, 100):
        assert raw_call(lib, "lpi_image_resample_u8_f", code, desc, src, ws, large, out, 224) == -22, code
    assert raw_call(lib, "lpi_image_resample_u8_f", F.BICUBIC, desc, src, ws, small, out, 224) == -22      # sized for bilinear: not written past
    assert raw_call(lib, "lpi_image_resample_u8_f", F.BICUBIC, desc, src, ws, large - 1, out, 224) == -22
    bad = desc.copy()
    bad[0, 5] = 641
    assert raw_call(lib, "lpi_image_resample_u8_f", F.BOX, bad, src, ws, large, out, 224) == -22
    torch.cuda.synchronize()
    assert _lib.launch_count() == n0 and bool((ws == 7).all()) and bool((out == 9).all())
    for code in (F.BICUBIC, F.BOX, F.BILINEAR):
        assert raw_call(lib, "lpi_image_resample_u8_f", code, desc, src, ws, large, out, 224) == 0
    torch.cuda.synchronize()
    assert _lib.launch_count() == n0 + 6
    batch = batch_of([(np.zeros((480, 640, 3), np.uint8), tuple(desc[0, 3:]))], 224, "bicubic")
    with pytest.raises(ValueError):
        imageops.resample_decoded(batch, device=DEV, filter="lanczos")
    assert torch.equal(imageops.resample_decoded(batch, device=DEV, filter="box"), imageops.resample_decoded(batch_of(
        [(np.zeros((480, 640, 3), np.uint8), tuple(desc[0, 3:]))], 224, "box"), device=DEV))


# ------------------------------------------------------------------------------------------------ CLIP's own preprocessing, end to end
@pytest.fixture(scope="module")
def jpeg_coco(tmp_path_factory):
    pytest.importorskip("PIL")
    root = tmp_path_factory.mktemp("coco_filters_gpu")
    rng = np.random.default_rng(11)
    train, val = [], []
    sizes = [(64, 48), (120, 90), (90, 130), (200, 150), (57, 61), (300, 40), (48, 64), (150, 150)]
    for i, (w, h) in enumerate(sizes):
        a = checkerboard(w, h, 3) if i % 3 == 1 else rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
        Image.fromarray(a).save(root / f"im{i}.jpg", quality=90)
        train.append({"image": f"im{i}.jpg", "caption": f"a photo of thing number {i}", "category": 11, "image_id": f"coco_{i}"})
        val.append({"image": f"im{i}.jpg", "caption": [f"first caption {i}", f"second caption {i}"], "category": 11, "image_id": i})
    (root / "train.json").write_text(json.dumps(train))
    (root / "val.json").write_text(json.dumps(val))
    return root


def clip_datasets(root, pixel_format, n_px):
    """The datasets SPrompts builds for a config with preprocess = 'clip' and a model of resolution n_px."""
    from lpi_amd.retrieval.methods import sprompt as S
    m = S.SPrompts.__new__(S.SPrompts)
    m.args = {"image_root": str(root), "annotation_train_root": str(root / "train.json"), "annotation_val_root": str(root / "val.json"),
              "pixel_format": pixel_format, "preprocess": "clip"}
    m._network = types.SimpleNamespace(clip_cfg=types.SimpleNamespace(image_resolution=n_px))
    return S.SPrompts._datasets(m, 0)


def clip_batches(root, pixel_format, n_px, seed=0):
    """(train images, eval images) of the whole folder in `pixel_format` under preprocess = 'clip': uint8 [8,3,S,S] on the host ('f32': float32)."""
    tr, ev = clip_datasets(root, pixel_format, n_px)
    torch.manual_seed(seed)
    a = [tr[i][0] for i in range(len(tr))]
    b = [ev[i][0] for i in range(len(ev))]
    if pixel_format in ("u8", "f32"):
        return torch.stack(a), torch.stack(b)
    collate, run = (D.collate_decoded, imageops.resample_decoded) if pixel_format == "decoded" else (D.collate_encoded, imageops.resample_encoded)
    out = []
    for items in (a, b):
        batch = collate([(x,) for x in items])[0]
        assert batch.filter == "bicubic" and batch.size == n_px
        out.append(run(batch, device=DEV).cpu())
    return tuple(out)


@pytest.mark.parametrize("n_px", [32, 224])
def test_four_pixel_formats_agree_under_clip_preprocessing(jpeg_coco, n_px):
    """The same JPEG folder through 'f32', 'u8' (Pillow on the host), 'decoded' and 'jpeg' (the GPU) with preprocess = 'clip': the same [B,3,S,S]
    bytes in the training form (fixed seed) and in the evaluation form; the 'f32' items are those bytes under CLIP's ToTensor + Normalize."""
    got = {pf: clip_batches(jpeg_coco, pf, n_px) for pf in D.PIXEL_FORMATS}
    for form in (0, 1):
        u8 = got["u8"][form]
        assert u8.dtype == torch.uint8 and tuple(u8.shape) == (8, 3, n_px, n_px)
        assert torch.equal(got["decoded"][form], u8), form
        assert torch.equal(got["jpeg"][form], u8), form
        assert torch.equal(got["f32"][form], D.normalise_u8(u8, D.CLIP_MEAN, D.CLIP_STD)), form
    # and they are not the reference loader's bytes
    ev = D.CocoEval(image_root=str(jpeg_coco), ann_file=str(jpeg_coco / "val.json"), tasks=[0], pixel_format="u8", size=n_px, resize=n_px)
    assert not torch.equal(torch.stack([ev[i][0] for i in range(8)]), got["u8"][1])


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_features_from_jpeg_with_clip_pixel_norm_equal_host_normalised_f32(jpeg_coco, dtype):
    """DualEncoder image features of the 'jpeg' batch under EngineOptions(pixel_norm='clip') (decode, bicubic resample, then ToTensor + Normalize inside
    lpi_patchify_u8 through the CLIP table) equal those of the host-normalised 'f32' items, to the bits; with the default table they do not."""
    from lpi_amd.engine import DualEncoder, EngineOptions
    cfg = synth.TINY
    sd = synth.clip_state_dict(cfg)
    S = cfg.image_resolution
    f32 = clip_batches(jpeg_coco, "f32", S)[1].to(DEV)
    jpeg = clip_batches(jpeg_coco, "jpeg", S)[1].to(DEV)
    enc = DualEncoder(cfg, sd, dtype=dtype, device=DEV, options=EngineOptions.from_env(pixel_norm="clip"))
    n0 = _lib.launch_count()
    a = enc.encode_image(jpeg).clone()
    b = enc.encode_image(f32).clone()
    torch.cuda.synchronize()
    assert _lib.launch_count() > n0 and bool(torch.isfinite(a).all())
    assert torch.equal(a, b)
    plain = DualEncoder(cfg, sd, dtype=dtype, device=DEV)
    assert not torch.equal(plain.encode_image(jpeg), b)
    pair = DualEncoder(cfg, sd, dtype=dtype, device=DEV, options=EngineOptions.from_env(pixel_norm=(D.CLIP_MEAN, D.CLIP_STD)))
    assert torch.equal(pair.encode_image(jpeg), b)


def tiny_args(**over):
    import os
    ret = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "lpi_amd", "retrieval")
    args = json.load(open(os.path.join(ret, "configs", "lpi", "coco_lpi.json")))
    args.update(backbonename="tiny", visual_dim=128, textual_dim=128, device=[DEV], compute_dtype="f32", batch_size=4, epochs=1, num_workers=0)
    args.update(over)
    return args


@pytest.fixture()
def synthetic_bpe(tmp_path, monkeypatch):
    import bpe_synth
    from lpi_amd.retrieval.models.clip import prompt_learner as PL
    monkeypatch.setenv("LPI_BPE_VOCAB", bpe_synth.write_table(tmp_path / "synthetic_bpe.txt.gz", seed=5))
    monkeypatch.setattr(PL, "_tokenizer", None)
    yield
    monkeypatch.setattr(PL, "_tokenizer", None)


def test_plugin_config_sets_datasets_and_engine_together(jpeg_coco, synthetic_bpe):
    """preprocess = 'clip' in the plugin's config: bicubic datasets of the model's resolution and an engine with CLIP's table; engine_options that name
    other statistics are refused."""
    from lpi_amd.retrieval.methods.sprompt import SPrompts
    paths = dict(image_root=str(jpeg_coco), annotation_train_root=str(jpeg_coco / "train.json"), annotation_val_root=str(jpeg_coco / "val.json"))
    m = SPrompts(tiny_args(preprocess="clip", pixel_format="jpeg", dataset_impl="coco", engine_options={"ln_fold": 1}, **paths))
    eng = m._network.to(DEV).engine
    assert eng.opt.pixel_norm == "clip" and eng.opt.ln_fold == 1
    tr, ev = m._datasets(0)
    S = synth.TINY.image_resolution
    assert tr.interpolation == ev.interpolation == "bicubic" and tr[0][0].size == S and ev[0][0].filter == "bicubic"
    assert min(ev[3][0].params[4:6]) == S
    plain = SPrompts(tiny_args(pixel_format="jpeg", dataset_impl="coco", **paths))
    assert plain._network.to(DEV).engine.opt.pixel_norm == "imagenet" and plain._datasets(0)[0][0][0].filter == "bilinear"
    with pytest.raises(ValueError, match="pixel_norm"):
        SPrompts(tiny_args(preprocess="clip", engine_options={"pixel_norm": "imagenet"}, **paths))._network.to(DEV)


def test_pipeline_with_a_bicubic_batch_and_a_redone_file():
    """BatchPipeline over bicubic EncodedBatches, one of them with a file whose GPU status is not OK (restart markers out of order): that batch is
    decoded again by Pillow and resampled again WITH THE BATCH'S FILTER; and over a bicubic DecodedBatch.  Every batch equals Pillow's bicubic bytes."""
    pytest.importorskip("PIL")
    import io
    from lpi_amd.pipeline import BatchPipeline
    rng = np.random.default_rng(12)
    good = C.encode(C.pixels(rng, 150, 90), "4:2:0", 85, restart_marker_blocks=2)
    files = [good, C.rst_out_of_order(good), C.encode(C.pixels(rng, 70, 120), "4:4:4", 60), C.encode(checkerboard(40, 30, 2), "4:4:4", 95),
             C.encode(C.pixels(rng, 300, 200), "4:2:2", 80), good]
    S = 224
    torch.manual_seed(4)
    t = D.encoded_transform("train", S, interpolation="bicubic")
    items = [t(f) for f in files]
    ids = torch.from_numpy(synth.token_ids(len(files), seed=4))
    enc = [D.collate_encoded([(x,) for x in items[3 * j:3 * j + 3]]) + [ids[3 * j:3 * j + 3]] for j in range(2)]
    assert all(b[0].filter == "bicubic" and not b[0].fallback for b in enc)
    d = imageops._issue_decode(enc[0][0], DEV, torch.cuda.current_stream())
    torch.cuda.synchronize()
    assert d.status[:3].tolist()[0] == 0 and d.status[:3].tolist()[1] != 0          # the re-launch path is taken for the first batch
    want = [torch.stack([D._to_u8_chw(D.apply_descriptor(Image.open(io.BytesIO(f)).convert("RGB"), x.params, S, interpolation="bicubic"))
                         for f, x in zip(files[3 * j:3 * j + 3], items[3 * j:3 * j + 3])]) for j in range(2)]
    bilinear = torch.stack([D._to_u8_chw(D.apply_descriptor(Image.open(io.BytesIO(f)).convert("RGB"), x.params, S)) for f, x in zip(files[:3], items[:3])])
    assert not torch.equal(bilinear, want[0])
    dec_t = D.decoded_transform("center", S, S, interpolation="bicubic")
    dec_items = [dec_t(Image.open(io.BytesIO(f)).convert("RGB")) for f in files[2:5]]
    dec = D.collate_decoded([(x,) for x in dec_items]) + [ids[:3]]
    want.append(torch.stack([D._to_u8_chw(D.apply_descriptor(Image.open(io.BytesIO(f)).convert("RGB"), x.params, S, interpolation="bicubic"))
                             for f, x in zip(files[2:5], dec_items)]))
    n = 0
    for j, b in enumerate(BatchPipeline(enc + [dec], DEV, None, depth=2, threads=3)):
        assert b.images.dtype == torch.uint8 and tuple(b.images.shape) == (3, 3, S, S)
        assert torch.equal(b.images.cpu(), want[j]), j
        n += 1
    assert n == 3
    assert torch.equal(imageops.resample_encoded(enc[0][0], device=DEV).cpu(), want[0])
