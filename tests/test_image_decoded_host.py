"""pixel_format='decoded', host side: the numpy restatement of Pillow's bilinear resample (tests/pil_resample.py, the GPU kernel's yardstick) against
Pillow; the transforms' parameter helpers against the transforms; the decoded items and their collate from the three datasets; the ragged host gather.
CPU only."""
import ctypes
import json

import numpy as np
import pytest
import torch

PIL = pytest.importorskip("PIL")
from PIL import Image  # noqa: E402

import pil_resample as R  # noqa: E402
from lpi_amd import _lib  # noqa: E402
from lpi_amd.retrieval.utils import data as D  # noqa: E402


def resize_cases(n, seed):
    """(w, h, ow, oh): random sizes, 1-px sources and outputs, 20x+ downscales, 8x+ upscales, extreme aspect ratios."""
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


def test_numpy_restatement_equals_pillow_bilinear():
    rng = np.random.default_rng(1)
    cases = resize_cases(110, 2)
    assert any(w >= 20 * ow for w, h, ow, oh in cases) and any(ow >= 8 * w for w, h, ow, oh in cases)
    for w, h, ow, oh in cases:
        src = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
        ref = np.asarray(Image.fromarray(src).resize((ow, oh), Image.BILINEAR))
        assert np.array_equal(R.resize(src, ow, oh), ref), (w, h, ow, oh)


def test_descriptor_restatement_equals_the_transforms_and_rng():
    """train_crop_params / test_crop_params through Pillow (apply_descriptor) and through the restatement give the transforms' 'u8' bytes, and the
    helpers draw exactly what the transforms draw."""
    rng = np.random.default_rng(3)
    for i, (w, h) in enumerate([(640, 480), (480, 640), (100, 900), (900, 64), (224, 224), (1, 50), (300, 2), (257, 26000)]):
        img = Image.fromarray(rng.integers(0, 256, (h, w, 3), dtype=np.uint8))
        for rep in range(3):
            torch.manual_seed(100 * i + rep)
            want = D.train_transform(img, pixel_format="u8")
            after = torch.get_rng_state()
            torch.manual_seed(100 * i + rep)
            desc = D.train_crop_params(w, h, 224)
            assert torch.equal(torch.get_rng_state(), after)
            assert torch.equal(D._to_u8_chw(D.apply_descriptor(img, desc, 224)), want)
            assert np.array_equal(R.apply(np.asarray(img), desc, 224), want.numpy())
        before = torch.get_rng_state()
        want = D.test_transform(img, pixel_format="u8")
        desc = D.test_crop_params(w, h, 256, 224)
        assert torch.equal(torch.get_rng_state(), before) and desc[8] == 0 and desc[:4] == (0, 0, w, h)
        assert np.array_equal(R.apply(np.asarray(img), desc, 224), want.numpy())


def test_invalid_descriptors_raise():
    ok = D.resample_descriptor(100, 80, (0, 0, 100, 80), (224, 224), (0, 0), False, 224)
    assert ok == (0, 0, 100, 80, 224, 224, 0, 0, 0)
    bad = [dict(box=(0, 0, 101, 80)), dict(box=(-1, 0, 10, 10)), dict(box=(5, 5, 5, 10)), dict(resized=(0, 224)), dict(origin=(1, 0)),
           dict(origin=(0, -1)), dict(size=0)]
    for b in bad:
        kw = dict(box=(0, 0, 100, 80), resized=(224, 224), origin=(0, 0), flip=False, size=224)
        kw.update(b)
        with pytest.raises(ValueError):
            D.resample_descriptor(100, 80, **kw)
    with pytest.raises(ValueError):
        D.DecodedImage(torch.zeros(4, 4, 3, dtype=torch.uint8), (0, 0, 5, 4, 4, 4, 0, 0, 0), 4)
    with pytest.raises(ValueError):
        D.DecodedImage(torch.zeros(4, 4, 3, dtype=torch.float32), (0, 0, 4, 4, 4, 4, 0, 0, 0), 4)


@pytest.fixture(scope="module")
def coco(tmp_path_factory):
    root = tmp_path_factory.mktemp("coco_decoded")
    rng = np.random.default_rng(4)
    train, val = [], []
    for i, (w, h) in enumerate([(320, 240), (240, 320), (500, 375), (64, 48), (224, 224)]):
        Image.fromarray(rng.integers(0, 256, size=(h, w, 3), dtype=np.uint8)).save(root / f"im{i}.png")
        train.append({"image": f"im{i}.png", "caption": f"a photo of thing {i}", "category": 11, "image_id": f"coco_{i}"})
        val.append({"image": f"im{i}.png", "caption": [f"first {i}", f"second {i}"], "category": 11, "image_id": i})
    (root / "train.json").write_text(json.dumps(train))
    (root / "val.json").write_text(json.dumps(val))
    return root


def check_batch(batch, n, size):
    imgs = batch[0]
    assert isinstance(imgs, D.DecodedBatch) and len(imgs) == n and imgs.size == size
    assert imgs.params.dtype == torch.int64 and tuple(imgs.params.shape) == (n, len(D.DESCRIPTOR_FIELDS))
    assert all(p.dtype == torch.uint8 and p.dim() == 3 and p.shape[2] == 3 for p in imgs.pixels)
    return imgs


@pytest.mark.parametrize("workers", [0, 2])
def test_decoded_items_and_collate(coco, workers):
    tr = D.Coco(image_root=str(coco), ann_file=str(coco / "train.json"), tasks=[0], pixel_format="decoded")
    ev = D.CocoEval(image_root=str(coco), ann_file=str(coco / "val.json"), tasks=[0], pixel_format="decoded")
    syn = D.SyntheticCoco(6, [0], 224, seed=3, pixel_format="decoded")
    # item contract, and the 'u8' bytes are the descriptor applied to the item's pixels
    torch.manual_seed(7)
    item = tr[2]
    torch.manual_seed(7)
    want = D.Coco(image_root=str(coco), ann_file=str(coco / "train.json"), tasks=[0], pixel_format="u8")[2][0]
    assert isinstance(item[0], D.DecodedImage) and item[1] == "a photo of thing 2" and item[2:] == (0, 0)
    assert tuple(item[0].pixels.shape) == (375, 500, 3)
    assert np.array_equal(R.apply(item[0].pixels.numpy(), item[0].params, 224), want.numpy())
    e = ev[1]
    want = D.CocoEval(image_root=str(coco), ann_file=str(coco / "val.json"), tasks=[0], pixel_format="u8")[1][0]
    assert e[1:] == (1, 0) and np.array_equal(R.apply(e[0].pixels.numpy(), e[0].params, 224), want.numpy())
    s = syn[4][0]
    assert 64 <= s.pixels.shape[0] <= 900 and 64 <= s.pixels.shape[1] <= 900 and torch.equal(s.pixels, syn[4][0].pixels)
    assert len({tuple(syn[i][0].pixels.shape) for i in range(6)}) > 1
    # collate at 0 and 2 workers, with pin_memory where a GPU is present
    for ds, bs in ((tr, 3), (ev, 2), (syn, 4)):
        loader = torch.utils.data.DataLoader(ds, batch_size=bs, shuffle=False, num_workers=workers, collate_fn=D.collate_decoded,
                                             pin_memory=torch.cuda.is_available())
        batches = list(loader)
        assert sum(len(b[0]) for b in batches) == len(ds)
        imgs = check_batch(batches[0], bs, 224)
        if ds is ev:
            assert batches[0][1].tolist() == [0, 1]
            assert torch.equal(imgs.params[0], torch.tensor(ds[0][0].params))
    pinned = D.collate_decoded([syn[0], syn[1]])[0]
    assert isinstance(pinned, D.DecodedBatch)
    with pytest.raises(ValueError):
        D.collate_decoded([(torch.zeros(3, 2, 2), "x")])


def test_invalid_pixel_format_raises(coco):
    for bad in ("f16", "DECODED", None):
        with pytest.raises(ValueError):
            D.SyntheticCoco(4, [0], pixel_format=bad)
        with pytest.raises(ValueError):
            D.Coco(image_root=str(coco), ann_file=str(coco / "train.json"), pixel_format=bad)
        with pytest.raises(ValueError):
            D.CocoEval(image_root=str(coco), ann_file=str(coco / "val.json"), pixel_format=bad)


def test_host_gather_v_copies_ragged_rows():
    lib = _lib.load()
    g = torch.Generator().manual_seed(0)
    sizes = [0, 1, 3, (1 << 20) + 7, 5, 3 << 20, 17]
    rows = [torch.randint(0, 256, (n,), dtype=torch.uint8, generator=g) for n in sizes]
    rows[2] = rows[1].expand(3).contiguous()
    for threads in (1, 4):
        dst = torch.full((sum(sizes) + 11,), 0xAB, dtype=torch.uint8)
        ptrs = (ctypes.c_void_p * len(rows))(*[r.data_ptr() if r.numel() else None for r in rows])
        nb = (ctypes.c_long * len(rows))(*sizes)
        rc = lib.lpi_host_gather_v(dst.data_ptr(), ctypes.cast(ptrs, ctypes.c_void_p), ctypes.cast(nb, ctypes.c_void_p), len(rows), threads)
        assert rc == 0
        assert torch.equal(dst[:sum(sizes)], torch.cat(rows)) and (dst[sum(sizes):] == 0xAB).all()
    nb = (ctypes.c_long * 2)(4, -1)
    ptrs = (ctypes.c_void_p * 2)(rows[3].data_ptr(), rows[3].data_ptr())
    assert lib.lpi_host_gather_v(dst.data_ptr(), ctypes.cast(ptrs, ctypes.c_void_p), ctypes.cast(nb, ctypes.c_void_p), 2, 2) == -22


def test_resample_entry_points_validate_without_a_gpu():
    """lpi_image_resample_workspace / _u8 refuse invalid descriptors on the host (no device call is reached: this machine may have no GPU)."""
    from lpi_amd import imageops
    good = np.array([[0, 100, 80, 0, 0, 100, 80, 224, 224, 0, 0, 1]], dtype=np.int64)
    n = imageops.workspace_bytes(good, 224)
    assert n == 256 + 224 * (4 + 3 + 3) * 4          # the table (96 bytes, padded to 256); upscales: 3 taps a side at most
    big = good.copy()
    big[0, 5], big[0, 1] = 4480, 4480
    assert imageops.workspace_bytes(big, 224) == 256 + 224 * (4 + 41 + 3) * 4
    lib = _lib.load()
    for field, value in ((5, 101), (3, 100), (7, 223), (9, 1), (11, 2), (0, -1), (1, 0)):
        bad = good.copy()
        bad[0, field] = value
        with pytest.raises(_lib.LpiError):
            imageops.workspace_bytes(bad, 224)
        rc = lib.lpi_image_resample_u8(1, 224, bad.ctypes.data, 8, 1 << 20, 8, 1 << 30, 8, None)
        assert rc == -22, field
    assert lib.lpi_image_resample_u8(1, 224, good.ctypes.data, 8, 100 * 80 * 3 - 1, 8, 1 << 30, 8, None) == -22      # source too short
    assert lib.lpi_image_resample_u8(1, 224, good.ctypes.data, 8, 100 * 80 * 3, 8, n - 1, 8, None) == -22           # workspace too small
    wide = good.copy()
    wide[0, 7:9] = 2000
    assert imageops.workspace_bytes(wide, 1024) > 0
    assert lib.lpi_image_resample_u8(1, 1025, wide.ctypes.data, 8, 100 * 80 * 3, 8, 1 << 30, 8, None) == -22         # S beyond the limit


@pytest.mark.parametrize("impl", ["synthetic", "coco"])
def test_plugin_loaders_for_decoded(coco, impl):
    """SPrompts' own dataset and loader setup (_datasets + _loaders, as incremental_train runs them) with pixel_format='decoded': the training batch is a
    DecodedBatch; the evaluation batch is one too for COCO, and stays the synthetic evaluation set's f32 images for dataset_impl='synthetic' (which has
    no decoded form) — each loader collates what its dataset yields."""
    import os
    from lpi_amd.retrieval.methods.sprompt import SPrompts
    ret = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "lpi_amd", "retrieval")
    args = json.load(open(os.path.join(ret, "configs", "lpi", "coco_lpi.json")))
    args.update(device=[torch.device("cpu")], backbonename="tiny", visual_dim=128, textual_dim=128, batch_size=3, num_workers=0, pixel_format="decoded",
                dataset_impl=impl, synthetic_train_size=6, synthetic_eval_images_per_task=4, image_root=str(coco),
                annotation_train_root=str(coco / "train.json"), annotation_val_root=str(coco / "val.json"))
    m = SPrompts(args)
    train_ds, test_ds = m._datasets(0)
    train_loader, test_loader = m._loaders(train_ds, test_ds)
    res = m._network.clip_cfg.image_resolution if impl == "synthetic" else 224
    check_batch(next(iter(train_loader)), 3, res)
    images = next(iter(test_loader))[0]
    if impl == "coco":
        assert isinstance(images, D.DecodedBatch) and len(images) == len(test_ds)
    else:
        assert torch.is_tensor(images) and images.dtype == torch.float32 and tuple(images.shape) == (4, 3, res, res)
