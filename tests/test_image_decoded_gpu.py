"""pixel_format='decoded' on a real MI355X: lpi_image_resample_u8 (through the C ABI, lpi_amd.imageops) against the numpy restatement of Pillow's
bilinear resample (tests/pil_resample.py) and Pillow itself, byte for byte; its host-side refusals; the plugin loop and the evaluation on 'decoded' against
'u8' (bit-identical losses, parameters, scores); BatchPipeline's decoded slots against direct calls."""
import json

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import pil_resample as R  # noqa: E402
from lpi_amd import _lib, imageops, synth  # noqa: E402
from lpi_amd.retrieval.utils import data as D  # noqa: E402

DEV = torch.device("cuda:0")
try:
    from PIL import Image
except ImportError:         # the restatement (pinned to Pillow by the CPU suite) is the yardstick then
    Image = None


def batch_of(items, size):
    """[(HWC uint8 array, descriptor)] -> DecodedBatch."""
    return D.DecodedBatch([torch.from_numpy(np.ascontiguousarray(a)) for a, _ in items], torch.tensor([list(d) for _, d in items], dtype=torch.int64),
                          size)


def check(items, size):
    got = imageops.resample_decoded(batch_of(items, size), device=DEV).cpu()
    assert got.shape == (len(items), 3, size, size) and got.dtype == torch.uint8 and got.is_contiguous()
    for i, (a, d) in enumerate(items):
        want = R.apply(a, d, size)
        assert np.array_equal(got[i].numpy(), want), (i, a.shape, d)
        if Image is not None:
            pil = D._to_u8_chw(D.apply_descriptor(Image.fromarray(a), d, size)).numpy()
            assert np.array_equal(want, pil), (i, a.shape, d)


def random_items(rng, n, size, lo=8, hi=700):
    items = []
    for i in range(n):
        w, h = (int(v) for v in rng.integers(lo, hi, 2))
        a = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
        if i % 3 == 2 and min(w, h) * size // 224 >= 1:
            resize = size * 8 // 7
            d = D.test_crop_params(w, h, resize, size)
        else:
            d = D.train_crop_params(w, h, size)
        if i % 2 and d[8] == 0 and i % 3 != 2:
            d = d[:8] + (1,)
        items.append((a, d))
    return items


@pytest.mark.parametrize("size", [224, 336])
def test_kernel_equals_pillow_on_random_descriptors(size):
    torch.manual_seed(size)
    rng = np.random.default_rng(size)
    items = random_items(rng, 64, size)
    assert {d[8] for _, d in items} == {0, 1} and any(d[:4] == (0, 0, a.shape[1], a.shape[0]) for a, d in items)
    check(items, size)                           # one mixed-size batch of 64
    check(items[:1], size)                       # B = 1


def test_kernel_extremes():
    """20x+ downscales, 8x+ upscales, a 1-px-wide source, a source wider than 4096 px, a crop Pillow resizes vertical-first, a 1-px output."""
    rng = np.random.default_rng(5)
    px = lambda w, h: rng.integers(0, 256, (h, w, 3), dtype=np.uint8)  # noqa: E731
    S = 224
    items = [
        (px(4600, 4700), (0, 0, 4600, 4700, S, S, 0, 0, 0)),            # 20.5x / 21x downscale
        (px(5000, 300), (100, 20, 4700, 260, S, S, 0, 0, 1)),           # wider than 4096, 20x horizontally
        (px(60, 50), (10, 5, 38, 33, S, S, 0, 0, 0)),                   # 8x upscale
        (px(1, 300), (0, 0, 1, 300, S, S, 0, 0, 1)),                    # 1 px wide
        (px(1, 300), D.test_crop_params(1, 300, 256, S)),               # 1 px wide, eval geometry (256 x 76800)
        (px(257, 26000), D.test_crop_params(257, 26000, 256, S)),       # > 100 x taller than wide, shrunk: Pillow's vertical-first order
        (px(20, 2202), (0, 0, 20, 2202, S, S, 0, 0, 1)),
        (px(4097, 64), D.test_crop_params(4097, 64, 256, S)),
    ]
    assert R.vertical_first(257, 26000, items[5][1][5]) and R.vertical_first(20, 2202, S)
    check(items, S)
    for a, d in items:
        check([(a, d)], S)
    one = px(7, 5)
    check([(one, (0, 0, 7, 5, 1, 1, 0, 0, 0))], 1)


def test_kernel_batch_of_256():
    torch.manual_seed(256)
    rng = np.random.default_rng(256)
    check(random_items(rng, 256, 224, 64, 480), 224)


def test_bad_descriptors_return_einval_before_any_launch():
    lib = _lib.load()
    a = torch.zeros(80 * 100 * 3, dtype=torch.uint8, device=DEV)
    good = np.array([[0, 100, 80, 0, 0, 100, 80, 224, 224, 0, 0, 0]], dtype=np.int64)
    ws = torch.empty(1 << 20, dtype=torch.uint8, device=DEV)
    out = torch.empty(3 * 224 * 224, dtype=torch.uint8, device=DEV)
    s = torch.cuda.current_stream().cuda_stream
    n0 = _lib.launch_count()
    for field, value in ((5, 101), (3, 100), (4, -1), (7, 0), (9, 1), (10, 1), (11, 2), (0, 1), (2, 81)):
        bad = good.copy()
        bad[0, field] = value
        rc = lib.lpi_image_resample_u8(1, 224, bad.ctypes.data, a.data_ptr(), a.numel(), ws.data_ptr(), ws.numel(), out.data_ptr(), s)
        assert rc == -22, (field, rc)
    assert lib.lpi_image_resample_u8(1, 224, good.ctypes.data, a.data_ptr(), a.numel(), ws.data_ptr(), 16, out.data_ptr(), s) == -22
    assert _lib.launch_count() == n0
    assert lib.lpi_image_resample_u8(1, 224, good.ctypes.data, a.data_ptr(), a.numel(), ws.data_ptr(), ws.numel(), out.data_ptr(), s) == 0
    torch.cuda.synchronize()
    assert _lib.launch_count() == n0 + 2
    with pytest.raises(_lib.LpiError):
        imageops.resample_decoded(batch_of([(np.zeros((4, 4, 3), np.uint8), (0, 0, 4, 4, 4, 4, 0, 0, 0))], 5), device=DEV)


# ------------------------------------------------------------------------------------------------ the plugin on 'decoded' against 'u8'
@pytest.fixture(scope="module")
def jpeg_coco(tmp_path_factory):
    pytest.importorskip("PIL")
    root = tmp_path_factory.mktemp("coco_jpeg")
    rng = np.random.default_rng(11)
    train, val = [], []
    sizes = [(64, 48), (120, 90), (90, 130), (200, 150), (57, 61), (300, 40), (48, 64), (150, 150)]
    for i, (w, h) in enumerate(sizes):
        Image.fromarray(rng.integers(0, 256, (h, w, 3), dtype=np.uint8)).save(root / f"im{i}.jpg", quality=90)
        train.append({"image": f"im{i}.jpg", "caption": f"a photo of thing number {i}", "category": 11, "image_id": f"coco_{i}"})
        val.append({"image": f"im{i}.jpg", "caption": [f"first caption {i}", f"second caption {i}"], "category": 11, "image_id": i})
    (root / "train.json").write_text(json.dumps(train))
    (root / "val.json").write_text(json.dumps(val))
    return root


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


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_plugin_train_and_eval_decoded_equals_u8(jpeg_coco, synthetic_bpe, dtype):
    """Two train_epoch steps over a JPEG COCO folder, then the task keys (clustering) and _evaluate_retrieval: the 'decoded' datasets (crop / resize /
    flip on the GPU) and the 'u8' ones (the same on the host with Pillow) under the same seed give bit-identical losses, gradients, parameters, score
    matrices and R@K."""
    from torch.utils.data import DataLoader
    from lpi_amd.retrieval.methods.sprompt import SPrompts
    root, S = str(jpeg_coco), synth.TINY.image_resolution
    got = {}
    for fmt in ("u8", "decoded"):
        if fmt == "u8":
            tr = D.Coco(image_root=root, ann_file=str(jpeg_coco / "train.json"), tasks=[0],
                        transform=lambda im: D.train_transform(im, size=S, pixel_format="u8"))
            ev = D.CocoEval(image_root=root, ann_file=str(jpeg_coco / "val.json"), tasks=[0],
                            transform=lambda im: D.test_transform(im, resize=S + 4, size=S, pixel_format="u8"))
            collate = None
        else:
            tr = D.Coco(image_root=root, ann_file=str(jpeg_coco / "train.json"), tasks=[0], pixel_format="decoded", size=S)
            ev = D.CocoEval(image_root=root, ann_file=str(jpeg_coco / "val.json"), tasks=[0], pixel_format="decoded", size=S, resize=S + 4)
            collate = D.collate_decoded
        m = SPrompts(tiny_args(compute_dtype=dtype, epochs=2))
        net = m._network.to(DEV)
        for t in range(len(net.prompts)):
            for k, v in synth.prompt_factors(9, 16, 128, 128, task=t).items():
                getattr(net.prompts[t], k).data = torch.from_numpy(v.copy()).to(DEV)
        net.numtask = 1
        opt, sch = m._setup_training()
        losses, grads = [], []

        def on_step(i, batch, out):
            losses.append({k: (v.detach().clone() if torch.is_tensor(v) else v) for k, v in out["loss"].items()})
            fg = getattr(opt, "flat_grad", None)
            grads.append(fg.detach().clone() if fg is not None else None)
            return False
        torch.manual_seed(0)
        loader = DataLoader(tr, batch_size=4, shuffle=False, num_workers=0, collate_fn=collate or D.collate_keep_images)
        m.train_epoch(loader, opt, 0, on_step=on_step)
        torch.cuda.synchronize()
        assert len(losses) == 2
        params = {k: getattr(net.prompts[0], k).detach().clone() for k in synth.PROMPT_NAMES}
        torch.manual_seed(1)
        m.clustering(DataLoader(tr, batch_size=4, shuffle=False, num_workers=0, collate_fn=collate or D.collate_keep_images))
        test_loader = DataLoader(ev, batch_size=3, shuffle=False, num_workers=0, pin_memory=True, collate_fn=collate)
        s_i2t, s_t2i, res = m._evaluate_retrieval(test_loader)
        got[fmt] = (losses, grads, params, [k.clone() for k in m.all_keys], s_i2t, s_t2i, res)
    a, b = got["u8"], got["decoded"]
    for la, lb in zip(a[0], b[0]):
        assert la.keys() == lb.keys()
        for k in la:
            va, vb = la[k], lb[k]
            if isinstance(va, tuple):
                assert all(torch.equal(x, y) for x, y in zip(va, vb)), k
            else:
                assert torch.equal(va, vb) if torch.is_tensor(va) else va == vb, k
    for ga, gb in zip(a[1], b[1]):
        assert (ga is None and gb is None) or torch.equal(ga, gb)
    for k in synth.PROMPT_NAMES:
        assert torch.equal(a[2][k], b[2][k]), k
    assert all(torch.equal(x, y) for x, y in zip(a[3], b[3]))
    assert np.array_equal(a[4], b[4]) and np.array_equal(a[5], b[5]) and a[6] == b[6]


def test_pipeline_decoded_slots_grow_and_match_direct_calls():
    """BatchPipeline over two passes whose batches differ in total bytes (the byte / workspace slots grow): every batch it hands out equals
    resample_decoded on the same DecodedBatch."""
    from lpi_amd.pipeline import BatchPipeline

    class Epochs:
        def __init__(self, lists):
            self.lists, self.n = lists, 0

        def __iter__(self):
            self.n += 1
            return iter(self.lists[(self.n - 1) % len(self.lists)])

    def batches(seed, n):
        ds = D.SyntheticCoco(4 * n, [0], 224, seed=seed, pixel_format="decoded")
        torch.manual_seed(seed)
        ids = torch.from_numpy(synth.token_ids(4 * n, seed=seed))
        return [D.collate_decoded([ds[4 * j + i] for i in range(4)])[:1] + [ids[4 * j:4 * j + 4]] for j in range(n)]
    small, large = batches(1, 3), batches(2, 3)
    # the first pass: 64 x 64 corners of the images (synthetic sides are >= 64 px), so the second pass's full-size images grow the slots
    small = [[D.DecodedBatch([p[:64, :64].contiguous() for p in b[0].pixels], torch.tensor([[0, 0, 64, 64, 224, 224, 0, 0, j % 2]] * 4), 224), b[1]]
             for j, b in enumerate(small)]
    want = [[imageops.resample_decoded(b[0], device=DEV).cpu() for b in lst] for lst in (small, large)]
    pipe = BatchPipeline(Epochs([small, large]), DEV, None, depth=2, threads=3)
    for ep in range(2):
        n = 0
        for j, b in enumerate(pipe):
            assert b.images.dtype == torch.uint8 and tuple(b.images.shape) == (4, 3, 224, 224)
            assert torch.equal(b.images.cpu(), want[ep][j]), (ep, j)
            n += 1
        assert n == 3
    assert pipe._retired, "the second pass's larger batches grew the slots"
