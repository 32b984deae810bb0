"""pixel_format='jpeg' on a real MI355X: lpi_jpeg_decode_u8 (through the C ABI, lpi_amd.imageops) against the committed Pillow decodes
(tests/golden/jpeg_pillow.npz) and Pillow itself, byte for byte; fallbacks, corrupt files, refusals; resample_encoded against resample_decoded."""
import hashlib
import json

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import jpeg_cases as C  # noqa: E402
from lpi_amd import _lib, imageops, synth  # noqa: E402
from lpi_amd.retrieval.utils import data as D  # noqa: E402

DEV = torch.device("cuda:0")


def encoded_batch(files, size=224, form="train", seed=0):
    """EncodedBatch of file bytes (the worker's transform: GPU files stay encoded, the others are decoded by Pillow), and the DecodedBatch of the same
    files and draws."""
    torch.manual_seed(seed)
    enc = D.collate_encoded([(D.encoded_transform(form, size)(f),) for f in files])[0]
    torch.manual_seed(seed)
    dec_t = D.decoded_transform(form, size)
    decs = [dec_t(D._pil().open(__import__("io").BytesIO(f)).convert("RGB")) for f in files]
    dec = D.collate_decoded([(d,) for d in decs])[0]
    return enc, dec


def gpu_statuses(enc):
    """The GPU statuses of the batch's GPU files (0: decoded exactly; the fallback would hide a kernel that is not)."""
    d = imageops._issue_decode(enc, DEV, torch.cuda.current_stream())
    torch.cuda.synchronize()
    return d.status[:len(d.gpu)].tolist()


def test_fixture_decodes_byte_for_byte(golden):
    g = golden("jpeg_pillow")
    files = [bytes(g["data"][g["offsets"][i]:g["offsets"][i + 1]]) for i in range(len(g["offsets"]) - 1)]
    enc = D.EncodedBatch(torch.from_numpy(g["data"].copy()), torch.from_numpy(g["offsets"].copy()), torch.zeros((len(files), 9), dtype=torch.int64),
                         torch.from_numpy(g["wh"].copy()), 224)
    n0 = _lib.launch_count()
    got = imageops.decode_jpeg(enc, device=DEV)
    assert _lib.launch_count() - n0 >= 4
    assert gpu_statuses(enc) == [0] * len(files)
    for i, px in enumerate(got):
        a = px.cpu().numpy()
        key = f"pixels{i}"
        if key in g:
            assert np.array_equal(a, g[key]), i
        else:
            assert hashlib.sha256(a.tobytes()).hexdigest() == str(g["sha256"][i]), i


def test_random_files_equal_pillow():
    pytest.importorskip("PIL")
    files = C.random_files(11, 256)
    enc, dec = encoded_batch(files)
    assert not enc.fallback
    assert gpu_statuses(enc) == [0] * len(files)
    got = imageops.decode_jpeg(enc, device=DEV)
    for i, f in enumerate(files):
        assert np.array_equal(got[i].cpu().numpy(), C.decode_pil(f)), i
    a = imageops.resample_encoded(enc, device=DEV).cpu()
    b = imageops.resample_decoded(dec, device=DEV).cpu()
    assert torch.equal(a, b)


def test_batch_shaped_like_the_tool():
    """One batch of 640 x 480 q90 4:2:0 files (the shape tools/decode_pipeline_bench.py measures)."""
    pytest.importorskip("PIL")
    rng = np.random.default_rng(640)
    files = [C.encode(C.pixels(rng, 640, 480), "4:2:0", 90) for _ in range(32)]
    enc, dec = encoded_batch(files, form="center")
    assert gpu_statuses(enc) == [0] * len(files)
    got = imageops.decode_jpeg(enc, device=DEV)
    for i, f in enumerate(files):
        assert np.array_equal(got[i].cpu().numpy(), C.decode_pil(f)), i
    assert torch.equal(imageops.resample_encoded(enc, device=DEV).cpu(), imageops.resample_decoded(dec, device=DEV).cpu())


def odd_files():
    """Files outside the envelope: progressive, CMYK, a PNG under a .jpg name; and two GPU files."""
    import io
    from PIL import Image
    rng = np.random.default_rng(3)
    a = C.pixels(rng, 77, 51)
    out = []
    for kw in ({"format": "JPEG", "progressive": True}, {"format": "PNG"}):
        b = io.BytesIO()
        Image.fromarray(a).save(b, **kw)
        out.append(b.getvalue())
    b = io.BytesIO()
    Image.fromarray(a).convert("CMYK").save(b, "JPEG")
    out.append(b.getvalue())
    return out + [C.encode(a, "4:2:2", 70), C.encode(a[:40, :33], gray=True, quality=85)]


def test_mixed_batch_with_fallbacks_equals_pillow():
    pytest.importorskip("PIL")
    files = odd_files()
    files = [files[3], files[0], files[1], files[4], files[2]]
    enc, dec = encoded_batch(files)
    assert sorted(enc.fallback) == [1, 2, 4]
    assert gpu_statuses(enc) == [0, 0]
    got = imageops.decode_jpeg(enc, device=DEV)
    for i, f in enumerate(files):
        assert np.array_equal(got[i].cpu().numpy(), C.decode_pil(f)), i
    assert torch.equal(imageops.resample_encoded(enc, device=DEV).cpu(), imageops.resample_decoded(dec, device=DEV).cpu())


def test_corrupt_and_truncated_files_give_pillows_result():
    """Flipped bits in the entropy data and a truncated file: the GPU status is not OK for at least the truncated one, and the result is Pillow's
    pixels (or Pillow's exception), whatever the kernel met."""
    pytest.importorskip("PIL")
    import jpeg_restate as J
    rng = np.random.default_rng(9)
    good = C.encode(C.pixels(rng, 200, 120), "4:2:0", 90)
    ent = J.parse(good)["ent"]
    flipped = bytearray(good)
    for pos in rng.integers(ent + 10, len(good) - 10, 6):
        flipped[pos] ^= 0x5A
    files = [good, bytes(flipped), good[:ent + (len(good) - ent) // 2], good]
    for f in files:
        assert imageops.jpeg_info(f)[0]
    enc = D.EncodedBatch(torch.frombuffer(bytearray(b"".join(files)), dtype=torch.uint8),
                         torch.tensor(np.concatenate(([0], np.cumsum([len(f) for f in files]))), dtype=torch.int64),
                         torch.tensor([[0, 0, 200, 120, 224, 224, 0, 0, 0]] * 4), torch.tensor([[200, 120]] * 4), 224)
    d = imageops._issue_decode(enc, DEV, torch.cuda.current_stream())
    torch.cuda.synchronize()
    st = d.status[:4].tolist()
    assert st[0] == 0 and st[3] == 0 and st[2] != 0, st
    for i, f in enumerate(files):
        one = D.EncodedBatch(enc.file(i).clone(), torch.tensor([0, len(f)]), enc.params[:1], enc.wh[:1], 224)
        try:
            want = C.decode_pil(f)
        except Exception as e:      # noqa: BLE001 — then decode_jpeg raises Pillow's exception
            with pytest.raises(type(e)):
                imageops.decode_jpeg(one, device=DEV)
            continue
        assert np.array_equal(imageops.decode_jpeg(one, device=DEV)[0].cpu().numpy(), want), (i, st)


def test_invalid_calls_return_einval_before_any_launch():
    lib = _lib.load()
    files = C.random_files(5, 2, 8, 64)
    host = np.frombuffer(b"".join(files), np.uint8).copy()
    offs = np.array([0, len(files[0]), host.size], dtype=np.int64)
    src = torch.from_numpy(host).to(DEV)
    ws_n = imageops.jpeg_workspace_bytes(host, offs)
    ws = torch.empty(ws_n, dtype=torch.uint8, device=DEV)
    status = torch.empty(2, dtype=torch.int32, device=DEV)
    w0, h0 = imageops.jpeg_info(files[0])[1:]
    w1, h1 = imageops.jpeg_info(files[1])[1:]
    out = torch.empty(3 * (w0 * h0 + w1 * h1), dtype=torch.uint8, device=DEV)
    good_off = np.array([0, 3 * w0 * h0], dtype=np.int64)
    s = torch.cuda.current_stream().cuda_stream

    def call(host_=host, offs_=offs, out_off=good_off, ws_bytes=ws_n, src_bytes=src.numel(), out_bytes=out.numel(), B=2):
        return lib.lpi_jpeg_decode_u8(B, host_.ctypes.data, offs_.ctypes.data, src.data_ptr(), src_bytes, out_off.ctypes.data, out.data_ptr(), out_bytes,
                                      status.data_ptr(), ws.data_ptr(), ws_bytes, s)
    n0 = _lib.launch_count()
    broken = host.copy()
    broken[offs[1] + 4:offs[1] + 6] = 0xFF                    # the first segment length of file 1
    assert call(host_=broken) == -22
    assert call(offs_=np.array([0, 3, host.size], dtype=np.int64)) == -22
    assert call(out_off=np.array([0, out.numel() - 5], dtype=np.int64)) == -22
    assert call(ws_bytes=16) == -22
    assert call(src_bytes=host.size - 1) == -22
    assert call(B=0) == -22
    assert _lib.launch_count() == n0
    assert call() == 0
    torch.cuda.synchronize()
    assert _lib.launch_count() == n0 + 4 and status.tolist() == [0, 0]
    assert np.array_equal(out[:3 * w0 * h0].view(h0, w0, 3).cpu().numpy(), C.decode_pil(files[0]))


# ------------------------------------------------------------------------------------------------ the plugin on 'jpeg' against 'decoded'
@pytest.fixture(scope="module")
def jpeg_coco(tmp_path_factory):
    pytest.importorskip("PIL")
    from PIL import Image
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
def test_plugin_train_and_eval_jpeg_equals_decoded(jpeg_coco, synthetic_bpe, dtype):
    """Two train_epoch steps over a JPEG COCO folder, then the task keys (clustering) and _evaluate_retrieval: the 'jpeg' datasets (decode, crop /
    resize / flip on the GPU) and the 'decoded' ones (Pillow's decode on the host) under the same seed give bit-identical losses, gradients,
    parameters, score matrices and R@K."""
    from torch.utils.data import DataLoader
    from lpi_amd.retrieval.methods.sprompt import SPrompts
    root, S = str(jpeg_coco), synth.TINY.image_resolution
    got = {}
    for fmt in ("decoded", "jpeg"):
        tr = D.Coco(image_root=root, ann_file=str(jpeg_coco / "train.json"), tasks=[0], pixel_format=fmt, size=S)
        ev = D.CocoEval(image_root=root, ann_file=str(jpeg_coco / "val.json"), tasks=[0], pixel_format=fmt, size=S, resize=S + 4)
        collate = D.collate_decoded if fmt == "decoded" else D.collate_encoded
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
        loader = DataLoader(tr, batch_size=4, shuffle=False, num_workers=0, collate_fn=collate)
        m.train_epoch(loader, opt, 0, on_step=on_step)
        torch.cuda.synchronize()
        assert len(losses) == 2
        params = {k: getattr(net.prompts[0], k).detach().clone() for k in synth.PROMPT_NAMES}
        torch.manual_seed(1)
        m.clustering(DataLoader(tr, batch_size=4, shuffle=False, num_workers=0, collate_fn=collate))
        test_loader = DataLoader(ev, batch_size=3, shuffle=False, num_workers=0, pin_memory=True, collate_fn=collate)
        s_i2t, s_t2i, res = m._evaluate_retrieval(test_loader)
        got[fmt] = (losses, grads, params, [k.clone() for k in m.all_keys], s_i2t, s_t2i, res)
    a, b = got["decoded"], got["jpeg"]
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


def test_pipeline_encoded_slots_grow_and_match_direct_calls():
    """BatchPipeline over two passes whose batches differ in bytes (the slots grow), a fallback item included: every batch it hands out equals
    resample_encoded on the same EncodedBatch."""
    pytest.importorskip("PIL")
    from lpi_amd.pipeline import BatchPipeline

    class Epochs:
        def __init__(self, lists):
            self.lists, self.n = lists, 0

        def __iter__(self):
            self.n += 1
            return iter(self.lists[(self.n - 1) % len(self.lists)])

    def batches(files, seed):
        torch.manual_seed(seed)
        t = D.encoded_transform("train", 224)
        ids = torch.from_numpy(synth.token_ids(len(files), seed=seed))
        return [D.collate_encoded([(t(f),) for f in files[4 * j:4 * j + 4]]) + [ids[4 * j:4 * j + 4]] for j in range(len(files) // 4)]
    small = batches(C.random_files(21, 12, 16, 80), 1)
    big_files = C.random_files(22, 12, 200, 500)
    big_files[5] = odd_files()[0]
    large = batches(big_files, 2)
    assert large[1][0].fallback
    want = [[imageops.resample_encoded(b[0], device=DEV).cpu() for b in lst] for lst in (small, large)]
    pipe = BatchPipeline(Epochs([small, large]), DEV, None, depth=2, threads=3)
    for ep in range(2):
        n = 0
        for j, b in enumerate(pipe):
            assert b.images.dtype == torch.uint8 and tuple(b.images.shape) == (4, 3, 224, 224)
            assert torch.equal(b.images.cpu(), want[ep][j]), (ep, j)
            n += 1
        assert n == 3
    assert pipe._retired, "the second pass's larger batches grew the slots"


def test_rewritten_headers_decode_on_the_gpu():
    """SOF1, 16-bit quantisation tables, tables in another order: decoded by the GPU (status OK), byte for byte Pillow's."""
    pytest.importorskip("PIL")
    a = C.pixels(np.random.default_rng(1), 61, 37)
    files = []
    for sampling in ("4:4:4", "4:2:2", "4:2:0"):
        f = C.encode(a, sampling, 80, restart_marker_blocks=3 if sampling == "4:2:2" else 0)
        files += [C.rewrite(f, sof1=True), C.rewrite(f, dqt16=True), C.rewrite(f, reorder=True), C.rewrite(f, sof1=True, dqt16=True, reorder=True)]
    enc, dec = encoded_batch(files)
    assert not enc.fallback and gpu_statuses(enc) == [0] * len(files)
    got = imageops.decode_jpeg(enc, device=DEV)
    for i, f in enumerate(files):
        assert np.array_equal(got[i].cpu().numpy(), C.decode_pil(f)), i
    assert torch.equal(imageops.resample_encoded(enc, device=DEV).cpu(), imageops.resample_decoded(dec, device=DEV).cpu())


def test_resample_encoded_redoes_a_failed_file():
    """A file whose restart markers are out of order: Pillow (libjpeg's resynchronisation) decodes it, the GPU status is not OK, and
    resample_encoded decodes it again with Pillow and resamples the batch again: the batch equals resample_decoded of Pillow's pixels."""
    pytest.importorskip("PIL")
    rng = np.random.default_rng(12)
    good = C.encode(C.pixels(rng, 150, 90), "4:2:0", 85, restart_marker_blocks=2)
    files = [good, C.rst_out_of_order(good), C.encode(C.pixels(rng, 70, 120), "4:4:4", 60)]
    enc, dec = encoded_batch(files)
    assert not enc.fallback
    st = gpu_statuses(enc)
    assert st[0] == 0 and st[1] != 0 and st[2] == 0, st
    assert torch.equal(imageops.resample_encoded(enc, device=DEV).cpu(), imageops.resample_decoded(dec, device=DEV).cpu())
    assert np.array_equal(imageops.decode_jpeg(enc, device=DEV)[1].cpu().numpy(), C.decode_pil(files[1]))
