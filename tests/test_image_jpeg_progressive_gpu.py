"""Progressive files in pixel_format='jpeg' on a real MI355X: lpi_jpeg_decode_u8_x with LPI_JPEG_PROGRESSIVE against the committed Pillow decodes
(tests/golden/jpeg_progressive_pillow.npz) and Pillow itself, byte for byte, every status 0 and nothing left to the fallback; mixed batches, corrupt
files, refusals, flags = 0 against the old entry points; the plugin on a folder of progressive files against pixel_format='decoded'."""
import ctypes
import hashlib
import io
import json

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import jpeg_cases as C  # noqa: E402
import jpeg_progressive as P  # noqa: E402
from lpi_amd import _lib, imageops, synth  # noqa: E402
from lpi_amd.retrieval.utils import data as D  # noqa: E402

DEV = torch.device("cuda:0")


def encoded_batch(files, size=224, form="train", seed=0, progressive=True):
    """EncodedBatch of file bytes under jpeg_progressive (GPU files stay encoded, the others are decoded by Pillow), and the DecodedBatch of the same
    files and draws."""
    torch.manual_seed(seed)
    enc = D.collate_encoded([(D.encoded_transform(form, size, progressive=progressive)(f),) for f in files])[0]
    torch.manual_seed(seed)
    dec_t = D.decoded_transform(form, size)
    dec = D.collate_decoded([(dec_t(D._pil().open(io.BytesIO(f)).convert("RGB")),) for f in files])[0]
    return enc, dec


def gpu_statuses(enc):
    d = imageops._issue_decode(enc, DEV, torch.cuda.current_stream())
    torch.cuda.synchronize()
    return d.status[:len(d.gpu)].tolist()


def assert_equals_pillow(files, enc, dec=None):
    """Every file decoded by the GPU (no fallback, every status 0) to Pillow's bytes."""
    assert not enc.fallback
    assert gpu_statuses(enc) == [0] * len(files)
    got = imageops.decode_jpeg(enc, device=DEV)
    for i, f in enumerate(files):
        assert np.array_equal(got[i].cpu().numpy(), C.decode_pil(f)), i
    if dec is not None:
        assert torch.equal(imageops.resample_encoded(enc, device=DEV).cpu(), imageops.resample_decoded(dec, device=DEV).cpu())


def test_fixture_decodes_byte_for_byte(golden):
    g = golden("jpeg_progressive_pillow")
    n = len(g["offsets"]) - 1
    enc = D.EncodedBatch(torch.from_numpy(g["data"].copy()), torch.from_numpy(g["offsets"].copy()), torch.zeros((n, 9), dtype=torch.int64),
                         torch.from_numpy(g["wh"].copy()), 224, progressive=True)
    n0 = _lib.launch_count()
    got = imageops.decode_jpeg(enc, device=DEV)
    assert _lib.launch_count() - n0 >= 8            # unstuff, huff, the scans' unstuff, three rounds of scans, idct, colour
    assert gpu_statuses(enc) == [0] * n
    for i, px in enumerate(got):
        a = px.cpu().numpy()
        if f"pixels{i}" in g:
            assert np.array_equal(a, g[f"pixels{i}"]), i
        else:
            assert hashlib.sha256(a.tobytes()).hexdigest() == str(g["sha256"][i]), i


def test_random_progressive_files_equal_pillow():
    pytest.importorskip("PIL")
    files = P.random_files(11, 256, 1, 400)
    enc, dec = encoded_batch(files)
    assert enc.progressive
    assert_equals_pillow(files, enc, dec)


def reencoded_files():
    rng = np.random.default_rng(31)
    out = []
    for sampling, gray in (("4:4:4", False), ("4:2:2", False), ("4:2:0", False), ("4:2:0", True)):
        for w, h in ((150, 90), (17, 33), (1, 1)):
            base = C.encode(C.pixels(rng, w, h), sampling, int(rng.integers(40, 96)), gray=gray)
            hdr, coef = P.baseline_coefficients(base)
            nc = len(hdr["comps"])
            for script in (P.spectral_script(nc), P.split_dc_script(nc), P.spectral_script(nc, (0, 5, 3, 0, 7)), P.split_dc_script(nc, (4, 0, 2))):
                out.append((base, P.reencode(hdr, coef, script)))
    return out


def test_reencoded_scripts_equal_pillow():
    """Spectral selection only, a DC scan per component, restart intervals that change and disappear between scans."""
    pytest.importorskip("PIL")
    pairs = reencoded_files()
    files = [f for _, f in pairs]
    enc, dec = encoded_batch(files)
    assert_equals_pillow(files, enc, dec)
    got = imageops.decode_jpeg(enc, device=DEV)
    for i, (base, _) in enumerate(pairs):
        assert np.array_equal(got[i].cpu().numpy(), C.decode_pil(base)), i


def test_batch_shaped_like_the_tool():
    """One batch of 32 progressive 640 x 480 q90 4:2:0 files (the shape tools/decode_pipeline_bench.py measures)."""
    pytest.importorskip("PIL")
    rng = np.random.default_rng(640)
    files = [P.encode(C.pixels(rng, 640, 480), "4:2:0", 90) for _ in range(32)]
    enc, dec = encoded_batch(files, form="center")
    assert_equals_pillow(files, enc, dec)


def test_mixed_batch_baseline_progressive_and_fallbacks():
    pytest.importorskip("PIL")
    from PIL import Image
    rng = np.random.default_rng(3)
    a = C.pixels(rng, 77, 51)
    png = io.BytesIO()
    Image.fromarray(a).save(png, "PNG")
    files = [C.encode(a, "4:2:2", 70), P.encode(a, "4:2:0", 80), P.cmyk_progressive(rng, 77, 51), P.encode(a[:40, :33], gray=True, quality=85),
             png.getvalue(), C.encode(a, "4:4:4", 95, restart_marker_blocks=3), P.encode(a, "4:4:4", 60, restart_marker_rows=1)]
    enc, dec = encoded_batch(files)
    assert sorted(enc.fallback) == [2, 4]
    assert gpu_statuses(enc) == [0] * 5
    got = imageops.decode_jpeg(enc, device=DEV)
    for i, f in enumerate(files):
        assert np.array_equal(got[i].cpu().numpy(), C.decode_pil(f)), i
    assert torch.equal(imageops.resample_encoded(enc, device=DEV).cpu(), imageops.resample_decoded(dec, device=DEV).cpu())
    # the same files without the key: the progressive ones are the worker's too
    plain, _ = encoded_batch(files, progressive=False)
    assert sorted(plain.fallback) == [1, 2, 3, 4, 6] and not plain.progressive


def test_corrupt_and_truncated_files_give_pillows_result():
    """Flipped bits in a middle scan, a file truncated inside its last scan, an RST out of order in a scan: the result is Pillow's pixels (or Pillow's
    exception), whatever the kernel met; the truncated file's status is not OK."""
    pytest.importorskip("PIL")
    rng = np.random.default_rng(9)
    good = P.encode(C.pixels(rng, 200, 120), "4:2:0", 90)
    scans = P.parse(good)["scans"]
    flipped = bytearray(good)
    mid = scans[5]
    for pos in rng.integers(mid["ent"] + 4, mid["end"] - 4, 6):
        flipped[pos] ^= 0x5A
        if flipped[pos] == 0xFF or flipped[pos - 1] == 0xFF:
            flipped[pos] = 0x5A             # no new marker: the scan structure stays what the parser saw
    last = scans[-1]
    truncated = good[:last["ent"] + (last["end"] - last["ent"]) // 2]
    with_rst = P.encode(C.pixels(rng, 200, 120), "4:2:0", 90, restart_marker_blocks=2)
    j = with_rst.index(b"\xff\xd0", P.parse(with_rst)["scans"][4]["ent"])
    rst = with_rst[:j + 1] + b"\xd1" + with_rst[j + 2:]
    files = [good, bytes(flipped), truncated, with_rst, rst, good]
    for f in files:
        assert imageops.jpeg_info(f, progressive=True) == (True, 200, 120)
    enc = D.EncodedBatch(torch.frombuffer(bytearray(b"".join(files)), dtype=torch.uint8),
                         torch.tensor(np.concatenate(([0], np.cumsum([len(f) for f in files]))), dtype=torch.int64),
                         torch.tensor([[0, 0, 200, 120, 224, 224, 0, 0, 0]] * 6), torch.tensor([[200, 120]] * 6), 224, progressive=True)
    st = gpu_statuses(enc)
    assert st[0] == 0 and st[3] == 0 and st[5] == 0 and st[2] != 0 and st[4] != 0, st
    for i, f in enumerate(files):
        one = D.EncodedBatch(enc.file(i).clone(), torch.tensor([0, len(f)]), enc.params[:1], enc.wh[:1], 224, progressive=True)
        try:
            want = C.decode_pil(f)
        except Exception as e:      # noqa: BLE001 — then decode_jpeg raises Pillow's exception
            with pytest.raises(type(e)):
                imageops.decode_jpeg(one, device=DEV)
            continue
        assert np.array_equal(imageops.decode_jpeg(one, device=DEV)[0].cpu().numpy(), want), (i, st)


def test_invalid_calls_return_einval_before_any_launch():
    pytest.importorskip("PIL")
    lib = _lib.load()
    rng = np.random.default_rng(5)
    files = [P.encode(C.pixels(rng, 40, 30), "4:2:0", 80), C.encode(C.pixels(rng, 33, 20), "4:4:4", 80)]
    host = np.frombuffer(b"".join(files), np.uint8).copy()
    offs = np.array([0, len(files[0]), host.size], dtype=np.int64)
    src = torch.from_numpy(host).to(DEV)
    ws_n = imageops.jpeg_workspace_bytes(host, offs, progressive=True)
    ws = torch.empty(ws_n, dtype=torch.uint8, device=DEV)
    status = torch.empty(2, dtype=torch.int32, device=DEV)
    out = torch.empty(3 * (40 * 30 + 33 * 20), dtype=torch.uint8, device=DEV)
    out_off = np.array([0, 3 * 40 * 30], dtype=np.int64)
    s = torch.cuda.current_stream().cuda_stream

    def call(flags=1, host_=host, offs_=offs, ws_bytes=ws_n):
        return lib.lpi_jpeg_decode_u8_x(flags, 2, host_.ctypes.data, offs_.ctypes.data, src.data_ptr(), src.numel(), out_off.ctypes.data, out.data_ptr(),
                                        out.numel(), status.data_ptr(), ws.data_ptr(), ws_bytes, s)
    head, sc, _ = P.chunks(files[0])
    cut = P.join(head, sc[:-1])                                     # an incomplete script
    cut_host = np.frombuffer(cut + files[1], np.uint8).copy()
    cut_offs = np.array([0, len(cut), cut_host.size], dtype=np.int64)
    n0 = _lib.launch_count()
    assert call(flags=2) == -22 and call(flags=3) == -22 and call(flags=-1) == -22       # unknown flag bits
    assert call(flags=0) == -22                                     # a progressive file without the flag
    assert call(host_=cut_host, offs_=cut_offs) == -22
    assert call(ws_bytes=ws_n - 1) == -22
    assert _lib.launch_count() == n0
    assert call() == 0
    torch.cuda.synchronize()
    assert _lib.launch_count() == n0 + 5 + 3 and status.tolist() == [0, 0]       # Pillow's script runs in three rounds
    assert np.array_equal(out[:3 * 40 * 30].view(30, 40, 3).cpu().numpy(), C.decode_pil(files[0]))
    assert np.array_equal(out[3 * 40 * 30:].view(20, 33, 3).cpu().numpy(), C.decode_pil(files[1]))


def test_flags_zero_is_the_old_entry_point():
    """flags = 0 through the _x entry points: the old entry points' bytes, workspace size, statuses and launches on baseline files."""
    pytest.importorskip("PIL")
    lib = _lib.load()
    files = C.random_files(11, 64)
    host = np.frombuffer(b"".join(files), np.uint8).copy()
    offs = np.concatenate(([0], np.cumsum([len(f) for f in files]))).astype(np.int64)
    wh = [imageops.jpeg_info(f)[1:] for f in files]
    out_off = np.concatenate(([0], np.cumsum([3 * w * h for w, h in wh]))).astype(np.int64)
    a, b = ctypes.c_long(0), ctypes.c_long(0)
    assert lib.lpi_jpeg_decode_workspace(64, host.ctypes.data, offs.ctypes.data, ctypes.addressof(a)) == 0
    assert lib.lpi_jpeg_decode_workspace_x(0, 64, host.ctypes.data, offs.ctypes.data, ctypes.addressof(b)) == 0
    assert a.value == b.value
    src = torch.from_numpy(host).to(DEV)
    s = torch.cuda.current_stream().cuda_stream
    outs, sts = [], []
    for which in ("old", "x0", "x1"):
        ws = torch.zeros(a.value, dtype=torch.uint8, device=DEV)
        out = torch.zeros(int(out_off[-1]), dtype=torch.uint8, device=DEV)
        status = torch.full((64,), -1, dtype=torch.int32, device=DEV)
        n0 = _lib.launch_count()
        tail = (host.ctypes.data, offs.ctypes.data, src.data_ptr(), src.numel(), out_off.ctypes.data, out.data_ptr(), out.numel(), status.data_ptr(),
                ws.data_ptr(), ws.numel(), s)
        rc = lib.lpi_jpeg_decode_u8(64, *tail) if which == "old" else lib.lpi_jpeg_decode_u8_x(0 if which == "x0" else 1, 64, *tail)
        torch.cuda.synchronize()
        assert rc == 0 and _lib.launch_count() == n0 + 4, which
        outs.append(out.cpu())
        sts.append(status.tolist())
    assert sts[0] == [0] * 64 and sts[1] == sts[0] and sts[2] == sts[0]
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2])
    for i, f in enumerate(files):
        w, h = wh[i]
        assert np.array_equal(outs[1][int(out_off[i]):int(out_off[i + 1])].view(h, w, 3).numpy(), C.decode_pil(f)), i


# ------------------------------------------------------------------------------------------------ the plugin on 'jpeg' against 'decoded'
@pytest.fixture(scope="module")
def progressive_coco(tmp_path_factory):
    pytest.importorskip("PIL")
    root = tmp_path_factory.mktemp("coco_jpeg_progressive")
    rng = np.random.default_rng(11)
    train, val = [], []
    sizes = [(64, 48), (120, 90), (90, 130), (200, 150), (57, 61), (300, 40), (48, 64), (150, 150)]
    for i, (w, h) in enumerate(sizes):
        (root / f"im{i}.jpg").write_bytes(P.encode(rng.integers(0, 256, (h, w, 3), dtype=np.uint8), ("4:2:0", "4:4:4", "4:2:2")[i % 3], 90, gray=i == 6))
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
def test_plugin_train_and_eval_progressive_equals_decoded(progressive_coco, synthetic_bpe, dtype):
    """Two train_epoch steps over a folder of progressive files, then the task keys (clustering) and _evaluate_retrieval: the 'jpeg' datasets with
    jpeg_progressive (every file decoded on the GPU) and the 'decoded' ones (Pillow's decode on the host) under the same seed give bit-identical
    losses, gradients, parameters, score matrices and R@K."""
    from torch.utils.data import DataLoader
    from lpi_amd.retrieval.methods.sprompt import SPrompts
    root, S = str(progressive_coco), synth.TINY.image_resolution
    got = {}
    for fmt in ("decoded", "jpeg"):
        kw = {"jpeg_progressive": True} if fmt == "jpeg" else {}
        tr = D.Coco(image_root=root, ann_file=str(progressive_coco / "train.json"), tasks=[0], pixel_format=fmt, size=S, **kw)
        ev = D.CocoEval(image_root=root, ann_file=str(progressive_coco / "val.json"), tasks=[0], pixel_format=fmt, size=S, resize=S + 4, **kw)
        if fmt == "jpeg":
            assert all(isinstance(tr[i][0], D.EncodedImage) for i in range(len(tr)))
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


def test_pipeline_encoded_slots_keep_the_flag():
    """BatchPipeline over batches of progressive and baseline files: every batch it hands out equals resample_encoded on the same EncodedBatch."""
    pytest.importorskip("PIL")
    from lpi_amd.pipeline import BatchPipeline
    files = [f for pair in zip(P.random_files(21, 6, 16, 200), C.random_files(21, 6, 16, 200)) for f in pair]
    torch.manual_seed(1)
    t = D.encoded_transform("train", 224, progressive=True)
    ids = torch.from_numpy(synth.token_ids(len(files), seed=1))
    batches = [D.collate_encoded([(t(f),) for f in files[4 * j:4 * j + 4]]) + [ids[4 * j:4 * j + 4]] for j in range(3)]
    assert all(b[0].progressive and not b[0].fallback for b in batches)
    want = [imageops.resample_encoded(b[0], device=DEV).cpu() for b in batches]
    n = 0
    for j, b in enumerate(BatchPipeline(batches, DEV, None, depth=2, threads=3)):
        assert b.images.dtype == torch.uint8 and torch.equal(b.images.cpu(), want[j]), j
        n += 1
    assert n == 3
