"""LPI_JPEG_LAYOUTS on a real MI355X: lpi_jpeg_decode_u8_x with the flag on 4:4:0, 4:1:1, 1x4, RGB, CMYK and YCCK files against Pillow and the
committed Pillow decodes (tests/golden/jpeg_layouts_pillow.npz), byte for byte, every status 0 and nothing left to the fallback; batches that mix
old and new kinds, and progressive files under both flags; invalid flags; flags = 0 against the old entry points; the plugin on a folder of such
files against pixel_format='decoded'."""
import ctypes
import hashlib
import io
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import jpeg_cases as C  # noqa: E402
import jpeg_layouts as L  # noqa: E402
import jpeg_progressive as P  # noqa: E402
from lpi_amd import _lib, imageops, synth  # noqa: E402
from lpi_amd.retrieval.utils import data as D  # noqa: E402

DEV = torch.device("cuda:0")
LAY, PROG = imageops.JPEG_LAYOUTS, imageops.JPEG_PROGRESSIVE


def encoded_batch(files, size=224, form="train", seed=0, **kw):
    """EncodedBatch of file bytes under the keywords kw of encoded_transform (GPU files stay encoded, the others are decoded by Pillow), and the
    DecodedBatch of the same files and draws."""
    torch.manual_seed(seed)
    enc = D.collate_encoded([(D.encoded_transform(form, size, **kw)(f),) for f in files])[0]
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
        assert np.array_equal(got[i].cpu().numpy(), C.decode_pil(f)), (i, L.parse(f)["ct"], L.parse(f)["comps"])
    if dec is not None:
        assert torch.equal(imageops.resample_encoded(enc, device=DEV).cpu(), imageops.resample_decoded(dec, device=DEV).cpu())


def raw_call(flags, files, ws_bytes=None):
    """lpi_jpeg_decode_u8_x through ctypes on fresh buffers: (return code, launches, workspace bytes, statuses, the output bytes, out offsets)."""
    lib = _lib.load()
    host = np.frombuffer(b"".join(files), np.uint8).copy()
    offs = np.concatenate(([0], np.cumsum([len(f) for f in files]))).astype(np.int64)
    wh = [C.decode_pil(f).shape[1::-1] for f in files]
    out_off = np.concatenate(([0], np.cumsum([3 * w * h for w, h in wh]))).astype(np.int64)
    n = ctypes.c_long(0)
    rc = lib.lpi_jpeg_decode_workspace_x(flags, len(files), host.ctypes.data, offs.ctypes.data, ctypes.addressof(n))
    if rc != 0:
        n.value = 4096
    ws = torch.zeros(n.value if ws_bytes is None else ws_bytes, dtype=torch.uint8, device=DEV)
    src = torch.from_numpy(host).to(DEV)
    out = torch.zeros(int(out_off[-1]), dtype=torch.uint8, device=DEV)
    status = torch.full((len(files),), -1, dtype=torch.int32, device=DEV)
    n0 = _lib.launch_count()
    rc2 = lib.lpi_jpeg_decode_u8_x(flags, len(files), host.ctypes.data, offs.ctypes.data, src.data_ptr(), src.numel(), out_off.ctypes.data,
                                   out.data_ptr(), out.numel(), status.data_ptr(), ws.data_ptr(), ws.numel(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return (rc or rc2), _lib.launch_count() - n0, n.value, status.tolist(), out.cpu(), out_off


def test_fixture_decodes_byte_for_byte(golden):
    g = golden("jpeg_layouts_pillow")
    n = len(g["offsets"]) - 1
    enc = D.EncodedBatch(torch.from_numpy(g["data"].copy()), torch.from_numpy(g["offsets"].copy()), torch.zeros((n, 9), dtype=torch.int64),
                         torch.from_numpy(g["wh"].copy()), 224, layouts=True)
    n0 = _lib.launch_count()
    got = imageops.decode_jpeg(enc, device=DEV)
    assert _lib.launch_count() - n0 == 5            # unstuff, huff for three and for four components, idct, colour
    assert gpu_statuses(enc) == [0] * n
    for i, px in enumerate(got):
        a = px.cpu().numpy()
        if f"pixels{i}" in g:
            assert np.array_equal(a, g[f"pixels{i}"]), (i, str(g["kind"][i]))
        else:
            assert hashlib.sha256(a.tobytes()).hexdigest() == str(g["sha256"][i]), (i, str(g["kind"][i]))


def test_seeded_files_of_every_kind_equal_pillow():
    """The 336 seeded files of the host suite in one batch through lpi_jpeg_decode_u8_x(4, ...): every status 0, Pillow's bytes."""
    pytest.importorskip("PIL")
    files = L.cases(78, 336)
    rc, launches, _, status, out, out_off = raw_call(LAY, files)
    assert rc == 0 and launches == 5 and status == [0] * len(files)
    for i, f in enumerate(files):
        want = C.decode_pil(f)
        assert np.array_equal(out[int(out_off[i]):int(out_off[i + 1])].view(want.shape).numpy(), want), (i, L.parse(f)["ct"], L.parse(f)["comps"])
    enc, dec = encoded_batch(files[:96], layouts=True)
    assert enc.layouts
    assert_equals_pillow(files[:96], enc, dec)


def test_h1v2_at_every_small_width():
    pytest.importorskip("PIL")
    rng = np.random.default_rng(12)
    files = [L.layout_file(rng, (1, 2), w, h, 90) if kind == "ycc" else L.colour_variant(kind, rng, (1, 2), w, h, 90)
             for w in (1, 2, 3, 4) for h in (1, 2, 3, 4, 15, 16, 17, 33) for kind in ("ycc", "cmyk", "ycck", "adobe 0")]
    enc, dec = encoded_batch(files, layouts=True)
    assert_equals_pillow(files, enc, dec)


def test_larger_files_of_the_new_kinds():
    """Photo-sized files, where every segment is cut into chunks for the speculative decoder: 4:4:0, 4:1:1, 1x4, CMYK and YCCK at 2x2 and 4x1, with
    and without restart intervals."""
    pytest.importorskip("PIL")
    rng = np.random.default_rng(640)
    files = [L.photo_like(rng, "4:4:0"), L.photo_like(rng, "4:1:1"), L.photo_like(rng, "1x4"), L.photo_like(rng, "cmyk"),
             L.colour_variant("ycck", rng, (4, 1), 613, 401, 92), L.colour_variant("cmyk no adobe", rng, (1, 2), 500, 333, 75, restart_marker_rows=1),
             L.colour_variant("ycck", rng, (2, 2), 320, 480, 85, restart_marker_blocks=7), L.layout_file(rng, (1, 4), 333, 517, 80, restart_marker_rows=2),
             L.colour_variant("adobe 0", rng, (4, 1), 640, 427, 88), L.colour_variant("keep_rgb", rng, (1, 1), 400, 300, 95)]
    enc, dec = encoded_batch(files, form="center", layouts=True)
    assert_equals_pillow(files, enc, dec)


def test_mixed_batch_old_kinds_new_kinds_and_fallbacks():
    pytest.importorskip("PIL")
    from PIL import Image
    rng = np.random.default_rng(3)
    a = C.pixels(rng, 77, 51)
    png = io.BytesIO()
    Image.fromarray(a).save(png, "PNG")
    files = [C.encode(a, "4:2:2", 70), L.layout_file(rng, (1, 2), 77, 51), L.colour_variant("cmyk", rng, (2, 2), 77, 51), C.encode(a, gray=True),
             png.getvalue(), L.colour_variant("ycck", rng, (1, 1), 40, 33), P.encode(a, "4:2:0", 80), C.encode(a, "4:4:4", 95, restart_marker_blocks=3),
             P.encode(a, gray=True, quality=85), L.layout_file(rng, (4, 1), 130, 9), P.cmyk_progressive(rng, 77, 51), C.encode(a, "4:2:0", 60)]
    enc, dec = encoded_batch(files, layouts=True)
    assert sorted(enc.fallback) == [4, 6, 8, 10]
    assert gpu_statuses(enc) == [0] * 8
    got = imageops.decode_jpeg(enc, device=DEV)
    for i, f in enumerate(files):
        assert np.array_equal(got[i].cpu().numpy(), C.decode_pil(f)), i
    assert torch.equal(imageops.resample_encoded(enc, device=DEV).cpu(), imageops.resample_decoded(dec, device=DEV).cpu())
    # the same files without the key: the new kinds are the worker's
    plain, _ = encoded_batch(files)
    assert sorted(plain.fallback) == [1, 2, 4, 5, 6, 8, 9, 10] and not plain.layouts
    # and with both keys the progressive YCbCr file is the GPU's, the progressive CMYK file still the host's
    both, dec2 = encoded_batch(files, layouts=True, progressive=True)
    assert sorted(both.fallback) == [4, 10] and both.layouts and both.progressive
    assert gpu_statuses(both) == [0] * 10
    assert torch.equal(imageops.resample_encoded(both, device=DEV).cpu(), imageops.resample_decoded(dec2, device=DEV).cpu())


def test_flags_five_progressive_beside_cmyk():
    pytest.importorskip("PIL")
    rng = np.random.default_rng(5)
    files = [P.encode(C.pixels(rng, 40, 30), "4:2:0", 80), L.colour_variant("cmyk", rng, (2, 2), 33, 20), L.layout_file(rng, (1, 2), 21, 40),
             C.encode(C.pixels(rng, 33, 20), "4:4:4", 80)]
    rc, launches, ws5, status, out, out_off = raw_call(LAY | PROG, files)
    assert rc == 0 and status == [0] * 4
    assert launches == 5 + 3 + 1            # the progressive path's 5 + R launches (Pillow's script: three rounds) and huff_kernel<4>
    for i, f in enumerate(files):
        want = C.decode_pil(f)
        assert np.array_equal(out[int(out_off[i]):int(out_off[i + 1])].view(want.shape).numpy(), want), i
    # each flag alone refuses the other's file, before any launch
    for flags in (0, PROG, LAY, 2, 3, 6, 7, -1):
        rc, launches, _, status, out, _ = raw_call(flags, files)
        assert rc == -22 and launches == 0 and status == [-1] * 4 and not out.any(), flags
    rc, launches, _, _, _, _ = raw_call(LAY | PROG, files, ws_bytes=ws5 - 1)
    assert rc == -22 and launches == 0


def test_flags_zero_and_four_on_todays_files():
    """Today's files: flags 0 gives the old entry point's bytes, workspace size, statuses and launch count, and so does flags 4."""
    pytest.importorskip("PIL")
    lib = _lib.load()
    files = C.random_files(11, 64)
    host = np.frombuffer(b"".join(files), np.uint8).copy()
    offs = np.concatenate(([0], np.cumsum([len(f) for f in files]))).astype(np.int64)
    wh = [imageops.jpeg_info(f)[1:] for f in files]
    out_off = np.concatenate(([0], np.cumsum([3 * w * h for w, h in wh]))).astype(np.int64)
    a, b, c = ctypes.c_long(0), ctypes.c_long(0), ctypes.c_long(0)
    assert lib.lpi_jpeg_decode_workspace(64, host.ctypes.data, offs.ctypes.data, ctypes.addressof(a)) == 0
    assert lib.lpi_jpeg_decode_workspace_x(0, 64, host.ctypes.data, offs.ctypes.data, ctypes.addressof(b)) == 0
    assert lib.lpi_jpeg_decode_workspace_x(LAY, 64, host.ctypes.data, offs.ctypes.data, ctypes.addressof(c)) == 0
    assert a.value == b.value == c.value
    src = torch.from_numpy(host).to(DEV)
    s = torch.cuda.current_stream().cuda_stream
    outs, sts = [], []
    for which in ("old", 0, LAY, LAY | PROG):
        ws = torch.zeros(a.value, dtype=torch.uint8, device=DEV)
        out = torch.zeros(int(out_off[-1]), dtype=torch.uint8, device=DEV)
        status = torch.full((64,), -1, dtype=torch.int32, device=DEV)
        n0 = _lib.launch_count()
        tail = (host.ctypes.data, offs.ctypes.data, src.data_ptr(), src.numel(), out_off.ctypes.data, out.data_ptr(), out.numel(), status.data_ptr(),
                ws.data_ptr(), ws.numel(), s)
        rc = lib.lpi_jpeg_decode_u8(64, *tail) if which == "old" else lib.lpi_jpeg_decode_u8_x(which, 64, *tail)
        torch.cuda.synchronize()
        assert rc == 0 and _lib.launch_count() == n0 + 4, which
        outs.append(out.cpu())
        sts.append(status.tolist())
    assert sts[0] == [0] * 64 and all(s_ == sts[0] for s_ in sts[1:])
    assert all(torch.equal(outs[0], o) for o in outs[1:])
    for i, f in enumerate(files):
        w, h = wh[i]
        assert np.array_equal(outs[1][int(out_off[i]):int(out_off[i + 1])].view(h, w, 3).numpy(), C.decode_pil(f)), i


def test_corrupt_files_of_the_new_kinds_give_pillows_result():
    """Flipped bits in the scan of a CMYK and of a 4:4:0 file, an RST out of order: Pillow's pixels (or its exception), whatever the kernel met."""
    pytest.importorskip("PIL")
    rng = np.random.default_rng(9)
    files = []
    for good in (L.colour_variant("cmyk", rng, (2, 2), 200, 120, 90), L.layout_file(rng, (1, 2), 200, 120, 90)):
        ent = L.parse(good)["ent"]
        flipped = bytearray(good)
        for pos in rng.integers(ent + 40, len(good) - 40, 6):
            flipped[pos] ^= 0x5A
            if flipped[pos] == 0xFF or flipped[pos - 1] == 0xFF:
                flipped[pos] = 0x5A
        files += [good, bytes(flipped)]
    files.append(C.rst_out_of_order(L.colour_variant("ycck", rng, (4, 1), 200, 120, 90, restart_marker_blocks=2)))
    for f in files:
        assert imageops.jpeg_info(f, layouts=True) == (True, 200, 120)
    offs = torch.tensor(np.concatenate(([0], np.cumsum([len(f) for f in files]))), dtype=torch.int64)
    enc = D.EncodedBatch(torch.frombuffer(bytearray(b"".join(files)), dtype=torch.uint8), offs, torch.tensor([[0, 0, 200, 120, 224, 224, 0, 0, 0]] * 5),
                         torch.tensor([[200, 120]] * 5), 224, layouts=True)
    st = gpu_statuses(enc)
    assert st[0] == 0 and st[2] == 0 and st[4] != 0, st
    for i, f in enumerate(files):
        one = D.EncodedBatch(enc.file(i).clone(), torch.tensor([0, len(f)]), enc.params[:1], enc.wh[:1], 224, layouts=True)
        try:
            want = C.decode_pil(f)
        except Exception as e:      # noqa: BLE001 — then decode_jpeg raises Pillow's exception
            with pytest.raises(type(e)):
                imageops.decode_jpeg(one, device=DEV)
            continue
        assert np.array_equal(imageops.decode_jpeg(one, device=DEV)[0].cpu().numpy(), want), (i, st)


# ------------------------------------------------------------------------------------------------ the plugin on 'jpeg' against 'decoded'
@pytest.fixture(scope="module")
def layouts_coco(tmp_path_factory):
    pytest.importorskip("PIL")
    root = tmp_path_factory.mktemp("coco_jpeg_layouts")
    rng = np.random.default_rng(11)
    train, val = [], []
    sizes = [(64, 48), (120, 90), (90, 130), (200, 150), (57, 61), (300, 40), (48, 64), (150, 150)]
    for i, (w, h) in enumerate(sizes):
        data = [L.layout_file(rng, (1, 2), w, h, 90), L.colour_variant("cmyk", rng, (2, 2), w, h, 90), L.layout_file(rng, (4, 1), w, h, 90),
                L.colour_variant("ycck", rng, (1, 2), w, h, 90), L.colour_variant("keep_rgb", rng, (1, 1), w, h, 90),
                L.layout_file(rng, (1, 4), w, h, 90), L.colour_variant("adobe 0", rng, (2, 1), w, h, 90), C.encode(C.pixels(rng, w, h), "4:2:0", 90)][i]
        (root / f"im{i}.jpg").write_bytes(data)
        train.append({"image": f"im{i}.jpg", "caption": f"a photo of thing number {i}", "category": 11, "image_id": f"coco_{i}"})
        val.append({"image": f"im{i}.jpg", "caption": [f"first caption {i}", f"second caption {i}"], "category": 11, "image_id": i})
    (root / "train.json").write_text(json.dumps(train))
    (root / "val.json").write_text(json.dumps(val))
    return root


def tiny_args(**over):
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
def test_plugin_train_and_eval_layouts_equals_decoded(layouts_coco, synthetic_bpe, dtype):
    """Two train_epoch steps over a folder of the new kinds, then the task keys (clustering) and _evaluate_retrieval: the 'jpeg' datasets with
    jpeg_layouts (every file decoded on the GPU, EncodedBatch.fallback empty) and the 'decoded' ones (Pillow's decode on the host) under the same
    seed give bit-identical losses, gradients, parameters, score matrices and R@K."""
    from torch.utils.data import DataLoader
    from lpi_amd.retrieval.methods.sprompt import SPrompts
    root, S = str(layouts_coco), synth.TINY.image_resolution
    got = {}
    for fmt in ("decoded", "jpeg"):
        kw = {"jpeg_layouts": True} if fmt == "jpeg" else {}
        tr = D.Coco(image_root=root, ann_file=str(layouts_coco / "train.json"), tasks=[0], pixel_format=fmt, size=S, **kw)
        ev = D.CocoEval(image_root=root, ann_file=str(layouts_coco / "val.json"), tasks=[0], pixel_format=fmt, size=S, resize=S + 4, **kw)
        collate = D.collate_decoded if fmt == "decoded" else D.collate_encoded
        if fmt == "jpeg":
            assert all(isinstance(tr[i][0], D.EncodedImage) for i in range(len(tr)))
            for ds, bs in ((tr, 4), (ev, 3)):
                assert all(b[0].layouts and not b[0].fallback for b in DataLoader(ds, batch_size=bs, shuffle=False, num_workers=0, collate_fn=collate))
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
    """BatchPipeline over batches of old and new kinds: every batch it hands out equals resample_encoded on the same EncodedBatch."""
    pytest.importorskip("PIL")
    from lpi_amd.pipeline import BatchPipeline
    files = [f for pair in zip(L.cases(21, 6), C.random_files(21, 6, 16, 200)) for f in pair]
    torch.manual_seed(1)
    t = D.encoded_transform("train", 224, layouts=True)
    ids = torch.from_numpy(synth.token_ids(len(files), seed=1))
    batches = [D.collate_encoded([(t(f),) for f in files[4 * j:4 * j + 4]]) + [ids[4 * j:4 * j + 4]] for j in range(3)]
    assert all(b[0].layouts and not b[0].fallback for b in batches)
    want = [imageops.resample_encoded(b[0], device=DEV).cpu() for b in batches]
    n = 0
    for j, b in enumerate(BatchPipeline(batches, DEV, None, depth=2, threads=3)):
        assert b.images.dtype == torch.uint8 and torch.equal(b.images.cpu(), want[j]), j
        n += 1
    assert n == 3
