"""pixel_format='jpeg' without a GPU: the numpy restatement of Pillow's baseline decode (tests/jpeg_restate.py) against Pillow and the committed
fixture; the host parser (lpi_jpeg_info through ctypes): frame sizes, envelope verdicts, LPI_EINVAL on broken headers; the data layer's
EncodedImage / EncodedBatch and its crop draws."""
import ctypes
import hashlib
import io
import json
import pickle

import numpy as np
import pytest
import torch

import jpeg_cases as C
import jpeg_restate as J
from lpi_amd import _lib, imageops
from lpi_amd.retrieval.utils import data as D


def files_of(g):
    return [bytes(g["data"][g["offsets"][i]:g["offsets"][i + 1]]) for i in range(len(g["offsets"]) - 1)]


def test_restatement_equals_fixture(golden):
    g = golden("jpeg_pillow")
    assert str(g["pillow"]).startswith("12.") and str(g["libjpeg_turbo"]).startswith("3.")
    full = digests = 0
    for i, f in enumerate(files_of(g)):
        w, h = (int(v) for v in g["wh"][i])
        if w * h > 201 * 250:
            continue            # plain-Python entropy decoding: the three largest files are the GPU suite's
        a = J.decode(f)
        assert a.shape == (h, w, 3)
        if f"pixels{i}" in g:
            assert np.array_equal(a, g[f"pixels{i}"]), i
            full += 1
        else:
            assert hashlib.sha256(a.tobytes()).hexdigest() == str(g["sha256"][i]), i
            digests += 1
    assert full == 48 and digests == 1


@pytest.mark.parametrize("sampling", ["4:4:4", "4:2:2", "4:2:0", "gray"])
def test_restatement_equals_pillow(sampling):
    pytest.importorskip("PIL")
    rng = np.random.default_rng(len(sampling) + (sampling == "gray"))
    n = 0
    for q in (30, 55, 75, 90, 100):
        for w, h in [(1, 1), (2, 3), (3, 2), (4, 5), (5, 4), (7, 9), (16, 16), (17, 33), (40, 23), (33, 40), (1, 40), (40, 1), (6, 2), (2, 6)]:
            for kw in ({}, {"optimize": True}, {"restart_marker_blocks": 1}, {"restart_marker_rows": 1}):
                f = C.encode(C.pixels(rng, w, h), "4:2:0" if sampling == "gray" else sampling, q, gray=sampling == "gray", **kw)
                if kw.get("restart_marker_blocks"):
                    assert J.parse(f)["ri"] > 0
                assert np.array_equal(J.decode(f), C.decode_pil(f)), (q, w, h, kw)
                n += 1
    assert n == 280


def odd(kind):
    from PIL import Image
    a = C.pixels(np.random.default_rng(4), 50, 30)
    b = io.BytesIO()
    if kind == "progressive":
        Image.fromarray(a).save(b, "JPEG", progressive=True)
    elif kind == "cmyk":
        Image.fromarray(a).convert("CMYK").save(b, "JPEG")
    elif kind == "png":
        Image.fromarray(a).save(b, "PNG")
    return b.getvalue()


def adobe(f):
    """f with an Adobe APP14 segment (transform 1) after SOI and its JFIF APP0 removed."""
    L = (f[4] << 8) | f[5]
    body = f[4 + L:] if f[2:4] == b"\xff\xe0" else f[2:]
    seg = b"Adobe" + bytes([0, 100, 0, 0, 0, 0, 1])
    return f[:2] + b"\xff\xee" + (len(seg) + 2).to_bytes(2, "big") + seg + body


def test_parser_frame_sizes_and_verdicts():
    pytest.importorskip("PIL")
    a = C.pixels(np.random.default_rng(4), 50, 30)
    assert imageops.jpeg_info(odd("progressive")) == (False, 50, 30)
    assert imageops.jpeg_info(odd("cmyk")) == (False, 50, 30)
    assert imageops.jpeg_info(odd("png")) == (False, 0, 0)
    assert imageops.jpeg_info(C.encode(a, gray=True)) == (True, 50, 30)
    assert imageops.jpeg_info(C.encode(a, "4:2:2", restart_marker_blocks=3)) == (True, 50, 30)
    assert imageops.jpeg_info(adobe(C.encode(a))) == (False, 50, 30)
    assert C.decode_pil(adobe(C.encode(a))).shape == (30, 50, 3)
    f = bytearray(C.encode(a, "4:4:4"))
    sof = f.index(b"\xff\xc0")
    f[sof + 11] = 0x41                   # luma 4 x 1: 4:1:1
    assert imageops.jpeg_info(bytes(f)) == (False, 50, 30)
    info = (ctypes.c_long * imageops.JPEG_INFO)()
    g = C.encode(a, "4:2:0", restart_marker_rows=1)
    assert _lib.load().lpi_jpeg_info(np.frombuffer(g, np.uint8).ctypes.data, len(g), ctypes.addressof(info)) == 0
    assert list(info)[:7] == [1, 50, 30, 3, 2, 2, 4] and info[7] == J.parse(g)["ent"]


def test_parser_einval_on_broken_headers():
    a = C.pixels(np.random.default_rng(5), 40, 24)
    f = C.encode(a)
    sos = f.index(b"\xff\xda")
    assert imageops.jpeg_info(f[:sos - 30]) is None                        # truncated header
    bad = bytearray(f)
    bad[4:6] = b"\xff\xf0"                                                 # APP0 length past the end
    assert imageops.jpeg_info(bytes(bad)) is None
    bad = bytearray(f)
    bad[sos + 6] = 0x33                                                    # the scan's first component names DC / AC table 3: never defined
    assert imageops.jpeg_info(bytes(bad)) is None
    garbage = b"\xff\xd8" + np.random.default_rng(6).integers(0, 256, 400, dtype=np.uint8).tobytes()
    assert imageops.jpeg_info(garbage) is None
    with pytest.raises(_lib.LpiError):
        imageops.jpeg_workspace_bytes(np.frombuffer(garbage, np.uint8), np.array([0, len(garbage)]))


@pytest.fixture(scope="module")
def coco(tmp_path_factory):
    pytest.importorskip("PIL")
    root = tmp_path_factory.mktemp("coco_jpeg_host")
    rng = np.random.default_rng(12)
    train = []
    names = []
    for i, (w, h) in enumerate([(64, 48), (120, 90), (90, 130), (57, 61), (300, 40), (48, 64)]):
        a = C.pixels(rng, w, h)
        data = C.encode(a, ("4:4:4", "4:2:2", "4:2:0")[i % 3], 80, gray=i == 5)
        if i == 2:
            data = odd("progressive")
        if i == 4:
            data = odd("png")
        (root / f"im{i}.jpg").write_bytes(data)
        names.append(f"im{i}.jpg")
        train.append({"image": f"im{i}.jpg", "caption": f"a photo of thing {i}", "category": 11, "image_id": i})
    (root / "train.json").write_text(json.dumps(train))
    (root / "val.json").write_text(json.dumps([dict(t, caption=[t["caption"]]) for t in train]))
    return root


def same_item(x, y):
    assert type(x) is type(y)
    if isinstance(x, D.EncodedImage):
        assert torch.equal(x.data, y.data) and x.params == y.params and x.wh == y.wh and x.size == y.size
    else:
        assert torch.equal(x.pixels, y.pixels) and x.params == y.params


def test_coco_jpeg_items_carry_the_decoded_crop_params(coco):
    for cls, ann in ((D.Coco, "train.json"), (D.CocoEval, "val.json")):
        kw = {} if cls is D.Coco else {"eval_transform": "center"}
        torch.manual_seed(3)
        jp = [cls(image_root=str(coco), ann_file=str(coco / ann), tasks=[0], pixel_format="jpeg", **kw)[i][0] for i in range(6)]
        torch.manual_seed(3)
        de = [cls(image_root=str(coco), ann_file=str(coco / ann), tasks=[0], pixel_format="decoded", **kw)[i][0] for i in range(6)]
        assert [type(x).__name__ for x in jp] == ["EncodedImage", "EncodedImage", "DecodedImage", "EncodedImage", "DecodedImage", "EncodedImage"]
        assert [x.params for x in jp] == [x.params for x in de]
        for x, y in zip(jp, de):
            if isinstance(x, D.DecodedImage):
                assert torch.equal(x.pixels, y.pixels)
            else:
                assert x.wh == (int(y.pixels.shape[1]), int(y.pixels.shape[0]))
    with pytest.raises(ValueError):
        D.SyntheticCoco(4, [0], pixel_format="jpeg")


def test_coco_jpeg_workers_equal_single_process(coco):
    from torch.utils.data import DataLoader
    ds = D.Coco(image_root=str(coco), ann_file=str(coco / "train.json"), tasks=[0], pixel_format="jpeg")
    got = []
    for workers in (0, 2):
        torch.manual_seed(0)
        loader = DataLoader(ds, batch_size=3, shuffle=False, num_workers=workers, collate_fn=D.collate_encoded,
                            generator=torch.Generator().manual_seed(0), worker_init_fn=lambda w: torch.manual_seed(100 + w))
        got.append(list(loader))
    # the crop draws come from each process's torch RNG: the draws-free parts equal the single-process ones, and the params equal a replay of the
    # workers' RNG streams (batch b is worker b % 2's, seeded by worker_init_fn)
    t = D.encoded_transform("train", 224)
    rng_state, replay = {}, []
    for b in range(len(got[1])):
        w = b % 2
        if w in rng_state:
            torch.set_rng_state(rng_state[w])
        else:
            torch.manual_seed(100 + w)
        replay.append([t(D._read(str(coco), ds.annotation[i]["image"])).params for i in range(3 * b, min(3 * b + 3, len(ds)))])
        rng_state[w] = torch.get_rng_state()
    for b, (a, c) in enumerate(zip(*got)):
        ea, eb = a[0], c[0]
        assert torch.equal(ea.data, eb.data) and torch.equal(ea.offsets, eb.offsets) and torch.equal(ea.wh, eb.wh)
        assert sorted(ea.fallback) == sorted(eb.fallback) and all(torch.equal(ea.fallback[i], eb.fallback[i]) for i in ea.fallback)
        assert list(a[1]) == list(c[1])
        assert [tuple(r) for r in eb.params.tolist()] == replay[b], b


def test_encoded_batch_pickles_as_one_tensor():
    pytest.importorskip("PIL")
    files = C.random_files(8, 6, 8, 60)
    torch.manual_seed(0)
    t = D.encoded_transform("train", 32)
    batch = D.collate_encoded([(t(f), i) for i, f in enumerate(files)])
    enc = batch[0]
    assert isinstance(enc, D.EncodedBatch) and len(enc) == 6 and not enc.fallback
    args = enc.__reduce__()[1]
    assert [a for a in args if torch.is_tensor(a) and a.dtype == torch.uint8] == [enc.data]
    assert enc.data.numel() == sum(len(f) for f in files)
    for i, f in enumerate(files):
        assert bytes(enc.file(i).numpy()) == f
    back = pickle.loads(pickle.dumps(enc))
    assert torch.equal(back.data, enc.data) and torch.equal(back.params, enc.params) and back.size == 32
    assert torch.equal(batch[1], torch.arange(6))


def test_rewritten_headers_inside_the_envelope():
    """SOF1, 16-bit quantisation tables, tables in another order (one per segment, Huffman tables before the frame, a COM between): inside the
    envelope, and the restatement equals Pillow on them.  A scan listing the components in another order than the frame is outside: libjpeg-turbo
    refuses it (Pillow raises), so the loader's Pillow decode has the last word."""
    pytest.importorskip("PIL")
    a = C.pixels(np.random.default_rng(1), 61, 37)
    for sampling in ("4:4:4", "4:2:2", "4:2:0"):
        f = C.encode(a, sampling, 80)
        for kw in ({"sof1": True}, {"dqt16": True}, {"reorder": True}, {"sof1": True, "dqt16": True, "reorder": True}):
            g = C.rewrite(f, **kw)
            assert imageops.jpeg_info(g) == (True, 61, 37), kw
            assert np.array_equal(J.decode(g), C.decode_pil(g)) and np.array_equal(C.decode_pil(g), C.decode_pil(f)), kw
        g = C.rewrite(f, swap_scan=True)
        assert imageops.jpeg_info(g) == (False, 61, 37)
        with pytest.raises(OSError):
            D.encoded_transform("train", 32)(g)
