"""LPI_JPEG_LAYOUTS without a GPU: the numpy restatement of the wider envelope (tests/jpeg_layouts.py: 4:4:0, 4:1:1, 1x4, RGB, CMYK, YCCK) against
Pillow and the committed fixture; the host parser's verdicts through lpi_jpeg_info_x with and without the flag; workspace sizes; the data layer's
jpeg_layouts keyword and config key."""
import ctypes
import hashlib
import json
import os
import pickle

import numpy as np
import pytest
import torch

import jpeg_cases as C
import jpeg_layouts as L
import jpeg_progressive as P
from lpi_amd import _lib, imageops
from lpi_amd.retrieval.utils import data as D

LAY, PROG = imageops.JPEG_LAYOUTS, imageops.JPEG_PROGRESSIVE


def info_x(f, flags):
    """(return code, the LPI_JPEG_INFO_X fields) of lpi_jpeg_info_x."""
    a = np.frombuffer(bytes(f), np.uint8)
    x = (ctypes.c_long * imageops.JPEG_INFO_X)()
    rc = _lib.load().lpi_jpeg_info_x(flags, a.ctypes.data, int(a.size), ctypes.addressof(x))
    return rc, list(x)


def packed(files):
    return (np.frombuffer(b"".join(files), np.uint8), np.concatenate(([0], np.cumsum([len(f) for f in files]))).astype(np.int64))


def today(hdr):
    """The file is inside the envelope without the flag (which refuses an Adobe APP14 without a JFIF APP0 whatever its transform says)."""
    return hdr["ct"] == "ycc" and hdr["comps"][0][1:3] in ((1, 1), (2, 1), (2, 2)) and (hdr["jfif"] or hdr["adobe"] is None)


def test_the_flag_is_bit_two():
    assert LAY == 4 and L.LAYOUTS == 4 and PROG == 1


def test_restatement_equals_pillow_on_seeded_files():
    """336 seeded files: the six geometries, each as YCbCr, as RGB by every marking, as CMYK (with and without the Adobe marker) and as YCCK; sizes
    from 1 x 1, every residue inside the last MCU among them; qualities 30-95; restart intervals; optimised tables.  The parser admits each under
    the flag and, unless it is one of today's files, refuses it without."""
    pytest.importorskip("PIL")
    rng = np.random.default_rng(78)
    kinds, ri = set(), set()
    for i in range(336):
        f = L.case(i, rng)
        hdr = L.parse(f)
        kinds.add((hdr["ct"], hdr["comps"][0][1:3]))
        ri.add((len(hdr["comps"]), hdr["ri"] > 0))
        assert imageops.jpeg_info(f, layouts=True) == (True, hdr["w"], hdr["h"]), i
        assert imageops.jpeg_info(f) == (today(hdr), hdr["w"], hdr["h"]), i
        assert np.array_equal(L.decode(f), C.decode_pil(f)), (i, hdr["ct"], hdr["comps"])
    assert kinds == {(ct, hv) for ct in ("ycc", "rgb", "cmyk", "ycck") for hv in L.GEOMETRIES}
    assert ri == {(3, False), (3, True), (4, False), (4, True)}


def test_h1v2_has_no_width_condition():
    """h2v1 and h2v2 replicate when the downsampled plane is at most 2 wide; h1v2 filters at every width — 1 and 2 among them — and at every height."""
    pytest.importorskip("PIL")
    rng = np.random.default_rng(12)
    n = 0
    for w in (1, 2, 3, 4):
        for h in (1, 2, 3, 4, 15, 16, 17, 33):
            for kind in ("ycc", "cmyk", "ycck", "adobe 0"):
                f = L.layout_file(rng, (1, 2), w, h, 90) if kind == "ycc" else L.colour_variant(kind, rng, (1, 2), w, h, 90)
                assert imageops.jpeg_info(f, layouts=True) == (True, w, h)
                assert np.array_equal(L.decode(f), C.decode_pil(f)), (w, h, kind)
                n += 1
    assert n == 128


def test_cmyk_formula_on_every_pair():
    """Pillow's convert("RGB") of every (c, k) pair against the integer formula the kernel uses."""
    from PIL import Image
    c, k = np.meshgrid(np.arange(256, dtype=np.uint8), np.arange(256, dtype=np.uint8))
    im = np.stack([c, c, c, k], axis=-1)
    want = np.asarray(Image.fromarray(im, "CMYK").convert("RGB"))
    got = L.cmyk_to_rgb(*(im[..., i].astype(np.int64) for i in range(4)))
    assert np.array_equal(got, want)


def test_restatement_equals_fixture(golden):
    g = golden("jpeg_layouts_pillow")
    assert str(g["pillow"]).startswith("12.") and str(g["libjpeg_turbo"]).startswith("3.")
    n = len(g["offsets"]) - 1
    assert n == 76
    here = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
    assert os.path.getsize(os.path.join(here, "jpeg_layouts_pillow.npz")) <= os.path.getsize(os.path.join(here, "jpeg_progressive_pillow.npz"))
    full, seen = 0, set()
    for i in range(n):
        f = bytes(g["data"][g["offsets"][i]:g["offsets"][i + 1]])
        w, h = (int(v) for v in g["wh"][i])
        hdr = L.parse(f)
        seen.add((str(g["kind"][i]), hdr["comps"][0][1:3]))
        assert info_x(f, LAY)[1][:6] == [1, w, h, len(hdr["comps"]), hdr["comps"][0][1], hdr["comps"][0][2]]
        if f"pixels{i}" not in g:
            continue                # the four large files are the GPU suite's
        a = L.decode(f)
        assert np.array_equal(a, g[f"pixels{i}"]) and hashlib.sha256(a.tobytes()).hexdigest() == str(g["sha256"][i]), i
        full += 1
    assert full == 72
    assert {k for k, _ in seen} == {"ycc", *L.COLOUR_VARIANTS} and {hv for _, hv in seen} == set(L.GEOMETRIES)


def one_of_each(rng, w=45, h=27):
    """{name: file} with one file of every kind the flag adds."""
    out = {f"ycc {H}x{V}": L.layout_file(rng, (H, V), w, h) for H, V in ((1, 2), (4, 1), (1, 4))}
    for kind in L.COLOUR_VARIANTS:
        for hv in ((1, 1), (2, 2), (1, 2), (4, 1)):
            out[f"{kind} {hv[0]}x{hv[1]}"] = L.colour_variant(kind, rng, hv, w, h)
    return out


def test_parser_verdicts_with_and_without_the_flag():
    pytest.importorskip("PIL")
    rng = np.random.default_rng(21)
    for name, f in one_of_each(rng).items():
        hdr = L.parse(f)
        nc, (H, V) = len(hdr["comps"]), hdr["comps"][0][1:3]
        rc, x = info_x(f, LAY)
        assert rc == 0 and x[:6] == [1, 45, 27, nc, H, V] and x[8:] == [0, 1], name
        assert info_x(f, LAY | PROG)[1] == x, name
        rc, y = info_x(f, 0)
        # without the flag: the verdict of today ('adobe 1' without JFIF, and keep_rgb, were refused whatever their sampling), and 1 x 1 reported
        # for a four-component file as ever
        assert rc == 0 and y[0] == 0 and y[1:4] == [45, 27, nc] and y[4:6] == ([H, V] if nc == 3 else [1, 1]), name
        assert info_x(f, PROG)[1] == y, name
        assert C.decode_pil(f).shape == (27, 45, 3), name


def test_parser_refuses_what_the_envelope_names():
    """Other factors, a later component that is not 1 x 1, fractional ratios (Pillow raises), 12-bit, arithmetic coding, two components, a scan that
    holds one component of three; a progressive CMYK or 4:4:0 file under both flags."""
    pytest.importorskip("PIL")
    rng = np.random.default_rng(22)
    for name, f in L.outside(rng).items():
        for flags in (0, LAY, LAY | PROG):
            rc, x = info_x(f, flags)
            assert rc == 0 and x[0] == 0, (name, flags)
        with pytest.raises(imageops._lib.LpiError):
            imageops.jpeg_workspace_bytes(*packed([f]), layouts=True)
        if name.startswith("fractional"):
            with pytest.raises(OSError):
                C.decode_pil(f)
    cmyk = P.cmyk_progressive(rng)
    assert info_x(cmyk, LAY | PROG)[1][0] == 0 and info_x(cmyk, LAY)[1][0] == 0 and C.decode_pil(cmyk).shape == (24, 40, 3)
    # a progressive 4:4:0 file: Pillow's progressive 4:2:2 file with the frame rewritten (the frame rule is checked before any scan)
    f = P.encode(C.pixels(rng, 32, 16), "4:2:2", 80)
    at = next(s[0] for s in P.walk(f) if s[1] == 0xC2) + 4
    f440 = f[:at + 1] + (32).to_bytes(2, "big") + (16).to_bytes(2, "big") + f[at + 5:at + 7] + b"\x12" + f[at + 8:]
    assert info_x(f, LAY | PROG)[1][0] == 1 and info_x(f440, LAY | PROG)[1][:3] == [0, 16, 32]
    # and a progressive file of today's kinds is admitted under both flags as under LPI_JPEG_PROGRESSIVE alone
    for g in P.random_files(5, 12, 1, 60):
        assert info_x(g, LAY | PROG) == info_x(g, PROG) and info_x(g, LAY)[1][0] == 0


def test_invalid_flags_are_einval():
    pytest.importorskip("PIL")
    f = C.encode(C.pixels(np.random.default_rng(1), 20, 12))
    a, o = packed([f])
    out = ctypes.c_long(0)
    for flags in (2, 3, 6, 7, -1):
        assert info_x(f, flags)[0] == -22, flags
        assert _lib.load().lpi_jpeg_decode_workspace_x(flags, 1, a.ctypes.data, o.ctypes.data, ctypes.addressof(out)) == -22, flags
    for flags in (0, 1, 4, 5):
        assert info_x(f, flags)[0] == 0, flags
        assert _lib.load().lpi_jpeg_decode_workspace_x(flags, 1, a.ctypes.data, o.ctypes.data, ctypes.addressof(out)) == 0, flags


def test_workspace_of_todays_files_does_not_change():
    """Baseline and progressive files of today's envelope: the same verdict fields and the same workspace bytes with and without the flag (the
    descriptor keeps its size; the fourth component's tables are only there for a batch that has such a file)."""
    pytest.importorskip("PIL")
    files = C.random_files(11, 64, 1, 200)
    for f in files:
        assert info_x(f, LAY) == info_x(f, 0)
    host, offs = packed(files)
    out = ctypes.c_long(0)
    _lib.load().lpi_jpeg_decode_workspace(64, host.ctypes.data, offs.ctypes.data, ctypes.addressof(out))
    assert out.value == imageops.jpeg_workspace_bytes(host, offs) == imageops.jpeg_workspace_bytes(host, offs, layouts=True) \
        == imageops.jpeg_workspace_bytes(host, offs, progressive=True, layouts=True)
    # 2320 bytes a descriptor, as before the flag existed: one 8 x 8 grayscale file needs the descriptor, 8 + 16 entropy bytes and one segment,
    # one coefficient block and one sample block, each rounded up to 256
    tiny = C.encode(np.zeros((8, 8, 3), np.uint8), gray=True)
    ent = len(tiny) - L.parse(tiny)["ent"] + 16
    up = lambda v: -(-v // 256) * 256      # noqa: E731
    assert imageops.jpeg_workspace_bytes(*packed([tiny]), layouts=True) == up(2320) + up(ent) + 256 + 256 + 256
    mixed = files[:8] + P.random_files(3, 8, 1, 90)
    host, offs = packed(mixed)
    assert imageops.jpeg_workspace_bytes(host, offs, progressive=True) == imageops.jpeg_workspace_bytes(host, offs, progressive=True, layouts=True)
    # a four-component file adds its planes and one table record
    rng = np.random.default_rng(2)
    cmyk = L.colour_variant("cmyk", rng, (2, 2), 40, 24)
    assert imageops.jpeg_workspace_bytes(*packed(files[:8] + [cmyk]), layouts=True) > imageops.jpeg_workspace_bytes(*packed(files[:8]), layouts=True)
    with pytest.raises(_lib.LpiError):
        imageops.jpeg_workspace_bytes(*packed(files[:8] + [cmyk]))


# ---------------------------------------------------------------------------------------------------------------------------------- Python surface
@pytest.fixture(scope="module")
def coco(tmp_path_factory):
    pytest.importorskip("PIL")
    root = tmp_path_factory.mktemp("coco_jpeg_layouts_host")
    rng = np.random.default_rng(14)
    train = []
    for i, (w, h) in enumerate([(64, 48), (120, 90), (90, 130), (57, 61), (300, 40), (48, 64)]):
        data = [L.layout_file(rng, (1, 2), w, h), C.encode(C.pixels(rng, w, h), "4:2:0", 80), L.colour_variant("cmyk", rng, (2, 2), w, h),
                L.layout_file(rng, (4, 1), w, h), L.colour_variant("keep_rgb", rng, (1, 1), w, h), P.cmyk_progressive(rng, w, h)][i]
        (root / f"im{i}.jpg").write_bytes(data)
        train.append({"image": f"im{i}.jpg", "caption": f"a photo of thing {i}", "category": 11, "image_id": i})
    (root / "train.json").write_text(json.dumps(train))
    (root / "val.json").write_text(json.dumps([dict(t, caption=[t["caption"]]) for t in train]))
    return root


def test_coco_items_with_and_without_jpeg_layouts(coco):
    for cls, ann in ((D.Coco, "train.json"), (D.CocoEval, "val.json")):
        kw = {} if cls is D.Coco else {"eval_transform": "center"}
        make = lambda **k: cls(image_root=str(coco), ann_file=str(coco / ann), tasks=[0], **kw, **k)        # noqa: E731
        torch.manual_seed(3)
        on = [make(pixel_format="jpeg", jpeg_layouts=True)[i][0] for i in range(6)]
        torch.manual_seed(3)
        off = [make(pixel_format="jpeg")[i][0] for i in range(6)]
        torch.manual_seed(3)
        de = [make(pixel_format="decoded")[i][0] for i in range(6)]
        assert [type(x).__name__ for x in on] == ["EncodedImage"] * 5 + ["DecodedImage"]
        assert [type(x).__name__ for x in off] == ["DecodedImage", "EncodedImage"] + ["DecodedImage"] * 4
        assert [x.params for x in on] == [x.params for x in de] == [x.params for x in off]
        for x, y in zip(on, de):
            if isinstance(x, D.EncodedImage):
                assert x.layouts and not x.progressive and x.wh == (int(y.pixels.shape[1]), int(y.pixels.shape[0]))
            else:
                assert torch.equal(x.pixels, y.pixels)
        assert not any(x.layouts for x in off if isinstance(x, D.EncodedImage))
        both = make(pixel_format="jpeg", jpeg_layouts=True, jpeg_progressive=True)
        assert both.jpeg_layouts and both.jpeg_progressive and both[0][0].layouts and both[0][0].progressive
        with pytest.raises(ValueError, match="jpeg_layouts widens the envelope of pixel_format='jpeg'"):
            make(pixel_format="decoded", jpeg_layouts=True)
        with pytest.raises(ValueError, match="jpeg_layouts"):
            make(jpeg_layouts=True)


def test_encoded_batch_carries_the_flag_and_refuses_a_mix():
    pytest.importorskip("PIL")
    rng = np.random.default_rng(9)
    files = [L.layout_file(rng, (1, 2), 40, 30), L.colour_variant("ycck", rng, (2, 1), 33, 20), L.colour_variant("rgb ids", rng, (1, 4), 20, 50)] \
        + C.random_files(8, 3, 8, 60)
    torch.manual_seed(0)
    t = D.encoded_transform("train", 32, layouts=True)
    enc = D.collate_encoded([(t(f), i) for i, f in enumerate(files)])[0]
    assert enc.layouts and not enc.progressive and not enc.fallback and len(enc) == 6
    back = pickle.loads(pickle.dumps(enc))
    assert back.layouts and not back.progressive and torch.equal(back.data, enc.data) and back.filter == enc.filter
    item = pickle.loads(pickle.dumps(t(files[0])))
    assert item.layouts and not item.progressive
    both = pickle.loads(pickle.dumps(D.encoded_transform("train", 32, progressive=True, layouts=True)(files[0])))
    assert both.layouts and both.progressive
    torch.manual_seed(0)
    plain = D.collate_encoded([(D.encoded_transform("train", 32)(f), i) for i, f in enumerate(files)])[0]
    assert not plain.layouts and sorted(plain.fallback) == [0, 1, 2]
    assert not pickle.loads(pickle.dumps(plain)).layouts
    assert not D.EncodedBatch(enc.data, enc.offsets, enc.params, enc.wh, 32).layouts
    assert imageops._batch_flags(enc) == LAY and imageops._batch_flags(plain) == 0
    assert imageops._batch_flags(D.EncodedBatch(enc.data, enc.offsets, enc.params, enc.wh, 32, progressive=True, layouts=True)) == LAY | PROG
    # items admitted by different envelopes do not share a batch
    with pytest.raises(ValueError, match="layouts"):
        D.collate_encoded([(D.encoded_transform("train", 32)(files[3]),), (t(files[0]),)])
    # a host-decoded item has no setting of its own
    odd = D.collate_encoded([(D.encoded_transform("train", 32)(files[0]),), (D.encoded_transform("train", 32)(files[3]),)])[0]
    assert sorted(odd.fallback) == [0] and not odd.layouts


def test_plugin_config_key_reaches_the_datasets(coco):
    from lpi_amd.retrieval.methods import sprompt

    class Stub:
        _datasets = sprompt.SPrompts._datasets

        def __init__(self, **args):
            self.args = dict(dict(image_root=str(coco), annotation_train_root=str(coco / "train.json"), annotation_val_root=str(coco / "val.json"),
                                  dataset_impl="coco"), **args)
    tr, ev = Stub(pixel_format="jpeg", jpeg_layouts=True)._datasets(0)
    assert tr.jpeg_layouts and ev.jpeg_layouts and not tr.jpeg_progressive and isinstance(tr[0][0], D.EncodedImage) and tr[0][0].layouts
    assert isinstance(ev[2][0], D.EncodedImage) and ev[2][0].layouts
    tr, ev = Stub(pixel_format="jpeg")._datasets(0)
    assert not tr.jpeg_layouts and isinstance(tr[0][0], D.DecodedImage)
    with pytest.raises(ValueError, match="jpeg_layouts"):
        Stub(pixel_format="u8", jpeg_layouts=True)._datasets(0)
    with pytest.raises(ValueError, match="jpeg_layouts"):
        Stub(jpeg_layouts=True)._datasets(0)
    with pytest.raises(ValueError, match="synthetic"):
        Stub(pixel_format="jpeg", jpeg_layouts=True, dataset_impl="synthetic")._datasets(0)
    # the check SPrompts' constructor runs before it builds anything
    sprompt._check_jpeg_layouts({"pixel_format": "jpeg", "jpeg_layouts": True})
    sprompt._check_jpeg_layouts({"pixel_format": "u8", "jpeg_layouts": False})
    for bad in ({"pixel_format": "decoded", "jpeg_layouts": True}, {"jpeg_layouts": True}):
        with pytest.raises(ValueError, match="jpeg_layouts"):
            sprompt._check_jpeg_layouts(bad)
