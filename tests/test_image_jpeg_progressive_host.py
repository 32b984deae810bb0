"""Progressive files in pixel_format='jpeg' without a GPU: the plain-Python restatement of jdphuff.c (tests/jpeg_progressive.py) against Pillow, on
Pillow's own files and on re-encoded scan scripts; the host parser's verdicts through lpi_jpeg_info_x with and without LPI_JPEG_PROGRESSIVE; the
data layer's jpeg_progressive keyword; the committed fixture."""
import ctypes
import hashlib
import json
import os
import pickle

import numpy as np
import pytest
import torch

import jpeg_cases as C
import jpeg_progressive as P
from lpi_amd import _lib, imageops
from lpi_amd.retrieval.utils import data as D

PROG = imageops.JPEG_PROGRESSIVE


def info_x(f, flags):
    """(return code, the LPI_JPEG_INFO_X fields) of lpi_jpeg_info_x."""
    a = np.frombuffer(bytes(f), np.uint8)
    x = (ctypes.c_long * imageops.JPEG_INFO_X)()
    rc = _lib.load().lpi_jpeg_info_x(flags, a.ctypes.data, int(a.size), ctypes.addressof(x))
    return rc, list(x)


def info_old(f):
    a = np.frombuffer(bytes(f), np.uint8)
    x = (ctypes.c_long * imageops.JPEG_INFO)()
    rc = _lib.load().lpi_jpeg_info(a.ctypes.data, int(a.size), ctypes.addressof(x))
    return rc, list(x)


def test_restatement_equals_pillow_on_seeded_progressive_files():
    """240 seeded files: every sampling and grayscale, qualities 30-100, sizes from 1 x 1, restart_marker_blocks and restart_marker_rows."""
    pytest.importorskip("PIL")
    rng = np.random.default_rng(77)
    kinds = set()
    for i in range(240):
        f = P.case(i, rng)
        hdr = P.parse(f)
        kinds.add((len(hdr["comps"]), hdr["comps"][0][1:3], any(s["ri"] for s in hdr["scans"])))
        assert P.script_ok(hdr) and len(hdr["scans"]) == (10 if len(hdr["comps"]) == 3 else 6)
        assert imageops.jpeg_info(f, progressive=True) == (True, hdr["w"], hdr["h"]), i
        assert imageops.jpeg_info(f) == (False, hdr["w"], hdr["h"]), i
        assert np.array_equal(P.decode(f), C.decode_pil(f)), i
    assert len(kinds) == 8           # 4:4:4, 4:2:2, 4:2:0 and grayscale, each with and without restart markers


def test_restatement_equals_fixture(golden):
    g = golden("jpeg_progressive_pillow")
    assert str(g["pillow"]).startswith("12.") and str(g["libjpeg_turbo"]).startswith("3.")
    n = len(g["offsets"]) - 1
    assert n == 52
    here = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
    assert os.path.getsize(os.path.join(here, "jpeg_progressive_pillow.npz")) <= os.path.getsize(os.path.join(here, "jpeg_pillow.npz"))
    full = 0
    for i in range(n):
        f = bytes(g["data"][g["offsets"][i]:g["offsets"][i + 1]])
        w, h = (int(v) for v in g["wh"][i])
        assert info_x(f, PROG)[1][:3] == [1, w, h] and info_x(f, PROG)[1][8] == 1
        if f"pixels{i}" not in g:
            continue                # the four large files are the GPU suite's
        a = P.decode(f)
        assert np.array_equal(a, g[f"pixels{i}"]) and hashlib.sha256(a.tobytes()).hexdigest() == str(g["sha256"][i]), i
        full += 1
    assert full == 48


def reencoded_cases():
    """(name, baseline original, progressive re-encoding) for every sampling and grayscale: spectral selection only, a DC scan per component, and the
    same with restart intervals that change and disappear between the scans."""
    rng = np.random.default_rng(31)
    out = []
    for sampling, gray in (("4:4:4", False), ("4:2:2", False), ("4:2:0", False), ("4:2:0", True)):
        for w, h in ((75, 50), (17, 33), (1, 1)):
            base = C.encode(C.pixels(rng, w, h), sampling, int(rng.integers(40, 96)), gray=gray)
            hdr, coef = P.baseline_coefficients(base)
            nc = len(hdr["comps"])
            for name, script in (("spectral", P.spectral_script(nc)), ("split_dc", P.split_dc_script(nc)),
                                 ("spectral_dri", P.spectral_script(nc, (0, 5, 3, 0, 7))), ("split_dc_dri", P.split_dc_script(nc, (4, 0, 2)))):
                out.append((f"{sampling}{'g' if gray else ''}-{w}x{h}-{name}", base, P.reencode(hdr, coef, script)))
    return out


def test_reencoded_scripts_pillow_first_then_the_restatement():
    pytest.importorskip("PIL")
    cases = reencoded_cases()
    assert len(cases) == 48
    for name, base, f in cases:
        want = C.decode_pil(base)
        assert np.array_equal(C.decode_pil(f), want), name           # Pillow reads the re-encoded file as its baseline original
        hdr = P.parse(f)
        assert all(s["ah"] == 0 and s["al"] == 0 for s in hdr["scans"]) and P.script_ok(hdr)
        if "dri" in name:
            assert len({s["ri"] for s in hdr["scans"]}) > 1
        assert np.array_equal(P.decode(f), want), name
        assert info_x(f, PROG)[1][0] == 1 and info_x(f, PROG)[1][9] == len(hdr["scans"]), name


def outside_files():
    """Progressive files outside the envelope with the flag, by name."""
    rng = np.random.default_rng(8)
    f = P.encode(C.pixels(rng, 96, 64), "4:2:0", 85)
    head, sc, _ = P.chunks(f)
    assert len(sc) == 10
    out = {"last scan removed": P.join(head, sc[:-1]),
           "refinement dropped from the middle": P.join(head, sc[:5] + sc[6:]),
           "Ah != previous Al": P.join(head, sc[:5] + [P.patch_sos(sc[5], ahal=0x32)] + sc[6:]),
           "AC scan with two components": P.join(head, sc[:1] + [P.patch_sos(sc[1], extra_component=2)] + sc[2:]),
           "AC scan before the DC scan": P.join(head, [sc[1], sc[0]] + sc[2:]),
           "CMYK": P.cmyk_progressive(rng)}
    for m in (0xC9, 0xCA, 0xCB, 0xCD, 0xCE, 0xCF):
        out[f"SOF{m - 0xC0}"] = P.with_sof(f, m)
    base = C.encode(C.pixels(rng, 40, 24), "4:4:4", 80)
    hdr, coef = P.baseline_coefficients(base)
    out["more scans than LPI_JPEG_MAX_SCANS"] = P.reencode(hdr, coef, [([0, 1, 2], 0, 0, 0)] + [([c], k, k, 0) for c in range(3) for k in range(1, 64)])
    return f, out


def test_parser_verdicts_with_and_without_the_flag():
    pytest.importorskip("PIL")
    good, outside = outside_files()
    assert info_x(good, PROG)[1] == [1, 96, 64, 3, 2, 2, 0, P.parse(good)["scans"][0]["ent"], 1, 10]
    assert C.decode_pil(outside["more scans than LPI_JPEG_MAX_SCANS"]).shape == (24, 40, 3)
    for name, f in outside.items():
        rc, x = info_x(f, PROG)
        assert rc == 0 and x[0] == 0, name
        assert imageops.jpeg_info(f, progressive=True)[0] is False, name
        # what the 'jpeg' path returns for it is Pillow's result: its pixels, or its exception
        t = D.encoded_transform("center", 32, 36, progressive=True)
        try:
            want = C.decode_pil(f)
        except Exception as e:      # noqa: BLE001
            with pytest.raises(type(e)):
                t(f)
            continue
        item = t(f)
        assert isinstance(item, D.DecodedImage) and np.array_equal(item.pixels.numpy(), want), name
    # a file that ends inside its last scan has a complete script: inside (the decoder then reports the end of data)
    assert info_x(good[:len(good) - 40], PROG)[1][0] == 1
    # truncated headers: LPI_EINVAL
    sof = good.index(b"\xff\xc2")
    for cut in (sof + 6, good.index(b"\xff\xda") + 5, good.index(b"\xff\xc4") + 9):
        assert info_x(good[:cut], PROG)[0] == -22 and imageops.jpeg_info(good[:cut], progressive=True) is None
    assert info_x(good, 2)[0] == -22 and info_x(good, 3)[0] == -22          # unknown flag bits
    # without the flag every verdict is lpi_jpeg_info's
    files = [good, good[:len(good) - 40], good[:sof + 6]] + list(outside.values()) + [f for _, _, f in reencoded_cases()[:8]] + C.random_files(11, 64, 1, 200)
    files += [b"", b"\x89PNG\r\n\x1a\n" + bytes(40), C.rewrite(C.random_files(2, 1, 8, 40)[0], swap_scan=True)]
    for k, f in enumerate(files):
        if not f:
            continue
        rc0, x0 = info_old(f)
        rc1, x1 = info_x(f, 0)
        assert rc0 == rc1 and (rc0 != 0 or x1[:imageops.JPEG_INFO] == x0), k
        assert x1[8] == 0
    # and the flag changes nothing for baseline files
    for f in C.random_files(11, 64, 1, 200):
        assert info_x(f, PROG)[1][:8] == info_old(f)[1] and info_x(f, PROG)[1][8:] == [0, 1]


def test_workspace_refuses_what_the_parser_refuses():
    pytest.importorskip("PIL")
    good, outside = outside_files()
    one = lambda f: (np.frombuffer(f, np.uint8), np.array([0, len(f)], dtype=np.int64))     # noqa: E731
    assert imageops.jpeg_workspace_bytes(*one(good), progressive=True) > 0
    with pytest.raises(_lib.LpiError):
        imageops.jpeg_workspace_bytes(*one(good))
    with pytest.raises(_lib.LpiError):
        imageops.jpeg_workspace_bytes(*one(outside["last scan removed"]), progressive=True)
    out = ctypes.c_long(0)
    a, o = one(good)
    assert _lib.load().lpi_jpeg_decode_workspace_x(2, 1, a.ctypes.data, o.ctypes.data, ctypes.addressof(out)) == -22
    # baseline files: the same bytes through the old entry point, flags = 0 and the flag
    files = C.random_files(11, 64, 1, 200)
    host = np.frombuffer(b"".join(files), np.uint8)
    offs = np.concatenate(([0], np.cumsum([len(f) for f in files]))).astype(np.int64)
    _lib.load().lpi_jpeg_decode_workspace(64, host.ctypes.data, offs.ctypes.data, ctypes.addressof(out))
    assert out.value == imageops.jpeg_workspace_bytes(host, offs) == imageops.jpeg_workspace_bytes(host, offs, progressive=True)


@pytest.fixture(scope="module")
def coco(tmp_path_factory):
    pytest.importorskip("PIL")
    root = tmp_path_factory.mktemp("coco_jpeg_progressive_host")
    rng = np.random.default_rng(13)
    train = []
    for i, (w, h) in enumerate([(64, 48), (120, 90), (90, 130), (57, 61), (300, 40), (48, 64)]):
        a = C.pixels(rng, w, h)
        if i % 2 == 0:
            data = P.encode(a, ("4:4:4", "4:2:2", "4:2:0")[i % 3], 80, gray=i == 4)
        else:
            data = C.encode(a, ("4:4:4", "4:2:2", "4:2:0")[i % 3], 80)
        if i == 5:
            data = P.cmyk_progressive(rng, w, h)
        (root / f"im{i}.jpg").write_bytes(data)
        train.append({"image": f"im{i}.jpg", "caption": f"a photo of thing {i}", "category": 11, "image_id": i})
    (root / "train.json").write_text(json.dumps(train))
    (root / "val.json").write_text(json.dumps([dict(t, caption=[t["caption"]]) for t in train]))
    return root


def test_coco_items_with_and_without_jpeg_progressive(coco):
    for cls, ann in ((D.Coco, "train.json"), (D.CocoEval, "val.json")):
        kw = {} if cls is D.Coco else {"eval_transform": "center"}
        make = lambda **k: cls(image_root=str(coco), ann_file=str(coco / ann), tasks=[0], **kw, **k)        # noqa: E731
        torch.manual_seed(3)
        on = [make(pixel_format="jpeg", jpeg_progressive=True)[i][0] for i in range(6)]
        torch.manual_seed(3)
        off = [make(pixel_format="jpeg")[i][0] for i in range(6)]
        torch.manual_seed(3)
        de = [make(pixel_format="decoded")[i][0] for i in range(6)]
        assert [type(x).__name__ for x in on] == ["EncodedImage"] * 5 + ["DecodedImage"]
        assert [type(x).__name__ for x in off] == ["DecodedImage", "EncodedImage", "DecodedImage", "EncodedImage", "DecodedImage", "DecodedImage"]
        assert [x.params for x in on] == [x.params for x in de] == [x.params for x in off]
        for x, y in zip(on, de):
            if isinstance(x, D.EncodedImage):
                assert x.progressive and x.wh == (int(y.pixels.shape[1]), int(y.pixels.shape[0]))
            else:
                assert torch.equal(x.pixels, y.pixels)
        assert not any(x.progressive for x in off if isinstance(x, D.EncodedImage))
        with pytest.raises(ValueError):
            make(pixel_format="decoded", jpeg_progressive=True)
        with pytest.raises(ValueError):
            make(jpeg_progressive=True)


def test_encoded_batch_carries_the_flag():
    pytest.importorskip("PIL")
    files = P.random_files(9, 3, 8, 60) + C.random_files(8, 3, 8, 60)
    torch.manual_seed(0)
    t = D.encoded_transform("train", 32, progressive=True)
    enc = D.collate_encoded([(t(f), i) for i, f in enumerate(files)])[0]
    assert enc.progressive and not enc.fallback and len(enc) == 6
    back = pickle.loads(pickle.dumps(enc))
    assert back.progressive and torch.equal(back.data, enc.data) and back.filter == enc.filter
    assert pickle.loads(pickle.dumps(t(files[0]))).progressive
    assert enc.pin_memory.__func__ is D.EncodedBatch.pin_memory
    torch.manual_seed(0)
    plain = D.collate_encoded([(D.encoded_transform("train", 32)(f), i) for i, f in enumerate(files)])[0]
    assert not plain.progressive and sorted(plain.fallback) == [0, 1, 2]
    assert not pickle.loads(pickle.dumps(plain)).progressive
    assert not D.EncodedBatch(enc.data, enc.offsets, enc.params, enc.wh, 32).progressive
    # one progressive item makes the batch's flag
    mixed = D.collate_encoded([(D.encoded_transform("train", 32)(files[3]),), (t(files[0]),)])[0]
    assert mixed.progressive


def test_plugin_config_key_reaches_the_datasets(coco):
    from lpi_amd.retrieval.methods import sprompt

    class Stub:
        _datasets = sprompt.SPrompts._datasets

        def __init__(self, **args):
            self.args = dict(image_root=str(coco), annotation_train_root=str(coco / "train.json"), annotation_val_root=str(coco / "val.json"),
                             dataset_impl="coco", **args)
    tr, ev = Stub(pixel_format="jpeg", jpeg_progressive=True)._datasets(0)
    assert tr.jpeg_progressive and ev.jpeg_progressive and isinstance(tr[0][0], D.EncodedImage) and tr[0][0].progressive
    assert isinstance(ev[0][0], D.EncodedImage) and ev[0][0].progressive
    tr, ev = Stub(pixel_format="jpeg")._datasets(0)
    assert not tr.jpeg_progressive and isinstance(tr[0][0], D.DecodedImage)
    with pytest.raises(ValueError):
        Stub(pixel_format="u8", jpeg_progressive=True)._datasets(0)
    with pytest.raises(ValueError):
        Stub(jpeg_progressive=True)._datasets(0)
    # the check SPrompts' constructor runs before it builds anything
    sprompt._check_jpeg_progressive({"pixel_format": "jpeg", "jpeg_progressive": True})
    sprompt._check_jpeg_progressive({"pixel_format": "u8", "jpeg_progressive": False})
    for bad in ({"pixel_format": "decoded", "jpeg_progressive": True}, {"jpeg_progressive": True}):
        with pytest.raises(ValueError):
            sprompt._check_jpeg_progressive(bad)
