"""Writes tests/golden/jpeg_layouts_pillow.npz: seeded baseline JPEG files of the layouts LPI_JPEG_LAYOUTS admits (tests/jpeg_layouts.py: 4:4:0, 4:1:1
and 1x4 by header rewriting; RGB by marking; CMYK and YCCK, each at all six geometries) and Pillow's decodes of them,
np.asarray(Image.open(f).convert("RGB")) — full arrays up to 80 x 80, SHA-256 digests above that — with the Pillow and libjpeg-turbo versions that
made them, in the layout of tests/golden/jpeg_pillow.npz plus `kind`, the colour variant of each file.
Run: python tools/make_jpeg_layouts_fixture.py"""
import hashlib
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tests"))


def main():
    import PIL
    from PIL import features
    import jpeg_cases as C
    import jpeg_layouts as L
    rng = np.random.default_rng(2028)
    kinds = ("ycc",) + L.COLOUR_VARIANTS
    sizes = [(1, 1), (2, 3), (7, 5), (8, 8), (16, 9), (17, 33), (40, 23), (64, 64), (80, 60), (33, 80), (79, 3), (2, 75)]
    specs = []
    for i, (w, h) in enumerate(sizes):
        for j, hv in enumerate(L.GEOMETRIES):
            kw = {}
            if (i + j) % 3 == 1:
                kw["restart_marker_blocks"] = 1 + (i + j) % 5
            if (i + j) % 4 == 2:
                kw["restart_marker_rows"] = 1 + (i + j) % 2
            specs.append((w, h, hv, kinds[(i + 3 * j) % len(kinds)], int(rng.integers(30, 96)), kw))
    specs += [(400, 300, (1, 2), "ycc", 90, {}), (333, 217, (4, 1), "ycck", 75, {"restart_marker_rows": 2}), (201, 150, (2, 2), "cmyk", 85, {}),
              (201, 250, (1, 4), "rgb ids", 60, {})]
    files, pixels, digests = [], {}, []
    for k, (w, h, hv, kind, q, kw) in enumerate(specs):
        f = L.layout_file(rng, hv, w, h, q, **kw) if kind == "ycc" else L.colour_variant(kind, rng, hv, w, h, q, **kw)
        a = C.decode_pil(f)
        assert a.shape == (h, w, 3)
        files.append(f)
        digests.append(hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest())
        if w <= 80 and h <= 80:
            pixels[f"pixels{k}"] = np.ascontiguousarray(a)
    offsets = np.concatenate(([0], np.cumsum([len(f) for f in files]))).astype(np.int64)
    out = os.path.join(REPO, "tests", "golden", "jpeg_layouts_pillow.npz")
    np.savez_compressed(out, data=np.frombuffer(b"".join(files), np.uint8), offsets=offsets,
                        wh=np.array([(w, h) for w, h, *_ in specs], dtype=np.int64), sha256=np.array(digests),
                        kind=np.array([s[3] for s in specs]), pillow=np.array(PIL.__version__),
                        libjpeg_turbo=np.array(str(features.version("libjpeg_turbo"))), **pixels)
    print(f"{out}: {len(files)} files, {os.path.getsize(out)} bytes")


if __name__ == "__main__":
    main()
