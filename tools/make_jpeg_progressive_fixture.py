"""Writes tests/golden/jpeg_progressive_pillow.npz: seeded progressive JPEG files (Pillow's encoder, progressive=True) and Pillow's decodes of them,
np.asarray(Image.open(f).convert("RGB")) — full arrays up to 128 x 128, SHA-256 digests above that — with the Pillow and libjpeg-turbo versions that
made them, in the layout of tests/golden/jpeg_pillow.npz.  Every sampling, grayscale, qualities 30-100, restart markers (blocks and rows), odd sizes.
Run: python tools/make_jpeg_progressive_fixture.py"""
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
    import jpeg_progressive as P
    rng = np.random.default_rng(2027)
    specs = []
    for i, (w, h) in enumerate([(1, 1), (3, 2), (5, 7), (8, 8), (16, 9), (17, 33), (40, 23), (64, 64), (100, 75), (128, 128), (127, 3), (2, 90)]):
        for j, sampling in enumerate(("4:4:4", "4:2:2", "4:2:0", "gray")):
            kw = {}
            if (i + j) % 3 == 1:
                kw["restart_marker_blocks"] = 1 + (i + j) % 5
            if (i + j) % 4 == 2:
                kw["restart_marker_rows"] = 1 + (i + j) % 2
            specs.append((w, h, sampling, int(rng.integers(30, 101)), kw))
    specs += [(400, 300, "4:2:0", 90, {}), (333, 217, "4:2:2", 75, {"restart_marker_rows": 2}), (201, 150, "4:4:4", 85, {}), (201, 250, "gray", 60, {})]
    files, pixels, digests = [], {}, []
    for k, (w, h, sampling, q, kw) in enumerate(specs):
        f = P.encode(C.pixels(rng, w, h), "4:2:0" if sampling == "gray" else sampling, q, gray=sampling == "gray", **kw)
        a = C.decode_pil(f)
        files.append(f)
        digests.append(hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest())
        if w <= 128 and h <= 128:
            pixels[f"pixels{k}"] = np.ascontiguousarray(a)
    offsets = np.concatenate(([0], np.cumsum([len(f) for f in files]))).astype(np.int64)
    out = os.path.join(REPO, "tests", "golden", "jpeg_progressive_pillow.npz")
    np.savez_compressed(out, data=np.frombuffer(b"".join(files), np.uint8), offsets=offsets,
                        wh=np.array([(w, h) for w, h, *_ in specs], dtype=np.int64), sha256=np.array(digests),
                        pillow=np.array(PIL.__version__), libjpeg_turbo=np.array(str(features.version("libjpeg_turbo"))), **pixels)
    print(f"{out}: {len(files)} files, {os.path.getsize(out)} bytes")


if __name__ == "__main__":
    main()
