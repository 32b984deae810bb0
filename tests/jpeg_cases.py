"""Seeded JPEG files for the pixel_format='jpeg' tests (Pillow writes them): smooth gradients plus noise, so that every quality level leaves real AC
data, at every chroma sampling, grayscale, with and without restart markers and optimised Huffman tables."""
import io

import numpy as np

SUBSAMPLING = {"4:4:4": 0, "4:2:2": 1, "4:2:0": 2}


def pixels(rng, w, h):
    yy, xx = np.mgrid[0:h, 0:w]
    fx, fy = rng.uniform(0.5, 9.0, 2)
    base = np.stack([(xx * fx + yy * fy) % 256, (xx * fy * 0.5 + yy * fx) % 256, (np.sin(xx / 7.0) * np.cos(yy / 5.0) * 120 + 128)], -1)
    return np.clip(base + rng.integers(-48, 48, base.shape), 0, 255).astype(np.uint8)


def encode(a, sampling="4:2:0", quality=90, gray=False, **kw):
    """JPEG bytes of HWC uint8 pixels a (Pillow's encoder)."""
    from PIL import Image
    im = Image.fromarray(a)
    buf = io.BytesIO()
    if gray:
        im.convert("L").save(buf, "JPEG", quality=quality, **kw)
    else:
        im.save(buf, "JPEG", quality=quality, subsampling=SUBSAMPLING[sampling], **kw)
    return buf.getvalue()


def random_files(seed, n, lo=1, hi=700):
    """n seeded files of random size in [lo, hi) a side: every sampling, grayscale, random quality, some with restart markers, some optimised."""
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n):
        w, h = (int(v) for v in rng.integers(lo, hi, 2))
        kw = {}
        if i % 5 == 1:
            kw["restart_marker_blocks"] = int(rng.integers(1, 40))
        elif i % 5 == 3:
            kw["restart_marker_rows"] = int(rng.integers(1, 4))
        if i % 4 == 2:
            kw["optimize"] = True
        out.append(encode(pixels(rng, w, h), ("4:4:4", "4:2:2", "4:2:0", None)[i % 4] or "4:2:0", int(rng.integers(30, 101)), gray=i % 4 == 3, **kw))
    return out


def decode_pil(data):
    from PIL import Image
    with Image.open(io.BytesIO(data)) as im:
        return np.asarray(im.convert("RGB"))


def segments_of(f):
    """The marker segments of a JPEG file before its SOS [(marker, payload)], and the rest (SOS segment + entropy-coded data + EOI)."""
    p, segs = 2, []
    while f[p + 1] != 0xDA:
        L = (f[p + 2] << 8) | f[p + 3]
        segs.append((f[p + 1], f[p + 4:p + 2 + L]))
        p += 2 + L
    return segs, f[p:]


def join(segs, rest):
    return b"\xff\xd8" + b"".join(b"\xff" + bytes([m]) + (len(pl) + 2).to_bytes(2, "big") + pl for m, pl in segs) + rest


def rewrite(f, sof1=False, dqt16=False, reorder=False, swap_scan=False):
    """The same baseline file with other headers: SOF1 instead of SOF0; 16-bit quantisation tables; one table per DQT / DHT segment, the Huffman
    tables first and in reverse order, a COM, the frame, then the quantisation tables in reverse order; or a scan that lists the two chroma
    components the other way round (the frame keeps its order: the file then means another image, decoded the same way by any decoder)."""
    segs, rest = segments_of(f)
    out = []
    for m, pl in segs:
        if m == 0xC0 and sof1:
            m = 0xC1
        if m == 0xDB and (dqt16 or reorder):
            q = 0
            while q < len(pl):
                pq, tq = pl[q] >> 4, pl[q] & 15
                vals = np.frombuffer(pl[q + 1:q + 1 + 64 * (pq + 1)], dtype=">u2" if pq else np.uint8).astype(np.int64)
                body = bytes([0x10 | tq]) + vals.astype(">u2").tobytes() if dqt16 else bytes([pl[q]]) + pl[q + 1:q + 65 + 64 * pq]
                out.append((0xDB, body))
                q += 1 + 64 * (pq + 1)
            continue
        if m == 0xC4 and reorder:
            q = 0
            while q < len(pl):
                n = 17 + sum(pl[q + 1:q + 17])
                out.append((0xC4, pl[q:q + n]))
                q += n
            continue
        out.append((m, pl))
    if reorder:
        app = [s for s in out if 0xE0 <= s[0] <= 0xEF]
        dht = [s for s in out if s[0] == 0xC4][::-1]
        sof = [s for s in out if s[0] in (0xC0, 0xC1)]
        dqt = [s for s in out if s[0] == 0xDB][::-1]
        rest_ = [s for s in out if not (0xE0 <= s[0] <= 0xEF or s[0] in (0xC4, 0xC0, 0xC1, 0xDB))]     # DRI and the like
        out = app + dht + [(0xFE, b"tables in another order")] + sof + rest_ + dqt
    if swap_scan:
        L = (rest[2] << 8) | rest[3]
        sos = bytearray(rest[4:2 + L])
        sos[3:5], sos[5:7] = sos[5:7], sos[3:5]
        rest = rest[:4] + bytes(sos) + rest[2 + L:]
    return join(out, rest)


def rst_out_of_order(f):
    """f (with restart markers) with its first RST0 turned into RST1: libjpeg resynchronises and Pillow decodes it; the GPU status is not OK."""
    i = f.index(b"\xff\xda")
    j = f.index(b"\xff\xd0", i)
    return f[:j + 1] + b"\xd1" + f[j + 2:]
