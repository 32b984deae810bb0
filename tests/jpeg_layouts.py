"""JPEG files of the layouts LPI_JPEG_LAYOUTS adds to the envelope of lpi_jpeg_decode_u8_x, and the numpy restatement of what Pillow 12
(libjpeg-turbo) does to them, built from the pieces of tests/jpeg_restate.py:

- the first component sampled 1x2 (4:4:0), 4x1 (4:1:1) or 1x4 over the others at 1x1: jdsample.c's h1v2 fancy upsampling (the 3:1 triangle filter
  down the columns, biases 1 / 2, whatever the width) and plain replication for 4x1 and 1x4;
- three components that libjpeg reads as RGB (an Adobe APP14 with transform 0 and no JFIF APP0, or the ids 'R','G','B' with neither marker):
  the planes as they are;
- four components, CMYK (no Adobe APP14, or transform 0) or YCCK (any other transform: the first three planes through the YCbCr tables, inverted):
  Pillow inverts all four planes, and convert("RGB") is clip(nk - MULDIV255(c, nk)) with nk = 255 - k.

Pillow cannot write 4:4:0, 4:1:1 or 1x4 files.  They are made by rewriting the frame header of a file it can write: the MCU of 2x1 and of 1x2 holds
the same blocks in the same order (two of the first component, one of each other), as does that of 2x2, 4x1 and 1x4 (four), so a file whose size
gives the same number of MCUs is a valid file of the other geometry.  Its pixels are scrambled; the decoder's work on it is exact all the same.
Rewriting a LATER component's factors changes the MCU: such files are corrupt data that Pillow decodes without raising, and are no positive cases."""
import io

import numpy as np

import jpeg_cases as C
import jpeg_restate as R
from jpeg_progressive import walk
from jpeg_restate import NotInEnvelope

LAYOUTS = 4                                                     # include/lpi_hip.h LPI_JPEG_LAYOUTS
GEOMETRIES = ((1, 1), (2, 1), (2, 2), (1, 2), (4, 1), (1, 4))   # the first component's (H, V) inside the envelope
SOURCE = {(1, 1): (1, 1), (2, 1): (2, 1), (1, 2): (2, 1), (2, 2): (2, 2), (4, 1): (2, 2), (1, 4): (2, 2)}       # what Pillow writes with the same MCU
SUBSAMPLING = {(1, 1): 0, (2, 1): 1, (2, 2): 2}


# ---------------------------------------------------------------------------------------------------------------------------------- files
def save(a, mode, hv, quality, **kw):
    """Pillow's JPEG of pixels a ([h, w, 3] for 'RGB', [h, w, 4] for 'CMYK') with the first component sampled hv in (1,1), (2,1), (2,2)."""
    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray(a, mode).save(buf, "JPEG", quality=quality, subsampling=SUBSAMPLING[hv], **kw)
    return buf.getvalue()


def frame(f):
    """(position of the SOF0 / SOF1 payload, the payload) of a file."""
    p, _, seg, _ = next(s for s in walk(f) if s[1] in (0xC0, 0xC1))
    return p + 4, seg


def reframe(f, hv, w, h):
    """f with the first component's sampling byte and the frame's size rewritten (see the module's text for when that is a valid file)."""
    at, _ = frame(f)
    f = bytearray(f)
    f[at + 1:at + 5] = h.to_bytes(2, "big") + w.to_bytes(2, "big")
    f[at + 7] = (hv[0] << 4) | hv[1]
    return bytes(f)


def layout_file(rng, hv, w, h, quality=85, mode="RGB", **kw):
    """A w x h file whose first component is sampled hv over 1x1 others: Pillow's file of the source geometry with the same MCU, at the size that
    has the MCU grid of w x h under hv, with its frame header rewritten."""
    sh, sv = SOURCE[hv]
    mx, my = -(-w // (8 * hv[0])), -(-h // (8 * hv[1]))
    sw, sh_ = 8 * sh * mx, 8 * sv * my
    a = C.pixels(rng, sw, sh_)
    if mode == "CMYK":
        a = np.concatenate([a, rng.integers(0, 256, (sh_, sw, 1), dtype=np.uint8)], axis=2)
    return reframe(save(a, mode, (sh, sv), quality, **kw), hv, w, h)


def without(f, marker, magic=b""):
    """f without its segments of that marker whose payload starts with magic."""
    segs, rest = C.segments_of(f)
    return C.join([(m, pl) for m, pl in segs if not (m == marker and pl.startswith(magic))], rest)


def with_adobe(f, transform):
    """f with its Adobe APP14's transform byte set, or with such a segment added behind SOI."""
    segs, rest = C.segments_of(f)
    if any(m == 0xEE and pl.startswith(b"Adobe") for m, pl in segs):
        return C.join([(m, pl[:11] + bytes([transform]) + pl[12:]) if m == 0xEE and pl.startswith(b"Adobe") else (m, pl) for m, pl in segs], rest)
    return C.join([(0xEE, b"Adobe" + bytes([0, 100, 0, 0, 0, 0, transform]))] + segs, rest)


def with_ids(f, ids):
    """f with its components' ids replaced, in the frame and in the scan."""
    at, seg = frame(f)
    f = bytearray(f)
    old = [seg[6 + 3 * i] for i in range(seg[5])]
    for i, c in enumerate(ids):
        f[at + 6 + 3 * i] = c
    p, _, sos, _ = next(s for s in walk(bytes(f)) if s[1] == 0xDA)
    for i in range(sos[0]):
        f[p + 5 + 2 * i] = ids[old.index(sos[1 + 2 * i])]
    return bytes(f)


COLOUR_VARIANTS = ("cmyk", "ycck", "cmyk no adobe", "keep_rgb", "rgb ids", "adobe 0", "adobe 1")


def colour_variant(kind, rng, hv, w, h, quality=85, **kw):
    """A file of one of COLOUR_VARIANTS with the first component sampled hv (the RGB planes of 'rgb ids' and 'adobe 0' are then subsampled)."""
    if kind in ("cmyk", "ycck", "cmyk no adobe"):
        f = layout_file(rng, hv, w, h, quality, "CMYK", **kw)
        return with_adobe(f, 2) if kind == "ycck" else (without(f, 0xEE, b"Adobe") if kind == "cmyk no adobe" else f)
    if kind == "keep_rgb":                      # Pillow refuses keep_rgb with subsampling: always 1x1
        return layout_file(rng, (1, 1), w, h, quality, keep_rgb=True, **kw)
    f = without(layout_file(rng, hv, w, h, quality, **kw), 0xE0, b"JFIF")
    return with_ids(f, b"RGB") if kind == "rgb ids" else with_adobe(f, int(kind[-1]))


def case(i, rng):
    """Seeded case i: the six geometries in turn, with three components (YCbCr, or one of the three-component colour variants) or four (the
    CMYK / YCCK variants); sizes down to 1 a side, every residue inside the last MCU among them; qualities 30..95; every fifth with
    restart_marker_blocks, every fifth with restart_marker_rows, every seventh with optimised tables."""
    hv = GEOMETRIES[i % 6]
    small = ((1, 1), (2, 1), (1, 2), (2, 2), (1, 40), (40, 1), (3, 5), (5, 3), (8, 8), (9, 17), (17, 9), (16, 32), (33, 31), (31, 33))
    w, h = small[(i // 6) % len(small)] if (i // 84) % 2 == 0 else (int(v) for v in rng.integers(1, 70, 2))      # 84 listed sizes, 84 drawn ones, ...
    kw = {}
    if i % 5 == 1:
        kw["restart_marker_blocks"] = int(rng.integers(1, 9))
    elif i % 5 == 3:
        kw["restart_marker_rows"] = int(rng.integers(1, 3))
    if i % 7 == 2:
        kw["optimize"] = True
    kinds = ("ycc",) + COLOUR_VARIANTS
    kind = kinds[(i // 6 + i // 84) % len(kinds)]
    q = int(rng.integers(30, 96))
    return layout_file(rng, hv, w, h, q, **kw) if kind == "ycc" else colour_variant(kind, rng, hv, w, h, q, **kw)


def cases(seed, n):
    rng = np.random.default_rng(seed)
    return [case(i, rng) for i in range(n)]


def photo_like(rng, kind, w=640, h=480, quality=90):
    """A larger file of one of the new kinds ('4:4:0', '4:1:1', 'cmyk'), for the tools' batches."""
    if kind == "cmyk":
        return layout_file(rng, (2, 2), w, h, quality, "CMYK")
    return layout_file(rng, {"4:4:0": (1, 2), "4:1:1": (4, 1), "1x4": (1, 4)}[kind], w, h, quality)


# ---------------------------------------------------------------------------------------------------------------------------------- restatement
def parse(data):
    """jpeg_restate.parse's dict for a baseline file inside the envelope of LPI_JPEG_LAYOUTS, and 'ct' in ('gray', 'ycc', 'rgb', 'cmyk', 'ycck');
    NotInEnvelope for anything else.  No check of the tables: the files are Pillow's."""
    data = bytes(data)
    if data[:2] != b"\xff\xd8":
        raise NotInEnvelope("not a JPEG file")
    hdr = dict(qt={}, dc={}, ac={}, ri=0, jfif=False, adobe=None, comps=None)
    for p, m, seg, end in walk(data):
        if m in (0xC0, 0xC1):
            hdr.update(prec=seg[0], h=(seg[1] << 8) | seg[2], w=(seg[3] << 8) | seg[4],
                       comps=[(seg[6 + 3 * i], seg[7 + 3 * i] >> 4, seg[7 + 3 * i] & 15, seg[8 + 3 * i]) for i in range(seg[5])])
        elif 0xC0 <= m <= 0xCF and m not in (0xC4, 0xC8):
            raise NotInEnvelope(f"marker {m:#x}")
        elif m == 0xC4:
            q = 0
            while q < len(seg):
                bits = list(seg[q + 1:q + 17])
                (hdr["dc"] if seg[q] >> 4 == 0 else hdr["ac"])[seg[q] & 15] = (bits, list(seg[q + 17:q + 17 + sum(bits)]))
                q += 17 + sum(bits)
        elif m == 0xDB:
            q = 0
            while q < len(seg):
                pq, tq = seg[q] >> 4, seg[q] & 15
                nat = np.zeros(64, np.int64)
                nat[R.ZIGZAG] = np.frombuffer(seg[q + 1:q + 1 + 64 * (pq + 1)], dtype=">u2" if pq else np.uint8).astype(np.int64)
                hdr["qt"][tq] = nat
                q += 1 + 64 * (pq + 1)
        elif m == 0xDD:
            hdr["ri"] = (seg[0] << 8) | seg[1]
        elif m == 0xE0:
            hdr["jfif"] = hdr["jfif"] or seg[:5] == b"JFIF\0"
        elif m == 0xEE and len(seg) >= 12 and seg[:5] == b"Adobe":
            hdr["adobe"] = seg[11]
        elif m == 0xDA:
            comps = hdr["comps"]
            if comps is None:
                raise ValueError("SOS before SOF")
            ns, nc = seg[0], len(comps)
            ids = [c[0] for c in comps]
            scan = [(ids.index(seg[1 + 2 * i]), seg[2 + 2 * i] >> 4, seg[2 + 2 * i] & 15) for i in range(ns)]
            if (seg[1 + 2 * ns], seg[2 + 2 * ns], seg[3 + 2 * ns]) != (0, 63, 0) or [s[0] for s in scan] != list(range(nc)):
                raise NotInEnvelope("scan")
            if hdr["prec"] != 8 or hdr["h"] == 0 or nc not in (1, 3, 4):
                raise NotInEnvelope("frame")
            if nc > 1 and ((comps[0][1], comps[0][2]) not in GEOMETRIES or any(c[1:3] != (1, 1) for c in comps[1:])):
                raise NotInEnvelope("sampling")
            if nc == 1:
                ct = "gray"
            elif nc == 4:
                ct = "ycck" if hdr["adobe"] not in (None, 0) else "cmyk"
            elif hdr["jfif"]:
                ct = "ycc"
            elif hdr["adobe"] is not None:
                ct = "rgb" if hdr["adobe"] == 0 else "ycc"
            else:
                ct = "rgb" if ids == [82, 71, 66] else "ycc"
            hdr.update(scan=scan, ent=p + 4 + len(seg), ct=ct)
            return hdr
    raise ValueError("no scan")


def upsample(p, H, V, dw, dh):
    """jdsample.c for a component behind the first, expansion (H, V): jpeg_restate's rules, h1v2's triangle filter, replication for 4x1 / 1x4."""
    if (H, V) in ((1, 1), (2, 1), (2, 2)):
        return R.upsample(p, H, V, dw, dh)
    p = p[:dh, :dw].astype(np.int64)
    if (H, V) == (1, 2):
        up = np.concatenate([p[:1], p[:-1]], axis=0)
        down = np.concatenate([p[1:], p[-1:]], axis=0)
        out = np.empty((2 * dh, dw), np.int64)
        out[0::2] = (3 * p + up + 1) >> 2
        out[1::2] = (3 * p + down + 2) >> 2
        return out
    return np.repeat(np.repeat(p, H, axis=1), V, axis=0)


def muldiv255(a, b):
    t = a * b + 128
    return ((t >> 8) + t) >> 8


def cmyk_to_rgb(c, m, y, k):
    """Pillow's convert("RGB") of a CMYK image with the planes c, m, y, k (its own, that is inverted, values)."""
    nk = 255 - k
    return np.clip(np.stack([nk - muldiv255(v, nk) for v in (c, m, y)], axis=-1), 0, 255).astype(np.uint8)


def decode(data):
    """np.asarray(Image.open(f).convert("RGB")) for a baseline file inside the envelope of LPI_JPEG_LAYOUTS."""
    hdr = parse(data)
    coef = R.decode_coefficients(hdr, bytes(data))
    comps, w, h, ct = hdr["comps"], hdr["w"], hdr["h"], hdr["ct"]
    planes = [R._plane(R.idct_islow(c, hdr["qt"][comps[i][3]])) for i, c in enumerate(coef)]
    first = planes[0][:h, :w].astype(np.int64)
    if ct == "gray":
        return np.repeat(first[:, :, None], 3, axis=2).astype(np.uint8)
    H, V = comps[0][1], comps[0][2]
    dw, dh = -(-w // H), -(-h // V)
    rest = [upsample(p, H, V, dw, dh)[:h, :w] for p in planes[1:]]
    if ct == "ycc":
        return R.ycc_to_rgb(first, rest[0], rest[1])
    if ct == "rgb":
        return np.stack([first, rest[0], rest[1]], axis=-1).astype(np.uint8)
    if ct == "ycck":                            # libjpeg: C, M, Y = 255 - R, G, B; Pillow inverts them back
        c, m, y = (R.ycc_to_rgb(first, rest[0], rest[1]).astype(np.int64)[..., i] for i in range(3))
    else:
        c, m, y = 255 - first, 255 - rest[0], 255 - rest[1]
    return cmyk_to_rgb(c, m, y, 255 - rest[2])


# ---------------------------------------------------------------------------------------------------------------------------------- outside
def outside(rng):
    """{name: file} of baseline files the envelope of LPI_JPEG_LAYOUTS names as the host's; Pillow raises on the fractional ones."""
    a = C.pixels(rng, 48, 32)
    out = {}
    for name, byte in (("3x1", 0x31), ("4x2", 0x42), ("2x4", 0x24), ("3x3", 0x33)):
        at, _ = frame(f := C.encode(a, "4:4:4", 80))
        out["first component " + name] = f[:at + 7] + bytes([byte]) + f[at + 8:]
    at, _ = frame(f := C.encode(a, "4:2:0", 80))
    out["second component 2x1"] = f[:at + 10] + b"\x21" + f[at + 11:]
    out["fractional 2x2 over 1x3"] = f[:at + 10] + b"\x13" + f[at + 11:]
    at, _ = frame(f := C.encode(a, "4:2:2", 80))
    out["fractional 3x1 over 2x1"] = f[:at + 7] + b"\x31" + f[at + 8:at + 10] + b"\x21" + f[at + 11:]
    out["12-bit"] = f[:at] + b"\x0c" + f[at + 1:]
    p = next(s[0] for s in walk(f) if s[1] == 0xC0)
    out["arithmetic"] = f[:p + 1] + b"\xc9" + f[p + 2:]
    out["two components"] = two_components(f)
    out["a scan of one component"] = first_scan_of_one(f)
    return out


def two_components(f):
    """f's frame and scan cut to their first two components."""
    segs, rest = C.segments_of(f)
    L = (rest[2] << 8) | rest[3]
    sos = b"\x02" + rest[5:9] + rest[2 + L - 3:2 + L]
    return C.join([(m, pl[:5] + b"\x02" + pl[6:12]) if m == 0xC0 else (m, pl) for m, pl in segs],
                  b"\xff\xda" + (len(sos) + 2).to_bytes(2, "big") + sos + rest[2 + L:])


def first_scan_of_one(f):
    """f's SOS cut to its first component, as the first scan of a sequential file with a scan per component begins."""
    segs, rest = C.segments_of(f)
    L = (rest[2] << 8) | rest[3]
    sos = rest[4:2 + L]
    sos = b"\x01" + sos[1:3] + sos[-3:]
    return C.join(segs, b"\xff\xda" + (len(sos) + 2).to_bytes(2, "big") + sos + rest[2 + L:])
