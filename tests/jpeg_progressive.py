"""Progressive JPEG files (SOF2) for the pixel_format='jpeg' tests, and a plain-Python restatement of libjpeg-turbo's progressive entropy decoder
(jdphuff.c) that yields the quantised coefficient arrays tests/jpeg_restate.py turns into pixels:

- the scan walk: every SOS with the Huffman tables and the restart interval in force at it, its entropy-coded bytes up to the next marker that is
  neither a stuffed 0xFF00 nor RSTn;
- the four scan kinds: DC first (Huffman-coded difference, predictor per component, stored << Al), DC refinement (one raw bit per block), AC first
  (run / size symbols, EOB runs that carry across blocks, ZRL, stored << Al), AC refinement (decode_mcu_AC_refine: correction bits for the nonzero
  coefficients a run passes over, new coefficients +-(1 << Al), EOB runs that still refine);
- a one-component scan walks the component's own block grid, ceil(cw / 8) x ceil(ch / 8) with cw = ceil(w * Hc / Hmax); an interleaved scan the
  frame's MCUs; restart intervals count those units and reset the predictors and the EOB run.

Also: a small re-encoder (coefficients + scan script -> progressive file, first-pass scans only, fixed Huffman tables, EOB runs, restart intervals
that may change between scans) and the file surgery the parser tests need.  Small images only: everything is plain Python."""
import io

import numpy as np

import jpeg_cases
import jpeg_restate as R
from jpeg_restate import ZIGZAG, BadData, NotInEnvelope

MAX_SCANS = 32          # include/lpi_hip.h LPI_JPEG_MAX_SCANS


def encode(a, sampling="4:2:0", quality=90, gray=False, **kw):
    """Progressive JPEG bytes of HWC uint8 pixels (Pillow's encoder).  Pillow sizes its output buffer as width x height bytes for progressive files
    and fails on small noisy images of high quality: ImageFile.MAXBLOCK is raised for the call and restored after."""
    from PIL import ImageFile
    old = ImageFile.MAXBLOCK
    ImageFile.MAXBLOCK = max(old, 1 << 24)
    try:
        return jpeg_cases.encode(a, sampling, quality, gray=gray, progressive=True, **kw)
    finally:
        ImageFile.MAXBLOCK = old


def case(i, rng, lo=1, hi=97):
    """Seeded case i: every sampling and grayscale, qualities 30..100, sizes from lo up, every fifth with restart_marker_blocks, every fifth with
    restart_marker_rows."""
    w, h = (int(v) for v in rng.integers(lo, hi, 2))
    if i < 8:
        w, h = ((1, 1), (1, 9), (9, 1), (8, 8), (16, 16), (17, 33), (2, 2), (3, 70))[i]
    kw = {}
    if i % 5 == 1:
        kw["restart_marker_blocks"] = int(rng.integers(1, 40))
    elif i % 5 == 3:
        kw["restart_marker_rows"] = int(rng.integers(1, 4))
    return encode(jpeg_cases.pixels(rng, w, h), ("4:4:4", "4:2:2", "4:2:0", None)[i % 4] or "4:2:0", int(rng.integers(30, 101)), gray=i % 4 == 3, **kw)


def random_files(seed, n, lo=1, hi=97):
    rng = np.random.default_rng(seed)
    return [case(i, rng, lo, hi) for i in range(n)]


# ---------------------------------------------------------------------------------------------------------------------------------- the scan walk
def entropy_end(data, p):
    """The end of the entropy-coded bytes that start at p: the next 0xFF followed by anything but 0x00, 0xFF or RSTn (or the end of the data)."""
    n = len(data)
    while True:
        p = data.find(b"\xff", p)
        if p < 0:
            return n
        if p + 1 >= n:
            return p
        nx = data[p + 1]
        if nx == 0 or 0xD0 <= nx <= 0xD7:
            p += 2
        elif nx == 0xFF:
            p += 1
        else:
            return p


def walk(data):
    """Every marker segment of a file: [(position, marker, payload, end)] where end is the end of the segment or, for an SOS, of its entropy-coded
    bytes; stops at EOI or at the end of the data."""
    data = bytes(data)
    n, p, out = len(data), 2, []
    while p + 4 <= n:
        while p + 1 < n and data[p] == 0xFF and data[p + 1] == 0xFF:
            p += 1
        if data[p] != 0xFF:
            raise ValueError("bad marker")
        m = data[p + 1]
        if m == 0xD9:
            break
        L = (data[p + 2] << 8) | data[p + 3]
        if L < 2 or p + 2 + L > n:
            raise ValueError("bad segment length")
        end = p + 2 + L
        if m == 0xDA:
            end = entropy_end(data, end)
        out.append((p, m, data[p + 4:p + 2 + L], end))
        p = end
    return out


def parse(data):
    """Headers and scans of a progressive file: dict(w, h, comps [(id, H, V, Tq)], qt, jfif, adobe, scans [dict(comps [(frame index, Td, Ta)], ss, se,
    ah, al, ri, dc, ac (the tables in force), ent, end)]).  NotInEnvelope for anything but SOF2."""
    data = bytes(data)
    if data[:2] != b"\xff\xd8":
        raise NotInEnvelope("not a JPEG file")
    hdr = dict(qt={}, comps=None, jfif=False, adobe=False, scans=[])
    dc, ac, ri = {}, {}, 0
    for p, m, seg, end in walk(data):
        if m == 0xC2:
            prec, h, w, nc = seg[0], (seg[1] << 8) | seg[2], (seg[3] << 8) | seg[4], seg[5]
            hdr.update(w=w, h=h, prec=prec, comps=[(seg[6 + 3 * i], seg[7 + 3 * i] >> 4, seg[7 + 3 * i] & 15, seg[8 + 3 * i]) for i in range(nc)])
        elif 0xC0 <= m <= 0xCF and m not in (0xC4, 0xC8, 0xCC):
            raise NotInEnvelope(f"SOF{m - 0xC0}")
        elif m == 0xC4:
            q = 0
            while q < len(seg):
                tc, th = seg[q] >> 4, seg[q] & 15
                bits = list(seg[q + 1:q + 17])
                vals = list(seg[q + 17:q + 17 + sum(bits)])
                (dc if tc == 0 else ac)[th] = (bits, vals)
                q += 17 + sum(bits)
        elif m == 0xDB:
            q = 0
            while q < len(seg):
                pq, tq = seg[q] >> 4, seg[q] & 15
                raw = np.frombuffer(seg[q + 1:q + 1 + 64 * (pq + 1)], dtype=">u2" if pq else np.uint8).astype(np.int64)
                nat = np.zeros(64, np.int64)
                nat[ZIGZAG] = raw
                hdr["qt"][tq] = nat
                q += 1 + 64 * (pq + 1)
        elif m == 0xDD:
            ri = (seg[0] << 8) | seg[1]
        elif m == 0xE0:
            hdr["jfif"] = hdr["jfif"] or seg[:5] == b"JFIF\0"
        elif m == 0xEE:
            hdr["adobe"] = hdr["adobe"] or seg[:5] == b"Adobe"
        elif m == 0xDA:
            ns = seg[0]
            ids = [c[0] for c in hdr["comps"]]
            comps = [(ids.index(seg[1 + 2 * i]), seg[2 + 2 * i] >> 4, seg[2 + 2 * i] & 15) for i in range(ns)]
            hdr["scans"].append(dict(comps=comps, ss=seg[1 + 2 * ns], se=seg[2 + 2 * ns], ah=seg[3 + 2 * ns] >> 4, al=seg[3 + 2 * ns] & 15, ri=ri,
                                     dc=dict(dc), ac=dict(ac), ent=p + 4 + len(seg), end=end))
    if hdr["comps"] is None:
        raise NotInEnvelope("no SOF2")
    return hdr


class _Bits:
    def __init__(self, seg):
        self.n = 8 * len(seg)
        self.v = int.from_bytes(seg, "big") if seg else 0
        self.p = 0

    def get(self, nb):
        if nb == 0:
            return 0
        if self.p + nb > self.n:
            raise BadData("premature end of data")
        self.p += nb
        return (self.v >> (self.n - self.p)) & ((1 << nb) - 1)

    def huff(self, tab):
        code = 0
        for l in range(1, 17):
            code = (code << 1) | self.get(1)
            if (l, code) in tab:
                return tab[(l, code)]
        raise BadData("invalid Huffman code")


def _extend(v, s):
    return v - (1 << s) + 1 if s and v < (1 << (s - 1)) else v


def _jcoef(v):
    return ((v + 32768) & 0xFFFF) - 32768


def geometry(hdr):
    """(MCUs per row, MCU rows, [(H, V)] per component as the decoder uses them) — a one-component frame is 1 x 1 whatever its SOF says."""
    comps, w, h = hdr["comps"], hdr["w"], hdr["h"]
    hv = [(1, 1)] if len(comps) == 1 else [(c[1], c[2]) for c in comps]
    hmax, vmax = max(x[0] for x in hv), max(x[1] for x in hv)
    return -(-w // (8 * hmax)), -(-h // (8 * vmax)), hv


def scan_grid(hdr, ci):
    """Blocks per row and block rows a one-component scan of component ci walks."""
    _, _, hv = geometry(hdr)
    hmax, vmax = max(x[0] for x in hv), max(x[1] for x in hv)
    cw, ch = -(-hdr["w"] * hv[ci][0] // hmax), -(-hdr["h"] * hv[ci][1] // vmax)
    return -(-cw // 8), -(-ch // 8)


def decode_coefficients(hdr, data):
    """Quantised coefficients after every scan, natural order: one int array [blocks_y, blocks_x, 64] per component (the MCU-padded grid)."""
    mx, my, hv = geometry(hdr)
    coef = [np.zeros((my * V, mx * H, 64), np.int64) for H, V in hv]
    for sc in hdr["scans"]:
        ss, se, ah, al = sc["ss"], sc["se"], sc["ah"], sc["al"]
        comps = sc["comps"]
        if len(comps) == 1:
            ci = comps[0][0]
            gw, gh = scan_grid(hdr, ci)
            units = [[(ci, 0, n // gw, n % gw)] for n in range(gw * gh)]
        else:
            units = [[(ci, si, (m // mx) * hv[ci][1] + y, (m % mx) * hv[ci][0] + x) for si, (ci, _, _) in enumerate(comps)
                      for y in range(hv[ci][1]) for x in range(hv[ci][0])] for m in range(mx * my)]
        ri = sc["ri"] or len(units)
        nseg = -(-len(units) // ri)
        segs, rst = R.segments(data[:sc["end"]], sc["ent"])
        if len(segs) < nseg or any(r != 0xD0 + (k % 8) for k, r in enumerate(rst[:nseg - 1])):
            raise BadData("restart markers")
        dct = [R._decoder(*sc["dc"][td]) if ss == 0 and ah == 0 else None for _, td, _ in comps]
        act = R._decoder(*sc["ac"][comps[0][2]]) if ss > 0 else None
        p1, m1 = 1 << al, -(1 << al)
        for s in range(nseg):
            b = _Bits(segs[s])
            pred = [0] * len(comps)
            eobrun = 0
            for unit in units[s * ri:(s + 1) * ri]:
                for ci, si, by, bx in unit:
                    blk = coef[ci][by, bx]
                    if ss == 0 and ah == 0:
                        t = b.huff(dct[si])
                        if t > 15:
                            raise BadData("DC size")
                        pred[si] += _extend(b.get(t), t)
                        blk[0] = _jcoef(pred[si] << al)
                    elif ss == 0:
                        if b.get(1):
                            blk[0] |= p1
                    elif ah == 0:
                        if eobrun > 0:
                            eobrun -= 1
                            continue
                        k = ss
                        while k <= se:
                            rs = b.huff(act)
                            r, sz = rs >> 4, rs & 15
                            if sz:
                                k += r
                                if k > se:
                                    raise BadData("coefficient index past the band")
                                blk[ZIGZAG[k]] = _jcoef(_extend(b.get(sz), sz) << al)
                            elif r == 15:
                                k += 15
                            else:
                                eobrun = (1 << r) + (b.get(r) if r else 0) - 1
                                break
                            k += 1
                    else:
                        k = ss
                        if eobrun == 0:
                            while k <= se:
                                rs = b.huff(act)
                                r, sz = rs >> 4, rs & 15
                                if sz:
                                    if sz != 1:
                                        raise BadData("refinement size")
                                    val = p1 if b.get(1) else m1
                                elif r != 15:
                                    eobrun = (1 << r) + (b.get(r) if r else 0)
                                    break
                                while k <= se:
                                    z = ZIGZAG[k]
                                    if blk[z] != 0:
                                        if b.get(1) and (blk[z] & p1) == 0:
                                            blk[z] += p1 if blk[z] >= 0 else m1
                                    else:
                                        r -= 1
                                        if r < 0:
                                            break
                                    k += 1
                                if sz:
                                    if k > se:
                                        raise BadData("coefficient index past the band")
                                    blk[ZIGZAG[k]] = val
                                k += 1
                        if eobrun > 0:
                            while k <= se:
                                z = ZIGZAG[k]
                                if blk[z] != 0 and b.get(1) and (blk[z] & p1) == 0:
                                    blk[z] += p1 if blk[z] >= 0 else m1
                                k += 1
                            eobrun -= 1
    return coef


def pixels_of(hdr, coef):
    """The coefficient arrays through jpeg_restate's dequantise / IDCT / upsample / colour steps."""
    comps, w, h = hdr["comps"], hdr["w"], hdr["h"]
    planes = [R._plane(R.idct_islow(c, hdr["qt"][comps[i][3]])) for i, c in enumerate(coef)]
    if len(comps) == 1:
        return np.repeat(planes[0][:h, :w][:, :, None], 3, axis=2)
    H, V = comps[0][1], comps[0][2]
    dw, dh = -(-w // H), -(-h // V)
    return R.ycc_to_rgb(planes[0][:h, :w].astype(np.int64), R.upsample(planes[1], H, V, dw, dh)[:h, :w], R.upsample(planes[2], H, V, dw, dh)[:h, :w])


def decode(data):
    """np.asarray(Image.open(f).convert("RGB")) of a progressive file inside the envelope."""
    hdr = parse(data)
    return pixels_of(hdr, decode_coefficients(hdr, bytes(data)))


def script_ok(hdr):
    """The envelope's rules for a scan script (include/lpi_hip.h): complete and orderly."""
    nc = len(hdr["comps"])
    cur = [[-1] * 64 for _ in range(nc)]
    if len(hdr["scans"]) > MAX_SCANS or not hdr["scans"]:
        return False
    for sc in hdr["scans"]:
        cs = [c[0] for c in sc["comps"]]
        ss, se, ah, al = sc["ss"], sc["se"], sc["ah"], sc["al"]
        if cs != sorted(set(cs)) or al > 13 or ss > se or se > 63 or (ss == 0 and se != 0) or (ss > 0 and len(cs) != 1) or (ah and al != ah - 1):
            return False
        for c in cs:
            if ss > 0 and cur[c][0] < 0:
                return False
            for k in range(ss, se + 1):
                if cur[c][k] != (ah if ah else -1):
                    return False
                cur[c][k] = al
    return all(v == 0 for c in cur for v in c)


# ---------------------------------------------------------------------------------------------------------------------------------- the re-encoder
class _Out:
    def __init__(self):
        self.acc, self.nb, self.out = 0, 0, bytearray()

    def put(self, v, nb):
        self.acc = (self.acc << nb) | (v & ((1 << nb) - 1))
        self.nb += nb
        while self.nb >= 8:
            byte = (self.acc >> (self.nb - 8)) & 255
            self.out.append(byte)
            if byte == 0xFF:
                self.out.append(0)
            self.nb -= 8
        self.acc &= (1 << self.nb) - 1

    def flush(self):
        if self.nb:
            self.put((1 << (8 - self.nb)) - 1, 8 - self.nb)


DC_VALS = list(range(12))                                                               # 4-bit codes
AC_VALS = [0x00, 0xF0] + [r << 4 for r in range(1, 15)] + [(r << 4) | s for r in range(16) for s in range(1, 11)]       # 8-bit codes


def _dht(tc, th, vals, length):
    bits = [0] * 16
    bits[length - 1] = len(vals)
    return b"\xff\xc4" + (19 + len(vals)).to_bytes(2, "big") + bytes([(tc << 4) | th]) + bytes(bits) + bytes(vals)


def _mag(v):
    s = abs(int(v)).bit_length()
    return s, (int(v) if v >= 0 else int(v) + (1 << s) - 1)


def baseline_coefficients(data):
    """(header, coefficient arrays) of a baseline file (tests/jpeg_restate.py)."""
    hdr = R.parse(data)
    return hdr, R.decode_coefficients(hdr, bytes(data))


def reencode(hdr, coef, script, marker=0xC2):
    """A progressive file with the frame and quantisation tables of hdr and the coefficients coef (the MCU-padded arrays), written scan by scan after
    script: [(frame components, Ss, Se, restart interval)], first-pass scans only (Ah = Al = 0).  Fixed Huffman tables (every DC size a 4-bit code,
    every AC symbol an 8-bit code), EOB runs across blocks, a DRI segment wherever the interval changes (0 switches the markers off)."""
    comps, w, h = hdr["comps"], hdr["w"], hdr["h"]
    nc = len(comps)
    mx, my, hv = geometry(hdr)
    out = bytearray(b"\xff\xd8\xff\xe0\x00\x10JFIF\x00\x01\x01\x00\x00\x01\x00\x01\x00\x00")
    for tq in sorted({c[3] for c in comps}):
        out += b"\xff\xdb\x00\x43" + bytes([tq]) + bytes(int(v) for v in hdr["qt"][tq][ZIGZAG])
    out += b"\xff" + bytes([marker]) + (8 + 3 * nc).to_bytes(2, "big") + b"\x08" + h.to_bytes(2, "big") + w.to_bytes(2, "big") + bytes([nc])
    for cid, H, V, tq in comps:
        out += bytes([cid, (H << 4) | V, tq])
    out += _dht(0, 0, DC_VALS, 4) + _dht(1, 0, AC_VALS, 8)
    ac_code = {v: i for i, v in enumerate(AC_VALS)}
    ri_now = 0
    for cs, ss, se, ri in script:
        if ri != ri_now:
            out += b"\xff\xdd\x00\x04" + ri.to_bytes(2, "big")
            ri_now = ri
        out += b"\xff\xda" + (6 + 2 * len(cs)).to_bytes(2, "big") + bytes([len(cs)]) + b"".join(bytes([comps[c][0], 0]) for c in cs) + bytes([ss, se, 0])
        if len(cs) == 1:
            gw, gh = scan_grid(hdr, cs[0])
            units = [[(cs[0], 0, n // gw, n % gw)] for n in range(gw * gh)]
        else:
            units = [[(ci, si, (m // mx) * hv[ci][1] + y, (m % mx) * hv[ci][0] + x) for si, ci in enumerate(cs)
                      for y in range(hv[ci][1]) for x in range(hv[ci][0])] for m in range(mx * my)]
        o = _Out()
        state = dict(eobrun=0)

        def flush_eob():
            e = state["eobrun"]
            if e:
                nb = e.bit_length() - 1
                o.put(ac_code[nb << 4], 8)
                o.put(e - (1 << nb), nb)
                state["eobrun"] = 0

        pred = [0] * len(cs)
        for n, unit in enumerate(units):
            if ri and n and n % ri == 0:
                flush_eob()
                o.flush()
                o.out += bytes([0xFF, 0xD0 + ((n // ri - 1) & 7)])
                pred = [0] * len(cs)
            for ci, si, by, bx in unit:
                blk = coef[ci][by, bx]
                if ss == 0:
                    s, bits = _mag(int(blk[0]) - pred[si])
                    pred[si] = int(blk[0])
                    o.put(DC_VALS.index(s), 4)
                    o.put(bits, s)
                    continue
                r = 0
                for k in range(ss, se + 1):
                    v = int(blk[ZIGZAG[k]])
                    if v == 0:
                        r += 1
                        continue
                    flush_eob()
                    while r > 15:
                        o.put(ac_code[0xF0], 8)
                        r -= 16
                    s, bits = _mag(v)
                    o.put(ac_code[(r << 4) | s], 8)
                    o.put(bits, s)
                    r = 0
                if r:
                    state["eobrun"] += 1
                    if state["eobrun"] == 0x7FFF:
                        flush_eob()
        flush_eob()
        o.flush()
        out += o.out
    return bytes(out + b"\xff\xd9")


def spectral_script(nc, ri=(0,)):
    """Spectral selection only: one interleaved DC scan, then the bands 1-9 and 10-63 of every component; ri: the restart intervals, cycled."""
    scans = [(list(range(nc)), 0, 0)] + [([c], a, b) for c in range(nc) for a, b in ((1, 9), (10, 63))]
    return [s + (ri[i % len(ri)],) for i, s in enumerate(scans)]


def split_dc_script(nc, ri=(0,)):
    """One DC scan per component (each walks the component's own block grid), then one AC scan 1-63 per component, chroma first."""
    scans = [([c], 0, 0) for c in range(nc)] + [([c], 1, 63) for c in reversed(range(nc))]
    return [s + (ri[i % len(ri)],) for i, s in enumerate(scans)]


# ---------------------------------------------------------------------------------------------------------------------------------- file surgery
def chunks(data):
    """(head, [scan chunks], tail): head ends behind the SOF2 segment's successors up to the first scan's tables; a scan chunk is the DHT / DRI
    segments in front of an SOS, the SOS and its entropy-coded bytes; tail is EOI."""
    data = bytes(data)
    segs = walk(data)
    sof = max(i for i, s in enumerate(segs) if s[1] == 0xC2)
    out, start = [], segs[sof][3]
    for p, m, _, end in segs[sof + 1:]:
        if m == 0xDA:
            out.append(data[start:end])
            start = end
    return data[:segs[sof][3]], out, data[start:]


def join(head, scan_chunks, tail=b"\xff\xd9"):
    return head + b"".join(scan_chunks) + tail


def patch_sos(chunk, ns=None, ahal=None, extra_component=None):
    """A scan chunk with another Ah/Al byte, or with a second component (id) added to its SOS."""
    i = chunk.index(b"\xff\xda")
    L = (chunk[i + 2] << 8) | chunk[i + 3]
    body = bytearray(chunk[i + 4:i + 2 + L])
    if ahal is not None:
        body[-1] = ahal
    if extra_component is not None:
        body = bytearray([body[0] + 1]) + body[1:1 + 2 * body[0]] + bytearray([extra_component, body[2]]) + body[1 + 2 * body[0]:]
    return chunk[:i] + b"\xff\xda" + (len(body) + 2).to_bytes(2, "big") + bytes(body) + chunk[i + 2 + L:]


def with_sof(data, marker):
    """The file with another SOFn marker in place of SOF2."""
    data = bytes(data)
    p = next(s[0] for s in walk(data) if s[1] == 0xC2)
    return data[:p + 1] + bytes([marker]) + data[p + 2:]


def cmyk_progressive(rng, w=40, h=24):
    from PIL import Image, ImageFile
    old = ImageFile.MAXBLOCK
    ImageFile.MAXBLOCK = max(old, 1 << 24)
    try:
        buf = io.BytesIO()
        Image.fromarray(rng.integers(0, 256, (h, w, 4), dtype=np.uint8), "CMYK").save(buf, "JPEG", quality=85, progressive=True)
        return buf.getvalue()
    finally:
        ImageFile.MAXBLOCK = old
