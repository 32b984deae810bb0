"""A numpy restatement of what Pillow 12 (libjpeg-turbo 3.1, default settings) does to a baseline JPEG inside the envelope of lpi_jpeg_decode_u8:
np.asarray(Image.open(f).convert("RGB")).  It is the yardstick of lpi_amd/csrc/jpeg.hip and is pinned to Pillow itself by the CPU suite
(tests/test_image_jpeg_host.py).  Step by step, as libjpeg does it:

- Huffman decoding of one sequential scan (DC differences, AC run/size pairs, restart intervals that reset the DC predictors);
- the integer "islow" IDCT of jidctint.c (CONST_BITS 13, PASS1_BITS 2) with its 10-bit range limit (x & 1023 -> sample);
- "fancy" chroma upsampling (jdsample.c): 2x1 = the 3:1 triangle filter with biases 1 / 2, 2x2 = the 3:1 filter in both directions with biases 8 / 7;
  edge columns / rows replicated at the component's downsampled size; a plain replicating upsample when the chroma plane is at most 2 samples wide;
- YCbCr -> RGB with jdcolor.c's 16-bit fixed-point tables;
- grayscale replicated into R, G, B (convert("RGB") of an "L" image).

Small images only: the entropy decoder is plain Python."""
import numpy as np

ZIGZAG = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28, 35, 42, 49, 56,
                   57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63])


class NotInEnvelope(Exception):
    """The file is valid but outside the GPU decoder's envelope (progressive, CMYK, Adobe, other sampling, ...)."""


def parse(data):
    """Headers of a JPEG byte string -> dict(w, h, comps [(id, H, V, Tq)], qt {Tq: natural-order int array}, dc / ac {Th: (bits, vals)}, scan
    [(frame index, Td, Ta)], ri, jfif, adobe, ent (offset of the entropy-coded data)).  ValueError on a structural error; NotInEnvelope."""
    data = bytes(data)
    n = len(data)
    if n < 4 or data[0] != 0xFF or data[1] != 0xD8:
        raise NotInEnvelope("not a JPEG file")
    p, hdr = 2, dict(qt={}, dc={}, ac={}, ri=0, jfif=False, adobe=False, comps=None)
    while True:
        while p < n and data[p] == 0xFF and p + 1 < n and data[p + 1] == 0xFF:
            p += 1
        if p + 4 > n or data[p] != 0xFF:
            raise ValueError("truncated header or bad marker")
        m = data[p + 1]
        L = (data[p + 2] << 8) | data[p + 3]
        if L < 2 or p + 2 + L > n:
            raise ValueError("bad segment length")
        seg = data[p + 4:p + 2 + L]
        p += 2 + L
        if m in (0xC0, 0xC1):
            if hdr["comps"] is not None or len(seg) < 6:
                raise ValueError("bad SOF")
            prec, h, w, nc = seg[0], (seg[1] << 8) | seg[2], (seg[3] << 8) | seg[4], seg[5]
            if len(seg) != 6 + 3 * nc or nc < 1:
                raise ValueError("bad SOF length")
            comps = [(seg[6 + 3 * i], seg[7 + 3 * i] >> 4, seg[7 + 3 * i] & 15, seg[8 + 3 * i]) for i in range(nc)]
            if any(not (1 <= H <= 4 and 1 <= V <= 4) or tq > 3 for _, H, V, tq in comps) or w == 0:
                raise ValueError("bad SOF fields")
            hdr.update(w=w, h=h, comps=comps, prec=prec)
        elif m in (0xC2, 0xC3, 0xC5, 0xC6, 0xC7, 0xC9, 0xCA, 0xCB, 0xCD, 0xCE, 0xCF):
            raise NotInEnvelope(f"SOF{m - 0xC0}")
        elif m == 0xC4:
            q = 0
            while q < len(seg):
                if q + 17 > len(seg):
                    raise ValueError("bad DHT")
                tc, th = seg[q] >> 4, seg[q] & 15
                bits = list(seg[q + 1:q + 17])
                cnt = sum(bits)
                if tc > 1 or th > 3 or cnt > 256 or q + 17 + cnt > len(seg):
                    raise ValueError("bad DHT")
                vals = list(seg[q + 17:q + 17 + cnt])
                if tc == 0 and any(v > 15 for v in vals):
                    raise ValueError("bad DC table")
                code = 0
                for l in range(16):
                    code += bits[l]
                    if code >= (1 << (l + 1)):               # jpeg_make_d_derived_tbl: the all-ones code is not a code
                        raise ValueError("bad Huffman table")
                    code <<= 1
                (hdr["dc"] if tc == 0 else hdr["ac"])[th] = (bits, vals)
                q += 17 + cnt
        elif m == 0xDB:
            q = 0
            while q < len(seg):
                pq, tq = seg[q] >> 4, seg[q] & 15
                size = 64 * (pq + 1)
                if pq > 1 or tq > 3 or q + 1 + size > len(seg):
                    raise ValueError("bad DQT")
                raw = np.frombuffer(seg[q + 1:q + 1 + size], dtype=">u2" if pq else np.uint8).astype(np.int64)
                nat = np.zeros(64, np.int64)
                nat[ZIGZAG] = raw
                hdr["qt"][tq] = nat
                q += 1 + size
        elif m == 0xDD:
            if len(seg) != 2:
                raise ValueError("bad DRI")
            hdr["ri"] = (seg[0] << 8) | seg[1]
        elif m == 0xE0:
            if seg[:5] == b"JFIF\0":
                hdr["jfif"] = True
        elif m == 0xEE:
            if len(seg) >= 12 and seg[:5] == b"Adobe":
                hdr["adobe"] = True
        elif m == 0xDA:
            if hdr["comps"] is None or len(seg) < 1:
                raise ValueError("SOS before SOF")
            ns = seg[0]
            if len(seg) != 4 + 2 * ns or ns < 1 or ns > 4:
                raise ValueError("bad SOS length")
            ids = [c[0] for c in hdr["comps"]]
            scan = []
            for i in range(ns):
                cid, t = seg[1 + 2 * i], seg[2 + 2 * i]
                if cid not in ids or any(ids[s[0]] == cid for s in scan):
                    raise ValueError("bad scan component")
                scan.append((ids.index(cid), t >> 4, t & 15))
            ss, se, ahal = seg[1 + 2 * ns], seg[2 + 2 * ns], seg[3 + 2 * ns]
            nc = len(hdr["comps"])
            if ns != nc or ss != 0 or se != 63 or ahal != 0 or hdr["prec"] != 8 or hdr["h"] == 0:
                raise NotInEnvelope("scan")
            if [s[0] for s in scan] != list(range(ns)):          # libjpeg-turbo refuses a full scan in another order than the frame's
                raise NotInEnvelope("scan order")
            for _, td, ta in scan:
                if td not in hdr["dc"] or ta not in hdr["ac"]:
                    raise ValueError("scan uses an undefined Huffman table")
            for _, _, _, tq in hdr["comps"]:
                if tq not in hdr["qt"]:
                    raise ValueError("undefined quantisation table")
            if nc == 3:
                if hdr["adobe"] and not hdr["jfif"]:
                    raise NotInEnvelope("Adobe")
                if not hdr["jfif"] and ids == [82, 71, 66]:
                    raise NotInEnvelope("RGB")
                if (hdr["comps"][0][1], hdr["comps"][0][2]) not in ((1, 1), (2, 1), (2, 2)) or any(c[1:3] != (1, 1) for c in hdr["comps"][1:]):
                    raise NotInEnvelope("sampling")
            elif nc != 1:
                raise NotInEnvelope("components")
            hdr.update(scan=scan, ent=p)
            return hdr
        elif m in (0xD8, 0xD9) or 0xD0 <= m <= 0xD7:
            raise ValueError("unexpected marker")
        elif m == 0xCC:
            raise NotInEnvelope("arithmetic coding")


def segments(data, start):
    """The entropy-coded bytes from `start` without stuffing, split at RSTn markers, up to the first other marker: [bytes, ...], [RSTn codes]."""
    out, segs, rst = bytearray(), [], []
    i, n = start, len(data)
    while i < n:
        b = data[i]
        if b != 0xFF:
            out.append(b)
            i += 1
            continue
        nxt = data[i + 1] if i + 1 < n else None
        if nxt == 0x00:
            out.append(0xFF)
            i += 2
        elif nxt == 0xFF:
            i += 1
        elif nxt is not None and 0xD0 <= nxt <= 0xD7:
            segs.append(bytes(out))
            rst.append(nxt)
            out = bytearray()
            i += 2
        else:
            break
    segs.append(bytes(out))
    return segs, rst


def _decoder(bits, vals):
    codes, code, k = {}, 0, 0
    for l in range(1, 17):
        for _ in range(bits[l - 1]):
            codes[(l, code)] = vals[k]
            k += 1
            code += 1
        code <<= 1
    return codes


class BadData(Exception):
    """The entropy-coded data is corrupt (Pillow then has the last word)."""


def decode_coefficients(hdr, data):
    """Quantised coefficients, natural order: one int array [blocks_y, blocks_x, 64] per component (the MCU-padded block grid)."""
    comps, w, h = hdr["comps"], hdr["w"], hdr["h"]
    nc = len(comps)
    hmax, vmax = max(c[1] for c in comps), max(c[2] for c in comps)
    if nc == 1:
        mx, my, lay = -(-w // 8), -(-h // 8), [(0, 1, 1)]
    else:
        mx, my = -(-w // (8 * hmax)), -(-h // (8 * vmax))
        lay = [(ci, comps[ci][1], comps[ci][2]) for ci, _, _ in hdr["scan"]]
    coef = [np.zeros((my * (V if nc > 1 else 1), mx * (H if nc > 1 else 1), 64), np.int64) for _, H, V, _ in comps]
    tabs = [(_decoder(*hdr["dc"][td]), _decoder(*hdr["ac"][ta])) for _, td, ta in hdr["scan"]]
    segs, rst = segments(data, hdr["ent"])
    nmcu = mx * my
    ri = hdr["ri"] or nmcu
    nseg = -(-nmcu // ri)
    if len(segs) < nseg or any(r != 0xD0 + (k % 8) for k, r in enumerate(rst[:nseg - 1])):
        raise BadData("restart markers")
    for s in range(nseg):
        bitstr = np.unpackbits(np.frombuffer(segs[s], np.uint8)) if segs[s] else np.zeros(0, np.uint8)
        pos = [0]

        def get(nb):
            if pos[0] + nb > len(bitstr):
                raise BadData("premature end of data")
            v = 0
            for b in bitstr[pos[0]:pos[0] + nb]:
                v = (v << 1) | int(b)
            pos[0] += nb
            return v

        def huff(tab):
            code = 0
            for l in range(1, 17):
                code = (code << 1) | get(1)
                if (l, code) in tab:
                    return tab[(l, code)]
            raise BadData("invalid Huffman code")

        def extend(v, s):
            return v - (1 << s) + 1 if s and v < (1 << (s - 1)) else v

        pred = [0] * nc
        for m in range(s * ri, min((s + 1) * ri, nmcu)):
            for si, (ci, H, V) in enumerate(lay):
                for by in range(V):
                    for bx in range(H):
                        dct, act = tabs[si]
                        t = huff(dct)
                        if t > 15:
                            raise BadData("DC size")
                        pred[ci] += extend(get(t), t)
                        blk = np.zeros(64, np.int64)
                        blk[0] = ((pred[ci] + 32768) & 0xFFFF) - 32768        # JCOEF
                        k = 1
                        while k < 64:
                            rs = huff(act)
                            r, sz = rs >> 4, rs & 15
                            if sz:
                                k += r
                                if k > 63:
                                    raise BadData("coefficient index past 63")
                                blk[ZIGZAG[k]] = extend(get(sz), sz)
                            elif r != 15:
                                break
                            else:
                                k += 15
                            k += 1
                        coef[ci][(m // mx) * V + by, (m % mx) * H + bx] = blk
    return coef


C13 = dict(f0298=2446, f0390=3196, f0541=4433, f0765=6270, f0899=7373, f1175=9633, f1501=12299, f1847=15137, f1961=16069, f2053=16819, f2562=20995,
           f3072=25172)


def _idct_1d(s0, s1, s2, s3, s4, s5, s6, s7, shift, bias):
    c = C13
    z1 = (s2 + s6) * c["f0541"]
    tmp2 = z1 + s6 * (-c["f1847"])
    tmp3 = z1 + s2 * c["f0765"]
    tmp0 = (s0 + s4) << 13
    tmp1 = (s0 - s4) << 13
    t10, t13, t11, t12 = tmp0 + tmp3, tmp0 - tmp3, tmp1 + tmp2, tmp1 - tmp2
    o0, o1, o2, o3 = s7, s5, s3, s1
    z1, z2, z3, z4 = o0 + o3, o1 + o2, o0 + o2, o1 + o3
    z5 = (z3 + z4) * c["f1175"]
    o0, o1, o2, o3 = o0 * c["f0298"], o1 * c["f2053"], o2 * c["f3072"], o3 * c["f1501"]
    z1, z2, z3, z4 = z1 * -c["f0899"], z2 * -c["f2562"], z3 * -c["f1961"] + z5, z4 * -c["f0390"] + z5
    o0, o1, o2, o3 = o0 + z1 + z3, o1 + z2 + z4, o2 + z2 + z3, o3 + z1 + z4
    d = lambda x: (x + bias) >> shift  # noqa: E731
    return [d(t10 + o3), d(t11 + o2), d(t12 + o1), d(t13 + o0), d(t13 - o0), d(t12 - o1), d(t11 - o2), d(t10 - o3)]


def idct_islow(coef, q):
    """jidctint.c jpeg_idct_islow on blocks [..., 64] (quantised, natural order) with table q[64] -> uint8 samples [..., 8, 8]."""
    x = (coef * q).reshape(coef.shape[:-1] + (8, 8))        # [.., row v, col u]
    cols = _idct_1d(*[x[..., k, :] for k in range(8)], 11, 1 << 10)           # pass 1 over columns: per u, the 8 rows
    ws = np.stack(cols, axis=-2)                                                # [.., y, u]
    rows = _idct_1d(*[ws[..., :, k] for k in range(8)], 18, 1 << 17)           # pass 2 over rows
    v = np.stack(rows, axis=-1) & 1023                                          # [.., y, x]
    return np.where(v < 128, v + 128, np.where(v < 512, 255, np.where(v < 896, 0, v - 896))).astype(np.uint8)


def _plane(blocks):
    by, bx = blocks.shape[:2]
    return blocks.transpose(0, 2, 1, 3).reshape(by * 8, bx * 8)


def upsample(p, H, V, dw, dh):
    """jdsample.c: component plane p (its first dh rows and dw columns are real) -> the H x V upsampled plane, int64."""
    p = p[:dh, :dw].astype(np.int64)
    if H == 1 and V == 1:
        return p
    if dw <= 2:                                  # plain replication (h2v1_upsample / h2v2_upsample)
        return np.repeat(np.repeat(p, H, axis=1), V, axis=0)
    left = np.concatenate([p[:, :1], p[:, :-1]], axis=1)
    right = np.concatenate([p[:, 1:], p[:, -1:]], axis=1)
    if V == 1:
        out = np.empty((dh, 2 * dw), np.int64)
        out[:, 0::2] = (3 * p + left + 1) >> 2
        out[:, 1::2] = (3 * p + right + 2) >> 2
        return out
    up = np.concatenate([p[:1], p[:-1]], axis=0)
    down = np.concatenate([p[1:], p[-1:]], axis=0)
    out = np.empty((2 * dh, 2 * dw), np.int64)
    for v, nb in ((0, up), (1, down)):
        cs = 3 * p + nb
        csl = np.concatenate([cs[:, :1], cs[:, :-1]], axis=1)
        csr = np.concatenate([cs[:, 1:], cs[:, -1:]], axis=1)
        out[v::2, 0::2] = (3 * cs + csl + 8) >> 4
        out[v::2, 1::2] = (3 * cs + csr + 7) >> 4
    return out


def _fix(x):
    return int(x * 65536 + 0.5)


def ycc_to_rgb(y, cb, cr):
    x = np.arange(256, dtype=np.int64) - 128
    cr_r = (_fix(1.40200) * x + 32768) >> 16
    cb_b = (_fix(1.77200) * x + 32768) >> 16
    cr_g = -_fix(0.71414) * x
    cb_g = -_fix(0.34414) * x + 32768
    r = y + cr_r[cr]
    g = y + ((cb_g[cb] + cr_g[cr]) >> 16)
    b = y + cb_b[cb]
    return np.clip(np.stack([r, g, b], axis=-1), 0, 255).astype(np.uint8)


def decode(data):
    """np.asarray(Image.open(f).convert("RGB")) for a file inside the envelope.  NotInEnvelope / ValueError (headers) / BadData (entropy data)."""
    hdr = parse(data)
    coef = decode_coefficients(hdr, data)
    comps, w, h = hdr["comps"], hdr["w"], hdr["h"]
    planes = [_plane(idct_islow(c, hdr["qt"][comps[i][3]])) for i, c in enumerate(coef)]
    if len(comps) == 1:
        y = planes[0][:h, :w]
        return np.repeat(y[:, :, None], 3, axis=2)
    H, V = comps[0][1], comps[0][2]
    dw, dh = -(-w // H), -(-h // V)
    y = planes[0][:h, :w].astype(np.int64)
    cb = upsample(planes[1], H, V, dw, dh)[:h, :w]
    cr = upsample(planes[2], H, V, dw, dh)[:h, :w]
    return ycc_to_rgb(y, cb, cr)
