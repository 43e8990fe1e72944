"""The definition of cvhip_jpeg_decode's pixels, restated sequentially in Python and numpy: the marker walk,
the tables, the EXIF focal length, the sequential Huffman decode, libjpeg's jidctint in 64-bit integers with a clamp, its
fancy upsampling, its fixed-point YCbCr to RGB, and the luma of `into_luma8`.

Pinned: the RGB8 of an encoder-made baseline file equals Pillow's (libjpeg-turbo's) `convert("RGB")` byte for byte
(tests/test_jpeg_ref.py).  NOT pinned: LUMA - (2126 r + 7152 g + 722 b) / 10000 truncated is the `image` crate's integer
sRGB luma as remembered from 0.25; the crate's text is not at hand, so this is an assumption that no test checks against
the crate (as cvref_resize states for its Lanczos3).  Beyond what an encoder emits (coefficients times a 16-bit DQT entry)
this file is the definition: 64-bit integers and a clamp to 0..255, where libjpeg's range table wraps."""
import struct

import numpy as np

INVALID, UNSUPPORTED = -1, -3
LUMA8, RGB8 = 0, 1
ZIGZAG = [0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
          35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63]


class JpegError(ValueError):
    def __init__(self, code, msg):
        super().__init__(msg)
        self.code = code


def _fail(code, msg):
    raise JpegError(code, msg)


def exif_focal_length_35mm(tiff):
    """FocalLengthIn35mmFilm of the TIFF block behind `Exif\\0\\0`: IFD0 -> 0x8769 -> 0xA405 (SHORT or LONG); 0 = none (a
    missing or broken block is none, as get_metadata falls back)."""
    n = len(tiff)
    if n < 8 or tiff[:2] not in (b"II", b"MM"):
        return 0
    e = "<" if tiff[:2] == b"II" else ">"
    if struct.unpack(e + "H", tiff[2:4])[0] != 42:
        return 0

    def find(ifd, tag, kinds):
        if ifd + 2 > n:
            return None
        count = struct.unpack(e + "H", tiff[ifd:ifd + 2])[0]
        for k in range(count):
            at = ifd + 2 + 12 * k
            if at + 12 > n:
                return None
            t, kind, cnt = struct.unpack(e + "HHI", tiff[at:at + 8])
            if t == tag:
                if kind not in kinds or cnt != 1:
                    return None
                return struct.unpack(e + ("H" if kind == 3 else "I"), tiff[at + 8:at + (10 if kind == 3 else 12)])[0]
        return None

    sub = find(struct.unpack(e + "I", tiff[4:8])[0], 0x8769, (4,))
    if sub is None:
        return 0
    return find(sub, 0xA405, (3, 4)) or 0


def parse(data):
    """The marker walk up to the scan -> dict.  Raises JpegError(INVALID | UNSUPPORTED)."""
    data = bytes(data)
    n = len(data)
    if n < 4 or data[0] != 0xFF or data[1] != 0xD8:
        _fail(INVALID, "no SOI")
    at = 2
    quant, huff, frame, restart, focal, adobe = {}, {}, None, 0, 0, None
    while True:
        if at >= n or data[at] != 0xFF:
            _fail(INVALID, "no marker")
        while at < n and data[at] == 0xFF:
            at += 1
        if at >= n:
            _fail(INVALID, "the file ends in a marker")
        m = data[at]
        at += 1
        if m == 0xD9 or m == 0xD8 or 0xD0 <= m <= 0xD7 or m == 0x00:
            _fail(INVALID, "marker %02X before the scan" % m)
        if m == 0x01:
            continue
        if at + 2 > n:
            _fail(INVALID, "truncated segment")
        length = data[at] << 8 | data[at + 1]
        if length < 2 or at + length > n:
            _fail(INVALID, "truncated segment")
        seg = data[at + 2:at + length]
        if m == 0xDB:
            k = 0
            while k < len(seg):
                pq, tq = seg[k] >> 4, seg[k] & 15
                if pq > 1 or tq > 3 or k + 1 + 64 * (pq + 1) > len(seg):
                    _fail(INVALID, "DQT")
                vals = [seg[k + 1 + i] if pq == 0 else seg[k + 1 + 2 * i] << 8 | seg[k + 2 + 2 * i] for i in range(64)]
                table = [0] * 64
                for i in range(64):
                    table[ZIGZAG[i]] = vals[i]
                quant[tq] = table
                k += 1 + 64 * (pq + 1)
        elif m == 0xC4:
            k = 0
            while k < len(seg):
                if k + 17 > len(seg):
                    _fail(INVALID, "DHT")
                tc, th = seg[k] >> 4, seg[k] & 15
                counts = list(seg[k + 1:k + 17])
                total = sum(counts)
                if tc > 1 or th > 3 or total > 256 or k + 17 + total > len(seg):
                    _fail(INVALID, "DHT")
                symbols = list(seg[k + 17:k + 17 + total])
                code, s, lut = 0, 0, np.zeros(65536, dtype=np.uint16)
                for bits in range(1, 17):
                    for _ in range(counts[bits - 1]):
                        if code >= (1 << bits):
                            _fail(INVALID, "DHT: the code space is overfull")
                        if tc == 0 and symbols[s] > 15:
                            _fail(INVALID, "DHT: a DC category above 15")
                        lut[code << (16 - bits):(code + 1) << (16 - bits)] = bits << 8 | symbols[s]
                        code, s = code + 1, s + 1
                    code <<= 1
                huff[(tc, th)] = {"counts": counts, "symbols": symbols, "lut": lut}
                k += 17 + total
        elif m == 0xDD:
            if len(seg) != 2:
                _fail(INVALID, "DRI")
            restart = seg[0] << 8 | seg[1]
        elif m == 0xC0:
            if frame is not None:
                _fail(INVALID, "two frames")
            if len(seg) < 6:
                _fail(INVALID, "SOF")
            p, h, w, nf = seg[0], seg[1] << 8 | seg[2], seg[3] << 8 | seg[4], seg[5]
            if len(seg) != 6 + 3 * nf:
                _fail(INVALID, "SOF")
            if p == 12:
                _fail(UNSUPPORTED, "12-bit")
            if p != 8:
                _fail(INVALID, "precision")
            if h == 0:
                _fail(UNSUPPORTED, "DNL")
            if w == 0:
                _fail(INVALID, "width 0")
            if nf in (2, 4):
                _fail(UNSUPPORTED, "2 or 4 components")
            if nf not in (1, 3):
                _fail(INVALID, "components")
            comps = [{"id": seg[6 + 3 * c], "h": seg[7 + 3 * c] >> 4, "v": seg[7 + 3 * c] & 15, "tq": seg[8 + 3 * c]} for c in range(nf)]
            for c in comps:
                if not 1 <= c["h"] <= 4 or not 1 <= c["v"] <= 4 or c["tq"] > 3:
                    _fail(INVALID, "SOF")
            if nf == 1:
                comps[0]["h"] = comps[0]["v"] = 1  # (a single component is never interleaved: its factors do not count)
            elif (comps[0]["h"], comps[0]["v"]) not in ((1, 1), (2, 1), (2, 2)) or any((c["h"], c["v"]) != (1, 1) for c in comps[1:]):
                _fail(UNSUPPORTED, "sampling")
            frame = {"width": w, "height": h, "comps": comps}
        elif 0xC1 <= m <= 0xCF and m not in (0xC4, 0xC8, 0xCC):
            _fail(UNSUPPORTED, "SOF%d" % (m - 0xC0))
        elif m == 0xCC:
            _fail(UNSUPPORTED, "arithmetic conditioning")
        elif m == 0xDC:
            _fail(UNSUPPORTED, "DNL")
        elif m == 0xE1 and seg[:6] == b"Exif\0\0" and focal == 0:
            focal = exif_focal_length_35mm(seg[6:])
        elif m == 0xEE and len(seg) >= 12 and seg[:5] == b"Adobe":
            adobe = seg[11]
        elif m == 0xDA:
            if frame is None:
                _fail(INVALID, "a scan before the frame")
            nf = len(frame["comps"])
            if len(seg) < 1 or len(seg) != 4 + 2 * seg[0]:
                _fail(INVALID, "SOS")
            ns = seg[0]
            if ns < 1 or ns > 4:
                _fail(INVALID, "SOS")
            if ns != nf:
                _fail(UNSUPPORTED, "more than one scan")
            for c in range(ns):
                comp = frame["comps"][c]
                if seg[1 + 2 * c] != comp["id"]:
                    _fail(UNSUPPORTED, "the scan's components are not the frame's in order")
                comp["td"], comp["ta"] = seg[2 + 2 * c] >> 4, seg[2 + 2 * c] & 15
                if comp["td"] > 3 or comp["ta"] > 3:
                    _fail(INVALID, "SOS")
                if (0, comp["td"]) not in huff or (1, comp["ta"]) not in huff or comp["tq"] not in quant:
                    _fail(INVALID, "a missing table")
            if nf == 3 and adobe is not None and adobe != 1:
                _fail(UNSUPPORTED, "an Adobe transform that is not YCbCr")
            start = at + length
            end = start
            while end < n:  # the scan ends at the first FF that is followed by neither 00, FF nor RSTn (or at the file's end)
                end = data.find(b"\xff", end)
                if end < 0 or end + 1 >= n:
                    end = n
                    break
                nx = data[end + 1]
                if nx == 0 or nx == 0xFF or 0xD0 <= nx <= 0xD7:
                    end += 1 if nx == 0xFF else 2
                    continue
                break
            k = end  # what follows the scan: a second scan or DNL is not built
            while k + 1 < n:
                if data[k] != 0xFF:
                    break
                while k < n and data[k] == 0xFF:
                    k += 1
                if k >= n or data[k] == 0xD9:
                    break
                if data[k] == 0xDC:
                    _fail(UNSUPPORTED, "DNL")
                if data[k] == 0xDA:
                    _fail(UNSUPPORTED, "more than one scan")
                if k + 2 >= n:
                    break
                k += 1 + (data[k + 1] << 8 | data[k + 2])
            hmax, vmax = frame["comps"][0]["h"], frame["comps"][0]["v"]
            mx, my = -(-frame["width"] // (8 * hmax)), -(-frame["height"] // (8 * vmax))
            return {**frame, "quant": quant, "huff": huff, "restart": restart, "scan": (start, end), "focal_length_35mm": focal,
                    "hmax": hmax, "vmax": vmax, "mcus_x": mx, "mcus_y": my, "data": data}
        at += length


def info(data):
    h = parse(data)
    return {"width": h["width"], "height": h["height"], "components": len(h["comps"]), "h": h["hmax"], "v": h["vmax"],
            "focal_length_35mm": h["focal_length_35mm"]}


def segments(h):
    """The scan cut at its RSTn markers -> the unstuffed bytes of every restart interval.  A data byte is one that is not the
    00 behind an FF, not an FF in front of an FF (fill), and no part of an RSTn marker."""
    data = h["data"]
    s0, s1 = h["scan"]
    mcus = h["mcus_x"] * h["mcus_y"]
    want = -(-mcus // h["restart"]) if h["restart"] else 1
    out, cur, i = [], bytearray(), s0
    while i < s1:
        b = data[i]
        if b == 0xFF and i + 1 < s1:
            nx = data[i + 1]
            if nx == 0:
                cur.append(0xFF)
                i += 2
                continue
            if nx == 0xFF:
                i += 1
                continue
            if nx != 0xD0 + (len(out) & 7) or len(out) + 1 >= want:  # (0xD0..0xD7 by the scan's range)
                _fail(INVALID, "a misnumbered or surplus RSTn")
            out.append(bytes(cur))
            cur = bytearray()
            i += 2
            continue
        cur.append(b)
        i += 1
    out.append(bytes(cur))
    if len(out) != want:
        _fail(INVALID, "a missing RSTn")
    return out


def entropy_decode(h):
    """-> coefficients [blocks, 64] int16 in natural order with the DC values summed (16-bit wrap), blocks in scan order; and
    what the decode met: the longest code, the bits of the longest block, the range of the DC sums before the wrap."""
    comps = h["comps"]
    slots = [c for c, comp in enumerate(comps) for _ in range(comp["h"] * comp["v"])]
    bpm = len(slots)
    mcus = h["mcus_x"] * h["mcus_y"]
    ri = h["restart"] or mcus
    coef = np.zeros((mcus * bpm, 64), dtype=np.int16)
    met = {"longest_code": 0, "longest_block_bits": 0, "dc_min": 0, "dc_max": 0}
    dc_lut = [h["huff"][(0, comps[c]["td"])]["lut"].tolist() for c in range(len(comps))]
    ac_lut = [h["huff"][(1, comps[c]["ta"])]["lut"].tolist() for c in range(len(comps))]
    block = 0
    for s, seg in enumerate(segments(h)):
        nbits = 8 * len(seg)
        buf = seg + b"\xff" * 8
        p = 0
        pred = [0] * len(comps)
        plain = [0] * len(comps)   # the sums without the wrap: what they leave is what the wrap is there for
        for _ in range(min(ri, mcus - s * ri) * bpm):
            c = slots[block % bpm]
            p0 = p
            row = [0] * 64
            k = 0
            while k < 64:
                i = p >> 3
                w = buf[i] << 24 | buf[i + 1] << 16 | buf[i + 2] << 8 | buf[i + 3]
                e = (dc_lut if k == 0 else ac_lut)[c][(w >> (16 - (p & 7))) & 0xFFFF]
                if e == 0:
                    _fail(INVALID, "a code that is not in its table")
                length, sym = e >> 8, e & 255
                met["longest_code"] = max(met["longest_code"], length)
                p += length
                run, size = (0, sym) if k == 0 else (sym >> 4, sym & 15)
                if k > 0 and size == 0:
                    if run == 15:
                        if k + 16 > 64:
                            _fail(INVALID, "a run past coefficient 63")
                        k += 16
                    else:
                        k = 64
                else:
                    k += run
                    if k > 63:
                        _fail(INVALID, "a run past coefficient 63")
                    v = 0
                    if size:
                        i = p >> 3
                        w = buf[i] << 24 | buf[i + 1] << 16 | buf[i + 2] << 8 | buf[i + 3]
                        v = (w >> (32 - (p & 7) - size)) & ((1 << size) - 1)
                        if v < (1 << (size - 1)):
                            v -= (1 << size) - 1
                        p += size
                    row[ZIGZAG[k]] = v
                    k += 1
                if p > nbits:
                    _fail(INVALID, "the data ends before the last MCU")
            plain[c] += row[0]
            met["dc_min"], met["dc_max"] = min(met["dc_min"], plain[c]), max(met["dc_max"], plain[c])
            pred[c] = (pred[c] + row[0]) & 0xFFFF
            row[0] = pred[c]
            coef[block] = np.array(row, dtype=np.int64).astype(np.uint16).view(np.int16)
            met["longest_block_bits"] = max(met["longest_block_bits"], p - p0)
            block += 1
    return coef, met


C = {"0_298": 2446, "0_390": 3196, "0_541": 4433, "0_765": 6270, "0_899": 7373, "1_175": 9633, "1_501": 12299, "1_847": 15137, "1_961": 16069,
     "2_053": 16819, "2_562": 20995, "3_072": 25172}


def _idct_pass(v, shift):
    """jidctint's one-dimensional pass over axis 1 of v [n, 8, 8] int64 (the eight inputs v[:, k, :]) -> the eight outputs."""
    z2, z3 = v[:, 2], v[:, 6]
    z1 = (z2 + z3) * C["0_541"]
    tmp2 = z1 - z3 * C["1_847"]
    tmp3 = z1 + z2 * C["0_765"]
    tmp0 = (v[:, 0] + v[:, 4]) << 13
    tmp1 = (v[:, 0] - v[:, 4]) << 13
    tmp10, tmp13, tmp11, tmp12 = tmp0 + tmp3, tmp0 - tmp3, tmp1 + tmp2, tmp1 - tmp2
    tmp0, tmp1, tmp2, tmp3 = v[:, 7], v[:, 5], v[:, 3], v[:, 1]
    z1, z2, z3, z4 = tmp0 + tmp3, tmp1 + tmp2, tmp0 + tmp2, tmp1 + tmp3
    z5 = (z3 + z4) * C["1_175"]
    tmp0, tmp1, tmp2, tmp3 = tmp0 * C["0_298"], tmp1 * C["2_053"], tmp2 * C["3_072"], tmp3 * C["1_501"]
    z1, z2, z3, z4 = -z1 * C["0_899"], -z2 * C["2_562"], -z3 * C["1_961"] + z5, -z4 * C["0_390"] + z5
    tmp0, tmp1, tmp2, tmp3 = tmp0 + z1 + z3, tmp1 + z2 + z4, tmp2 + z2 + z3, tmp3 + z1 + z4
    out = [tmp10 + tmp3, tmp11 + tmp2, tmp12 + tmp1, tmp13 + tmp0, tmp13 - tmp0, tmp12 - tmp1, tmp11 - tmp2, tmp10 - tmp3]
    return np.stack([(o + (1 << (shift - 1))) >> shift for o in out], axis=1)


def idct(coef, quant):
    """coef [n, 64] int16, quant [64] (natural order) -> [n, 8, 8] uint8."""
    v = (coef.astype(np.int64) * np.array(quant, dtype=np.int64)).reshape(-1, 8, 8)
    ws = _idct_pass(v, 11)                                   # columns: the inputs are the rows of a column
    out = _idct_pass(ws.transpose(0, 2, 1), 18).transpose(0, 2, 1)  # rows
    return np.clip(out + 128, 0, 255).astype(np.uint8)


def planes(h, coef):
    """-> per component its whole plane of blocks (padding included) as uint8."""
    comps = h["comps"]
    bpm = sum(c["h"] * c["v"] for c in comps)
    mx, my = h["mcus_x"], h["mcus_y"]
    out, slot = [], 0
    for comp in comps:
        ch, cv = comp["h"], comp["v"]
        plane = np.zeros((my, cv, 8, mx, ch, 8), dtype=np.uint8)
        for by in range(cv):
            for bx in range(ch):
                px = idct(coef[slot + by * ch + bx::bpm], h["quant"][comp["tq"]]).reshape(my, mx, 8, 8)
                plane[:, by, :, :, bx, :] = px.transpose(0, 2, 1, 3)
        slot += ch * cv
        out.append(plane.reshape(my * cv * 8, mx * ch * 8))
    return out


def upsample(plane, dw, dh, hs, vs):
    """libjpeg's fancy upsampling of the dh x dw samples that count by hs x vs (1x1, 2x1 or 2x2) -> [dh * vs, dw * hs]."""
    p = plane[:dh, :dw].astype(np.int64)
    if hs == 1 and vs == 1:
        return p
    if dw <= 2:
        return np.repeat(np.repeat(p, vs, axis=0), hs, axis=1)
    left, right = np.concatenate([p[:, :1], p[:, :-1]], axis=1), np.concatenate([p[:, 1:], p[:, -1:]], axis=1)
    if vs == 1:
        out = np.empty((dh, 2 * dw), dtype=np.int64)
        out[:, 0::2] = (3 * p + left + 1) >> 2
        out[:, 1::2] = (3 * p + right + 2) >> 2
        out[:, 0], out[:, -1] = p[:, 0], p[:, -1]
        return out
    out = np.empty((2 * dh, 2 * dw), dtype=np.int64)
    above, below = np.concatenate([p[:1], p[:-1]], axis=0), np.concatenate([p[1:], p[-1:]], axis=0)
    for k, other in ((0, above), (1, below)):
        t = 3 * p + other
        tl, tr = np.concatenate([t[:, :1], t[:, :-1]], axis=1), np.concatenate([t[:, 1:], t[:, -1:]], axis=1)
        out[k::2, 0::2] = (3 * t + tl + 8) >> 4
        out[k::2, 1::2] = (3 * t + tr + 7) >> 4
        out[k::2, 0], out[k::2, -1] = (4 * t[:, 0] + 8) >> 4, (4 * t[:, -1] + 7) >> 4
    return out


def decode(data, mode=RGB8, drop_rows=0, met=None):
    """The file -> [H - drop_rows, W] (LUMA8) or [H - drop_rows, W, 3] (RGB8) uint8."""
    h = parse(data)
    w, hh = h["width"], h["height"]
    if drop_rows >= hh:
        _fail(INVALID, "drop_rows >= H")
    coef, m = entropy_decode(h)
    if met is not None:
        met.update(m)
    pl = planes(h, coef)
    if len(pl) == 1:
        y = pl[0][:hh, :w]
        out = y if mode == LUMA8 else np.repeat(y[:, :, None], 3, axis=2)
        return np.ascontiguousarray(out[:hh - drop_rows])
    hs, vs = h["hmax"], h["vmax"]
    y = pl[0][:hh, :w].astype(np.int64)
    dw, dh = -(-w // hs), -(-hh // vs)
    cb, cr = (upsample(p, dw, dh, hs, vs)[:hh, :w] - 128 for p in pl[1:])
    r = np.clip(y + ((91881 * cr + 32768) >> 16), 0, 255)
    b = np.clip(y + ((116130 * cb + 32768) >> 16), 0, 255)
    g = np.clip(y + ((-22554 * cb - 46802 * cr + 32768) >> 16), 0, 255)
    if mode == LUMA8:
        out = ((2126 * r + 7152 * g + 722 * b) // 10000).astype(np.uint8)
    else:
        out = np.stack([r, g, b], axis=2).astype(np.uint8)
    return np.ascontiguousarray(out[:hh - drop_rows])


def luma_of_rgb(rgb):
    rgb = np.asarray(rgb).astype(np.int64)
    return ((2126 * rgb[..., 0] + 7152 * rgb[..., 1] + 722 * rgb[..., 2]) // 10000).astype(np.uint8)


def calibration_matrix(width, height, focal_length_35mm):
    """SourceImage::calibration_matrix (reconstruction.rs:164-185) in f64; 0 / None falls back to 1."""
    diagonal_35mm = np.sqrt(np.float64(24.0 * 24.0 + 36.0 * 36.0))
    diagonal = np.sqrt(np.float64(width) * np.float64(width) + np.float64(height) * np.float64(height))
    f = np.float64(focal_length_35mm or 1) * diagonal / diagonal_35mm
    return np.array([[f, 0.0, width / 2.0], [0.0, f, height / 2.0], [0.0, 0.0, 1.0]], dtype=np.float64)
