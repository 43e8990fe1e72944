"""The definition of cvhip_tiff_info / cvhip_tiff_decode in numpy: the walk of a classic TIFF file's first
IFD, the SEM text block of tag 34683 / 34682 (src/reconstruction.rs:80-144 rule for rule, with Rust's str::parse grammar
and an exact decimal -> f32 rounding), the strips' decompression (none, TIFF 6.0 LZW as libtiff reads it, PackBits),
Predictor 2 and the conversion to Luma8 / RGB8.  The decompressed samples are pinned to Pillow (libtiff) by
tests/test_tiff_ref.py; the 16 -> 8 bit rule, the luma rule, the WhiteIsZero inversion and the dropped fourth sample are
into_luma8 / into_rgb8 as remembered, not pinned to the `image` crate."""
from fractions import Fraction

import numpy as np

OK, INVALID, UNSUPPORTED = 0, -1, -3
LUMA8, RGB8 = 0, 1
DROP_DATABAR = 0xFFFFFFFF
TYPE_SIZE = {1: 1, 2: 1, 3: 2, 4: 4, 5: 8, 6: 1, 7: 1, 8: 2, 9: 4, 10: 8, 11: 4, 12: 8, 13: 4}
SCALARS = (256, 257, 259, 262, 266, 277, 278, 284, 317)
ARRAYS = (258, 273, 279, 338, 339)
TILE_TAGS = (322, 323, 324, 325)


class TiffError(Exception):
    def __init__(self, code, why=""):
        super().__init__(f"{code}: {why}")
        self.code = code


# ---- Rust's str::parse::<f32> / ::<u32> ------------------------------------------------------------------------------------
def _digits(s, at):
    end = at
    while end < len(s) and "0" <= s[end] <= "9":
        end += 1
    return end


def round_f32(x: Fraction) -> np.float32:
    """The f32 nearest to the non-negative rational x, ties to even (one rounding)."""
    if x == 0:
        return np.float32(0.0)
    e = x.numerator.bit_length() - x.denominator.bit_length()
    if Fraction(2) ** e > x:
        e -= 1
    e = max(e, -126)
    ulp = Fraction(2) ** (e - 23)
    q = x / ulp
    m = q.numerator // q.denominator
    rest = q - m
    if rest > Fraction(1, 2) or (rest == Fraction(1, 2) and (m & 1)):
        m += 1
    value = m * ulp
    if value >= Fraction(2) ** 128:
        return np.float32(np.inf)
    return np.float32(float(value))   # (exact: 24 bits in a double)


def parse_f32(s: str):
    """str::parse::<f32> -> np.float32 or None."""
    at, sign = 0, 1.0
    if s[:1] in ("+", "-"):
        sign, at = (-1.0 if s[0] == "-" else 1.0), 1
    body = s[at:]
    if body.lower() in ("inf", "infinity"):
        return np.float32(sign * np.inf)
    if body.lower() == "nan":
        return np.float32(np.nan)
    if not body.isascii():
        return None
    i = _digits(body, 0)
    whole, frac = body[:i], ""
    if body[i:i + 1] == ".":
        j = _digits(body, i + 1)
        frac, i = body[i + 1:j], j
    if not whole and not frac:
        return None
    exp = 0
    if body[i:i + 1] in ("e", "E") and i < len(body):
        k = i + 1
        esign = 1
        if body[k:k + 1] in ("+", "-"):
            esign, k = (-1 if body[k] == "-" else 1), k + 1
        j = _digits(body, k)
        if j == k:
            return None
        exp, i = esign * int(body[k:j]), j
    if i != len(body):
        return None
    mant = (whole + frac).lstrip("0")
    if not mant:
        return np.float32(sign * 0.0)
    exp -= len(frac)
    if len(mant) + exp > 45:
        return np.float32(sign * np.inf)
    if len(mant) + exp < -60:
        return np.float32(sign * 0.0)
    return np.float32(sign) * round_f32(Fraction(int(mant)) * Fraction(10) ** exp)


def parse_u32(s: str):
    """str::parse::<u32> -> int or None."""
    if s[:1] == "+":
        s = s[1:]
    if not s or not s.isascii() or _digits(s, 0) != len(s):
        return None
    v = int(s)
    return v if v < 2 ** 32 else None


def _tag_value(line, parse):
    if "=" not in line:
        return None
    return parse(line.split("=", 1)[1])


def sem_text(text: str):
    """The loop of reconstruction.rs:107-136 over the block's text -> (scale_w, scale_h, tilt or None, databar_height)."""
    section, sw, sh, tilt, databar = "", None, None, None, 0
    lines = text.replace("\r", "\n").split("\n")
    if lines and lines[-1] == "":
        lines.pop()
    for line in lines:
        if line.startswith("[") and line.endswith("]"):
            section = line
            continue
        if section == "[Scan]":
            if line.startswith("PixelWidth"):
                sw = sw if sw is not None else _tag_value(line, parse_f32)
            elif line.startswith("PixelHeight"):
                sh = sh if sh is not None else _tag_value(line, parse_f32)
        elif section == "[Stage]":
            if line.startswith("StageT="):
                tilt = _tag_value(line, parse_f32)
        elif section == "[PrivateFei]" and line.startswith("DatabarHeight="):
            v = _tag_value(line, parse_u32)
            if v is not None:
                databar = v
    one = np.float32(1.0)
    return (sw if sw is not None else one, sh if sh is not None else one, tilt, databar)


def sem_bytes(raw: bytes):
    """An ASCII value as kamadak-exif splits it (at NUL bytes) and the reference joins it (a piece that is not UTF-8 is empty)."""
    text = ""
    for piece in raw.split(b"\0"):
        try:
            text += piece.decode("utf-8")
        except UnicodeDecodeError:
            pass
    return sem_text(text)


# ---- the IFD ------------------------------------------------------------------------------------------------------------
def _ifd_entries(data, order, ifd):
    """[(tag, type, count, at of the value field)] or None when the IFD does not lie in the file."""
    n = len(data)
    if ifd + 2 > n:
        return None
    count = int.from_bytes(data[ifd:ifd + 2], order)
    if ifd + 2 + 12 * count > n:
        return None
    out = []
    for k in range(count):
        at = ifd + 2 + 12 * k
        out.append((int.from_bytes(data[at:at + 2], order), int.from_bytes(data[at + 2:at + 4], order), int.from_bytes(data[at + 4:at + 8], order), at + 8))
    return out


def _value_at(data, order, kind, count, at):
    """Where the value's bytes lie (inline or at the offset), or None when they reach past the file."""
    total = TYPE_SIZE[kind] * count
    if total > 4:
        at = int.from_bytes(data[at:at + 4], order)
    return at if at + total <= len(data) else None


def _exif_focal(data, order, entries):
    def find(ents, tag, short_too):
        for t, kind, count, at in ents or []:
            if t != tag:
                continue
            if count != 1 or not (kind == 4 or (short_too and kind == 3)):
                return None
            return int.from_bytes(data[at:at + (2 if kind == 3 else 4)], order)
        return None
    sub = find(entries, 34665, False)
    if sub is None:
        return 0
    return find(_ifd_entries(data, order, sub), 0xA405, True) or 0


def parse(data: bytes) -> dict:
    data = bytes(data)
    n = len(data)
    if n < 8:
        raise TiffError(INVALID, "truncated header")
    if data[:2] == b"II":
        order = "little"
    elif data[:2] == b"MM":
        order = "big"
    else:
        raise TiffError(INVALID, "no TIFF byte order")
    magic = int.from_bytes(data[2:4], order)
    if magic == 43:
        raise TiffError(UNSUPPORTED, "BigTIFF")
    if magic != 42:
        raise TiffError(INVALID, "no TIFF magic")
    entries = _ifd_entries(data, order, int.from_bytes(data[4:8], order))
    if entries is None:
        raise TiffError(INVALID, "truncated IFD")
    tags, tiles, sem = {}, False, {}
    for tag, kind, count, at in entries:
        if tag in TILE_TAGS:
            tiles = True
        if tag in (34682, 34683) and tag not in sem:
            sem[tag] = (kind, count, at)
        if tag not in SCALARS and tag not in ARRAYS or tag in tags:
            continue
        if kind not in (3, 4) or count == 0 or (tag in SCALARS and count != 1):
            raise TiffError(INVALID, f"tag {tag}: type or count")
        where = _value_at(data, order, kind, count, at)
        if where is None:
            raise TiffError(INVALID, f"tag {tag} reaches past the file")
        size = TYPE_SIZE[kind]
        tags[tag] = [int.from_bytes(data[where + size * k:where + size * (k + 1)], order) for k in range(count)]
    if tiles:
        raise TiffError(UNSUPPORTED, "tiles")
    for tag in (256, 257, 262, 273):
        if tag not in tags:
            raise TiffError(INVALID, f"tag {tag} is missing")
    width, height = tags[256][0], tags[257][0]
    if width == 0 or height == 0:
        raise TiffError(INVALID, "width or height 0")
    if width >= 65536 or height >= 65536:
        raise TiffError(UNSUPPORTED, "a dimension of 65536 or more")
    spp = tags.get(277, [1])[0]
    if spp == 0:
        raise TiffError(INVALID, "no samples")
    if spp == 2 or spp > 4:
        raise TiffError(UNSUPPORTED, "2 samples or more than 4")
    bps = tags.get(258, [1])
    if len(bps) not in (1, spp):
        raise TiffError(INVALID, "BitsPerSample count")
    if any(b != bps[0] for b in bps) or bps[0] not in (8, 16):
        raise TiffError(UNSUPPORTED, "bits per sample")
    bps = bps[0]
    if any(f != 1 for f in tags.get(339, [1])):
        raise TiffError(UNSUPPORTED, "sample format")
    fill = tags.get(266, [1])[0]
    if fill == 2:
        raise TiffError(UNSUPPORTED, "FillOrder 2")
    if fill != 1:
        raise TiffError(INVALID, "FillOrder")
    planar = tags.get(284, [1])[0]
    if planar == 2:
        raise TiffError(UNSUPPORTED, "PlanarConfiguration 2")
    if planar != 1:
        raise TiffError(INVALID, "PlanarConfiguration")
    compression = tags.get(259, [1])[0]
    if compression not in (1, 5, 32773):
        raise TiffError(UNSUPPORTED, "compression")
    predictor = tags.get(317, [1])[0]
    if predictor == 3:
        raise TiffError(UNSUPPORTED, "Predictor 3")
    if predictor not in (1, 2):
        raise TiffError(INVALID, "Predictor")
    photometric = tags[262][0]
    if not ((spp == 1 and photometric in (0, 1)) or (spp in (3, 4) and photometric == 2)):
        raise TiffError(UNSUPPORTED, "photometric interpretation and samples")
    rps = tags.get(278, [0xFFFFFFFF])[0]
    if rps == 0:
        raise TiffError(INVALID, "RowsPerStrip 0")
    rps = min(rps, height)
    nstrips = -(-height // rps)
    row_bytes = width * spp * (bps // 8)
    if rps * row_bytes >= 2 ** 31:
        raise TiffError(UNSUPPORTED, "a strip of 2^31 bytes or more")
    offsets = tags[273]
    if len(offsets) != nstrips:
        raise TiffError(INVALID, "StripOffsets count")
    rows = [min(rps, height - s * rps) for s in range(nstrips)]
    if 279 in tags:
        counts = tags[279]
    elif compression != 1:
        raise TiffError(INVALID, "StripByteCounts is missing")
    else:
        counts = [r * row_bytes for r in rows]
    if len(counts) != nstrips:
        raise TiffError(INVALID, "StripByteCounts count")
    for s in range(nstrips):
        if counts[s] >= 2 ** 31:
            raise TiffError(UNSUPPORTED, "a strip of 2^31 bytes or more")
        if offsets[s] + counts[s] > n:
            raise TiffError(INVALID, "a strip reaches past the file")
        if compression == 1 and counts[s] < rows[s] * row_bytes:
            raise TiffError(INVALID, "a strip shorter than its rows")
        if compression == 5 and counts[s] >= 2 and data[offsets[s]] == 0 and (data[offsets[s] + 1] & 1):
            raise TiffError(UNSUPPORTED, "old-style LZW")
    found, tilt, databar, sw, sh = False, None, 0, np.float32(1.0), np.float32(1.0)
    block = sem.get(34683, sem.get(34682))
    if block is not None and block[0] == 2:
        where = _value_at(data, order, 2, block[1], block[2])
        if where is not None:
            found = True
            sw, sh, tilt, databar = sem_bytes(data[where:where + block[1]])
    return {"width": width, "height": height, "samples": spp, "bits": bps, "compression": compression, "photometric": photometric,
            "predictor": predictor, "strips": nstrips, "rows_per_strip": rps, "focal_length_35mm": _exif_focal(data, order, entries),
            "databar_height": databar, "sem": found, "tilt_angle": tilt, "scale": (sw, sh), "order": order, "offsets": offsets,
            "counts": counts, "rows": rows, "row_bytes": row_bytes}


def sem_metadata(data: bytes):
    """(scale_w, scale_h, tilt or None, databar_height, found) of a file."""
    h = parse(data)
    return (h["scale"][0], h["scale"][1], h["tilt_angle"], h["databar_height"], h["sem"])


# ---- decompression --------------------------------------------------------------------------------------------------------
def unpackbits(src: bytes, need: int) -> bytes:
    out, at = bytearray(), 0
    while len(out) < need:
        if at >= len(src):
            raise TiffError(INVALID, "PackBits: the input ends first")
        n = src[at]
        at += 1
        if n < 128:
            if at + n + 1 > len(src):
                raise TiffError(INVALID, "PackBits: the input ends first")
            out += src[at:at + n + 1]
            at += n + 1
        elif n > 128:
            if at >= len(src):
                raise TiffError(INVALID, "PackBits: the input ends first")
            out += bytes([src[at]]) * (257 - n)
            at += 1
    return bytes(out[:need])


def code_width(c: int) -> int:
    """The width of the c-th code after a Clear (c = 0 is the first): the next free entry is 257 + c."""
    return 9 if c < 254 else 10 if c < 766 else 11 if c < 1790 else 12


# libtiff's table has 5119 slots and it goes on filling them when entry 4095 is taken (no code can name those); the code that
# finds no slot left - 4862 codes after the Clear - is an error there, and so here
MAX_CODES = 5119 - 257


def unlzw(src: bytes, need: int, stats=None) -> bytes:
    """stats (a dict): codes, clears, longest, widths (a set) are added up."""
    out = bytearray()
    starts, lens = [], []   # of the c-th code since the Clear: where its string begins in out, its length
    bit, c, codes, clears, longest, widths = 0, 0, 0, 0, 0, set()
    total = 8 * len(src)
    while len(out) < need:
        w = code_width(c)
        if bit + w > total:
            raise TiffError(INVALID, "LZW: the input ends first")
        word = int.from_bytes(src[bit // 8:bit // 8 + 3].ljust(3, b"\0"), "big")
        code = (word >> (24 - w - (bit & 7))) & ((1 << w) - 1)
        bit += w
        codes += 1
        widths.add(w)
        if code == 256:
            clears += 1
            c, starts, lens = 0, [], []
            continue
        if code == 257:
            raise TiffError(INVALID, "LZW: EOI before the rows are full")
        if c >= MAX_CODES:
            raise TiffError(INVALID, "LZW: no Clear for 4862 codes")
        if code < 256:
            if c < 4096:
                starts.append(len(out)), lens.append(1)
            out.append(code)
            longest = max(longest, 1)
        else:
            j = code - 258   # entry 258 + j: the string of code j and the first byte of code j + 1
            if j >= c:
                raise TiffError(INVALID, "LZW: a code above the next entry")
            at, length = starts[j], lens[j] + 1
            if c < 4096:
                starts.append(len(out)), lens.append(length)
            for k in range(length):
                out.append(out[at + k])
            longest = max(longest, length)
        c += 1
    if stats is not None:
        stats["codes"] = stats.get("codes", 0) + codes
        stats["clears"] = stats.get("clears", 0) + clears
        stats["longest"] = max(stats.get("longest", 0), longest)
        stats.setdefault("widths", set()).update(widths)
    return bytes(out[:need])


def samples(data: bytes, stats=None):
    """(header, [height, width, samples] uint8 or uint16: the file's samples, Predictor 2 undone, nothing else applied)."""
    data = bytes(data)
    h = parse(data)
    raw = bytearray()
    for s in range(h["strips"]):
        src, need = data[h["offsets"][s]:h["offsets"][s] + h["counts"][s]], h["rows"][s] * h["row_bytes"]
        if h["compression"] == 1:
            raw += src[:need]
        elif h["compression"] == 5:
            raw += unlzw(src, need, stats)
        else:
            raw += unpackbits(src, need)
    if stats is not None:
        stats["strips"] = h["strips"]
    dtype = np.uint8 if h["bits"] == 8 else np.dtype("<u2" if h["order"] == "little" else ">u2")
    a = np.frombuffer(bytes(raw), dtype=dtype).reshape(h["height"], h["width"], h["samples"]).astype(np.uint8 if h["bits"] == 8 else np.uint16)
    if h["predictor"] == 2:
        a = np.cumsum(a.astype(np.uint32), axis=1).astype(a.dtype)   # (the wrap of the cast is the sum modulo 2^8 or 2^16)
    return h, a


def convert(h, a, fmt):
    """[height, width(, 3)] uint8 of the samples."""
    a = a.astype(np.uint32)
    top = 255 if h["bits"] == 8 else 65535
    if h["photometric"] == 0:
        a = top - a
    a = a[:, :, :3]
    if fmt == RGB8:
        if h["bits"] == 16:
            a = (a + 128) // 257
        return np.ascontiguousarray(np.repeat(a, 3, axis=2) if a.shape[2] == 1 else a).astype(np.uint8)
    luma = a[:, :, 0] if a.shape[2] == 1 else (2126 * a[:, :, 0] + 7152 * a[:, :, 1] + 722 * a[:, :, 2]) // 10000
    if h["bits"] == 16:
        luma = (luma + 128) // 257
    return luma.astype(np.uint8)


def decode(data: bytes, fmt: int = LUMA8, drop_rows: int = 0, stats=None) -> np.ndarray:
    if fmt not in (LUMA8, RGB8):
        raise TiffError(INVALID, "format")
    h = parse(data)
    if drop_rows == DROP_DATABAR:
        drop_rows = h["databar_height"]
    if drop_rows >= h["height"]:
        raise TiffError(INVALID, "drop_rows leaves no row")
    h, a = samples(data, stats)
    return np.ascontiguousarray(convert(h, a, fmt)[:h["height"] - drop_rows])


def info(data: bytes) -> dict:
    h = parse(data)
    return {k: h[k] for k in ("width", "height", "samples", "bits", "compression", "photometric", "predictor", "strips", "rows_per_strip",
                              "databar_height", "sem", "tilt_angle", "scale")} | {"focal_length_35mm": h["focal_length_35mm"] or None}
