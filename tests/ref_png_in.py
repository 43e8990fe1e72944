"""PNG files in, restated: the definition of what cvhip_png_decode returns.  tests/ref_png.py is the
encoder's.  parse - the chunk walk (png_decode_common.hpp); inflate - a pure-Python RFC 1950 / 1951 decoder with its own
error rules and statistics (pinned to zlib.decompress on every valid scene by tests/test_png_in_ref.py); unfilter - the five
filters a byte at a time (unfilter_fast: the same along anti-diagonals in numpy, pinned to it); decode - the samples and
their conversion to Luma8 and RGB8.

Defined here, not pinned to the `image` crate: 16-bit samples are big-endian and reduce by (v + 128) // 257; 1/2/4-bit grey
scales by 255 // (2^bits - 1); a palette index becomes its PLTE entry; alpha and tRNS are dropped; the luma of a colour pixel
is (2126 r + 7152 g + 722 b) // 10000 (of 16-bit samples in 16 bits, then reduced); gAMA / sRGB / iCCP are ignored.
Code lengths: over-subscribed ones are refused, incomplete ones too unless no code is longer than one bit (zlib's rule: the
single-code table RFC 1951 allows, and the table without codes, whose use is the error); HLIT above 286 and HDIST above 30
are refused as zlib refuses them.  Bytes behind the Adler-32 are ignored; distances up to 32 768 are accepted whatever CINFO
says."""
import struct
import zlib

import numpy as np

OK, INVALID, UNSUPPORTED = 0, -1, -3
LUMA8, RGB8 = 0, 1
SIGNATURE = b"\x89PNG\r\n\x1a\n"
CL_ORDER = (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)
LEGAL = {0: (1, 2, 4, 8, 16), 2: (8, 16), 3: (1, 2, 4, 8), 4: (8, 16), 6: (8, 16)}
CHANNELS = {0: 1, 2: 3, 3: 1, 4: 2, 6: 4}


class PngError(Exception):
    def __init__(self, code, why):
        super().__init__(why)
        self.code = code


def _bad(why):
    return PngError(INVALID, why)


def exif_focal_length_35mm(tiff: bytes) -> int:
    """FocalLengthIn35mmFilm of a bare TIFF structure: IFD0 -> 0x8769 -> 0xA405, SHORT or LONG, count 1; 0 = none."""
    n = len(tiff)
    if n < 8 or tiff[:2] not in (b"II", b"MM"):
        return 0
    o = "<" if tiff[:2] == b"II" else ">"
    if struct.unpack_from(o + "H", tiff, 2)[0] != 42:
        return 0

    def find(ifd, tag, short_too):
        if ifd + 2 > n:
            return None
        for k in range(struct.unpack_from(o + "H", tiff, ifd)[0]):
            at = ifd + 2 + 12 * k
            if at + 12 > n:
                return None
            t, kind, count = struct.unpack_from(o + "HHI", tiff, at)
            if t != tag:
                continue
            if count != 1 or not (kind == 4 or (short_too and kind == 3)):
                return None
            return struct.unpack_from(o + ("H" if kind == 3 else "I"), tiff, at + 8)[0]
        return None

    sub = find(struct.unpack_from(o + "I", tiff, 4)[0], 0x8769, False)
    if sub is None:
        return 0
    return find(sub, 0xA405, True) or 0


def parse(data: bytes) -> dict:
    """The chunk walk up to IEND.  The CRC of every chunk but the IDATs is checked here; theirs by decode()."""
    n = len(data)
    if n < 8 or data[:8] != SIGNATURE:
        raise _bad("no PNG signature")
    h = {"focal_length_35mm": 0, "flags": 0, "palette": b"", "idat": []}
    at, first, in_idat = 8, True, False
    while True:
        if n - at < 12:
            raise _bad("no IEND" if at == n else "a chunk runs past the file")
        length = struct.unpack_from(">I", data, at)[0]
        if length > n - at - 12:
            raise _bad("a chunk runs past the file")
        typ, body = data[at + 4:at + 8], data[at + 8:at + 8 + length]
        crc = struct.unpack_from(">I", data, at + 8 + length)[0]
        if first and (typ != b"IHDR" or length != 13):
            raise _bad("the first chunk is not a 13-byte IHDR")
        if typ != b"IDAT" and zlib.crc32(typ + body) != crc:
            raise _bad("a chunk's CRC")
        if typ == b"IHDR":
            if not first:
                raise _bad("a second IHDR")
            w, hh, depth, colour, comp, filt, lace = struct.unpack(">IIBBBBB", body)
            if w == 0 or hh == 0:
                raise _bad("a zero dimension")
            if depth not in LEGAL.get(colour, ()):
                raise _bad("an illegal colour type / bit depth pair")
            if comp or filt:
                raise _bad("a compression or filter method other than 0")
            if lace > 1:
                raise _bad("an interlace method above 1")
            if lace == 1:
                raise PngError(UNSUPPORTED, "Adam7 interlacing")
            if w >= 65536 or hh >= 65536:
                raise PngError(UNSUPPORTED, "a dimension of 65 536 or more")
            channels = CHANNELS[colour]
            h.update(width=w, height=hh, colour=colour, depth=depth, interlace=lace, channels=channels,
                     bpp=max(1, channels * depth // 8), row_bytes=(w * channels * depth + 7) // 8)
            if (h["row_bytes"] + 1) * hh >= 1 << 31:
                raise PngError(UNSUPPORTED, "a filtered image of 2^31 bytes or more")
        elif typ == b"PLTE":
            if h["palette"] or h["idat"]:
                raise _bad("a PLTE out of place")
            if length == 0 or length % 3 or length > 768:
                raise _bad("a PLTE whose length is not 3 .. 768 in threes")
            h["palette"], h["flags"] = bytes(body), h["flags"] | 1
        elif typ == b"IDAT":
            if h["idat"] and not in_idat:
                raise _bad("IDAT chunks that are not consecutive")
            h["idat"].append((at + 8, length, crc))
        elif typ == b"IEND":
            if not h["idat"]:
                raise _bad("no IDAT")
            if h["colour"] == 3 and not h["palette"]:
                raise _bad("colour type 3 without PLTE")
            return h
        elif typ == b"tRNS":
            h["flags"] |= 2
        elif typ == b"eXIf":
            if h["focal_length_35mm"] == 0:
                h["focal_length_35mm"] = exif_focal_length_35mm(bytes(body))
        elif not typ[0] & 0x20:
            raise _bad("an unknown critical chunk")
        in_idat, first = typ == b"IDAT", False
        at += length + 12


def info(data: bytes) -> tuple:
    """cvhip_png_info's out_info[8]."""
    h = parse(data)
    return (h["width"], h["height"], h["colour"], h["depth"], h["interlace"], len(h["idat"]), h["focal_length_35mm"], h["flags"])


def stream_of(data: bytes, h=None) -> bytes:
    h = h or parse(data)
    return b"".join(data[o:o + n] for o, n, _crc in h["idat"])


# ---- inflate ------------------------------------------------------------------------------------------------------------------
def build_code(lengths):
    """(length, code) -> symbol of the canonical code; refuses over-subscribed and (beyond one bit) incomplete lengths."""
    count = [0] * 16
    for n in lengths:
        count[n] += 1
    count[0] = 0
    left, longest = 1, 0
    for bits in range(1, 16):
        left = left * 2 - count[bits]
        if left < 0:
            raise _bad("over-subscribed code lengths")
        if count[bits]:
            longest = bits
    if left > 0 and longest > 1:
        raise _bad("incomplete code lengths")
    code, nxt = 0, [0] * 16
    for bits in range(1, 16):
        code = (code + count[bits - 1]) << 1
        nxt[bits] = code
    table = {}
    for s, n in enumerate(lengths):
        if n:
            table[(n, nxt[n])] = s
            nxt[n] += 1
    return table, longest


FIXED_LENGTHS = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8, [5] * 32


class _Bits:
    def __init__(self, data):
        self.d, self.p, self.n = bytes(data) + b"\0" * 8, 0, len(data) * 8

    def take(self, k):
        v = (int.from_bytes(self.d[self.p >> 3:(self.p >> 3) + 8], "little") >> (self.p & 7)) & ((1 << k) - 1)
        self.p += k
        if self.p > self.n:
            raise _bad("the stream ends before the final block's end-of-block")
        return v

    def symbol(self, table):
        code = 0
        for n in range(1, 16):
            code = code << 1 | self.take(1)
            s = table.get((n, code))
            if s is not None:
                return s, n
        raise _bad("a code that is not in its table")


def inflate(stream: bytes, want=None):
    """-> (the bytes, stats).  stats: stored / fixed / dynamic block counts, blocks (type, first bit, bits, output bytes,
    longest code used), longest_code, max_distance, max_length, extra13 (a distance code with 13 extra bits was used),
    overlaps (the distances below their length), zero_stored, repeat16_crosses, dist_none (a dynamic block without a
    distance code), dist_single, empty_blocks (only an end-of-block), back_blocks (the most blocks a copy reached back
    over), stored_after (the bit alignments, mod 8, of the block ends a stored block followed), adler_at."""
    stream = bytes(stream)
    if len(stream) < 2:
        raise _bad("the stream ends before the final block's end-of-block")
    cmf, flg = stream[0], stream[1]
    if cmf & 15 != 8 or cmf >> 4 > 7 or flg & 32 or (cmf << 8 | flg) % 31:
        raise _bad("the zlib header")
    b = _Bits(stream)
    b.p = 16
    out = bytearray()
    st = {"stored": 0, "fixed": 0, "dynamic": 0, "blocks": [], "longest_code": 0, "max_distance": 0, "max_length": 0, "extra13": False,
          "overlaps": set(), "zero_stored": 0, "repeat16_crosses": 0, "dist_none": 0, "dist_single": 0, "empty_blocks": 0, "back_blocks": 0,
          "stored_after": set()}
    starts = []  # the output position at which each block began
    final, prev_end = 0, None
    while not final:
        first_bit = b.p
        final, btype = b.take(1), b.take(2)
        before = len(out)
        starts.append(before)
        longest_used = 0
        if btype == 3:
            raise _bad("block type 3")
        if btype == 0:
            if prev_end is not None:
                st["stored_after"].add(prev_end % 8)
            b.p = (b.p + 7) & ~7
            length, nlen = b.take(16), b.take(16)
            if length ^ 0xFFFF != nlen:
                raise _bad("a stored block whose NLEN is not ~LEN")
            if b.p + 8 * length > b.n:
                raise _bad("the stream ends before the final block's end-of-block")
            out += stream[b.p >> 3:(b.p >> 3) + length]
            b.p += 8 * length
            st["stored"] += 1
            st["zero_stored"] += length == 0
        else:
            if btype == 1:
                lit_lengths, dist_lengths = FIXED_LENGTHS
                st["fixed"] += 1
            else:
                hlit, hdist, hclen = b.take(5) + 257, b.take(5) + 1, b.take(4) + 4
                if hlit > 286 or hdist > 30:
                    raise _bad("too many length or distance symbols")
                cl = [0] * 19
                for i in range(hclen):
                    cl[CL_ORDER[i]] = b.take(3)
                cl_table, _ = build_code(cl)
                lengths = []
                while len(lengths) < hlit + hdist:
                    s, _n = b.symbol(cl_table)
                    if s < 16:
                        lengths.append(s)
                        continue
                    if s == 16:
                        if not lengths:
                            raise _bad("a repeat code 16 with nothing before it")
                        value, repeat = lengths[-1], 3 + b.take(2)
                        st["repeat16_crosses"] += len(lengths) < hlit < len(lengths) + repeat
                    elif s == 17:
                        value, repeat = 0, 3 + b.take(3)
                    else:
                        value, repeat = 0, 11 + b.take(7)
                    if len(lengths) + repeat > hlit + hdist:
                        raise _bad("code lengths running past HLIT + HDIST")
                    lengths += [value] * repeat
                lit_lengths, dist_lengths = lengths[:hlit], lengths[hlit:]
                if lit_lengths[256] == 0:
                    raise _bad("no code for symbol 256")
                st["dynamic"] += 1
                st["dist_none"] += not any(dist_lengths)
                st["dist_single"] += sum(1 for n in dist_lengths if n) == 1
            lit, _ = build_code(lit_lengths)
            dist, _ = build_code(dist_lengths)
            while True:
                s, n = b.symbol(lit)
                longest_used = max(longest_used, n)
                if s < 256:
                    out.append(s)
                    continue
                if s == 256:
                    break
                if s >= 286:
                    raise _bad("a literal/length symbol 286 or 287")
                if s < 265:
                    length = s - 254
                elif s < 285:
                    e = (s - 261) >> 2
                    length = 3 + ((4 + ((s - 261) & 3)) << e) + b.take(e)
                else:
                    length = 258
                d, n = b.symbol(dist)
                longest_used = max(longest_used, n)
                if d >= 30:
                    raise _bad("a distance symbol 30 or 31")
                if d < 4:
                    distance = d + 1
                else:
                    e = (d >> 1) - 1
                    distance = 1 + ((2 + (d & 1)) << e) + b.take(e)
                    st["extra13"] |= e == 13
                if distance > len(out):
                    raise _bad("a distance reaching before the first output byte")
                st["max_distance"], st["max_length"] = max(st["max_distance"], distance), max(st["max_length"], length)
                if distance < length:
                    st["overlaps"].add(distance)
                source = len(out) - distance
                st["back_blocks"] = max(st["back_blocks"], sum(1 for at in starts if at > source))
                for k in range(length):
                    out.append(out[source + k])
            st["empty_blocks"] += len(out) == before
        st["blocks"].append((btype, first_bit, b.p - first_bit, len(out) - before, longest_used))
        st["longest_code"] = max(st["longest_code"], longest_used)
        prev_end = b.p
    at = (b.p + 7) // 8
    if at + 4 > len(stream):
        raise _bad("the stream ends before the final block's end-of-block")
    if want is not None and len(out) != want:
        raise _bad("output that is not height x (1 + row bytes) bytes")
    if struct.unpack_from(">I", stream, at)[0] != zlib.adler32(bytes(out)):
        raise _bad("a wrong Adler-32")
    st["adler_at"] = at
    return bytes(out), st


# ---- the filters --------------------------------------------------------------------------------------------------------------
def _paeth(a, b, c):
    p = a + b - c
    pa, pb, pc = abs(p - a), abs(p - b), abs(p - c)
    return a if pa <= pb and pa <= pc else b if pb <= pc else c


def unfilter(filtered: bytes, height: int, row_bytes: int, bpp: int) -> np.ndarray:
    """[height, row_bytes] uint8, a byte at a time (the definition)."""
    rows = np.zeros((height, row_bytes), dtype=np.uint8)
    up = [0] * row_bytes
    for y in range(height):
        base = y * (row_bytes + 1)
        t = filtered[base]
        if t > 4:
            raise _bad("a filter-type byte above 4")
        cur = [0] * row_bytes
        for i in range(row_bytes):
            a = cur[i - bpp] if i >= bpp else 0
            c = up[i - bpp] if i >= bpp else 0
            pred = 0 if t == 0 else a if t == 1 else up[i] if t == 2 else (a + up[i]) >> 1 if t == 3 else _paeth(a, up[i], c)
            cur[i] = (filtered[base + 1 + i] + pred) & 255
        rows[y] = cur
        up = cur
    return rows


def unfilter_fast(filtered: bytes, height: int, row_bytes: int, bpp: int) -> np.ndarray:
    """unfilter along anti-diagonals (pixel x of row y at step x + y), vectorised over the rows."""
    f = np.frombuffer(bytes(filtered), dtype=np.uint8).reshape(height, row_bytes + 1)
    types = f[:, 0].astype(np.int64)
    if (types > 4).any():
        raise _bad("a filter-type byte above 4")
    npix = row_bytes // bpp
    x = f[:, 1:].astype(np.int64).reshape(height, npix, bpp)
    out = np.zeros((height + 1, npix + 1, bpp), dtype=np.int64)  # a row of zeros above, a pixel of zeros to the left
    ys = np.arange(height)
    for step in range(height + npix - 1):
        y = ys[max(0, step - npix + 1):min(height, step + 1)]
        px = step - y
        a, b, c = out[y + 1, px], out[y, px + 1], out[y, px]
        p = a + b - c
        pa, pb, pc = abs(p - a), abs(p - b), abs(p - c)
        pae = np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, b, c))
        t = types[y][:, None]
        pred = np.where(t == 0, 0, np.where(t == 1, a, np.where(t == 2, b, np.where(t == 3, (a + b) >> 1, pae))))
        out[y + 1, px + 1] = (x[y, px] + pred) & 255
    return out[1:, 1:].reshape(height, row_bytes).astype(np.uint8)


# ---- the pixels ---------------------------------------------------------------------------------------------------------------
def samples_of(rows: np.ndarray, h: dict) -> np.ndarray:
    """[height, width, channels] of the samples as integers."""
    w, depth, ch = h["width"], h["depth"], h["channels"]
    if depth == 8:
        s = rows.astype(np.int64)
    elif depth == 16:
        s = rows[:, 0::2].astype(np.int64) << 8 | rows[:, 1::2].astype(np.int64)
    else:
        bits = np.unpackbits(rows, axis=1)[:, :w * depth].reshape(rows.shape[0], w, depth).astype(np.int64)
        s = np.zeros((rows.shape[0], w), dtype=np.int64)
        for k in range(depth):
            s = s << 1 | bits[:, :, k]
    return s.reshape(rows.shape[0], w, ch)


def convert(samples: np.ndarray, h: dict) -> dict:
    """-> luma [h, w] and rgb [h, w, 3], uint8."""
    colour, depth = h["colour"], h["depth"]
    reduce16 = lambda v: (v + 128) // 257
    if colour in (0, 4):
        v = samples[:, :, 0]
        g = reduce16(v) if depth == 16 else v if depth == 8 else v * (255 // ((1 << depth) - 1))
        return {"luma": g.astype(np.uint8), "rgb": np.repeat(g[:, :, None], 3, axis=2).astype(np.uint8)}
    if colour == 3:
        pal = np.frombuffer(h["palette"], dtype=np.uint8).reshape(-1, 3).astype(np.int64)
        if (samples[:, :, 0] >= len(pal)).any():
            raise _bad("a palette index beyond the PLTE")
        rgb = pal[samples[:, :, 0]]
    else:
        rgb = samples[:, :, :3]
    luma = (2126 * rgb[:, :, 0] + 7152 * rgb[:, :, 1] + 722 * rgb[:, :, 2]) // 10000
    if depth == 16:
        rgb, luma = reduce16(rgb), reduce16(luma)
    return {"luma": luma.astype(np.uint8), "rgb": rgb.astype(np.uint8)}


def decode(data: bytes, inflater=None, fast=False) -> dict:
    """-> luma, rgb, samples, header, stats.  inflater: a stand-in for inflate's bytes (zlib.decompress, which the CPU tests
    pin inflate to) for pictures too large for the pure-Python one; fast: unfilter_fast."""
    h = parse(data)
    for o, n, crc in h["idat"]:
        if zlib.crc32(b"IDAT" + data[o:o + n]) != crc:
            raise _bad("a chunk's CRC")
    want = h["height"] * (h["row_bytes"] + 1)
    stream = stream_of(data, h)
    if inflater is None:
        filtered, stats = inflate(stream, want)
    else:
        filtered, stats = inflater(stream), None
        if len(filtered) != want:
            raise _bad("output that is not height x (1 + row bytes) bytes")
    rows = (unfilter_fast if fast else unfilter)(filtered, h["height"], h["row_bytes"], h["bpp"])
    samples = samples_of(rows, h)
    return {**convert(samples, h), "samples": samples, "header": h, "stats": stats, "filtered": filtered}
