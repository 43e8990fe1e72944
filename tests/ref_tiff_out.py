"""The definition of cvhip_tiff_encode in numpy and plain Python: the classic little-endian TIFF file of an
8-bit image with 1 to 4 channels - the IFD, the strips, uncompressed / TIFF 6.0 LZW as libtiff writes it / PackBits per row,
Predictor 2.  The library equals encode() byte for byte.  The LZW payloads are pinned to Pillow (libtiff) by
tests/test_tiff_out_ref.py; the container and the PackBits packets are this library's own (libtiff packs rows differently)
and are pinned by decoding (ref_tiff.samples and Pillow)."""
import struct

import numpy as np

import ref_tiff

OK, INVALID, UNSUPPORTED = 0, -1, -3
NONE, LZW, PACKBITS = 1, 5, 32773
CLEAR, EOI = 256, 257
CLEAR_AFTER = 3836   # codes since a Clear: entry 4093 was the last one added (libtiff clears when 4094 would be next)
SHORT, LONG = 3, 4


class TiffOutError(Exception):
    def __init__(self, code, why=""):
        super().__init__(f"{code}: {why}")
        self.code = code


def default_rows_per_strip(row_bytes):
    """TIFF 6.0's "about 8 KB"."""
    return max(1, 8192 // row_bytes)


def predict(rows, channels):
    """Predictor 2 of [rows, row_bytes] uint8: each byte minus the byte `channels` before it in its row, modulo 256."""
    out = rows.copy()
    out[:, channels:] = rows[:, channels:] - rows[:, :-channels]
    return out


# ---- LZW -------------------------------------------------------------------------------------------------------------------
def lzw_codes(data: bytes):
    """The codes of a strip, Clear and EOI included.  Entry 258 + j is the string of code j (since the Clear) and the first
    byte of code j + 1; after the 3836th code since a Clear stands a Clear - also when that code is the strip's last, in front
    of EOI (libtiff's LZWPostEncode counts the last code like any other; tests/test_tiff_out_ref.py pins it)."""
    codes, table, prefix, c = [CLEAR], {}, -1, 0
    for byte in data:
        if prefix < 0:
            prefix = byte
            continue
        found = table.get((prefix, byte))
        if found is not None:
            prefix = found
            continue
        codes.append(prefix)
        table[(prefix, byte)] = 258 + c
        c += 1
        prefix = byte
        if c == CLEAR_AFTER:
            codes.append(CLEAR)
            table, c = {}, 0
    if prefix >= 0:
        codes.append(prefix)
        c += 1
        if c == CLEAR_AFTER:
            codes.append(CLEAR)
    codes.append(EOI)
    return codes


def lzw_pack(codes):
    """MSB first; the c-th code since a Clear is ref_tiff.code_width(c) bits wide (the Clear itself counts on, the code
    behind it is the 0th); zero bits fill the last byte."""
    acc, n, c, out = 0, 0, 0, bytearray()
    for code in codes:
        w = ref_tiff.code_width(c)
        acc, n = (acc << w) | code, n + w
        while n >= 8:
            out.append((acc >> (n - 8)) & 255)
            n -= 8
        acc &= (1 << n) - 1
        c = 0 if code == CLEAR else c + 1
    if n:
        out.append((acc << (8 - n)) & 255)
    return bytes(out)


def lzw(data: bytes) -> bytes:
    return lzw_pack(lzw_codes(data))


def lzw_stagings(data: bytes, stage):
    """The strip's codes as they leave an encoder that takes the strip `stage` bytes at a time (tiff_lzw_kernel: LZW_CHUNK),
    from the code sequence of lzw_codes alone -> per staging a dict of
      codes   the codes that leave in it: the first Clear in staging 0; a code with the byte behind its string, the byte that
              did not extend it; a table-full Clear with the same byte; the pending string, a Clear behind it and EOI in the
              last staging
      end     the bit position of the stream behind the staging's last code, modulo 32
      clears  the residues (byte index modulo `stage`) of the bytes with which a table-full Clear left
      crosses whether the staging's last code lies in two 32-bit words of the stream
    A code's string is as long as the decoder's: 1 below 256, else one more than the string of the code its entry was made
    from.  No table of (prefix, byte) pairs and no probe order: the bytes do not depend on how the strings are found."""
    codes, n = lzw_codes(data), len(data)
    count = max(1, -(-n // stage))
    out = [dict(codes=[], end=0, clears=[], crosses=False) for _ in range(count)]
    assert codes[0] == CLEAR and codes[-1] == EOI
    at, lengths, where = 0, [], [0]   # the bytes the codes so far stand for; of the codes since the Clear; the staging of each code
    for code in codes[1:-1]:
        if code == CLEAR:
            where.append(where[-1])
            if at < n:
                out[where[-1]]["clears"].append(at % stage)
            lengths = []
            continue
        length = 1 if code < 256 else lengths[code - 258] + 1
        lengths.append(length)
        at += length
        where.append(at // stage if at < n else count - 1)
    where.append(count - 1)
    assert at == n and where == sorted(where)
    bit, c = 0, 0
    for code, k in zip(codes, where):
        w = ref_tiff.code_width(c)
        s = out[k]
        s["codes"].append(code)
        s["crosses"] = bit // 32 != (bit + w - 1) // 32
        bit += w
        c = 0 if code == CLEAR else c + 1
        s["end"] = bit % 32
    for before, s in zip(out, out[1:]):   # (a staging without a code ends where the one in front of it ended)
        if not s["codes"]:
            s["end"] = before["end"]
    assert (bit + 7) // 8 == len(lzw_pack(codes))
    return out


# ---- PackBits --------------------------------------------------------------------------------------------------------------
def packbits_row(row: bytes):
    """The greedy walk of one row (tiff_scenes.packbits on the row alone) -> [(is a run, start, length)]."""
    out, at, n = [], 0, len(row)
    while at < n:
        run = 1
        while at + run < n and run < 128 and row[at + run] == row[at]:
            run += 1
        if run >= 3:
            out.append((True, at, run))
            at += run
            continue
        end = at
        while end < n and end - at < 128 and not (end + 2 < n and row[end] == row[end + 1] == row[end + 2]):
            end += 1
        out.append((False, at, end - at))
        at = end
    return out


def packbits_row_closed(row: bytes):
    """The same packets without a walk: every maximal run of 3 or more equal bytes gives run packets of 128 from its first byte
    and one of the remainder when that is 3 or more; a remainder of 1 or 2 is literal.  The literal bytes form regions (maximal
    stretches); a region is cut every 128 bytes from its start."""
    a = np.frombuffer(bytes(row), dtype=np.uint8)
    n = len(a)
    starts = np.flatnonzero(np.concatenate([[True], a[1:] != a[:-1]]))
    ends = np.concatenate([starts[1:], [n]])
    in_run = np.zeros(n, dtype=bool)
    packets = []
    for s, e in zip(starts.tolist(), ends.tolist()):
        length = e - s
        if length < 3:
            continue
        rest = length % 128
        covered = length if rest >= 3 or rest == 0 else length - rest
        in_run[s:s + covered] = True
        for at in range(s, s + covered, 128):
            packets.append((True, at, min(128, s + covered - at)))
    lit = np.flatnonzero(~in_run)
    if len(lit):
        region_starts = lit[np.concatenate([[True], lit[1:] != lit[:-1] + 1])]
        region_ends = lit[np.concatenate([lit[1:] != lit[:-1] + 1, [True]])] + 1
        for s, e in zip(region_starts.tolist(), region_ends.tolist()):
            for at in range(s, e, 128):
                packets.append((False, at, min(128, e - at)))
    return sorted(packets, key=lambda p: p[1])


def packbits_bytes(row: bytes, packets) -> bytes:
    out = bytearray()
    for run, at, length in packets:
        if run:
            out += bytes([257 - length, row[at]])
        else:
            out += bytes([length - 1]) + row[at:at + length]
    return bytes(out)


# ---- the file --------------------------------------------------------------------------------------------------------------
def check(width, height, channels, compression, predictor, rows_per_strip):
    """The refusals, in the library's order -> (row_bytes, rows per strip, strips)."""
    if width == 0 or height == 0:
        raise TiffOutError(INVALID, "width or height 0")
    if not 1 <= channels <= 4:
        raise TiffOutError(INVALID, "channels")
    if compression not in (NONE, LZW, PACKBITS):
        raise TiffOutError(INVALID, "compression")
    if predictor not in (1, 2):
        raise TiffOutError(INVALID, "predictor")
    if predictor == 2 and compression != LZW:
        raise TiffOutError(INVALID, "Predictor 2 without LZW")
    if width >= 65536 or height >= 65536:
        raise TiffOutError(UNSUPPORTED, "a dimension of 65536 or more")
    row_bytes = width * channels
    rps = min(rows_per_strip or default_rows_per_strip(row_bytes), height)
    if rps * row_bytes >= 2 ** 31:
        raise TiffOutError(UNSUPPORTED, "a strip of 2^31 bytes or more")
    strips = -(-height // rps)
    if compression == NONE:   # (the size is known without the pixels; a compressed file is measured)
        last = (height - (strips - 1) * rps) * row_bytes
        full = rps * row_bytes
        size = header(width, height, channels, compression, predictor, rps, strips)[1] + (strips - 1) * (full + (full & 1)) + last
        if size >= 2 ** 32:
            raise TiffOutError(UNSUPPORTED, "a file of 2^32 bytes or more")
    return row_bytes, rps, strips


def worst_strip(compression, rows, row_bytes):
    """The bound on a strip's bytes that the library holds its scratch by."""
    n = rows * row_bytes
    if compression == NONE:
        return n
    if compression == PACKBITS:
        return rows * (row_bytes + -(-row_bytes // 128))
    codes = n + 2 + n // CLEAR_AFTER + 1   # a code a byte, the first Clear and EOI, the Clears
    return (12 * codes + 7) // 8


def header(width, height, channels, compression, predictor, rps, strips, first_offset=0, first_count=0):
    """The bytes in front of the StripOffsets array (or of the strips, when there is one strip: its offset and count stand
    inline) -> (bytes, where the strips begin).  first_offset / first_count: of the one strip."""
    entries = [(256, LONG, [width]), (257, LONG, [height]), (258, SHORT, [8] * channels), (259, SHORT, [compression]),
               (262, SHORT, [1 if channels <= 2 else 2]), (273, LONG, None), (277, SHORT, [channels]), (278, LONG, [rps]),
               (279, LONG, None), (284, SHORT, [1])]
    if predictor == 2:
        entries.append((317, SHORT, [2]))
    if channels in (2, 4):
        entries.append((338, SHORT, [2]))
    at = 8 + 2 + 12 * len(entries) + 4
    tail, fields = b"", b""
    data_at = at + (2 * channels if channels > 2 else 0) + (8 * strips if strips > 1 else 0)
    for tag, kind, values in entries:
        if values is None:
            count = strips
            if strips == 1:
                value = struct.pack("<I", data_at if tag == 273 else first_count)
            else:
                value = struct.pack("<I", at)
                at += 4 * strips
        else:
            count = len(values)
            packed = struct.pack("<" + ("H" if kind == SHORT else "I") * count, *values)
            if len(packed) > 4:
                value = struct.pack("<I", at)
                tail += packed
                at += len(packed)
            else:
                value = packed.ljust(4, b"\0")
        fields += struct.pack("<HHI", tag, kind, count) + value
    assert first_offset in (0, data_at) and at == data_at
    return b"II" + struct.pack("<HI", 42, 8) + struct.pack("<H", len(entries)) + fields + b"\0\0\0\0" + tail, data_at


def encode(pixels, compression=LZW, predictor=1, rows_per_strip=0, stats=None, sections=None) -> bytes:
    """pixels: [height, width] or [height, width, channels] uint8 -> the file.  stats (a dict): strips, codes, clears, packets.
    sections (a list): the bytes before the first strip, the strips with their padding, 0."""
    a = np.ascontiguousarray(pixels, dtype=np.uint8)
    if a.ndim == 2:
        a = a[:, :, None]
    height, width, channels = a.shape
    row_bytes, rps, strips = check(width, height, channels, compression, predictor, rows_per_strip)
    rows = a.reshape(height, row_bytes)
    if predictor == 2:
        rows = predict(rows, channels)
    payloads, codes, clears, packets = [], 0, 0, 0
    for s in range(strips):
        part = rows[s * rps:(s + 1) * rps]
        if compression == NONE:
            payloads.append(part.tobytes())
        elif compression == LZW:
            cs = lzw_codes(part.tobytes())
            codes, clears = codes + len(cs), clears + cs.count(CLEAR)
            payloads.append(lzw_pack(cs))
        else:
            out = b""
            for row in part:
                ps = packbits_row(row.tobytes())
                packets += len(ps)
                out += packbits_bytes(row.tobytes(), ps)
            payloads.append(out)
    head, data_at = header(width, height, channels, compression, predictor, rps, strips, first_count=len(payloads[0]))
    body, offsets = bytearray(), []
    for p in payloads:
        if len(body) & 1:
            body.append(0)
        offsets.append(data_at + len(body))
        body += p
    if data_at + len(body) >= 2 ** 32:
        raise TiffOutError(UNSUPPORTED, "a file of 2^32 bytes or more")
    if strips > 1:
        head += struct.pack("<%dI" % strips, *offsets) + struct.pack("<%dI" % strips, *(len(p) for p in payloads))
    assert len(head) == data_at
    if stats is not None:
        stats.update(strips=strips, codes=codes, clears=clears, packets=packets)
    if sections is not None:
        sections[:] = [data_at, len(body), 0]
    return head + bytes(body)


def strips_of(data: bytes):
    """[(offset, count)] of a file of encode() (also of 2 channels, which ref_tiff refuses)."""
    tags = {}
    for k in range(struct.unpack_from("<H", data, 8)[0]):
        tag, kind, count, value = struct.unpack_from("<HHII", data, 10 + 12 * k)
        tags[tag] = (count, value)
    n = tags[273][0]
    if n == 1:
        return [(tags[273][1], tags[279][1])]
    return list(zip(struct.unpack_from("<%dI" % n, data, tags[273][1]), struct.unpack_from("<%dI" % n, data, tags[279][1])))
