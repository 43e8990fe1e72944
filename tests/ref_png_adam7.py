"""PNG files in, Adam7 interlaced files too, restated: the definition of what cvhip_png_ext_decode returns.
Inflate, the filters, the samples and their conversion are tests/ref_png_in.py's and are not restated; this adds the
geometry.  An interlaced stream holds seven reduced images one behind the other: pass p takes the pixels
(X0[p] + px * DX[p], Y0[p] + py * DY[p]), ceil((W - X0) / DX) x ceil((H - Y0) / DY) of them; a pass with no column or no
row has no bytes at all, not even filter bytes; each pass is `ph` rows of 1 + ceil(pw * pixel_bits / 8) bytes, unfiltered
on its own with zeros above its first row and the whole image's bpp; the padding bits at the end of a sub-byte row are not
samples.  The stream must inflate to exactly the passes' bytes.  UNSUPPORTED: that sum is 2^31 or more, or a dimension is
65 536 or more.  The header of an interlaced file is ref_png_in.parse's of the same file with interlace 0 in its IHDR (and
the CRC made right): every other rule of the chunk walk holds as it stands.  A file that is not interlaced is
ref_png_in's, with a table of one pass."""
import struct
import zlib

import numpy as np

import ref_png_in
from ref_png_in import INVALID, LUMA8, OK, RGB8, UNSUPPORTED, PngError  # noqa: F401

X0, Y0 = (0, 4, 0, 2, 0, 1, 0), (0, 0, 4, 0, 2, 0, 1)
DX, DY = (8, 8, 4, 4, 2, 2, 1), (8, 8, 8, 4, 4, 2, 2)


def _chunk(typ, body=b""):
    return struct.pack(">I", len(body)) + typ + body + struct.pack(">I", zlib.crc32(typ + body))


def pass_table(w, h, pixel_bits, interlace=1):
    """Per pass: width, height, row_bytes, first_row (among all passes' rows), offset (in the filtered image), x0, y0,
    log_dx, log_dy - an empty pass has width = height = row_bytes = 0 - and the filtered image's size."""
    table, first_row, offset = [], 0, 0
    for p in range(7 if interlace else 1):
        x0, y0, dx, dy = (X0[p], Y0[p], DX[p], DY[p]) if interlace else (0, 0, 1, 1)
        pw = -(-(w - x0) // dx) if w > x0 else 0
        ph = -(-(h - y0) // dy) if h > y0 else 0
        if pw == 0 or ph == 0:
            pw = ph = 0
        row_bytes = (pw * pixel_bits + 7) // 8
        table.append({"width": pw, "height": ph, "row_bytes": row_bytes, "first_row": first_row, "offset": offset, "x0": x0, "y0": y0,
                      "log_dx": dx.bit_length() - 1, "log_dy": dy.bit_length() - 1})
        if ph:
            first_row, offset = first_row + ph, offset + ph * (1 + row_bytes)
    return table, offset


def _interlaced(data) -> bool:
    """A 13-byte IHDR comes first, its CRC is right and its interlace byte is 1 (anything else is ref_png_in.parse's to judge)."""
    return (len(data) >= 33 and data[:8] == ref_png_in.SIGNATURE and data[8:16] == b"\0\0\0\x0dIHDR" and data[28] == 1
            and zlib.crc32(data[12:29]) == struct.unpack_from(">I", data, 29)[0])


def parse(data: bytes) -> dict:
    """ref_png_in.parse's header with interlace 0 or 1, and passes, the count of the non-empty ones, pass_rows and filtered."""
    data = bytes(data)
    lace = _interlaced(data)
    if lace:
        plain = _chunk(b"IHDR", data[16:28] + b"\0")
        # IHDR's own refusals first, in their order (a file of this IHDR and nothing that could be wrong behind it)
        ref_png_in.parse(ref_png_in.SIGNATURE + plain + _chunk(b"PLTE", b"\0\0\0") + _chunk(b"IDAT") + _chunk(b"IEND"))
        w, hh, depth, colour = struct.unpack_from(">IIBB", data, 16)
        if pass_table(w, hh, ref_png_in.CHANNELS[colour] * depth)[1] >= 1 << 31:
            raise PngError(UNSUPPORTED, "passes of 2^31 bytes or more")
        data = data[:8] + plain + data[33:]
    h = ref_png_in.parse(data)
    table, filtered = pass_table(h["width"], h["height"], h["channels"] * h["depth"], lace)
    h.update(interlace=int(lace), pass_table=table, passes=sum(1 for e in table if e["height"]), pass_rows=sum(e["height"] for e in table),
             filtered=filtered)
    return h


def info(data: bytes) -> tuple:
    """cvhip_png_ext_info's out_info[8]."""
    h = parse(data)
    return (h["width"], h["height"], h["colour"], h["depth"], h["interlace"], len(h["idat"]), h["focal_length_35mm"], h["flags"])


def pass_rows(filtered: bytes, h: dict, fast=False):
    """Per non-empty pass: (its table entry, its unfiltered rows [height, row_bytes])."""
    unfilter = ref_png_in.unfilter_fast if fast else ref_png_in.unfilter
    out = []
    for e in h["pass_table"]:
        if e["height"]:
            part = filtered[e["offset"]:e["offset"] + e["height"] * (1 + e["row_bytes"])]
            out.append((e, unfilter(part, e["height"], e["row_bytes"], h["bpp"])))
    return out


def filter_types(filtered: bytes, h: dict):
    """Per pass (the empty ones too) the filter type of each of its rows."""
    return [[filtered[e["offset"] + y * (1 + e["row_bytes"])] for y in range(e["height"])] for e in h["pass_table"]]


def row_segments(filtered: bytes, h: dict) -> int:
    """The row segments of the unfilter pass: a pass's first row starts one, and every None or Sub row."""
    return sum(sum(1 for y, t in enumerate(types) if y == 0 or t < 2) for types in filter_types(filtered, h))


def decode(data: bytes, inflater=None, fast=False) -> dict:
    """-> luma, rgb, samples, header, stats, filtered, as ref_png_in.decode."""
    data = bytes(data)
    h = parse(data)
    for o, n, crc in h["idat"]:
        if zlib.crc32(b"IDAT" + data[o:o + n]) != crc:
            raise PngError(INVALID, "a chunk's CRC")
    stream = ref_png_in.stream_of(data, h)
    filtered, stats = ref_png_in.inflate(stream) if inflater is None else (inflater(stream), None)
    if len(filtered) != h["filtered"]:
        raise PngError(INVALID, "output that is not the passes' bytes")
    samples = np.zeros((h["height"], h["width"], h["channels"]), dtype=np.int64)
    for e, rows in pass_rows(filtered, h, fast):
        sub = ref_png_in.samples_of(rows, {"width": e["width"], "depth": h["depth"], "channels": h["channels"]})
        samples[e["y0"]::1 << e["log_dy"], e["x0"]::1 << e["log_dx"]] = sub
    return {**ref_png_in.convert(samples, h), "samples": samples, "header": h, "stats": stats, "filtered": filtered,
            "row_segments": row_segments(filtered, h)}
