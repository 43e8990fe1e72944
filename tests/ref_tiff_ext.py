"""The definition of cvhip_tiff_ext_info / cvhip_tiff_ext_decode in numpy: ref_tiff's walk of the first IFD
extended by Deflate (compression 8 and 32946) and by tiles (tags 322 to 325), check for check in the order of
tiff_common::parse(.., extended = true); the streams' decompression - ref_tiff's unlzw and unpackbits, ref_png_in's inflate
for the zlib streams -, the tile gather, Predictor 2 per tile, and ref_tiff's conversion to Luma8 / RGB8.

A file is a table of streams: strips of rows_per_strip rows of the image's width, or tiles - strips of TileLength rows of
TileWidth pixels, the edge tiles whole, their padding decoded and dropped.  The defined rules: a zlib stream inflates to
exactly the bytes of its strip or tile (fewer or more is INVALID: the Adler-32 is always checked, so the stream ends where
the rows do; libtiff stops when the rows are full and reads a longer stream); a distance reaches no further back than its own
stream's first byte; streams x rows x row bytes of 2^31 or more with Deflate is UNSUPPORTED, and so are Deflate streams whose
byte counts add up to more than the file (streams that share bytes)."""
import numpy as np

import ref_png_in
import ref_tiff
from ref_tiff import INVALID, UNSUPPORTED, LUMA8, RGB8, DROP_DATABAR, TiffError, SCALARS, ARRAYS, TYPE_SIZE

TILE_SCALARS, TILE_ARRAYS = (322, 323), (324, 325)
DEFLATE = (8, 32946)


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
    entries = ref_tiff._ifd_entries(data, order, int.from_bytes(data[4:8], order))
    if entries is None:
        raise TiffError(INVALID, "truncated IFD")
    tags, sem = {}, {}
    scalars, known = SCALARS + TILE_SCALARS, SCALARS + ARRAYS + TILE_SCALARS + TILE_ARRAYS
    for tag, kind, count, at in entries:
        if tag in (34682, 34683) and tag not in sem:
            sem[tag] = (kind, count, at)
        if tag not in known or tag in tags:
            continue
        if kind not in (3, 4) or count == 0 or (tag in scalars and count != 1):
            raise TiffError(INVALID, f"tag {tag}: type or count")
        where = ref_tiff._value_at(data, order, kind, count, at)
        if where is None:
            raise TiffError(INVALID, f"tag {tag} reaches past the file")
        size = TYPE_SIZE[kind]
        tags[tag] = [int.from_bytes(data[where + size * k:where + size * (k + 1)], order) for k in range(count)]
    tiles = any(tag in tags for tag in TILE_SCALARS + TILE_ARRAYS)
    if tiles and (273 in tags or 279 in tags):
        raise TiffError(INVALID, "strip tags and tile tags")
    for tag in (256, 257, 262) + ((322, 323, 324) if tiles else (273,)):
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
    if compression not in (1, 5, 32773) + DEFLATE:
        raise TiffError(UNSUPPORTED, "compression")
    predictor = tags.get(317, [1])[0]
    if predictor == 3:
        raise TiffError(UNSUPPORTED, "Predictor 3")
    if predictor not in (1, 2):
        raise TiffError(INVALID, "Predictor")
    photometric = tags[262][0]
    if not ((spp == 1 and photometric in (0, 1)) or (spp in (3, 4) and photometric == 2)):
        raise TiffError(UNSUPPORTED, "photometric interpretation and samples")
    row_bytes = width * spp * (bps // 8)
    tile_w = tile_l = across = down = 0
    if tiles:
        tile_w, tile_l = tags[322][0], tags[323][0]
        if tile_w == 0 or tile_l == 0 or tile_w % 16 or tile_l % 16:
            raise TiffError(UNSUPPORTED, "a tile width or length that is no multiple of 16")
        across, down = -(-width // tile_w), -(-height // tile_l)
        rps, nstreams, stream_row_bytes = tile_l, across * down, tile_w * spp * (bps // 8)
        offsets, counts = tags[324], tags.get(325)
    else:
        rps = tags.get(278, [0xFFFFFFFF])[0]
        if rps == 0:
            raise TiffError(INVALID, "RowsPerStrip 0")
        rps = min(rps, height)
        nstreams, stream_row_bytes = -(-height // rps), row_bytes
        offsets, counts = tags[273], tags.get(279)
    if stream_row_bytes >= 2 ** 31 or rps >= 2 ** 31 or rps * stream_row_bytes >= 2 ** 31:
        raise TiffError(UNSUPPORTED, "a strip or tile of 2^31 bytes or more")
    if len(offsets) != nstreams:
        raise TiffError(INVALID, "offsets count")
    rows = [rps if tiles else min(rps, height - s * rps) for s in range(nstreams)]
    if counts is None:
        if compression != 1:
            raise TiffError(INVALID, "byte counts are missing")
        counts = [r * stream_row_bytes for r in rows]
    if len(counts) != nstreams:
        raise TiffError(INVALID, "byte counts count")
    for s in range(nstreams):
        if counts[s] >= 2 ** 31:
            raise TiffError(UNSUPPORTED, "a strip or tile of 2^31 bytes or more")
        if offsets[s] + counts[s] > n:
            raise TiffError(INVALID, "a strip or tile reaches past the file")
        if compression == 1 and counts[s] < rows[s] * stream_row_bytes:
            raise TiffError(INVALID, "a strip or tile shorter than its rows")
        if compression == 5 and counts[s] >= 2 and data[offsets[s]] == 0 and (data[offsets[s] + 1] & 1):
            raise TiffError(UNSUPPORTED, "old-style LZW")
    if compression in DEFLATE and sum(counts) > n:
        raise TiffError(UNSUPPORTED, "Deflate: streams that overlap")
    if compression in DEFLATE and nstreams * rps * stream_row_bytes >= 2 ** 31:
        raise TiffError(UNSUPPORTED, "Deflate: 2^31 decompressed bytes or more")
    found, tilt, databar, sw, sh = False, None, 0, np.float32(1.0), np.float32(1.0)
    block = sem.get(34683, sem.get(34682))
    if block is not None and block[0] == 2:
        where = ref_tiff._value_at(data, order, 2, block[1], block[2])
        if where is not None:
            found = True
            sw, sh, tilt, databar = ref_tiff.sem_bytes(data[where:where + block[1]])
    # the position of every stream's top-left sample
    xs = [s % across * tile_w if tiles else 0 for s in range(nstreams)]
    ys = [s // across * tile_l if tiles else s * rps for s in range(nstreams)]
    return {"width": width, "height": height, "samples": spp, "bits": bps, "compression": compression, "photometric": photometric,
            "predictor": predictor, "strips": nstreams, "rows_per_strip": rps, "focal_length_35mm": ref_tiff._exif_focal(data, order, entries),
            "databar_height": databar, "sem": found, "tilt_angle": tilt, "scale": (sw, sh), "order": order, "offsets": offsets,
            "counts": counts, "rows": rows, "row_bytes": row_bytes, "stream_row_bytes": stream_row_bytes, "xs": xs, "ys": ys,
            "tile_width": tile_w, "tile_length": tile_l, "tiles_across": across, "tiles_down": down}


SUBSEQ_BITS, WINDOW = 1024, 256   # png_decode_common.hpp: a settle window is 256 subsequences of 1024 bits; PIECE x 256 bytes of a stored block


def _token_bits(src: bytes, first_bit: int, btype: int):
    """(the first token's bit, the end-of-block code's length) of the fixed or dynamic block whose header begins at first_bit."""
    if btype == 1:
        return first_bit + 3, 7
    b = ref_png_in._Bits(src)
    b.p = first_bit + 3
    hlit, hdist, hclen = b.take(5) + 257, b.take(5) + 1, b.take(4) + 4
    cl = [0] * 19
    for i in range(hclen):
        cl[ref_png_in.CL_ORDER[i]] = b.take(3)
    table, _ = ref_png_in.build_code(cl)
    lengths = []
    while len(lengths) < hlit + hdist:
        sym, _n = b.symbol(table)
        if sym < 16:
            lengths.append(sym)
        elif sym == 16:
            lengths += [lengths[-1]] * (3 + b.take(2))
        else:
            lengths += [0] * (3 + b.take(3) if sym == 17 else 11 + b.take(7))
    return b.p, lengths[256]


def chain_counts(src: bytes, blocks) -> tuple:
    """(subsequences, settle windows) of one accepted stream, from inflate's block table: a block's windows of 256 subsequences
    of 1024 bits begin at its first token; a token belongs to the subsequence it begins in; the one the end-of-block begins in
    is the block's last.  A stored block has no subsequences and a window per 256 x 1024 bytes."""
    subsequences = windows = 0
    for btype, first_bit, bits, produced, _longest in blocks:
        if btype == 0:
            windows += -(-produced // (WINDOW * 1024))
            continue
        first, eob = _token_bits(src, first_bit, btype)
        span = first_bit + bits - eob - first   # from the first token's bit to the end-of-block's
        windows += span // (WINDOW * SUBSEQ_BITS) + 1
        subsequences += span // SUBSEQ_BITS + 1
    return subsequences, windows


def stream_bytes(data: bytes, h: dict, s: int, stats=None) -> bytes:
    """Stream s decompressed: rows[s] x stream_row_bytes bytes."""
    src, need = data[h["offsets"][s]:h["offsets"][s] + h["counts"][s]], h["rows"][s] * h["stream_row_bytes"]
    if h["compression"] == 1:
        return src[:need]
    if h["compression"] == 5:
        return ref_tiff.unlzw(src, need, stats)
    if h["compression"] == 32773:
        return ref_tiff.unpackbits(src, need)
    try:
        out, st = ref_png_in.inflate(src, want=need)
    except ref_png_in.PngError as e:
        raise TiffError(INVALID, f"Deflate: {e}") from None
    if stats is not None:
        stats.setdefault("inflate", []).append(st)
        for k in ("stored", "fixed", "dynamic"):
            stats[k] = stats.get(k, 0) + st[k]
        for k, v in zip(("subsequences", "windows"), chain_counts(src, st["blocks"])):
            stats[k] = stats.get(k, 0) + v
    return out


def samples(data: bytes, stats=None):
    """(header, [height, width, samples] uint8 or uint16: the file's samples, Predictor 2 undone from every stream's left edge)."""
    data = bytes(data)
    h = parse(data)
    spp = h["samples"]
    dtype = np.uint8 if h["bits"] == 8 else np.dtype("<u2" if h["order"] == "little" else ">u2")
    plain = np.uint8 if h["bits"] == 8 else np.uint16
    wide = h["stream_row_bytes"] // (spp * h["bits"] // 8)   # a stream's pixels per row
    across = h["tiles_across"] or 1
    full = np.zeros((-(-h["strips"] // across) * h["rows_per_strip"], across * wide, spp), dtype=plain)   # (tiles padded)
    for s in range(h["strips"]):
        a = np.frombuffer(stream_bytes(data, h, s, stats), dtype=dtype).reshape(h["rows"][s], wide, spp).astype(plain)
        if h["predictor"] == 2:
            a = np.cumsum(a.astype(np.uint32), axis=1).astype(plain)   # (the wrap of the cast is the sum modulo 2^8 or 2^16)
        full[h["ys"][s]:h["ys"][s] + h["rows"][s], h["xs"][s]:h["xs"][s] + wide] = a
    if stats is not None:
        stats["streams"] = h["strips"]
    return h, np.ascontiguousarray(full[:h["height"], :h["width"]])


def decode(data: bytes, fmt: int = LUMA8, drop_rows: int = 0, stats=None) -> np.ndarray:
    if fmt not in (LUMA8, RGB8):
        raise TiffError(INVALID, "format")
    h = parse(data)
    if drop_rows == DROP_DATABAR:
        drop_rows = h["databar_height"]
    if drop_rows >= h["height"]:
        raise TiffError(INVALID, "drop_rows leaves no row")
    h, a = samples(data, stats)
    return np.ascontiguousarray(ref_tiff.convert(h, a, fmt)[:h["height"] - drop_rows])


def info(data: bytes) -> dict:
    h = parse(data)
    return {k: h[k] for k in ("width", "height", "samples", "bits", "compression", "photometric", "predictor", "strips", "rows_per_strip",
                              "databar_height", "sem", "tilt_angle", "scale", "tile_width", "tile_length", "tiles_across")} | {
                                  "focal_length_35mm": h["focal_length_35mm"] or None}
