"""The Adam7 PNG files of the interlaced decoder's tests, all made at test time: an Adam7 writer built from
png_in_scenes' pack, apply_filters, ihdr(lace=1) and idats - Pillow reads such files and cannot write them - with a chosen
filter cycle per pass, and the smallest files that reach each case.  SPECS[name]() -> (samples, depth, colour, keywords of
adam7_png); scene(name) -> the file's bytes; plain(name) -> the same samples as a file that is not interlaced;
restated(name) -> ref_png_adam7's decode of it (computed once); refused() -> name: (bytes, code).  The unfilter kernel
works on tiles of 384 bytes of a row and batches of 64 rows of a segment (png_in_scenes.TILE_BYTES, BATCH_ROWS)."""
import functools
import zlib

import numpy as np

import png_in_scenes as base
import ref_png_adam7
import ref_png_in
from ref_png_adam7 import DX, DY, X0, Y0

INVALID, UNSUPPORTED = ref_png_in.INVALID, ref_png_in.UNSUPPORTED
CYCLE = (0, 1, 2, 3, 4)


# ---- the writer -----------------------------------------------------------------------------------------------------------------
def adam7_filtered(samples, depth, filters=(0,), pad_ones=False):
    """[h, w, ch] samples -> the filtered bytes of the seven passes, one behind the other.  filters: a cycle of filter types,
    counted from each pass's first row, or a function pass -> cycle.  pad_ones: the padding bits of a sub-byte row are ones."""
    ch = samples.shape[2]
    out = b""
    for p in range(7):
        sub = samples[Y0[p]::DY[p], X0[p]::DX[p]]
        if sub.shape[0] == 0 or sub.shape[1] == 0:
            continue   # no bytes at all
        rows = base.pack(sub, depth)
        spare = rows.shape[1] * 8 - sub.shape[1] * ch * depth
        if pad_ones and spare:
            rows[:, -1] |= (1 << spare) - 1
        out += base.apply_filters(rows, filters(p) if callable(filters) else filters, max(1, ch * depth // 8))
    return out


def adam7_file(w, h, depth, colour, stream, cuts=(), before=()):
    return ref_png_in.SIGNATURE + base.ihdr(w, h, depth, colour, lace=1) + b"".join(before) + base.idats(stream, cuts) + base.chunk(b"IEND")


def adam7_png(samples, depth, colour, filters=(0,), before=(), cuts=(), compress=None, pad_ones=False):
    h, w, _ = samples.shape
    filtered = adam7_filtered(samples, depth, filters, pad_ones)
    stream = (compress or zlib.compress)(filtered)
    return adam7_file(w, h, depth, colour, stream, cuts(filtered, stream) if callable(cuts) else cuts, before)


def rotated(start):
    return tuple(CYCLE[(start + k) % 5] for k in range(5))


# ---- the valid scenes -----------------------------------------------------------------------------------------------------------
SPECS = {}


def _typed(colour, depth, w, h, tag, entries=None, **kw):
    """Random samples of a colour type; colour type 3: a PLTE of `entries` colours (default: all 2^depth) and indices below."""
    ch = ref_png_in.CHANNELS[colour]
    top = 1 << depth
    if colour == 3:
        entries = entries or top
        top = entries
        kw["before"] = (base.chunk(b"PLTE", base.rng(tag + "p").integers(0, 256, 3 * entries).astype(np.uint8).tobytes()), *kw.get("before", ()))
    return base.rng(tag).integers(0, top, (h, w, ch)), depth, colour, kw


# the size sweep: every pattern of missing passes (1 x 1: pass 0 alone; w <= 4: no pass 1; h = 1: no passes 2, 4, 6).  The filter
# cycle starts elsewhere in every pass and file, so that Up, Average and Paeth each stand on some first row of every pass.
SWEEP = [(w, h) for w in range(1, 10) for h in range(1, 10)]
for _w, _h in SWEEP:
    SPECS["z_%dx%d" % (_w, _h)] = functools.partial(_typed, 2, 8, _w, _h, "z%d%d" % (_w, _h),
                                                    filters=functools.partial(lambda w, h, p: rotated(w + 2 * h + p), _w, _h))
# sub-byte rows: every pass width around a byte's end and a row's, padding bits that are ones, a PLTE shorter than 2^depth
SUB_BYTE = [(kind, d, w, h) for kind in ("grey", "pal") for d in (1, 2, 4) for w in (1, 2, 7, 8, 9, 15, 16, 17, 63, 64, 65) for h in (1, 2, 9)]
for _kind, _d, _w, _h in SUB_BYTE:
    _name = "k_%s_d%d_%dx%d" % (_kind, _d, _w, _h)
    if _kind == "grey":
        SPECS[_name] = functools.partial(_typed, 0, _d, _w, _h, _name, filters=(4, 3, 2, 1, 0))
    else:
        SPECS[_name] = functools.partial(_typed, 3, _d, _w, _h, _name, entries=(1 << _d) - 1, filters=(2, 4, 1, 3), pad_ones=True)
# every colour type and depth
TYPES = [(c, d, w, h) for c, depths in ref_png_in.LEGAL.items() for d in depths for w, h in ((17, 9), (65, 5))]
for _c, _d, _w, _h in TYPES:
    SPECS["s_c%d_d%d_%dx%d" % (_c, _d, _w, _h)] = functools.partial(_typed, _c, _d, _w, _h, "s%d%d%d" % (_c, _d, _w), filters=(3, 4, 0, 2, 1))
# the batch seam: a pass of more than 64 rows under Paeth is one segment of two batches (pass 6 of 131 rows has 65, pass 0 of 521 has 66)
SPECS["b_9x131_grey8"] = functools.partial(_typed, 0, 8, 9, 131, "b131", filters=(4,))
SPECS["b_9x521_rgba16"] = functools.partial(_typed, 6, 16, 9, 521, "b521", filters=(4,))
# the tile seam: pass rows above 384 bytes (521 RGBA16 pixels: pass 0 has 528 bytes, pass 6 has 4168; 131 RGB pixels: 393 and 786 in pass 6)
SPECS["t_521x9_rgba16"] = functools.partial(_typed, 6, 16, 521, 9, "t521", filters=(3, 4))
SPECS["t_131x9_rgb8"] = functools.partial(_typed, 2, 8, 131, 9, "t131a", filters=(4, 3, 2))
SPECS["t_131x9_rgb16"] = functools.partial(_typed, 2, 16, 131, 9, "t131b", filters=(4, 3, 2))
# a different cycle in each pass
MIXED = ((4, 4, 1, 2), (3,), (0, 4, 2), (2, 2, 2, 1), (4, 3, 2, 1, 0), (1, 4), (3, 0, 4, 4, 2, 2, 1))
SPECS["m_40x40"] = functools.partial(_typed, 4, 8, 40, 40, "m40", filters=lambda p: MIXED[p])


def _smooth(w, h, ch, tag, **kw):
    return base.smooth(h, w, ch, tag), 8, {1: 0, 3: 2}[ch], kw


def _pass_cuts(filtered, stream):
    """IDAT cuts of a stream that is one stored block (two bytes of zlib header, five of the block's): at every pass's first
    byte and right behind it, so a filter byte ends a chunk, begins one, and stands alone in one."""
    assert len(filtered) < 65536 and len(stream) == len(filtered) + 11
    edges, at = [], 0
    for p in range(7):
        sub_h, sub_w = len(range(Y0[p], 23, DY[p])), len(range(X0[p], 29, DX[p]))
        edges += [7 + at, 7 + at + 1]
        at += sub_h * (1 + 3 * sub_w)
    assert at == len(filtered)
    return edges


# the stream: IDAT chunks cut at the pass boundaries, many small blocks, stored blocks
SPECS["i_pass_cuts"] = functools.partial(_smooth, 29, 23, 3, "cuts", filters=CYCLE, compress=base.compressor(level=0), cuts=_pass_cuts)
SPECS["i_mem1"] = lambda: (base._noise_rgb(40, 48, "a7mem"), 8, 2, dict(filters=(1, 4, 2), compress=base.compressor(level=6, memLevel=1)))
SPECS["i_stored"] = lambda: (base._noise_rgb(40, 48, "a7st"), 8, 2, dict(filters=(4,), compress=base.compressor(level=0)))
# the options' file, and image.load's (an eXIf focal length)
SPECS["o_13x21"] = functools.partial(_smooth, 13, 21, 3, "opt", filters=(4, 3, 2, 1, 0))
FOCAL = 41
SPECS["x_exif"] = functools.partial(_smooth, 11, 7, 3, "exif", filters=(1, 4), before=(base.chunk(b"eXIf", base.exif_block(FOCAL, True, ">")),))


def names():
    return sorted(SPECS)


@functools.lru_cache(maxsize=None)
def spec(name):
    return SPECS[name]()


@functools.lru_cache(maxsize=None)
def scene(name) -> bytes:
    samples, depth, colour, kw = spec(name)
    return adam7_png(samples, depth, colour, **kw)


@functools.lru_cache(maxsize=None)
def plain(name) -> bytes:
    """The scene's samples as a file that is not interlaced."""
    samples, depth, colour, kw = spec(name)
    return base.image_png(samples, depth, colour, CYCLE, kw.get("before", ()))


@functools.lru_cache(maxsize=None)
def restated(name) -> dict:
    return ref_png_adam7.decode(scene(name), fast=True)


# ---- the refused files ------------------------------------------------------------------------------------------------------------
def _good_samples():
    return base.smooth(6, 7, 3, "good")


def _patched(filtered, at, value):
    out = bytearray(filtered)
    out[at] = value
    return bytes(out)


@functools.lru_cache(maxsize=None)
def refused() -> dict:
    """name: (bytes, code).  The header decides the UNSUPPORTED ones and the headers taken from png_in_scenes.refused()."""
    U, I = UNSUPPORTED, INVALID
    out = {}
    samples = _good_samples()
    good = adam7_png(samples, 8, 2, CYCLE)
    filtered = adam7_filtered(samples, 8, CYCLE)
    table, total = ref_png_adam7.pass_table(7, 6, 24)
    assert total == len(filtered)
    # an Adam7 header over a stream that is not interlaced (png_in_scenes' u_adam7), and the other way round
    out["i_plain_stream"] = (base.refused()["u_adam7"][0], I)
    out["i_adam7_stream"] = (base.png(7, 6, 8, 2, zlib.compress(filtered)), I)
    last = max(p for p in range(7) if table[p]["height"])
    out["i_pass_short"] = (adam7_file(7, 6, 8, 2, zlib.compress(filtered[:table[last]["offset"]])), I)
    out["i_one_byte"] = (adam7_file(7, 6, 8, 2, b"\x78"), I)
    out["i_filter_5_pass3_first"] = (adam7_file(7, 6, 8, 2, zlib.compress(_patched(filtered, table[3]["offset"], 5))), I)
    e = table[6]
    out["i_filter_5_pass6_last"] = (adam7_file(7, 6, 8, 2, zlib.compress(_patched(filtered, e["offset"] + (e["height"] - 1) * (1 + e["row_bytes"]), 5))), I)
    # 5 x 1 at two bits: pass 1 is the one pixel (4, 0), the only index beyond a PLTE of three colours
    indices = np.array([[[0], [1], [2], [1], [3]]])
    plte = (base.chunk(b"PLTE", bytes(range(9))),)
    assert ref_png_adam7.pass_table(5, 1, 2)[0][1]["width"] == 1
    out["i_index_beyond_pass1"] = (adam7_png(indices, 2, 3, (0,), plte), I)
    # headers of png_in_scenes.refused() with interlace 1
    for name in ("i_zero_width", "i_pair", "i_compression", "i_crc_ihdr", "i_no_idat", "i_critical", "i_no_iend", "i_crc_idat", "i_adler"):
        data, code = base.refused()[name]
        assert data[28] == 0
        laced = bytearray(data)
        laced[28] = 1
        if name != "i_crc_ihdr":
            laced[29:33] = zlib.crc32(bytes(laced[12:29])).to_bytes(4, "big")
        out[name + "_laced"] = (bytes(laced), code)
    out["i_interlace_2"] = (base.refused()["i_interlace_2"][0], I)
    out["u_wide"] = (base._reihdr(good, w=65536), U)
    out["u_tall"] = (base._reihdr(good, h=65536), U)
    # 8-bit grey, 32767 x 65535: 2 147 450 880 bytes when not interlaced, below 2^31; the passes' filter bytes take it above
    assert 65535 * 32768 < 1 << 31 <= ref_png_adam7.pass_table(32767, 65535, 8)[1]
    out["u_passes_2g"] = (base._reihdr(good, w=32767, h=65535, colour=0, depth=8), U)
    return out
