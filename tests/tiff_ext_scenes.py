"""Deflate and tiled TIFF files for the tests of cvhip_tiff_ext_decode, built at run time with zlib and
tiff_scenes' writer: scene(name) -> the file's bytes, source(name) -> the picture it was written from, refused() -> the files
that are refused, with the code.  write_tiles is the tile writer: edge tiles whole, their padding filled with a value the
picture never needs, Predictor 2 from every tile's left edge."""
import functools
import struct
import zlib

import numpy as np

import tiff_scenes
from tiff_scenes import ASCII, LONG, SHORT, INVALID, UNSUPPORTED, SEM_TEXT, assemble, picture, write

ENCODERS = {1: lambda b: b, 5: tiff_scenes.lzw, 32773: tiff_scenes.packbits, 8: lambda b: zlib.compress(b, 6), 32946: lambda b: zlib.compress(b, 6)}
COMPRESSIONS = tuple(ENCODERS)


def deflate(level=6, strategy=zlib.Z_DEFAULT_STRATEGY, mem_level=8):
    def encode(raw):
        c = zlib.compressobj(level, zlib.DEFLATED, 15, mem_level, strategy)
        return c.compress(raw) + c.flush()
    return encode


def mixed_blocks(raw: bytes) -> bytes:
    """One zlib stream of fixed, dynamic and stored blocks: four raw deflate pieces end to end, each but the last ended by a
    sync flush (an empty stored block, which leaves it at a byte's end and not final), each with what lies before it as its
    dictionary, so its copies reach back across the block ends."""
    quarter, out = len(raw) // 4, b"\x78\x9c"
    for k, (level, strategy) in enumerate(((6, zlib.Z_FIXED), (9, zlib.Z_DEFAULT_STRATEGY), (0, zlib.Z_DEFAULT_STRATEGY), (9, zlib.Z_DEFAULT_STRATEGY))):
        part, seen = raw[k * quarter:(k + 1) * quarter if k < 3 else len(raw)], raw[:k * quarter][-32768:]
        c = zlib.compressobj(level, zlib.DEFLATED, -15, 9, strategy, seen) if seen else zlib.compressobj(level, zlib.DEFLATED, -15, 9, strategy)
        out += c.compress(part) + c.flush(zlib.Z_FINISH if k == 3 else zlib.Z_SYNC_FLUSH)
    return out + struct.pack(">I", zlib.adler32(raw))


def write_tiles(a, tw, tl, order="<", compression=1, predictor=1, encoder=None, photometric=None, tile_order=None, extra=(), override=None,
                data_at=8, exif_focal=None, pad=0xAB):
    """a: [h, w, spp] uint8 / uint16 in tiles of tw x tl pixels."""
    h, w, spp = a.shape
    bits = 8 * a.dtype.itemsize
    across, down = -(-w // tw), -(-h // tl)
    full = np.full((down * tl, across * tw, spp), pad if bits == 8 else pad * 257, dtype=a.dtype)
    full[:h, :w] = a
    encoder = encoder or ENCODERS[compression]
    tiles = []
    for t in range(across * down):
        tile = full[t // across * tl:(t // across + 1) * tl, t % across * tw:(t % across + 1) * tw]
        stored = tile.copy()
        if predictor == 2:
            stored[:, 1:] = tile[:, 1:] - tile[:, :-1]
        tiles.append(encoder(stored.astype(stored.dtype.newbyteorder(order)).tobytes()))
    body, offsets = bytearray(b"\0" * (data_at - 8)), [0] * len(tiles)
    for t in (tile_order if tile_order is not None else range(len(tiles))):
        offsets[t] = 8 + len(body)
        body += tiles[t]
    entries = {256: (SHORT, [w]), 257: (SHORT, [h]), 258: (SHORT, [bits] * spp), 259: (SHORT, [compression]),
               262: (SHORT, [(1 if spp == 1 else 2) if photometric is None else photometric]), 277: (SHORT, [spp]),
               322: (SHORT, [tw]), 323: (SHORT, [tl]), 324: (LONG, offsets), 325: (LONG, [len(t) for t in tiles])}
    if predictor != 1:
        entries[317] = (SHORT, [predictor])
    if spp == 4:
        entries[338] = (SHORT, [2])
    for tag, typ, values in extra:
        entries[tag] = (typ, values)
    for tag, value in (override or {}).items():
        if value is None:
            entries.pop(tag, None)
        else:
            entries[tag] = value
    return assemble(order, entries, bytes(body), 42, exif_focal, True)


def high_noise(h, w, seed):
    """Noise of the values 144 .. 255: nine bits each in a fixed block, which zlib ends after 32 767 symbols (memLevel 9) - 294 903
    bits, more than a settle window's 256 x 1024."""
    return np.random.default_rng(seed).integers(144, 256, size=(h, w, 1)).astype(np.uint8)


def repeating(h, w, seed):
    """Eight rows of noise, repeated: copies at a distance of eight rows."""
    return np.tile(picture(8, w, seed=seed, kind="noise"), (h // 8, 1, 1))


def four_quarters(h, w, seed):
    """The picture of "s_mixed", a quarter per piece of mixed_blocks: repeated noise (a fixed block with copies), six-bit noise (a
    dynamic block), noise (stored), and the first quarter again (a dynamic block of copies that reach back over all of them)."""
    top = repeating(h // 4, w, seed)
    return np.concatenate([top, picture(h // 4, w, seed=seed + 1, kind="noise") & 0xFC, picture(h // 4, w, seed=seed + 2, kind="noise"), top])


def _flat_with_edge(h, w):
    a = picture(h, w, kind="flat")
    a[0, 0] = 3
    return a


SEM = [(34682, ASCII, SEM_TEXT.encode() + b"\0")]


def _pictures():
    P = picture
    return {
        # ---- Deflate strips
        "s_1x1": (P(1, 1, seed=3), dict(compression=8)),
        "s_stored": (P(47, 33, seed=2), dict(compression=8, encoder=deflate(0))),
        "s_fixed": (P(47, 33, seed=2), dict(compression=8, encoder=deflate(6, zlib.Z_FIXED))),
        "s_dynamic": (picture(47, 33, seed=35, kind="noise") & 0xF0, dict(compression=8, encoder=deflate(9))),
        "s_mixed": (four_quarters(64, 96, 31), dict(compression=8, encoder=mixed_blocks)),
        "s_flat": (_flat_with_edge(64, 64), dict(compression=8)),
        "s_70_strips": (P(70, 5, seed=5), dict(compression=8, rps=1)),
        "s_out_of_order": (P(47, 33, seed=2), dict(compression=8, rps=7, strip_order=[3, 0, 6, 1, 5, 2, 4], data_at=9)),
        "s_twins": (np.concatenate([P(8, 40, seed=32)] * 2), dict(compression=8, rps=8)),
        "s_window": (high_noise(96, 512, 33), dict(compression=8, encoder=deflate(6, zlib.Z_FIXED, 9))),
        "s_32946": (P(47, 33, seed=2), dict(compression=32946, rps=7)),
        "s_mm_g16_pred": (P(47, 33, 1, 16, seed=6), dict(order=">", compression=8, predictor=2, rps=7)),
        "s_ii_g16": (P(47, 33, 1, 16, seed=6), dict(order="<", compression=8, rps=7)),
        "s_wiz": (P(47, 33, seed=2), dict(compression=8, photometric=0, rps=7)),
        "s_rgb8_pred_rps7": (P(47, 33, 3, seed=8), dict(compression=8, predictor=2, rps=7)),
        "s_rgba16_mm": (P(13, 33, 4, 16, seed=9), dict(order=">", compression=8, rps=5)),
        "s_sem": (P(47, 33, seed=2), dict(compression=8, rps=7, extra=SEM, exif_focal=35)),
    }


def _tiled():
    P = picture
    t = {}
    for c in COMPRESSIONS:
        t[f"t_small_{c}"] = (P(3, 5, seed=40), dict(tw=16, tl=16, compression=c))                       # smaller than one tile
        t[f"t_ragged_{c}"] = (P(47, 33, seed=41), dict(tw=16, tl=16, compression=c))                    # ragged right and bottom
        t[f"t_exact_{c}"] = (P(32, 48, seed=42), dict(tw=48, tl=32, compression=c))                     # one tile, exactly the image
        t[f"t_wide_{c}"] = (P(20, 33, seed=43), dict(tw=64, tl=16, compression=c))                      # a tile wider than the image
    for name, spp, bits, order in (("g8", 1, 8, "<"), ("g16", 1, 16, ">"), ("rgb8", 3, 8, "<"), ("rgb16", 3, 16, "<")):
        for tw in (16, 256, 272):
            t[f"t_pred_{name}_{tw}"] = (P(5, 600, spp, bits, seed=44, kind="noise"), dict(tw=tw, tl=16, order=order, compression=8, predictor=2))
    t["t_pred_g8_272_raw"] = (P(5, 600, seed=44, kind="noise"), dict(tw=272, tl=16, compression=1, predictor=2))
    t["t_pred_rgb8_16_lzw"] = (P(5, 600, 3, seed=44, kind="noise"), dict(tw=16, tl=16, compression=5, predictor=2))
    t["t_rgb_16x32_32946_pred"] = (P(47, 33, 3, seed=45), dict(tw=16, tl=32, compression=32946, predictor=2))
    t["t_g16_mm_32x16_pred"] = (P(47, 33, 1, 16, seed=46), dict(tw=32, tl=16, order=">", compression=8, predictor=2))
    t["t_rgb_raw"] = (P(47, 33, 3, seed=47), dict(tw=16, tl=16, compression=1))
    t["t_rgba_out_of_order"] = (P(20, 40, 4, seed=48), dict(tw=16, tl=16, compression=8, tile_order=[5, 2, 4, 0, 3, 1], data_at=11))
    t["t_sem"] = (P(47, 33, seed=2), dict(tw=16, tl=16, compression=8, predictor=2, extra=SEM, exif_focal=35))
    return t


def names():
    return sorted(_pictures()) + sorted(_tiled())


def source(name):
    return (_pictures().get(name) or _tiled()[name])[0]


@functools.lru_cache(maxsize=None)
def scene(name) -> bytes:
    if name in _pictures():
        a, kw = _pictures()[name]
        kw = dict(kw)
        kw.setdefault("encoder", ENCODERS[kw["compression"]])
        order = kw.pop("order", "<")
        return write(a, order, **kw)
    a, kw = _tiled()[name]
    return write_tiles(a, **kw)


def _stream(*blocks, adler=None, header=b"\x78\x9c"):
    """A zlib stream of stored blocks (the last one final) around `adler` (default: the right one)."""
    out, data = bytearray(header), b"".join(blocks)
    for k, b in enumerate(blocks):
        out += bytes([1 if k == len(blocks) - 1 else 0]) + struct.pack("<HH", len(b), len(b) ^ 0xFFFF) + b
    return bytes(out) + struct.pack(">I", zlib.adler32(data) if adler is None else adler)


def _bits(*fields):
    """(value, bits) fields, first bit lowest -> bytes."""
    acc = n = 0
    for v, w in fields:
        acc |= v << n
        n += w
    return acc.to_bytes((n + 7) // 8, "little")


def _code(v, w):
    """A Huffman code of w bits: its first bit first."""
    return (int(format(v, f"0{w}b")[::-1], 2), w)


@functools.lru_cache(maxsize=None)
def refused():
    """{name: (file, code, the header decides it)}"""
    g = picture(6, 5, seed=20)
    raw = g.tobytes()   # 30 bytes
    out = {}

    def add(name, data, code, header):
        out[name] = (data, code, header)

    def one(stream):
        return write(g, compression=8, encoder=lambda b: stream)

    good = zlib.compress(raw, 6)
    add("i_short_output", one(_stream(raw[:29])), INVALID, False)
    add("i_long_output", one(_stream(raw + b"\7")), INVALID, False)
    # fixed block: literal 'A' (0x41 + 0x30, 8 bits), then length 3 (symbol 257: 0000001) at distance 2 (code 00001): before the first byte
    far = b"\x78\x9c" + _bits((1, 1), (1, 2), _code(0x30 + 65, 8), _code(1, 7), _code(1, 5), _code(0, 7)) + b"\0\0\0\0"
    add("i_copy_before_first_byte", write(picture(1, 4, seed=20), compression=8, encoder=lambda b: far), INVALID, False)
    # the second of two identical strips takes 29 of its 30 bytes from the first one's: a literal, then length 29 (symbol 271,
    # extra 2) at distance 30 (symbol 9, extra 5), which is not inside the stream
    twin = b"\x78\x9c" + _bits((1, 1), (1, 2), _code(0x30 + 7, 8), _code(15, 7), (2, 2), _code(9, 5), (5, 3), _code(0, 7)) + b"\0\0\0\0"
    add("i_copy_into_neighbour", write(np.concatenate([g, g]), compression=8, rps=6, encoder=lambda b, n=iter((good, twin)): next(n)), INVALID, False)
    add("i_adler", one(good[:-1] + bytes([good[-1] ^ 1])), INVALID, False)
    add("i_zlib_header", one(b"\x78\x9d" + good[2:]), INVALID, False)
    add("i_zlib_method", one(b"\x79\x9c" + good[2:]), INVALID, False)
    add("i_block_type_3", one(b"\x78\x9c" + _bits((1, 1), (3, 2)) + b"\0" * 8), INVALID, False)
    add("i_nlen", one(b"\x78\x9c" + b"\1\x1e\0\x1e\0" + raw + struct.pack(">I", zlib.adler32(raw))), INVALID, False)
    # a dynamic block whose code-length code is over-subscribed: HCLEN = 4, four lengths of 1
    add("i_code_lengths", one(b"\x78\x9c" + _bits((1, 1), (2, 2), (0, 5), (0, 5), (0, 4), (1, 3), (1, 3), (1, 3), (1, 3)) + b"\0" * 8), INVALID, False)
    # fixed block: literal/length symbol 286 (11000110, 8 bits) is not a symbol
    add("i_no_such_symbol", one(b"\x78\x9c" + _bits((1, 1), (1, 2), _code(0b11000110, 8), _code(0, 7)) + b"\0" * 8), INVALID, False)
    add("i_truncated_stream", one(good[:-6]), INVALID, False)
    add("i_tile_strip_tags", write(g, extra=[(322, SHORT, [16]), (323, SHORT, [16]), (324, LONG, [8]), (325, LONG, [30])]), INVALID, True)
    ok = dict(tw=16, tl=16)
    add("u_tile_width_24", write_tiles(g, 24, 16), UNSUPPORTED, True)
    add("u_tile_length_8", write_tiles(g, 16, 8), UNSUPPORTED, True)
    add("u_tile_width_0", write_tiles(g, 16, 16, override={322: (SHORT, [0])}), UNSUPPORTED, True)
    add("i_tile_offsets_count", write_tiles(g, **ok, override={324: (LONG, [8, 8])}), INVALID, True)
    add("i_tile_counts_count", write_tiles(g, **ok, override={325: (LONG, [256, 256])}), INVALID, True)
    add("i_tile_counts_missing", write_tiles(g, **ok, compression=8, override={325: None}), INVALID, True)
    add("i_tile_no_length", write_tiles(g, **ok, override={323: None}), INVALID, True)
    add("i_tile_no_offsets", write_tiles(g, **ok, override={324: None}), INVALID, True)
    add("i_tile_short", write_tiles(g, **ok, override={325: (LONG, [255])}), INVALID, True)
    add("i_tile_past_file", write_tiles(g, **ok, override={324: (LONG, [100000])}), INVALID, True)
    add("i_tile_width_type", write_tiles(g, **ok, override={322: (ASCII, b"16\0")}), INVALID, True)
    # 50000 x 50000 grey in two strips of 25000 rows: each below 2^31 bytes, together not
    add("u_deflate_2_31", write(g, compression=8, encoder=ENCODERS[8], override={256: (LONG, [50000]), 257: (LONG, [50000]), 278: (LONG, [25000]), 273: (LONG, [8, 8]),
                                                            279: (LONG, [8, 8])}), UNSUPPORTED, True)
    # tile sizes are LONGs: 2^31 x 2^31 RGBA tiles are 2^64 bytes, which is 0 in 64 bits; a width near 2^32 wraps the tiles across
    rgba = picture(6, 5, 4, seed=22)
    add("u_tile_2_64", write_tiles(rgba, **ok, override={322: (LONG, [1 << 31]), 323: (LONG, [1 << 31])}), UNSUPPORTED, True)
    add("u_tile_2_64_deflate", write_tiles(rgba, **ok, compression=8, override={322: (LONG, [1 << 31]), 323: (LONG, [1 << 31])}), UNSUPPORTED, True)
    add("u_tile_width_2_32", write_tiles(g, **ok, override={322: (LONG, [0xFFFFFFF0])}), UNSUPPORTED, True)
    add("u_tile_length_2_32", write_tiles(g, **ok, compression=5, override={323: (LONG, [0xFFFFFFF0])}), UNSUPPORTED, True)
    # six strips that all name the same 100 bytes: more compressed bytes than the file has
    shared = write(g, compression=8, rps=1, encoder=ENCODERS[8], override={273: (LONG, [8] * 6), 279: (LONG, [100] * 6)})
    assert 108 <= len(shared) < 600
    add("u_deflate_streams_overlap", shared, UNSUPPORTED, True)
    add("u_bigtiff", write_tiles(g, **ok).replace(b"II*\0", b"II+\0", 1), UNSUPPORTED, True)
    add("u_planar_2", write_tiles(picture(6, 5, 3, seed=21), **ok, compression=8, extra=[(284, SHORT, [2])]), UNSUPPORTED, True)
    add("u_predictor_3", write_tiles(g, **ok, compression=8, override={317: (SHORT, [3])}), UNSUPPORTED, True)
    add("u_bits_4", write(g, compression=8, encoder=ENCODERS[8], override={258: (SHORT, [4])}), UNSUPPORTED, True)
    add("u_compression_7", write_tiles(g, **ok, override={259: (SHORT, [7])}), UNSUPPORTED, True)
    add("i_lzw_tile_short", write_tiles(g, **ok, compression=5, encoder=lambda b: tiff_scenes._bad_lzw("short")), INVALID, False)
    add("i_pb_tile_short", write_tiles(g, **ok, compression=32773, encoder=lambda b: tiff_scenes.packbits(b)[:-2]), INVALID, False)
    return out
