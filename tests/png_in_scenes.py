"""The PNG files of the decoder's tests, all made at test time: a PNG writer with a chosen filter per row,
chosen IDAT split points and chosen chunks; a deflate token writer for the streams no encoder emits; zlib.compressobj with
chosen memLevel / strategy / flushes; Pillow's own save.  scene(name) -> the file's bytes, restated(name) -> ref_png_in's
decode of it (computed once), refused() -> name: (bytes, code).  The settle window of the device's inflate is 256
subsequences of 1024 bits, which is larger than the 255 412-bit block of "b_noise160": "t_fixed_long", a fixed block of
307 370 bits, and "t_far_long", a dynamic one of 284 026 bits, are the scenes that exceed it."""
import functools
import heapq
import io
import struct
import zlib

import numpy as np

import ref_png_in

INVALID, UNSUPPORTED = ref_png_in.INVALID, ref_png_in.UNSUPPORTED
SEED = 20240607


# ---- pictures -------------------------------------------------------------------------------------------------------------------
def rng(tag):
    return np.random.default_rng([SEED, zlib.crc32(tag.encode())])


def skewed(tag, n):
    """Bytes that zlib compresses into dynamic blocks (uniform noise comes out as stored blocks)."""
    return np.minimum(rng(tag).geometric(0.08, n) - 1, 255).astype(np.uint8)


def smooth(h, w, ch, tag="smooth", top=255):
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    planes = [np.sin(x / (7.0 + 3 * c) + c) * np.cos(y / (11.0 - 2 * c)) * 0.5 + 0.5 for c in range(ch)]
    noise = rng(tag).integers(0, 3, (h, w, ch))
    return np.clip(np.stack(planes, axis=2) * (top - 2) + noise, 0, top).astype(np.int64)


def pack(samples, depth):
    """[h, w, ch] integer samples -> [h, row_bytes] uint8."""
    h = samples.shape[0]
    flat = samples.reshape(h, -1).astype(np.int64)
    if depth == 8:
        return flat.astype(np.uint8)
    if depth == 16:
        out = np.zeros((h, flat.shape[1] * 2), dtype=np.uint8)
        out[:, 0::2], out[:, 1::2] = flat >> 8, flat & 255
        return out
    bits = ((flat[:, :, None] >> np.arange(depth - 1, -1, -1)) & 1).reshape(h, -1).astype(np.uint8)
    return np.packbits(bits, axis=1)


# ---- the PNG writer -------------------------------------------------------------------------------------------------------------
def chunk(typ, body=b"", crc=None):
    body = bytes(body)
    return struct.pack(">I", len(body)) + typ + body + struct.pack(">I", zlib.crc32(typ + body) if crc is None else crc)


def apply_filters(rows, filters, bpp):
    """[h, row_bytes] uint8 and a filter type per row -> the filtered image's bytes."""
    h, n = rows.shape
    out = bytearray()
    zero = np.zeros(n, dtype=np.int64)
    for y in range(h):
        cur, up = rows[y].astype(np.int64), rows[y - 1].astype(np.int64) if y else zero
        a = np.concatenate([np.zeros(bpp, dtype=np.int64), cur[:-bpp]]) if n > bpp else np.zeros(n, dtype=np.int64)
        c = np.concatenate([np.zeros(bpp, dtype=np.int64), up[:-bpp]]) if n > bpp else np.zeros(n, dtype=np.int64)
        t = filters[y % len(filters)]
        p = a + up - c
        pa, pb, pc = abs(p - a), abs(p - up), abs(p - c)
        pred = [zero, a, up, (a + up) >> 1, np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, up, c))][t]
        out.append(t)
        out += ((cur - pred) & 255).astype(np.uint8).tobytes()
    return bytes(out)


def ihdr(w, h, depth, colour, comp=0, filt=0, lace=0):
    return chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, depth, colour, comp, filt, lace))


def idats(stream, cuts=()):
    """The stream as IDAT chunks cut at `cuts` (positions; a repeated position gives an empty chunk)."""
    edges = [0, *sorted(cuts), len(stream)]
    return b"".join(chunk(b"IDAT", stream[a:b]) for a, b in zip(edges, edges[1:]))


def png(w, h, depth, colour, stream, cuts=(), before=(), after=()):
    return ref_png_in.SIGNATURE + ihdr(w, h, depth, colour) + b"".join(before) + idats(stream, cuts) + b"".join(after) + chunk(b"IEND")


def image_png(samples, depth, colour, filters=(0,), before=(), cuts=(), compress=None):
    """A file of [h, w, ch] samples."""
    h, w, ch = samples.shape
    rows = pack(samples, depth)
    filtered = apply_filters(rows, filters, max(1, ch * depth // 8))
    return png(w, h, depth, colour, (compress or zlib.compress)(filtered), cuts, before)


def compressor(**kw):
    def run(data, flushes=()):
        c = zlib.compressobj(**kw)
        out, at = b"", 0
        for where, mode in flushes:
            out += c.compress(data[at:where]) + c.flush(mode)
            at = where
        return out + c.compress(data[at:]) + c.flush()
    return run


# ---- the deflate token writer ---------------------------------------------------------------------------------------------------
def length_symbol(length):
    if length == 258:
        return 285, 0, 0
    if length < 11:
        return 254 + length, 0, 0
    x = length - 3
    e = x.bit_length() - 3
    return 257 + 4 * (e + 1) + ((x >> e) & 3), e, x & ((1 << e) - 1)


def distance_symbol(distance):
    if distance <= 4:
        return distance - 1, 0, 0
    x = distance - 1
    e = x.bit_length() - 2
    return 2 * (e + 1) + ((x >> e) & 1), e, x & ((1 << e) - 1)


def huffman_lengths(freqs, limit=15):
    """Code lengths of a complete code over the symbols used (at least two get a code)."""
    used = [s for s, f in enumerate(freqs) if f]
    lengths = [0] * len(freqs)
    for s in range(len(freqs)):
        if len(used) >= 2:
            break
        if s not in used:
            used.append(s)
    heap = [(freqs[s] or 1, s, (s,)) for s in used]
    heapq.heapify(heap)
    while len(heap) > 1:
        fa, ka, sa = heapq.heappop(heap)
        fb, kb, sb = heapq.heappop(heap)
        for s in sa + sb:
            lengths[s] += 1
        heapq.heappush(heap, (fa + fb, min(ka, kb), sa + sb))
    assert max(lengths) <= limit
    return lengths


def canonical(lengths):
    count = [0] * 17
    for n in lengths:
        count[n] += 1
    count[0] = 0
    code, nxt = 0, [0] * 17
    for bits in range(1, 17):
        code = (code + count[bits - 1]) << 1
        nxt[bits] = code
    codes = [0] * len(lengths)
    for s, n in enumerate(lengths):
        if n:
            codes[s] = nxt[n]
            nxt[n] += 1
    return codes


CL_LENGTHS = [4] * 13 + [5] * 6  # of the code-length code: complete, every symbol has a code


class Deflate:
    """Bits, first bit lowest.  A token: a literal 0 .. 255 or (length, distance)."""

    def __init__(self, cmf=0x78, flg=0x9C):
        self.bits, self.n = 0, 0
        self.put(cmf, 8), self.put(flg, 8)

    def put(self, value, count):
        self.bits |= (value & ((1 << count) - 1)) << self.n
        self.n += count

    def code(self, code, count):  # a Huffman code: its first bit first
        for k in range(count - 1, -1, -1):
            self.put(code >> k, 1)

    def stored(self, data, final=False, nlen=None):
        self.put(final, 1), self.put(0, 2)
        self.n = (self.n + 7) & ~7
        self.put(len(data), 16), self.put(len(data) ^ 0xFFFF if nlen is None else nlen, 16)
        self.put(int.from_bytes(bytes(data), "little"), 8 * len(data))   # (byte after byte, first bit lowest)

    def tokens(self, tokens, lit_lengths, dist_lengths, raw_symbols=()):
        lit, dist = canonical(lit_lengths), canonical(dist_lengths)
        for t in tokens:
            if isinstance(t, tuple):
                s, e, v = length_symbol(t[0])
                self.code(lit[s], lit_lengths[s]), self.put(v, e)
                s, e, v = distance_symbol(t[1])
                self.code(dist[s], dist_lengths[s]), self.put(v, e)
            else:
                self.code(lit[t], lit_lengths[t])
        for s in raw_symbols:  # symbols written as they are (286, 287)
            self.code(lit[s], lit_lengths[s])
        self.code(lit[256], lit_lengths[256])

    def fixed(self, tokens, final=False, raw_symbols=(), raw_distance=None):
        self.put(final, 1), self.put(1, 2)
        lit_lengths, dist_lengths = ref_png_in.FIXED_LENGTHS
        if raw_distance is not None:  # a length-3 match whose distance symbol is written as it is (30, 31)
            lit = canonical(lit_lengths)
            self.code(lit[257], 7), self.code(raw_distance, 5)
        self.tokens(tokens, lit_lengths, dist_lengths, raw_symbols)

    def dynamic(self, tokens, final=False, lit_lengths=None, dist_lengths=None, rle=False, hlit=None, lengths_override=None, cl_symbols=None):
        """lit_lengths / dist_lengths: chosen code lengths (default: a Huffman code of the tokens; no distance used: HDIST = 1
        with length 0; one used: the single code of one bit).  rle: repeat codes 16 / 17 / 18 over both tables as one run.
        cl_symbols: the code-length symbols as (symbol, extra value) pairs, instead of those of the lengths."""
        lf, df = [0] * 286, [0] * 30
        lf[256] = 1
        for t in tokens:
            if isinstance(t, tuple):
                lf[length_symbol(t[0])[0]] += 1
                df[distance_symbol(t[1])[0]] += 1
            else:
                lf[t] += 1
        if lit_lengths is None:
            lit_lengths = huffman_lengths(lf)
        if dist_lengths is None:
            used = [s for s, f in enumerate(df) if f]
            dist_lengths = [0] if not used else [int(s == used[0]) for s in range(used[0] + 1)] if len(used) == 1 else huffman_lengths(df)
        lit_lengths, dist_lengths = list(lit_lengths), list(dist_lengths)
        if hlit is None:
            hlit = max(257, max(s for s, n in enumerate(lit_lengths) if n) + 1)
        hdist = max(1, max([s for s, n in enumerate(dist_lengths) if n], default=0) + 1)
        sent = lengths_override if lengths_override is not None else lit_lengths[:hlit] + (dist_lengths + [0] * 30)[:hdist]
        self.put(final, 1), self.put(2, 2)
        self.put(hlit - 257, 5), self.put(hdist - 1, 5), self.put(19 - 4, 4)
        for s in ref_png_in.CL_ORDER:
            self.put(CL_LENGTHS[s], 3)
        cl = canonical(CL_LENGTHS)
        if cl_symbols is None:
            cl_symbols, i = [], 0
            while i < len(sent):
                run = 1
                while rle and i + run < len(sent) and sent[i + run] == sent[i]:
                    run += 1
                if rle and sent[i] == 0 and run >= 3:
                    take = min(run, 138)
                    cl_symbols.append((17, take - 3) if take < 11 else (18, take - 11))
                elif rle and run >= 4:
                    take = min(run - 1, 6)
                    cl_symbols += [(sent[i], 0), (16, take - 3)]
                    take += 1
                else:
                    take = 1
                    cl_symbols.append((sent[i], 0))
                i += take
        for s, v in cl_symbols:
            self.code(cl[s], CL_LENGTHS[s])
            self.put(v, {16: 2, 17: 3, 18: 7}.get(s, 0))
        self.tokens(tokens, (lit_lengths + [0] * 288)[:288], (dist_lengths + [0] * 32)[:32])

    def finish(self, data, adler=None, tail=b""):
        self.n = (self.n + 7) & ~7
        return self.bits.to_bytes(self.n // 8, "little") + struct.pack(">I", zlib.adler32(bytes(data)) if adler is None else adler) + tail


def expand(tokens, start=b""):
    out = bytearray(start)
    for t in tokens:
        if isinstance(t, tuple):
            for _ in range(t[0]):
                out.append(out[-t[1]])
        else:
            out.append(t)
    return bytes(out)


def grey_file(filtered, w, h, stream, **kw):
    assert len(filtered) == h * (w + 1)
    return png(w, h, 8, 0, stream, **kw)


# ---- the valid scenes -----------------------------------------------------------------------------------------------------------
SCENES = {}


def scene_of(name):
    def register(fn):
        SCENES[name] = fn
        return fn
    return register


def _typed(colour, depth, h, w, tag, filters=(0,), before=(), **kw):
    ch = ref_png_in.CHANNELS[colour]
    samples = rng(tag).integers(0, 1 << depth, (h, w, ch))
    if colour == 3:
        n = min(1 << depth, 256)
        before = (chunk(b"PLTE", rng(tag + "p").integers(0, 256, 3 * n).astype(np.uint8).tobytes()), *before)
    return image_png(samples, depth, colour, filters, before, **kw)


for _colour, _depths in ref_png_in.LEGAL.items():
    for _depth in _depths:
        for _h, _w in ((1, 1), (5, 3)):
            SCENES["s_c%d_d%d_%dx%d" % (_colour, _depth, _w, _h)] = functools.partial(_typed, _colour, _depth, _h, _w, "s%d%d%d" % (_colour, _depth, _w),
                                                                                     filters=(0, 1, 2, 3, 4))
for _depth in (1, 2, 4):
    for _w in (1, 7, 9):
        SCENES["s_grey_d%d_w%d" % (_depth, _w)] = functools.partial(_typed, 0, _depth, 4, _w, "w%d%d" % (_depth, _w), filters=(4, 3, 2, 1))
        SCENES["s_pal_d%d_w%d" % (_depth, _w)] = functools.partial(_typed, 3, _depth, 4, _w, "p%d%d" % (_depth, _w), filters=(1, 4))
for _name, _colour, _depth in (("rgb", 2, 8), ("rgba", 6, 8), ("la", 4, 8), ("rgb16", 2, 16)):
    SCENES["s_47x33_" + _name] = functools.partial(_typed, _colour, _depth, 33, 47, _name, filters=(0, 1, 2, 3, 4))
SCENES["s_pal256"] = functools.partial(_typed, 3, 8, 9, 31, "pal256", filters=(0, 4))


@scene_of("s_pal2_trns")
def _():
    samples = rng("pal2").integers(0, 2, (6, 13, 1))
    return image_png(samples, 1, 3, (0, 2), (chunk(b"PLTE", bytes([10, 20, 30, 200, 100, 50])), chunk(b"tRNS", bytes([0, 255]))))


@scene_of("s_grey_trns_gama")
def _():
    return image_png(smooth(7, 9, 1), 8, 0, (4,), (chunk(b"gAMA", struct.pack(">I", 45455)), chunk(b"tRNS", b"\0\x05"), chunk(b"teSt", b"\0" * 8)))


for _t in range(5):
    SCENES["f_all_%d" % _t] = functools.partial(lambda t: image_png(smooth(12, 19, 3, "f%d" % t), 8, 2, (t,)), _t)
SCENES["f_cycle"] = lambda: image_png(smooth(23, 17, 3, "cycle"), 8, 2, (0, 1, 2, 3, 4))
for _t in (2, 3, 4):
    SCENES["f_first_%d" % _t] = functools.partial(lambda t: image_png(smooth(3, 21, 4, "first%d" % t), 8, 6, (t, 1)), _t)
for _name, _colour, _depth in (("bpp1", 0, 8), ("bpp2", 4, 8), ("bpp3", 2, 8), ("bpp4", 6, 8), ("bpp6", 2, 16), ("bpp8", 6, 16)):
    SCENES["f_" + _name] = functools.partial(_typed, _colour, _depth, 9, 11, "b" + _name, filters=(4, 3, 1, 2, 4, 4, 0))


@scene_of("f_paeth_ties")
def _():
    # a = b, b = c, a = c and all equal, in every order of the three: few distinct values
    return image_png(rng("ties").integers(0, 3, (16, 24, 1)) * 40, 8, 0, (4,))


SCENES["f_130_paeth"] = lambda: image_png(smooth(130, 23, 3, "p130"), 8, 2, (4,))
SCENES["f_third_sub"] = lambda: image_png(smooth(70, 15, 3, "third"), 8, 2, (1, 4, 3))


def _noise_rgb(h, w, tag):
    return skewed(tag, h * w * 3).reshape(h, w, 3).astype(np.int64)


SCENES["b_mem1"] = lambda: image_png(_noise_rgb(40, 48, "mem3"), 8, 2, compress=compressor(level=6, memLevel=1))
SCENES["b_mem8"] = lambda: image_png(_noise_rgb(40, 48, "mem3"), 8, 2, compress=compressor(level=6, memLevel=8))
SCENES["b_fixed"] = lambda: image_png(_noise_rgb(40, 48, "mem3"), 8, 2, compress=compressor(level=6, strategy=zlib.Z_FIXED))
SCENES["b_stored"] = lambda: image_png(_noise_rgb(40, 48, "mem3"), 8, 2, compress=compressor(level=0))
SCENES["b_flushes"] = lambda: image_png(_noise_rgb(40, 48, "flush"), 8, 2,
                                        compress=lambda d: compressor(level=6)(d, ((1500, zlib.Z_SYNC_FLUSH), (3100, zlib.Z_FULL_FLUSH))))
SCENES["b_noise160"] = lambda: image_png(_noise_rgb(160, 160, "n160"), 8, 2, compress=compressor(level=6, memLevel=9))


def token_picture(w, h, tag, plan):
    """A grey 8-bit picture (filter type 0 on every row) and the tokens that write its filtered bytes.  plan: a number n - n
    literals of a random picture (0 at the filter bytes) - or a (length, distance) copy; literals fill the rest."""
    total, rand = h * (w + 1), rng(tag).integers(0, 256, h * (w + 1))
    tokens, out = [], bytearray()

    def literals(n):
        for _ in range(n):
            v = 0 if len(out) % (w + 1) == 0 else int(rand[len(out)])
            tokens.append(v), out.append(v)

    for step in plan:
        if isinstance(step, tuple):
            tokens.append(step)
            out[:] = expand([step], out)
        else:
            literals(step)
    literals(total - len(out))
    assert len(out) == total and all(out[y * (w + 1)] <= 4 for y in range(h))
    return tokens, bytes(out)


@scene_of("t_far_long")
def _():
    # distance 32 768 (rows are 256 bytes: a filter byte is copied from a filter byte) and 24 577, codes with 13 extra bits; length 258
    tokens, out = token_picture(255, 140, "far", [32768, (258, 32768), (258, 32768), (3, 24577)])
    d = Deflate()
    d.dynamic(tokens, final=True)
    return grey_file(out, 255, 140, d.finish(out))


@scene_of("t_overlaps")
def _():
    # copies with distance < length: 1, 2, 3 (= bpp of this RGB file)
    w, h = 20, 6
    row = 1 + 3 * w
    tokens = []
    for y, dist in zip(range(h), (1, 2, 3, 1, 2, 3)):
        tokens += [0] + [y + 1, 2 * y + 2, 3 * y + 3][:dist] + [(row - 1 - dist, dist)]
    out = expand(tokens)
    d = Deflate()
    d.dynamic(tokens, final=True)
    return png(w, h, 8, 2, d.finish(out))


@scene_of("t_three_blocks_back")
def _():
    # a copy of a copy of a copy, each in its own block, and a copy that reaches back through three blocks
    w, h = 15, 8
    d = Deflate()
    blocks = [[0] + list(range(10, 25)), [(16, 16)], [(16, 16)], [(16, 16), (16, 64), (16, 16), (16, 16), (16, 48)]]
    d.dynamic(blocks[0]), d.fixed(blocks[1]), d.dynamic(blocks[2]), d.fixed(blocks[3], final=True)
    out = expand(sum(blocks, []))
    return grey_file(out, w, h, d.finish(out))


@scene_of("t_stored_alignments")
def _():
    # a stored block behind a block that ends at each of the 8 bit alignments (j nine-bit literals move the end by j bits); a
    # block that is only an end-of-block, fixed and dynamic; a final empty stored block
    w, h = 50, 3
    rest = rng("align").integers(0, 200, h * (w + 1)).astype(np.uint8)
    for y in range(h):
        rest[y * (w + 1)] = y + 1
    d, out = Deflate(), bytearray()
    for j in range(8):
        piece = [0] if j == 0 else [200] * j
        d.fixed(piece)
        d.stored(bytes([7, 9]))
        out += bytes(piece) + bytes([7, 9])
    d.fixed([])
    d.dynamic([])
    tail = bytes(rest[len(out):])
    d.dynamic(list(tail))
    d.stored(b"", final=True)
    out += tail
    return grey_file(bytes(out), w, h, d.finish(out))


@scene_of("t_literals_only")
def _():
    # a dynamic block with HDIST = 1 and that one distance length 0; a repeat code 16 that runs from the literal lengths into
    # the distance lengths (second block)
    w, h = 9, 6
    picture = rng("lit").integers(0, 16, (h, w)).astype(np.uint8)
    filtered = b"".join(b"\0" + picture[y].tobytes() for y in range(h))
    half = len(filtered) // 2
    d = Deflate()
    d.dynamic(list(filtered[:half]))
    # lengths: literals 0 .. 15 five bits (16 codes), 256 and 257 .. 259 three bits (4 codes); distances 0 .. 3 three bits, 4 .. 7 three bits:
    lit = [5] * 16 + [0] * 240 + [3, 3, 3, 3]
    assert sum(2.0 ** -n for n in lit if n) == 1.0
    dist = [3] * 8
    d.dynamic(list(filtered[half:-5]) + [(5, 5)], final=True, lit_lengths=lit, dist_lengths=dist, rle=True)
    out = expand([(5, 5)], filtered[:-5])
    return grey_file(out, w, h, d.finish(out))


@scene_of("t_fixed_long")
def _():
    # one fixed block of 34 000 nine-bit literals: longer than a settle window of 256 x 1024 bits
    w, h = 200, 170
    picture = rng("long").integers(144, 256, (h, w)).astype(np.uint8)
    filtered = b"".join(b"\0" + picture[y].tobytes() for y in range(h))
    d = Deflate()
    d.fixed(list(filtered), final=True)
    return grey_file(filtered, w, h, d.finish(filtered))


SCENES["flat200"] = lambda: image_png(np.zeros((200, 200, 1), dtype=np.int64), 8, 0, compress=compressor(level=9))


def _rgb4733():
    return _typed(2, 8, 33, 47, "rgb", filters=(0, 1, 2, 3, 4))


def _resplit(cuts_of):
    base = _rgb4733()
    h = ref_png_in.parse(base)
    stream = ref_png_in.stream_of(base, h)
    return png(47, 33, 8, 2, stream, cuts_of(len(stream)))


SCENES["i_one"] = _rgb4733
SCENES["i_bytes"] = lambda: _resplit(lambda n: range(1, n))
SCENES["i_empties"] = lambda: _resplit(lambda n: (0, 0, 100, 100, 100, n // 2, n, n))
SCENES["i_header_adler"] = lambda: _resplit(lambda n: (1, n - 2))


def exif_block(focal, short=True, order="<", broken=False):
    o = order
    head = (b"II" if o == "<" else b"MM") + struct.pack(o + "HI", 42, 8)
    ifd0 = struct.pack(o + "H", 1) + struct.pack(o + "HHII", 0x8769, 4, 1, 1 << 20 if broken else 26) + struct.pack(o + "I", 0)
    value = struct.pack(o + "HH", focal, 0) if short else struct.pack(o + "I", focal)
    sub = struct.pack(o + "H", 1) + struct.pack(o + "HHI", 0xA405, 3 if short else 4, 1) + value + struct.pack(o + "I", 0)
    return head + ifd0 + sub


FOCAL = {}
for _short in (True, False):
    for _order in "<>":
        _name = "x_%s_%s" % ("short" if _short else "long", "le" if _order == "<" else "be")
        FOCAL[_name] = 35 + 2 * len(FOCAL)
        SCENES[_name] = functools.partial(lambda s, o, f: image_png(smooth(5, 6, 3), 8, 2, (1,), (chunk(b"eXIf", exif_block(f, s, o)),)), _short, _order, FOCAL[_name])
SCENES["x_broken"] = lambda: image_png(smooth(5, 6, 3), 8, 2, (1,), (chunk(b"eXIf", exif_block(50, broken=True)),))


def _pillow(optimize):
    from PIL import Image

    buf = io.BytesIO()
    Image.fromarray(smooth(300, 300, 3, "pil").astype(np.uint8)).save(buf, "PNG", optimize=optimize)
    return buf.getvalue()


SCENES["p_default"] = functools.partial(_pillow, False)
SCENES["p_optimize"] = functools.partial(_pillow, True)


# ---- the seams of the unfilter kernel: tiles of 384 bytes of a row, batches of 64 rows of a segment ----------------------------
TILE_BYTES, BATCH_ROWS = 384, 64
BPP_KINDS = {1: (0, 8), 2: (4, 8), 3: (2, 8), 4: (6, 8), 6: (2, 16), 8: (6, 16)}   # bpp: (colour type, depth)
SEAMS = {}   # name: (bpp, row bytes, the filter type of every row), what tests/test_png_in_ref.py finds in the file


def segments_of(types):
    """The lengths of the row segments: a segment begins at row 0 and at every None or Sub row."""
    starts = [y for y, t in enumerate(types) if y == 0 or t < 2] + [len(types)]
    return [b - a for a, b in zip(starts, starts[1:])]


def _seam(name, colour, depth, w, h, filters):
    row_bytes = (w * ref_png_in.CHANNELS[colour] * depth + 7) // 8
    SEAMS[name] = (max(1, ref_png_in.CHANNELS[colour] * depth // 8), row_bytes, [filters[y % len(filters)] for y in range(h)])
    SCENES[name] = functools.partial(_typed, colour, depth, h, w, name, filters=filters)


# two full tiles and a pixel, two full batches and two rows, noise (zlib stores it: about 100 KB a file): one segment of 130
# rows under Paeth, Average and Up / Average / Paeth in turn, and 130 segments of a Sub row, where `last` alone is carried
for _bpp, (_colour, _depth) in BPP_KINDS.items():
    for _tag, _filters in (("paeth", (4,)), ("average", (3,)), ("mixed", (2, 3, 4)), ("sub", (1,))):
        _seam("m_bpp%d_%s" % (_bpp, _tag), _colour, _depth, 2 * TILE_BYTES // _bpp + 1, 2 * BATCH_ROWS + 2, _filters)
    # a row of exactly one tile and of exactly two: the last tile has nothing behind it
    for _tiles in (1, 2):
        _seam("m_bpp%d_%dtiles" % (_bpp, _tiles), _colour, _depth, _tiles * TILE_BYTES // _bpp, 20, (1, 4, 3, 2, 4, 3, 2))
# segments that end on batch edges, rows of 450 bytes: 64 rows (the next batch finds no row of its segment), 65 rows, 63 rows
# (the next segment begins at lane 63 of the batch), and a last row alone
SEGMENT_EDGES = (0,) + (4,) * 63 + (1,) + (2,) * 64 + (1,) + (3,) * 62 + (0,) + (0,)
_seam("g_segment_edges", 2, 8, 150, len(SEGMENT_EDGES), SEGMENT_EDGES)
# packed samples, rows of a tile and a byte and of two tiles and a byte
for _kind, _colour, _depth in (("grey", 0, 1), ("grey", 0, 2), ("grey", 0, 4), ("pal", 3, 4)):
    for _tiles in (1, 2):
        _seam("k_%s_d%d_%d" % (_kind, _depth, _tiles * TILE_BYTES + 1), _colour, _depth, _tiles * TILE_BYTES * 8 // _depth + 1, 3, (1, 4, 3))


@scene_of("t_stored_65535")
def _():
    # a stored block of the largest LEN, a second stored block behind it, then a dynamic block
    w, h = 255, 260
    filtered = apply_filters(pack(rng("st65535").integers(0, 256, (h, w, 1)), 8), (0, 1, 2, 3, 4), 1)
    d = Deflate()
    d.stored(filtered[:65535]), d.stored(filtered[65535:66000])
    d.dynamic(list(filtered[66000:]), final=True)
    return grey_file(filtered, w, h, d.finish(filtered))


SEAMS["t_stored_65535"] = (1, 255, [y % 5 for y in range(260)])


def names():
    return sorted(SCENES)


@functools.lru_cache(maxsize=None)
def scene(name) -> bytes:
    return SCENES[name]()


@functools.lru_cache(maxsize=None)
def restated(name) -> dict:
    return ref_png_in.decode(scene(name), fast=True)


# ---- the refused files: a good file and the smallest edit ----------------------------------------------------------------------
def _good():
    return image_png(smooth(6, 7, 3, "good"), 8, 2, (0, 1, 2, 3, 4))


def _good_stream():
    return ref_png_in.stream_of(_good())


def _with_stream(stream, w=7, h=6, depth=8, colour=2):
    return png(w, h, depth, colour, stream)


def _patch(data, at, value):
    out = bytearray(data)
    out[at] = value
    return bytes(out)


def _reihdr(data, **kw):
    """The good file with fields of its IHDR changed (and the CRC made right again)."""
    w, h, depth, colour, comp, filt, lace = struct.unpack(">IIBBBBB", data[16:29])
    f = {"w": w, "h": h, "depth": depth, "colour": colour, "comp": comp, "filt": filt, "lace": lace, **kw}
    return data[:8] + ihdr(f["w"], f["h"], f["depth"], f["colour"], f["comp"], f["filt"], f["lace"]) + data[33:]


def _filtered_good():
    return zlib.decompress(_good_stream())


@functools.lru_cache(maxsize=None)
def refused() -> dict:
    good, stream, filtered = _good(), _good_stream(), _filtered_good()
    idat_at = good.index(b"IDAT") - 4
    iend_at = good.index(b"IEND") - 4
    out = {}
    U, I = UNSUPPORTED, INVALID
    out["u_adam7"] = (_reihdr(good, lace=1), U)
    out["u_wide"] = (_reihdr(good, w=65536), U)
    out["u_tall"] = (_reihdr(good, h=65536), U)
    out["u_2g"] = (_reihdr(good, w=65535, h=65535, colour=6, depth=16), U)
    out["i_signature"] = (_patch(good, 0, 0x88), I)
    out["i_first_chunk"] = (good[:8] + chunk(b"gAMA", struct.pack(">I", 45455)) + good[8:], I)
    out["i_ihdr_14"] = (good[:8] + chunk(b"IHDR", good[16:29] + b"\0") + good[33:], I)
    out["i_zero_width"] = (_reihdr(good, w=0), I)
    out["i_zero_height"] = (_reihdr(good, h=0), I)
    out["i_pair"] = (_reihdr(good, depth=4), I)
    out["i_colour_1"] = (_reihdr(good, colour=1), I)
    out["i_compression"] = (_reihdr(good, comp=1), I)
    out["i_filter_method"] = (_reihdr(good, filt=1), I)
    out["i_interlace_2"] = (_reihdr(good, lace=2), I)
    pal = image_png(rng("rp").integers(0, 4, (5, 6, 1)), 2, 3, (0,), (chunk(b"PLTE", bytes(range(12))),))
    plte_at = pal.index(b"PLTE") - 4
    out["i_no_plte"] = (pal[:plte_at] + pal[plte_at + 24:], I)
    out["i_plte_10"] = (pal[:plte_at] + chunk(b"PLTE", bytes(10)) + pal[plte_at + 24:], I)
    out["i_plte_771"] = (pal[:plte_at] + chunk(b"PLTE", bytes(771)) + pal[plte_at + 24:], I)
    out["i_index_beyond"] = (pal[:plte_at] + chunk(b"PLTE", bytes(9)) + pal[plte_at + 24:], I)
    out["i_no_idat"] = (good[:idat_at] + good[iend_at:], I)
    half = len(stream) // 2
    out["i_idat_apart"] = (ref_png_in.SIGNATURE + ihdr(7, 6, 8, 2) + chunk(b"IDAT", stream[:half]) + chunk(b"tEXt", b"a\0b") + chunk(b"IDAT", stream[half:]) + chunk(b"IEND"), I)
    out["i_chunk_past"] = (good[:idat_at] + struct.pack(">I", 1 << 20) + good[idat_at + 4:], I)
    out["i_no_iend"] = (good[:iend_at], I)
    out["i_cut_in_iend"] = (good[:-3], I)
    out["i_critical"] = (good[:idat_at] + chunk(b"ABCD", b"xy") + good[idat_at:], I)
    out["i_crc_ihdr"] = (_patch(good, 32, good[32] ^ 1), I)
    out["i_crc_idat"] = (_patch(good, iend_at - 1, good[iend_at - 1] ^ 0x80), I)
    out["i_crc_iend"] = (_patch(good, len(good) - 1, good[-1] ^ 1), I)
    out["i_crc_text"] = (good[:idat_at] + chunk(b"tEXt", b"a\0b", crc=5) + good[idat_at:], I)
    for name, cmf, flg in (("cm", 0x79, 0x9C), ("cinfo", 0x88, 0x9C), ("fdict", 0x78, 0xBC), ("fcheck", 0x78, 0x9D)):
        if name != "fcheck":  # (FCHECK made right for the others: the named field alone is wrong)
            flg = (flg & 0xE0) + (31 - ((cmf << 8 | (flg & 0xE0)) % 31)) % 31
        out["i_zlib_" + name] = (_with_stream(bytes([cmf, flg]) + stream[2:]), I)

    def made(write, data=filtered, **kw):
        d = Deflate()
        write(d)
        return _with_stream(d.finish(data, **kw))

    lits = list(filtered)
    out["i_btype3"] = (made(lambda d: (d.put(1, 1), d.put(3, 2), d.put(0, 32))), I)
    out["i_nlen"] = (made(lambda d: d.stored(filtered, final=True, nlen=len(filtered))), I)
    over = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 6
    over[0] = 1
    out["i_oversubscribed"] = (made(lambda d: d.dynamic(lits, final=True, lit_lengths=over, dist_lengths=[5] * 30)), I)
    incomplete = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 6
    out["i_incomplete"] = (made(lambda d: d.dynamic(lits, final=True, lit_lengths=incomplete, dist_lengths=[0])), I)
    out["i_incomplete_dist"] = (made(lambda d: d.dynamic(lits, final=True, dist_lengths=[2, 2, 2])), I)
    out["i_repeat_first"] = (made(lambda d: d.dynamic(lits, final=True, cl_symbols=[(16, 0)] + [(8, 0)] * 300)), I)
    out["i_lengths_past"] = (made(lambda d: d.dynamic(lits, final=True, lit_lengths=[8] * 256 + [1], dist_lengths=[0],
                                                      cl_symbols=[(8, 0)] * 256 + [(1, 0), (18, 127)])), I)
    out["i_no_256"] = (no_eob_file(), I)
    out["i_symbol_286"] = (made(lambda d: d.fixed(lits, final=True, raw_symbols=[286])), I)
    out["i_distance_30"] = (made(lambda d: d.fixed(lits, final=True, raw_distance=30)), I)
    out["i_too_far"] = (made(lambda d: d.fixed(lits[:5] + [(3, 6)] + lits[8:], final=True)), I)
    full = Deflate()
    full.fixed(lits, final=True)
    whole = full.finish(filtered)
    out["i_no_final_eob"] = (_with_stream(whole[:len(whole) - 6]), I)
    out["i_not_final"] = (made(lambda d: d.fixed(lits)), I)
    out["i_short_output"] = (made(lambda d: d.fixed(lits[:-1], final=True), data=filtered[:-1]), I)
    out["i_long_output"] = (made(lambda d: d.fixed(lits + [0], final=True), data=filtered + b"\0"), I)
    out["i_adler"] = (made(lambda d: d.fixed(lits, final=True), adler=zlib.adler32(filtered) ^ 1), I)
    out["i_adler_cut"] = (_with_stream(whole[:-2]), I)
    bad_filter = bytearray(filtered)
    bad_filter[22 * 3] = 5
    out["i_filter_5"] = (_with_stream(zlib.compress(bytes(bad_filter))), I)
    return out


def no_eob_file():
    """A dynamic block whose lengths give symbol 256 no code."""
    filtered = _filtered_good()
    d = Deflate()
    lengths = [8] * 256 + [0]  # complete over the literals, nothing for 256
    d.put(1, 1), d.put(2, 2), d.put(0, 5), d.put(0, 5), d.put(15, 4)
    for s in ref_png_in.CL_ORDER:
        d.put(CL_LENGTHS[s], 3)
    cl = canonical(CL_LENGTHS)
    for n in lengths + [0]:
        d.code(cl[n], CL_LENGTHS[n])
    d.put(0, 64)
    return _with_stream(d.finish(filtered))


# accepted here though malformed elsewhere (excluded by name from the comparison with Pillow)
ACCEPTED_HERE = ("a_tail_behind_adler", "a_far_cinfo")


@functools.lru_cache(maxsize=None)
def accepted() -> dict:
    out = {"a_tail_behind_adler": _with_stream(_good_stream() + b"tail")}
    # CINFO = 0 (a 256-byte window) with a distance of 300
    w, h = 30, 20
    tokens, filtered = token_picture(w, h, "cinfo", [311, (20, 300)])
    d = Deflate(cmf=0x08, flg=(31 - (0x08 << 8) % 31) % 31)
    d.dynamic(tokens, final=True)
    out["a_far_cinfo"] = grey_file(bytes(filtered), w, h, d.finish(filtered))
    return out
