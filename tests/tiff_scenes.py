"""TIFF files for the tests of cvhip_tiff_decode: a writer of its own - both byte orders, SHORT or LONG
values, inline or at offsets, strips in any order, LZW and PackBits encoders that can be steered to the cases the decoder
has to get right - and a wrapper around Pillow's (libtiff's) writer.  scene(name) -> the file's bytes; refused() -> the files
that are refused, with the code; SEM_BLOCKS -> texts of the SEM block with the expected metadata."""
import functools
import io
import struct

import numpy as np

import ref_tiff

INVALID, UNSUPPORTED = ref_tiff.INVALID, ref_tiff.UNSUPPORTED
BYTE, ASCII, SHORT, LONG = 1, 2, 3, 4


# ---- pictures -----------------------------------------------------------------------------------------------------------------
def picture(h, w, spp=1, bits=8, seed=1, kind="smooth"):
    """[h, w, spp] uint8 or uint16, deterministic."""
    rng = np.random.default_rng(seed)
    top = (1 << bits) - 1
    if kind == "noise":
        a = rng.integers(0, top + 1, size=(h, w, spp))
    elif kind == "flat":
        a = np.full((h, w, spp), 77 if bits == 8 else 30000)
    else:
        y, x = np.mgrid[0:h, 0:w]
        a = np.stack([(x * (3 + c) + y * (5 - c) + rng.integers(0, 3, size=(h, w))) * (1 if bits == 8 else 211) for c in range(spp)], axis=2) % (top + 1)
    return a.astype(np.uint8 if bits == 8 else np.uint16)


# ---- encoders -------------------------------------------------------------------------------------------------------------------
class _Bits:
    def __init__(self):
        self.acc, self.n, self.out, self.c, self.widths = 0, 0, bytearray(), 0, set()

    def code(self, code):
        w = ref_tiff.code_width(self.c)
        self.widths.add(w)
        self.acc, self.n = (self.acc << w) | code, self.n + w
        while self.n >= 8:
            self.out.append((self.acc >> (self.n - 8)) & 255)
            self.n -= 8
        self.acc &= (1 << self.n) - 1
        self.c = 0 if code == 256 else self.c + 1

    def done(self):
        if self.n:
            self.out.append((self.acc << (8 - self.n)) & 255)
        return bytes(self.out)


def lzw(data: bytes, clear_every=3836, initial_clear=True, clears=1, eoi=True, junk=b"", literals=False, trace=None):
    """TIFF 6.0 LZW of data.  clear_every: a Clear after that many codes (libtiff clears when entry 4094 is next: 3836 codes);
    None - never, the table fills and stays.  clears: how many Clear codes stand where one does.  literals: no strings."""
    bits, table, w = _Bits(), {}, b""
    self_overlaps, clear_at, eoi_at = 0, [], None

    def clear():
        for _ in range(clears):
            clear_at.append(bits.c)   # (the Clear is the c-th code since the Clear before it: lane c % 64 of its batch)
            bits.code(256)
        table.clear()

    def emit(string):
        nonlocal self_overlaps
        code = string[0] if len(string) == 1 else table[string]
        if len(string) > 1 and code == 258 + bits.c - 1:   # (the entry the decoder is only now adding: its string overlaps itself)
            self_overlaps += 1
        bits.code(code)

    if initial_clear:
        clear()
    for byte in data:
        k = bytes([byte])
        if not literals and (w + k in table or not w):
            w += k
            continue
        if literals and not w:
            w = k
            continue
        emit(w)
        if 258 + bits.c - 1 < 4096:
            table[w + k] = 258 + bits.c - 1   # (entry 258 + j: the string of code j and the first byte of code j + 1)
        w = k
        if clear_every is not None and bits.c >= clear_every:
            clear()
    if w:
        emit(w)
    last = bits.c   # the codes since the last Clear: the rows are full behind them
    if eoi:
        eoi_at = bits.c
        bits.code(257)
    if trace is not None:
        trace.update(widths=bits.widths, self_overlaps=self_overlaps, clear_at=clear_at, eoi_at=eoi_at, codes_after_last_clear=last)
    return bits.done() + junk


def packbits(data: bytes, noop_every=0, overshoot=False):
    """PackBits of data as one stream (packets cross row ends).  noop_every: a header 128 in front of every n-th packet;
    overshoot: the last packet is a run of 128 that reaches past the data."""
    out, at, n, packets = bytearray(), 0, len(data), 0

    def header(b):
        nonlocal packets
        if noop_every and packets % noop_every == 0:
            out.append(128)
        packets += 1
        out.append(b)

    while at < n:
        run = 1
        while at + run < n and run < 128 and data[at + run] == data[at]:
            run += 1
        if run >= 3:
            if overshoot and at + run == n:
                run = 128
            header(257 - run)
            out.append(data[at])
            at += run
            continue
        end = at
        while end < n and end - at < 128 and not (end + 2 < n and data[end] == data[end + 1] == data[end + 2]):
            end += 1
        header(end - at - 1)
        out += data[at:end]
        at = end
    return bytes(out)


def packets(plan):
    """A PackBits stream written packet by packet.  plan: ("run", n, byte), ("lit", bytes) or ("noop",) -> (stream, the
    bytes it expands to)."""
    stream, data = bytearray(), bytearray()
    for p in plan:
        if p[0] == "noop":
            stream.append(128)
        elif p[0] == "run":
            assert 2 <= p[1] <= 128
            stream += bytes([257 - p[1], p[2]])
            data += bytes([p[2]]) * p[1]
        else:
            assert 1 <= len(p[1]) <= 128
            stream += bytes([len(p[1]) - 1]) + bytes(p[1])
            data += bytes(p[1])
    return bytes(stream), bytes(data)


def short_packets(total, count, run_first, seed, noop_at=None, cut=0):
    """A plan of `count` packets that expand to `total` bytes (+ `cut`, which the last packet, a run, reaches past the strip's
    rows): two-byte runs and one-byte literals in turn, the first packets lengthened by what the short ones leave over.
    noop_at: the packet of that number (from 0) is a header 128."""
    rng = np.random.default_rng(seed)
    kinds = [(k % 2 == 0) == run_first for k in range(count)]   # True: a run
    if cut:
        kinds[-1] = True
    lens = [2 if run else 1 for run in kinds]
    if noop_at is not None:
        lens[noop_at] = 0
    if cut:
        lens[-1] = 1 + cut   # one byte inside the rows
    slack = total + cut - sum(lens)
    assert slack >= 0
    for k in range(count):
        if lens[k] and not (cut and k == count - 1):
            add = min(slack, 128 - lens[k])
            lens[k], slack = lens[k] + add, slack - add
    assert slack == 0
    plan, before = [], -1
    for run, n in zip(kinds, lens):
        if n == 0:
            plan.append(("noop",))
            continue
        values = rng.integers(0, 256, size=1 if run else n)
        values[0] = (values[0] if values[0] != before else values[0] + 1) % 256
        plan.append(("run", n, int(values[0])) if run else ("lit", bytes(values.astype(np.uint8))))
        before = int(values[-1])
    return plan


# the strips of "o_pb_batches", 300 bytes each (3 rows of 100): (packets, a run first, the number of a header 128, the bytes
# the last packet reaches past the rows).  A batch of the kernel is 64 packets; the 64th and 65th have the numbers 63 and 64
PB_BATCHES = ((64, True, None, 0), (65, True, None, 0), (65, False, None, 0), (128, False, None, 0), (129, True, None, 0), (200, True, None, 0),
              (130, True, 64, 0), (193, False, 128, 0), (65, True, None, 7), (129, False, None, 100))


def pb_batches():
    plans = [short_packets(300, n, first, 40 + k, noop, cut) for k, (n, first, noop, cut) in enumerate(PB_BATCHES)]
    made = [packets(plan) for plan in plans]
    a = np.frombuffer(b"".join(data[:300] for _, data in made), dtype=np.uint8).reshape(3 * len(made), 100, 1)
    streams = iter([stream for stream, _ in made])
    return write(a, compression=32773, rps=3, encoder=lambda raw: next(streams))


def _lzw_full_batches(eoi):
    """33 pixels wide, the height at which the codes behind the initial Clear are a multiple of 64: the rows are full at a
    batch's end and EOI, where there is one, would be the next batch's first code."""
    for h in range(20, 200):
        a, trace = picture(h, 33, seed=2), {}
        lzw(a.tobytes(), trace=trace)
        if trace["codes_after_last_clear"] % 64 == 0:
            return write(a, compression=5, encoder=functools.partial(lzw, eoi=eoi))
    raise AssertionError("no height ends its codes at a batch's end")


# ---- the writer -----------------------------------------------------------------------------------------------------------------
def write(a, order="<", compression=1, predictor=1, rps=None, photometric=None, strip_order=None, long_values=False, byte_counts=True,
          encoder=None, extra=(), override=None, magic=42, data_at=8, bps_once=False, exif_focal=None, exif_short=True):
    """a: [h, w, spp] uint8 / uint16.  order: "<" (II) or ">" (MM).  rps: None - no RowsPerStrip tag.  strip_order: the order
    the strips lie in the file.  extra: (tag, type, values or bytes) entries.  override: {tag: (type, values) or None (drop)}."""
    h, w, spp = a.shape
    bits = 8 * a.dtype.itemsize
    rows_per = h if rps is None or rps > h else rps
    nstrips = -(-h // rows_per)
    stored = a
    if predictor == 2:
        stored = a.copy()
        stored[:, 1:] = a[:, 1:] - a[:, :-1]   # (wraps modulo 2^8 or 2^16)
    raw = stored.astype(stored.dtype.newbyteorder(order)).tobytes()
    row_bytes = w * spp * bits // 8
    encoder = encoder or {1: lambda b: b, 5: lzw, 32773: packbits}[compression]
    strips = [encoder(raw[s * rows_per * row_bytes:(s + 1) * rows_per * row_bytes]) for s in range(nstrips)]
    body, offsets = bytearray(b"\0" * (data_at - 8)), [0] * nstrips
    for s in (strip_order if strip_order is not None else range(nstrips)):
        offsets[s] = 8 + len(body)
        body += strips[s]
    if photometric is None:
        photometric = 1 if spp == 1 else 2
    kind = LONG if long_values else SHORT
    entries = {256: (kind, [w]), 257: (kind, [h]), 258: (SHORT, [bits] * (1 if bps_once else spp)), 259: (SHORT, [compression]),
               262: (SHORT, [photometric]), 273: (LONG if long_values or 8 + len(body) >= 65536 else SHORT, offsets), 277: (SHORT, [spp])}
    if rps is not None:
        entries[278] = (kind, [rps])
    if byte_counts:
        entries[279] = (LONG if long_values or max(len(s) for s in strips) >= 65536 else SHORT, [len(s) for s in strips])
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
    return assemble(order, entries, bytes(body), magic, exif_focal, exif_short)


def _pack(order, typ, values):
    if isinstance(values, (bytes, bytearray)):
        return bytes(values), len(values)
    fmt = {BYTE: "B", SHORT: "H", LONG: "I", 13: "I", 11: "f", 8: "h"}[typ]
    return struct.pack(order + fmt * len(values), *values), len(values)


def assemble(order, entries, body, magic=42, exif_focal=None, exif_short=True):
    """header, body (it begins at byte 8), the values that do not fit, the Exif IFD, then the IFD."""
    blob = bytearray(body)
    if len(blob) & 1:
        blob.append(0)
    if exif_focal is not None:
        exif_at = 8 + len(blob)
        value = struct.pack(order + ("HH" if exif_short else "I"), *((exif_focal, 0) if exif_short else (exif_focal,)))
        blob += struct.pack(order + "HHHI", 1, 0xA405, SHORT if exif_short else LONG, 1) + value + b"\0\0\0\0"
        entries = {**entries, 34665: (LONG, [exif_at])}
    fields = []
    for tag in sorted(entries):
        typ, values = entries[tag]
        packed, count = _pack(order, typ, values)
        if len(packed) > 4:
            at = 8 + len(blob)
            blob += packed
            if len(blob) & 1:
                blob.append(0)
            packed = struct.pack(order + "I", at)
        fields.append(struct.pack(order + "HHI", tag, typ, count) + packed.ljust(4, b"\0"))
    ifd = 8 + len(blob)
    head = (b"II" if order == "<" else b"MM") + struct.pack(order + "HI", magic, ifd)
    return head + bytes(blob) + struct.pack(order + "H", len(fields)) + b"".join(fields) + b"\0\0\0\0"


def pillow(a, compression="raw", predictor=False, sem=None, strip_rows=None):
    """Pillow's (libtiff's) file of a: [h, w] / [h, w, 3 | 4] uint8, or [h, w] uint16."""
    from PIL import Image, TiffImagePlugin

    img = Image.fromarray(a if a.ndim == 2 or a.shape[2] > 1 else a[:, :, 0])
    info = TiffImagePlugin.ImageFileDirectory_v2()
    if predictor:
        info[317] = 2
    if sem is not None:
        info[34682] = sem
        info.tagtype[34682] = 2
    if strip_rows is not None:
        info[278] = strip_rows
    buf = io.BytesIO()
    img.save(buf, format="TIFF", compression=compression, tiffinfo=info)
    return buf.getvalue()


LZW_CLEAR_EVERY = (63, 64, 127, 128)   # the mid-stream Clears at lane 63 and at lane 0 of a batch
SEM_TEXT = "[Scan]\r\nPixelWidth=2.5e-9\r\nPixelHeight=5e-9\r\n[Stage]\r\nStageT=0\r\n[PrivateFei]\r\nDatabarHeight=5\r\n"


def _scenes():
    P = picture
    g8 = P(47, 33, seed=2)
    s = {
        "o_1x1_g8": lambda: write(P(1, 1, seed=3)),
        "o_1x1_rgb16_lzw_pred": lambda: write(P(1, 1, 3, 16, seed=3), ">", 5, 2),
        "o_3x5_g8_mm": lambda: write(P(5, 3, seed=4), ">", rps=2),
        "o_g8_rps1": lambda: write(g8, rps=1),
        "o_g8_rps7": lambda: write(g8, rps=7, data_at=9),
        "o_g8_rps47": lambda: write(g8, rps=47),
        "o_g8_rps_absent": lambda: write(g8),
        "o_g8_rps_large_long": lambda: write(g8, ">", rps=1 << 20, long_values=True, byte_counts=False),
        "o_70_strips_lzw": lambda: write(P(70, 5, seed=5), compression=5, rps=1),
        "o_70_strips_packbits": lambda: write(P(70, 5, seed=5, kind="flat"), ">", compression=32773, rps=1),
        "o_g16_ii": lambda: write(P(47, 33, 1, 16, seed=6), "<", rps=7),
        "o_g16_mm": lambda: write(P(47, 33, 1, 16, seed=6), ">", rps=7, data_at=11),
        "o_wiz_g8": lambda: write(g8, photometric=0, rps=7),
        "o_wiz_g16_lzw": lambda: write(P(47, 33, 1, 16, seed=7), "<", 5, photometric=0, rps=7),
        "o_rgb8": lambda: write(P(47, 33, 3, seed=8), rps=7),
        "o_rgb8_bps_once": lambda: write(P(5, 3, 3, seed=8), bps_once=True),
        "o_rgba8_mm_lzw": lambda: write(P(47, 33, 4, seed=9), ">", 5, rps=7),
        "o_rgb16_ii": lambda: write(P(47, 33, 3, 16, seed=10), "<", rps=7),
        "o_rgb16_mm_packbits": lambda: write(P(47, 33, 3, 16, seed=10), ">", 32773, rps=7),
        "o_rgb16_257_pred_lzw": lambda: write(P(3, 257, 3, 16, seed=11, kind="noise"), "<", 5, 2, rps=2),
        "o_pred_g8": lambda: write(P(47, 33, seed=12, kind="noise"), predictor=2, rps=7),
        "o_pred_g8_300_packbits": lambda: write(P(4, 300, seed=13, kind="noise"), ">", 32773, 2, rps=3),
        "o_pred_g16_mm_lzw": lambda: write(P(47, 33, 1, 16, seed=14), ">", 5, 2, rps=7),
        "o_pred_g16_ii": lambda: write(P(5, 600, 1, 16, seed=14, kind="noise"), "<", 1, 2, rps=2, data_at=9),
        "o_pred_rgb8_lzw": lambda: write(P(47, 33, 3, seed=15), "<", 5, 2, rps=7),
        "o_pred_rgba8_ii": lambda: write(P(5, 300, 4, seed=15, kind="noise"), "<", 1, 2),
        "o_out_of_order_lzw": lambda: write(g8, compression=5, rps=7, strip_order=[3, 0, 6, 1, 5, 2, 4], data_at=9),
        "o_out_of_order_raw_mm": lambda: write(P(47, 33, 1, 16, seed=6), ">", rps=7, strip_order=[6, 5, 4, 3, 2, 1, 0], data_at=13),
        "o_lzw_literals": lambda: write(g8, compression=5, encoder=functools.partial(lzw, literals=True, clear_every=200)),
        "o_lzw_flat": lambda: write(P(64, 64, kind="flat"), compression=5),
        "o_lzw_mid_clear": lambda: write(g8, compression=5, encoder=functools.partial(lzw, clear_every=100)),
        "o_lzw_two_clears": lambda: write(g8, compression=5, encoder=functools.partial(lzw, clear_every=70, clears=2)),
        "o_lzw_no_initial_clear": lambda: write(g8, compression=5, encoder=functools.partial(lzw, initial_clear=False)),
        "o_lzw_no_eoi": lambda: write(g8, compression=5, encoder=functools.partial(lzw, eoi=False)),
        "o_lzw_eoi_junk": lambda: write(g8, compression=5, encoder=functools.partial(lzw, junk=b"\xff\x00\xaa\x55\x80")),
        "o_lzw_12_bits": lambda: write(P(64, 128, seed=16, kind="noise"), compression=5, rps=32),
        "o_lzw_full_table": lambda: write(P(34, 128, seed=16, kind="noise"), compression=5, encoder=functools.partial(lzw, clear_every=None)),
        "o_pb_noop": lambda: write(g8, compression=32773, rps=7, encoder=functools.partial(packbits, noop_every=2)),
        "o_pb_128": lambda: write(np.concatenate([P(2, 300, kind="flat"), P(2, 300, seed=17, kind="noise")]), compression=32773, rps=2),
        "o_pb_crossing_rows": lambda: write(P(47, 33, kind="flat"), compression=32773, rps=7),
        "o_pb_cut": lambda: write(P(47, 33, kind="flat"), compression=32773, rps=7, encoder=functools.partial(packbits, overshoot=True)),
        # the seams of the 64-packet and 64-code batches (the c-th code since a Clear is lane c % 64 of its batch)
        "o_pb_batches": pb_batches,
        **{"o_lzw_clear_%d" % n: functools.partial(write, g8, compression=5, encoder=functools.partial(lzw, clear_every=n)) for n in LZW_CLEAR_EVERY},
        "o_lzw_two_clears_64": lambda: write(g8, compression=5, encoder=functools.partial(lzw, clear_every=64, clears=2)),
        "o_lzw_eoi_first_of_batch": lambda: _lzw_full_batches(True),
        "o_lzw_full_at_batch_end": lambda: _lzw_full_batches(False),
        "o_sem_exif": lambda: write(g8, rps=7, extra=[(34682, ASCII, SEM_TEXT.encode() + b"\0")], exif_focal=35),
        "o_exif_long_mm": lambda: write(g8, ">", rps=7, exif_focal=70000, exif_short=False),
        "p_g8_raw": lambda: pillow(g8[:, :, 0]),
        "p_g8_lzw": lambda: pillow(g8[:, :, 0], "tiff_lzw"),
        "p_g8_packbits": lambda: pillow(g8[:, :, 0], "packbits"),
        "p_g8_lzw_pred": lambda: pillow(g8[:, :, 0], "tiff_lzw", True),
        "p_g16_lzw": lambda: pillow(P(47, 33, 1, 16, seed=6)[:, :, 0], "tiff_lzw"),
        "p_g16_lzw_pred": lambda: pillow(P(47, 33, 1, 16, seed=6)[:, :, 0], "tiff_lzw", True),
        "p_rgb8_packbits": lambda: pillow(P(47, 33, 3, seed=8), "packbits"),
        "p_rgb8_lzw_pred": lambda: pillow(P(47, 33, 3, seed=8), "tiff_lzw", True),
        "p_rgba8_lzw": lambda: pillow(P(47, 33, 4, seed=9), "tiff_lzw"),
        "p_g8_strips": lambda: pillow(g8[:, :, 0], "tiff_lzw", strip_rows=7),
        "p_noise_600x500_lzw": lambda: pillow(P(500, 600, seed=18, kind="noise")[:, :, 0], "tiff_lzw"),
        "p_sem": lambda: pillow(g8[:, :, 0], "tiff_lzw", sem=SEM_TEXT),
    }
    return s


# Pillow does not read these as defined - it opens no 16-bit RGB, libtiff refuses a stream without the initial Clear, and
# neither honours Predictor 2 on uncompressed or PackBits strips -: they are compared with the picture they were written from
_SOURCES = {"o_1x1_rgb16_lzw_pred": lambda: picture(1, 1, 3, 16, seed=3), "o_rgb16_ii": lambda: picture(47, 33, 3, 16, seed=10),
            "o_rgb16_mm_packbits": lambda: picture(47, 33, 3, 16, seed=10),
            "o_rgb16_257_pred_lzw": lambda: picture(3, 257, 3, 16, seed=11, kind="noise"),
            "o_lzw_no_initial_clear": lambda: picture(47, 33, seed=2), "o_pred_g8": lambda: picture(47, 33, seed=12, kind="noise"),
            "o_pred_g8_300_packbits": lambda: picture(4, 300, seed=13, kind="noise"),
            "o_pred_g16_ii": lambda: picture(5, 600, 1, 16, seed=14, kind="noise"),
            "o_pred_rgba8_ii": lambda: picture(5, 300, 4, seed=15, kind="noise")}
NOT_FOR_PILLOW = tuple(sorted(_SOURCES))


def names():
    return sorted(_scenes())


@functools.lru_cache(maxsize=None)
def scene(name) -> bytes:
    return _scenes()[name]()


def source(name):
    """The picture a NOT_FOR_PILLOW scene was written from."""
    return _SOURCES[name]()


def patch_entry(data: bytes, tag: int, value: int) -> bytes:
    """The file with the value field of the first IFD's entry `tag` replaced (files of this writer in II order)."""
    ifd = struct.unpack_from("<I", data, 4)[0]
    for k in range(struct.unpack_from("<H", data, ifd)[0]):
        at = ifd + 2 + 12 * k
        if struct.unpack_from("<H", data, at)[0] == tag:
            return data[:at + 8] + struct.pack("<I", value) + data[at + 12:]
    raise KeyError(tag)


def _bad_lzw(kind):
    bits = _Bits()
    if kind == "above":
        for code in (256, 10, 11, 300):
            bits.code(code)
    elif kind == "first":
        for code in (256, 258, 10):
            bits.code(code)
    elif kind == "eoi":
        for code in (256, 10, 11, 257, 12, 13):
            bits.code(code)
    else:
        for code in (256, 10, 11):
            bits.code(code)
    return bits.done()


@functools.lru_cache(maxsize=None)
def refused():
    """{name: (file, code)}: one file per kind of refusal."""
    g = picture(6, 5, seed=20)
    rgb = picture(6, 5, 3, seed=21)
    ok = write(g, rps=2)
    out = {}

    def add(name, data, code):
        out[name] = (data, code)

    add("u_bigtiff", write(g, magic=43), UNSUPPORTED)
    add("u_tiles", write(g, extra=[(322, SHORT, [16]), (323, SHORT, [16]), (324, LONG, [8]), (325, LONG, [30])]), UNSUPPORTED)
    add("u_planar_2", write(rgb, extra=[(284, SHORT, [2])]), UNSUPPORTED)
    add("u_bits_4", write(g, override={258: (SHORT, [4])}), UNSUPPORTED)
    add("u_bits_32", write(g, override={258: (SHORT, [32])}), UNSUPPORTED)
    add("u_bits_differ", write(rgb, override={258: (SHORT, [8, 8, 16])}), UNSUPPORTED)
    add("u_bits_absent", write(g, override={258: None}), UNSUPPORTED)
    add("u_float", write(picture(6, 5, 1, 16, seed=20), extra=[(339, SHORT, [3])]), UNSUPPORTED)
    add("u_signed", write(g, extra=[(339, SHORT, [2])]), UNSUPPORTED)
    add("u_palette", write(g, photometric=3), UNSUPPORTED)
    add("u_cmyk", write(picture(6, 5, 4, seed=22), photometric=5), UNSUPPORTED)
    add("u_ycbcr", write(rgb, photometric=6), UNSUPPORTED)
    add("u_cielab", write(rgb, photometric=8), UNSUPPORTED)
    add("u_grey_rgb", write(g, photometric=2), UNSUPPORTED)
    add("u_2_samples", write(picture(6, 5, 2, seed=23), photometric=1), UNSUPPORTED)
    add("u_5_samples", write(picture(6, 5, 5, seed=23), photometric=2), UNSUPPORTED)
    for c in (2, 3, 4, 6, 7, 8, 32946, 50000):
        add(f"u_compression_{c}", write(g, override={259: (SHORT, [c])}), UNSUPPORTED)
    add("u_predictor_3", write(g, override={317: (SHORT, [3])}), UNSUPPORTED)
    add("u_fill_order_2", write(g, extra=[(266, SHORT, [2])]), UNSUPPORTED)
    add("u_width_65536", write(g, override={256: (LONG, [65536])}), UNSUPPORTED)
    add("u_strip_2_31", write(g, override={279: (LONG, [1 << 31])}), UNSUPPORTED)
    add("u_old_lzw", write(g, compression=5, encoder=lambda b: b"\x00\x01" + lzw(b)), UNSUPPORTED)
    add("i_truncated_header", ok[:7], INVALID)
    add("i_byte_order", b"XX" + ok[2:], INVALID)
    add("i_magic", write(g, magic=41), INVALID)
    add("i_truncated_ifd", ok[:-20], INVALID)
    add("i_ifd_past_file", ok[:4] + struct.pack("<I", len(ok) + 10) + ok[8:], INVALID)
    long_ok = write(g, rps=2, long_values=True)
    add("i_entry_past_file", patch_entry(long_ok, 273, len(long_ok) - 4), INVALID)
    add("i_strip_past_file", write(g, rps=2, override={273: (LONG, [8, 18, 100000])}), INVALID)
    add("i_width_0", write(g, override={256: (SHORT, [0])}), INVALID)
    add("i_height_0", write(g, override={257: (SHORT, [0])}), INVALID)
    add("i_no_width", write(g, override={256: None}), INVALID)
    add("i_no_photometric", write(g, override={262: None}), INVALID)
    add("i_no_offsets", write(g, override={273: None}), INVALID)
    add("i_offsets_count", write(g, rps=2, override={273: (LONG, [8, 18])}), INVALID)
    add("i_counts_count", write(g, rps=2, override={279: (LONG, [10, 10])}), INVALID)
    add("i_counts_missing_lzw", write(g, compression=5, byte_counts=False), INVALID)
    add("i_short_strip", write(g, rps=2, override={279: (LONG, [10, 9, 10])}), INVALID)
    add("i_rows_per_strip_0", write(g, override={278: (SHORT, [0])}), INVALID)
    add("i_width_type", write(g, override={256: (ASCII, b"5\0")}), INVALID)
    for kind in ("above", "first", "eoi", "short"):
        add(f"i_lzw_{kind}", write(g, compression=5, encoder=lambda b, kind=kind: _bad_lzw(kind)), INVALID)
    # libtiff's table has 5119 slots and goes on filling them past entry 4095; it refuses the code that finds none left
    add("i_lzw_table_overflow", write(picture(64, 128, seed=16, kind="noise"), compression=5, encoder=functools.partial(lzw, clear_every=None)), INVALID)
    add("i_pb_short", write(g, compression=32773, encoder=lambda b: packbits(b)[:-2]), INVALID)
    add("i_pb_literal_cut", write(g, compression=32773, encoder=lambda b: b"\x7f" + b[:20]), INVALID)
    return out


# (the text of the block, (scale width, scale height, tilt or None, databar height)); f32 values as Python floats of the f32
def _f(x):
    return float(np.float32(x))


SEM_BLOCKS = [
    ("plain", SEM_TEXT.encode(), (_f(2.5e-9), _f(5e-9), 0.0, 5)),
    ("nuls_inside", b"[Sc\0an]\nPixel\0Width=2\n[Private\0Fei]\nDatabarHeight=1\0002\n\0", (2.0, 1.0, None, 12)),
    ("not_utf8_piece", b"[Scan]\nPixelWidth=2\n\0\xff[Stage]\n\0PixelHeight=3\n", (2.0, 3.0, None, 0)),
    ("cr_lf_mix", b"[Scan]\rPixelWidth=3\r\n\nPixelHeight=4\n[Stage]\rStageT=52.5", (3.0, 4.0, 52.5, 0)),
    ("prefix_only", b"[Scan]\nPixelWidthX=7\nPixelHeight\n", (7.0, 1.0, None, 0)),
    ("first_fails_second_parses", b"[Scan]\nPixelWidth=abc\nPixelWidth=6\nPixelWidth=8\n", (6.0, 1.0, None, 0)),
    ("tilt_fails_after_one_parsed", b"[Stage]\nStageT=10\nStageT=ten\n", (1.0, 1.0, None, 0)),
    ("tilt_last_wins", b"[Stage]\nStageT=10\nStageT=-20.5\n", (1.0, 1.0, -20.5, 0)),
    ("leading_space", b"[Scan]\nPixelWidth= 1\nPixelHeight=1 \n[PrivateFei]\nDatabarHeight= 3\n", (1.0, 1.0, None, 0)),
    ("databar_plus", b"[PrivateFei]\nDatabarHeight=+3\n", (1.0, 1.0, None, 3)),
    ("databar_minus_zero", b"[PrivateFei]\nDatabarHeight=7\nDatabarHeight=-0\n", (1.0, 1.0, None, 7)),
    ("databar_overflow", b"[PrivateFei]\nDatabarHeight=4294967295\nDatabarHeight=4294967296\n", (1.0, 1.0, None, 4294967295)),
    ("small_inf_hex", b"[Scan]\nPixelWidth=1e-9\nPixelHeight=0x10\nPixelHeight=-INF\n[Stage]\nStageT=infinity\n", (_f(1e-9), float("-inf"), float("inf"), 0)),
    ("double_rounding", b"[Scan]\nPixelWidth=1.00000005960464477539062500000000000000000000001\n", (1.0000001192092896, 1.0, None, 0)),
    ("second_equals", b"[Scan]\nPixelWidth=1=2\nPixelWidth=.5e1\n[Stage]\nStageT=1.\n", (5.0, 1.0, 1.0, 0)),
    ("wrong_section", b"[Stage]\nPixelWidth=3\nDatabarHeight=4\n[Scan]x\nPixelWidth=9\n", (1.0, 1.0, None, 0)),
    ("section_must_close", b"[Scan\nPixelWidth=3\n[Scan]\nPixelHeight=4\n[]\nPixelWidth=5\n", (1.0, 4.0, None, 0)),
    ("subnormal_and_huge", b"[Scan]\nPixelWidth=1e-45\nPixelHeight=1e39\n", (_f(1e-45), float("inf"), None, 0)),
]


def sem_file(raw: bytes, tag=34682, typ=ASCII, second=None):
    """A small file with the block in `tag` (and `second`: (tag, type, bytes), another block)."""
    extra = [(tag, typ, raw)] + ([second] if second else [])
    return write(picture(20, 5, seed=24), extra=extra)
