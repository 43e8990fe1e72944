"""The JPEG files of the decoder's tests: (a) files that Pillow (libjpeg-turbo) encodes at test time, and
(b) files from `write`, a minimal baseline writer from coefficient arrays, tables, sampling and DRI, which forces what an
encoder does not give on demand.  tests/test_jpeg_ref.py checks that each forced file reaches its case."""
import functools
import io

import numpy as np

import ref_jpeg

SUBSEQ_BITS = 1024  # jpeg_common.hpp's SUBSEQ_BITS
SAMPLING = {"444": 0, "422": 1, "420": 2}


def _picture(w, h, kind, seed=0):
    rng = np.random.RandomState(1000 + seed)
    if kind == "noise":
        return rng.randint(0, 256, size=(h, w, 3)).astype(np.uint8)
    if kind == "flat":
        return np.full((h, w, 3), (200, 40, 90), dtype=np.uint8)
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    img = np.stack([127 + 120 * np.sin(x / 5.0 + seed), 127 + 120 * np.cos(y / 7.0), 255 * (x + y) / max(w + h - 2, 1)], axis=2)
    return np.clip(img + rng.randint(-6, 7, size=img.shape), 0, 255).astype(np.uint8)


def pillow_jpeg(pixels, grey=False, **options):
    from PIL import Image

    img = Image.fromarray(pixels[:, :, 1] if grey else pixels)
    buf = io.BytesIO()
    img.save(buf, format="JPEG", **options)
    return buf.getvalue()


def exif_bytes(focal, short=True, big_endian=False):
    """An `Exif\\0\\0`-less TIFF block: IFD0 with 0x8769 -> an IFD with 0xA405 as SHORT or LONG."""
    import struct

    e = ">" if big_endian else "<"
    value = struct.pack(e + "HH", focal, 0) if short else struct.pack(e + "I", focal)
    return ((b"MM" if big_endian else b"II") + struct.pack(e + "HI", 42, 8)
            + struct.pack(e + "HHHII", 1, 0x8769, 4, 1, 26) + struct.pack(e + "I", 0)
            + struct.pack(e + "HHHI", 1, 0xA405, 3 if short else 4, 1) + value + struct.pack(e + "I", 0))


# ---- (b) the writer ---------------------------------------------------------------------------------------------------------------
def table(lengths):
    """{symbol: code length} -> (counts[16], symbols) of a DHT segment, canonical."""
    order = sorted(lengths, key=lambda s: (lengths[s], s))
    return [sum(1 for s in order if lengths[s] == n) for n in range(1, 17)], order


def _codes(tab):
    counts, symbols = tab
    out, code, k = {}, 0, 0
    for bits in range(1, 17):
        for _ in range(counts[bits - 1]):
            out[symbols[k]] = (code, bits)
            code, k = code + 1, k + 1
        code <<= 1
    return out


DC_PLAIN = table({s: 4 for s in range(12)})
AC_PLAIN = table({0x00: 2, 0xF0: 3, **{r << 4 | s: 8 if r < 4 and s < 6 else 16 for r in range(16) for s in range(1, 11)}})
DC_LONG = table({0: 1, **{s: 16 for s in range(1, 12)}})
AC_LONG = table({0x00: 2, 0xF0: 3, **{r << 4 | s: 16 for r in range(16) for s in range(1, 11)}})


def write(width, height, coef, quant, sampling=(1, 1), restart=0, dc=DC_PLAIN, ac=AC_PLAIN, dqt16=False, fill=0, components=3,
          sof=0xC0, precision=8, chroma_sampling=(1, 1), adobe=None, dnl=False, extra_scan=False, app=()):
    """coef [blocks, 64] in natural order, blocks in scan order with DC VALUES (the writer takes the differences); quant
    [64] natural order, for every component; fill: FF bytes put in front of every RSTn and EOI."""
    def seg(marker, body):
        return bytes([0xFF, marker]) + (len(body) + 2).to_bytes(2, "big") + bytes(body)

    out = bytearray(b"\xff\xd8")
    for body in app:
        out += seg(body[0], body[1])
    if adobe is not None:
        out += seg(0xEE, b"Adobe" + bytes([0, 100, 0, 0, 0, 0, adobe]))
    zz = [quant[ref_jpeg.ZIGZAG[i]] for i in range(64)]
    out += seg(0xDB, bytes([0x10]) + b"".join(v.to_bytes(2, "big") for v in zz) if dqt16 else bytes([0x00] + zz))
    hs, vs = sampling
    frame = [precision] + list(height.to_bytes(2, "big")) + list(width.to_bytes(2, "big")) + [components]
    for c in range(components):
        ch, cv = (hs, vs) if c == 0 else chroma_sampling
        frame += [c + 1, ch << 4 | cv, 0]
    out += seg(sof, frame)
    for cls, tab in ((0, dc), (1, ac)):
        out += seg(0xC4, [cls << 4] + tab[0] + tab[1])
    if restart:
        out += seg(0xDD, restart.to_bytes(2, "big"))
    out += seg(0xDA, [components] + [v for c in range(components) for v in (c + 1, 0)] + [0, 63, 0])
    slots = [0] * (hs * vs) + [c for c in range(1, components) for _ in range(chroma_sampling[0] * chroma_sampling[1])]
    bpm = len(slots)
    dcc, acc = _codes(dc), _codes(ac)
    acc_bits, acc_n, rst = 0, 0, 0
    scan = bytearray()

    def put(value, n):
        nonlocal acc_bits, acc_n
        acc_bits, acc_n = acc_bits << n | value, acc_n + n
        while acc_n >= 8:
            b = (acc_bits >> (acc_n - 8)) & 0xFF
            scan.append(b)
            if b == 0xFF:
                scan.append(0)
            acc_n -= 8
        acc_bits &= (1 << acc_n) - 1

    def magnitude(v):
        size = int(abs(v)).bit_length()
        return size, (v if v >= 0 else v + (1 << size) - 1)

    pred = [0] * components
    for b in range(len(coef)):
        if restart and b and b % (restart * bpm) == 0:
            if acc_n:
                put((1 << (8 - acc_n)) - 1, 8 - acc_n)
            scan.extend(b"\xff" * fill + bytes([0xFF, 0xD0 + (rst & 7)]))
            rst += 1
            pred = [0] * components
        c = slots[b % bpm]
        row = [int(v) for v in coef[b]]
        size, bits = magnitude(row[0] - pred[c])
        pred[c] = row[0]
        put(*dcc[size])
        put(bits, size)
        run = 0
        for k in range(1, 64):
            v = row[ref_jpeg.ZIGZAG[k]]
            if v == 0:
                run += 1
                continue
            while run > 15:
                put(*acc[0xF0])
                run -= 16
            size, bits = magnitude(v)
            put(*acc[run << 4 | size])
            put(bits, size)
            run = 0
        if run:
            put(*acc[0x00])
    if acc_n:
        put((1 << (8 - acc_n)) - 1, 8 - acc_n)
    out += scan
    if dnl:
        out += seg(0xDC, height.to_bytes(2, "big"))
    if extra_scan:
        out += seg(0xDA, [1, 1, 0, 0, 63, 0]) + b"\x00"
    out += b"\xff" * fill + b"\xff\xd9"
    return bytes(out)


def _blocks(width, height, sampling, components=3):
    mx, my = -(-width // (8 * sampling[0])), -(-height // (8 * sampling[1]))
    return mx * my * (sampling[0] * sampling[1] + components - 1)


def _small_coef(n, seed):
    rng = np.random.RandomState(seed)
    coef = np.zeros((n, 64), dtype=np.int64)
    coef[:, 0] = rng.randint(-60, 60, size=n)
    for b in range(n):
        k = rng.randint(0, 12)
        coef[b, rng.choice(np.arange(1, 64), size=k, replace=False)] = rng.randint(-5, 6, size=k)
    return coef


QUANT_PLAIN = [8 + (i % 8) + (i // 8) for i in range(64)]


def forced_codes16():
    """17 x 9 at 4:2:0 (one MCU row of two MCUs): 16-bit codes, a 16-bit DQT with an entry above 255, ZRL chains, an
    EOB-less block, and a block of 63 coefficients of category 10 - about 1.6 kbit, longer than a subsequence."""
    n = _blocks(17, 9, (2, 2))
    coef = _small_coef(n, 5)
    coef[1, :] = 0
    coef[1, 0], coef[1, ref_jpeg.ZIGZAG[40]], coef[1, ref_jpeg.ZIGZAG[63]] = 7, 3, -2   # ZRL ZRL, then ZRL, and no EOB
    rng = np.random.RandomState(6)
    coef[3, 1:] = rng.choice([-1, 1], size=63) * rng.randint(512, 1024, size=63)         # category 10 throughout
    coef[3, 0] = -1000
    coef[7, :] = 0                                                                       # DC alone
    quant = list(QUANT_PLAIN)
    quant[63] = 300
    return write(17, 9, coef, quant, sampling=(2, 2), dc=DC_LONG, ac=AC_LONG, dqt16=True)


def forced_restart():
    """40 x 40 at 4:4:4 (25 MCUs), DRI 2: thirteen intervals (RST7 -> RST0), the last of one MCU; FF FF fill in front of
    every marker; coefficients in an encoder's range, so Pillow opens it to the same pixels."""
    return write(40, 40, _small_coef(_blocks(40, 40, (1, 1)), 7), QUANT_PLAIN, restart=2, fill=2)


def forced_plain422():
    return write(21, 10, _small_coef(_blocks(21, 10, (2, 1)), 8), QUANT_PLAIN, sampling=(2, 1), restart=1)


def forced_grey():
    return write(9, 17, _small_coef(_blocks(9, 17, (1, 1), 1), 9), QUANT_PLAIN, components=1, dc=DC_LONG)


FORCED = {"w_codes16": forced_codes16, "w_restart": forced_restart, "w_plain422": forced_plain422, "w_grey": forced_grey}
FORCED_IN_ENCODER_RANGE = ("w_restart", "w_plain422", "w_grey", "w_fill_straddles")


def _ff00_at_chunk_end(seed):
    """A noise file with an FF 00 pair whose FF is the last byte of a 256-byte piece of the scan (pieces counted from the
    scan's first byte: the segment kernel's blocks), so the pair straddles two blocks and two waves."""
    data = pillow_jpeg(_picture(160, 160, "noise", seed), quality=95, subsampling=0)
    s0, s1 = ref_jpeg.parse(data)["scan"]
    return data, any(data[i] == 0xFF and data[i + 1] == 0 for i in range(s0 + 255, s1 - 1, 256))


def noise160():
    for seed in range(64):
        data, ok = _ff00_at_chunk_end(seed)
        if ok:
            return data
    raise AssertionError("no seed puts an FF 00 pair across a piece boundary")


# ---- the seams of the kernels' units: 256 subsequences a workgroup of the sync kernel, 64 and 256 bytes of the scan a wave
# and a workgroup of the byte kernels -------------------------------------------------------------------------------------
SYNC_LANES, WAVE_BYTES, GROUP_BYTES = 256, 64, 256


def seams(data):
    """Where a file's restart intervals and markers lie relative to those units.  sub_first[s]: the number of interval s's
    first subsequence; spanning: the intervals whose subsequences lie in two workgroups; lane0: those that begin at lane 0 of
    a workgroup behind the first; straddles[unit]: per RSTn whose bytes or FF fill lie on both sides of a unit's edge, the
    bytes of the run FF .. FF Dn in front of the edge."""
    h = ref_jpeg.parse(data)
    subs = [max(1, -(-8 * len(seg) // SUBSEQ_BITS)) for seg in ref_jpeg.segments(h)]
    first = [0]
    for n in subs:
        first.append(first[-1] + n)
    s0, s1 = h["scan"]
    scan = data[s0:s1]
    straddles = {WAVE_BYTES: [], GROUP_BYTES: []}
    for i in range(1, len(scan)):
        if scan[i - 1] == 0xFF and 0xD0 <= scan[i] <= 0xD7:
            start = i - 1
            while start and scan[start - 1] == 0xFF:
                start -= 1
            for unit, met in straddles.items():
                met += [(i - start - k, i - start + 1) for k in range(i - start) if (i - k) % unit == 0]   # (bytes in front, bytes of the run)
    return {"intervals": len(subs), "subsequences": first[-1], "sub_first": first,
            "spanning": [s for s in range(len(subs)) if first[s] // SYNC_LANES != (first[s + 1] - 1) // SYNC_LANES],
            "lane0": [s for s in range(1, len(subs)) if first[s] % SYNC_LANES == 0], "straddles": straddles}


def restart_noise(size, more_than=SYNC_LANES, want="spanning", markers=False, grey=False, **options):
    """Pillow's file of size x size noise with restart intervals, more subsequences than `more_than`, an interval that spans
    two workgroups of the sync kernel (or begins at lane 0 of a later one) and, with markers, an RSTn whose FF is the last
    byte of a 64-byte piece of the scan and another whose FF is the last of a 256-byte piece: the first seed that gives them."""
    for seed in range(64):
        data = pillow_jpeg(_picture(size, size, "noise", seed), grey=grey, **options)
        at = seams(data)
        split = {unit: [s for s in at["straddles"][unit] if s[0] == 1] for unit in (WAVE_BYTES, GROUP_BYTES)}   # FF | Dn
        if markers and not (split[GROUP_BYTES] and len(split[WAVE_BYTES]) > len(split[GROUP_BYTES])):
            continue
        if at[want]:
            assert at["subsequences"] > more_than and ref_jpeg.parse(data)["restart"] == options["restart_marker_blocks"]
            return data
    raise AssertionError("no seed gives the seams")


def forced_fill_straddles():
    """160 x 160 at 4:4:4, DRI 1 (400 intervals), FF FF fill in front of every marker: at the 64-byte and at the 256-byte
    edges some marker has one fill byte, both fill bytes, and both with its own FF in front of the edge."""
    n = _blocks(160, 160, (1, 1))
    for seed in range(64):
        data = write(160, 160, _small_coef(n, 100 + seed), QUANT_PLAIN, restart=1, fill=2)
        at = seams(data)["straddles"]
        if all({s for s in at[unit] if s[1] == 4} >= {(1, 4), (2, 4), (3, 4)} for unit in (WAVE_BYTES, GROUP_BYTES)):
            return data
    raise AssertionError("no seed puts the fill and the markers across the edges")


def _dc_ramp(width, height, restart):
    """4:4:4; the luma DC values climb by about 1 900 a block and the Cb values fall as fast (the largest difference a
    baseline file can hold is 2 047), so within 18 MCUs of an interval's start the sums leave the int16 range: the
    definition wraps them (and the coefficients are far outside an encoder's range: Pillow is no witness here)."""
    n = _blocks(width, height, (1, 1))
    coef = _small_coef(n, 11)
    rng = np.random.RandomState(12)
    per = restart or n // 3
    for m in range(n // 3):
        k = m % per + 1
        coef[3 * m, 0] = 1900 * k + rng.randint(-40, 40)
        coef[3 * m + 1, 0] = -1900 * k + rng.randint(-40, 40)
    return write(width, height, coef, QUANT_PLAIN, restart=restart)


FORCED.update({"w_dc_wrap": lambda: _dc_ramp(48, 48, 0), "w_dc_wrap_rst": lambda: _dc_ramp(48, 48, 20), "w_fill_straddles": forced_fill_straddles})
# name: (size, options of restart_noise): the files with restart intervals over several workgroups of the sync kernel
RESTART = {
    "e_rst7_120_444": (120, dict(quality=95, subsampling=0, restart_marker_blocks=7)),
    "e_rst1_120_444": (120, dict(quality=95, subsampling=0, restart_marker_blocks=1, want="lane0", markers=True)),
    "e_rst5_128_422": (128, dict(quality=100, subsampling=1, restart_marker_blocks=5)),
    "e_rst3_160_grey": (160, dict(quality=100, grey=True, restart_marker_blocks=3)),
    "e_rst3_176_420": (176, dict(quality=100, subsampling=2, restart_marker_blocks=3)),
    "e_rst5_200_444": (200, dict(quality=95, subsampling=0, restart_marker_blocks=5, more_than=2 * SYNC_LANES)),
}

ENCODED = {
    **{name: functools.partial(restart_noise, size, **options) for name, (size, options) in RESTART.items()},
    "e_1x1_420": lambda: pillow_jpeg(_picture(1, 1, "smooth"), quality=90, subsampling=2),
    "e_3x5_420": lambda: pillow_jpeg(_picture(3, 5, "noise"), quality=90, subsampling=2),
    "e_4x4_420": lambda: pillow_jpeg(_picture(4, 4, "noise"), quality=95, subsampling=2),
    "e_5x3_422": lambda: pillow_jpeg(_picture(5, 3, "noise"), quality=95, subsampling=1),
    "e_4x3_422": lambda: pillow_jpeg(_picture(4, 3, "noise", 2), quality=95, subsampling=1),
    "e_8x8_444": lambda: pillow_jpeg(_picture(8, 8, "smooth"), quality=50, subsampling=0),
    "e_17x9_444": lambda: pillow_jpeg(_picture(17, 9, "noise"), quality=100, subsampling=0),
    "e_17x9_422": lambda: pillow_jpeg(_picture(17, 9, "smooth"), quality=95, subsampling=1, optimize=True),
    "e_17x9_420": lambda: pillow_jpeg(_picture(17, 9, "noise"), quality=50, subsampling=2),
    "e_33x47_420_rst1": lambda: pillow_jpeg(_picture(33, 47, "smooth"), quality=95, subsampling=2, restart_marker_blocks=1),
    "e_33x47_422_rst3": lambda: pillow_jpeg(_picture(33, 47, "noise"), quality=100, subsampling=1, restart_marker_blocks=3, optimize=True),
    "e_33x47_444_rstrow": lambda: pillow_jpeg(_picture(33, 47, "smooth", 1), quality=50, subsampling=0, restart_marker_rows=1),
    "e_17x9_grey": lambda: pillow_jpeg(_picture(17, 9, "noise"), grey=True, quality=95),
    "e_33x47_grey_rst3": lambda: pillow_jpeg(_picture(33, 47, "smooth"), grey=True, quality=50, restart_marker_blocks=3, optimize=True),
    "e_exif": lambda: pillow_jpeg(_picture(24, 16, "smooth"), quality=90, subsampling=2, exif=b"Exif\0\0" + exif_bytes(28)),
    "e_noise160_444": noise160,
    "e_flat256_420": lambda: pillow_jpeg(_picture(256, 256, "flat"), quality=90, subsampling=2),
}
FOCAL = {"e_exif": 28}


def names():
    return sorted(ENCODED) + sorted(FORCED)


@functools.lru_cache(maxsize=None)
def scene(name):
    return (ENCODED.get(name) or FORCED[name])()


@functools.lru_cache(maxsize=None)
def restated(name):
    """The file's pixels by tests/ref_jpeg.py: {"rgb", "luma", "met"}; computed once and left unchanged."""
    met = {}
    rgb = ref_jpeg.decode(scene(name), ref_jpeg.RGB8, met=met)
    luma = ref_jpeg.decode(scene(name), ref_jpeg.LUMA8)
    rgb.setflags(write=False)
    luma.setflags(write=False)
    return {"rgb": rgb, "luma": luma, "met": met}


def refused():
    """name -> (file, code): every kind of file that is refused."""
    from PIL import Image

    U, I = ref_jpeg.UNSUPPORTED, ref_jpeg.INVALID
    pic = _picture(17, 9, "smooth")
    good = scene("e_17x9_420")
    n6 = _blocks(17, 9, (2, 2))
    coef = _small_coef(n6, 3)
    out = {
        "progressive": (pillow_jpeg(pic, quality=90, progressive=True), U),
        "sof1_extended": (write(17, 9, coef, QUANT_PLAIN, sampling=(2, 2), sof=0xC1), U),
        "sof3_lossless": (write(17, 9, coef, QUANT_PLAIN, sampling=(2, 2), sof=0xC3), U),
        "sof9_arithmetic": (write(17, 9, coef, QUANT_PLAIN, sampling=(2, 2), sof=0xC9), U),
        "twelve_bit": (write(17, 9, coef, QUANT_PLAIN, sampling=(2, 2), precision=12), U),
        "two_components": (write(17, 9, _small_coef(_blocks(17, 9, (1, 1), 2), 3), QUANT_PLAIN, components=2), U),
        "adobe_rgb": (write(17, 9, coef, QUANT_PLAIN, sampling=(2, 2), adobe=0), U),
        "two_scans": (write(17, 9, coef, QUANT_PLAIN, sampling=(2, 2), extra_scan=True), U),
        "h1v2": (write(17, 9, _small_coef(_blocks(17, 9, (1, 2)), 3), QUANT_PLAIN, sampling=(1, 2)), U),
        "chroma_2x1": (write(17, 9, coef, QUANT_PLAIN, sampling=(2, 2), chroma_sampling=(2, 1)), U),
        "dnl": (write(17, 9, coef, QUANT_PLAIN, sampling=(2, 2), dnl=True), U),
    }
    buf = io.BytesIO()
    Image.fromarray(np.dstack([pic, pic[:, :, :1]])).convert("CMYK").save(buf, format="JPEG")
    out["four_components"] = (buf.getvalue(), U)
    s0, s1 = ref_jpeg.parse(good)["scan"]
    dht = good.index(b"\xff\xc4")
    sof = good.index(b"\xff\xc0")
    out["truncated_header"] = (good[:sof + 6], I)
    out["truncated_scan"] = (good[:s0 + (s1 - s0) // 2], I)
    out["scan_cut_at_eoi"] = (good[:s0 + (s1 - s0) // 2] + b"\xff\xd9", I)
    out["no_huffman_table"] = (good[:dht] + good[dht + 2 + int.from_bytes(good[dht + 2:dht + 4], "big"):], I)
    out["width_0"] = (good[:sof + 7] + b"\0\0" + good[sof + 9:], I)
    out["height_0"] = (good[:sof + 5] + b"\0\0" + good[sof + 7:], U)   # (the height would come by DNL)
    out["empty"] = (b"", I)
    out["not_a_jpeg"] = (b"\x89PNG\r\n\x1a\n" + bytes(64), I)
    rst = scene("e_33x47_420_rst1")
    k = rst.index(b"\xff\xd1", ref_jpeg.parse(rst)["scan"][0])
    out["misnumbered_rst"] = (rst[:k + 1] + b"\xd3" + rst[k + 2:], I)
    out["missing_rst"] = (rst[:k] + rst[k + 2:], I)
    # a code that is in no table: DC_LONG has no code of all ones, the scan begins with sixteen of them
    bad = bytearray(write(8, 8, _small_coef(3, 2), QUANT_PLAIN, dc=DC_LONG))
    b0 = ref_jpeg.parse(bytes(bad))["scan"][0]
    bad[b0:b0 + 2] = b"\xff\x00"
    out["unknown_code"] = (bytes(bad[:b0 + 2]) + b"\xff\x00" + bytes(bad[b0 + 2:]), I)
    # a run past coefficient 63: a block whose AC symbols are (15, 1) five times
    run = np.zeros((3, 64), dtype=np.int64)
    codes = _codes(AC_PLAIN)
    bits = "".join(format(c, "0%db" % n) for c, n in [_codes(DC_PLAIN)[0]] + [codes[0xF1], (1, 1)] * 5)
    bits += "1" * (-len(bits) % 8)
    base = write(8, 8, run, QUANT_PLAIN)
    r0, r1 = ref_jpeg.parse(base)["scan"]
    out["run_past_63"] = (base[:r0] + bytes(int(bits[i:i + 8], 2) for i in range(0, len(bits), 8)).replace(b"\xff", b"\xff\x00") + base[r1:], I)
    return out
