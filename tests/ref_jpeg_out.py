"""The JPEG file of cvhip_jpeg_encode restated in Python: the file is libjpeg's - what
PIL.Image.save(format="JPEG", quality=q, subsampling=s, optimize=o) writes where Pillow is built on libjpeg(-turbo) -
baseline, one interleaved scan, no restart markers (tests/test_jpeg_out_ref.py holds it against Pillow byte for byte).

Defined here, where libjpeg gives nothing to follow:
  * the alpha of 2- and 4-channel pixels is dropped (Pillow refuses such input): the file is that of the grey or RGB part;
  * optimal_table takes counts of any size (libjpeg ignores a count above 10^9) and folds code lengths of any depth down to
    16 by the Annex K.3 step (libjpeg refuses a depth above 32); for what libjpeg accepts the tables are libjpeg's.
"""
from __future__ import annotations

import numpy as np

S444, S422, S420 = 0, 1, 2  # Pillow's subsampling numbers (CVHIP_JPEG_SAMPLING_*)
STUFF_TILE = 1024           # bytes of the unstuffed stream that one workgroup of the stuffing pass copies (counters only)

ZIGZAG = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21,
                   28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61,
                   54, 47, 55, 62, 63])

# ---- ITU-T T.81 Annex K: the example quantisation tables (natural order) and Huffman tables ---------------------------------------
QUANT_LUMA = np.array([16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51,
                       87, 80, 62, 18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120,
                       101, 72, 92, 95, 98, 112, 100, 103, 99])
QUANT_CHROMA = np.array([17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99,
                         99, 99, 99, 99] + [99] * 32)
DC_LUMA = ([0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0], list(range(12)))
DC_CHROMA = ([0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0], list(range(12)))
AC_LUMA = ([0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7D],
           [0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32,
            0x81, 0x91, 0xA1, 0x08, 0x23, 0x42, 0xB1, 0xC1, 0x15, 0x52, 0xD1, 0xF0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0A, 0x16,
            0x17, 0x18, 0x19, 0x1A, 0x25, 0x26, 0x27, 0x28, 0x29, 0x2A, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3A, 0x43, 0x44, 0x45,
            0x46, 0x47, 0x48, 0x49, 0x4A, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5A, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69,
            0x6A, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7A, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8A, 0x92, 0x93, 0x94,
            0x95, 0x96, 0x97, 0x98, 0x99, 0x9A, 0xA2, 0xA3, 0xA4, 0xA5, 0xA6, 0xA7, 0xA8, 0xA9, 0xAA, 0xB2, 0xB3, 0xB4, 0xB5, 0xB6,
            0xB7, 0xB8, 0xB9, 0xBA, 0xC2, 0xC3, 0xC4, 0xC5, 0xC6, 0xC7, 0xC8, 0xC9, 0xCA, 0xD2, 0xD3, 0xD4, 0xD5, 0xD6, 0xD7, 0xD8,
            0xD9, 0xDA, 0xE1, 0xE2, 0xE3, 0xE4, 0xE5, 0xE6, 0xE7, 0xE8, 0xE9, 0xEA, 0xF1, 0xF2, 0xF3, 0xF4, 0xF5, 0xF6, 0xF7, 0xF8,
            0xF9, 0xFA])
AC_CHROMA = ([0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77],
             [0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81,
              0x08, 0x14, 0x42, 0x91, 0xA1, 0xB1, 0xC1, 0x09, 0x23, 0x33, 0x52, 0xF0, 0x15, 0x62, 0x72, 0xD1, 0x0A, 0x16, 0x24, 0x34,
              0xE1, 0x25, 0xF1, 0x17, 0x18, 0x19, 0x1A, 0x26, 0x27, 0x28, 0x29, 0x2A, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3A, 0x43, 0x44,
              0x45, 0x46, 0x47, 0x48, 0x49, 0x4A, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5A, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68,
              0x69, 0x6A, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7A, 0x82, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8A, 0x92,
              0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9A, 0xA2, 0xA3, 0xA4, 0xA5, 0xA6, 0xA7, 0xA8, 0xA9, 0xAA, 0xB2, 0xB3, 0xB4,
              0xB5, 0xB6, 0xB7, 0xB8, 0xB9, 0xBA, 0xC2, 0xC3, 0xC4, 0xC5, 0xC6, 0xC7, 0xC8, 0xC9, 0xCA, 0xD2, 0xD3, 0xD4, 0xD5, 0xD6,
              0xD7, 0xD8, 0xD9, 0xDA, 0xE2, 0xE3, 0xE4, 0xE5, 0xE6, 0xE7, 0xE8, 0xE9, 0xEA, 0xF2, 0xF3, 0xF4, 0xF5, 0xF6, 0xF7, 0xF8,
              0xF9, 0xFA])
STANDARD_TABLES = (DC_LUMA, AC_LUMA, DC_CHROMA, AC_CHROMA)  # the order of the DHT segments: DC0, AC0, DC1, AC1


def quant_table(base, quality: int):
    """jpeg_set_quality with force_baseline: the table in natural order"""
    scale = 5000 // quality if quality < 50 else 200 - 2 * quality
    return np.clip((np.asarray(base, dtype=np.int64) * scale + 50) // 100, 1, 255)


# ---- the planes -----------------------------------------------------------------------------------------------------------------------
def ycc(rgb):
    """jccolor's rgb_ycc_convert"""
    r, g, b = (rgb[..., k].astype(np.int64) for k in range(3))
    y = (19595 * r + 38470 * g + 7471 * b + 32768) >> 16
    cb = (-11059 * r - 21709 * g + 32768 * b + (128 << 16) + 32767) >> 16
    cr = (32768 * r - 27439 * g - 5329 * b + (128 << 16) + 32767) >> 16
    return y, cb, cr


def pad(plane, rows: int, cols: int):
    """the last row and the last column replicated out to rows x cols"""
    return np.pad(plane, ((0, rows - plane.shape[0]), (0, cols - plane.shape[1])), mode="edge")


def component_plane(plane, hf: int, vf: int, blocks_x: int, blocks_y: int, rows_mcu: int):
    """One component's samples, blocks_y * 8 rows of blocks_x * 8, from the full-size plane: the SOURCE rows replicated to the
    right out to blocks_x * 8 * hf samples and at the bottom to a multiple of vf only; downsampled by hf x vf (jcsample's
    h2v1 / h2v2 with their alternating bias); then the DOWNSAMPLED rows replicated down to the MCU row (rows_mcu rows)."""
    src = pad(plane, -(-plane.shape[0] // vf) * vf, blocks_x * 8 * hf)
    if (hf, vf) == (1, 1):
        out = src
    elif (hf, vf) == (2, 1):
        bias = np.arange(src.shape[1] // 2) & 1  # 0, 1, 0, 1, ...
        out = (src[:, 0::2] + src[:, 1::2] + bias) >> 1
    else:
        bias = 1 + (np.arange(src.shape[1] // 2) & 1)  # 1, 2, 1, 2, ...
        out = (src[0::2, 0::2] + src[0::2, 1::2] + src[1::2, 0::2] + src[1::2, 1::2] + bias) >> 2
    return pad(out, max(rows_mcu, out.shape[0]), out.shape[1])[:blocks_y * 8]


# ---- jfdctint: the slow integer DCT ------------------------------------------------------------------------------------------------------
CONST_BITS, PASS1_BITS = 13, 2
F_0_298, F_0_390, F_0_541, F_0_765, F_0_899, F_1_175 = 2446, 3196, 4433, 6270, 7373, 9633
F_1_501, F_1_847, F_1_961, F_2_053, F_2_562, F_3_072 = 12299, 15137, 16069, 16819, 20995, 25172


def _descale(x, n):
    return (x + (1 << (n - 1))) >> n


def _pass(d, first: bool):
    """one pass over the last axis of d [..., 8]"""
    t0, t7, t1, t6 = d[..., 0] + d[..., 7], d[..., 0] - d[..., 7], d[..., 1] + d[..., 6], d[..., 1] - d[..., 6]
    t2, t5, t3, t4 = d[..., 2] + d[..., 5], d[..., 2] - d[..., 5], d[..., 3] + d[..., 4], d[..., 3] - d[..., 4]
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    out = np.zeros_like(d)
    n = CONST_BITS - PASS1_BITS if first else CONST_BITS + PASS1_BITS
    if first:
        out[..., 0], out[..., 4] = (t10 + t11) << PASS1_BITS, (t10 - t11) << PASS1_BITS
    else:
        out[..., 0], out[..., 4] = _descale(t10 + t11, PASS1_BITS), _descale(t10 - t11, PASS1_BITS)
    z1 = (t12 + t13) * F_0_541
    out[..., 2] = _descale(z1 + t13 * F_0_765, n)
    out[..., 6] = _descale(z1 - t12 * F_1_847, n)
    z1, z2, z3, z4 = t4 + t7, t5 + t6, t4 + t6, t5 + t7
    z5 = (z3 + z4) * F_1_175
    t4, t5, t6, t7 = t4 * F_0_298, t5 * F_2_053, t6 * F_3_072, t7 * F_1_501
    z1, z2, z3, z4 = -z1 * F_0_899, -z2 * F_2_562, -z3 * F_1_961 + z5, -z4 * F_0_390 + z5
    out[..., 7], out[..., 5] = _descale(t4 + z1 + z3, n), _descale(t5 + z2 + z4, n)
    out[..., 3], out[..., 1] = _descale(t6 + z2 + z3, n), _descale(t7 + z1 + z4, n)
    return out


def fdct_quantise(blocks, quant):
    """blocks [n, 8, 8] of samples, quant [64] natural -> [n, 64] coefficients in zigzag order"""
    d = _pass(blocks.astype(np.int64) - 128, True)                        # the rows
    d = _pass(d.transpose(0, 2, 1), False).transpose(0, 2, 1).reshape(-1, 64)  # the columns
    q8 = np.asarray(quant, dtype=np.int64) * 8
    mag = (np.abs(d) + (q8 >> 1)) // q8
    return (np.sign(d) * mag)[:, ZIGZAG]


# ---- Huffman tables --------------------------------------------------------------------------------------------------------------------
def optimal_lengths_unfolded(freq):
    """jpeg_gen_optimal_table up to its code sizes: freq [256] -> codesize [257] (the 257th symbol keeps the all-ones code free)"""
    freq = [int(f) for f in freq] + [1]
    codesize, others = [0] * 257, [-1] * 257
    while True:
        c1, v = -1, None
        for i in range(257):  # the least non-zero count; of equal counts the LARGEST symbol
            if freq[i] and (v is None or freq[i] <= v):
                v, c1 = freq[i], i
        c2, v = -1, None
        for i in range(257):
            if freq[i] and i != c1 and (v is None or freq[i] <= v):
                v, c2 = freq[i], i
        if c2 < 0:
            return codesize
        freq[c1] += freq[c2]
        freq[c2] = 0
        codesize[c1] += 1
        while others[c1] >= 0:
            c1 = others[c1]
            codesize[c1] += 1
        others[c1] = c2
        codesize[c2] += 1
        while others[c2] >= 0:
            c2 = others[c2]
            codesize[c2] += 1


def optimal_table(freq):
    """jpeg_gen_optimal_table: freq [256] -> (bits [16], values)"""
    codesize = optimal_lengths_unfolded(freq)
    top = max(max(codesize), 16)
    bits = [0] * (top + 1)
    for n in codesize:
        if n:
            bits[n] += 1
    for i in range(top, 16, -1):  # Annex K.3: no code longer than 16
        while bits[i] > 0:
            j = i - 2
            while bits[j] == 0:
                j -= 1
            bits[i] -= 2
            bits[i - 1] += 1
            bits[j + 1] += 2
            bits[j] -= 1
    i = 16
    while i and bits[i] == 0:
        i -= 1
    if i:
        bits[i] -= 1  # the 257th symbol's code (no counts at all: an empty table)
    values = [s for n in range(1, top + 1) for s in range(256) if codesize[s] == n]
    return bits[1:17], values


def code_table(bits, values):
    """symbol -> (code, length) of a table: the canonical codes of Annex C"""
    table, code, k = {}, 0, 0
    for n in range(1, 17):
        for _ in range(bits[n - 1]):
            table[values[k]] = (code, n)
            code, k = code + 1, k + 1
        code <<= 1
    return table


# ---- the entropy coder ------------------------------------------------------------------------------------------------------------------
def block_symbols(coef, pred: int):
    """One block's symbols: [(is_ac, symbol, value bits, their count)], coef in zigzag order"""
    out = []
    diff = int(coef[0]) - pred
    n = abs(diff).bit_length()
    out.append((0, n, (diff if diff >= 0 else diff - 1) & ((1 << n) - 1), n))
    run = 0
    for k in range(1, 64):
        v = int(coef[k])
        if v == 0:
            run += 1
            continue
        while run > 15:
            out.append((1, 0xF0, 0, 0))
            run -= 16
        n = abs(v).bit_length()
        out.append((1, run << 4 | n, (v if v >= 0 else v - 1) & ((1 << n) - 1), n))
        run = 0
    if run:
        out.append((1, 0x00, 0, 0))
    return out


def geometry(width: int, height: int, components: int, sampling: int):
    hs, vs = ((1, 1), (2, 1), (2, 2))[sampling] if components == 3 else (1, 1)
    g = {"hs": hs, "vs": vs, "mcus_x": -(-width // (8 * hs)), "mcus_y": -(-height // (8 * vs)),
         "blocks_x": -(-width // 8), "blocks_y": -(-height // 8), "blocks_per_mcu": hs * vs + 2 if components == 3 else 1}
    return g


def header(width, height, components, hs, vs, quants, tables):
    """SOI .. SOS: quants in natural order, tables as (bits, values) in the order DC0, AC0, DC1, AC1"""
    def segment(marker, body):
        return bytes([0xFF, marker]) + (len(body) + 2).to_bytes(2, "big") + bytes(body)

    out = b"\xFF\xD8" + segment(0xE0, b"JFIF\x00\x01\x01\x00\x00\x01\x00\x01\x00\x00")
    for k, q in enumerate(quants):
        out += segment(0xDB, bytes([k]) + bytes(int(v) for v in np.asarray(q)[ZIGZAG]))
    frame = bytes([8]) + height.to_bytes(2, "big") + width.to_bytes(2, "big") + bytes([components])
    for c in range(components):
        frame += bytes([c + 1, (hs << 4 | vs) if c == 0 else 0x11, min(c, 1)])
    out += segment(0xC0, frame)
    for k, (bits, values) in enumerate(tables):
        out += segment(0xC4, bytes([(k & 1) << 4 | k >> 1]) + bytes(bits) + bytes(values))
    scan = bytes([components])
    for c in range(components):
        scan += bytes([c + 1, 0x11 * min(c, 1)])
    return out + segment(0xDA, scan + bytes([0, 63, 0]))


def encode(pixels, quality: int = 75, sampling: int = S420, optimize: bool = False):
    """-> dict: file, sections (before the scan data, the data, after), stats (blocks, dummy_blocks, bits, stuffed - what
    cvhip_jpeg_encode_last_stats reports), histograms (DC0, AC0, DC1, AC1: 256 counts each), and counters of what the scan met."""
    px = np.asarray(pixels, dtype=np.uint8)
    if px.ndim == 2:
        px = px[:, :, None]
    height, width, channels = px.shape
    components = 1 if channels <= 2 else 3
    g = geometry(width, height, components, sampling)
    hs, vs, mcus_x, mcus_y = g["hs"], g["vs"], g["mcus_x"], g["mcus_y"]
    quants = [quant_table(QUANT_LUMA, quality)] + ([quant_table(QUANT_CHROMA, quality)] if components == 3 else [])
    planes = [px[..., 0].astype(np.int64)] if components == 1 else list(ycc(px))
    coefs = []  # per component [blocks_y, blocks_x, 64]
    for c, plane in enumerate(planes):
        hf, vf = (1, 1) if c == 0 else (hs, vs)
        bx, by = (g["blocks_x"], g["blocks_y"]) if c == 0 else (mcus_x, mcus_y)
        rows_mcu = mcus_y * 8 * (vs if c == 0 else 1)
        comp = component_plane(plane, hf, vf, bx, by, rows_mcu)
        blocks = comp.reshape(by, 8, bx, 8).transpose(0, 2, 1, 3).reshape(-1, 8, 8)
        coefs.append(fdct_quantise(blocks, quants[min(c, 1)]).reshape(by, bx, 64))
    # the scan's blocks in MCU order: (component, coefficients); a dummy block has the DC of the block before it and no AC
    order, dummies = [], 0
    for my in range(mcus_y):
        for mx in range(mcus_x):
            for c in range(components):
                for k in range(hs * vs if c == 0 else 1):
                    x, y = (mx * hs + k % hs, my * vs + k // hs) if c == 0 else (mx, my)
                    if x < coefs[c].shape[1] and y < coefs[c].shape[0]:
                        order.append((c, coefs[c][y, x]))
                    else:
                        dummy = np.zeros(64, dtype=np.int64)
                        dummy[0] = order[-1][1][0]
                        order.append((c, dummy))
                        dummies += 1
    pred, symbols = [0] * components, []
    for c, coef in order:
        symbols.append((min(c, 1), block_symbols(coef, pred[c])))
        pred[c] = int(coef[0])
    hist = np.zeros((4, 256), dtype=np.int64)
    for t, syms in symbols:
        for is_ac, s, _v, _n in syms:
            hist[2 * t + is_ac, s] += 1
    n_tables = 2 if components == 1 else 4
    tables = [optimal_table(hist[k]) for k in range(n_tables)] if optimize else list(STANDARD_TABLES[:n_tables])
    codes = [code_table(*t) for t in tables]
    nbits, pieces = 0, []
    met = {"zrl": 0, "eob": 0, "coef63": 0, "dc_category": {}, "ac_category": 0, "longest_block": 0, "shortest_block": 1 << 30,
           "ends_on_dword": 0, "long_from_dword": 0}
    for t, syms in symbols:
        before = nbits
        for is_ac, s, v, n in syms:
            code, length = codes[2 * t + is_ac][s]
            if length + n:
                pieces.append(format(code << n | v, "0%db" % (length + n)))
            nbits += length + n
            if is_ac:
                met["zrl"] += s == 0xF0
                met["eob"] += s == 0
                met["ac_category"] = max(met["ac_category"], s & 15)
            else:
                sign = 0 if n == 0 else 1 if v >> (n - 1) else -1
                met["dc_category"][sign * n] = met["dc_category"].get(sign * n, 0) + 1
        met["coef63"] += syms[-1][0] == 1 and syms[-1][1] != 0
        met["longest_block"], met["shortest_block"] = max(met["longest_block"], nbits - before), min(met["shortest_block"], nbits - before)
        # the 32-bit words of the unstuffed stream: a block that ends exactly on a word's boundary (nothing left to share with
        # the next block), and a block of more than 32 bits that starts on one (its first word is not shared with the one before)
        met["ends_on_dword"] += nbits % 32 == 0
        met["long_from_dword"] += before % 32 == 0 and nbits - before > 32
    padding = -nbits % 8
    raw = int("".join(pieces) + "1" * padding, 2).to_bytes((nbits + padding) // 8, "big")
    data = raw.replace(b"\xFF", b"\xFF\x00")
    met["adjacent_ff"] = b"\xFF\xFF" in raw
    met["last_byte_ff"] = raw.endswith(b"\xFF")
    met["tile_end_ff"] = any(raw[k] == 0xFF for k in range(STUFF_TILE - 1, len(raw) - 1, STUFF_TILE))
    met["raw_bytes"] = len(raw)
    head = header(width, height, components, hs, vs, quants, tables)
    return {"file": head + data + b"\xFF\xD9", "sections": (len(head), len(data), 2),
            "stats": {"blocks": len(order), "dummy_blocks": dummies, "bits": nbits, "stuffed": len(data) - len(raw)},
            "histograms": [[int(v) for v in hist[k]] for k in range(n_tables)], "tables": tables, "quants": quants, "met": met}
