"""The PNG file image of cvhip_png_encode, restated in Python and numpy.  This file is the definition:
the library must produce these bytes.  It shares no code with the product and uses zlib nowhere (the tests compare the two).

The file: signature, IHDR (depth 8, colour type 0 / 4 / 2 / 6 for 1 / 2 / 3 / 4 channels, no interlace), ONE IDAT, IEND.
The IDAT data: 78 01, one dynamic-Huffman deflate block (BFINAL = 1), the Adler-32 of the filtered bytes.
Tokens are made per row (filter byte included), from repeats of the previous byte only: a match always has distance 1.
"""
from __future__ import annotations

import numpy as np

SIGNATURE = bytes([0x89, 0x50, 0x4E, 0x47, 0x0D, 0x0A, 0x1A, 0x0A])
COLOUR_TYPE = {1: 0, 2: 4, 3: 2, 4: 6}
FILTER_NONE, FILTER_SUB, FILTER_UP, FILTER_AVERAGE, FILTER_PAETH, FILTER_ADAPTIVE = range(6)
CL_ORDER = (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)
# RFC 1951 3.2.5: length symbols 257..285 -> (base length, extra bits)
LENGTH_BASE = (3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258)
LENGTH_EXTRA = (0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0)
TOKEN_MATCH = 256  # a token is a literal 0..255, or TOKEN_MATCH + (length - 3) for a match of 3..258 at distance 1


# ---- checksums, bit by bit --------------------------------------------------------------------------------------------------------
def crc32(data: bytes) -> int:
    table = []
    for n in range(256):
        c = n
        for _ in range(8):
            c = (c >> 1) ^ 0xEDB88320 if c & 1 else c >> 1
        table.append(c)
    c = 0xFFFFFFFF
    for b in data:
        c = table[(c ^ b) & 0xFF] ^ (c >> 8)
    return c ^ 0xFFFFFFFF


def adler32(data: bytes) -> int:
    a, b = 1, 0
    d = np.frombuffer(bytes(data), dtype=np.uint8).astype(np.int64)
    for start in range(0, len(d), 4096):  # (a block of 4096 keeps every sum far below 2^63)
        block = d[start:start + 4096]
        n = len(block)
        b = (b + n * a + int((block * np.arange(n, 0, -1)).sum())) % 65521
        a = (a + int(block.sum())) % 65521
    return (b << 16) | a


# ---- filters ------------------------------------------------------------------------------------------------------------------------
def _filter_row(kind: int, row: np.ndarray, up: np.ndarray, bpp: int) -> np.ndarray:
    x = row.astype(np.int32)
    b = up.astype(np.int32)
    a = np.concatenate([np.zeros(bpp, dtype=np.int32), x[:-bpp]]) if len(x) > bpp else np.zeros(len(x), dtype=np.int32)
    c = np.concatenate([np.zeros(bpp, dtype=np.int32), b[:-bpp]]) if len(x) > bpp else np.zeros(len(x), dtype=np.int32)
    if kind == FILTER_NONE:
        pred = np.zeros_like(x)
    elif kind == FILTER_SUB:
        pred = a
    elif kind == FILTER_UP:
        pred = b
    elif kind == FILTER_AVERAGE:
        pred = (a + b) >> 1
    else:
        p = a + b - c
        pa, pb, pc = np.abs(p - a), np.abs(p - b), np.abs(p - c)
        pred = np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, b, c))
    return ((x - pred) & 0xFF).astype(np.uint8)


def row_score(filtered: np.ndarray) -> int:
    v = filtered.astype(np.int64)
    return int(np.where(v < 128, v, 256 - v).sum())


def filter_rows(pixels: np.ndarray, kind: int):
    """pixels [h, w, c] uint8 -> (filtered [h, 1 + w * c] uint8 with the filter byte in column 0, scores: per row the five
    scores in ADAPTIVE mode, else None)."""
    h, w, ch = pixels.shape
    rows = pixels.reshape(h, w * ch)
    out = np.zeros((h, 1 + w * ch), dtype=np.uint8)
    scores = [] if kind == FILTER_ADAPTIVE else None
    zero = np.zeros(w * ch, dtype=np.uint8)
    for y in range(h):
        up = rows[y - 1] if y else zero
        if kind == FILTER_ADAPTIVE:
            cand = [_filter_row(k, rows[y], up, ch) for k in range(5)]
            sc = [row_score(f) for f in cand]
            best = min(range(5), key=lambda k: (sc[k], k))
            scores.append(sc)
            out[y, 0], out[y, 1:] = best, cand[best]
        else:
            out[y, 0], out[y, 1:] = kind, _filter_row(kind, rows[y], up, ch)
    return out, scores


# ---- tokens -------------------------------------------------------------------------------------------------------------------------
def row_tokens(b: np.ndarray) -> list:
    """The tokens of one row's bytes (filter byte first)."""
    out = [int(b[0])]
    n = len(b)
    i = 1
    while i < n:
        if b[i] != b[i - 1]:
            out.append(int(b[i]))
            i += 1
            continue
        j = i
        while j < n and b[j] == b[j - 1]:
            j += 1
        run = j - i  # a maximal interval of repeating positions
        while run >= 3:
            m = min(run, 258)
            out.append(TOKEN_MATCH + m - 3)
            run -= m
        out.extend([int(b[i])] * run)
        i = j
    return out


def length_symbol(length: int):
    """-> (symbol 257..285, extra bits, their value)"""
    if length == 258:
        return 285, 0, 0
    k = max(i for i in range(28) if LENGTH_BASE[i] <= length)
    return 257 + k, LENGTH_EXTRA[k], length - LENGTH_BASE[k]


def token_symbol(token: int) -> int:
    return token if token < TOKEN_MATCH else length_symbol(token - TOKEN_MATCH + 3)[0]


# ---- codes --------------------------------------------------------------------------------------------------------------------------
def package_merge(freqs, limit: int) -> list:
    """Length-limited code lengths of the symbols with freqs > 0 (0 for the others)."""
    leaves = sorted((f, s) for s, f in enumerate(freqs) if f > 0)
    k = len(leaves)
    lengths = [0] * len(freqs)
    if k == 0:
        return lengths
    if k == 1:
        lengths[leaves[0][1]] = 1
        return lengths
    # an item: (weight, how often each leaf is in it)
    leaf_items = []
    for i, (f, _s) in enumerate(leaves):
        c = np.zeros(k, dtype=np.int64)
        c[i] = 1
        leaf_items.append((f, c))
    current = list(leaf_items)
    for _ in range(limit - 1):
        packages = [(current[2 * i][0] + current[2 * i + 1][0], current[2 * i][1] + current[2 * i + 1][1]) for i in range(len(current) // 2)]
        merged, li, pi = [], 0, 0
        while li < k or pi < len(packages):
            if pi >= len(packages) or (li < k and leaf_items[li][0] <= packages[pi][0]):  # leaves first on equal weight
                merged.append(leaf_items[li])
                li += 1
            else:
                merged.append(packages[pi])
                pi += 1
        current = merged
    total = np.zeros(k, dtype=np.int64)
    for _w, c in current[:2 * k - 2]:
        total += c
    for i, (_f, s) in enumerate(leaves):
        lengths[s] = int(total[i])
    return lengths


def canonical_codes(lengths) -> list:
    """RFC 1951 3.2.2 -> the code of each symbol, as the RFC numbers it (its first bit is the most significant)."""
    max_len = max(lengths) if len(lengths) else 0
    count = [0] * (max_len + 2)
    for n in lengths:
        count[n] += 1
    count[0] = 0
    code, next_code = 0, [0] * (max_len + 2)
    for bits in range(1, max_len + 1):
        code = (code + count[bits - 1]) << 1
        next_code[bits] = code
    codes = [0] * len(lengths)
    for s, n in enumerate(lengths):
        if n:
            codes[s] = next_code[n]
            next_code[n] += 1
    return codes


class BitWriter:
    def __init__(self):
        self.done, self.acc, self.held, self.n = bytearray(), 0, 0, 0  # n: all bits so far; held: those still in acc

    def bits(self, value: int, count: int):
        """`count` bits of value, least significant first (header fields, extra bits)"""
        self.acc |= (value & ((1 << count) - 1)) << self.held
        self.held += count
        self.n += count
        while self.held >= 8:
            self.done.append(self.acc & 0xFF)
            self.acc >>= 8
            self.held -= 8

    def code(self, code: int, count: int):
        """a Huffman code: most significant bit first"""
        rev = int(format(code, "0%db" % count)[::-1], 2) if count else 0
        self.bits(rev, count)

    def tobytes(self) -> bytes:
        return bytes(self.done) + (bytes([self.acc]) if self.held else b"")


def block_header(litlen_lengths):
    """The dynamic block's header for the literal/length code lengths (286 of them) -> (BitWriter, dict of its parts)."""
    hlit = max(s for s, n in enumerate(litlen_lengths) if n) + 1
    hlit = max(hlit, 257)
    sent = list(litlen_lengths[:hlit]) + [1]  # HDIST = 1: distance symbol 0, one bit
    cl_freq = [0] * 19
    for n in sent:
        cl_freq[n] += 1
    cl_lengths = package_merge(cl_freq, 7)
    cl_codes = canonical_codes(cl_lengths)
    hclen = max(4, max(i for i, s in enumerate(CL_ORDER) if cl_lengths[s]) + 1)
    w = BitWriter()
    w.bits(1, 1)  # BFINAL
    w.bits(2, 2)  # BTYPE = 10
    w.bits(hlit - 257, 5)
    w.bits(0, 5)  # HDIST - 1
    w.bits(hclen - 4, 4)
    for s in CL_ORDER[:hclen]:
        w.bits(cl_lengths[s], 3)
    for n in sent:
        w.code(cl_codes[n], cl_lengths[n])
    return w, {"hlit": hlit, "hclen": hclen, "cl_lengths": cl_lengths, "cl_freq": cl_freq}


def chunk(kind: bytes, data: bytes) -> bytes:
    return len(data).to_bytes(4, "big") + kind + data + crc32(kind + data).to_bytes(4, "big")


def as_image(pixels) -> np.ndarray:
    p = np.ascontiguousarray(pixels, dtype=np.uint8)
    if p.ndim == 2:
        p = p[:, :, None]
    assert p.ndim == 3 and 1 <= p.shape[2] <= 4 and p.shape[0] and p.shape[1]
    return p


def encode(pixels, kind: int = FILTER_ADAPTIVE) -> dict:
    """-> dict: file (bytes), sections (bytes before the IDAT data, the IDAT data, bytes after it), filtered [h, 1 + w c],
    scores, histogram (286), litlen_lengths (286), header (hlit, hclen, cl_lengths, cl_freq), header_bits."""
    p = as_image(pixels)
    h, w, ch = p.shape
    filtered, scores = filter_rows(p, kind)
    tokens = [row_tokens(filtered[y]) for y in range(h)]
    hist = [0] * 286
    for row in tokens:
        for t in row:
            hist[token_symbol(t)] += 1
    hist[256] += 1
    lengths = package_merge(hist, 15)
    codes = canonical_codes(lengths)
    wr, parts = block_header(lengths)
    header_bits = wr.n
    for row in tokens:
        for t in row:
            if t < TOKEN_MATCH:
                wr.code(codes[t], lengths[t])
            else:
                s, extra, value = length_symbol(t - TOKEN_MATCH + 3)
                wr.code(codes[s], lengths[s])
                wr.bits(value, extra)
                wr.bits(0, 1)  # the one distance code
        # (nothing crosses a row)
    wr.code(codes[256], lengths[256])
    raw = filtered.tobytes()
    idat = b"\x78\x01" + wr.tobytes() + adler32(raw).to_bytes(4, "big")
    ihdr = w.to_bytes(4, "big") + h.to_bytes(4, "big") + bytes([8, COLOUR_TYPE[ch], 0, 0, 0])
    file = SIGNATURE + chunk(b"IHDR", ihdr) + chunk(b"IDAT", idat) + chunk(b"IEND", b"")
    return {"file": file, "sections": (41, len(idat), 16), "filtered": filtered, "scores": scores, "histogram": hist,
            "litlen_lengths": lengths, "header": parts, "header_bits": header_bits}


def stored_size(raw_bytes: int) -> int:
    """the zlib stream of the same bytes in stored deflate blocks"""
    return raw_bytes + 5 * -(-raw_bytes // 65535) + 6
