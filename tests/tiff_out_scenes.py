"""Pictures for cvhip_tiff_encode, each on a seam of the encoder.  scene(name) -> (pixels [h, w, c] uint8,
compression, predictor, rows_per_strip); names() -> all of them.  mesh.GRID_LANES / 64 and / 256 are the waves of one
tiff_lzw_kernel launch and the workgroups of one tiff_copy_kernel launch.  LZW_STAGE is the bytes of a strip the LZW kernel stages
at a time (tiff_encode_common.hpp's LZW_CHUNK); a strip longer than it is walked in pieces."""
import functools

import numpy as np

import ref_tiff_out as R
from cybervision_amd import mesh  # (GRID_LANES only: importing it loads no library)
from tiff_scenes import picture

NONE, LZW, PACKBITS = R.NONE, R.LZW, R.PACKBITS
LZW_STAGE = 1024


def noise(n, seed):
    return np.random.default_rng(seed).integers(0, 256, size=n, dtype=np.uint8)


@functools.lru_cache(maxsize=None)
def noise_strip(data_codes, seed=31):
    """The shortest prefix of a noise sequence whose strip has `data_codes` codes between its first Clear and what ends it."""
    base = noise(data_codes + 400, seed)
    lo, hi = 1, len(base)
    while lo < hi:   # (the count does not fall when a byte is added)
        mid = (lo + hi) // 2
        if len(R.lzw_codes(base[:mid].tobytes())) - 2 - (data_codes >= R.CLEAR_AFTER) >= data_codes:
            hi = mid
        else:
            lo = mid + 1
    return base[:lo].reshape(1, lo, 1)


@functools.lru_cache(maxsize=None)
def bit_tail_strip(tail):
    """A short noise strip whose code stream ends `tail` bits into its last byte (tail 1 .. 7), of odd length."""
    base = noise(200, 32)
    for n in range(20, 200):
        codes = R.lzw_codes(base[:n].tobytes())
        bits = 9 * len(codes)   # (fewer than 254 codes)
        if bits % 8 == tail and len(R.lzw_pack(codes)) % 2 == 1:
            return base[:n].reshape(1, n, 1)
    raise AssertionError(tail)


@functools.lru_cache(maxsize=None)
def pair_distinct():
    """65280 bytes of which no two adjacent pairs are equal: LZW never finds a string of two bytes in its table, so every byte
    after the first costs a code - the most codes a staging of the kernel can hold."""
    return np.array([v for a in range(256) for b in range(a + 1, 256) for v in (a, b)], dtype=np.uint8)


CLEAR_AT_WINDOW = range(270, 300)   # lead-ins tried by clear_at (found by hand: 282 .. 285 for the residues 1022, 1023, 0, 1)


@functools.lru_cache(maxsize=None)
def clear_at(residue):
    """6000 bytes - a flat lead-in of 0x80, then pair_distinct() - whose first table-full Clear leaves with a byte at
    `residue` of a staging; the lead-in's length is searched in CLEAR_AT_WINDOW."""
    for lead in CLEAR_AT_WINDOW:
        data = np.concatenate([np.full(lead, 0x80, dtype=np.uint8), pair_distinct()[:6000 - lead]])
        clears = [r for s in R.lzw_stagings(data.tobytes(), LZW_STAGE) for r in s["clears"]]
        if clears and clears[0] == residue:
            return data.reshape(1, 6000, 1)
    raise AssertionError(residue)


PB_SWEEP = [(n, p) for n in (2, 3, 4, 128, 129, 130, 131) for p in (61, 62, 63, 64, 65, 66, 253, 254, 255, 256, 257, 258)]


def pb_sweep_rows():
    """Rows of 700 bytes, one per (n, p) of PB_SWEEP: a run of n bytes of 255 that starts at position p - on either side of
    lane 64 and of workgroup 256 of a kernel that walks a row in parallel - between literals without equal neighbours (all
    below 251, so the run does not grow)."""
    def literal(n, first):
        return ((np.arange(n) * 7 + first) % 251).astype(np.uint8)

    rows = [np.concatenate([literal(p, 1), np.full(n, 255, dtype=np.uint8), literal(700 - p - n, 9)]) for n, p in PB_SWEEP]
    return np.stack(rows).reshape(len(rows), 700, 1)


def widest_rgba(seed):
    """2 x 65535 x 4, the widest row the encoder takes: steps of 97 pixels, equal in the four channels (runs; zeros behind
    Predictor 2), with one byte in fifty replaced by noise (literals)."""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:2, 0:65535]
    a = np.repeat(((x // 97 + 3 * y) % 256)[:, :, None], 4, axis=2).astype(np.uint8)
    hit = rng.integers(0, 50, size=a.shape) == 0
    a[hit] = rng.integers(0, 256, size=int(hit.sum()), dtype=np.uint8)
    return a


def second_trip_rows():
    """GRID_LANES / 64 noise rows of 40 bytes and the first 6 of them again: with a row a strip, strip s and strip
    s + GRID_LANES / 64 are equal and are the first and the second strip of one wave of tiff_lzw_kernel."""
    rows = noise(mesh.GRID_LANES // 64 * 40, 35).reshape(-1, 40, 1)
    return np.concatenate([rows, rows[:6]])


def pb_rows():
    """Rows of 600 bytes on the packet seams: runs of 2, 3, 127 .. 131 and 258, literals of 127, 128, 129, a triple in the
    last three bytes."""
    rng = np.random.default_rng(33)

    def literal(n, first=1):
        v = (np.arange(n) * 7 + first) % 251   # (no two neighbours equal)
        return v.astype(np.uint8)

    def row(parts):
        out = np.concatenate(parts)
        fill = literal(600 - len(out), 3)
        fill[0] = out[-1] ^ 0x55   # (the last run does not grow)
        return np.concatenate([out, fill])[:600]

    def run(n, v):
        return np.full(n, v, dtype=np.uint8)

    rows = [row([literal(5), run(n, 200), literal(4, 9)]) for n in (2, 3, 127, 128, 129, 130, 131, 258)]
    rows += [row([run(4, 9), literal(n, 20), run(5, 250)]) for n in (127, 128, 129)]
    last = literal(600, 5)
    last[-3:] = 99
    rows.append(last)
    rows.append(run(600, 7))
    rows.append(rng.integers(0, 2, size=600, dtype=np.uint8))
    return np.stack(rows).reshape(len(rows), 600, 1)


def _scenes():
    P = picture
    s = {}
    # ---- LZW code widths: EOI is the c-th code since the Clear, 9 | 10 bits at c = 253 | 254, and so on
    for seam in (254, 766, 1790):
        for c in (seam - 1, seam, seam + 1):
            s["lzw_width_%d" % c] = functools.partial(lambda c: (noise_strip(c), LZW, 1, 1), c)
    # ---- LZW Clear at table-full
    s["lzw_noise_8192_one_strip"] = lambda: (P(64, 128, seed=16, kind="noise"), LZW, 1, 64)
    s["lzw_last_code_3835"] = lambda: (noise_strip(3835), LZW, 1, 1)
    s["lzw_last_code_3836"] = lambda: (noise_strip(3836), LZW, 1, 1)   # libtiff: Clear, then EOI of 9 bits
    s["lzw_last_code_3837"] = lambda: (noise_strip(3837), LZW, 1, 1)
    s["lzw_flat"] = lambda: (P(64, 64, kind="flat"), LZW, 1, 64)   # self-overlapping strings, the longest string
    s["lzw_flat_pred"] = lambda: (P(64, 64, kind="flat"), LZW, 2, 64)
    s["lzw_1x1"] = lambda: (P(1, 1, seed=3), LZW, 1, 0)
    s["lzw_1x1_rgba_pred"] = lambda: (P(1, 1, 4, seed=3), LZW, 2, 0)
    # ---- LZW bit packing
    for tail in range(1, 8):
        s["lzw_tail_%d" % tail] = functools.partial(lambda t: (np.repeat(bit_tail_strip(t), 3, axis=0), LZW, 1, 1), tail)   # odd payloads: padding
    # ---- Predictor 2
    s["pred_g8"] = lambda: (P(47, 33, seed=12, kind="noise"), LZW, 2, 7)   # (noise: differences wrap modulo 256)
    s["pred_ga8"] = lambda: (P(13, 9, 2, seed=12), LZW, 2, 4)
    s["pred_rgb8"] = lambda: (P(47, 33, 3, seed=15), LZW, 2, 7)
    s["pred_rgba8"] = lambda: (P(47, 33, 4, seed=9, kind="noise"), LZW, 2, 7)
    s["pred_width_1_rgb"] = lambda: (P(9, 1, 3, seed=15, kind="noise"), LZW, 2, 4)
    s["pred_wrap"] = lambda: (np.array([[[0], [255], [0], [1], [200], [100]], [[255], [0], [0], [0], [128], [127]]], dtype=np.uint8), LZW, 2, 2)
    # ---- PackBits
    s["pb_seams"] = lambda: (pb_rows(), PACKBITS, 1, 5)
    s["pb_two_flat_rows"] = lambda: (P(2, 50, kind="flat"), PACKBITS, 1, 2)   # a run that would cross the row end
    s["pb_1_byte_rows"] = lambda: (P(5, 1, seed=4), PACKBITS, 1, 2)
    for w in (63, 64, 65, 257):
        s["pb_width_%d" % w] = functools.partial(lambda w: (np.random.default_rng(w).integers(0, 3, size=(6, w, 1), dtype=np.uint8), PACKBITS, 1, 4), w)
        s["pb_flat_width_%d" % w] = functools.partial(lambda w: (P(3, w, kind="flat"), PACKBITS, 1, 2), w)
    s["pb_rgb"] = lambda: (P(20, 33, 3, seed=8), PACKBITS, 1, 0)
    s["pb_rgba_sparse"] = lambda: (P(20, 33, 4, seed=8) * (P(20, 33, 1, seed=5) > 128), PACKBITS, 1, 3)
    # ---- strips and scans
    s["one_strip_raw"] = lambda: (P(7, 5, seed=2), NONE, 1, 0)
    s["two_strips_raw_rgb"] = lambda: (P(7, 5, 3, seed=2), NONE, 1, 4)   # an odd first strip (60 B is even: 4 x 15), a short last
    s["odd_strips_raw"] = lambda: (P(7, 5, seed=2), NONE, 1, 1)
    s["raw_1_byte_strips"] = lambda: (P(5, 1, seed=4), NONE, 1, 1)   # the copy kernel's units of one byte, a padding byte between them
    s["ga_raw"] = lambda: (P(7, 5, 2, seed=2), NONE, 1, 3)
    for n in (64, 65, 256, 257):
        s["strips_%d_lzw" % n] = functools.partial(lambda n: (P(n, 3, seed=n), LZW, 1, 1), n)
    s["strips_65_packbits"] = lambda: (P(65, 3, seed=6), PACKBITS, 1, 1)
    s["strips_1025_lzw"] = lambda: (P(1025, 1, seed=7), LZW, 1, 1)
    s["strips_1025_raw"] = lambda: (P(1025, 1, seed=7), NONE, 1, 1)
    s["short_last_strip_lzw"] = lambda: (P(47, 33, 4, seed=9), LZW, 1, 7)
    s["default_rps_below_8192"] = lambda: (P(5, 2047, 4, seed=10), LZW, 2, 0)   # row_bytes 8188: 1 row a strip
    s["default_rps_equal_8192"] = lambda: (P(3, 2048, 4, seed=10), LZW, 2, 0)
    s["default_rps_above_8192"] = lambda: (P(3, 2049, 4, seed=10), PACKBITS, 1, 0)
    s["default_rps_small_rows"] = lambda: (P(300, 33, seed=11), LZW, 1, 0)   # 248 rows a strip, a short last one
    s["lzw_strip_64k"] = lambda: (P(64, 1024, seed=12), LZW, 2, 64)   # 64 stagings of the kernel; smooth: long strings cross them
    s["lzw_strip_64k_noise_2_strips"] = lambda: (P(72, 1024, seed=13, kind="noise"), LZW, 1, 64)
    # ---- LZW stagings of the kernel (LZW_STAGE bytes): the densest, strips beside a multiple of it, a last staging of 1 byte
    D = pair_distinct
    for n in (1023, 1024, 1025, 2047, 2048, 2049, 4096):
        s["lzw_dense_%d" % n] = functools.partial(lambda n: (D()[:n].reshape(1, n, 1), LZW, 1, 1), n)
    for r in (1022, 1023, 0, 1):   # a table-full Clear with the last and the first bytes of a staging
        s["lzw_clear_at_%d" % r] = functools.partial(lambda r: (clear_at(r), LZW, 1, 1), r)
    s["lzw_dense_strips"] = lambda: (D().reshape(85, 768, 1), LZW, 1, 16)   # strips of 12 stagings close to their scratch stride, a short last one
    s["lzw_flat_640k"] = lambda: (P(640, 1024, kind="flat"), LZW, 1, 640)   # strings longer than a staging: stagings without a code
    s["pred_rows_1023"] = lambda: (P(5, 341, 3, seed=17, kind="noise"), LZW, 2, 5)   # rows that start in mid-staging
    s["pred_rows_1028"] = lambda: (P(5, 257, 4, seed=18, kind="noise"), LZW, 2, 5)
    s["pred_rows_1025"] = lambda: (P(5, 1025, 1, seed=19, kind="noise"), LZW, 2, 5)
    # ---- launches: a wave's second strip, the copy kernel's second trip over rows, the most rows, the widest row
    s["strips_lzw_second_trip"] = lambda: (second_trip_rows(), LZW, 1, 1)
    s["strips_65535_lzw"] = lambda: (P(65535, 1, seed=20), LZW, 1, 1)
    s["strips_65535_packbits"] = lambda: (P(65535, 1, seed=20), PACKBITS, 1, 1)
    s["pb_rows_second_trip"] = lambda: (np.random.default_rng(36).integers(0, 3, size=(mesh.GRID_LANES // 256 + 6, 37, 1), dtype=np.uint8), PACKBITS, 1, 7)
    s["widest_rgba_packbits"] = lambda: (widest_rgba(37), PACKBITS, 1, 0)
    s["widest_rgba_lzw_pred"] = lambda: (widest_rgba(37), LZW, 2, 0)
    s["pb_seam_sweep"] = lambda: (pb_sweep_rows(), PACKBITS, 1, 5)
    return s


def names():
    return sorted(_scenes())


def lzw_names():
    return [n for n in names() if scene(n)[1] == LZW]


@functools.lru_cache(maxsize=None)
def scene(name):
    pixels, compression, predictor, rps = _scenes()[name]()
    pixels = np.ascontiguousarray(pixels, dtype=np.uint8)
    pixels.setflags(write=False)
    return pixels, compression, predictor, rps


def strip_bytes(name):
    """What the scene's strips compress: the bytes of each strip's rows, behind Predictor 2 where the scene has it."""
    pixels, compression, predictor, rps = scene(name)
    h, w, c = pixels.shape
    _row_bytes, rows_per_strip, strips = R.check(w, h, c, compression, predictor, rps)
    rows = pixels.reshape(h, w * c)
    if predictor == 2:
        rows = R.predict(rows, c)
    return [rows[s * rows_per_strip:(s + 1) * rows_per_strip].tobytes() for s in range(strips)]


@functools.lru_cache(maxsize=None)
def expected(name):
    """(the file, stats, sections) of the restatement - computed once."""
    pixels, compression, predictor, rps = scene(name)
    stats, sections = {}, []
    data = R.encode(pixels, compression, predictor, rps, stats, sections)
    return data, stats, tuple(sections)


# (width, height, channels, compression, predictor, rows_per_strip) -> the code
REFUSED = {
    "width_0": ((0, 4, 1, LZW, 1, 0), R.INVALID), "height_0": ((4, 0, 1, LZW, 1, 0), R.INVALID),
    "channels_0": ((4, 4, 0, LZW, 1, 0), R.INVALID), "channels_5": ((4, 4, 5, LZW, 1, 0), R.INVALID),
    "compression_0": ((4, 4, 1, 0, 1, 0), R.INVALID), "compression_8": ((4, 4, 1, 8, 1, 0), R.INVALID),
    "predictor_0": ((4, 4, 1, LZW, 0, 0), R.INVALID), "predictor_3": ((4, 4, 1, LZW, 3, 0), R.INVALID),
    "predictor_2_raw": ((4, 4, 1, NONE, 2, 0), R.INVALID), "predictor_2_packbits": ((4, 4, 1, PACKBITS, 2, 0), R.INVALID),
    "width_65536": ((65536, 1, 1, NONE, 1, 0), R.UNSUPPORTED), "height_65536": ((1, 65536, 1, NONE, 1, 0), R.UNSUPPORTED),
    "strip_2_31": ((65535, 65535, 1, NONE, 1, 40000), R.UNSUPPORTED),
    "file_2_32": ((65535, 65535, 1, NONE, 1, 1), R.UNSUPPORTED),
}
