"""The images the PNG tests encode (tests/ref_png.py is the definition of the file): name -> (pixels, filter).  Every image is
the smallest at which one part of the encoder can break; test_png_ref.py asserts, on the restatement alone, that each scene
does reach the case it is here for (DESIGN.md 4.15 lists the tokeniser's and the trailer's seams and the scene of each)."""
from __future__ import annotations

import functools

import numpy as np

import ref_png

RUNS = (2, 3, 4, 258, 259, 260, 261, 516, 517)  # repeat runs of the `runs` scene, one row each


def _paeth(a, b, c):
    p = a + b - c
    pa, pb, pc = abs(p - a), abs(p - b), abs(p - c)
    return a if pa <= pb and pa <= pc else b if pb <= pc else c


def runs():
    """Grey rows for filter 0: value 200 repeated run + 1 times (a literal and a repeat run of exactly `run` positions), then a
    filler that never repeats."""
    width = 600
    img = np.zeros((len(RUNS), width), dtype=np.uint8)
    for y, run in enumerate(RUNS):
        img[y, :run + 1] = 200
        img[y, run + 1:] = 10 + (np.arange(width - run - 1) % 2) * 7 + (np.arange(width - run - 1) % 3)
    return img


def filler(n: int):
    """n bytes of 10 .. 19 of which no two neighbours are equal: the filler behind the runs of runs()"""
    return 10 + (np.arange(n) % 2) * 7 + (np.arange(n) % 3)


def run_row(width: int, start: int, run: int, value: int):
    """A grey row for filter 0 whose filtered bytes (the filter's 0 first, so a pixel's position is its index + 1) repeat at
    exactly the `run` positions from `start` on: `value` at the run + 1 pixels from position start - 1, filler around them."""
    assert 2 <= start and start + run <= width + 1 and run >= 1
    row = filler(width)
    row[start - 2:start - 1 + run] = value
    if start - 1 + run < width:
        row[start - 1 + run:] = filler(width - (start - 1 + run))
    return row.astype(np.uint8)


# run_seams: one row per (first repeating position, repeating positions).  The tokeniser (row_tokens in png_kernels.hip)
# takes 64 positions a step; the starts lie around lanes 0 .. 2 and 61 .. 63 of the first three steps, the lengths around
# every count at which a run's chunks of 258, its rest of 0 .. 2 literals or its look of 320 bytes past a step change.
SEAM_STARTS = (2, 61, 62, 63, 64, 65, 66, 126, 127, 128, 129)
SEAM_RUNS = (*range(1, 9), *range(59, 68), 128, 129, *range(256, 263), *range(319, 328), *range(516, 520), *range(576, 584))
SEAM_WIDTH = 999


def run_seams():
    return np.stack([run_row(SEAM_WIDTH, s, run, 200) for s in SEAM_STARTS for run in SEAM_RUNS])


# run_ends_<w>: every row's run ends at the row's last byte, RUN_END_PAST[w] bytes past the step (the second, positions 64 ..
# 127) in which it starts, at lane 62 (rows 0 and 2) or 63 (rows 1 and 3).  The run's byte is 0, the byte behind every row
# but the last is the next row's filter byte, 0 too: a look past the step that did not stop at the row's end would find the
# run one byte longer.  0: no byte follows the step, so there is no look; 12 gives a look that breaks in its third lane.
RUN_END_PAST = {127: 0, 128: 1, 131: 4, 132: 5, 133: 6, 139: 12, 384: 257, 446: 319}
RUN_END_STARTS = (126, 127, 126, 127)


def run_ends(width: int):
    return np.stack([run_row(width, s, width + 1 - s, 0) for s in RUN_END_STARTS])


def channels(c: int):
    """37 x 5 with c channels: a slope and noise"""
    rng = np.random.RandomState(100 + c)
    y, x = np.mgrid[0:5, 0:37]
    base = (3 * x + 5 * y)[:, :, None] + 40 * np.arange(c)[None, None, :]
    return ((base + rng.randint(0, 4, size=(5, 37, c))) & 0xFF).astype(np.uint8)


def adaptive():
    """130 x 96 RGB in bands of 16 rows, each built so that one filter leaves (nearly) nothing: flat zero rows (all five
    scores tie), small values under a noisy row (None), a ramp along the row (Sub), the row above plus little (Up), the
    Average and the Paeth predictor followed exactly."""
    rng = np.random.RandomState(7)
    w, h, c = 130, 96, 3
    img = np.zeros((h, w, c), dtype=np.int64)
    for y in range(16, h):
        band = y // 16
        noisy = rng.randint(0, 256, size=(w, c))
        if y % 16 == 0 or y % 2 == 1:
            img[y] = noisy  # a row nothing predicts, above every constructed row
        elif band == 1:
            img[y] = rng.randint(0, 2, size=(w, c)) * (np.arange(w)[:, None] % 2)
        elif band == 2:
            img[y] = (np.arange(w)[:, None] * 2 + 11 * np.arange(c)[None, :] + y) & 0xFF
        elif band == 3:
            img[y] = (img[y - 1] + rng.randint(0, 2, size=(w, c))) & 0xFF
        elif band == 4:
            for x in range(w):
                left = img[y, x - 1] if x else np.zeros(c, dtype=np.int64)
                img[y, x] = (left + img[y - 1, x]) >> 1
        else:
            for x in range(w):
                for k in range(c):
                    a = int(img[y, x - 1, k]) if x else 0
                    cc = int(img[y - 1, x - 1, k]) if x else 0
                    img[y, x, k] = _paeth(a, int(img[y - 1, x, k]), cc)
    return img.astype(np.uint8)


def limit():
    """~18 KB of grey for filter 0 whose symbol counts are the Fibonacci numbers 1, 1, 2, 3, ... 6765, so that an unlimited
    Huffman code is a chain deeper than 15: the end-of-block symbol is one of the ones, the 144 filter bytes (literal 0) are
    the 144, the pixels are the others."""
    fib = [1, 2]
    while fib[-1] < 6765:
        fib.append(fib[-1] + fib[-2])
    rows = 144
    counts = [n for n in fib if n != rows]
    counts[-1] += -sum(counts) % rows  # (whole rows: the most frequent byte, the chain's top, takes the difference)
    ordered = np.concatenate([np.full(n, 3 + 2 * k, dtype=np.uint8) for k, n in reversed(list(enumerate(counts)))])
    width = len(ordered) // rows
    data = np.zeros_like(ordered)  # dealt onto the even, then the odd places: no byte repeats, so every one is a literal
    half = (len(ordered) + 1) // 2
    data[0::2], data[1::2] = ordered[:half], ordered[half:]
    return data.reshape(-1, width)


def smooth_noise():
    """96 x 128 RGB: a smooth surface with two bits of noise"""
    rng = np.random.RandomState(3)
    y, x = np.mgrid[0:128, 0:96]
    base = (128 + 100 * np.sin(x / 23.0) * np.cos(y / 31.0)).astype(np.int64)[:, :, None] + 9 * np.arange(3)[None, None, :]
    return ((base + rng.randint(0, 4, size=(128, 96, 3))) & 0xFF).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def scenes():
    """name -> (pixels, filter)"""
    rng = np.random.RandomState(5)
    s = {
        "grey_1x1": (np.array([[77]], dtype=np.uint8), ref_png.FILTER_ADAPTIVE),
        "rgba_1x1": (np.array([[[1, 2, 3, 4]]], dtype=np.uint8), ref_png.FILTER_ADAPTIVE),
        "column_1x300": ((np.arange(300) * 7 % 251).astype(np.uint8).reshape(300, 1), ref_png.FILTER_ADAPTIVE),
        "runs": (runs(), ref_png.FILTER_NONE),
        "adaptive": (adaptive(), ref_png.FILTER_ADAPTIVE),
        "limit": (limit(), ref_png.FILTER_NONE),
        "wide_row": (np.full((3, 20000, 4), 0xFF, dtype=np.uint8), ref_png.FILTER_NONE),
        "tall_3x1025": (rng.randint(0, 256, size=(1025, 3, 3)).astype(np.uint8), ref_png.FILTER_ADAPTIVE),  # pure noise
        # more rows than one launch has waves (CVHIP_MESH_GRID_LANES / 64 = 4096): a wave takes a second row; every third row flat
        "tall_6x4500": ((rng.randint(0, 256, size=(4500, 6)) * (np.arange(4500)[:, None] % 3 > 0) + 9).astype(np.uint8), ref_png.FILTER_SUB),
        "flat": (np.full((120, 256, 3), 90, dtype=np.uint8), ref_png.FILTER_ADAPTIVE),
        "smooth_noise": (smooth_noise(), ref_png.FILTER_ADAPTIVE),
        "run_seams": (run_seams(), ref_png.FILTER_NONE),
        # more rows than Adler's modulus 65521: the trailer's reduction of the rows behind a row, and 18 rows a wave
        "column_1x70000": ((np.arange(70000) * 7 % 251).astype(np.uint8).reshape(70000, 1), ref_png.FILTER_NONE),
    }
    for w in RUN_END_PAST:
        s["run_ends_%d" % w] = (run_ends(w), ref_png.FILTER_NONE)
    for c in (1, 2, 3, 4):
        s["channels_%d" % c] = (channels(c), ref_png.FILTER_ADAPTIVE)
        for k in range(5):
            if c in (1, 3) or k == 4:
                s["channels_%d_filter_%d" % (c, k)] = (channels(c), k)
    return s


# the scenes that hold noise only: the encoder has no stored-block fallback, so their files may exceed stored blocks
NOISE = ("tall_3x1025", "tall_6x4500")


@functools.lru_cache(maxsize=None)
def restated(name):
    """ref_png.encode of a scene, computed once"""
    pixels, kind = scenes()[name]
    return ref_png.encode(pixels, kind)
