"""tests/ref_png.py - the definition of cvhip_png_encode's file - against decoders that share nothing with
it: zlib and Pillow must return the input exactly.  And the scenes (tests/png_scenes.py) against the cases they are there
for, on the restatement alone.  No GPU."""
import heapq
import io
import struct
import zlib
from fractions import Fraction

import numpy as np
import pytest
from PIL import Image

import png_scenes
import ref_png

NAMES = sorted(png_scenes.scenes())
MODES = {1: "L", 2: "LA", 3: "RGB", 4: "RGBA"}


def chunks(file: bytes):
    assert file[:8] == ref_png.SIGNATURE
    at, out = 8, []
    while at < len(file):
        (n,) = struct.unpack(">I", file[at:at + 4])
        out.append((file[at + 4:at + 8], file[at + 8:at + 8 + n], struct.unpack(">I", file[at + 8 + n:at + 12 + n])[0]))
        at += 12 + n
    assert at == len(file)
    return out


@pytest.mark.parametrize("name", NAMES)
def test_independent_decoders_return_the_input(name):
    pixels, kind = png_scenes.scenes()[name]
    r = png_scenes.restated(name)
    p = ref_png.as_image(pixels)
    h, w, c = p.shape
    parts = chunks(r["file"])
    assert [k for k, _d, _c in parts] == [b"IHDR", b"IDAT", b"IEND"]
    for k, d, crc in parts:
        assert crc == zlib.crc32(k + d)
    assert parts[0][1] == struct.pack(">IIBBBBB", w, h, 8, ref_png.COLOUR_TYPE[c], 0, 0, 0)
    idat = parts[1][1]
    assert r["sections"] == (41, len(idat), 16) and sum(r["sections"]) == len(r["file"])
    assert idat[:2] == b"\x78\x01"
    raw = r["filtered"].tobytes()
    assert zlib.decompress(idat) == raw
    assert struct.unpack(">I", idat[-4:])[0] == zlib.adler32(raw) == ref_png.adler32(raw)
    if kind != ref_png.FILTER_ADAPTIVE:
        assert (r["filtered"][:, 0] == kind).all()
    im = Image.open(io.BytesIO(r["file"]))
    im.load()
    assert im.mode == MODES[c] and im.size == (w, h)
    assert (np.asarray(im).reshape(h, w, c) == p).all()


@pytest.mark.parametrize("name", NAMES)
def test_codes_are_complete_and_within_their_limits(name):
    r = png_scenes.restated(name)
    lengths = r["litlen_lengths"]
    used = [n for n in lengths if n]
    assert max(used) <= 15 and sum(Fraction(1, 1 << n) for n in used) == 1
    assert all((n > 0) == (f > 0) for n, f in zip(lengths, r["histogram"]))
    cl = [n for n in r["header"]["cl_lengths"] if n]
    assert max(cl) <= 7 and sum(Fraction(1, 1 << n) for n in cl) == 1
    assert 4 <= r["header"]["hclen"] <= 19 and 257 <= r["header"]["hlit"] <= 286


def huffman_depth(freqs):
    """the deepest leaf of an unlimited Huffman code"""
    heap = [(f, 0) for f in freqs if f]
    heapq.heapify(heap)
    while len(heap) > 1:
        a, b = heapq.heappop(heap), heapq.heappop(heap)
        heapq.heappush(heap, (a[0] + b[0], max(a[1], b[1]) + 1))
    return heap[0][1]


def test_scenes_reach_their_cases():
    r = png_scenes.restated("adaptive")
    chosen = set(int(v) for v in r["filtered"][:, 0])
    assert chosen == {0, 1, 2, 3, 4}, chosen
    assert any(sorted(sc)[0] == sorted(sc)[1] for sc in r["scores"])  # a tie for the best score
    r = png_scenes.restated("limit")
    assert huffman_depth(r["histogram"]) > 15 and max(r["litlen_lengths"]) == 15
    for name in ("grey_1x1", "rgba_1x1"):
        r = png_scenes.restated(name)
        assert r["header"]["hlit"] == 257 and sum(r["histogram"][257:]) == 0
    r = png_scenes.restated("runs")
    assert r["header"]["hlit"] == 286
    for y, run in enumerate(png_scenes.RUNS):  # each row's run is exactly as long as its name says
        row = r["filtered"][y]
        rep = np.flatnonzero(row[1:] == row[:-1]) + 1
        assert len(rep) == run and (rep == np.arange(2, 2 + run)).all()
    want = {2: [200, 200], 3: [256], 4: [257], 258: [511], 259: [511, 200], 260: [511, 200, 200], 261: [511, 256],
            516: [511, 511], 517: [511, 511, 200]}
    for y, run in enumerate(png_scenes.RUNS):
        assert ref_png.row_tokens(r["filtered"][y])[2:2 + len(want[run])] == want[run]
    r = png_scenes.restated("wide_row")
    assert r["filtered"].shape == (3, 80001)
    assert 255 * 80001 * 80001 // 2 > 1 << 32  # a row's weighted Adler sum does not fit in 32 bits


@pytest.mark.parametrize("name", ["flat", "smooth_noise"])
def test_smaller_than_stored_blocks(name):
    """(the pure-noise scenes are exempt: there is no stored-block fallback, png_scenes.NOISE)"""
    r = png_scenes.restated(name)
    assert name not in png_scenes.NOISE
    assert r["sections"][1] < ref_png.stored_size(r["filtered"].size)


def test_length_symbols_are_the_rfcs():
    for length in range(3, 259):
        s, extra, value = ref_png.length_symbol(length)
        assert ref_png.LENGTH_BASE[s - 257] + value == length and 0 <= value < (1 << extra) or (extra == 0 and value == 0)
    assert ref_png.length_symbol(258) == (285, 0, 0) and ref_png.length_symbol(257) == (284, 5, 30)
    assert ref_png.crc32(b"IEND") == zlib.crc32(b"IEND") == 0xAE426082
