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


STEP, LOOK, CHUNK = 64, 320, 258  # row_tokens in png_kernels.hip: positions a step, bytes it can look past a step, the longest match
RUN_SCENES = ["run_seams"] + ["run_ends_%d" % w for w in png_scenes.RUN_END_PAST]


def row_runs(row):
    """[(first repeating position, one past the last)] of the maximal runs of a row's filtered bytes"""
    rep = np.flatnonzero(row[1:] == row[:-1]) + 1
    cuts = np.flatnonzero(np.diff(rep) > 1) + 1
    return [(int(r[0]), int(r[-1]) + 1) for r in np.split(rep, cuts) if len(r)]


def row_looks(row):
    """The steps in which the wave looks past the step, from the filtered bytes alone: [(past, at_row_end, by_start)].  A token
    begins at a run's position 0 or 1 modulo 258 only, and such a position needs the run's length ahead of it; so the wave looks
    in a step iff one of them lies in the step, the run goes on to the step's lane 63 and the row goes on behind the step.
    past = the run's positions behind the step, at most 320; at_row_end: the run ends with the row, inside the window;
    by_start: the position that asks is the run's own first, at lane 62 or 63 (the first step in which a run can look)."""
    n, out = len(row), []
    for first, end in row_runs(row):
        for base in range(first - first % STEP, end, STEP):
            asks = [q for q in range(max(first, base), base + STEP) if (q - first) % CHUNK <= 1]
            if asks and end >= base + STEP and base + STEP < n:
                past = min(LOOK, end - (base + STEP))
                out.append((past, end == n and past < LOOK, asks[0] == first and first % STEP >= STEP - 2))
    return out


def row_rests(row):
    """[(literals, lane of the first)] of the rests of one or two literals behind a run's last match of 258, where the run
    began in an earlier step: the lane's offset in its chunk comes from the carry between the steps"""
    return [((end - first) % CHUNK, (end - (end - first) % CHUNK) % STEP) for first, end in row_runs(row)
            if end - first > CHUNK and (end - first) % CHUNK in (1, 2)]


def test_run_scenes_are_what_their_names_say():
    """(guards the scene builder, as the check of `runs` above does)"""
    f = png_scenes.restated("run_seams")["filtered"]
    pairs = [(s, run) for s in png_scenes.SEAM_STARTS for run in png_scenes.SEAM_RUNS]
    assert f.shape == (517, 1000) == (len(pairs), png_scenes.SEAM_WIDTH + 1) and (f[:, 0] == 0).all()
    for row, (s, run) in zip(f, pairs):
        assert row_runs(row) == [(s, s + run)]
        matches, rest = [], run
        while rest >= 3:
            matches.append(ref_png.TOKEN_MATCH + min(rest, CHUNK) - 3)
            rest -= min(rest, CHUNK)
        want = [int(v) for v in row[:s]] + matches + [200] * rest + [int(v) for v in row[s + run:]]
        assert ref_png.row_tokens(row) == want, (s, run)
    for w, d in png_scenes.RUN_END_PAST.items():
        f = png_scenes.restated("run_ends_%d" % w)["filtered"]
        assert f.shape == (4, w + 1) == (4, 2 * STEP + d) and (f[:, 0] == 0).all()
        for row, s in zip(f, png_scenes.RUN_END_STARTS):
            assert row_runs(row) == [(s, w + 1)] and s % STEP >= STEP - 2 and row[-1] == 0  # (0: the byte behind the row, too)


def test_run_scenes_reach_every_look():
    """The look past a step (`past = first * LOOK_BYTES + same`, five bytes a lane) in every shape, over run_seams and the
    run_ends scenes together and by the looks of runs that START at lane 62 or 63: no byte of the run behind the step; a break
    in the first lane's five bytes, at each of them; in lanes 1, 2, 51 and 63; a run of exactly 257 behind the step, and of 320
    or more; a run that ends where the row ends, inside the window; and no look where the row ends with the step.  Beyond
    those: a look asked for by a position 258 into its run, and rests of one and of two literals on lanes 0 and 1."""
    looks, rests = [], []
    for name in RUN_SCENES:
        for row in png_scenes.restated(name)["filtered"]:
            looks += row_looks(row)
            rests += row_rests(row)
    by_start = [look for look in looks if look[2]]
    pasts = {past for past, _end, _start in by_start}
    assert {0, 1, 2, 3, 4} <= pasts                                  # first == 0, every `same`
    for first in (1, 2, 51, 63):
        assert pasts & set(range(5 * first, 5 * first + 5)), first
    assert 257 in pasts and max(pasts) == LOOK and 319 in pasts
    ends = {past for past, end, _start in by_start if end}
    assert {1, 4, 5, 6, 12, 257, 319} <= ends                        # the bound q + k < n in the first lane, in later ones, in the last
    assert any(not start for _past, _end, start in looks)
    assert not row_looks(png_scenes.restated("run_ends_127")["filtered"][0])  # the row ends with the step: nothing to look at
    assert {(1, 0), (1, 1), (2, 0), (2, 1)} <= set(rests)
    # the earlier scenes, for the record: `runs` looks from lane 2 (a run of 258 has 196 positions behind its step), wide_row's
    # one run ends with its row, 257 and then 1 byte behind its last two looks
    assert {past for row in png_scenes.restated("runs")["filtered"] for past, _e, _s in row_looks(row)} == {196, 197, 198, 199, LOOK}
    assert {past for row in png_scenes.restated("wide_row")["filtered"] for past, _e, _s in row_looks(row)} == {1, 257, LOOK}


def test_column_has_more_rows_than_adlers_modulus():
    height = png_scenes.restated("column_1x70000")["filtered"].shape[0]
    assert height == 70000 > 65521 and (height - 1) % 65521 != height - 1  # (the rows behind row 0, reduced)


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
