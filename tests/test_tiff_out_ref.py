"""tests/ref_tiff_out.py, the definition of cvhip_tiff_encode, against what can read or write the same file
on the CPU: ref_tiff.samples and Pillow read every scene's file back to the pixels; every LZW strip equals the strip libtiff
(through Pillow) writes for the same rows, RowsPerStrip and predictor - the strip whose last code is the 3836th since a
Clear included, where libtiff puts a Clear in front of EOI; the PackBits closed form equals the greedy walk; the scenes reach
the seams they are named for - of the format, of the LZW kernel's staging (ref_tiff_out.lzw_stagings) and of the launches."""
import io

import numpy as np
import pytest

import ref_tiff
import ref_tiff_out as R
import tiff_out_scenes as S
from cybervision_amd import mesh  # (GRID_LANES only: importing it loads no library)

MODES = {1: "L", 2: "LA", 3: "RGB", 4: "RGBA"}


@pytest.mark.parametrize("name", S.names())
def test_file_reads_back(name):
    pixels, compression, predictor, rps = S.scene(name)
    data, stats, sections = S.expected(name)
    h, w, c = pixels.shape
    if c != 2:   # (cvhip_tiff_decode and its restatement refuse 2 samples)
        header, samples = ref_tiff.samples(data)
        assert np.array_equal(samples, pixels)
        assert (header["compression"], header["predictor"], header["strips"]) == (compression, predictor, stats["strips"])
    from PIL import Image

    img = Image.open(io.BytesIO(data))
    assert img.mode == MODES[c] and img.size == (w, h)
    assert np.array_equal(np.asarray(img).reshape(h, w, c), pixels)
    assert sections[0] + sections[1] == len(data) and sections[2] == 0
    offsets = R.strips_of(data)
    assert offsets[0][0] == sections[0] and all(o % 2 == 0 for o, _ in offsets)
    assert all(o + n + ((o + n) & 1) == o2 for (o, n), (o2, _) in zip(offsets, offsets[1:]))


def pillow_strips(pixels, predictor, rps):
    from PIL import Image, TiffImagePlugin

    h, w, c = pixels.shape
    info = TiffImagePlugin.ImageFileDirectory_v2()
    info[278] = rps
    if predictor == 2:
        info[317] = 2
    buf = io.BytesIO()
    Image.fromarray(pixels[:, :, 0] if c == 1 else pixels).save(buf, format="TIFF", compression="tiff_lzw", tiffinfo=info)
    data = buf.getvalue()
    tags = Image.open(io.BytesIO(data)).tag_v2
    assert tags[278] == rps and tags.get(317, 1) == predictor
    return [data[o:o + n] for o, n in zip(tags[273], tags[279])]


@pytest.mark.parametrize("name", S.lzw_names())
def test_lzw_strips_are_libtiffs(name):
    pixels, compression, predictor, rps = S.scene(name)
    data, stats, _ = S.expected(name)
    row_bytes, rows, strips = R.check(pixels.shape[1], pixels.shape[0], pixels.shape[2], compression, predictor, rps)
    theirs = pillow_strips(pixels, predictor, rows)
    ours = [data[o:o + n] for o, n in R.strips_of(data)]
    assert len(ours) == len(theirs) == strips
    assert ours == theirs


def test_clear_in_front_of_eoi():
    """The strip whose last code is the 3836th since the Clear: Clear, then EOI of 9 bits - libtiff's bytes (above) decide."""
    for n, clears in ((3835, 1), (3836, 2), (3837, 2)):
        codes = R.lzw_codes(S.noise_strip(n).tobytes())
        assert codes.count(R.CLEAR) == clears
        assert codes[-1] == R.EOI and (codes[-2] == R.CLEAR) == (n == 3836)


def test_scene_seams():
    for c in (253, 254, 255, 765, 766, 767, 1789, 1790, 1791):
        assert len(R.lzw_codes(S.scene("lzw_width_%d" % c)[0].tobytes())) == c + 2
    assert S.expected("lzw_noise_8192_one_strip")[1]["clears"] >= 2 and S.expected("lzw_noise_8192_one_strip")[1]["strips"] == 1
    for tail in range(1, 8):
        codes = R.lzw_codes(S.scene("lzw_tail_%d" % tail)[0][0].tobytes())
        assert 9 * len(codes) % 8 == tail and len(R.lzw_pack(codes)) % 2 == 1
    assert [S.expected(n)[1]["strips"] for n in ("one_strip_raw", "two_strips_raw_rgb", "strips_64_lzw", "strips_65_lzw", "strips_256_lzw",
                                                "strips_257_lzw", "strips_1025_lzw")] == [1, 2, 64, 65, 256, 257, 1025]
    assert [R.check(w, 3, 4, R.LZW, 1, 0)[1] for w in (2047, 2048, 2049)] == [1, 1, 1] and R.default_rows_per_strip(33) == 248
    assert S.scene("lzw_strip_64k")[0].size == 65536 > S.LZW_STAGE
    lengths = {(run, n) for row in S.scene("pb_seams")[0] for run, _, n in R.packbits_row(row.tobytes())}
    assert {(True, 3), (True, 127), (True, 128), (False, 127), (False, 128)} <= lengths
    assert S.expected("pb_two_flat_rows")[1]["packets"] == 2
    staging_seams()
    launch_seams()


def stagings(name):
    """lzw_stagings of every strip of the scene, at the kernel's staging size."""
    return [R.lzw_stagings(strip, S.LZW_STAGE) for strip in S.strip_bytes(name)]


def test_staging_restatement():
    """lzw_stagings against lzw_codes and lzw_pack: the codes in order, every byte accounted for (asserted inside), a staging a
    strip when the stage is the strip, and at a stage of 1 byte each code with the byte behind its string."""
    data = S.noise(5000, 44).tobytes() + bytes(300) + S.noise(3000, 45).tobytes()
    codes = R.lzw_codes(data)
    for stage in (1, 7, S.LZW_STAGE, len(data) - 1, len(data), len(data) + 1):
        st = R.lzw_stagings(data, stage)
        assert len(st) == -(-len(data) // stage) and [c for s in st for c in s["codes"]] == codes
        assert st[-1]["end"] == sum(ref_tiff.code_width(c) for c in widths_index(codes)) % 32
    one = R.lzw_stagings(data, 1)
    assert one[0]["codes"] == [R.CLEAR] and one[1]["codes"] == [data[0]] and one[-1]["codes"][-1] == R.EOI
    assert [s["clears"] for s in one if s["clears"]] == [[0]] * (codes.count(R.CLEAR) - 1)
    assert len(R.lzw_stagings(b"\x05", S.LZW_STAGE)) == 1 and R.lzw_stagings(b"\x05", S.LZW_STAGE)[0]["codes"] == [R.CLEAR, 5, R.EOI]


def widths_index(codes):
    c = 0
    for code in codes:
        yield c
        c = 0 if code == R.CLEAR else c + 1


def staging_seams():
    """The LZW scenes on the seams of the kernel's staging (S.LZW_STAGE bytes at a time), by lzw_stagings."""
    stage = S.LZW_STAGE
    D = S.pair_distinct()
    pairs = list(zip(D[:-1].tolist(), D[1:].tolist()))
    assert len(D) == 65280 and len(set(pairs)) == len(pairs)   # no two adjacent pairs equal: a code a byte
    # ---- the codes of a staging, strips beside a multiple of the staging
    counts = {1023: [1025], 1024: [1026], 1025: [1024, 3], 2047: [1024, 1025], 2048: [1024, 1026], 2049: [1024, 1024, 3],
              4096: [1024, 1024, 1024, 1027]}
    for n, want in counts.items():
        pixels = S.scene("lzw_dense_%d" % n)[0]
        assert pixels.shape == (1, n, 1) and pixels.tobytes() == D[:n].tobytes()
        st, = stagings("lzw_dense_%d" % n)
        assert [len(s["codes"]) for s in st] == want
    st, = stagings("lzw_dense_4096")
    assert st[3]["clears"] == [R.CLEAR_AFTER % stage] and R.CLEAR_AFTER // stage == 3   # the Clear leaves with byte 3836
    # the bound on a staging's codes: a code for each of its bytes, one Clear - the strip's first or one at table-full, which
    # are CLEAR_AFTER codes apart and so never in one staging -, then the pending string, a Clear behind it and EOI.  The
    # last two Clears cannot both occur either, so the most that is reached is one less
    most = stage + 1 + 3
    assert R.CLEAR_AFTER > most and most < stage + 8   # LZW_CHUNK_CODES of tiff_encode_common.hpp
    assert max(len(s["codes"]) for n in S.lzw_names() for strip in stagings(n) for s in strip) == most - 1 == 1027
    # ---- a table-full Clear with the last and the first bytes of a staging
    for r, k in ((1022, 3), (1023, 3), (0, 4), (1, 4)):
        pixels = S.scene("lzw_clear_at_%d" % r)[0]
        assert pixels.shape == (1, 6000, 1)
        st, = stagings("lzw_clear_at_%d" % r)
        assert [(j, s["clears"]) for j, s in enumerate(st) if s["clears"]] == [(k, [r % stage])]
        lead = int(np.argmax(pixels.ravel() != 0x80))
        assert lead in S.CLEAR_AT_WINDOW and pixels.ravel()[lead:].tobytes() == D[:6000 - lead].tobytes()
    # ---- strips of 12 stagings close to their scratch stride
    pixels, _, _, rps = S.scene("lzw_dense_strips")
    assert pixels.shape == (85, 768, 1) and rps == 16 and pixels.tobytes() == D.tobytes()
    sizes = [n for _, n in R.strips_of(S.expected("lzw_dense_strips")[0])]
    assert len(sizes) == 6 and [len(st) for st in stagings("lzw_dense_strips")] == [12] * 5 + [4]
    # a code a byte at 9 to 12 bits against the bound's 12: 43222 of 46032 bits over the 3836 codes between two Clears
    assert all(0.93 * R.worst_strip(R.LZW, 16, 768) < n <= R.worst_strip(R.LZW, 16, 768) for n in sizes[:5])
    # ---- stagings without a code
    st, = stagings("lzw_flat_640k")
    assert len(st) == 640 and sum(len(s["codes"]) for s in st) == 1147 == S.expected("lzw_flat_640k")[1]["codes"]
    empty = [k for k, s in enumerate(st) if not s["codes"]]
    assert len(empty) == 7 and all(st[k]["end"] == st[k - 1]["end"] != 0 for k in empty)   # (a partial word is carried through)
    # ---- every carried bit count at a staging's end; a last code of a staging in two words
    ends, crossing = set(), 0
    for n in S.lzw_names():
        for strip in stagings(n):
            ends |= {s["end"] for s in strip[:-1]}
            crossing += sum(s["crosses"] and bool(s["codes"]) for s in strip[:-1])
    assert ends == set(range(32)) and crossing >= 1
    # ---- Predictor 2 across rows that start in mid-staging
    for name, row_bytes in (("pred_rows_1023", 1023), ("pred_rows_1028", 1028), ("pred_rows_1025", 1025)):
        pixels, compression, predictor, rps = S.scene(name)
        assert (pixels.shape[0], pixels.shape[1] * pixels.shape[2], compression, predictor, rps) == (5, row_bytes, R.LZW, 2, 5)
        assert all((r * row_bytes) % stage != 0 for r in range(1, 5)) and S.expected(name)[1]["strips"] == 1


def launch_seams():
    """The scenes past one launch of tiff_lzw_kernel (a wave a strip) and of tiff_copy_kernel (a workgroup a unit), the most rows
    and the widest row, and the PackBits runs on either side of lane 64 and workgroup 256 of a row."""
    T, U = mesh.GRID_LANES // 64, mesh.GRID_LANES // 256
    pixels, compression, _, rps = S.scene("strips_lzw_second_trip")
    assert pixels.shape == (T + 6, 40, 1) and (compression, rps) == (R.LZW, 1) and S.expected("strips_lzw_second_trip")[1]["strips"] == T + 6
    assert (pixels[T:] == pixels[:6]).all() and len({row.tobytes() for row in pixels[:T]}) == T
    for name, compression in (("strips_65535_lzw", R.LZW), ("strips_65535_packbits", R.PACKBITS)):
        assert S.scene(name)[0].shape == (65535, 1, 1) and S.scene(name)[1:] == (compression, 1, 1)
        assert S.expected(name)[1]["strips"] == 65535 > 15 * T and 65535 > 63 * U
        with pytest.raises(R.TiffOutError):
            R.check(1, 65536, 1, compression, 1, 1)
    assert 65535 < mesh.GRID_LANES   # a lane a row or a strip (tiff_packbits_kernel, tiff_sizes_kernel, tiff_table_kernel): one trip
    pixels, compression, _, rps = S.scene("pb_rows_second_trip")
    assert pixels.shape == (U + 6, 37, 1) and (compression, rps) == (R.PACKBITS, 7) and U % 7 != 0 and (U + 6) % 7 != 0
    assert set(np.unique(pixels)) == {0, 1, 2}
    for name, compression, predictor in (("widest_rgba_packbits", R.PACKBITS, 1), ("widest_rgba_lzw_pred", R.LZW, 2)):
        pixels, cmp_, pred, rps = S.scene(name)
        assert pixels.shape == (2, 65535, 4) and (cmp_, pred, rps) == (compression, predictor, 0)
        assert R.check(65535, 2, 4, compression, predictor, 0) == (262140, 1, 2)
        with pytest.raises(R.TiffOutError):
            R.check(65536, 2, 4, compression, predictor, 0)
    kinds = {run for row in S.scene("widest_rgba_packbits")[0].reshape(2, -1) for run, _, _ in R.packbits_row(row.tobytes())}
    assert kinds == {True, False} and S.expected("widest_rgba_lzw_pred")[1]["clears"] > 2
    rows = S.scene("pb_seam_sweep")[0]
    assert S.PB_SWEEP == [(n, p) for n in (2, 3, 4, 128, 129, 130, 131) for p in (*range(61, 67), *range(253, 259))]
    assert rows.shape == (len(S.PB_SWEEP), 700, 1)
    for (n, p), row in zip(S.PB_SWEEP, rows.reshape(len(rows), -1)):
        runs = [(at, length) for run, at, length in R.packbits_row(row.tobytes()) if run]
        assert runs == {2: [], 3: [(p, 3)], 4: [(p, 4)], 128: [(p, 128)], 129: [(p, 128)], 130: [(p, 128)], 131: [(p, 128), (p + 128, 3)]}[n]
        assert (row[p:p + n] == 255).all() and row[p - 1] != 255 and row[p + n] != 255


@pytest.mark.parametrize("name,code", [(k, v[1]) for k, v in S.REFUSED.items()])
def test_refusals(name, code):
    with pytest.raises(R.TiffOutError) as e:
        R.check(*S.REFUSED[name][0])
    assert e.value.code == code


def test_packbits_closed_form():
    rows = [row.tobytes() for n in S.names() if S.scene(n)[1] == R.PACKBITS for row in S.scene(n)[0].reshape(S.scene(n)[0].shape[0], -1)]
    rng = np.random.default_rng(3)
    rows += [rng.integers(0, 2, size=int(rng.integers(1, 40)), dtype=np.uint8).tobytes() for _ in range(3000)]
    rows += [(rng.integers(0, 40, size=int(rng.integers(250, 700))) == 0).astype(np.uint8).tobytes() for _ in range(300)]
    for row in rows:
        walk = R.packbits_row(row)
        assert R.packbits_row_closed(row) == walk
        assert ref_tiff.unpackbits(R.packbits_bytes(row, walk), len(row)) == row
