"""tests/ref_tiff_out.py, the definition of cvhip_tiff_encode, against what can read or write the same file
on the CPU: ref_tiff.samples and Pillow read every scene's file back to the pixels; every LZW strip equals the strip libtiff
(through Pillow) writes for the same rows, RowsPerStrip and predictor - the strip whose last code is the 3836th since a
Clear included, where libtiff puts a Clear in front of EOI; the PackBits closed form equals the greedy walk."""
import io

import numpy as np
import pytest

import ref_tiff
import ref_tiff_out as R
import tiff_out_scenes as S

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
