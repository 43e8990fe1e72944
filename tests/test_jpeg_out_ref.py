"""tests/ref_jpeg_out.py, the definition of cvhip_jpeg_encode's file, against Pillow on libjpeg-turbo: the WHOLE file of every
scene (tests/jpeg_out_scenes.py) equals what PIL.Image.save writes at the scene's quality, sampling and optimize setting, and
Pillow and tests/ref_jpeg.py (the decoder's restatement) decode it to the same pixels.  And from the restatement's own
counters: every scene reaches the case it is there for."""
import io

import numpy as np
import pytest
from PIL import Image, features

import jpeg_out_scenes
import ref_jpeg
import ref_jpeg_out

NAMES = sorted(jpeg_out_scenes.scenes())


def pillow_file(pixels, quality, sampling, optimize):
    buf = io.BytesIO()
    Image.fromarray(jpeg_out_scenes.opaque(pixels)).save(buf, format="JPEG", quality=quality, subsampling=sampling, optimize=optimize)
    return buf.getvalue()


def test_pillow_is_built_on_libjpeg_turbo():
    assert features.check_feature("libjpeg_turbo")


@pytest.mark.parametrize("name", NAMES)
def test_restated_file_is_pillows(name):
    """A grey scene's sampling is 4:4:4: the encoder ignores the argument for one component and its SOF0 says 1x1, where Pillow
    would record the argument's factors there (the only byte that differs; test_grey_ignores_sampling)."""
    pixels, quality, sampling, optimize = jpeg_out_scenes.scenes()[name]
    want = pillow_file(pixels, quality, sampling, optimize)
    got = jpeg_out_scenes.restated(name)
    assert got["file"] == want
    sos = 10 if jpeg_out_scenes.opaque(pixels).ndim == 2 else 14  # the SOS segment ends the first section
    assert sum(got["sections"]) == len(want) and got["file"][got["sections"][0] - sos:][:2] == b"\xFF\xDA" and got["file"][-2:] == b"\xFF\xD9"


@pytest.mark.parametrize("name", NAMES)
def test_pillow_and_the_decoders_restatement_decode_it_alike(name):
    file = jpeg_out_scenes.restated(name)["file"]
    pixels = jpeg_out_scenes.opaque(jpeg_out_scenes.scenes()[name][0])
    pil = Image.open(io.BytesIO(file))
    want = np.asarray(pil.convert("RGB"))
    got = ref_jpeg.decode(file)
    assert got.shape == want.shape == (*pixels.shape[:2], 3)
    assert (got == want).all()


def test_grey_ignores_sampling():
    pixels, quality, _sampling, optimize = jpeg_out_scenes.scenes()["last_byte_ff"]
    files = [ref_jpeg_out.encode(pixels, quality, s, optimize)["file"] for s in (0, 1, 2)]
    assert files[0] == files[1] == files[2]
    theirs = pillow_file(pixels, quality, 2, optimize)
    differ = [k for k, (a, b) in enumerate(zip(files[0], theirs)) if a != b]
    assert len(theirs) == len(files[0]) and differ == [100] and (files[0][100], theirs[100]) == (0x11, 0x22)  # SOF0's factors


def test_alpha_is_dropped():
    for name, plain in jpeg_out_scenes.ALPHA_COPIES.items():
        assert jpeg_out_scenes.scenes()[name][0].shape[2] in (2, 4)
        assert jpeg_out_scenes.restated(name)["file"] == jpeg_out_scenes.restated(plain)["file"]


def stats(name):
    r = jpeg_out_scenes.restated(name)
    return r["stats"], r["met"]


def test_scenes_reach_their_cases():
    # the whole MCU is padding; at 4:2:0 three of the four luma blocks are dummies
    assert stats("grey_1x1")[0]["blocks"] == 1 and stats("rgb_1x1_444")[0] == {**stats("rgb_1x1_444")[0], "blocks": 3, "dummy_blocks": 0}
    assert (stats("rgb_1x1_422")[0]["blocks"], stats("rgb_1x1_422")[0]["dummy_blocks"]) == (4, 1)
    assert (stats("rgb_1x1_420")[0]["blocks"], stats("rgb_1x1_420")[0]["dummy_blocks"]) == (6, 3)
    # a dummy column and a dummy row: in one MCU, in MCUs below each other, in MCUs side by side
    assert stats("rgb_8x8_420")[0]["dummy_blocks"] == 3
    assert stats("rgb_8x24_420")[0]["dummy_blocks"] == 2 * 4 - 3 and stats("rgb_24x8_420")[0]["dummy_blocks"] == 2 * 4 - 3
    assert stats("rgb_9x17_420")[0]["dummy_blocks"] == 2 and stats("rgb_17x33_420")[0]["dummy_blocks"] == 4 * 6 - 3 * 5
    assert stats("rgb_9x9_422")[0]["dummy_blocks"] == 0 and stats("rgb_9x9_422")[0]["blocks"] == 2 * 4
    # the clamp at 255, both sides of the switch of the scale's formula, tables of ones
    assert jpeg_out_scenes.restated("quality_1")["quants"][0].max() == 255 and jpeg_out_scenes.restated("quality_1")["quants"][0].min() == 255
    assert jpeg_out_scenes.restated("quality_49")["quants"][0][0] == (16 * (5000 // 49) + 50) // 100
    assert jpeg_out_scenes.restated("quality_50")["quants"][0][0] == 16 and jpeg_out_scenes.restated("quality_51")["quants"][0][0] == (16 * 98 + 50) // 100
    assert all((q == 1).all() for q in jpeg_out_scenes.restated("quality_100")["quants"])
    # AC category 10, a coefficient 63 that is not zero, a long block (see the module's note on how long a block can be)
    st, met = stats("noise_16x16_q100")
    assert met["ac_category"] == 10 and met["coef63"] >= 1 and met["longest_block"] > 900
    # DC differences of category 11 in both signs
    st, met = stats("dc_swing_8x64_q100")
    assert met["dc_category"].get(11, 0) >= 3 and met["dc_category"].get(-11, 0) >= 3
    st, met = stats("noise_32x32_q1")
    assert met["zrl"] >= 1 and met["eob"] >= 1
    # 6-bit blocks, many to a dword; with optimize every table holds one symbol
    st, met = stats("flat_64x64")
    assert met["shortest_block"] <= 6 and st["bits"] < 8 * st["blocks"]
    assert all(sum(bits) == 1 for bits, _values in jpeg_out_scenes.restated("flat_64x64_optimize")["tables"])
    assert stats("adjacent_ff")[1]["adjacent_ff"] and stats("last_byte_ff")[1]["last_byte_ff"]
    st, met = stats("tile_end_ff")
    assert met["tile_end_ff"] and met["raw_bytes"] > ref_jpeg_out.STUFF_TILE
    assert jpeg_out_scenes.restated("last_byte_ff")["file"][-4:] == b"\xFF\x00\xFF\xD9"
    # more blocks than a workgroup's lanes, and than one step of the scan (1024); more than one stuffing tile
    assert stats("grey_strip_8x40000")[0]["blocks"] == 5000 and stats("rgb_2048x24_420")[0]["blocks"] == 1536
    assert stats("rgb_2048x24_420")[0]["dummy_blocks"] == 256 and stats("grey_strip_8x40000")[1]["raw_bytes"] > 4 * ref_jpeg_out.STUFF_TILE
    assert any(jpeg_out_scenes.restated(n)["stats"]["stuffed"] for n in NAMES)


def test_no_block_can_pass_1500_bits_under_the_annex_k_tables():
    """The figure behind `longest_block > 900` above.  The DCT keeps the energy of a block: sum of c^2 <= 64 * 128^2.  Under the
    Annex K luma table a coefficient of category n costs code + n bits: 3, 4, 6, 8, 10, 13, 15, 18, 25, 26 for n = 1 .. 10, and
    needs |c| >= 2^(n-1); the most bits for the energy is 63 coefficients of category 8 - 63 * 18 + 27 for the DC = 1161 - so no
    block reaches 1500, and binary noise comes to about 1000."""
    table = ref_jpeg_out.code_table(*ref_jpeg_out.AC_LUMA)
    cost = {n: table[n][1] + n for n in range(1, 11)}
    assert [cost[n] for n in range(1, 11)] == [3, 4, 6, 8, 10, 13, 15, 18, 25, 26]
    budget = 64 * 128 ** 2
    most = 0  # over the mixes of two categories: as many of the higher one as the energy allows, the rest of the lower one
    for n in range(1, 11):
        fit = min(63, budget // (1 << (n - 1)) ** 2)
        rest = budget - fit * (1 << (n - 1)) ** 2
        for m in range(1, n):  # the remaining places filled with one lower category
            more = min(63 - fit, rest // (1 << (m - 1)) ** 2)
            most = max(most, fit * cost[n] + more * cost[m])
        most = max(most, fit * cost[n])
    assert most + 27 < 1500
