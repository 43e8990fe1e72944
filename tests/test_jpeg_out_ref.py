"""tests/ref_jpeg_out.py, the definition of cvhip_jpeg_encode's file, against Pillow on libjpeg-turbo: the WHOLE file of every
scene (tests/jpeg_out_scenes.py) equals what PIL.Image.save writes at the scene's quality, sampling and optimize setting, and
Pillow and tests/ref_jpeg.py (the decoder's restatement) decode it to the same pixels - but for the two scenes of 65535 pixels,
which Pillow refuses (asserted too).  And from the restatement's own counters: every scene reaches the case it is there for,
with the launch sizes taken from mesh.GRID_LANES and ref_jpeg_out.STUFF_TILE."""
import io

import numpy as np
import pytest
from PIL import Image, features

import jpeg_out_scenes
import ref_jpeg
import ref_jpeg_out
from cybervision_amd import mesh  # (GRID_LANES only: importing it loads no library)

NAMES = sorted(jpeg_out_scenes.scenes())
PILLOWS = [n for n in NAMES if n not in jpeg_out_scenes.OVERSIZE]  # the scenes that Pillow takes
TRANSFORM_BLOCKS = 32  # blocks a workgroup of jpeg_transform_kernel takes in one step (eight lanes a block)


def pillow_file(pixels, quality, sampling, optimize):
    buf = io.BytesIO()
    Image.fromarray(jpeg_out_scenes.opaque(pixels)).save(buf, format="JPEG", quality=quality, subsampling=sampling, optimize=optimize)
    return buf.getvalue()


def test_pillow_is_built_on_libjpeg_turbo():
    assert features.check_feature("libjpeg_turbo")


@pytest.mark.parametrize("name", PILLOWS)
def test_restated_file_is_pillows(name):
    """A grey scene's sampling is 4:4:4: the encoder ignores the argument for one component and its SOF0 says 1x1, where Pillow
    would record the argument's factors there (the only byte that differs; test_grey_ignores_sampling).  The two scenes of
    jpeg_out_scenes.OVERSIZE are not here: test_pillow_refuses_the_oversize_scenes."""
    pixels, quality, sampling, optimize = jpeg_out_scenes.scenes()[name]
    want = pillow_file(pixels, quality, sampling, optimize)
    got = jpeg_out_scenes.restated(name)
    assert got["file"] == want
    sos = 10 if jpeg_out_scenes.opaque(pixels).ndim == 2 else 14  # the SOS segment ends the first section
    assert sum(got["sections"]) == len(want) and got["file"][got["sections"][0] - sos:][:2] == b"\xFF\xDA" and got["file"][-2:] == b"\xFF\xD9"


def test_pillow_refuses_the_oversize_scenes():
    """what keeps them out of the two tests against Pillow: libjpeg stops at 65500, and Pillow cannot open such a file either"""
    assert set(jpeg_out_scenes.OVERSIZE) == set(NAMES) - set(PILLOWS) and len(jpeg_out_scenes.OVERSIZE) == 2
    for name in jpeg_out_scenes.OVERSIZE:
        pixels, quality, sampling, optimize = jpeg_out_scenes.scenes()[name]
        assert max(pixels.shape) == 65535 > 65500
        with pytest.raises(OSError):
            pillow_file(pixels, quality, sampling, optimize)
        with pytest.raises(OSError):
            Image.open(io.BytesIO(jpeg_out_scenes.restated(name)["file"])).load()


def test_oversize_scenes_say_their_size_and_decode_to_it():
    """SOF0 behind JFIF and one DQT: FF C0, length 11, precision 8, height, width - FF FF where the dimension is 65535 - and the
    decoder's restatement, which has no such limit, returns an image of that shape."""
    for name, (height, width) in (("grey_65535x8", (8, 65535)), ("grey_8x65535", (65535, 8))):
        file = jpeg_out_scenes.restated(name)["file"]
        assert jpeg_out_scenes.scenes()[name][0].shape == (height, width)
        at = file.index(b"\xFF\xC0")
        assert at == 2 + 18 + 69 and file[at + 2:at + 5] == b"\x00\x0B\x08"
        assert file[at + 5:at + 9] == height.to_bytes(2, "big") + width.to_bytes(2, "big") and b"\xFF\xFF" in file[at + 5:at + 9]
        assert file[at + 9:at + 13] == b"\x01\x01\x11\x00"
        assert ref_jpeg.decode(file).shape == (height, width, 3)


@pytest.mark.parametrize("name", PILLOWS)
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
    # more blocks than one launch of the transform takes, 32 a workgroup, and a last group of fewer than 32 in the second trip;
    # a dummy column in every MCU (24 wide: the second MCU's right half) and a dummy row under the last MCU row
    st, met = stats("rgb_24x65496_420_optimize")
    assert st["blocks"] > TRANSFORM_BLOCKS * (mesh.GRID_LANES // 256) and st["blocks"] % TRANSFORM_BLOCKS != 0
    assert st["blocks"] - st["blocks"] % TRANSFORM_BLOCKS > TRANSFORM_BLOCKS * (mesh.GRID_LANES // 256)  # (the ragged group is in the second trip)
    assert (st["blocks"], st["dummy_blocks"], st["bits"], st["stuffed"]) == (49128, 8191, 2778440, 953)
    assert st["dummy_blocks"] == 2 * 4094 + 2 * 2 - 1 and 65496 % 16 == 8 and 65496 + 8 > 65500
    # a block that ends exactly on a 32-bit word of the unstuffed stream, and a block of more than 32 bits that starts on
    # one (jpeg_write_kernel's plain store of a first word that no block in front shares)
    for name in ("grey_strip_8x40000", "rgb_24x65496_420_optimize"):
        assert stats(name)[1]["ends_on_dword"] >= 1 and stats(name)[1]["long_from_dword"] >= 1, name
    # 8192 blocks in a row and in a column
    assert stats("grey_65535x8")[0]["blocks"] == stats("grey_8x65535")[0]["blocks"] == 8192


def scan_of(file: bytes):
    """(bytes up to and including the SOS segment, FF 00 pairs in the scan's data) of a baseline file with one scan"""
    at = 2
    while True:
        assert file[at] == 0xFF
        marker, at = file[at + 1], at + 2 + int.from_bytes(file[at + 2:at + 4], "big")
        if marker == 0xDA:
            return at, file[at:-2].count(b"\xFF\x00")


def test_the_big_scene_is_pillows_and_is_past_one_launch():
    """The one slow test here (the restatement of 262656 blocks takes a quarter of a minute): the scene that
    test_jpeg_out_gpu.py compares with Pillow's file is the restatement's too, and it is past every launch it is there for -
    a lane a block (the dummy-DC, histogram, length and write kernels), 32 blocks a workgroup, and three launches of 1024-byte
    stuffing tiles."""
    pixels, quality, sampling, optimize = jpeg_out_scenes.big_scene("grey_4104x4096_optimize")
    assert not set(jpeg_out_scenes.BIG) & set(NAMES) and pixels.shape == (4096, 4104)
    got = ref_jpeg_out.encode(pixels, quality, sampling, optimize)
    want = pillow_file(pixels, quality, sampling, optimize)
    assert got["file"] == want
    st, met = got["stats"], got["met"]
    lanes, groups = mesh.GRID_LANES, mesh.GRID_LANES // 256
    assert st["blocks"] > lanes and st["blocks"] > TRANSFORM_BLOCKS * groups
    assert met["raw_bytes"] > 3 * groups * ref_jpeg_out.STUFF_TILE
    assert (st["blocks"], st["dummy_blocks"], st["bits"], met["raw_bytes"], st["stuffed"]) == (262656, 0, 25609363, 3201171, 8724)
    # what the GPU test derives from Pillow's file is what the restatement says
    assert scan_of(want) == (got["sections"][0], st["stuffed"])
    g = ref_jpeg_out.geometry(pixels.shape[1], pixels.shape[0], 1, sampling)
    assert g["mcus_x"] * g["mcus_y"] * g["blocks_per_mcu"] == st["blocks"]
    assert met["ends_on_dword"] >= 1 and met["long_from_dword"] >= 1
    # the colour scene of BIG, from its geometry alone: the last MCU, with its three dummy blocks, begins past one launch
    g = ref_jpeg_out.geometry(3352, 3352, 3, ref_jpeg_out.S420)
    assert (g["mcus_x"] * g["mcus_y"] - 1) * g["blocks_per_mcu"] > lanes
    assert g["mcus_x"] * 2 == g["blocks_x"] + 1 and g["mcus_y"] * 2 == g["blocks_y"] + 1


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
