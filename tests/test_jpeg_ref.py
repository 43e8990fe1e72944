"""tests/ref_jpeg.py, the definition of cvhip_jpeg_decode's pixels, against Pillow (libjpeg-turbo) on the CPU,
and tests/jpeg_scenes.py: every forced scene reaches the case it is there for."""
import io

import numpy as np
import pytest

import jpeg_scenes
import ref_jpeg


def pillow_rgb(data):
    from PIL import Image

    return np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))


@pytest.mark.parametrize("name", sorted(jpeg_scenes.ENCODED))
def test_encoder_made_files_decode_as_pillow_does(name):
    want = jpeg_scenes.restated(name)
    rgb = pillow_rgb(jpeg_scenes.scene(name))
    assert rgb.shape == want["rgb"].shape and (rgb == want["rgb"]).all()
    assert (want["luma"] == ref_jpeg.luma_of_rgb(rgb)).all()   # (of a grey file: (10000 v) / 10000, its plane)


def test_grey_files_are_their_plane():
    from PIL import Image

    for name in ("e_17x9_grey", "e_33x47_grey_rst3", "w_grey"):
        data = jpeg_scenes.scene(name)
        want = jpeg_scenes.restated(name)
        assert ref_jpeg.info(data)["components"] == 1
        assert (np.asarray(Image.open(io.BytesIO(data))) == want["luma"]).all()
        assert (want["rgb"] == want["luma"][:, :, None]).all()


@pytest.mark.parametrize("name", jpeg_scenes.FORCED_IN_ENCODER_RANGE)
def test_the_writers_files_open_in_pillow(name):
    """Where the writer's coefficients are in an encoder's range, libjpeg-turbo returns the restated pixels."""
    assert (pillow_rgb(jpeg_scenes.scene(name)) == jpeg_scenes.restated(name)["rgb"]).all()


def _scan(data):
    h = ref_jpeg.parse(data)
    return h, data[h["scan"][0]:h["scan"][1]]


def test_forced_scenes_reach_their_cases():
    # 16-bit codes, a 16-bit DQT with an entry past 8 bits, a block longer than a subsequence, a block without EOB
    data = jpeg_scenes.scene("w_codes16")
    met = jpeg_scenes.restated("w_codes16")["met"]
    assert met["longest_code"] == 16 and met["longest_block_bits"] > jpeg_scenes.SUBSEQ_BITS
    dqt = data.index(b"\xff\xdb")
    assert data[dqt + 4] >> 4 == 1
    h = ref_jpeg.parse(data)
    assert max(h["quant"][0]) > 255
    coef, _ = ref_jpeg.entropy_decode(h)
    assert coef[1, ref_jpeg.ZIGZAG[63]] != 0 and np.count_nonzero(coef[1]) == 3   # ZRL chains up to an EOB-less end
    assert np.count_nonzero(coef[3]) == 64 and np.abs(coef[3, 1:]).min() >= 512    # category 10 throughout
    assert (ref_jpeg.info(data)["h"], ref_jpeg.info(data)["v"]) == (2, 2)
    # more than eight intervals, a DRI that does not divide the MCU count, FF FF fill
    data = jpeg_scenes.scene("w_restart")
    h, scan = _scan(data)
    mcus = h["mcus_x"] * h["mcus_y"]
    assert h["restart"] == 2 and mcus % 2 == 1 and len(ref_jpeg.segments(h)) == 13
    assert b"\xff\xff\xff\xd7" in scan and scan.index(b"\xff\xd7") < scan.rindex(b"\xff\xd0")   # RST7, then RST0 again
    assert data.endswith(b"\xff\xff\xff\xd9")


def test_encoded_scenes_reach_their_cases():
    # chroma planes of at most two columns (replication), at 4:2:0 and at 4:2:2
    for name, sampling in (("e_1x1_420", (2, 2)), ("e_3x5_420", (2, 2)), ("e_4x4_420", (2, 2)), ("e_4x3_422", (2, 1))):
        info = ref_jpeg.info(jpeg_scenes.scene(name))
        assert (info["h"], info["v"]) == sampling and -(-info["width"] // 2) <= 2
    info = ref_jpeg.info(jpeg_scenes.scene("e_5x3_422"))   # three chroma columns: the smallest fancy h2v1 row
    assert (info["h"], info["v"], -(-info["width"] // 2)) == (2, 1, 3)
    for name, sampling in (("e_17x9_444", (1, 1)), ("e_17x9_422", (2, 1)), ("e_17x9_420", (2, 2))):
        info = ref_jpeg.info(jpeg_scenes.scene(name))
        assert (info["h"], info["v"], info["width"] % 16, info["height"] % 16) == (*sampling, 1, 9)
    # restart intervals of 1 and 3 MCUs and of an MCU row
    for name, interval in (("e_33x47_420_rst1", 1), ("e_33x47_422_rst3", 3), ("e_33x47_grey_rst3", 3)):
        assert ref_jpeg.parse(jpeg_scenes.scene(name))["restart"] == interval
    h = ref_jpeg.parse(jpeg_scenes.scene("e_33x47_444_rstrow"))
    assert h["restart"] == h["mcus_x"]
    # the noise file: no DRI, more subsequences than a workgroup has lanes, an FF 00 pair across a 256-byte piece boundary
    h, scan = _scan(jpeg_scenes.scene("e_noise160_444"))
    assert h["restart"] == 0 and 8 * len(ref_jpeg.segments(h)[0]) > 256 * jpeg_scenes.SUBSEQ_BITS
    assert any(scan[i] == 0xFF and scan[i + 1] == 0 for i in range(255, len(scan) - 1, 256))
    # the flat file: dozens of MCUs in one subsequence
    h, scan = _scan(jpeg_scenes.scene("e_flat256_420"))
    assert 8 * len(ref_jpeg.segments(h)[0]) / (h["mcus_x"] * h["mcus_y"]) * 24 < jpeg_scenes.SUBSEQ_BITS
    # the EXIF block
    assert ref_jpeg.info(jpeg_scenes.scene("e_exif"))["focal_length_35mm"] == 28
    assert jpeg_scenes.restated("e_17x9_420")["met"]["longest_code"] == 16


def test_exif_walk():
    for short in (True, False):
        for big in (True, False):
            assert ref_jpeg.exif_focal_length_35mm(jpeg_scenes.exif_bytes(35, short, big)) == 35
    block = jpeg_scenes.exif_bytes(35)
    for cut in range(len(block)):
        assert ref_jpeg.exif_focal_length_35mm(block[:cut]) in (0, 35)   # (a broken block is none - or whole enough)
    assert ref_jpeg.exif_focal_length_35mm(b"II*\0" + b"\xff" * 12) == 0


@pytest.mark.parametrize("name", sorted(jpeg_scenes.refused()))
def test_refused_files(name):
    data, code = jpeg_scenes.refused()[name]
    with pytest.raises(ref_jpeg.JpegError) as err:
        ref_jpeg.decode(data)
    assert err.value.code == code
    if name in ("progressive", "four_components"):   # (made by Pillow: valid files that are not built)
        from PIL import Image

        Image.open(io.BytesIO(data)).load()


def test_drop_rows_and_calibration_matrix():
    data = jpeg_scenes.scene("e_17x9_420")
    want = jpeg_scenes.restated("e_17x9_420")
    assert (ref_jpeg.decode(data, ref_jpeg.RGB8, drop_rows=8) == want["rgb"][:1]).all()
    with pytest.raises(ref_jpeg.JpegError):
        ref_jpeg.decode(data, drop_rows=9)
    k = ref_jpeg.calibration_matrix(6000, 4000, 28)
    assert k[0, 0] == k[1, 1] == 28.0 * np.sqrt(6000.0 ** 2 + 4000.0 ** 2) / np.sqrt(24.0 ** 2 + 36.0 ** 2)
    assert (k[0, 2], k[1, 2]) == (3000.0, 2000.0)
    assert ref_jpeg.calibration_matrix(640, 480, None)[0, 0] == np.sqrt(640.0 ** 2 + 480.0 ** 2) / np.sqrt(24.0 ** 2 + 36.0 ** 2)
