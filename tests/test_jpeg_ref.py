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


def test_earlier_restart_scenes_stay_inside_one_workgroup():
    """What the seam scenes below are there for: of the scenes before them, the one with more than 256 subsequences has no
    DRI, and no RSTn has its FF as the last byte of a 64-byte piece of the scan."""
    new = set(jpeg_scenes.RESTART) | {"w_dc_wrap", "w_dc_wrap_rst", "w_fill_straddles"}
    for name in set(jpeg_scenes.names()) - new:
        at = jpeg_scenes.seams(jpeg_scenes.scene(name))
        assert at["intervals"] == 1 or at["subsequences"] <= 30
        assert not [s for s in at["straddles"][jpeg_scenes.WAVE_BYTES] if s[0] == s[1] - 1] and not at["lane0"]
        assert not at["spanning"] or at["intervals"] == 1
        met = jpeg_scenes.restated(name)["met"]
        assert -32768 <= met["dc_min"] and met["dc_max"] <= 32767


@pytest.mark.parametrize("name", sorted(jpeg_scenes.RESTART))
def test_restart_scenes_cross_the_sync_kernels_workgroups(name):
    """More than 256 subsequences in a file with restart intervals: a second launch of the sync kernel, an interval whose
    subsequences lie in two workgroups (the lanes behind its first take exit_in[i - 1] across the boundary), or one that
    begins at lane 0 of a later workgroup (known: it takes nothing)."""
    size, options = jpeg_scenes.RESTART[name]
    data = jpeg_scenes.scene(name)
    h, at = ref_jpeg.parse(data), jpeg_scenes.seams(data)
    assert h["restart"] == options["restart_marker_blocks"] and (h["width"], h["height"]) == (size, size)
    assert at["intervals"] == -(-h["mcus_x"] * h["mcus_y"] // h["restart"]) == len(ref_jpeg.segments(h)) > 25
    assert at["subsequences"] > options.get("more_than", jpeg_scenes.SYNC_LANES)
    assert at[options.get("want", "spanning")]
    for s in at["spanning"]:
        first, last = at["sub_first"][s], at["sub_first"][s + 1] - 1
        assert first // 256 + 1 == last // 256 and last % 256 < first % 256
    for s in at["lane0"]:
        assert at["sub_first"][s] >= 256 and at["sub_first"][s] % 256 == 0
    assert len(data) <= 100 * 1024


def test_restart_scenes_as_a_set():
    at = {name: jpeg_scenes.seams(jpeg_scenes.scene(name)) for name in jpeg_scenes.RESTART}
    info = {name: ref_jpeg.info(jpeg_scenes.scene(name)) for name in jpeg_scenes.RESTART}
    assert {(i["components"], i["h"], i["v"]) for i in info.values()} == {(3, 1, 1), (3, 2, 1), (3, 2, 2), (1, 1, 1)}
    assert sum(1 for a in at.values() if a["spanning"]) >= 5 and any(a["lane0"] for a in at.values())
    # a workgroup with a neighbour on both sides, and an interval across each of its boundaries
    big = at["e_rst5_200_444"]
    assert big["subsequences"] > 512 and {big["sub_first"][s] // 256 for s in big["spanning"]} >= {0, 1}
    # the table of the scenes' sizes (libjpeg-turbo's encoder decides them; another encoder must not hollow them out)
    assert {n: (a["intervals"], a["subsequences"] > 256) for n, a in at.items()} == {
        "e_rst7_120_444": (33, True), "e_rst1_120_444": (225, True), "e_rst5_128_422": (26, True), "e_rst3_160_grey": (134, True),
        "e_rst3_176_420": (41, True), "e_rst5_200_444": (125, True)}


def test_markers_straddle_the_byte_kernels_pieces():
    """An RSTn whose FF is the last byte of a 64-byte piece of the scan (two waves' ballots) and another whose FF is the last
    of a 256-byte piece (two workgroups); with FF FF fill: the edge behind the first fill byte, behind the second and behind
    the marker's own FF."""
    W, G = jpeg_scenes.WAVE_BYTES, jpeg_scenes.GROUP_BYTES
    at = jpeg_scenes.seams(jpeg_scenes.scene("e_rst1_120_444"))["straddles"]
    assert (1, 2) in at[G] and at[W].count((1, 2)) > at[G].count((1, 2))
    data = jpeg_scenes.scene("w_fill_straddles")
    h, scan = _scan(data)
    at = jpeg_scenes.seams(data)
    assert h["restart"] == 1 and at["intervals"] == 400 and scan.count(b"\xff\xff\xff") == 399 and data.endswith(b"\xff\xff\xff\xd9")
    for unit in (W, G):
        assert {(1, 4), (2, 4), (3, 4)} <= set(at["straddles"][unit])
    # (seams() is told by the bytes themselves)
    for unit in (W, G):
        for k in (1, 2, 3):
            assert any(scan[i - k:i + 4 - k] == b"\xff\xff\xff" + bytes([scan[i + 3 - k]]) and 0xD0 <= scan[i + 3 - k] <= 0xD7
                       for i in range(unit, len(scan) - 4, unit))


def test_dc_sums_leave_the_int16_range():
    """The luma sums climb past 32 767 and the Cb sums fall past -32 768: the restatement wraps them as the definition says
    (4.16), and a decoder that keeps them in a wider integer differs.  With DRI the sums start again at zero."""
    for name, restart in (("w_dc_wrap", 0), ("w_dc_wrap_rst", 20)):
        data = jpeg_scenes.scene(name)
        h = ref_jpeg.parse(data)
        met = jpeg_scenes.restated(name)["met"]
        assert h["restart"] == restart and met["dc_max"] > 32767 and met["dc_min"] < -32768
        coef, _ = ref_jpeg.entropy_decode(h)
        dc = coef[:, 0].astype(np.int64).reshape(-1, 3)
        steps = np.diff(dc[:, 0])
        wraps = np.flatnonzero(steps < -60000)
        assert len(wraps) >= 1 and dc[wraps[0], 0] > 30000 and dc[wraps[0] + 1, 0] < -30000     # 32 7xx -> -3x xxx
        assert (np.diff(dc[:, 1]) > 60000).any()
        if restart:
            assert abs(dc[restart, 0] - dc[0, 0]) < 100 and abs(dc[restart - 1, 0] - dc[restart, 0]) > 20000   # the sum starts again
        # the pixels tell: the blocks behind the wrap are dark where an unwrapped sum would leave them bright
        luma = jpeg_scenes.restated(name)["luma"]
        assert luma.min() < 64 and luma.max() > 192


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
