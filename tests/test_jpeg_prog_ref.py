"""tests/ref_jpeg_prog.py, the definition of cvhip_jpeg_progressive_decode's pixels, without a GPU: its RGB8
equals Pillow's (libjpeg-turbo's) `convert("RGB")` byte for byte on every encoder-made progressive file and on every file of
the test's own writer (all lie within an encoder's coefficient range); the same coefficients written as a baseline file and
decoded by tests/ref_jpeg.py give the same pixels; every forced file reaches its case; every refused file raises its code."""
import io

import numpy as np
import pytest

import jpeg_prog_scenes
import jpeg_scenes
import ref_jpeg
import ref_jpeg_prog


@pytest.mark.parametrize("name", jpeg_prog_scenes.names())
def test_restatement_is_pillow(name):
    from PIL import Image

    assert name in jpeg_prog_scenes.ENCODED or name in jpeg_prog_scenes.IN_ENCODER_RANGE
    want = np.asarray(Image.open(io.BytesIO(jpeg_prog_scenes.scene(name))).convert("RGB"))
    got = jpeg_prog_scenes.restated(name)
    assert got["rgb"].shape == want.shape and (got["rgb"] == want).all()
    assert (got["luma"] == ref_jpeg.luma_of_rgb(got["rgb"])).all()
    info = ref_jpeg_prog.info(jpeg_prog_scenes.scene(name))
    assert (info["height"], info["width"]) == want.shape[:2] and info["scans"] == len(got["met"]["scans"])
    assert info["focal_length_35mm"] == jpeg_prog_scenes.FOCAL.get(name, 0)


@pytest.mark.parametrize("name", sorted(jpeg_prog_scenes.COEFFICIENTS))
def test_same_coefficients_as_a_baseline_file(name):
    w, h, coef, options = jpeg_prog_scenes.COEFFICIENTS[name]()
    baseline = jpeg_scenes.write(w, h, coef, jpeg_scenes.QUANT_PLAIN, **options)
    assert (ref_jpeg.decode(baseline) == jpeg_prog_scenes.restated(name)["rgb"]).all()
    assert (ref_jpeg.decode(baseline, ref_jpeg.LUMA8) == jpeg_prog_scenes.restated(name)["luma"]).all()


def test_drop_rows():
    data = jpeg_prog_scenes.scene("q_33x47_420")
    for mode, key in ((ref_jpeg_prog.RGB8, "rgb"), (ref_jpeg_prog.LUMA8, "luma")):
        assert (ref_jpeg_prog.decode(data, mode, drop_rows=5) == jpeg_prog_scenes.restated("q_33x47_420")[key][:42]).all()
    with pytest.raises(ref_jpeg_prog.JpegError):
        ref_jpeg_prog.decode(data, drop_rows=47)


def _scans(name):
    return jpeg_prog_scenes.restated(name)["met"]["scans"]   # (components, Ss, Se, Ah, Al, DRI, intervals)


def test_pillow_files_have_all_four_scan_kinds():
    for name in sorted(jpeg_prog_scenes.ENCODED):
        kinds = {(ss > 0, ah > 0) for _, ss, _, ah, _, _, _ in _scans(name)}
        assert kinds == {(False, False), (False, True), (True, False), (True, True)}, name
    assert any(s[5] == 1 for s in _scans("q_33x47_422_rst1")) and any(s[5] == 3 for s in _scans("q_33x47_420_rst3"))


def test_forced_cases_are_reached():
    met = {name: jpeg_prog_scenes.restated(name)["met"] for name in jpeg_prog_scenes.FORCED}
    # DC scans per component, as mozjpeg writes them; bands 1-2, 3-9 and 10-63; Al = 3: three refinement passes
    moz = met["p_mozjpeg_420"]["scans"]
    assert [s[0] for s in moz[:3]] == [(0,), (1,), (2,)] and all(s[1:5] == (0, 0, 0, 3) for s in moz[:3])
    for band in ((1, 2), (3, 9), (10, 63)):
        assert [s[3:5] for s in moz if s[0] == (0,) and s[1:3] == band] == [(0, 3), (3, 2), (2, 1), (1, 0)]
    # Y alone and then Cb + Cr together; spectral selection only; DRI changing between scans
    ytc = met["p_y_then_chroma_422"]["scans"]
    assert ytc[0][0] == (0,) and ytc[1][0] == (1, 2) and all(s[3:5] == (0, 0) for s in ytc)
    assert [s[5] for s in ytc] == [2, 3, 1, 0, 3, 3] and ytc[3][6] == 1 and ytc[2][6] > ytc[4][6] > 1
    # the luma's own raster is not the MCU-padded grid: 21 x 10 at 4:2:2 has 3 x 2 luma blocks in 2 x 2 MCUs of two
    h = ref_jpeg_prog.parse(jpeg_prog_scenes.scene("p_y_then_chroma_422"))
    assert h["scans"][0]["mcus"] == 6 and h["mcus_x"] * h["mcus_y"] * 2 == 8
    # a table slot redefined between scans: one DHT per scan, all in slot 0
    data = jpeg_prog_scenes.scene("p_refine_444")
    assert data.count(b"\xff\xc4") >= 10 and len({id(s["ac"]) for s in ref_jpeg_prog.parse(data)["scans"] if s["ac"]}) >= 6
    # the refinement cases
    for name in ("p_refine_444", "p_refine_grey_rst"):
        for case in ("zrl_in_refinement", "zrl_over_history", "new_at_se_in_refinement", "history_after_last_new", "corrections_in_eob_run",
                     "eob_run_ends_scan"):
            assert met[name][case], (name, case)
    assert met["p_refine_grey_rst"]["scans"][0][5:] == (4, 4)
    # an EOB run of 16384 blocks, and no smaller grey image has one: 16384 blocks are 1024 x 1024 pixels
    assert met["p_eob16384"]["longest_eob_run"] == 16384
    assert jpeg_prog_scenes.restated("p_eob16384")["luma"].shape == (1024, 1024)
    # 16-bit codes
    assert met["p_codes16"]["longest_code"] == 16
    # long EOB runs in the flat image
    assert jpeg_prog_scenes.restated("q_flat256_420")["met"]["longest_eob_run"] >= 256


def test_the_noise_image_is_the_smallest_that_crosses_a_workgroup():
    """Without DRI, an AC-first scan of more than 256 subsequences; at 8 pixels less no AC-first scan has that many."""
    size = jpeg_prog_scenes.noise_size()
    data = jpeg_prog_scenes.scene("q_noise_grey")
    assert jpeg_prog_scenes._most_first_subsequences(data) > 256
    assert all(s[5] == 0 for s in _scans("q_noise_grey"))
    smaller = jpeg_prog_scenes._pillow(size - 8, size - 8, "noise", grey=True, quality=95)
    assert jpeg_prog_scenes._most_first_subsequences(smaller) <= 256


@pytest.mark.parametrize("name", sorted(jpeg_prog_scenes.refused()))
def test_refused_files_raise_their_code(name):
    data, code = jpeg_prog_scenes.refused()[name]
    with pytest.raises(ref_jpeg_prog.JpegError) as err:
        ref_jpeg_prog.decode(data)
    assert err.value.code == code
    if name not in ("baseline", "sof0_two_scans"):
        assert b"\xff\xc2" in data


def test_the_old_entry_point_still_refuses_progressive_files():
    for name in ("q_17x9_420", "p_refine_444"):
        with pytest.raises(ref_jpeg.JpegError) as err:
            ref_jpeg.decode(jpeg_prog_scenes.scene(name))
        assert err.value.code == ref_jpeg.UNSUPPORTED
