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


def _met(name):
    return jpeg_prog_scenes.restated(name)["met"]


def test_dense_history_reads_every_piece_of_a_correction_field():
    """get_field takes a field in pieces of 16 bits: fields of one piece exactly, one bit more, two, three, and all but one bit of
    four in front of a new coefficient, the whole band's 63 bits by a block entered inside an EOB run, 32 bits in front of a ZRL's
    target.  A correction bit 1 on a bit that history has set cannot be written into a file the walk accepts: every coefficient of
    a band was last sent at Al = this scan's Ah, so its bit Al is clear - no scene has one (the device's test stays the kernel's)."""
    met = _met("p_dense_history")
    assert {16, 17, 32, 33, 48, 49, 62, 63} <= met["correction_field_bits"]
    assert {16, 17, 32, 33, 48, 49, 62} <= met["correction_field_bits_before_new"]
    assert 63 in met["correction_field_bits_in_eob_run"] and met["new_at_se_in_refinement"]
    assert met["zrl_over_history"] and met["zrl_history_between"] >= 17 and 32 in met["correction_field_bits_before_zrl"]
    assert jpeg_prog_scenes.restated("p_dense_history")["luma"].shape == (16, 48)
    assert all(_met(name)["correction_on_set_bit"] == 0 for name in jpeg_prog_scenes.names())
    # (Pillow's noise scenes read long fields too - up to 62 bits in q_noise_grey -, at whatever widths the noise gives; the writer's
    # earlier scenes none above 7)
    assert max(max(_met(name)["correction_field_bits"], default=0) for name in set(jpeg_prog_scenes.FORCED) - set(jpeg_prog_scenes.SEAMS)) <= 7


@pytest.mark.parametrize("key", sorted(jpeg_prog_scenes.DC_SLOTS))
def test_dc_slots_subsequences_begin_inside_the_mcu(key):
    """An interleaved DC-first scan of more than three subsequences whose first blocks lie at three slots of the MCU at least, a chroma
    slot and (where luma has more than one) a luma slot above 0 among them, with DC differences that are not zero."""
    size, sampling, seed = jpeg_prog_scenes.DC_SLOTS[key]
    met = _met("p_dc_slots_" + key)
    slots = met["dc_entry_slots"]
    luma = sampling[0] * sampling[1]
    assert met["scans"][0][:5] == ((0, 1, 2), 0, 0, 0, 0) and met["subsequences"][0] > 3
    assert all(per_mcu == luma + 2 and slot < per_mcu for slot, per_mcu in slots) and len(slots) >= 3
    assert any(slot >= luma for slot, _ in slots) and (luma == 1 or any(0 < slot < luma for slot, _ in slots))
    assert jpeg_prog_scenes.dc_slots_ok(slots, sampling)
    assert jpeg_prog_scenes.scene("p_dc_slots_" + key) == jpeg_prog_scenes._dc_slots_file(size, sampling, seed)   # the seed written down
    assert _met("q_flat256_420")["dc_entry_slots"]   # (the one earlier scene with such a scan: its differences are all zero)


def test_rst_every_block_has_more_intervals_than_a_workgroup_in_every_scan():
    for name in ("p_rst_every_block", "p_rst_every_block_fill"):
        met = _met(name)
        assert len(met["scans"]) == 6 and all(s[5:] == (1, 289) for s in met["scans"]) and met["intervals"] == 1734
        first = [n for s, n in zip(met["scans"], met["subsequences"]) if s[3] == 0]
        assert len(first) == 3 and sum(first) > 768 and all(n == 289 for n in first)   # each subsequence the first of its interval
    plain, filled = jpeg_prog_scenes.scene("p_rst_every_block"), jpeg_prog_scenes.scene("p_rst_every_block_fill")
    assert len(filled) == len(plain) + 6 * 288 + 1


@pytest.mark.parametrize("long_codes", [False, True])
def test_wide_first_crosses_a_workgroup_inside_a_later_first_scan(long_codes):
    """The band 6 .. 63 first scan - the third of the first scans' shared lane space - has more than 256 subsequences in its one
    interval, a multiple of 256 lanes falls strictly inside it, an EOBn (n >= 1) is the last symbol of a subsequence, and a symbol
    and an EOBn lie across a boundary.  With 16-bit codes: the smallest multiple of 8 at which seed 0 passes 256 subsequences; the
    scene's own seed does not pass them 8 pixels below either."""
    name = "p_wide_first_codes16" if long_codes else "p_wide_first"
    size, seed = jpeg_prog_scenes.WIDE_FIRST[long_codes]
    data = jpeg_prog_scenes.scene(name)
    assert data == jpeg_prog_scenes._wide_first_file(size, seed, long_codes)
    subs, inside, counts = jpeg_prog_scenes.wide_first_seams(data)
    met = _met(name)
    assert subs > 256 and inside and all(n > 0 for n in counts) and all(s[5] == 0 for s in met["scans"])
    assert met["longest_eob_run"] >= 4 and met["longest_code"] == (16 if long_codes else met["longest_code"])
    if long_codes:
        assert all(jpeg_prog_scenes.wide_first_seams(jpeg_prog_scenes._wide_first_file(size - 8, s, True))[0] <= 256 for s in (0, seed))
    else:
        assert size == 384


def test_chunk_seams_lie_where_the_byte_kernels_cut():
    """In scans behind the first: FF 00, FF Dn and fill FF whose FF ends a 64-byte chunk and a 256-byte workgroup of virtual bytes, a
    scan of a multiple of 64 bytes and one of a byte more - restated here from the parsed file."""
    data = jpeg_prog_scenes.scene("p_chunk_seams")
    assert jpeg_prog_scenes.chunk_seams(data) >= jpeg_prog_scenes.CHUNK_SEAMS
    assert data == jpeg_prog_scenes._chunk_seams_file(*jpeg_prog_scenes.CHUNK_SEAMS_FILE)
    h = ref_jpeg_prog.parse(data)
    lengths = [s["range"][1] - s["range"][0] for s in h["scans"]]
    assert lengths[-2] % 64 == 0 and lengths[-1] % 64 == 1 and all(s["restart"] == 1 for s in h["scans"])
    # the same once more on the virtual bytes themselves: every scan laid out from a multiple of 64, a filler byte between them
    virtual = b"".join(data[a:b] + b"\x01" * (-(b - a) % 64) for a, b in (s["range"] for s in h["scans"]))
    later = -(-lengths[0] // 64) * 64
    at = {pair: {i % 256 for i in range(later, len(virtual) - 1) if virtual[i:i + 2] == pair and i % 64 == 63}
          for pair in (b"\xff\x00", b"\xff\xd0", b"\xff\xd1", b"\xff\xd2", b"\xff\xd3", b"\xff\xd4", b"\xff\xd5", b"\xff\xd6", b"\xff\xd7", b"\xff\xff")}
    marker = set().union(*(at[bytes([0xFF, 0xD0 + k])] for k in range(8)))
    assert 255 in at[b"\xff\x00"] and at[b"\xff\x00"] - {255} and 255 in marker and marker - {255} and at[b"\xff\xff"]
    # no earlier scene of the writer or of Pillow has them all
    assert not any(jpeg_prog_scenes.chunk_seams(jpeg_prog_scenes.scene(name)) >= jpeg_prog_scenes.CHUNK_SEAMS
                   for name in ("p_refine_grey_rst", "q_33x47_422_rst1", "q_33x47_420_rst3"))


def test_mozjpeg_420_under_dri():
    """DRI 5 divides neither the luma raster's 5 blocks across nor the 9 chroma blocks; DRI 1.  Every scan kind runs per component."""
    for restart, name in ((5, "p_mozjpeg_420_rst5"), (1, "p_mozjpeg_420_rst1")):
        scans = _met(name)["scans"]
        assert len(scans) == 48 and all(s[5] == restart for s in scans)
        luma = [s for s in scans if s[0] == (0,)]
        assert {(s[1] > 0, s[3] > 0) for s in luma} == {(False, False), (False, True), (True, False), (True, True)}
        assert all(s[6] == -(-30 // restart) for s in luma) and all(s[6] == -(-9 // restart) for s in scans if s[0] != (0,))
    h = ref_jpeg_prog.parse(jpeg_prog_scenes.scene("p_mozjpeg_420_rst5"))
    assert h["scans"][0]["across"] == 5 and h["scans"][0]["mcus"] == 30 and h["mcus_x"] * h["mcus_y"] * 4 == 36


def test_refine_tails_take_every_length():
    """The last refinement's intervals are 1 .. 17 bytes long - both sides of the reader's 8-byte fast path, twice - and five end on their
    last correction bit without a pad bit."""
    met = _met("p_refine_tails")
    assert met["refine_interval_bytes"] == set(range(1, 18)) and met["refine_interval_without_pad"] >= 5
    assert met["scans"][-2][1:5] == (1, 63, 1, 0) and met["scans"][-2][5:] == (1, len(jpeg_prog_scenes.REFINE_TAILS))


def test_al_high_shifts():
    met = _met("p_al_high")
    assert jpeg_prog_scenes.AL_HIGH == (5, 6)
    assert [s[3:5] for s in met["scans"] if s[1] == 0] == [(0, 5)] + [(ah, ah - 1) for ah in (5, 4, 3, 2, 1)]
    assert [s[3:5] for s in met["scans"] if s[1:3] == (1, 63)] == [(ah, ah - 1) for ah in (6, 5, 4, 3, 2, 1)]
    coef, _ = ref_jpeg_prog.entropy_decode(ref_jpeg_prog.parse(jpeg_prog_scenes.scene("p_al_high")))
    assert np.abs(coef[:, 1:].astype(np.int64)).max() >= 256 and np.abs(coef[:, 0].astype(np.int64)).max() >= 256   # category 9
    assert max(s[4] for name in jpeg_prog_scenes.names() if name != "p_al_high" for s in _met(name)["scans"]) <= 3


@pytest.mark.parametrize("name", jpeg_prog_scenes.REFUSED_SEAMS)
def test_refused_seams_raise_their_code(name):
    data, code = jpeg_prog_scenes.refused_seams()[name]
    with pytest.raises(ref_jpeg_prog.JpegError) as err:
        ref_jpeg_prog.decode(data)
    assert err.value.code == code == ref_jpeg.INVALID
    ref_jpeg_prog.parse(data)   # the walk and the progression are whole: the entropy decode refuses it


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
