"""tests/ref_png_in.py, the definition of cvhip_png_decode's pixels, without a GPU: its inflate against
zlib.decompress on every valid scene, its samples against Pillow where Pillow exposes them, the block structure and the
forced cases of the scenes through its statistics, the code of every refused file, and Pillow's refusal of the malformed
files where Pillow checks the same thing."""
import io
import zlib

import numpy as np
import pytest

import png_in_scenes as scenes
import ref_png_in as ref


@pytest.mark.parametrize("name", scenes.names())
def test_inflate_is_zlib_and_the_filters_agree(name):
    data = scenes.scene(name)
    want = scenes.restated(name)
    h = want["header"]
    assert zlib.decompress(ref.stream_of(data)) == want["filtered"]
    if h["height"] * h["row_bytes"] <= 20000:   # the byte-at-a-time definition against the anti-diagonal one
        assert (ref.unfilter(want["filtered"], h["height"], h["row_bytes"], h["bpp"]) ==
                ref.unfilter_fast(want["filtered"], h["height"], h["row_bytes"], h["bpp"])).all()
    assert want["luma"].shape == (h["height"], h["width"]) and want["rgb"].shape == (h["height"], h["width"], 3)
    assert ref.info(data)[:5] == (h["width"], h["height"], h["colour"], h["depth"], 0)
    assert ref.info(data)[6] == scenes.FOCAL.get(name, 0)


@pytest.mark.parametrize("name", scenes.names())
def test_samples_are_pillows(name):
    """L, LA, RGB, RGBA, P, 1/2/4-bit grey and I;16: Pillow's raw samples.  (16-bit RGB and grey + alpha Pillow reduces
    itself; those are not compared.)"""
    from PIL import Image

    want = scenes.restated(name)
    h = want["header"]
    im = Image.open(io.BytesIO(scenes.scene(name)))
    im.load()
    s = want["samples"]
    if h["depth"] == 16 and h["colour"] != 0:
        return
    got = np.asarray(im)
    if h["colour"] == 0 and h["depth"] == 16:
        assert im.mode.startswith("I;16") or im.mode == "I"
        assert (got.astype(np.int64) == s[:, :, 0]).all()
    elif h["colour"] == 0 and h["depth"] < 8:
        if "transparency" in im.info:
            return
        if im.mode == "1":
            assert (got.astype(np.int64) == s[:, :, 0]).all()
        else:   # Pillow scales to 8 bits as the definition does
            assert (got.astype(np.int64) == s[:, :, 0] * (255 // ((1 << h["depth"]) - 1))).all()
            assert (got == want["luma"]).all()
    elif h["colour"] == 3:
        assert im.mode == "P" and (got.astype(np.int64) == s[:, :, 0]).all()
        assert (np.asarray(im.convert("RGB")) == want["rgb"]).all()
    else:
        assert im.mode == {0: "L", 2: "RGB", 4: "LA", 6: "RGBA"}[h["colour"]]
        assert (got.reshape(s.shape).astype(np.int64) == s).all()


def _stats(name):
    return scenes.restated(name)["stats"]


def test_block_structure_of_the_encoder_scenes():
    """What zlib made of the pictures (zlib 1.2.11 here): a different zlib must not hollow a scene out."""
    st = _stats("b_mem1")
    assert (st["stored"], st["fixed"], st["dynamic"]) == (0, 1, 36) and max(b[2] for b in st["blocks"]) <= 1255
    assert len({b[1] % 8 for b in st["blocks"]}) == 8          # block boundaries at every bit alignment
    st = _stats("b_mem8")
    assert (st["stored"], st["fixed"], st["dynamic"]) == (0, 0, 1) and st["blocks"][0][2] > 30000 and st["longest_code"] >= 11
    st = _stats("b_fixed")
    assert (st["stored"], st["fixed"], st["dynamic"]) == (0, 1, 0)
    st = _stats("b_stored")
    assert st["fixed"] == st["dynamic"] == 0 and st["stored"] >= 1
    st = _stats("b_flushes")
    assert st["zero_stored"] >= 2 and st["dynamic"] >= 1
    st = _stats("b_noise160")
    assert st["dynamic"] == 2 and st["longest_code"] == 15 and st["max_distance"] > 32000
    assert sum(b[2] for b in st["blocks"]) > 256 * 1024     # more subsequences than a workgroup has lanes
    st = _stats("flat200")
    assert (st["stored"], st["fixed"], st["dynamic"]) == (0, 0, 1) and st["blocks"][0][2] == 440
    assert st["max_distance"] == 1 and st["max_length"] == 258 and len(scenes.restated("flat200")["filtered"]) == 40200
    assert len(ref.parse(scenes.scene("p_default"))["idat"]) >= 1


def test_forced_scenes_reach_their_cases():
    st = _stats("t_far_long")
    assert st["max_distance"] == 32768 and st["max_length"] == 258 and st["extra13"]
    assert st["blocks"][0][2] > 256 * 1024                     # a dynamic block longer than a settle window
    assert _stats("t_overlaps")["overlaps"] == {1, 2, 3}
    assert _stats("t_three_blocks_back")["back_blocks"] == 3
    st = _stats("t_stored_alignments")
    assert st["stored_after"] == set(range(8)) and st["empty_blocks"] == 2 and st["zero_stored"] == 1
    assert st["blocks"][-1][0] == 0 and st["blocks"][-1][3] == 0  # the final block: stored and empty
    st = _stats("t_literals_only")
    assert st["dist_none"] == 1 and st["repeat16_crosses"] >= 1
    st = _stats("t_fixed_long")
    assert st["fixed"] == 1 and st["blocks"][0][2] > 256 * 1024  # longer than a settle window
    assert len(ref.parse(scenes.scene("i_bytes"))["idat"]) == len(ref.stream_of(scenes.scene("i_one")))
    assert [n for _o, n, _c in ref.parse(scenes.scene("i_empties"))["idat"]].count(0) >= 4
    cuts = [n for _o, n, _c in ref.parse(scenes.scene("i_header_adler"))["idat"]]
    assert cuts[0] == 1 and cuts[-1] == 2
    for name in ("i_bytes", "i_empties", "i_header_adler"):
        assert (scenes.restated(name)["rgb"] == scenes.restated("i_one")["rgb"]).all()
    assert ref.info(scenes.scene("s_pal2_trns"))[7] == 3 and ref.info(scenes.scene("s_grey_trns_gama"))[7] == 2
    assert ref.info(scenes.scene("x_broken"))[6] == 0
    types = [scenes.restated("f_third_sub")["filtered"][y * 46] for y in range(70)]
    assert types[:3] == [1, 4, 3] and set(scenes.restated("f_130_paeth")["filtered"][::70]) == {4}


@pytest.mark.parametrize("name", sorted(scenes.refused()))
def test_refused_files_raise_their_code(name):
    data, code = scenes.refused()[name]
    with pytest.raises(ref.PngError) as err:
        ref.decode(data)
    assert err.value.code == code


def test_accepted_here():
    for name in scenes.ACCEPTED_HERE:
        ref.decode(scenes.accepted()[name])
    assert ref.parse(scenes.accepted()["a_far_cinfo"]) and ref.stream_of(scenes.accepted()["a_far_cinfo"])[0] == 0x08


PILLOW_CHECKS_TOO = ("i_signature", "i_crc_ihdr", "i_adler", "i_too_far", "i_no_final_eob", "i_btype3", "i_nlen", "i_oversubscribed")


@pytest.mark.parametrize("name", PILLOW_CHECKS_TOO)
def test_pillow_refuses_them_too(name):
    from PIL import Image

    with pytest.raises(Exception):
        im = Image.open(io.BytesIO(scenes.refused()[name][0]))
        im.load()
