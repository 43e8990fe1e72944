"""tests/ref_tiff_ext.py, the definition of cvhip_tiff_ext_decode, on the CPU: its samples are Pillow's
(libtiff's) on every scene Pillow reads and the source picture's on all of them; every scene of tests/tiff_ext_scenes.py
reaches the case it is named for - asserted from inflate's block table and from the geometry, so that another zlib build cannot
quietly empty a case -; every file of the strip reader decodes to ref_tiff's pixels; the refusals get their codes."""
import io

import numpy as np
import pytest

import ref_tiff
import ref_tiff_ext
import tiff_ext_scenes
import tiff_scenes

SUBSEQ_BITS, WINDOW = 1024, 256   # png_decode_common.hpp: a settle window is 256 subsequences of 1024 bits

# Pillow opens no 16-bit RGB(A), and libtiff does not honour Predictor 2 on uncompressed data: compared with the source alone
NOT_FOR_PILLOW = ("s_rgba16_mm", "t_pred_g8_272_raw", "t_pred_rgb16_16", "t_pred_rgb16_256", "t_pred_rgb16_272")


def _stats(name):
    stats = {}
    h, a = ref_tiff_ext.samples(tiff_ext_scenes.scene(name), stats)
    return h, a, stats


@pytest.mark.parametrize("name", tiff_ext_scenes.names())
def test_samples_are_the_sources_and_libtiffs(name):
    from PIL import Image

    data = tiff_ext_scenes.scene(name)
    h, a = ref_tiff_ext.samples(data)
    assert a.dtype == tiff_ext_scenes.source(name).dtype and (a == tiff_ext_scenes.source(name)).all()
    if name not in NOT_FOR_PILLOW:
        got = np.asarray(Image.open(io.BytesIO(data)))
        got = got[:, :, None] if got.ndim == 2 else got
        if h["photometric"] == 0:   # (Pillow inverts WhiteIsZero when it opens the file)
            got = 255 - got
        assert got.shape == a.shape and (got.astype(np.uint32) == a).all()
    for fmt in (ref_tiff.LUMA8, ref_tiff.RGB8):
        assert (ref_tiff_ext.decode(data, fmt) == ref_tiff.convert(h, a, fmt)).all()


def test_few_scenes_skip_pillow():
    assert set(NOT_FOR_PILLOW) <= set(tiff_ext_scenes.names()) and 8 * len(NOT_FOR_PILLOW) <= len(tiff_ext_scenes.names())


@pytest.mark.parametrize("name", tiff_scenes.names())
def test_strip_files_decode_as_before(name):
    """A file the strip reader accepts: ref_tiff's pixels, header and counts through the extended restatement."""
    data, old, new = tiff_scenes.scene(name), {}, {}
    for fmt in (ref_tiff.LUMA8, ref_tiff.RGB8):
        assert (ref_tiff_ext.decode(data, fmt, stats=new) == ref_tiff.decode(data, fmt, stats=old)).all()
    assert {k: new.get(k) for k in ("codes", "clears", "longest")} == {k: old.get(k) for k in ("codes", "clears", "longest")}
    info = ref_tiff_ext.info(data)
    assert {k: v for k, v in info.items() if not k.startswith("tile")} == ref_tiff.info(data)
    assert (info["tile_width"], info["tile_length"], info["tiles_across"]) == (0, 0, 0)


def test_deflate_scenes_reach_their_cases():
    def kinds(name):
        st = _stats(name)[2]
        return st["stored"], st["fixed"], st["dynamic"]

    assert kinds("s_1x1")[0] == 0 and _stats("s_1x1")[0]["strips"] == 1
    assert kinds("s_stored") == (1, 0, 0) and kinds("s_fixed") == (0, 1, 0) and kinds("s_dynamic") == (0, 0, 1)
    # several blocks of all three kinds in one stream, copies that reach back over block ends
    h, _a, st = _stats("s_mixed")
    assert h["strips"] == 1 and min(kinds("s_mixed")) >= 1 and len(st["inflate"][0]["blocks"]) >= 5
    assert st["inflate"][0]["back_blocks"] >= 3 and st["inflate"][0]["max_distance"] > 96 * 32
    # one long chain of distance-1 copies: resolved by pointer doubling in about log2(4095) rounds
    st = _stats("s_flat")[2]["inflate"][0]
    assert st["overlaps"] == {1} and st["max_distance"] == 1 and st["max_length"] == 258 and sum(b[3] for b in st["blocks"]) == 64 * 64
    assert _stats("s_70_strips")[0]["strips"] == 70 and len(_stats("s_70_strips")[2]["inflate"]) == 70
    h = _stats("s_out_of_order")[0]
    assert h["offsets"] != sorted(h["offsets"]) and any(o % 2 for o in h["offsets"]) and any(o % 4 for o in h["offsets"])
    # two identical neighbours: the same stream twice, with copies inside each
    data, h = tiff_ext_scenes.scene("s_twins"), _stats("s_twins")[0]
    streams = [data[o:o + n] for o, n in zip(h["offsets"], h["counts"])]
    assert len(streams) == 2 and streams[0] == streams[1] and _stats("s_twins")[2]["inflate"][1]["max_distance"] > 0
    # a block whose tokens take more bits than a settle window holds: its decode crosses the window's end
    h, _a, st = _stats("s_window")
    assert h["strips"] == 1 and h["counts"][0] > WINDOW * SUBSEQ_BITS // 8
    assert max(b[2] for b in st["inflate"][0]["blocks"] if b[0] != 0) > WINDOW * SUBSEQ_BITS + 3
    assert _stats("s_32946")[0]["compression"] == 32946 and _stats("t_rgb_16x32_32946_pred")[0]["compression"] == 32946
    assert (_stats("s_mm_g16_pred")[0]["order"], _stats("s_ii_g16")[0]["order"]) == ("big", "little")
    assert _stats("s_wiz")[0]["photometric"] == 0 and _stats("s_rgba16_mm")[0]["samples"] == 4 and _stats("s_rgb8_pred_rps7")[0]["samples"] == 3
    h = _stats("s_rgb8_pred_rps7")[0]
    assert (h["predictor"], h["rows_per_strip"], h["rows"][-1]) == (2, 7, 5)
    h = _stats("s_sem")[0]
    assert (h["databar_height"], h["focal_length_35mm"], h["sem"]) == (5, 35, True)


def test_tiled_scenes_reach_their_cases():
    for c in tiff_ext_scenes.COMPRESSIONS:
        h = _stats(f"t_small_{c}")[0]
        assert h["compression"] == c and (h["width"], h["height"], h["strips"], h["tile_width"]) == (5, 3, 1, 16)
        h = _stats(f"t_ragged_{c}")[0]
        assert (h["tiles_across"], h["tiles_down"], h["strips"]) == (3, 3, 9) and h["width"] % 16 and h["height"] % 16
        h = _stats(f"t_exact_{c}")[0]
        assert (h["tile_width"], h["tile_length"], h["strips"]) == (h["width"], h["height"], 1)
        h = _stats(f"t_wide_{c}")[0]
        assert h["tile_width"] > h["width"] and (h["tiles_across"], h["tiles_down"]) == (1, 2)
    for name in ("g8", "g16", "rgb8", "rgb16"):
        # 600 pixels in chunks of 256 lanes: tiles of 16 restart four times inside a wave, of 256 at every chunk's end, of 272
        # carry over the chunk's end at 256 and restart in mid-chunk at 272 and 544
        for tw, across in ((16, 38), (256, 3), (272, 3)):
            h = _stats(f"t_pred_{name}_{tw}")[0]
            assert (h["predictor"], h["width"], h["tile_width"], h["tiles_across"]) == (2, 600, tw, across)
    assert _stats("t_pred_g8_272_raw")[0]["compression"] == 1 and _stats("t_pred_rgb8_16_lzw")[0]["compression"] == 5
    h = _stats("t_rgba_out_of_order")[0]
    assert h["offsets"] != sorted(h["offsets"]) and any(o % 4 for o in h["offsets"]) and h["samples"] == 4
    h = _stats("t_sem")[0]
    assert (h["databar_height"], h["focal_length_35mm"], h["sem"], h["predictor"], h["compression"], h["strips"]) == (5, 35, True, 2, 8, 9)
    # the padding of the edge tiles is decoded and dropped: it is there, and it is not the picture's
    data, h = tiff_ext_scenes.scene("t_ragged_1"), _stats("t_ragged_1")[0]
    last = data[h["offsets"][8]:h["offsets"][8] + h["counts"][8]]
    assert last[-1] == 0xAB and len(last) == 256


@pytest.mark.parametrize("name", sorted(tiff_ext_scenes.refused()))
def test_refused(name):
    data, code, header = tiff_ext_scenes.refused()[name]
    with pytest.raises(ref_tiff.TiffError) as err:
        ref_tiff_ext.decode(data)
    assert err.value.code == code
    if header:
        with pytest.raises(ref_tiff.TiffError) as err:
            ref_tiff_ext.parse(data)
        assert err.value.code == code
    else:
        assert ref_tiff_ext.parse(data)["width"] > 0


def test_the_strip_readers_refusals():
    """What the strip reader refuses is refused here with the same code, but for its tiles and its Deflate compressions."""
    for name, (data, code) in tiff_scenes.refused().items():
        with pytest.raises(ref_tiff.TiffError) as err:
            ref_tiff_ext.decode(data)
        want = ref_tiff.INVALID if name in ("u_tiles", "u_compression_8", "u_compression_32946") else code
        assert err.value.code == want, name
