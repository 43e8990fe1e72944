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


def _rows(name):
    """(bpp, row bytes, the filter type of every row) by zlib's inflate of the file's stream."""
    data = scenes.scene(name)
    h = ref.parse(data)
    filtered = zlib.decompress(ref.stream_of(data, h))
    stride = h["row_bytes"] + 1
    assert len(filtered) == h["height"] * stride
    return h["bpp"], h["row_bytes"], list(filtered[::stride])


@pytest.mark.parametrize("name", sorted(scenes.SEAMS))
def test_seam_scenes_reach_their_seams(name):
    """Every scene of the unfilter kernel's seams: its bpp, its row bytes and its filter types as built, in the file; rows past
    a tile (or exactly one, or two); a segment past a batch where the scene is there for that; under 100 KB or so."""
    bpp, row_bytes, types = scenes.SEAMS[name]
    assert _rows(name) == (bpp, row_bytes, types)
    want = scenes.restated(name)
    assert zlib.decompress(ref.stream_of(scenes.scene(name))) == want["filtered"]
    T, B = scenes.TILE_BYTES, scenes.BATCH_ROWS
    lengths = scenes.segments_of(types)
    assert sum(lengths) == len(types) == want["header"]["height"]
    assert len(scenes.scene(name)) <= 102 * 1024
    kind = name.split("_")[-1]
    if name.startswith("m_bpp") and kind.endswith("tiles"):
        assert row_bytes == int(kind[0]) * T and set(types) == {1, 2, 3, 4} and len(types) == 20
    elif name.startswith("m_bpp"):
        assert row_bytes == 2 * T + bpp and len(types) == 2 * B + 2                      # two tiles and a pixel, two batches and two rows
        assert want["header"]["width"] == {1: 769, 2: 385, 3: 257, 4: 193, 6: 129, 8: 97}[bpp]
        assert (lengths, set(types)) == {"paeth": ([130], {4}), "average": ([130], {3}), "mixed": ([130], {2, 3, 4}), "sub": ([1] * 130, {1})}[kind]
    elif name.startswith("k_"):
        assert want["header"]["depth"] < 8 and bpp == 1 and row_bytes in (T + 1, 2 * T + 1) and types == [1, 4, 3]
        assert (want["header"]["width"] * want["header"]["depth"] - 1) // 8 == row_bytes - 1 and want["header"]["width"] * want["header"]["depth"] % 8 != 0
    # the samples are noise: every byte value at the tiles' edges, so a misplaced byte shows
    rows = ref.unfilter_fast(want["filtered"], len(types), row_bytes, bpp)
    if row_bytes > T:
        assert len(np.unique(rows[:, T - 8:T + 8])) > 16


def test_segment_edges_scene():
    bpp, row_bytes, types = _rows("g_segment_edges")
    assert (bpp, row_bytes) == (3, 450) and row_bytes > scenes.TILE_BYTES
    assert scenes.segments_of(types) == [64, 65, 63, 1, 1]
    starts = [y for y, t in enumerate(types) if y == 0 or t < 2]
    assert starts == [0, 64, 129, 192, 193] and [types[y] for y in starts] == [0, 1, 1, 0, 0]
    # the second batch of the first segment finds no row; of the second, one row; the third segment's batch meets the next
    # segment's first row at lane 63
    assert (starts[1] - starts[0]) % 64 == 0 and (starts[2] - starts[1]) % 64 == 1 and (starts[3] - starts[2]) == 63
    assert {types[y] for y in range(1, 64)} == {4} and {types[y] for y in range(65, 129)} == {2} and {types[y] for y in range(130, 192)} == {3}


def test_stored_block_of_65535():
    st = _stats("t_stored_65535")
    assert [(b[0], b[3]) for b in st["blocks"][:2]] == [(0, 65535), (0, 465)] and st["blocks"][2][0] == 2 and len(st["blocks"]) == 3
    assert (st["stored"], st["fixed"], st["dynamic"]) == (2, 0, 1)
    assert len(scenes.restated("t_stored_65535")["filtered"]) == 260 * 256 >= 65536


def test_the_seam_matrix_is_whole():
    """Over all scenes: for every bpp and every filter type but None, a row longer than a tile under that type; for every bpp
    and Up, Average and Paeth, a row under that type that is the 65th or a later one of its segment."""
    past_tile, past_batch = set(), set()
    for name in scenes.names():
        h = scenes.restated(name)["header"]
        types = list(scenes.restated(name)["filtered"][::h["row_bytes"] + 1])
        since = 0
        for y, t in enumerate(types):
            since = 0 if y == 0 or t < 2 else since + 1
            if h["row_bytes"] > scenes.TILE_BYTES:
                past_tile.add((h["bpp"], t))
            if since >= scenes.BATCH_ROWS:
                past_batch.add((h["bpp"], t))
    assert past_tile >= {(bpp, t) for bpp in scenes.BPP_KINDS for t in (1, 2, 3, 4)}
    assert past_batch >= {(bpp, t) for bpp in scenes.BPP_KINDS for t in (2, 3, 4)}
    # ... and both at once (the carried pixels of a lane that is not in the first batch)
    assert set(scenes.BPP_KINDS) == {1, 2, 3, 4, 6, 8}


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
