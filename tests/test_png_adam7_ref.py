"""tests/ref_png_adam7.py, the definition of cvhip_png_ext_decode's pixels, without a GPU: it equals Pillow
on every valid scene Pillow exposes samples for, it equals ref_png_in.decode of the same samples written without
interlacing, zlib.decompress of every stream has the passes' length, and the scenes of tests/png_adam7_scenes.py reach
their cases - the patterns of missing passes, Up / Average / Paeth on every pass's first row, the segment counts, and the
rows that cross a batch of 64 rows or a tile of 384 bytes."""
import io
import zlib

import numpy as np
import pytest

import png_adam7_scenes as scenes
import png_in_scenes as base
import ref_png_adam7 as ref
import ref_png_in


def test_samples_are_pillows():
    """L, LA, RGB, RGBA, P, 1/2/4-bit grey and I;16 (16-bit RGB and grey + alpha Pillow reduces itself: not compared)."""
    from PIL import Image

    compared = 0
    for name in scenes.names():
        want = scenes.restated(name)
        h, s = want["header"], want["samples"]
        im = Image.open(io.BytesIO(scenes.scene(name)))
        im.load()
        assert im.info.get("interlace") == 1 and h["interlace"] == 1, name
        if h["depth"] == 16 and h["colour"] != 0:
            continue
        got = np.asarray(im)
        compared += 1
        if h["colour"] == 0 and h["depth"] == 16:
            assert (got.astype(np.int64) == s[:, :, 0]).all(), name
        elif h["colour"] == 0 and h["depth"] < 8:
            scale = 1 if im.mode == "1" else 255 // ((1 << h["depth"]) - 1)
            assert (got.astype(np.int64) == s[:, :, 0] * scale).all(), name
        elif h["colour"] == 3:
            assert im.mode == "P" and (got.astype(np.int64) == s[:, :, 0]).all(), name
            assert (np.asarray(im.convert("RGB")) == want["rgb"]).all(), name
        else:
            assert im.mode == {0: "L", 2: "RGB", 4: "LA", 6: "RGBA"}[h["colour"]], name
            assert (got.reshape(s.shape).astype(np.int64) == s).all(), name
    assert compared >= len(scenes.SWEEP) + len(scenes.SUB_BYTE) + 20


def test_the_same_samples_without_interlacing():
    for name in scenes.names():
        want, plain = scenes.restated(name), ref_png_in.decode(scenes.plain(name), fast=True)
        assert (want["samples"] == scenes.spec(name)[0]).all() and (plain["samples"] == want["samples"]).all(), name
        assert (plain["luma"] == want["luma"]).all() and (plain["rgb"] == want["rgb"]).all(), name
        # a file that is not interlaced through this restatement: ref_png_in's, one pass, the plain segments
        again = ref.decode(scenes.plain(name), fast=True)
        assert again["header"]["passes"] == 1 and again["header"]["filtered"] == len(plain["filtered"]), name
        assert (again["rgb"] == plain["rgb"]).all() and (again["luma"] == plain["luma"]).all(), name
        types = ref.filter_types(again["filtered"], again["header"])[0]
        assert again["row_segments"] == len(base.segments_of(types)), name
    for name in ("s_47x33_rgb", "f_third_sub", "s_pal2_trns", "k_grey_d1_385", "x_short_be"):
        again, plain = ref.decode(base.scene(name), fast=True), base.restated(name)
        assert (again["rgb"] == plain["rgb"]).all() and (again["luma"] == plain["luma"]).all(), name
        assert ref.info(base.scene(name)) == ref_png_in.info(base.scene(name))


def test_streams_have_the_passes_length():
    for name in scenes.names():
        data = scenes.scene(name)
        h = ref.parse(data)
        filtered = zlib.decompress(ref_png_in.stream_of(data, h))
        assert len(filtered) == h["filtered"] == sum(e["height"] * (1 + e["row_bytes"]) for e in h["pass_table"]), name
        assert filtered == scenes.restated(name)["filtered"], name   # ref_png_in.inflate's bytes
        assert h["pass_rows"] == sum(e["height"] for e in h["pass_table"])
        assert sum(e["width"] * e["height"] for e in h["pass_table"]) == h["width"] * h["height"], name   # every pixel is in one pass


def test_geometry_against_a_plain_count():
    """pass_table's sizes are the counts of the pixels (x, y) with x = x0 mod dx, y = y0 mod dy."""
    for w in range(1, 20):
        for h in range(1, 20):
            table, total = ref.pass_table(w, h, 24)
            seen = np.zeros((h, w), dtype=int)
            for p, e in enumerate(table):
                xs, ys = range(ref.X0[p], w, ref.DX[p]), range(ref.Y0[p], h, ref.DY[p])
                assert (e["width"], e["height"]) == ((len(xs), len(ys)) if len(xs) and len(ys) else (0, 0))
                assert (1 << e["log_dx"], 1 << e["log_dy"]) == (ref.DX[p], ref.DY[p])
                for y in ys:
                    for x in xs:
                        seen[y, x] += 1
                        # the kernel's rule for a pixel's pass
                        assert p == (6 if y & 1 else 5 if x & 1 else 4 if y & 2 else 3 if x & 2 else 2 if y & 4 else 1 if x & 4 else 0)
            assert (seen == 1).all()


def test_the_sweep_reaches_every_pattern_of_passes():
    patterns, first = set(), [set() for _ in range(7)]
    for w, h in scenes.SWEEP:
        r = scenes.restated("z_%dx%d" % (w, h))
        present = tuple(e["height"] > 0 for e in r["header"]["pass_table"])
        patterns.add(present)
        for p, types in enumerate(ref.filter_types(r["filtered"], r["header"])):
            if types:
                first[p].add(types[0])
        assert present[1] == (w > 4) and present[2] == (h > 4) and present[3] == (w > 2) and present[4] == (h > 2), (w, h)
        assert present[5] == (w > 1) and present[6] == (h > 1), (w, h)
    assert scenes.restated("z_1x1")["header"]["passes"] == 1 and scenes.restated("z_9x9")["header"]["passes"] == 7
    assert len(patterns) == 16   # x: passes 1, 3, 5 vanish below 5, 3, 2 columns - four patterns; y alike
    for p in range(7):
        assert first[p] >= {2, 3, 4}, p


def test_sub_byte_scenes():
    for kind, d, w, h in scenes.SUB_BYTE:
        name = "k_%s_d%d_%dx%d" % (kind, d, w, h)
        r = scenes.restated(name)
        head = r["header"]
        if kind == "pal":
            assert len(head["palette"]) == 3 * ((1 << d) - 1)
            # the padding bits are ones wherever a pass row has any
            for e, rows in ref.pass_rows(r["filtered"], head, fast=True):
                spare = e["row_bytes"] * 8 - e["width"] * d
                assert (rows[:, -1] & ((1 << spare) - 1) == (1 << spare) - 1).all(), name
    spares = {e["row_bytes"] * 8 - e["width"] * d for kind, d, w, h in scenes.SUB_BYTE for e in scenes.restated("k_%s_d%d_%dx%d" % (kind, d, w, h))["header"]["pass_table"]
              if e["height"]}
    assert spares == {0, 1, 2, 3, 4, 5, 6, 7}


def test_every_type_is_there():
    assert len(scenes.TYPES) == 30
    for c, d, w, h in scenes.TYPES:
        head = scenes.restated("s_c%d_d%d_%dx%d" % (c, d, w, h))["header"]
        assert (head["colour"], head["depth"], head["width"], head["height"], head["passes"]) == (c, d, w, h, 7)


def test_seam_scenes_reach_their_seams():
    T, B = base.TILE_BYTES, base.BATCH_ROWS
    for name, p, rows in (("b_9x131_grey8", 6, 65), ("b_9x521_rgba16", 0, 66)):
        r = scenes.restated(name)
        assert r["header"]["pass_table"][p]["height"] == rows > B
        assert r["header"]["passes"] == 7 and r["row_segments"] == 7, name
        assert all(set(types) == {4} for types in ref.filter_types(r["filtered"], r["header"]))
    r = scenes.restated("t_521x9_rgba16")
    table = r["header"]["pass_table"]
    assert (table[0]["row_bytes"], table[6]["row_bytes"]) == (528, 4168) and T < 528 < 2 * T and 4168 > 10 * T
    assert {t for types in ref.filter_types(r["filtered"], r["header"]) for t in types} == {3, 4}
    assert scenes.restated("t_131x9_rgb8")["header"]["pass_table"][6]["row_bytes"] == 393 == T + 9
    assert scenes.restated("t_131x9_rgb16")["header"]["pass_table"][6]["row_bytes"] == 786 == 2 * T + 18


def test_mixed_and_stream_scenes():
    r = scenes.restated("m_40x40")
    types = ref.filter_types(r["filtered"], r["header"])
    for p in range(7):
        assert types[p] == [scenes.MIXED[p][y % len(scenes.MIXED[p])] for y in range(len(types[p]))]
    assert r["row_segments"] == sum(len(base.segments_of(t)) for t in types) == 2 + 1 + 2 + 3 + 5 + 10 + 6   # counted by hand, pass by pass
    # the cuts: every pass's filter byte ends a chunk's predecessor and is a chunk of its own
    data = scenes.scene("i_pass_cuts")
    h = ref.parse(data)
    assert len(h["idat"]) == 15 and [n for _o, n, _c in h["idat"]][1::2] == [1] * 7
    at, ends = 0, []
    for _o, n, _c in h["idat"]:
        at += n
        ends.append(at - 7)
    assert [e["offset"] for e in h["pass_table"]] == ends[0:14:2]
    assert scenes.restated("i_mem1")["stats"]["dynamic"] > 20
    s = scenes.restated("i_stored")["stats"]
    assert s["stored"] >= 1 and s["fixed"] == s["dynamic"] == 0


def test_refused_files_raise_their_code():
    for name, (data, code) in scenes.refused().items():
        with pytest.raises(ref.PngError) as raised:
            ref.decode(data)
        assert raised.value.code == code, name
    assert str(pytest.raises(ref.PngError, ref.decode, scenes.refused()["i_plain_stream"][0]).value) == "output that is not the passes' bytes"
    assert str(pytest.raises(ref.PngError, ref.decode, scenes.refused()["i_adam7_stream"][0]).value) == "output that is not the passes' bytes"
    assert str(pytest.raises(ref.PngError, ref.decode, scenes.refused()["i_pass_short"][0]).value) == "output that is not the passes' bytes"
    assert str(pytest.raises(ref.PngError, ref.parse, scenes.refused()["u_passes_2g"][0]).value) == "passes of 2^31 bytes or more"
    # the old definition still refuses every interlaced file as not built, and reads the 2^31 header when it is not interlaced
    for name in ("z_9x9", "o_13x21"):
        assert pytest.raises(ref_png_in.PngError, ref_png_in.parse, scenes.scene(name)).value.code == ref.UNSUPPORTED
    plain = bytearray(scenes.refused()["u_passes_2g"][0])
    plain[28] = 0
    plain[29:33] = zlib.crc32(bytes(plain[12:29])).to_bytes(4, "big")
    assert ref.parse(bytes(plain))["filtered"] == 65535 * 32768 == ref_png_in.parse(bytes(plain))["height"] * (ref_png_in.parse(bytes(plain))["row_bytes"] + 1)
    # pass 1's only pixel holds the index beyond the PLTE
    data = scenes.refused()["i_index_beyond_pass1"][0]
    h = ref.parse(data)
    e = h["pass_table"][1]
    assert (e["width"], e["height"]) == (1, 1) and zlib.decompress(ref_png_in.stream_of(data, h))[e["offset"] + 1] >> 6 == 3 == len(h["palette"]) // 3
