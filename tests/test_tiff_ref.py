"""tests/ref_tiff.py, the definition of cvhip_tiff_decode's pixels and metadata, against Pillow (libtiff) on the
CPU, and tests/tiff_scenes.py: every steered scene reaches the case it is there for."""
import io

import numpy as np
import pytest

import ref_tiff
import tiff_scenes


def pillow_samples(data):
    from PIL import Image

    a = np.asarray(Image.open(io.BytesIO(data)))
    return a[:, :, None] if a.ndim == 2 else a


@pytest.mark.parametrize("name", tiff_scenes.names())
def test_samples_are_libtiffs(name):
    """The decompressed samples (Predictor 2 undone, nothing else applied) equal Pillow's; then the conversions apply.  The
    scenes Pillow cannot open (16-bit RGB) are compared with the picture they were written from."""
    data = tiff_scenes.scene(name)
    h, a = ref_tiff.samples(data)
    if name in tiff_scenes.NOT_FOR_PILLOW:
        want = tiff_scenes.source(name)
    else:
        want = pillow_samples(data)
        if h["photometric"] == 0 and h["bits"] == 8:
            want = 255 - want   # (Pillow inverts 8-bit WhiteIsZero itself; it leaves 16-bit as stored)
    assert a.shape == want.shape and a.dtype.itemsize == want.dtype.itemsize and want.dtype.kind == "u" and (a == want).all()
    luma, rgb = ref_tiff.decode(data, ref_tiff.LUMA8), ref_tiff.decode(data, ref_tiff.RGB8)
    assert luma.shape == a.shape[:2] and rgb.shape == a.shape[:2] + (3,) and luma.dtype == rgb.dtype == np.uint8
    v = a.astype(np.int64)
    if h["photometric"] == 0:
        v = (255 if h["bits"] == 8 else 65535) - v
    if h["bits"] == 8:
        assert (rgb == (v[:, :, :3] if v.shape[2] > 1 else np.repeat(v, 3, axis=2))).all()
    else:
        assert (np.abs(rgb.astype(np.int64) * 257 - (v[:, :, :3] if v.shape[2] > 1 else v)) <= 128).all()   # (the nearest 8-bit value)
    if v.shape[2] == 1:
        assert (luma == rgb[:, :, 0]).all()


def test_few_scenes_skip_pillow():
    assert set(tiff_scenes.NOT_FOR_PILLOW) <= set(tiff_scenes.names())
    assert 4 * len(tiff_scenes.NOT_FOR_PILLOW) <= len(tiff_scenes.names())


def test_pillow_opens_what_it_wrote_as_written():
    for name, pic in (("p_g16_lzw_pred", tiff_scenes.picture(47, 33, 1, 16, seed=6)), ("p_rgb8_lzw_pred", tiff_scenes.picture(47, 33, 3, seed=8)),
                      ("p_noise_600x500_lzw", tiff_scenes.picture(500, 600, seed=18, kind="noise"))):
        h, a = ref_tiff.samples(tiff_scenes.scene(name))
        assert (a == pic).all(), name
    assert ref_tiff.parse(tiff_scenes.scene("p_g16_lzw_pred"))["predictor"] == 2 and ref_tiff.parse(tiff_scenes.scene("p_g8_lzw"))["compression"] == 5
    assert ref_tiff.parse(tiff_scenes.scene("p_rgb8_packbits"))["compression"] == 32773


def _stats(name):
    stats = {}
    ref_tiff.samples(tiff_scenes.scene(name), stats)
    return stats


def test_scenes_reach_their_cases():
    P = ref_tiff.parse
    assert [P(tiff_scenes.scene(n))["strips"] for n in ("o_g8_rps1", "o_g8_rps7", "o_g8_rps47", "o_g8_rps_absent", "o_g8_rps_large_long")] == [47, 7, 1, 1, 1]
    assert P(tiff_scenes.scene("o_g8_rps7"))["rows"][-1] == 5 and P(tiff_scenes.scene("o_g8_rps7"))["offsets"][0] % 2 == 1
    assert P(tiff_scenes.scene("o_70_strips_lzw"))["strips"] == P(tiff_scenes.scene("o_70_strips_packbits"))["strips"] == 70
    offsets = P(tiff_scenes.scene("o_out_of_order_lzw"))["offsets"]
    assert offsets != sorted(offsets) and offsets != sorted(offsets, reverse=True)
    noise = _stats("p_noise_600x500_lzw")
    assert noise["strips"] > 1 and 12 in noise["widths"] and noise["clears"] > 2 * noise["strips"]
    assert _stats("o_lzw_12_bits")["widths"] == {9, 10, 11, 12}
    lit = _stats("o_lzw_literals")
    assert lit["longest"] == 1 and lit["codes"] > 33 * 47 and lit["clears"] > 1
    trace = {}
    flat = tiff_scenes.picture(64, 64, kind="flat").tobytes()
    tiff_scenes.lzw(flat, trace=trace)
    stats = _stats("o_lzw_flat")
    assert trace["self_overlaps"] >= stats["codes"] - 4 and stats["longest"] > 64   # (all but the first literal, the Clear)
    assert _stats("o_lzw_mid_clear")["clears"] > 3
    two = _stats("o_lzw_two_clears")
    assert two["clears"] >= 4 and two["clears"] % 2 == 0
    data = tiff_scenes.scene("o_lzw_no_initial_clear")
    assert data[P(data)["offsets"][0]] != 0x80 and _stats("o_lzw_no_initial_clear")["clears"] == 0
    full = _stats("o_lzw_full_table")
    assert full["clears"] == 1 and full["codes"] > 4200   # (the table is full after 3839 codes; the stream goes on)
    over = tiff_scenes.refused()["i_lzw_table_overflow"][0]   # ... but not past libtiff's 5119 slots
    stats = {}
    assert len(ref_tiff.unlzw(over[8:8 + P(over)["counts"][0]], 5034, stats)) == 5034 and stats["codes"] == 1 + ref_tiff.MAX_CODES
    with pytest.raises(ref_tiff.TiffError):
        ref_tiff.unlzw(over[8:8 + P(over)["counts"][0]], 5036)
    a, b = tiff_scenes.scene("o_lzw_no_eoi"), tiff_scenes.scene("o_lzw_eoi_junk")
    assert P(b)["counts"][0] >= P(a)["counts"][0] + 5
    # PackBits: the headers met
    def headers(name):
        data, met = tiff_scenes.scene(name), []
        h = P(data)
        for s in range(h["strips"]):
            src, at = data[h["offsets"][s]:h["offsets"][s] + h["counts"][s]], 0
            while at < len(src):
                met.append(src[at])
                at += 1 + (src[at] + 1 if src[at] < 128 else 1 if src[at] > 128 else 0)
        return met
    assert 128 in headers("o_pb_noop")
    assert 129 in headers("o_pb_128") and 127 in headers("o_pb_128")
    assert max(257 - b for b in headers("o_pb_crossing_rows") if b > 128) > 33
    assert sum(257 - b for b in headers("o_pb_cut") if b > 128) > 47 * 33


def _packets(data):
    """Per strip the headers the decoder meets until the strip's rows are full (a header 128 is a packet of no bytes), and
    the bytes the last one reaches past the rows."""
    h, out = ref_tiff.parse(data), []
    for s in range(h["strips"]):
        src, need = data[h["offsets"][s]:h["offsets"][s] + h["counts"][s]], h["rows"][s] * h["row_bytes"]
        at, made, met = 0, 0, []
        while made < need:
            b = src[at]
            met.append(b)
            at += 1 + (b + 1 if b < 128 else 1 if b > 128 else 0)
            made += b + 1 if b < 128 else 257 - b if b > 128 else 0
        assert at == len(src)
        out.append((met, made - need))
    return out


def test_packbits_strips_cross_the_64_packet_batches():
    """o_pb_batches: one launch, a wave per strip, each at its own packet count; what the 64th and the 65th packet are."""
    data = tiff_scenes.scene("o_pb_batches")
    got = _packets(data)
    assert len(got) == len(tiff_scenes.PB_BATCHES) == ref_tiff.parse(data)["strips"]
    kind = lambda b: "noop" if b == 128 else "run" if b > 128 else "lit"
    for (met, over), (count, run_first, noop, cut) in zip(got, tiff_scenes.PB_BATCHES):
        assert len(met) == count and over == cut
        assert [k for k, b in enumerate(met) if b == 128] == ([] if noop is None else [noop])
        if count > 64 and noop is None and not (cut and count == 65):
            assert (kind(met[63]), kind(met[64])) == (("lit", "run") if run_first else ("run", "lit"))
        assert sum(1 for b in met if b in (0, 255)) >= count - 4   # one-byte literals and two-byte runs, but for the first
    counts = [len(met) for met, _ in got]
    assert counts[:6] == [64, 65, 65, 128, 129, 200]
    orders = {(kind(met[63]), kind(met[64])) for met, _ in got if len(met) > 64}
    assert {("run", "lit"), ("lit", "run"), ("lit", "noop")} <= orders          # both ways round; a header 128 first in a batch
    assert any(noop is not None and noop % 64 == 0 for _, _, noop, _ in tiff_scenes.PB_BATCHES)
    # a packet cut by the strip's rows as a batch's first packet: the 65th, and the 129th
    assert [(len(met) - 1) % 64 for met, over in got if over] == [0, 0] and [over for _, over in got if over] == [7, 100]
    # the other PackBits scenes stay inside one batch, but for Pillow's files
    assert max(len(met) for name in ("o_pb_noop", "o_pb_128", "o_pb_crossing_rows", "o_pb_cut") for met, _ in _packets(tiff_scenes.scene(name))) < 64


def _lzw_trace(a, **kw):
    trace = {}
    tiff_scenes.lzw(a.tobytes(), trace=trace, **kw)
    return trace


def test_lzw_clears_and_ends_sit_on_batch_edges():
    """The c-th code since a Clear (the initial one: c = 0) is lane c % 64 of a 64-code batch."""
    g8 = tiff_scenes.picture(47, 33, seed=2)
    for n in tiff_scenes.LZW_CLEAR_EVERY:
        trace = _lzw_trace(g8, clear_every=n)
        assert trace["clear_at"][0] == 0 and len(trace["clear_at"]) >= 4 and set(trace["clear_at"][1:]) == {n}
        assert n % 64 == (63 if n in (63, 127) else 0)
        assert _stats("o_lzw_clear_%d" % n)["clears"] == len(trace["clear_at"])
    trace = _lzw_trace(g8, clear_every=64, clears=2)
    assert trace["clear_at"][:4] == [0, 0, 64, 0] and _stats("o_lzw_two_clears_64")["clears"] == len(trace["clear_at"])
    # the earlier scenes: no mid-stream Clear at lane 0 or 63
    for kw in ({"clear_every": 100}, {"clear_every": 70, "clears": 2}, {"clear_every": 200, "literals": True}):
        assert not {c % 64 for c in _lzw_trace(g8, **kw)["clear_at"] if c} & {0, 63}
    # the rows are full with a batch's last code: EOI is the next batch's first code, or there is none
    a = ref_tiff.samples(tiff_scenes.scene("o_lzw_eoi_first_of_batch"))[1]
    assert (a == ref_tiff.samples(tiff_scenes.scene("o_lzw_full_at_batch_end"))[1]).all() and a.shape[1:] == (33, 1)
    with_eoi, without = _lzw_trace(a), _lzw_trace(a, eoi=False)
    assert with_eoi["clear_at"] == without["clear_at"] == [0]
    assert with_eoi["eoi_at"] % 64 == 0 and with_eoi["eoi_at"] >= 128 and without["eoi_at"] is None
    assert without["codes_after_last_clear"] == with_eoi["eoi_at"]
    assert _stats("o_lzw_full_at_batch_end")["codes"] == _stats("o_lzw_eoi_first_of_batch")["codes"] == 1 + with_eoi["eoi_at"]
    one, other = tiff_scenes.scene("o_lzw_eoi_first_of_batch"), tiff_scenes.scene("o_lzw_full_at_batch_end")
    assert ref_tiff.parse(one)["counts"][0] >= ref_tiff.parse(other)["counts"][0]
    assert _lzw_trace(g8)["eoi_at"] % 64 != 0                                   # (the earlier scenes' strip does not)


@pytest.mark.parametrize("name", sorted(tiff_scenes.refused()))
def test_refused(name):
    data, code = tiff_scenes.refused()[name]
    for fmt in (ref_tiff.LUMA8, ref_tiff.RGB8):
        with pytest.raises(ref_tiff.TiffError) as err:
            ref_tiff.decode(data, fmt)
        assert err.value.code == code
    assert name[0] == ("u" if code == ref_tiff.UNSUPPORTED else "i")


def test_refused_by_pillow_too_where_the_stream_is_broken():
    from PIL import Image

    for name in ("i_lzw_above", "i_lzw_short", "i_pb_short", "i_lzw_table_overflow"):
        with pytest.raises(Exception):
            Image.open(io.BytesIO(tiff_scenes.refused()[name][0])).load()


@pytest.mark.parametrize("name,raw,want", tiff_scenes.SEM_BLOCKS, ids=[b[0] for b in tiff_scenes.SEM_BLOCKS])
def test_sem_blocks(name, raw, want):
    sw, sh, tilt, databar = ref_tiff.sem_bytes(raw)
    got = (float(sw), float(sh), None if tilt is None else float(tilt), databar)
    assert got == want
    assert ref_tiff.sem_metadata(tiff_scenes.sem_file(raw))[:4] == (sw, sh, tilt, databar)


def test_sem_tags():
    a, b = b"[PrivateFei]\nDatabarHeight=3\n", b"[PrivateFei]\nDatabarHeight=4\n"
    S, A = tiff_scenes.sem_file, tiff_scenes.ASCII
    assert ref_tiff.sem_metadata(S(a, 34682))[3:] == (3, True) and ref_tiff.sem_metadata(S(a, 34683))[3:] == (3, True)
    assert ref_tiff.sem_metadata(S(a, 34682, second=(34683, A, b)))[3:] == (4, True)   # 34683 is taken before 34682
    assert ref_tiff.sem_metadata(S(a, 34682, second=(34683, tiff_scenes.BYTE, b)))[3:] == (0, False)   # ... whatever its type
    assert ref_tiff.sem_metadata(S(a, 34682, typ=7))[3:] == (0, False)
    assert ref_tiff.sem_metadata(S(b"ab\0", 34682))[3:] == (0, True)   # (an inline value)
    assert ref_tiff.sem_metadata(tiff_scenes.write(tiff_scenes.picture(3, 3)))[4] is False
    info = ref_tiff.info(tiff_scenes.scene("o_sem_exif"))
    assert info["databar_height"] == 5 and info["focal_length_35mm"] == 35 and info["tilt_angle"] == 0.0
    assert ref_tiff.info(tiff_scenes.scene("o_exif_long_mm"))["focal_length_35mm"] == 70000
    assert ref_tiff.info(tiff_scenes.scene("p_sem"))["databar_height"] == 5
    assert ref_tiff.decode(tiff_scenes.scene("p_sem"), drop_rows=ref_tiff.DROP_DATABAR).shape == (42, 33)


def test_f32_is_rounded_once():
    text = "1.00000005960464477539062500000000000000000000001"
    assert float(ref_tiff.parse_f32(text)) == 1.0000001192092896 and np.float32(float(text)) == np.float32(1.0)
    for s in ("0.1", "16777217", "3.4028235e38", "3.4028236e38", "1e-45", "7e-46", "1.17549435e-38", "123456789.125", "5e-324", "00012.5e+003"):
        # numpy parses a string to f32 through a double, so compare with the exact rational rounded by hand instead
        from fractions import Fraction
        got = ref_tiff.parse_f32(s)
        exact = Fraction(s)
        if np.isinf(got):
            assert exact >= Fraction(2) ** 128 - Fraction(2) ** 103
            continue
        with np.errstate(over="ignore"):
            lo, hi = np.nextafter(got, np.float32(-np.inf)), np.nextafter(got, np.float32(np.inf))
        err = abs(Fraction(float(got)) - exact)
        assert err <= abs(Fraction(float(lo)) - exact) and (np.isinf(hi) or err <= abs(Fraction(float(hi)) - exact)), s
    assert [ref_tiff.parse_f32(s) for s in ("", "+", ".", "e5", "1e", "1e+", " 1", "1 ", "0x10", "1_0", "infin", "1f")] == [None] * 12
    assert [ref_tiff.parse_u32(s) for s in ("", "+", "-0", "-1", " 1", "1.0", "4294967296", "0x1")] == [None] * 8
    assert [ref_tiff.parse_u32(s) for s in ("0", "+3", "007", "4294967295")] == [0, 3, 7, 4294967295]
