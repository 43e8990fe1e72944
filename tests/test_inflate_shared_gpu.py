"""The inflate stage that the PNG reader and the TIFF reader's Deflate strips share (csrc/inflate_stage.inc; DESIGN.md 4.18 and
4.23): one zlib stream through both.  For a byte matrix R of H rows by 1 + W columns whose column 0 is zero, the stream of R's
bytes is the IDAT data of a grey 8-bit PNG of H x W pixels (R is its filtered image, every row of filter type None) and the one
strip of a Deflate grey 8-bit TIFF of H x (1 + W) pixels.  Both readers must give their restatement's pixels (tests/ref_png_in.py,
tests/ref_tiff_ext.py), the same pixels but for column 0, and the same counts of what inflate met.  The streams are the
smallest that reach each branch of the chain kernel; every comparison is equality."""
import ctypes as C
import functools
import math
import zlib

import numpy as np
import pytest

import png_in_scenes
import ref_png_in
import ref_tiff
import ref_tiff_ext
import tiff_ext_scenes
import tiff_scenes
from cybervision_amd import _lib, image

pytestmark = pytest.mark.gpu
INVALID = -1  # CVHIP_ERR_INVALID
WINDOW_BITS = 256 * 1024  # a settle window: 256 subsequences of 1024 bits
SHARED = ("stored_blocks", "fixed_blocks", "dynamic_blocks", "subsequences", "settle_rounds", "settle_windows", "copy_rounds")


def _matrix(h, w, tag, low=0, high=256):
    r = png_in_scenes.rng(tag).integers(low, high, (h, 1 + w)).astype(np.uint8)
    r[:, 0] = 0
    return r


def _mixed():
    """16 x 33: a stored block of four rows; a fixed block of a row of literals and a copy of the stored block's four rows; a
    final dynamic block of a row of literals and a copy of six rows, five of them the fixed block's."""
    fresh = _matrix(6, 32, "shared_mixed")
    row = lambda k: [int(v) for v in fresh[k]]  # noqa: E731
    d = png_in_scenes.Deflate()
    d.stored(fresh[:4].tobytes())
    fixed, dynamic = row(4) + [(132, 165)], row(5) + [(198, 198)]
    d.fixed(fixed)
    d.dynamic(dynamic, final=True)
    raw = png_in_scenes.expand(fixed + dynamic, fresh[:4].tobytes())
    return np.frombuffer(raw, dtype=np.uint8).reshape(16, 33), d.finish(raw)


def _window():
    """200 x 201 of the values 144 .. 255, nine bits each in a fixed block, which zlib ends after 32 767 symbols (memLevel 9):
    more bits than a settle window."""
    r = _matrix(200, 200, "shared_window", 144)
    return r, tiff_ext_scenes.deflate(6, zlib.Z_FIXED, 9)(r.tobytes())


def _stored():
    """256 x 256: a stored block of 65 535 bytes - 64 records, the last of 1 023 bytes - and one of the last byte."""
    r = _matrix(256, 255, "shared_stored")
    raw = r.tobytes()
    d = png_in_scenes.Deflate()
    d.stored(raw[:65535])
    d.stored(raw[65535:], final=True)
    return r, d.finish(raw)


FLAT_COPIES = 4094


def _flat():
    """64 x 64 of zeros: two literals, then 4 094 bytes copied at distance 1."""
    r = np.zeros((64, 64), dtype=np.uint8)
    d = png_in_scenes.Deflate()
    d.fixed([0, 0] + [(258, 1)] * (FLAT_COPIES // 258) + [(FLAT_COPIES % 258, 1)], final=True)
    return r, d.finish(r.tobytes())


STREAMS = {"mixed": _mixed, "window": _window, "stored": _stored, "flat": _flat}


def _files(r, stream):
    h, w = r.shape[0], r.shape[1] - 1
    return png_in_scenes.grey_file(r.tobytes(), w, h, stream), tiff_scenes.write(r[:, :, None], compression=8, rps=h, encoder=lambda strip: stream)


@functools.lru_cache(maxsize=None)
def restated(name):
    r, stream = STREAMS[name]()
    assert zlib.decompress(stream) == r.tobytes() and not r[:, 0].any()
    png, tiff = _files(r, stream)
    stats = {}
    return {"r": r, "png": png, "tiff": tiff, "png_luma": ref_png_in.decode(png)["luma"], "tiff_luma": ref_tiff_ext.decode(tiff, ref_tiff.LUMA8, stats=stats),
            "blocks": stats["inflate"][0]["blocks"], "counts": (stats["subsequences"], stats["windows"])}


def same(got, want):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == np.uint8
    bad = np.argwhere(got != want)
    if len(bad):
        at = tuple(int(v) for v in bad[0])
        pytest.fail(f"{len(bad)} of {want.size} bytes differ, the first at {at}: {int(got[at])} against {int(want[at])}")
    return True


@pytest.mark.parametrize("name", sorted(STREAMS))
def test_one_stream_through_both_readers(gpu_device, name):
    want = restated(name)
    png = image.decode_png(gpu_device, want["png"], "L")
    png_stats = image.png_last_stats()
    tiff = image.decode_tiff_ext(gpu_device, want["tiff"], "L", 0)
    tiff_stats = image.tiff_ext_last_stats()
    assert same(png, want["png_luma"]) and same(tiff, want["tiff_luma"])
    assert same(png, want["r"][:, 1:]) and same(tiff[:, 1:], png)
    assert tiff_stats["streams"] == 1
    assert {k: png_stats[k] for k in SHARED} == {k: tiff_stats[k] for k in SHARED}
    # the restatement's counts (ref_tiff_ext.chain_counts), and that the stream reaches the branch it is named for: from the
    # restatement's block table, (BTYPE, .., bits, ..) per block
    assert (png_stats["subsequences"], png_stats["settle_windows"]) == want["counts"]
    kinds = [b[0] for b in want["blocks"]]
    assert (png_stats["stored_blocks"], png_stats["fixed_blocks"], png_stats["dynamic_blocks"]) == tuple(kinds.count(k) for k in (0, 1, 2))
    if name == "mixed":
        assert kinds == [0, 1, 2]
    if name == "window":
        assert max(b[2] for b in want["blocks"] if b[0] != 0) > WINDOW_BITS + 3 and png_stats["settle_windows"] > len(kinds)
    if name == "stored":
        assert kinds == [0, 0]
    if name == "flat":
        assert png_stats["copy_rounds"] == math.ceil(math.log2(FLAT_COPIES)) + 1


def _call(entry, device, data, fmt, out, cap):
    size = C.c_uint64(0xDEAD)
    buf = np.frombuffer(data, dtype=np.uint8)
    return getattr(_lib.lib(), entry)(device.handle, C.c_void_p(buf.ctypes.data), len(data), fmt, 0, out, cap, C.byref(size))


@pytest.mark.parametrize("extra", [-1, 1])
def test_a_stream_of_the_wrong_size_is_refused_by_both(gpu_device, extra):
    """A stream that inflates to one byte too few, and to one byte too many: CVHIP_ERR_INVALID from both readers, on the host
    and on the device, and not a byte of `out` written."""
    import torch

    r = _matrix(6, 4, "shared_size")
    raw = r.tobytes()
    data = raw[:-1] if extra < 0 else raw + b"\7"
    d = png_in_scenes.Deflate()
    d.stored(data, final=True)
    stream = d.finish(data)
    assert len(zlib.decompress(stream)) == len(raw) + extra
    png, tiff = _files(r, stream)
    with pytest.raises(ref_png_in.PngError) as png_err:
        ref_png_in.decode(png)
    with pytest.raises(ref_tiff.TiffError) as tiff_err:
        ref_tiff_ext.decode(tiff)
    assert png_err.value.code == tiff_err.value.code == INVALID
    for entry, file in (("cvhip_png_decode", png), ("cvhip_tiff_ext_decode", tiff)):
        buf = np.full(1 << 12, 0xA5, dtype=np.uint8)
        for fmt in (ref_tiff.LUMA8, ref_tiff.RGB8):
            assert _call(entry, gpu_device, file, fmt, C.c_void_p(buf.ctypes.data), buf.size) == INVALID
            assert (buf == 0xA5).all()
        d_out = torch.full((1 << 12,), 0x5A, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        assert _call(entry, gpu_device, file, ref_tiff.RGB8, C.c_void_p(d_out.data_ptr()), d_out.numel()) == INVALID
        torch.cuda.synchronize()
        assert (d_out.cpu().numpy() == 0x5A).all()
