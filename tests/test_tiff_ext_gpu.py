"""Deflate and tiled TIFF files on the device (cvhip_tiff_ext_decode; csrc/tiff_ext_kernels.hip, csrc/tiff_common.hpp with
extended = true) against tests/ref_tiff_ext.py, the definition of the pixels and the metadata.  Every
comparison is equality.  The scenes (tests/tiff_ext_scenes.py) are a few KB to a few tens of KB, the smallest at which each part
can break; tests/test_tiff_ext_ref.py checks, without a GPU, that they reach those cases and that Pillow (libtiff) reads the
same samples."""
import ctypes as C
import functools

import numpy as np
import pytest

import ref_tiff
import ref_tiff_ext
import tiff_ext_scenes
import tiff_scenes
from cybervision_amd import _lib, image

pytestmark = pytest.mark.gpu
INVALID, UNSUPPORTED = -1, -3  # CVHIP_ERR_INVALID, CVHIP_ERR_UNSUPPORTED


def same(got, want):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == np.uint8
    bad = np.argwhere(got != want)
    if len(bad):
        at = tuple(int(v) for v in bad[0])
        pytest.fail(f"{len(bad)} of {want.size} bytes differ, the first at {at}: {int(got[at])} against {int(want[at])}")
    return True


@functools.lru_cache(maxsize=None)
def restated(name):
    data, stats = tiff_ext_scenes.scene(name), {}
    return {"luma": ref_tiff_ext.decode(data, ref_tiff.LUMA8), "rgb": ref_tiff_ext.decode(data, ref_tiff.RGB8, stats=stats), "stats": stats}


@pytest.mark.parametrize("name", tiff_ext_scenes.names())
def test_pixels_are_the_restated_pixels(gpu_device, name):
    """Deflate strips: 1 x 1; a single stored, fixed and dynamic block; several blocks of all kinds with copies across their
    ends; a flat strip (one chain of distance-1 copies); 70 strips; strips out of file order at odd offsets; two identical
    neighbours; a block longer than a settle window; code 32946; both byte orders, 8 and 16 bits, grey, WhiteIsZero, RGB and RGBA.
    Tiles with each of the five compressions: an image smaller than a tile, ragged right and bottom, one tile exactly the image,
    a tile wider than the image.  Predictor 2 in tiles of 16, 256 and 272 pixels on rows of 600, in 8 and 16 bits, grey and RGB,
    on stored and LZW tiles too."""
    data = tiff_ext_scenes.scene(name)
    want = restated(name)
    assert same(image.decode_tiff_ext(gpu_device, data, "RGB", 0), want["rgb"])
    stats = image.tiff_ext_last_stats()
    assert same(image.decode_tiff_ext(gpu_device, data, "L", 0), want["luma"])
    info, ref = image.tiff_ext_info(data), ref_tiff_ext.info(data)
    assert (info["height"], info["width"]) == want["luma"].shape
    scale = tuple(float(v) for v in ref["scale"])
    assert info == {**ref, "scale": scale, "tilt_angle": None if ref["tilt_angle"] is None else float(ref["tilt_angle"])}
    # what the decompression met: the restatement's counts
    st = want["stats"]
    assert stats["streams"] == info["strips"] == st["streams"]
    assert (stats["codes"], stats["clears"], stats["longest"]) == tuple(st.get(k, 0) for k in ("codes", "clears", "longest"))
    assert (stats["stored_blocks"], stats["fixed_blocks"], stats["dynamic_blocks"]) == tuple(st.get(k, 0) for k in ("stored", "fixed", "dynamic"))
    assert (stats["subsequences"], stats["settle_windows"]) == (st.get("subsequences", 0), st.get("windows", 0))
    assert (stats["copy_rounds"] > 0) == (info["compression"] in ref_tiff_ext.DEFLATE)
    # the old entry points still refuse the file
    with pytest.raises(_lib.CvhipError) as raised:
        image.tiff_info(data)
    assert raised.value.code == UNSUPPORTED


def test_stats_are_the_restated_counts(gpu_device):
    """The multi-block, the window-crossing and the flat scene: blocks by kind, subsequences and settle windows equal the
    restatement's counts (ref_tiff_ext.chain_counts, from inflate's block table and each block's first token bit); a chain of n
    distance-1 copies resolves in ceil(log2 n) rounds and the one that changes nothing.  The most settle rounds of a window are
    not restated ("Unpinned"): they are at least one where a subsequence begins inside a token."""
    got = {}
    for name in ("s_mixed", "s_window", "s_flat"):
        image.decode_tiff_ext(gpu_device, tiff_ext_scenes.scene(name), "L", 0)
        got[name] = image.tiff_ext_last_stats()
        st = restated(name)["stats"]
        assert (got[name]["stored_blocks"], got[name]["fixed_blocks"], got[name]["dynamic_blocks"]) == (st["stored"], st["fixed"], st["dynamic"])
        assert (got[name]["subsequences"], got[name]["settle_windows"], got[name]["streams"]) == (st["subsequences"], st["windows"], 1)
    assert min(got["s_mixed"][k] for k in ("stored_blocks", "fixed_blocks", "dynamic_blocks")) >= 1 and got["s_mixed"]["settle_windows"] == 4
    assert got["s_window"]["settle_windows"] == 3 and got["s_window"]["subsequences"] > 256     # the first block takes two windows
    assert got["s_flat"]["copy_rounds"] == 13     # 4094 bytes at distance 1 behind two literals: 12 halvings, and the round that changes nothing
    image.decode_tiff_ext(gpu_device, tiff_ext_scenes.scene("s_70_strips"), "L", 0)
    assert image.tiff_ext_last_stats()["streams"] == 70 and image.tiff_ext_last_stats()["fixed_blocks"] == 70


def _call(device, data, fmt, drop, out, cap):
    size = C.c_uint64(0xDEAD)
    buf = np.frombuffer(data, dtype=np.uint8) if len(data) else np.zeros(1, dtype=np.uint8)
    rc = _lib.lib().cvhip_tiff_ext_decode(device.handle, C.c_void_p(buf.ctypes.data), len(data), fmt, drop, out, cap, C.byref(size))
    return rc, size.value


@pytest.mark.parametrize("name", ["s_rgb8_pred_rps7", "t_sem"])
def test_one_scene_every_way_out(gpu_device, name):
    import torch

    data = tiff_ext_scenes.scene(name)
    rgb, luma = restated(name)["rgb"], restated(name)["luma"]
    h, w = luma.shape
    databar = ref_tiff_ext.info(data)["databar_height"]
    assert databar == (5 if name == "t_sem" else 0)
    # two calls on one handle; a device tensor; drop_rows, and the file's own DatabarHeight
    assert same(image.decode_tiff_ext(gpu_device, data, "RGB", 0), rgb) and same(image.decode_tiff_ext(gpu_device, data, "RGB", 0), rgb)
    assert same(image.decode_tiff_ext(gpu_device, data, "RGB", 0, out="device").cpu().numpy(), rgb)
    for drop in (1, h - 1):
        assert same(image.decode_tiff_ext(gpu_device, data, "RGB", drop_rows=drop), rgb[:h - drop])
        assert same(image.decode_tiff_ext(gpu_device, data, "L", drop_rows=drop), luma[:h - drop])
    assert same(image.decode_tiff_ext(gpu_device, data, "L"), luma[:h - databar])
    assert same(image.decode_tiff_ext(gpu_device, data, "RGB", image.TIFF_DROP_DATABAR), rgb[:h - databar])
    assert same(ref_tiff_ext.decode(data, ref_tiff.LUMA8, ref_tiff.DROP_DATABAR), luma[:h - databar])
    # out in device memory at offsets 0..3 and 8, between canaries; cap = 0 writes nothing
    for fmt, pixels in ((ref_tiff.RGB8, rgb), (ref_tiff.LUMA8, luma)):
        size = pixels.size
        d_out = torch.full((size + 16,), 0x5A, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        assert _call(gpu_device, data, fmt, 0, C.c_void_p(d_out.data_ptr()), 0) == (0, size)
        assert _call(gpu_device, data, fmt, 0, None, 0) == (0, size)
        assert _call(gpu_device, data, fmt, 0xFFFFFFFF, None, 0) == (0, size // h * (h - databar))
        torch.cuda.synchronize()
        assert (d_out.cpu().numpy() == 0x5A).all()
        for offset in (0, 1, 2, 3, 8):
            d_out.fill_(0x5A)
            torch.cuda.synchronize()
            assert _call(gpu_device, data, fmt, 0, C.c_void_p(d_out.data_ptr() + offset), size + 16 - offset) == (0, size)
            torch.cuda.synchronize()
            out = d_out.cpu().numpy()
            assert same(out[offset:offset + size].reshape(pixels.shape), pixels), offset
            assert (out[:offset] == 0x5A).all() and (out[offset + size:] == 0x5A).all()
        # a buffer that is too small: the code, and nothing written, on the device and on the host
        d_out.fill_(0x5A)
        torch.cuda.synchronize()
        assert _call(gpu_device, data, fmt, 0, C.c_void_p(d_out.data_ptr()), size - 1) == (INVALID, size)
        torch.cuda.synchronize()
        assert (d_out.cpu().numpy() == 0x5A).all()
        buf = np.full(size + 3, 0xA5, dtype=np.uint8)
        p = C.c_void_p(buf.ctypes.data)
        assert _call(gpu_device, data, fmt, 0, p, 1)[0] == INVALID and (buf == 0xA5).all()
        assert _call(gpu_device, data, fmt, h, p, size)[0] == INVALID and (buf == 0xA5).all()        # drop_rows >= H
        assert _call(gpu_device, data, fmt, 0xFFFFFFFE, p, size)[0] == INVALID and (buf == 0xA5).all()
        assert _call(gpu_device, data, fmt, 0, None, size)[0] == INVALID
        assert _call(gpu_device, data, 2, 0, p, size)[0] == INVALID and (buf == 0xA5).all()          # no such format
        # the image fits the buffer exactly, at an odd host address too
        assert _call(gpu_device, data, fmt, 0, p, size) == (0, size) and same(buf[:size].reshape(pixels.shape), pixels)
        buf.fill(0xA5)
        assert _call(gpu_device, data, fmt, 0, C.c_void_p(buf.ctypes.data + 3), size) == (0, size)
        assert same(buf[3:].reshape(pixels.shape), pixels) and (buf[:3] == 0xA5).all()


def _refused_everywhere(gpu_device, data, code, header):
    import torch

    if header:
        with pytest.raises(_lib.CvhipError) as raised:
            image.tiff_ext_info(data)
        assert raised.value.code == code
    else:
        assert image.tiff_ext_info(data)["width"] > 0   # (only the decompression refuses it)
    buf = np.full(1 << 16, 0xA5, dtype=np.uint8)
    for fmt in (ref_tiff.LUMA8, ref_tiff.RGB8):
        assert _call(gpu_device, data, fmt, 0, C.c_void_p(buf.ctypes.data), buf.size)[0] == code
        assert (buf == 0xA5).all()
    d_out = torch.full((1 << 16,), 0x5A, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    assert _call(gpu_device, data, ref_tiff.RGB8, 0, C.c_void_p(d_out.data_ptr()), d_out.numel())[0] == code
    torch.cuda.synchronize()
    assert (d_out.cpu().numpy() == 0x5A).all()
    with pytest.raises(_lib.CvhipError) as raised:
        image.decode_tiff_ext(gpu_device, data, "RGB")
    assert raised.value.code == code


@pytest.mark.parametrize("name", sorted(tiff_ext_scenes.refused()))
def test_refused_files_leave_the_buffer_alone(gpu_device, name):
    """Every defined refusal: a stream shorter or longer than its rows, a copy in front of its own stream's first byte - of
    the file's first stream, and of a second one whose neighbour holds the very bytes -, a wrong Adler-32, a bad zlib header,
    block type 3, NLEN, bad code lengths, a symbol that does not exist, a truncated stream; tile sizes that are no multiples of
    16, wrong table sizes, strip tags beside tile tags, 2^31 decompressed bytes; what stays refused.  The code, from
    cvhip_tiff_ext_info where the header decides it and from cvhip_tiff_ext_decode always, and not a byte of `out` written."""
    data, code, header = tiff_ext_scenes.refused()[name]
    with pytest.raises(ref_tiff.TiffError) as err:
        ref_tiff_ext.decode(data)
    assert err.value.code == code
    _refused_everywhere(gpu_device, data, code, header)


@pytest.mark.parametrize("name", sorted(tiff_scenes.refused()))
def test_the_strip_readers_refusals(gpu_device, name):
    """What cvhip_tiff_decode refuses: the restatement's code here too - the same, but for its tile and Deflate files, whose
    strips are no tiles and no zlib streams."""
    data = tiff_scenes.refused()[name][0]
    header = False
    with pytest.raises(ref_tiff.TiffError) as err:
        ref_tiff_ext.decode(data)
    try:
        ref_tiff_ext.parse(data)
    except ref_tiff.TiffError:
        header = True
    _refused_everywhere(gpu_device, data, err.value.code, header)


@pytest.mark.parametrize("name", ["o_pred_g16_ii", "o_rgba8_mm_lzw", "o_rgb16_mm_packbits", "o_70_strips_lzw", "o_pb_batches", "p_noise_600x500_lzw", "o_sem_exif"])
def test_superset(gpu_device, name):
    """Files the old entry point accepts, of each compression: its bytes, its header and its counts through the new one."""
    data = tiff_scenes.scene(name)
    for mode in ("L", "RGB"):
        old = image.decode_tiff(gpu_device, data, mode)
        old_stats = image.tiff_last_stats()
        assert same(image.decode_tiff_ext(gpu_device, data, mode), old)
        new_stats = image.tiff_ext_last_stats()
        assert (new_stats["streams"], new_stats["codes"], new_stats["clears"], new_stats["longest"]) == tuple(old_stats.values())
    info = image.tiff_ext_info(data)
    assert {k: v for k, v in info.items() if not k.startswith("tile")} == image.tiff_info(data)
    assert (info["tile_width"], info["tile_length"], info["tiles_across"]) == (0, 0, 0)
