"""Adam7 interlaced PNG files on the device (cvhip_png_ext_decode; csrc/png_decode_kernels.hip, csrc/png_decode_common.hpp;
DESIGN.md 4.24) against tests/ref_png_adam7.py, the definition of the pixels.  Every comparison is byte equality.  The
scenes (tests/png_adam7_scenes.py) are the smallest at which each part can break; tests/test_png_adam7_ref.py checks,
without a GPU, that they reach those cases and that Pillow agrees with the restatement."""
import ctypes as C

import numpy as np
import pytest

import png_adam7_scenes as scenes
import png_in_scenes
import ref_png_adam7 as ref
from cybervision_amd import _lib, image

pytestmark = pytest.mark.gpu
INVALID, UNSUPPORTED = -1, -3  # CVHIP_ERR_INVALID, CVHIP_ERR_UNSUPPORTED


def same(got, want, what=""):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == np.uint8, what
    bad = np.argwhere(got != want)
    if len(bad):
        at = tuple(int(v) for v in bad[0])
        pytest.fail(f"{what}: {len(bad)} of {want.size} bytes differ, the first at {at}: {int(got[at])} against {int(want[at])}")
    return True


def _info(data):
    i = image.png_ext_info(data)
    return (i["width"], i["height"], i["colour_type"], i["bit_depth"], i["interlace"], i["idat_chunks"], i["focal_length_35mm"] or 0,
            int(i["plte"]) | int(i["trns"]) << 1)


def _check(device, names):
    for name in names:
        data, want = scenes.scene(name), scenes.restated(name)
        assert same(image.decode_png_ext(device, data, "RGB"), want["rgb"], name)
        assert same(image.decode_png_ext(device, data, "L"), want["luma"], name)
        assert _info(data) == ref.info(data) and _info(data)[4] == 1, name
        s = image.png_ext_last_stats()
        assert (s["row_segments"], s["passes"]) == (want["row_segments"], want["header"]["passes"]), name
        block_counts = (s["stored_blocks"], s["fixed_blocks"], s["dynamic_blocks"])
        assert block_counts == (want["stats"]["stored"], want["stats"]["fixed"], want["stats"]["dynamic"]), name


def test_the_size_sweep(gpu_device):
    """Every (w, h) in 1..9 x 1..9: all patterns of missing passes, Up / Average / Paeth on every pass's first row."""
    _check(gpu_device, ["z_%dx%d" % wh for wh in scenes.SWEEP])


def test_sub_byte_rows(gpu_device):
    """Grey and palette at 1, 2 and 4 bits; the palette files have a short PLTE and padding bits that are ones."""
    _check(gpu_device, ["k_%s_d%d_%dx%d" % k for k in scenes.SUB_BYTE])


def test_every_other_scene(gpu_device):
    """Every colour type and depth, the batch and tile seams, the mixed filters, the stream's shapes."""
    rest = [n for n in scenes.names() if n[0] not in "zk"]
    assert len(rest) == len(scenes.TYPES) + 11
    _check(gpu_device, rest)


def _call(device, data, fmt, drop, out, cap):
    size = C.c_uint64(0xDEAD)
    buf = np.frombuffer(data, dtype=np.uint8) if len(data) else np.zeros(1, dtype=np.uint8)
    rc = _lib.lib().cvhip_png_ext_decode(device.handle, C.c_void_p(buf.ctypes.data), len(data), fmt, drop, out, cap, C.byref(size))
    return rc, size.value


def test_one_scene_every_way_out(gpu_device):
    import torch

    name = "o_13x21"
    data = scenes.scene(name)
    want = scenes.restated(name)
    rgb, luma = want["rgb"], want["luma"]
    h, w = luma.shape
    assert (w, h) == (13, 21)
    # two calls on one handle; a device tensor; drop_rows
    assert same(image.decode_png_ext(gpu_device, data, "RGB"), rgb) and same(image.decode_png_ext(gpu_device, data, "RGB"), rgb)
    assert same(image.decode_png_ext(gpu_device, data, "RGB", out="device").cpu().numpy(), rgb)
    for drop in (1, 3, h - 1):
        assert same(image.decode_png_ext(gpu_device, data, "RGB", drop_rows=drop), rgb[:h - drop])
        assert same(image.decode_png_ext(gpu_device, data, "L", drop_rows=drop), luma[:h - drop])
    # out in device memory at offsets 0..3 and 8, between canaries; cap = 0 writes nothing
    for fmt, pixels in ((ref.RGB8, rgb), (ref.LUMA8, luma)):
        size = pixels.size
        d_out = torch.full((size + 16,), 0x5A, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        assert _call(gpu_device, data, fmt, 0, C.c_void_p(d_out.data_ptr()), 0) == (0, size)
        assert _call(gpu_device, data, fmt, 0, None, 0) == (0, size)
        torch.cuda.synchronize()
        assert (d_out.cpu().numpy() == 0x5A).all()
        for offset in (0, 1, 2, 3, 8):
            d_out.fill_(0x5A)
            torch.cuda.synchronize()
            assert _call(gpu_device, data, fmt, 0, C.c_void_p(d_out.data_ptr() + offset), size + 16 - offset) == (0, size)
            torch.cuda.synchronize()
            out = d_out.cpu().numpy()
            assert same(out[offset:offset + size].reshape(pixels.shape), pixels, offset)
            assert (out[:offset] == 0x5A).all() and (out[offset + size:] == 0x5A).all()
        # a buffer one byte short: the code, and nothing written, on the device and on the host
        d_out.fill_(0x5A)
        torch.cuda.synchronize()
        assert _call(gpu_device, data, fmt, 0, C.c_void_p(d_out.data_ptr()), size - 1) == (INVALID, size)
        torch.cuda.synchronize()
        assert (d_out.cpu().numpy() == 0x5A).all()
        buf = np.full(size, 0xA5, dtype=np.uint8)
        p = C.c_void_p(buf.ctypes.data)
        assert _call(gpu_device, data, fmt, 0, p, 1)[0] == INVALID and (buf == 0xA5).all()
        assert _call(gpu_device, data, fmt, h, p, size)[0] == INVALID and (buf == 0xA5).all()        # drop_rows >= H
        assert _call(gpu_device, data, fmt, 0, None, size)[0] == INVALID
        assert _call(gpu_device, data, 2, 0, p, size)[0] == INVALID and (buf == 0xA5).all()          # no such format
        # the image fits the buffer exactly (a host buffer)
        assert _call(gpu_device, data, fmt, 0, p, size) == (0, size) and same(buf.reshape(pixels.shape), pixels)


def test_refused_files_leave_the_buffers_alone(gpu_device):
    """The code from cvhip_png_ext_info where the header decides it and from cvhip_png_ext_decode always, and not a byte of
    `out` written, in host or device memory."""
    import torch

    d_out = torch.full((1 << 16,), 0x5A, dtype=torch.uint8, device="cuda")
    host = np.full(1 << 16, 0xA5, dtype=np.uint8)
    for name, (data, code) in sorted(scenes.refused().items()):
        try:
            ref.parse(data)
            header_code = 0
        except ref.PngError as err:
            header_code = err.code
            assert header_code == code, name
        buf = np.frombuffer(data, dtype=np.uint8)
        info = np.zeros(8, dtype=np.uint32)
        assert _lib.lib().cvhip_png_ext_info(C.c_void_p(buf.ctypes.data), len(data), C.c_void_p(info.ctypes.data)) == header_code, name
        for fmt in (ref.LUMA8, ref.RGB8):
            assert _call(gpu_device, data, fmt, 0, C.c_void_p(host.ctypes.data), host.size)[0] == code, name
            assert (host == 0xA5).all(), name
        torch.cuda.synchronize()
        assert _call(gpu_device, data, ref.RGB8, 0, C.c_void_p(d_out.data_ptr()), d_out.numel())[0] == code, name
        torch.cuda.synchronize()
        assert (d_out.cpu().numpy() == 0x5A).all(), name
        with pytest.raises(_lib.CvhipError) as raised:
            image.decode_png_ext(gpu_device, data, "RGB")
        assert raised.value.code == code, name


def test_the_old_entry_points_answer_as_before(gpu_device):
    """An Adam7 file stays UNSUPPORTED through cvhip_png_info and cvhip_png_decode."""
    data = scenes.scene("o_13x21")
    for call in (lambda: image.png_info(data), lambda: image.decode_png(gpu_device, data, "RGB")):
        with pytest.raises(_lib.CvhipError) as raised:
            call()
        assert raised.value.code == UNSUPPORTED


def test_stats(gpu_device):
    def stats(name):
        image.decode_png_ext(gpu_device, scenes.scene(name), "L")
        return image.png_ext_last_stats()

    # Paeth rows throughout: a segment per pass - seven side by side where the file that is not interlaced has one
    for name in ("b_9x131_grey8", "b_9x521_rgba16"):
        s = stats(name)
        assert (s["row_segments"], s["passes"]) == (7, 7), name
    assert stats("z_1x1")["passes"] == 1 and stats("z_4x1")["passes"] == 3 and stats("z_9x1")["passes"] == 4
    s = stats("m_40x40")
    assert s["row_segments"] == scenes.restated("m_40x40")["row_segments"] == 29 and s["passes"] == 7
    assert stats("i_mem1")["dynamic_blocks"] > 20 and stats("i_stored")["stored_blocks"] >= 1
    # a file that is not interlaced: one pass, cvhip_png_decode's segments; the old statistics are the old entry point's own
    image.decode_png(gpu_device, png_in_scenes.scene("f_130_paeth"), "L")
    image.decode_png_ext(gpu_device, png_in_scenes.scene("f_third_sub"), "L")
    s = image.png_ext_last_stats()
    assert (s["row_segments"], s["passes"]) == (24, 1) and image.png_last_stats()["row_segments"] == 1
    raw = np.full(10, 77, dtype=np.uint64)
    assert _lib.lib().cvhip_png_ext_last_stats(C.c_void_p(raw.ctypes.data)) == 0 and raw[8] == 1 and raw[9] == 0


def test_image_load(gpu_device, tmp_path):
    """image.load sends a file whose IHDR says interlace 1 to the new path (the old one refuses it as not built)."""
    name = "x_exif"
    (tmp_path / "a.png").write_bytes(scenes.scene(name))
    want = scenes.restated(name)
    src = image.load(gpu_device, tmp_path / "a.png", rgb=True)
    assert same(src.img, want["luma"]) and same(src.rgb, want["rgb"])
    assert src.focal_length_35mm == scenes.FOCAL
    assert (src.scale, src.tilt_angle, src.databar_height) == ((1.0, 1.0), None, 0)
    dev = image.load(gpu_device, tmp_path / "a.png", out="device")
    assert same(dev.img.cpu().numpy(), want["luma"]) and dev.rgb is None
    cut = image.load(gpu_device, tmp_path / "a.png", drop_rows=2)
    assert same(cut.img, want["luma"][:-2])


@pytest.mark.parametrize("name", ["s_47x33_rgb16", "m_bpp3_mixed", "k_pal_d4_769", "b_mem1", "x_long_le"])
def test_files_that_are_not_interlaced(gpu_device, name):
    """decode_png_ext gives the bytes decode_png gives."""
    data = png_in_scenes.scene(name)
    for mode in ("RGB", "L"):
        assert same(image.decode_png_ext(gpu_device, data, mode), image.decode_png(gpu_device, data, mode), name)
    assert image.png_ext_info(data) == image.png_info(data)
    assert image.png_ext_last_stats()["passes"] == 1
