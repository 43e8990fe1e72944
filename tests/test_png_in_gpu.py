"""The PNG decoder on the device (cvhip_png_decode; csrc/png_decode_kernels.hip, csrc/png_decode_common.hpp)
against tests/ref_png_in.py, the definition of the pixels.  Every comparison is byte equality.  The scenes
(tests/png_in_scenes.py) are the smallest at which each part can break; tests/test_png_in_ref.py checks, without a GPU, that
they reach those cases and that zlib and Pillow agree with the restatement."""
import ctypes as C

import numpy as np
import pytest

import png_in_scenes as scenes
import ref_png_in as ref
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


def _info(data):
    i = image.png_info(data)
    return (i["width"], i["height"], i["colour_type"], i["bit_depth"], i["interlace"], i["idat_chunks"], i["focal_length_35mm"] or 0,
            int(i["plte"]) | int(i["trns"]) << 1)


@pytest.mark.parametrize("name", scenes.names())
def test_pixels_are_the_restated_pixels(gpu_device, name):
    data = scenes.scene(name)
    want = scenes.restated(name)
    assert same(image.decode_png(gpu_device, data, "RGB"), want["rgb"])
    assert same(image.decode_png(gpu_device, data, "L"), want["luma"])
    assert _info(data) == ref.info(data)
    assert image.png_info(data)["focal_length_35mm"] == scenes.FOCAL.get(name)


@pytest.mark.parametrize("name", scenes.ACCEPTED_HERE)
def test_accepted_here(gpu_device, name):
    """Bytes behind the Adler-32; a distance beyond the window CINFO announces."""
    data = scenes.accepted()[name]
    want = ref.decode(data)
    assert same(image.decode_png(gpu_device, data, "RGB"), want["rgb"]) and same(image.decode_png(gpu_device, data, "L"), want["luma"])


def _call(device, data, fmt, drop, out, cap):
    size = C.c_uint64(0xDEAD)
    buf = np.frombuffer(data, dtype=np.uint8) if len(data) else np.zeros(1, dtype=np.uint8)
    rc = _lib.lib().cvhip_png_decode(device.handle, C.c_void_p(buf.ctypes.data), len(data), fmt, drop, out, cap, C.byref(size))
    return rc, size.value


def test_one_scene_every_way_out(gpu_device):
    import torch

    name = "s_47x33_rgb"
    data = scenes.scene(name)
    want = scenes.restated(name)
    rgb, luma = want["rgb"], want["luma"]
    h, w = luma.shape
    # two calls on one handle; a device tensor; drop_rows
    assert same(image.decode_png(gpu_device, data, "RGB"), rgb) and same(image.decode_png(gpu_device, data, "RGB"), rgb)
    assert same(image.decode_png(gpu_device, data, "RGB", out="device").cpu().numpy(), rgb)
    for drop in (1, h - 1):
        assert same(image.decode_png(gpu_device, data, "RGB", drop_rows=drop), rgb[:h - drop])
        assert same(image.decode_png(gpu_device, data, "L", drop_rows=drop), luma[:h - drop])
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
            assert same(out[offset:offset + size].reshape(pixels.shape), pixels), offset
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


@pytest.mark.parametrize("name", sorted(scenes.refused()))
def test_refused_files_leave_the_buffer_alone(gpu_device, name):
    """Every kind of file that is not built (UNSUPPORTED) and every kind of malformed file (INVALID): the code, from
    cvhip_png_info where the header decides it and from cvhip_png_decode always, and not a byte of `out` written."""
    import torch

    data, code = scenes.refused()[name]
    try:
        ref.parse(data)
        header_code = 0
    except ref.PngError as err:
        header_code = err.code
        assert header_code == code
    buf = np.frombuffer(data, dtype=np.uint8)
    info = np.zeros(8, dtype=np.uint32)
    assert _lib.lib().cvhip_png_info(C.c_void_p(buf.ctypes.data), len(data), C.c_void_p(info.ctypes.data)) == header_code
    buf = np.full(1 << 16, 0xA5, dtype=np.uint8)
    for fmt in (ref.LUMA8, ref.RGB8):
        assert _call(gpu_device, data, fmt, 0, C.c_void_p(buf.ctypes.data), buf.size)[0] == code
        assert (buf == 0xA5).all()
    d_out = torch.full((1 << 16,), 0x5A, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    assert _call(gpu_device, data, ref.RGB8, 0, C.c_void_p(d_out.data_ptr()), d_out.numel())[0] == code
    torch.cuda.synchronize()
    assert (d_out.cpu().numpy() == 0x5A).all()
    with pytest.raises(_lib.CvhipError) as raised:
        image.decode_png(gpu_device, data, "RGB")
    assert raised.value.code == code


def test_stats(gpu_device):
    def stats(name):
        image.decode_png(gpu_device, scenes.scene(name), "L")
        return image.png_last_stats()

    s = stats("b_mem1")
    assert (s["stored_blocks"], s["fixed_blocks"], s["dynamic_blocks"]) == (0, 1, 36)
    s = stats("b_stored")
    assert s["stored_blocks"] >= 1 and s["fixed_blocks"] == s["dynamic_blocks"] == 0
    s = stats("b_noise160")
    assert s["subsequences"] > 256 and s["dynamic_blocks"] == 2
    s = stats("t_fixed_long")
    assert s["settle_windows"] >= 2 and s["subsequences"] > 256     # the block longer than a settle window
    # the flat picture: one literal and copies at distance 1, a chain 40 199 deep - doubling takes 16 rounds and the one
    # that changes nothing
    s = stats("flat200")
    assert 15 <= s["copy_rounds"] <= 32
    # None and Sub rows start a segment
    assert stats("f_130_paeth")["row_segments"] == 1
    assert stats("f_third_sub")["row_segments"] == 24
    # segments that end on batch edges (64, 65 and 63 rows, two rows alone); 130 rows as one segment and as 130
    assert stats("g_segment_edges")["row_segments"] == len(scenes.segments_of(scenes.SEGMENT_EDGES)) == 5
    assert stats("m_bpp3_paeth")["row_segments"] == 1 and stats("m_bpp1_sub")["row_segments"] == 130
    for name in scenes.names():
        want = scenes.restated(name)["stats"]
        s = stats(name)
        assert (s["stored_blocks"], s["fixed_blocks"], s["dynamic_blocks"]) == (want["stored"], want["fixed"], want["dynamic"]), name
        if name in scenes.SEAMS:
            assert s["row_segments"] == len(scenes.segments_of(scenes.SEAMS[name][2])), name


def test_image_load(gpu_device, tmp_path):
    name = "x_short_be"
    (tmp_path / "a.png").write_bytes(scenes.scene(name))
    want = scenes.restated(name)
    src = image.load(gpu_device, tmp_path / "a.png", rgb=True)
    assert same(src.img, want["luma"]) and same(src.rgb, want["rgb"])
    assert src.focal_length_35mm == scenes.FOCAL[name]
    assert (src.scale, src.tilt_angle, src.databar_height) == ((1.0, 1.0), None, 0)
    dev = image.load(gpu_device, tmp_path / "a.png", out="device")
    assert same(dev.img.cpu().numpy(), want["luma"]) and dev.rgb is None
    cut = image.load(gpu_device, tmp_path / "a.png", drop_rows=2)
    assert same(cut.img, want["luma"][:-2])
    (tmp_path / "no.bin").write_bytes(b"neither TIFF nor PNG nor JPEG")
    with pytest.raises(_lib.CvhipError) as raised:
        image.load(gpu_device, tmp_path / "no.bin")
    assert raised.value.code == INVALID
