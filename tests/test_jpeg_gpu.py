"""The JPEG decoder on the device (cvhip_jpeg_decode; csrc/jpeg_kernels.hip, csrc/jpeg_common.hpp) against
tests/ref_jpeg.py, the definition of the pixels.  Every comparison is byte equality.  The scenes (tests/jpeg_scenes.py) are
the smallest at which each part can break; tests/test_jpeg_ref.py checks, without a GPU, that they reach those cases and
that Pillow decodes the encoder-made ones to the same pixels."""
import ctypes as C

import numpy as np
import pytest

import jpeg_scenes
import ref_jpeg
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


@pytest.mark.parametrize("name", jpeg_scenes.names())
def test_pixels_are_the_restated_pixels(gpu_device, name):
    """1 x 1, 3 x 5 and 4 x 4 at 4:2:0 and 4 x 3 at 4:2:2 (chroma planes of at most 2 columns: replication); 5 x 3 at 4:2:2; 8 x 8; 17 x 9 and
    33 x 47 (partial MCUs both ways) in every sampling and in grey; quality 50, 95 and 100; optimised tables; restart
    intervals of 1 and 3 MCUs and of an MCU row; an EXIF block; 160 x 160 noise without DRI (more subsequences than a
    workgroup has lanes, an FF 00 pair across two workgroups of the byte kernels); a flat image (dozens of MCUs in a
    subsequence); and the writer's files: 16-bit codes, a 16-bit DQT, ZRL chains, a block without EOB, a block longer than
    a subsequence, thirteen intervals with a short last one and FF FF fill.  The seams (tests/test_jpeg_ref.py shows each on
    the CPU): noise with restart intervals over two to four workgroups of the sync kernel in every sampling, an interval
    across a workgroup boundary or at lane 0 of a later one; an RSTn, and FF FF fill with it, split by the 64-byte and 256-byte
    pieces of the byte kernels; DC sums that leave the int16 range, with and without DRI."""
    data = jpeg_scenes.scene(name)
    want = jpeg_scenes.restated(name)
    assert same(image.decode_jpeg(gpu_device, data, "RGB"), want["rgb"])
    assert same(image.decode_jpeg(gpu_device, data, "L"), want["luma"])
    info = image.jpeg_info(data)
    assert (info["height"], info["width"]) == want["luma"].shape
    assert info["focal_length_35mm"] == jpeg_scenes.FOCAL.get(name)


def _call(device, data, fmt, drop, out, cap):
    size = C.c_uint64(0xDEAD)
    buf = np.frombuffer(data, dtype=np.uint8) if len(data) else np.zeros(1, dtype=np.uint8)
    rc = _lib.lib().cvhip_jpeg_decode(device.handle, C.c_void_p(buf.ctypes.data), len(data), fmt, drop, out, cap, C.byref(size))
    return rc, size.value


def test_one_scene_every_way_out(gpu_device):
    import torch

    name = "e_33x47_420_rst1"
    data = jpeg_scenes.scene(name)
    want = jpeg_scenes.restated(name)
    rgb, luma = want["rgb"], want["luma"]
    h, w = luma.shape
    # two calls on one handle; a device tensor; drop_rows
    assert same(image.decode_jpeg(gpu_device, data, "RGB"), rgb) and same(image.decode_jpeg(gpu_device, data, "RGB"), rgb)
    assert same(image.decode_jpeg(gpu_device, data, "RGB", out="device").cpu().numpy(), rgb)
    for drop in (1, h - 1):
        assert same(image.decode_jpeg(gpu_device, data, "RGB", drop_rows=drop), rgb[:h - drop])
        assert same(image.decode_jpeg(gpu_device, data, "L", drop_rows=drop), luma[:h - drop])
    # the grey file as RGB8: its plane three times
    grey = jpeg_scenes.restated("e_17x9_grey")
    assert (grey["rgb"] == grey["luma"][:, :, None]).all()
    assert same(image.decode_jpeg(gpu_device, jpeg_scenes.scene("e_17x9_grey"), "RGB"), grey["rgb"])
    # out in device memory at offsets 0..3 and 8, between canaries; cap = 0 writes nothing
    for fmt, pixels in ((ref_jpeg.RGB8, rgb), (ref_jpeg.LUMA8, luma)):
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
        # a buffer that is too small: the code, and nothing written, on the device and on the host
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
        # the image fits the buffer exactly
        assert _call(gpu_device, data, fmt, 0, p, size) == (0, size) and same(buf.reshape(pixels.shape), pixels)


@pytest.mark.parametrize("name", sorted(jpeg_scenes.refused()))
def test_refused_files_leave_the_buffer_alone(gpu_device, name):
    """Every kind of file that is not built (UNSUPPORTED) and every kind of malformed file (INVALID): the code, from
    cvhip_jpeg_info where the header decides it and from cvhip_jpeg_decode always, and not a byte of `out` written."""
    import torch

    data, code = jpeg_scenes.refused()[name]
    with pytest.raises(ref_jpeg.JpegError) as err:
        ref_jpeg.decode(data)
    assert err.value.code == code
    buf = np.full(1 << 16, 0xA5, dtype=np.uint8)
    for fmt in (ref_jpeg.LUMA8, ref_jpeg.RGB8):
        assert _call(gpu_device, data, fmt, 0, C.c_void_p(buf.ctypes.data), buf.size)[0] == code
        assert (buf == 0xA5).all()
    d_out = torch.full((1 << 16,), 0x5A, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    assert _call(gpu_device, data, ref_jpeg.RGB8, 0, C.c_void_p(d_out.data_ptr()), d_out.numel())[0] == code
    torch.cuda.synchronize()
    assert (d_out.cpu().numpy() == 0x5A).all()
    with pytest.raises(_lib.CvhipError) as raised:
        image.decode_jpeg(gpu_device, data, "RGB")
    assert raised.value.code == code


@pytest.mark.parametrize("name", sorted(jpeg_scenes.RESTART))
def test_restart_scenes_need_more_than_one_workgroup(gpu_device, name):
    """Restart intervals over several workgroups of the sync kernel (tests/test_jpeg_ref.py: an interval across a workgroup
    boundary, or at lane 0 of a later one): the intervals and subsequences the restatement counts, and a second launch."""
    data = jpeg_scenes.scene(name)
    at = jpeg_scenes.seams(data)
    assert same(image.decode_jpeg(gpu_device, data, "L"), jpeg_scenes.restated(name)["luma"])
    stats = image.jpeg_last_stats()
    assert (stats["intervals"], stats["subsequences"]) == (at["intervals"], at["subsequences"])
    assert stats["subsequences"] > 256 and stats["sync_launches"] >= 2


def test_the_noise_scene_needs_more_than_one_workgroup(gpu_device):
    data = jpeg_scenes.scene("e_noise160_444")
    image.decode_jpeg(gpu_device, data, "L")
    stats = image.jpeg_last_stats()
    assert stats["intervals"] == 1 and stats["subsequences"] > 256 and stats["sync_launches"] >= 2
