"""The TIFF decoder on the device (cvhip_tiff_decode; csrc/tiff_kernels.hip, csrc/tiff_common.hpp) against
tests/ref_tiff.py, the definition of the pixels and the metadata.  Every comparison is equality.  The scenes
(tests/tiff_scenes.py) are the smallest at which each part can break; tests/test_tiff_ref.py checks, without a GPU, that
they reach those cases and that Pillow (libtiff) reads the same samples."""
import ctypes as C
import functools

import numpy as np
import pytest

import ref_tiff
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
    data, stats = tiff_scenes.scene(name), {}
    return {"luma": ref_tiff.decode(data, ref_tiff.LUMA8), "rgb": ref_tiff.decode(data, ref_tiff.RGB8, stats=stats), "stats": stats}


@pytest.mark.parametrize("name", tiff_scenes.names())
def test_pixels_are_the_restated_pixels(gpu_device, name):
    """1 x 1 and 3 x 5; 33 x 47 in strips of 1, 7 (a short last strip), 47 and no RowsPerStrip; 70 strips (more than a
    workgroup has waves); grey and RGB(A) in 8 and 16 bits and both byte orders; WhiteIsZero; Predictor 2 with every
    compression, on rows of 257, 300 and 600 pixels (longer than a wave's and a workgroup's span of the scan); strips out of file
    order and at odd offsets; LZW: literals only, the self-overlapping code throughout, Clears in mid-stream and in pairs, no
    initial Clear, no EOI, junk behind EOI, 12-bit codes, a full table, libtiff's 600 x 500 noise file; PackBits: header 128,
    runs and literals of 128, packets crossing row ends, a packet cut at the strip's end; Pillow's files of each kind.  The
    batches' seams (tests/test_tiff_ref.py shows each on the CPU): strips of 64, 65, 128, 129 and 200 packets in one launch,
    a run, a literal, a header 128 and a cut packet as a batch's first; Clears at lane 63 and lane 0 of a 64-code batch, in
    pairs too; rows that are full with a batch's last code, with EOI behind it and without."""
    data = tiff_scenes.scene(name)
    want = restated(name)
    assert same(image.decode_tiff(gpu_device, data, "RGB", 0), want["rgb"])
    stats = image.tiff_last_stats()
    assert same(image.decode_tiff(gpu_device, data, "L", 0), want["luma"])
    info, ref = image.tiff_info(data), ref_tiff.info(data)
    assert (info["height"], info["width"]) == want["luma"].shape
    scale = tuple(float(v) for v in ref["scale"])
    assert info == {**ref, "scale": scale, "tilt_angle": None if ref["tilt_angle"] is None else float(ref["tilt_angle"])}
    # what the decompression met: the restatement's counts
    assert stats["strips"] == info["strips"]
    assert (stats["codes"], stats["clears"], stats["longest"]) == tuple(want["stats"].get(k, 0) for k in ("codes", "clears", "longest"))


def test_stats_show_the_cases(gpu_device):
    image.decode_tiff(gpu_device, tiff_scenes.scene("o_70_strips_lzw"), "L", 0)
    assert image.tiff_last_stats()["strips"] == 70
    image.decode_tiff(gpu_device, tiff_scenes.scene("p_noise_600x500_lzw"), "L", 0)
    stats, want = image.tiff_last_stats(), restated("p_noise_600x500_lzw")["stats"]
    # (more than 1790 codes between two Clears: 12-bit codes, as libtiff writes them)
    assert 12 in want["widths"] and stats["clears"] == want["clears"] > stats["strips"] > 1 and stats["codes"] == want["codes"]
    assert stats["codes"] > 1790 * stats["clears"]
    image.decode_tiff(gpu_device, tiff_scenes.scene("o_lzw_flat"), "L", 0)
    assert image.tiff_last_stats()["longest"] > 64   # (strings longer than a wave)


def _call(device, data, fmt, drop, out, cap):
    size = C.c_uint64(0xDEAD)
    buf = np.frombuffer(data, dtype=np.uint8) if len(data) else np.zeros(1, dtype=np.uint8)
    rc = _lib.lib().cvhip_tiff_decode(device.handle, C.c_void_p(buf.ctypes.data), len(data), fmt, drop, out, cap, C.byref(size))
    return rc, size.value


@pytest.mark.parametrize("name", ["o_sem_exif", "o_pred_rgb8_lzw"])
def test_one_scene_every_way_out(gpu_device, name):
    import torch

    data = tiff_scenes.scene(name)
    rgb, luma = restated(name)["rgb"], restated(name)["luma"]
    h, w = luma.shape
    databar = ref_tiff.info(data)["databar_height"]
    assert databar == (5 if name == "o_sem_exif" else 0)
    # two calls on one handle; a device tensor; drop_rows, and the file's own DatabarHeight
    assert same(image.decode_tiff(gpu_device, data, "RGB", 0), rgb) and same(image.decode_tiff(gpu_device, data, "RGB", 0), rgb)
    assert same(image.decode_tiff(gpu_device, data, "RGB", 0, out="device").cpu().numpy(), rgb)
    for drop in (1, h - 1):
        assert same(image.decode_tiff(gpu_device, data, "RGB", drop_rows=drop), rgb[:h - drop])
        assert same(image.decode_tiff(gpu_device, data, "L", drop_rows=drop), luma[:h - drop])
    assert same(image.decode_tiff(gpu_device, data, "L"), luma[:h - databar])
    assert same(image.decode_tiff(gpu_device, data, "RGB", image.TIFF_DROP_DATABAR), rgb[:h - databar])
    assert same(ref_tiff.decode(data, ref_tiff.LUMA8, ref_tiff.DROP_DATABAR), luma[:h - databar])
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


@pytest.mark.parametrize("name", sorted(tiff_scenes.refused()))
def test_refused_files_leave_the_buffer_alone(gpu_device, name):
    """Every kind of file that is not built (UNSUPPORTED) and every kind of malformed file (INVALID): the code, from
    cvhip_tiff_info where the header decides it and from cvhip_tiff_decode always, and not a byte of `out` written."""
    import torch

    data, code = tiff_scenes.refused()[name]
    with pytest.raises(ref_tiff.TiffError) as err:
        ref_tiff.decode(data)
    assert err.value.code == code
    try:
        ref_tiff.parse(data)
        assert image.tiff_info(data)["width"] > 0   # (only the decompression refuses it)
    except ref_tiff.TiffError:
        with pytest.raises(_lib.CvhipError) as raised:
            image.tiff_info(data)
        assert raised.value.code == code
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
        image.decode_tiff(gpu_device, data, "RGB")
    assert raised.value.code == code


def test_sem_blocks(gpu_device):
    """The SEM table through cvhip_tiff_info (the host parser is compared field by field in tests/test_tiff_host_cpu.py)."""
    for name, raw, want in tiff_scenes.SEM_BLOCKS:
        info = image.tiff_info(tiff_scenes.sem_file(raw))
        assert (info["scale"][0], info["scale"][1], info["tilt_angle"], info["databar_height"], info["sem"]) == want + (True,), name
