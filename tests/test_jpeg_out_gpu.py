"""The JPEG encoder on the device (cvhip_jpeg_encode; csrc/jpeg_encode_kernels.hip, csrc/jpeg_encode_common.hpp; DESIGN.md
4.20) against tests/ref_jpeg_out.py, the definition of the file.  Every comparison is byte equality.  The scenes
(tests/jpeg_out_scenes.py) are the smallest at which each part can break; tests/test_jpeg_out_ref.py checks, without a GPU,
that they reach those cases and that the expected files are Pillow's."""
import ctypes as C
import io

import numpy as np
import pytest

import jpeg_out_scenes
import ref_jpeg
import ref_jpeg_out
from cybervision_amd import _lib, mesh
from cybervision_amd.mesh import jpeg_encode_last_stats  # (without the encoder every test here fails at this import)

pytestmark = pytest.mark.gpu
NAMES = sorted(jpeg_out_scenes.scenes())
INVALID, UNSUPPORTED = -1, -3  # CVHIP_ERR_INVALID, CVHIP_ERR_UNSUPPORTED


def same(got, want):
    got = np.asarray(got, dtype=np.uint8).tobytes()
    if got != want:
        k = next((i for i, (a, b) in enumerate(zip(got, want)) if a != b), min(len(got), len(want)))
        pytest.fail(f"file images differ: {len(got)} against {len(want)} bytes, first difference at byte {k}: "
                    f"{got[max(k - 16, 0):k + 16].hex()} against {want[max(k - 16, 0):k + 16].hex()}")
    return True


@pytest.mark.parametrize("name", NAMES)
def test_file_is_the_restated_file(gpu_device, name):
    """1x1 images (an MCU of padding, three dummy blocks of four); dummy columns and rows and the order of the bottom edge's
    two replications; odd sizes at every sampling; quality 1, 49, 50, 51, 100; AC category 10 and a coefficient 63; DC
    differences of category 11 in both signs; ZRL and EOB; 6-bit blocks, twenty to a dword, and tables of one symbol; two
    FF bytes in a row, an FF as the padded last byte and as the last byte of a stuffing tile; 5000 and 1536 blocks (more
    than a workgroup, more than one step of the scan); 2 and 4 channels; 49128 blocks at 24 x 65496 (the transform's second
    trip over its 1024 workgroups, a ragged last group, dummies in both trips); 65535 wide and 65535 high (SOF0's FF FF, the
    clamps at the last row and column, 8192 blocks in a line)."""
    pixels, quality, sampling, optimize = jpeg_out_scenes.scenes()[name]
    want = jpeg_out_scenes.restated(name)
    sections = []
    got = mesh.jpeg(gpu_device, pixels, quality, sampling, optimize, sections=sections)
    assert same(got, want["file"])
    assert tuple(sections) == want["sections"]
    assert jpeg_encode_last_stats() == want["stats"]


def scan_of(file: bytes):
    """(bytes up to and including the SOS segment, FF 00 pairs in the scan's data) of a baseline file with one scan"""
    at = 2
    while True:
        assert file[at] == 0xFF
        marker, at = file[at + 1], at + 2 + int.from_bytes(file[at + 2:at + 4], "big")
        if marker == 0xDA:
            return at, file[at:-2].count(b"\xFF\x00")


@pytest.mark.parametrize("name", jpeg_out_scenes.BIG)
def test_past_one_launch_of_lanes(gpu_device, name):
    """More blocks than mesh.GRID_LANES, so the kernels that take a lane a block make a second trip: the histogram, the lengths
    and the write in the grey scene (4104 x 4096 with optimize, 262656 blocks), whose 3.2 MB of unstuffed stream are also more
    than three launches of 1024-byte tiles in the two stuffing kernels; the dummy-DC kernel in the colour scene (3352 x 3352 at
    4:2:0, 264600 blocks), whose last MCUs hold dummy blocks.  The expected file is Pillow's - the restatement would take a
    quarter of a minute, test_jpeg_out_ref.py pins it to Pillow on the grey scene once - and sections and stats are read
    from that file and from the geometry."""
    from PIL import Image

    pixels, quality, sampling, optimize = jpeg_out_scenes.big_scene(name)
    buf = io.BytesIO()
    Image.fromarray(pixels).save(buf, format="JPEG", quality=quality, subsampling=sampling, optimize=optimize)
    want = buf.getvalue()
    head, stuffed = scan_of(want)
    raw = len(want) - head - 2 - stuffed
    g = ref_jpeg_out.geometry(pixels.shape[1], pixels.shape[0], 1 if pixels.ndim == 2 else 3, sampling)
    blocks = g["mcus_x"] * g["mcus_y"] * g["blocks_per_mcu"]
    dummies = g["mcus_x"] * g["mcus_y"] * g["hs"] * g["vs"] - g["blocks_x"] * g["blocks_y"]
    assert blocks > mesh.GRID_LANES and (dummies > 0) == (pixels.ndim == 3)
    if pixels.ndim == 2:
        assert raw > 3 * (mesh.GRID_LANES // 256) * ref_jpeg_out.STUFF_TILE
    sections = []
    got = mesh.jpeg(gpu_device, pixels, quality, sampling, optimize, sections=sections)
    assert same(got, want)
    assert tuple(sections) == (head, len(want) - head - 2, 2)
    stats = jpeg_encode_last_stats()
    assert (stats["blocks"], stats["dummy_blocks"], stats["stuffed"]) == (blocks, dummies, stuffed)
    assert 8 * (raw - 1) < stats["bits"] <= 8 * raw


def test_grey_ignores_sampling(gpu_device):
    pixels, quality, _sampling, optimize = jpeg_out_scenes.scenes()["last_byte_ff"]
    want = jpeg_out_scenes.restated("last_byte_ff")["file"]
    for sampling in mesh.JpegSampling:
        assert same(mesh.jpeg(gpu_device, pixels, quality, sampling, optimize), want)


def _call(device, pixels, w, h, c, quality, sampling, optimize, out, cap, sections=None):
    size = C.c_uint64(0xDEAD)
    rc = _lib.lib().cvhip_jpeg_encode(device.handle, pixels, w, h, c, quality, sampling, optimize, out, cap, C.byref(size), sections)
    return rc, size.value


def test_one_scene_every_way_in_and_out(gpu_device):
    import torch
    from PIL import Image

    name = "smooth_rgb_70x50_422_optimize"
    pixels, q, s, o = jpeg_out_scenes.scenes()[name]
    o = int(o)
    want = jpeg_out_scenes.restated(name)
    file, size = want["file"], len(want["file"])
    h, w, c = pixels.shape
    host = mesh.jpeg(gpu_device, pixels, q, s, o)
    assert same(host, file) and same(mesh.jpeg(gpu_device, pixels, q, s, o), file)  # two calls, the same bytes
    opened = np.asarray(Image.open(io.BytesIO(host.tobytes())).convert("RGB"))
    assert opened.shape == pixels.shape and (opened == ref_jpeg.decode(file)).all()  # a picture, and the one the file defines
    # pixels from a device tensor
    d_pixels = torch.from_numpy(pixels).cuda()
    assert same(mesh.jpeg(gpu_device, d_pixels, q, s, o), file)
    # out in device memory, at every alignment; cap = 0 writes nothing
    d_out = torch.full((size + 16,), 0x5A, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    src = C.c_void_p(d_pixels.data_ptr())
    sec = np.zeros(3, dtype=np.uint64)
    assert _call(gpu_device, src, w, h, c, q, s, o, C.c_void_p(d_out.data_ptr()), 0, mesh._p(sec)) == (0, size)
    assert tuple(int(v) for v in sec) == want["sections"]
    assert _call(gpu_device, src, w, h, c, q, s, o, None, 0) == (0, size)
    torch.cuda.synchronize()
    assert (d_out.cpu().numpy() == 0x5A).all()
    for offset in (0, 1, 2, 3, 8):
        d_out.fill_(0x5A)
        torch.cuda.synchronize()
        assert _call(gpu_device, src, w, h, c, q, s, o, C.c_void_p(d_out.data_ptr() + offset), size + 16 - offset) == (0, size)
        torch.cuda.synchronize()
        out = d_out.cpu().numpy()
        assert same(out[offset:offset + size], file), offset
        assert (out[:offset] == 0x5A).all() and (out[offset + size:] == 0x5A).all()
    # a buffer that is too small, and each argument that is refused: the code, and nothing written
    buf = np.full(size, 0xA5, dtype=np.uint8)
    p, b = mesh._p(pixels), mesh._p(buf)
    for args, code in (((p, w, h, c, q, s, o, b, size - 1), INVALID),
                       ((p, w, h, c, q, s, o, b, 1), INVALID),
                       ((p, 0, h, c, q, s, o, b, size), INVALID),
                       ((p, w, 0, c, q, s, o, b, size), INVALID),
                       ((p, 65536, h, c, q, s, o, b, size), INVALID),
                       ((p, w, 65536, c, q, s, o, b, size), INVALID),
                       ((p, w, h, 0, q, s, o, b, size), INVALID),
                       ((p, w, h, 5, q, s, o, b, size), INVALID),
                       ((p, w, h, c, 0, s, o, b, size), INVALID),
                       ((p, w, h, c, 101, s, o, b, size), INVALID),
                       ((p, w, h, c, q, 3, o, b, size), INVALID),
                       ((p, w, h, c, q, s, 2, b, size), INVALID),
                       ((None, w, h, c, q, s, o, b, size), INVALID),
                       ((p, w, h, c, q, s, o, None, size), INVALID),
                       ((p, 65535, 65535, 3, q, 0, o, b, size), UNSUPPORTED),   # 3 * 8192^2 blocks
                       ((p, 65535, 65535, 1, q, 0, o, b, size), UNSUPPORTED)):  # 8192^2 = 2^26 blocks
        rc, _size = _call(gpu_device, *args)
        assert rc == code, (args[1:7], rc)
        assert (buf == 0xA5).all()
    assert _lib.lib().cvhip_jpeg_encode(gpu_device.handle, p, w, h, c, q, s, o, b, size, None, None) == INVALID  # no out_size
    assert _lib.lib().cvhip_jpeg_encode(None, p, w, h, c, q, s, o, b, size, C.byref(C.c_uint64(0)), None) == INVALID  # no device
    assert (buf == 0xA5).all()
    d_out.fill_(0x5A)
    torch.cuda.synchronize()
    assert _call(gpu_device, src, w, h, c, q, s, o, C.c_void_p(d_out.data_ptr()), size - 1)[0] == INVALID
    torch.cuda.synchronize()
    assert (d_out.cpu().numpy() == 0x5A).all()
    # the whole image fits the buffer exactly
    assert _call(gpu_device, p, w, h, c, q, s, o, b, size) == (0, size) and same(buf, file)
