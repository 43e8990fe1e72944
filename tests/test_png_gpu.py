"""The PNG encoder on the device (cvhip_png_encode; csrc/png_kernels.hip, csrc/png_common.hpp) against
tests/ref_png.py, the definition of the file.  Every comparison is byte equality.  The scenes (tests/png_scenes.py) are the
smallest at which each part can break; tests/test_png_ref.py checks, without a GPU, that they reach those cases and that
zlib and Pillow decode the expected files to the input."""
import ctypes as C
import io

import numpy as np
import pytest

import png_scenes
from cybervision_amd import _lib, mesh

pytestmark = pytest.mark.gpu
NAMES = sorted(png_scenes.scenes())
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
    """1x1 images (no match, HLIT = 257); a column of 300 rows of a few bits each (many rows in one dword); runs of exactly 2,
    3, 4, 258 .. 261, 516 and 517 (match splitting, symbol 285, HLIT = 286); every channel count at an odd width and every
    fixed filter; the adaptive choice with ties; the 15-bit limit; an 80 001-byte row (look-ahead across steps, Adler sums
    past 32 bits); 1025 rows, and 4500 rows (more than a launch has waves: a wave takes a second row); flat and smooth
    images; run_seams, 517 rows of one run each that begins around lanes 0 .. 2 and 61 .. 63 with every length at which the
    look past a step breaks in another lane or byte, the chunks of 258 or the rest of one or two literals change; the
    run_ends images, whose runs of zeros end with their row 0 to 319 bytes past a step, a zero behind them; a column of 70000
    rows (more than Adler's 65521 behind a row, 18 rows a wave)."""
    pixels, kind = png_scenes.scenes()[name]
    want = png_scenes.restated(name)
    sections = []
    got = mesh.png(gpu_device, pixels, kind, sections=sections)
    assert same(got, want["file"])
    assert tuple(sections) == want["sections"]


def _call(device, pixels, w, h, c, kind, out, cap, sections=None):
    size = C.c_uint64(0xDEAD)
    rc = _lib.lib().cvhip_png_encode(device.handle, pixels, w, h, c, kind, out, cap, C.byref(size), sections)
    return rc, size.value


def test_adaptive_scene_every_way_in_and_out(gpu_device):
    import torch
    from PIL import Image

    pixels, kind = png_scenes.scenes()["adaptive"]
    want = png_scenes.restated("adaptive")
    file, size = want["file"], len(want["file"])
    h, w, c = pixels.shape
    host = mesh.png(gpu_device, pixels, kind)
    assert same(host, file) and same(mesh.png(gpu_device, pixels, kind), file)  # two calls, the same bytes
    assert (np.asarray(Image.open(io.BytesIO(host.tobytes()))) == pixels).all()
    # pixels from a device tensor
    d_pixels = torch.from_numpy(pixels).cuda()
    assert same(mesh.png(gpu_device, d_pixels, kind), file)
    # out in device memory, at an even and at an odd address; cap = 0 writes nothing
    d_out = torch.full((size + 16,), 0x5A, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    src = C.c_void_p(d_pixels.data_ptr())
    sec = np.zeros(3, dtype=np.uint64)
    assert _call(gpu_device, src, w, h, c, kind, C.c_void_p(d_out.data_ptr()), 0, mesh._p(sec)) == (0, size)
    assert tuple(int(v) for v in sec) == want["sections"]
    assert _call(gpu_device, src, w, h, c, kind, None, 0) == (0, size)
    torch.cuda.synchronize()
    assert (d_out.cpu().numpy() == 0x5A).all()
    for offset in (0, 1, 2, 3, 8):
        d_out.fill_(0x5A)
        torch.cuda.synchronize()
        assert _call(gpu_device, src, w, h, c, kind, C.c_void_p(d_out.data_ptr() + offset), size + 16 - offset) == (0, size)
        torch.cuda.synchronize()
        out = d_out.cpu().numpy()
        assert same(out[offset:offset + size], file), offset
        assert (out[:offset] == 0x5A).all() and (out[offset + size:] == 0x5A).all()
    # a buffer that is too small, and each argument that is refused: the code, and nothing written
    buf = np.full(size, 0xA5, dtype=np.uint8)
    p = mesh._p(pixels)
    for args, code in (((p, w, h, c, kind, mesh._p(buf), size - 1), INVALID),
                       ((p, w, h, c, kind, mesh._p(buf), 1), INVALID),
                       ((p, 0, h, c, kind, mesh._p(buf), size), INVALID),
                       ((p, w, 0, c, kind, mesh._p(buf), size), INVALID),
                       ((p, w, h, 0, kind, mesh._p(buf), size), INVALID),
                       ((p, w, h, 5, kind, mesh._p(buf), size), INVALID),
                       ((p, w, h, c, 6, mesh._p(buf), size), INVALID),
                       ((None, w, h, c, kind, mesh._p(buf), size), INVALID),
                       ((p, w, h, c, kind, None, size), INVALID),
                       ((p, 1 << 31, 1, 2, kind, mesh._p(buf), size), UNSUPPORTED),
                       ((p, 65536, 65536, 1, kind, mesh._p(buf), size), UNSUPPORTED)):
        rc, _size = _call(gpu_device, *args)
        assert rc == code, (args[1:5], rc)
        assert (buf == 0xA5).all()
    d_out.fill_(0x5A)
    torch.cuda.synchronize()
    assert _call(gpu_device, src, w, h, c, kind, C.c_void_p(d_out.data_ptr()), size - 1)[0] == INVALID
    torch.cuda.synchronize()
    assert (d_out.cpu().numpy() == 0x5A).all()
    # the whole image fits the buffer exactly
    assert _call(gpu_device, p, w, h, c, kind, mesh._p(buf), size) == (0, size) and same(buf, file)
