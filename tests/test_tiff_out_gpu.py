"""The TIFF encoder on the device (cvhip_tiff_encode; csrc/tiff_encode_kernels.hip, csrc/tiff_encode_common.hpp; DESIGN.md
4.21) against tests/ref_tiff_out.py, the definition of the file.  Every comparison is byte equality.  The scenes
(tests/tiff_out_scenes.py) are the smallest at which each part can break; tests/test_tiff_out_ref.py checks, without a GPU,
that they reach those cases, that the files read back and that the LZW strips are libtiff's."""
import ctypes as C

import numpy as np
import pytest

import tiff_out_scenes as S
from cybervision_amd import _lib, mesh
from cybervision_amd.mesh import tiff_encode_last_stats  # (without the encoder every test here fails at this import)

pytestmark = pytest.mark.gpu
INVALID, UNSUPPORTED = -1, -3  # CVHIP_ERR_INVALID, CVHIP_ERR_UNSUPPORTED


def same(got, want):
    got = np.asarray(got, dtype=np.uint8).tobytes()
    if got != want:
        k = next((i for i, (a, b) in enumerate(zip(got, want)) if a != b), min(len(got), len(want)))
        pytest.fail(f"file images differ: {len(got)} against {len(want)} bytes, first difference at byte {k}: "
                    f"{got[max(k - 16, 0):k + 16].hex()} against {want[max(k - 16, 0):k + 16].hex()}")
    return True


@pytest.mark.parametrize("name", S.names())
def test_file_is_the_restated_file(gpu_device, name):
    """LZW: EOI and the last codes on either side of each change of the code width; Clears at table-full, in mid-strip and in
    front of EOI; a flat strip; 1 x 1; streams that end 1 to 7 bits into a byte, payloads of odd length; Predictor 2 at 1 to 4
    channels, several rows a strip, width 1, wrapping differences; a 64 KB strip, 64 stagings of the kernel.  PackBits: runs of
    2, 3, 127 .. 131 and 258, literals of 127 .. 129, a triple at a row's end, flat rows, 1-byte rows, widths around 64 and 257.
    Strips: 1 (inline offset and count), 2, 64, 65, 256, 257, 1025; a short last strip; the default rows per strip."""
    pixels, compression, predictor, rps = S.scene(name)
    want, stats, want_sections = S.expected(name)
    sections = []
    got = mesh.tiff(gpu_device, pixels, compression, predictor, rps, sections=sections)
    assert same(got, want)
    assert tuple(sections) == want_sections
    assert tiff_encode_last_stats() == stats


def test_python_defaults(gpu_device):
    pixels = S.scene("pred_rgb8")[0]
    import ref_tiff_out as R

    assert same(mesh.tiff(gpu_device, pixels), R.encode(pixels, R.LZW, 2, 0))
    assert same(mesh.tiff(gpu_device, pixels, mesh.TiffCompression.PACKBITS), R.encode(pixels, R.PACKBITS, 1, 0))
    assert same(mesh.tiff(gpu_device, pixels[:, :, 0], mesh.TiffCompression.NONE), R.encode(pixels[:, :, :1], R.NONE, 1, 0))
    assert [int(m) for m in mesh.TiffCompression] == [1, 5, 32773]


def _call(device, pixels, w, h, c, compression, predictor, rps, out, cap, sections=None):
    size = C.c_uint64(0xDEAD)
    rc = _lib.lib().cvhip_tiff_encode(device.handle, pixels, w, h, c, compression, predictor, rps, out, cap, C.byref(size), sections)
    return rc, size.value


@pytest.mark.parametrize("name", ["short_last_strip_lzw", "pb_rgba_sparse", "two_strips_raw_rgb"])
def test_every_way_in_and_out(gpu_device, name):
    import torch

    pixels, cmp_, pred, rps = S.scene(name)
    file, _stats, want_sections = S.expected(name)
    size = len(file)
    h, w, c = pixels.shape
    assert same(mesh.tiff(gpu_device, pixels, cmp_, pred, rps), file) and same(mesh.tiff(gpu_device, pixels, cmp_, pred, rps), file)
    # pixels from a device tensor
    d_pixels = torch.from_numpy(np.array(pixels)).cuda()
    assert same(mesh.tiff(gpu_device, d_pixels, cmp_, pred, rps), file)
    # out in device memory, at every alignment, canaries around it; cap = 0 writes nothing
    d_out = torch.full((size + 16,), 0x5A, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    src = C.c_void_p(d_pixels.data_ptr())
    sec = np.zeros(3, dtype=np.uint64)
    assert _call(gpu_device, src, w, h, c, cmp_, pred, rps, C.c_void_p(d_out.data_ptr()), 0, mesh._p(sec)) == (0, size)
    assert tuple(int(v) for v in sec) == want_sections
    assert _call(gpu_device, src, w, h, c, cmp_, pred, rps, None, 0) == (0, size)
    torch.cuda.synchronize()
    assert (d_out.cpu().numpy() == 0x5A).all()
    for offset in (0, 1, 2, 3):
        d_out.fill_(0x5A)
        torch.cuda.synchronize()
        assert _call(gpu_device, src, w, h, c, cmp_, pred, rps, C.c_void_p(d_out.data_ptr() + offset), size) == (0, size)  # the exact cap
        torch.cuda.synchronize()
        out = d_out.cpu().numpy()
        assert same(out[offset:offset + size], file), offset
        assert (out[:offset] == 0x5A).all() and (out[offset + size:] == 0x5A).all()
    # host pixels into device memory, device pixels into host memory (at an odd address, canaries around)
    d_out.fill_(0x5A)
    torch.cuda.synchronize()
    assert _call(gpu_device, mesh._p(pixels), w, h, c, cmp_, pred, rps, C.c_void_p(d_out.data_ptr() + 1), size) == (0, size)
    torch.cuda.synchronize()
    assert same(d_out.cpu().numpy()[1:1 + size], file)
    buf = np.full(size + 8, 0xA5, dtype=np.uint8)
    for offset in (0, 1, 2, 3):
        buf[:] = 0xA5
        assert _call(gpu_device, src, w, h, c, cmp_, pred, rps, C.c_void_p(buf.ctypes.data + offset), size) == (0, size)
        assert same(buf[offset:offset + size], file) and (buf[:offset] == 0xA5).all() and (buf[offset + size:] == 0xA5).all()
    # a buffer that is too small: refused, nothing written - in host and in device memory
    buf[:] = 0xA5
    for cap in (size - 1, 1):
        assert _call(gpu_device, mesh._p(pixels), w, h, c, cmp_, pred, rps, mesh._p(buf), cap)[0] == INVALID
    assert (buf == 0xA5).all()
    d_out.fill_(0x5A)
    torch.cuda.synchronize()
    assert _call(gpu_device, src, w, h, c, cmp_, pred, rps, C.c_void_p(d_out.data_ptr()), size - 1)[0] == INVALID
    torch.cuda.synchronize()
    assert (d_out.cpu().numpy() == 0x5A).all()


def test_refusals_write_nothing(gpu_device):
    pixels = np.zeros(64, dtype=np.uint8)
    buf = np.full(4096, 0xA5, dtype=np.uint8)
    p, b = mesh._p(pixels), mesh._p(buf)
    for name, (args, code) in S.REFUSED.items():
        rc, _size = _call(gpu_device, p, *args, b, buf.size)
        assert rc == code, (name, rc)
        assert (buf == 0xA5).all()
    L = _lib.lib()
    ok = (4, 4, 1, 5, 1, 0)
    assert _call(gpu_device, None, *ok, b, buf.size)[0] == INVALID
    assert _call(gpu_device, p, *ok, None, buf.size)[0] == INVALID
    assert L.cvhip_tiff_encode(gpu_device.handle, p, *ok, b, buf.size, None, None) == INVALID  # no out_size
    assert L.cvhip_tiff_encode(None, p, *ok, b, buf.size, C.byref(C.c_uint64(0)), None) == INVALID  # no device
    assert L.cvhip_tiff_encode_last_stats(None) == INVALID
    assert (buf == 0xA5).all()
