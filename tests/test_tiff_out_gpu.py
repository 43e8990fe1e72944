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
    Strips: 1 (inline offset and count), 2, 64, 65, 256, 257, 1025; a short last strip; the default rows per strip.
    The LZW kernel's staging (S.LZW_STAGE bytes at a time; tests/test_tiff_out_ref.py holds each scene to its seam): a code a byte
    in strips of a staging less, equal and more a byte, of two stagings likewise, and of four with the table-full Clear inside -
    1027 codes in a staging; that Clear with the last two and the first two bytes of a staging; strips of 12 such stagings side by
    side in the scratch; a flat strip of 640 stagings, seven of them without a code, where the carried word must survive; every
    carried bit count 0 to 31; Predictor 2 over rows of 1023, 1025 and 1028 bytes, five a strip.  Launches: GRID_LANES / 64 + 6
    strips, the last six equal to the first six - a wave's second strip; 65535 rows, a row a strip, LZW and PackBits;
    GRID_LANES / 256 + 6 PackBits rows, seven a strip - the copy kernel's second trip over rows; rows of 65535 x 4 bytes, PackBits
    and LZW with Predictor 2; PackBits runs of 2 to 4 and 128 to 131 from positions 61 to 66 and 253 to 258 of a row."""
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


@pytest.mark.parametrize("name", ["short_last_strip_lzw", "pb_rgba_sparse", "two_strips_raw_rgb", "pb_1_byte_rows", "odd_strips_raw", "raw_1_byte_strips"])
def test_every_way_in_and_out(gpu_device, name):
    """The last three: units of the copy kernel of 2 bytes (PackBits rows of a byte), of 5 bytes and of 1 byte (raw strips, a
    padding byte between them) - shorter than the bytes in front of the first aligned dword - at every alignment of `out`."""
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


@pytest.mark.parametrize("name", ["pred_rgb8", "pb_rgba_sparse", "two_strips_raw_rgb"])
def test_pixels_at_any_address(gpu_device, name):
    """`pixels` 1, 2 and 3 bytes into a larger device tensor and into a larger host array: the same file.  LZW with Predictor 2
    (the byte `channels` in front is read too), PackBits, and uncompressed, where the copy kernel reads the pixels themselves."""
    import torch

    pixels, cmp_, pred, rps = S.scene(name)
    file = S.expected(name)[0]
    size = len(file)
    h, w, c = pixels.shape
    flat = pixels.reshape(-1)
    out = np.zeros(size, dtype=np.uint8)
    for offset in (1, 2, 3):
        host = np.full(flat.size + 8, 0xA5, dtype=np.uint8)
        host[offset:offset + flat.size] = flat
        dev = torch.from_numpy(host).cuda()
        torch.cuda.synchronize()
        for src in (C.c_void_p(dev.data_ptr() + offset), C.c_void_p(host.ctypes.data + offset)):
            out[:] = 0
            assert _call(gpu_device, src, w, h, c, cmp_, pred, rps, mesh._p(out), size) == (0, size)
            assert same(out, file), offset
        assert (dev.cpu().numpy() == host).all()   # (read only)


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
