"""The progressive JPEG decoder on the device (cvhip_jpeg_progressive_decode; csrc/jpeg_prog_kernels.hip,
csrc/jpeg_prog_common.hpp) against tests/ref_jpeg_prog.py, the definition of the pixels.  Every comparison is
byte equality.  The scenes (tests/jpeg_prog_scenes.py) are the smallest at which each part can break;
tests/test_jpeg_prog_ref.py checks, without a GPU, that they reach those cases and that Pillow decodes them to the same
pixels."""
import ctypes as C

import numpy as np
import pytest

import jpeg_prog_scenes
import jpeg_scenes
import ref_jpeg_prog
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


def _levels(scans):
    """The launch level of every scan (components, Ss, Se, Ah, Al, ..): a first scan 0; a refinement one behind every earlier
    scan of one of its components whose band overlaps its own."""
    levels = []
    for k, b in enumerate(scans):
        behind = [la + 1 for a, la in zip(scans[:k], levels) if b[3] and set(a[0]) & set(b[0]) and a[1] <= b[2] and b[1] <= a[2]]
        levels.append(max(behind, default=0))
    return levels


@pytest.mark.parametrize("name", jpeg_prog_scenes.names())
def test_pixels_are_the_restated_pixels(gpu_device, name):
    """Pillow's progressive files (libjpeg's default script: all four scan kinds) at 1 x 1, 8 x 8, 17 x 9 and 33 x 47 in
    every sampling and in grey, quality 50 and 95, restart intervals of 1 and 3 blocks, an EXIF block, grey noise without DRI
    whose AC-first scan has more than 256 subsequences, a flat 256 x 256 image (long EOB runs); and the writer's files: DC
    scans per component and three refinement passes, Y alone and then Cb + Cr with DRI changing between scans, the refinement
    cases (ZRL over history, a new coefficient at Se, history behind the last new one, correction bits inside an EOB run, a
    run that ends on the scan's last block) with and without restart intervals, 16-bit codes, an EOB run of 16384 blocks; and
    the seam scenes (jpeg_prog_scenes.SEAMS; tests/test_jpeg_prog_ref.py proves each reaches its seam): correction fields of every
    piece count, subsequences of an interleaved DC scan that begin inside the MCU, 289 restart intervals in every scan, a
    workgroup seam inside a later first scan with EOB runs, the byte kernels' 64- and 256-byte edges in later scans, per-component
    DC scans of a 4:2:0 file under DRI 5 and 1, refinement intervals of 1 .. 17 bytes, Al = 5 and 6.
    The counts of the last decode are the restatement's."""
    data = jpeg_prog_scenes.scene(name)
    want = jpeg_prog_scenes.restated(name)
    assert same(image.decode_jpeg_progressive(gpu_device, data, "RGB"), want["rgb"])
    stats = image.jpeg_progressive_last_stats()
    met = want["met"]
    assert (stats["scans"], stats["intervals"], stats["longest_eob_run"]) == (len(met["scans"]), met["intervals"], met["longest_eob_run"])
    assert stats["subsequences"] == sum(met["subsequences"])
    refinements = [level for s, level in zip(met["scans"], _levels(met["scans"])) if s[1] > 0 and s[3] > 0]
    assert (stats["ac_refinement_scans"], stats["ac_refinement_launches"]) == (len(refinements), len(set(refinements)))
    assert same(image.decode_jpeg_progressive(gpu_device, data, "L"), want["luma"])
    info = image.jpeg_progressive_info(data)
    assert (info["height"], info["width"], info["scans"]) == want["luma"].shape + (len(met["scans"]),)
    assert info["focal_length_35mm"] == jpeg_prog_scenes.FOCAL.get(name)


def test_the_noise_scene_needs_more_than_one_workgroup(gpu_device):
    """No DRI and an AC-first scan of more than 256 subsequences (tests/test_jpeg_prog_ref.py): the first scans' states settle
    across workgroups of the synchronisation kernel, in a second launch at least; a small file settles in the one launch."""
    image.decode_jpeg_progressive(gpu_device, jpeg_prog_scenes.scene("q_noise_grey"), "L")
    stats = image.jpeg_progressive_last_stats()
    assert stats["intervals"] == stats["scans"] and stats["subsequences"] > 256 and stats["sync_launches"] >= 2 and stats["workgroup_rounds"] >= 1
    image.decode_jpeg_progressive(gpu_device, jpeg_prog_scenes.scene("q_8x8_444"), "L")
    assert image.jpeg_progressive_last_stats()["sync_launches"] == 1


@pytest.mark.parametrize("name", ["p_wide_first", "p_wide_first_codes16"])
def test_the_wide_first_scenes_need_more_than_one_workgroup(gpu_device, name):
    """The workgroup seam lies inside the band 6 .. 63 first scan, behind the DC and band 1 .. 5 scans' lanes, where an EOB run's
    blocks are counted across it."""
    image.decode_jpeg_progressive(gpu_device, jpeg_prog_scenes.scene(name), "L")
    stats = image.jpeg_progressive_last_stats()
    assert stats["intervals"] == stats["scans"] == 6 and stats["subsequences"] > 256 and stats["sync_launches"] >= 2 and stats["workgroup_rounds"] >= 1
    assert stats["longest_eob_run"] == jpeg_prog_scenes.restated(name)["met"]["longest_eob_run"] >= 4


def test_a_restart_interval_per_block_in_every_scan(gpu_device):
    """289 intervals in each of 6 scans: the interval and scan searches, the marker numbering and the segment kernel past one workgroup
    of intervals, 578 refinement waves in two launches; with and without a fill byte."""
    for name in ("p_rst_every_block", "p_rst_every_block_fill"):
        assert same(image.decode_jpeg_progressive(gpu_device, jpeg_prog_scenes.scene(name), "L"), jpeg_prog_scenes.restated(name)["luma"])
        stats = image.jpeg_progressive_last_stats()
        assert stats["intervals"] == 1734 and stats["subsequences"] == 1734 and stats["scans"] == 6
        assert (stats["ac_refinement_scans"], stats["ac_refinement_launches"]) == (2, 2)


def _call(device, data, fmt, drop, out, cap):
    size = C.c_uint64(0xDEAD)
    buf = np.frombuffer(data, dtype=np.uint8) if len(data) else np.zeros(1, dtype=np.uint8)
    rc = _lib.lib().cvhip_jpeg_progressive_decode(device.handle, C.c_void_p(buf.ctypes.data), len(data), fmt, drop, out, cap, C.byref(size))
    return rc, size.value


def test_one_scene_every_way_out(gpu_device):
    import torch

    name = "q_33x47_420_rst3"
    data = jpeg_prog_scenes.scene(name)
    want = jpeg_prog_scenes.restated(name)
    rgb, luma = want["rgb"], want["luma"]
    h, w = luma.shape
    # two calls on one handle; a device tensor; drop_rows
    assert same(image.decode_jpeg_progressive(gpu_device, data, "RGB"), rgb) and same(image.decode_jpeg_progressive(gpu_device, data, "RGB"), rgb)
    assert same(image.decode_jpeg_progressive(gpu_device, data, "RGB", out="device").cpu().numpy(), rgb)
    for drop in (1, h - 1):
        assert same(image.decode_jpeg_progressive(gpu_device, data, "RGB", drop_rows=drop), rgb[:h - drop])
        assert same(image.decode_jpeg_progressive(gpu_device, data, "L", drop_rows=drop), luma[:h - drop])
    # the grey file as RGB8: its plane three times
    grey = jpeg_prog_scenes.restated("q_33x47_grey")
    assert (grey["rgb"] == grey["luma"][:, :, None]).all()
    # out in device memory at offsets 0..3 and 8, between canaries; cap = 0 writes nothing
    for fmt, pixels in ((ref_jpeg_prog.RGB8, rgb), (ref_jpeg_prog.LUMA8, luma)):
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


def _refused_leaves_the_buffer_alone(gpu_device, data, code, size=1 << 16):
    import torch

    buf = np.full(size, 0xA5, dtype=np.uint8)
    for fmt in (ref_jpeg_prog.LUMA8, ref_jpeg_prog.RGB8):
        assert _call(gpu_device, data, fmt, 0, C.c_void_p(buf.ctypes.data), buf.size)[0] == code
        assert (buf == 0xA5).all()
    d_out = torch.full((size,), 0x5A, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    assert _call(gpu_device, data, ref_jpeg_prog.RGB8, 0, C.c_void_p(d_out.data_ptr()), d_out.numel())[0] == code
    torch.cuda.synchronize()
    assert (d_out.cpu().numpy() == 0x5A).all()
    with pytest.raises(_lib.CvhipError) as raised:
        image.decode_jpeg_progressive(gpu_device, data, "RGB")
    assert raised.value.code == code


@pytest.mark.parametrize("name", sorted(jpeg_prog_scenes.refused()))
def test_refused_files_leave_the_buffer_alone(gpu_device, name):
    """Incomplete progressions, a multi-scan SOF0 file and a baseline file (UNSUPPORTED: outside SOF2), scan headers outside
    T.81 G.1, s = 2 in a refinement, a scan cut short, a misnumbered and a missing RSTn (INVALID): the code, and not a byte of `out` written."""
    _refused_leaves_the_buffer_alone(gpu_device, *jpeg_prog_scenes.refused()[name])


@pytest.mark.parametrize("name", jpeg_prog_scenes.REFUSED_SEAMS)
def test_refused_seams_leave_the_buffer_alone(gpu_device, name):
    """A refinement scan that ends inside a 63-bit correction field, a first scan that ends on a subsequence boundary with blocks
    missing, marker 257 of a later scan misnumbered (INVALID): the code, and not a byte of `out` written.  The walk accepts these
    files, so the sizing call answers, and the buffers hold the whole RGB8 image and 16 bytes more: the capacity check passes and the
    refusal is the kernels'."""
    data, code = jpeg_prog_scenes.refused_seams()[name]
    info = ref_jpeg_prog.info(data)
    rgb_bytes = info["width"] * info["height"] * 3
    assert _call(gpu_device, data, ref_jpeg_prog.RGB8, 0, None, 0) == (0, rgb_bytes)
    assert _call(gpu_device, data, ref_jpeg_prog.LUMA8, 0, None, 0) == (0, rgb_bytes // 3)
    _refused_leaves_the_buffer_alone(gpu_device, data, code, size=rgb_bytes + 16)


@pytest.mark.parametrize("name", sorted(jpeg_prog_scenes.COEFFICIENTS))
def test_load_takes_the_progressive_path_and_gives_the_baseline_pixels(gpu_device, tmp_path, name):
    """image.load of a progressive file equals image.load of the baseline file with the same coefficients."""
    w, h, coef, options = jpeg_prog_scenes.COEFFICIENTS[name]()
    (tmp_path / "p.jpg").write_bytes(jpeg_prog_scenes.scene(name))
    (tmp_path / "b.jpg").write_bytes(jpeg_scenes.write(w, h, coef, jpeg_scenes.QUANT_PLAIN, **options))
    got, want = image.load(gpu_device, tmp_path / "p.jpg", rgb=True), image.load(gpu_device, tmp_path / "b.jpg", rgb=True)
    assert same(got.img, want.img) and same(got.rgb, want.rgb)
    assert same(got.img, jpeg_prog_scenes.restated(name)["luma"])
    assert got.focal_length_35mm is None and got.databar_height == 0
    dropped = image.load(gpu_device, tmp_path / "p.jpg", drop_rows=3, out="device")
    assert same(dropped.img.cpu().numpy(), want.img[:h - 3])


def test_load_reads_the_focal_length_of_a_progressive_file(gpu_device, tmp_path):
    (tmp_path / "p.jpg").write_bytes(jpeg_prog_scenes.scene("q_exif"))
    got = image.load(gpu_device, tmp_path / "p.jpg")
    assert got.focal_length_35mm == 28 and same(got.img, jpeg_prog_scenes.restated("q_exif")["luma"])
