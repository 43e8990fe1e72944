"""cvhip_surface_subset and cvhip_select_smallest_u64 (max_points, triangulation.rs:837-843) on the device
against the restatement (tests/ref_subset.py), exactly: the kept rows, the gathered points and track rows, host arrays and
device tensors, every output left out in turn, and every argument error.  Output buffers are filled with 0xA5 before each call
and must hold it past out_n, and everywhere after an error."""
import ctypes as C

import numpy as np
import pytest

import ref_subset
from cybervision_amd import _lib, triangulation

pytestmark = pytest.mark.gpu

W, G = triangulation.SUBSET_WG_ROWS, triangulation.SUBSET_GRID_ROWS
SIZES = [1, 2, 63, 64, 65, 255, 256, 257, W - 1, W, W + 1, G + 1, 2**20 + 3]
PAD = 19       # elements of every output buffer past min(n, m)
FILL = 0xA5
INVALID, UNSUPPORTED = -1, -3


def counts(n):
    return sorted({0, 1, 2, n // 2, n - 1, n, n + 1})


def _ptr(a):
    if a is None:
        return None
    return C.c_void_p(a.data_ptr() if hasattr(a, "data_ptr") else a.ctypes.data)


def filled(count, dtype, device):
    """`count` elements of 0xA5 bytes: a numpy array, or a device tensor viewed through numpy's dtype."""
    host = np.full(int(count) * np.dtype(dtype).itemsize, FILL, dtype=np.uint8)
    if not device:
        return host.view(dtype)
    import torch

    return torch.from_numpy(host).cuda()


def as_host(buf, dtype):
    return buf.cpu().numpy().view(dtype) if hasattr(buf, "data_ptr") else buf


def untouched(a):
    return bool((np.ascontiguousarray(a).view(np.uint8) == FILL).all())


def to_device(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a).reshape(-1).view(np.uint8).copy()).cuda()


def device_select(dev, keys, n, m, device=False, rows=True):
    """One cvhip_select_smallest_u64 call on `keys` (numpy or device bytes) -> (rc, out_n, rows buffer on the host)."""
    k = min(n, m)
    out_rows = filled(k + PAD, np.uint64, device) if rows else None
    out_n = C.c_uint64(0xA5A5)
    rc = _lib.lib().cvhip_select_smallest_u64(dev.handle, _ptr(keys), n, m, _ptr(out_rows), C.byref(out_n))
    return rc, out_n.value, None if out_rows is None else as_host(out_rows, np.uint64)


def device_subset(dev, n, m, seed, points, tracks, m_cams, device=False, want=(True, True, True)):
    """One cvhip_surface_subset call -> (rc, out_n, rows, points, tracks buffers on the host; None where not asked for)."""
    k = min(n, m)
    out_rows = filled(k + PAD, np.uint64, device) if want[0] else None
    out_points = filled((k + PAD) * 3, np.float64, device) if want[1] else None
    out_tracks = filled((k + PAD) * 2 * m_cams, np.int32, device) if want[2] else None
    out_n = C.c_uint64(0xA5A5)
    rc = _lib.lib().cvhip_surface_subset(dev.handle, n, m, seed, _ptr(points), _ptr(tracks), m_cams, _ptr(out_rows), _ptr(out_points),
                                         _ptr(out_tracks), C.byref(out_n))
    host = [None if b is None else as_host(b, t) for b, t in ((out_rows, np.uint64), (out_points, np.float64), (out_tracks, np.int32))]
    return (rc, out_n.value, *host)


def check_rows(got, out_n, want):
    assert out_n == len(want)
    assert np.array_equal(got[:out_n], want)
    assert untouched(got[out_n:])


def surface_arrays(n, m_cams, seed=1):
    rng = np.random.default_rng(seed)
    points = rng.standard_normal((n, 3))
    tracks = rng.integers(-1, 4096, size=(n, m_cams, 2), dtype=np.int32)
    return points, tracks


@pytest.mark.parametrize("n", SIZES)
def test_select_shapes(gpu_device, n):
    """Random full-width keys and keys from 0 .. 15 (ties at every size) at every n and m; the large sizes from device memory."""
    rng = np.random.default_rng(n)
    device = n > 4 * W
    for keys in (rng.integers(0, 2**64, size=n, dtype=np.uint64), rng.integers(0, 16, size=n, dtype=np.uint64)):
        order = ref_subset.key_order(keys)
        d_keys = to_device(keys) if device else keys
        for m in counts(n):
            rc, out_n, rows = device_select(gpu_device, d_keys, n, m, device=device)
            assert rc == 0, _lib.lib().cvhip_last_error()
            check_rows(rows, out_n, ref_subset.select_smallest(keys, m, order))


def key_set(name, n, rng):
    top = np.uint64(0x0123456789ABCD00)
    if name == "all_equal":
        return np.full(n, 0xDEADBEEF12345678, dtype=np.uint64)
    if name == "bit0":
        return np.uint64(0x8000000000000000) | rng.integers(0, 2, size=n, dtype=np.uint64)
    if name == "low_byte":
        return top | rng.integers(0, 256, size=n, dtype=np.uint64)
    if name == "low_byte_duplicates":
        return top | rng.integers(0, 7, size=n, dtype=np.uint64) * np.uint64(37)
    if name == "extremes":
        return np.where(rng.integers(0, 2, size=n) == 1, np.uint64(2**64 - 1), np.uint64(0))
    if name == "ascending":
        return np.arange(n, dtype=np.uint64) * np.uint64(0x0000010000000001)
    if name == "descending":
        return (np.uint64(2**64 - 1) - np.arange(n, dtype=np.uint64) * np.uint64(0x0000010000000001))
    if name == "small_values":
        return rng.integers(0, 16, size=n, dtype=np.uint64)
    assert name == "full_width"
    return rng.integers(0, 2**64, size=n, dtype=np.uint64)


@pytest.mark.parametrize("name", ["all_equal", "bit0", "low_byte", "low_byte_duplicates", "extremes", "ascending", "descending",
                                  "small_values", "full_width"])
def test_select_key_sets(gpu_device, name):
    """The key sets where a radix descent or the tie rule can go wrong, within a wave, past a workgroup trip and over several."""
    rng = np.random.default_rng(len(name))
    for n in (65, W + 1, 3 * W + 77):
        keys = key_set(name, n, rng)
        order = ref_subset.key_order(keys)
        for m in counts(n) + [n // 3, W]:
            for device in (False, True):
                rc, out_n, rows = device_select(gpu_device, to_device(keys) if device else keys, n, m, device=device)
                assert rc == 0, _lib.lib().cvhip_last_error()
                check_rows(rows, out_n, ref_subset.select_smallest(keys, m, order))


def test_select_past_2_31_rows(gpu_device):
    """2^31 + W + 1 descending keys, generated in device memory (17 GB): the m smallest are the LAST m rows, all past 2^31 -
    the row arithmetic is 64-bit and the counters hold more than 2^31.  The keys differ in their top bytes, so the first pass
    counts every row into its bins."""
    import torch

    n = 2**31 + W + 1
    keys = torch.arange(n - 1, -1, -1, dtype=torch.int64, device="cuda").bitwise_left_shift_(30)
    torch.cuda.synchronize()
    for m in (1, W + 3):
        rc, out_n, rows = device_select(gpu_device, keys, n, m, device=True)
        assert rc == 0, _lib.lib().cvhip_last_error()
        check_rows(rows, out_n, np.arange(n - m, n, dtype=np.uint64))
    del keys
    torch.cuda.empty_cache()


def test_select_without_rows(gpu_device):
    keys = np.arange(100, dtype=np.uint64)
    assert device_select(gpu_device, keys, 100, 7, rows=False)[:2] == (0, 7)
    assert device_select(gpu_device, keys, 100, 700, rows=False)[:2] == (0, 100)
    assert device_select(gpu_device, None, 0, 5)[:2] == (0, 0)


@pytest.mark.parametrize("n", SIZES)
def test_subset_shapes(gpu_device, n):
    """The hashed subset at every n and m with three cameras, rows, points and track rows; the large sizes in device memory."""
    seed, m_cams = 3, 3
    points, tracks = surface_arrays(n, m_cams)
    device = n > 4 * W
    d_points, d_tracks = (to_device(points), to_device(tracks)) if device else (points, tracks)
    order = ref_subset.key_order(ref_subset.keys(n, seed))
    for m in counts(n):
        rc, out_n, rows, pts, trk = device_subset(gpu_device, n, m, seed, d_points, d_tracks, m_cams, device=device)
        assert rc == 0, _lib.lib().cvhip_last_error()
        want = ref_subset.subset_rows(n, m, seed) if m >= n else ref_subset.select_smallest(ref_subset.keys(n, seed), m, order)
        check_rows(rows, out_n, want)
        idx = want.astype(np.int64)
        assert pts[:out_n * 3].tobytes() == points[idx].tobytes() and untouched(pts[out_n * 3:])
        assert trk[:out_n * 2 * m_cams].tobytes() == tracks[idx].tobytes() and untouched(trk[out_n * 2 * m_cams:])


@pytest.mark.parametrize("seed", [0, 1, 3, 2**64 - 1])
def test_subset_seeds_cameras_and_outputs(gpu_device, seed):
    """Every seed with 1, 2, 3 and 8 cameras, host arrays and device tensors, and each output left out in turn (its input too)."""
    n = 2 * W + 77
    for m_cams in (1, 2, 3, 8):
        points, tracks = surface_arrays(n, m_cams, seed=m_cams)
        sources = {False: (points, tracks), True: (to_device(points), to_device(tracks))}
        for m in (1, n // 4, n - 1, n, n + 5):
            want = ref_subset.subset_rows(n, m, seed)
            idx = want.astype(np.int64)
            for device in (False, True):
                src_p, src_t = sources[device]
                for wanted in ((True, True, True), (False, True, True), (True, False, True), (True, True, False), (False, False, False)):
                    rc, out_n, rows, pts, trk = device_subset(gpu_device, n, m, seed, src_p if wanted[1] else None,
                                                              src_t if wanted[2] else None, m_cams if wanted[2] else 0, device=device,
                                                              want=wanted)
                    assert rc == 0, _lib.lib().cvhip_last_error()
                    assert out_n == len(want)
                    if rows is not None:
                        check_rows(rows, out_n, want)
                    if pts is not None:
                        assert pts[:out_n * 3].tobytes() == points[idx].tobytes() and untouched(pts[out_n * 3:])
                    if trk is not None:
                        assert trk[:out_n * 2 * m_cams].tobytes() == tracks[idx].tobytes() and untouched(trk[out_n * 2 * m_cams:])


def test_python_wrappers(gpu_device):
    """triangulation.subset on a perspective-shaped surface and on affine_surface's, and triangulation.select_smallest."""
    n = W + 300
    points, tracks = surface_arrays(n, 3)
    cams = [triangulation.Camera(np.zeros(3), np.zeros(3), np.eye(3, 4)) for _ in range(3)]
    surface = triangulation.Surface(points=points, track_index=np.arange(n, dtype=np.int64)[::-1].copy(), tracks=tracks, cameras=cams,
                                    ba_iterations=4, ba_history=[1, 0, 1, 1], ba_residual_norms=(2.0, 1.0))
    got, info = triangulation.subset(gpu_device, surface, 100, seed=9)
    want = ref_subset.subset_rows(n, 100, 9)
    idx = want.astype(np.int64)
    assert set(info) == {"rows_in", "rows_out", "seed", "rows"} and (info["rows_in"], info["rows_out"], info["seed"]) == (n, 100, 9)
    assert np.array_equal(info["rows"], want)
    assert got.points.tobytes() == points[idx].tobytes() and got.tracks.tobytes() == tracks[idx].tobytes()
    assert np.array_equal(got.track_index, surface.track_index[idx])
    assert got.cameras is surface.cameras and (got.ba_iterations, got.ba_history, got.ba_residual_norms) == (4, [1, 0, 1, 1], (2.0, 1.0))
    whole, info = triangulation.subset(gpu_device, surface, n)
    assert info["rows_out"] == n and whole.points.tobytes() == points.tobytes() and whole.tracks.tobytes() == tracks.tobytes()
    affine = triangulation.affine_surface(np.round(points * 100), tracks[:, 0])
    got, info = triangulation.subset(gpu_device, affine, 50, seed=2)
    idx = ref_subset.subset_rows(n, 50, 2).astype(np.int64)
    assert got.points.tobytes() == affine.points[idx].tobytes() and got.tracks.tobytes() == affine.tracks[idx].tobytes()
    assert np.array_equal(got.track_index, idx) and len(got.cameras) == 2
    keys = np.random.default_rng(0).integers(0, 50, size=n, dtype=np.uint64)
    assert np.array_equal(triangulation.select_smallest(gpu_device, keys, 333), ref_subset.select_smallest(keys, 333))


def test_argument_errors(gpu_device):
    """Every CVHIP_ERR_INVALID and CVHIP_ERR_UNSUPPORTED case of the two entry points; nothing is written."""
    L = _lib.lib()
    n, m_cams = 100, 2
    points, tracks = surface_arrays(n, m_cams)
    keys = np.arange(n, dtype=np.uint64)

    def subset_rc(dev=gpu_device.handle, n=n, points=points, tracks=tracks, m_cams=m_cams, rows=True, pts=True, trk=True, out=True):
        bufs = [filled(100 * c, t, False) if on else None for on, c, t in ((rows, 1, np.uint64), (pts, 3, np.float64), (trk, 16, np.int32))]
        out_n = C.c_uint64(0xA5A5)
        rc = L.cvhip_surface_subset(dev, n, 10, 0, _ptr(points), _ptr(tracks), m_cams, *(_ptr(b) for b in bufs),
                                    C.byref(out_n) if out else None)
        assert out_n.value == 0xA5A5 and all(untouched(b) for b in bufs if b is not None)
        return rc

    assert subset_rc(dev=None) == INVALID
    assert subset_rc(out=False) == INVALID
    assert subset_rc(points=None) == INVALID
    assert subset_rc(tracks=None, m_cams=0) == INVALID
    assert subset_rc(m_cams=0) == INVALID
    assert subset_rc(m_cams=0, trk=False) == INVALID  # tracks of no camera, even when they are not gathered
    assert subset_rc(m_cams=9) == UNSUPPORTED
    assert subset_rc(n=2**32 - 1) == UNSUPPORTED
    assert subset_rc(n=2**40) == UNSUPPORTED

    def select_rc(dev=gpu_device.handle, keys=keys, n=n, out=True):
        rows = filled(100, np.uint64, False)
        out_n = C.c_uint64(0xA5A5)
        rc = L.cvhip_select_smallest_u64(dev, _ptr(keys), n, 10, _ptr(rows), C.byref(out_n) if out else None)
        assert out_n.value == 0xA5A5 and untouched(rows)
        return rc

    assert select_rc(dev=None) == INVALID
    assert select_rc(out=False) == INVALID
    assert select_rc(keys=None) == INVALID
    assert select_rc(n=2**32 - 1) == UNSUPPORTED
