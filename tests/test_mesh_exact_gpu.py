"""The mesh stage on the device (csrc/mesh_kernels.hip) against the numpy restatement (tests/ref_mesh.py) on
tests/mesh_exact_scenes.py's scenes, where every threshold rule is met exactly (tests/test_mesh_exact_ref.py counts how
often): r = 0 and dyadic cameras, so that no library function runs and every projection and depth is an exact IEEE result
on both sides.

Everything is compared by equality: equal shapes, equal NaN masks, equal BITS wherever the restatement's value is not NaN.
The stage is one IEEE operation per written operation in the written order, so this follows from the design and is not a
measured number; a kernel with >= for >, < for <=, half-to-even rounding, a plain `<` sort of the vertices or a fused
multiply-add in an interpolation differs from the restatement here."""
import ctypes as C
import functools

import numpy as np
import pytest

import mesh_exact_scenes as mx
import ref_mesh
from cybervision_amd import _lib, mesh

pytestmark = pytest.mark.gpu
THRESHOLDS = (("all", mesh.WIDE_ALL), ("none", mesh.WIDE_NONE), ("default", mesh.WIDE_THRESHOLD_DEFAULT))
SCALES = (-1.0, 0.5)
NO_POLYGONS = np.zeros((0, 3), dtype=np.uint32)


def same_bits(got, want):
    """equal shapes, equal NaN masks, equal bits wherever `want` is not NaN"""
    got, want = np.ascontiguousarray(got, dtype=np.float64), np.ascontiguousarray(want, dtype=np.float64)
    if got.shape != want.shape or not np.array_equal(np.isnan(got), np.isnan(want)):
        return False
    on = ~np.isnan(want)
    return bool(np.array_equal(got.view(np.uint64)[on], want.view(np.uint64)[on]))


def same_image(img, want):
    want_map, want_origin, want_min, want_max = want
    return same_bits(img["map"], want_map) and same_bits(img["origin"], want_origin) and \
        same_bits([img["min_depth"], img["max_depth"]], [want_min, want_max])


@functools.lru_cache(maxsize=None)
def reference(i):
    """The restatement for camera_i of the scene, computed once: polygons, camera points, the other cameras' buffers, flags,
    statistics, the depth images of SCALES and the number of polygons they draw."""
    s = mx.scene()
    polys = mx.polygons(i)
    idx, xy = ref_mesh.camera_points(s.surface, i)
    keep, stats = ref_mesh.cull(s.surface, i, polys)
    in_range = ref_mesh.selected(s.surface, i, need_seen=False)[0]
    return {"polygons": polys, "index": idx, "xy": xy, "keep": keep, "stats": stats,
            "buffers": {j: ref_mesh.depth_buffer(s.surface, j) for j in range(3) if j != i},
            "images": {scale: ref_mesh.depth_image(s.surface, i, scale, polys) for scale in SCALES},
            "drawn": int(in_range[polys.astype(np.int64)].all(axis=1).sum())}


@functools.lru_cache(maxsize=None)
def device_scene():
    return mx.device(mx.scene())


@pytest.mark.parametrize("i", range(3))
def test_scene_matches_restatement_bit_for_bit(gpu_device, i):
    """Camera points, both other cameras' buffers, flags, statistics and the depth images of camera_i, under every
    threshold of the wave path."""
    s, dev, want = mx.scene(), device_scene(), reference(i)
    polys = want["polygons"]
    try:
        for name, thr in THRESHOLDS:
            mesh.set_wide_threshold(gpu_device, thr)
            idx, xy = mesh.camera_points(gpu_device, dev, s.image_dims, i)
            assert np.array_equal(idx, want["index"]) and xy.shape == want["xy"].shape and xy.tobytes() == want["xy"].tobytes(), name
            for j, want_buf in want["buffers"].items():
                buf = mesh.depth_buffer(gpu_device, dev, s.image_dims, j)
                assert same_bits(buf, want_buf), (name, j)
            keep, stats = mesh.cull(gpu_device, dev, s.image_dims, i, polys)
            assert np.array_equal(keep, want["keep"]), (name, np.nonzero(keep != want["keep"])[0][:20], polys[keep != want["keep"]][:20])
            for j in range(3):
                got = (stats[j]["width"], stats[j]["height"], stats[j]["occupied"], stats[j]["dropped"])
                assert got == want["stats"][j], (name, j, got, want["stats"][j])
                if j != i:
                    assert name == "default" or stats[j]["wide"] == (len(polys) if name == "all" else 0)
                    assert name != "default" or 0 < stats[j]["wide"] < len(polys)
            for scale in SCALES:
                img = mesh.depth_image(gpu_device, dev, s.image_dims, i, scale, polys)
                assert same_image(img, want["images"][scale]), (name, scale)
                assert name == "default" or img["wide"] == (want["drawn"] if name == "all" else 0)
    finally:
        mesh.set_wide_threshold(gpu_device, mesh.WIDE_THRESHOLD_DEFAULT)


def test_wave_walk_reaches_the_third_column_step_and_the_last_row(gpu_device):
    """Camera 0's buffer is 181 cells wide.  A long thin polygon whose only obstructing cell, (150, 60), lies in the third
    64-lane step of its last emitted row, a small one whose only obstructing cell lies in its last emitted row, and beside
    each a twin one row up that obstructs nothing (mesh_exact_scenes.wave_case)."""
    s = mx.wave_case()
    buf = ref_mesh.depth_buffer(s.surface, 0)
    assert buf.shape == (109, 181) and all(buf[y, x] == 1.5 for x, y in s.cells)
    assert ref_mesh.obstructs(s.surface, 0, s.polygons).tolist() == [True, False, True, False]
    assert not ref_mesh.obstructs(s.surface, 2, s.polygons).any()
    # (150, 60) is the only cell under the long polygon's pixels that holds anything, and it is met in the row's third step
    x, y = s.surface.project(0)
    pts = ref_mesh.polygon_points(s.surface, 0, s.polygons[:1].astype(np.int64), x, y, s.surface.depth(0))
    hits = [(int(a), int(b)) for _, xs, ys, _ in ref_mesh.walk(pts, 181, 109) for a, b in zip(xs, ys) if not np.isnan(buf[b, a])]
    row = [int(a) for _, xs, ys, _ in ref_mesh.walk(pts, 181, 109) for a, b in zip(xs, ys) if b == 60]
    assert hits == [(150, 60)] and (150 - min(row)) // 64 == 2
    want, want_stats = ref_mesh.cull(s.surface, 1, s.polygons)
    assert want.tolist() == [False, True, False, True]
    dev = mx.device(s)
    try:
        for name, thr in THRESHOLDS:
            mesh.set_wide_threshold(gpu_device, thr)
            keep, stats = mesh.cull(gpu_device, dev, s.image_dims, 1, s.polygons)
            assert keep.tolist() == want.tolist(), name
            assert [(stats[j]["width"], stats[j]["height"], stats[j]["occupied"], stats[j]["dropped"]) for j in range(3)] == want_stats, name
            assert stats[0]["wide"] == {"all": 4, "none": 0, "default": 2}[name], name  # (the long pair: 16 rows x 171 columns)
            assert same_bits(mesh.depth_buffer(gpu_device, dev, s.image_dims, 0), buf), name
    finally:
        mesh.set_wide_threshold(gpu_device, mesh.WIDE_THRESHOLD_DEFAULT)


def capped_camera_points(device, surface, image_dims, camera, cap):
    args, _keep = mesh._surface_args(surface, image_dims)
    idx, xy, n = np.full(cap, 0xFFFFFFFF, dtype=np.uint32), np.full((cap, 2), -7.0), C.c_uint64(0)
    _lib.check(_lib.lib().cvhip_mesh_camera_points(device.handle, *args, camera, C.c_void_p(idx.ctypes.data), C.c_void_p(xy.ctypes.data),
                                                   cap, C.byref(n)), "cvhip_mesh_camera_points")
    return idx, xy, n.value


@pytest.mark.parametrize("n", [1, 255, 256, 257, mesh.GRID_LANES + 777])
def test_sizes_match_restatement_bit_for_bit(gpu_device, n):
    """One track, one block of the select pair less one, exactly one, one more, and more tracks than one grid-stride launch
    has lanes (a second iteration of the projection's loop, every partial extent folded, more than 1024 select blocks with
    a ragged last one, a sparse selection): camera points - all, and the first half -, the buffer and the splat-only depth
    image of every camera."""
    s = mx.sized(n)
    dev = mx.device(s)
    for j in range(3):
        want_idx, want_xy = ref_mesh.camera_points(s.surface, j)
        idx, xy = mesh.camera_points(gpu_device, dev, s.image_dims, j)
        assert np.array_equal(idx, want_idx) and xy.shape == want_xy.shape and xy.tobytes() == want_xy.tobytes(), j
        assert len(idx) == n if n < 1000 else (len(idx) > 2000 and idx[0] == 0 and idx[-1] == n - 1)
        cap = len(want_idx) // 2
        if cap:
            idx, xy, count = capped_camera_points(gpu_device, dev, s.image_dims, j, cap)
            assert count == len(want_idx) and np.array_equal(idx, want_idx[:cap]) and xy.tobytes() == want_xy[:cap].tobytes(), j
        assert same_bits(mesh.depth_buffer(gpu_device, dev, s.image_dims, j), ref_mesh.depth_buffer(s.surface, j)), j
        img = mesh.depth_image(gpu_device, dev, s.image_dims, j, -1.0, NO_POLYGONS)
        assert same_image(img, ref_mesh.depth_image(s.surface, j, -1.0, NO_POLYGONS)), j
        if n == 1:  # (integer projections in camera 1: a 1 x 1 map, clamped into with width - 1 = 0)
            assert img["map"].shape == ((1, 1) if j == 1 else (2, 2)) and img["min_depth"] == img["max_depth"] == np.nanmax(img["map"])


def test_no_tracks(gpu_device):
    s = mx.sized(0)
    dev = mx.device(s)
    for j in range(3):
        idx, xy = mesh.camera_points(gpu_device, dev, s.image_dims, j)
        assert len(idx) == 0 and xy.shape == (0, 2)
        assert mesh.depth_buffer(gpu_device, dev, s.image_dims, j).shape == (0, 0)
        with pytest.raises(_lib.CvhipError, match="No point projections found") as exc:
            mesh.depth_image(gpu_device, dev, s.image_dims, j, -1.0, NO_POLYGONS)
        assert exc.value.code == -6
        with pytest.raises(_lib.CvhipError) as exc:
            mesh.cull(gpu_device, dev, s.image_dims, j, np.zeros((1, 3), dtype=np.uint32))
        assert exc.value.code == -1  # CVHIP_ERR_INVALID: the polygon names a track >= n


@pytest.mark.parametrize("i", range(3))
def test_edge_scene_with_its_own_dims_per_camera_bit_for_bit(gpu_device, i):
    """mesh_exact_scenes.edge_scene: exact cameras with images of 320 x 200, 200 x 320 and 240 x 320 and tracks exactly on
    and a quarter below both ends of every camera's img_range on each axis.  Camera points, the other cameras' buffers
    (each as wide and high as its own range), flags, statistics and the depth image, bit for bit, under every threshold of
    the wave path.  Width for height in img_range, or another camera's dims, selects other tracks in every camera
    (tests/test_mesh_exact_ref.py)."""
    s = mx.edge_scene()
    dev = mx.device(s)
    polys = mx.edge_polygons(i)
    want_idx, want_xy = ref_mesh.camera_points(s.surface, i)
    want_keep, want_stats = ref_mesh.cull(s.surface, i, polys)
    want_images = {scale: ref_mesh.depth_image(s.surface, i, scale, polys) for scale in SCALES}
    try:
        for name, thr in THRESHOLDS:
            mesh.set_wide_threshold(gpu_device, thr)
            idx, xy = mesh.camera_points(gpu_device, dev, s.image_dims, i)
            assert np.array_equal(idx, want_idx) and xy.shape == want_xy.shape and xy.tobytes() == want_xy.tobytes(), name
            for j in range(3):
                if j != i:
                    assert same_bits(mesh.depth_buffer(gpu_device, dev, s.image_dims, j), ref_mesh.depth_buffer(s.surface, j)), (name, j)
            keep, stats = mesh.cull(gpu_device, dev, s.image_dims, i, polys)
            assert np.array_equal(keep, want_keep), (name, np.nonzero(keep != want_keep)[0])
            for j in range(3):
                got = (stats[j]["width"], stats[j]["height"], stats[j]["occupied"], stats[j]["dropped"])
                assert got == want_stats[j], (name, j, got, want_stats[j])
            for scale in SCALES:
                img = mesh.depth_image(gpu_device, dev, s.image_dims, i, scale, polys)
                assert same_image(img, want_images[scale]), (name, scale)
    finally:
        mesh.set_wide_threshold(gpu_device, mesh.WIDE_THRESHOLD_DEFAULT)
