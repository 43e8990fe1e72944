"""The mesh stage on the device (cvhip_mesh_*, csrc/mesh_kernels.hip) against the numpy restatement
(tests/ref_mesh.py): camera points, depth buffers, culling flags and the depth image on tests/mesh_scenes.py's scenes for
2, 3, 4 and 8 cameras, both walk paths, the NaN / infinity cases, more polygons than one launch's lanes, the merge, the
errors, and the new reconstruction function end to end.

Geometry (projections, rows, columns, x_c) is the same IEEE operations on both sides: pixels, masks and flags are EQUAL.
Depths go through sin / cos of the device's library: 1e-9 relative, the project's bound for f64 stages; near_threshold
lists what could hang on that and is empty for the scenes' seeds (test_mesh_ref.py checks the same on the CPU)."""
import ctypes as C
import functools

import numpy as np
import pytest

import mesh_scenes
import ref_mesh
from cybervision_amd import _lib, mesh, reconstruction, synth, triangulation

pytestmark = pytest.mark.gpu
RTOL = 1e-9
CASES = [(m, i) for m in (2, 3, 4, 8) for i in range(m)]


@functools.lru_cache(maxsize=None)
def scene(m):
    s = mesh_scenes.scene(m)
    s.device = mesh_scenes.device_surface(s)
    return s


@functools.lru_cache(maxsize=None)
def reference(m, i):
    """The restatement for camera_i of scene(m), computed once: polygons, near, keep, stats, the depth image."""
    s = scene(m)
    polys = mesh_scenes.polygons(s, i)
    near = ref_mesh.Near()
    ref_mesh.camera_points(s.surface, i, near=near)
    keep, stats = ref_mesh.cull(s.surface, i, polys, near=near)
    image = ref_mesh.depth_image(s.surface, i, -1.0, polys, near=near)
    return polys, near, keep, stats, image


@functools.lru_cache(maxsize=None)
def reference_buffer(m, j):
    return ref_mesh.depth_buffer(scene(m).surface, j)


def close(a, b):
    """equal masks, values within RTOL relative"""
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and np.array_equal(np.isnan(a), np.isnan(b)) and \
        bool(np.all(np.abs(a - b)[~np.isnan(b)] <= RTOL * np.abs(b)[~np.isnan(b)]))


def same_bytes(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.tobytes() == b.tobytes()


@pytest.mark.parametrize("m,i", CASES)
def test_cull_and_depth_image_match_restatement(gpu_device, m, i):
    s = scene(m)
    polys, near, want_keep, want_stats, want_image = reference(m, i)
    assert near.empty(), (near.polygons, near.cells, near.tracks)
    # camera points: the same tracks in track order, the same projections
    want_idx, want_xy = ref_mesh.camera_points(s.surface, i)
    idx, xy = mesh.camera_points(gpu_device, s.device, s.image_dims, i)
    assert np.array_equal(idx, want_idx) and same_bytes(xy, want_xy) and len(idx) > 1000
    # one other camera's buffer per case (every camera's over the cases of a scene): dimensions, mask, depths
    j = (i + 1) % m
    buf = mesh.depth_buffer(gpu_device, s.device, s.image_dims, j)
    assert close(buf, reference_buffer(m, j))
    # flags and statistics
    keep, stats = mesh.cull(gpu_device, s.device, s.image_dims, i, polys)
    assert np.array_equal(keep, want_keep)
    for k in range(m):
        got = (stats[k]["width"], stats[k]["height"], stats[k]["occupied"], stats[k]["dropped"])
        assert got == want_stats[k], (k, got, want_stats[k])
        if k != i:
            assert 0.05 * len(polys) <= stats[k]["dropped"] <= 0.95 * len(polys)
            assert 0 < stats[k]["wide"] < len(polys)  # the long triangles take the wave path, the lattice's do not
    assert stats[i] == dict.fromkeys(mesh.STATS, 0)
    # the depth image of the same polygons
    img = mesh.depth_image(gpu_device, s.device, s.image_dims, i, -1.0, polys)
    want_map, want_origin, want_min, want_max = want_image
    assert img["origin"] == want_origin and close(img["map"], want_map)
    assert abs(img["min_depth"] - want_min) <= RTOL * abs(want_min) and abs(img["max_depth"] - want_max) <= RTOL * abs(want_max)
    assert 0 < img["wide"] < len(polys)


def test_both_paths_give_the_same_flags_and_maps(gpu_device):
    """Thresholds 0 (every polygon through the wave path), UINT32_MAX (none) and the default: identical flags and maps; the
    default sends polygons down both paths (out_stats)."""
    m, i = 3, 0
    s = scene(m)
    polys, _, want_keep, _, _ = reference(m, i)
    runs = {}
    try:
        for name, thr in (("all", mesh.WIDE_ALL), ("none", mesh.WIDE_NONE), ("default", mesh.WIDE_THRESHOLD_DEFAULT)):
            mesh.set_wide_threshold(gpu_device, thr)
            keep, stats = mesh.cull(gpu_device, s.device, s.image_dims, i, polys)
            img = mesh.depth_image(gpu_device, s.device, s.image_dims, i, -1.0, polys)
            runs[name] = (keep, stats, img)
    finally:
        mesh.set_wide_threshold(gpu_device, mesh.WIDE_THRESHOLD_DEFAULT)
    for name in ("all", "none"):
        assert np.array_equal(runs[name][0], runs["default"][0]) and same_bytes(runs[name][2]["map"], runs["default"][2]["map"])
        for k in (1, 2):
            assert {q: runs[name][1][k][q] for q in ("width", "height", "occupied", "dropped")} == \
                   {q: runs["default"][1][k][q] for q in ("width", "height", "occupied", "dropped")}
    assert np.array_equal(runs["default"][0], want_keep)
    for k in (1, 2):
        assert runs["all"][1][k]["wide"] == len(polys) and runs["none"][1][k]["wide"] == 0
        assert 1 <= runs["default"][1][k]["wide"] < len(polys)
    assert runs["all"][2]["wide"] == len(polys) and runs["none"][2]["wide"] == 0 and 1 <= runs["default"][2]["wide"] < len(polys)


def test_exact_cases(gpu_device):
    """Repeated vertices ([v, v, w], [v, w, w], [v, v, v]: the walk runs on NaN and infinity and emits nothing), a polygon
    entirely outside the buffer, and a camera in which no track is visible (a 0 x 0 buffer): the restatement's flags, under
    every threshold."""
    m, i, j = 3, 0, 1
    s = scene(m)
    polys, _, _, _, _ = reference(m, i)
    x, _ = s.surface.project(j)
    w = reference_buffer(m, j).shape[1]
    tri = s.triangles
    out = tri[(x[tri].max(axis=1) < -1.0) | (x[tri].min(axis=1) > w + 1.0)]
    assert len(out) > 0
    v, u = int(polys[10, 0]), int(polys[500, 1])
    special = np.array([[v, v, u], [v, u, u], [v, v, v], [u, u, v], out[0], out[-1]], dtype=np.uint32)
    cases = np.concatenate([special, polys[:200]])
    want, _ = ref_mesh.cull(s.surface, i, cases)
    assert want[:6].all() and not want[6:].all()
    try:
        for thr in (mesh.WIDE_ALL, mesh.WIDE_NONE, mesh.WIDE_THRESHOLD_DEFAULT):
            mesh.set_wide_threshold(gpu_device, thr)
            keep, _ = mesh.cull(gpu_device, s.device, s.image_dims, i, cases)
            assert np.array_equal(keep, want), thr
            got = mesh.depth_image(gpu_device, s.device, s.image_dims, i, -1.0, special)["map"]
            assert close(got, ref_mesh.depth_image(s.surface, i, -1.0, special)[0])
    finally:
        mesh.set_wide_threshold(gpu_device, mesh.WIDE_THRESHOLD_DEFAULT)
    # no track visible in cameras 1 and 2: 0 x 0 buffers, nothing obstructs
    blind = triangulation.Surface(points=s.device.points, track_index=s.device.track_index, tracks=s.device.tracks.copy(),
                                  cameras=s.device.cameras)
    blind.tracks[:, 1:] = -1
    keep, stats = mesh.cull(gpu_device, blind, s.image_dims, i, polys)
    assert keep.all() and all(stats[k] == dict.fromkeys(mesh.STATS, 0) for k in range(m))
    assert mesh.depth_buffer(gpu_device, blind, s.image_dims, 1).shape == (0, 0)
    assert len(mesh.camera_points(gpu_device, blind, s.image_dims, 1)[0]) == 0


def test_more_polygons_than_one_launch(gpu_device):
    """The polygon list tiled past mesh.GRID_LANES (the lanes of one grid-stride launch, CVHIP_MESH_GRID_LANES): the flags are
    the small result tiled, the depth image is the untiled one bit for bit (the maximum is idempotent)."""
    m, i = 3, 0
    s = scene(m)
    polys, _, want_keep, _, _ = reference(m, i)
    reps = mesh.GRID_LANES // len(polys) + 2
    big = np.tile(polys, (reps, 1))
    assert len(big) > mesh.GRID_LANES + len(polys)
    keep, stats = mesh.cull(gpu_device, s.device, s.image_dims, i, big)
    assert np.array_equal(keep, np.tile(want_keep, reps))
    small_keep, small_stats = mesh.cull(gpu_device, s.device, s.image_dims, i, polys)
    assert all(stats[k]["dropped"] == reps * small_stats[k]["dropped"] and stats[k]["wide"] == reps * small_stats[k]["wide"] for k in range(m))
    a = mesh.depth_image(gpu_device, s.device, s.image_dims, i, -1.0, big)
    b = mesh.depth_image(gpu_device, s.device, s.image_dims, i, -1.0, polys)
    assert same_bytes(a["map"], b["map"]) and a["wide"] == reps * b["wide"]


def test_deterministic_and_device_pointers(gpu_device):
    """Two runs give the same bytes for flags, buffers and maps; points, tracks, polygons and the outputs in device memory
    give the same bytes as in host memory."""
    import torch

    m, i = 4, 2
    s = scene(m)
    polys = reference(m, i)[0]
    runs = []
    for _ in range(2):
        keep, stats = mesh.cull(gpu_device, s.device, s.image_dims, i, polys)
        runs.append((keep, stats, mesh.depth_buffer(gpu_device, s.device, s.image_dims, 0),
                     mesh.depth_image(gpu_device, s.device, s.image_dims, i, 1.0, polys)["map"]))
    assert same_bytes(runs[0][0], runs[1][0]) and runs[0][1] == runs[1][1]
    assert same_bytes(runs[0][2], runs[1][2]) and same_bytes(runs[0][3], runs[1][3])
    args, _keep = mesh._surface_args(s.device, s.image_dims)
    d_pts, d_tracks, d_poly = (torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (s.device.points, s.device.tracks, polys.view(np.int32)))
    d_keep = torch.full((len(polys),), 7, dtype=torch.uint8, device="cuda")
    h, w = runs[0][3].shape
    d_map = torch.zeros((h, w), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()  # (the tensors are filled on torch's stream, the library works on its own)
    dargs = [C.c_void_p(d_pts.data_ptr()), C.c_void_p(d_tracks.data_ptr())] + args[2:]
    stats = np.zeros((m, 5), dtype=np.uint64)
    L = _lib.lib()
    _lib.check(L.cvhip_mesh_cull(gpu_device.handle, *dargs, i, C.c_void_p(d_poly.data_ptr()), len(polys), C.c_void_p(d_keep.data_ptr()),
                                 C.c_void_p(stats.ctypes.data)), "cvhip_mesh_cull")
    cw, ch = C.c_uint64(0), C.c_uint64(0)
    _lib.check(L.cvhip_mesh_depth_image(gpu_device.handle, *dargs, i, 1.0, C.c_void_p(d_poly.data_ptr()), len(polys),
                                        C.c_void_p(d_map.data_ptr()), h * w, C.byref(cw), C.byref(ch), None, None, None),
               "cvhip_mesh_depth_image")
    torch.cuda.synchronize()
    assert np.array_equal(d_keep.cpu().numpy().astype(bool), runs[0][0]) and (cw.value, ch.value) == (w, h)
    assert same_bytes(d_map.cpu().numpy(), runs[0][3])
    assert [int(v) for v in stats[0]] == [runs[0][1][0][q] for q in mesh.STATS]


def test_merge_matches_restatement(gpu_device):
    """Rotation, sort, a triple shared by two cameras (the lowest keeps it), duplicates within a camera, the grouping by
    camera - on a hand-made list and on the scene's kept polygons with camera 1's list seeded with camera 0's."""
    per = [(0, [[5, 2, 9], [9, 5, 2], [7, 8, 3]]), (1, [[2, 9, 5], [1, 4, 6], [2, 5, 9]]), (2, [[6, 1, 4], [0, 1, 2]])]
    polys, cams = mesh.merge(gpu_device, np.concatenate([np.array(p) for _, p in per]), np.concatenate([[c] * len(p) for c, p in per]))
    want_p, want_c = ref_mesh.merge(per)
    assert np.array_equal(polys, want_p) and np.array_equal(cams, want_c)
    assert polys.tolist() == [[2, 9, 5], [3, 7, 8], [1, 4, 6], [2, 5, 9], [0, 1, 2]] and cams.tolist() == [0, 0, 1, 1, 2]
    m = 3
    kept = []
    for i in range(m):
        p, _, keep, _, _ = reference(m, i)
        kept.append((i, p[keep]))
    kept[1] = (1, np.concatenate([kept[1][1], np.roll(kept[0][1][:300], 1, axis=1)]))  # camera 0's polygons again, rotated
    polys, cams = mesh.merge(gpu_device, np.concatenate([p for _, p in kept]), np.concatenate([np.full(len(p), c) for c, p in kept]))
    want_p, want_c = ref_mesh.merge(kept)
    assert np.array_equal(polys, want_p) and np.array_equal(cams, want_c)
    assert len(polys) < sum(len(p) for _, p in kept) and (np.diff(cams.astype(np.int64)) >= 0).all()
    empty_p, empty_c = mesh.merge(gpu_device, np.zeros((0, 3)), np.zeros(0))
    assert len(empty_p) == 0 and len(empty_c) == 0


def test_create_matches_restatement(gpu_device):
    """mesh.create with the lattice split as the caller's Delaunay: the merged list and its cameras equal the restatement's."""
    m = 3
    s = scene(m)
    tri = [mesh_scenes.lattice_triangulate(s, i) for i in range(m)]
    calls = iter(tri)
    got = mesh.create(gpu_device, s.device, s.image_dims, lambda xy: next(calls)(xy))
    calls = iter(tri)
    want_p, want_c, per = ref_mesh.create(s.surface, lambda xy: next(calls)(xy))
    assert np.array_equal(got["polygons"], want_p) and np.array_equal(got["camera"], want_c)
    assert [c["kept"] for c in got["per_camera"]] == [int(k.sum()) for _, _, k in per]


def test_errors_and_sizing(gpu_device):
    m, i = 3, 0
    s = scene(m)
    polys = reference(m, i)[0]
    n = len(s.device.points)
    args, _keep = mesh._surface_args(s.device, s.image_dims)
    L = _lib.lib()
    # a vertex out of range: CVHIP_ERR_INVALID, nothing written
    bad = polys.copy()
    bad[len(bad) // 2, 1] = n
    keep = np.full(len(bad), 7, dtype=np.uint8)
    stats = np.full((m, 5), 9, dtype=np.uint64)
    rc = L.cvhip_mesh_cull(gpu_device.handle, *args, i, C.c_void_p(bad.ctypes.data), len(bad), C.c_void_p(keep.ctypes.data),
                           C.c_void_p(stats.ctypes.data))
    assert rc == -1 and (keep == 7).all() and (stats == 9).all() and b"track" in L.cvhip_last_error()
    with pytest.raises(_lib.CvhipError) as exc:
        mesh.depth_image(gpu_device, s.device, s.image_dims, i, -1.0, bad)
    assert exc.value.code == -1
    # more cameras than CVHIP_TRIANGULATE_MAX_CAMERAS, none at all, a camera index past m
    cam = s.device.cameras[0]
    many = triangulation.Surface(points=s.device.points, track_index=s.device.track_index,
                                 tracks=np.full((n, 9, 2), -1, dtype=np.int32), cameras=[cam] * 9)
    for call in (lambda: mesh.cull(gpu_device, many, [(320, 320)] * 9, 0, polys), lambda: mesh.camera_points(gpu_device, many, [(320, 320)] * 9, 0),
                 lambda: mesh.depth_image(gpu_device, many, [(320, 320)] * 9, 0, 1.0, polys)):
        with pytest.raises(_lib.CvhipError) as exc:
            call()
        assert exc.value.code == -3
    none = triangulation.Surface(points=s.device.points, track_index=s.device.track_index,
                                 tracks=np.zeros((n, 0, 2), dtype=np.int32), cameras=[])
    with pytest.raises(_lib.CvhipError) as exc:
        mesh.cull(gpu_device, none, [], 0, polys)
    assert exc.value.code == -1
    with pytest.raises(_lib.CvhipError) as exc:
        mesh.camera_points(gpu_device, s.device, s.image_dims, m)
    assert exc.value.code == -1
    # no projection in range: the reference's message
    far = triangulation.Surface(points=s.device.points + np.array([1e6, 0.0, 0.0]), track_index=s.device.track_index,
                                tracks=s.device.tracks, cameras=s.device.cameras)
    with pytest.raises(_lib.CvhipError, match="No point projections found") as exc:
        mesh.depth_image(gpu_device, far, s.image_dims, 0, -1.0, polys)
    assert exc.value.code == -6
    # cap = 0 sizes the outputs and writes nothing
    cnt = C.c_uint64(0)
    _lib.check(L.cvhip_mesh_camera_points(gpu_device.handle, *args, i, None, None, 0, C.byref(cnt)), "cvhip_mesh_camera_points")
    assert cnt.value == len(ref_mesh.camera_points(s.surface, i)[0])
    w, h = C.c_uint64(0), C.c_uint64(0)
    origin = np.zeros(2)
    _lib.check(L.cvhip_mesh_depth_image(gpu_device.handle, *args, i, -1.0, C.c_void_p(polys.ctypes.data), len(polys), None, 0,
                                        C.byref(w), C.byref(h), C.c_void_p(origin.ctypes.data), None, None), "cvhip_mesh_depth_image")
    want_map, want_origin, _, _ = reference(m, i)[4]
    assert (h.value, w.value) == want_map.shape and tuple(origin) == want_origin
    small = np.zeros(16)
    assert L.cvhip_mesh_depth_image(gpu_device.handle, *args, i, -1.0, C.c_void_p(polys.ctypes.data), len(polys),
                                    C.c_void_p(small.ctypes.data), 16, C.byref(w), C.byref(h), None, None, None) == -1
    assert (small == 0).all()
    # a cap below the count: the first `cap` points
    idx, xy = np.zeros(10, dtype=np.uint32), np.zeros((10, 2))
    _lib.check(L.cvhip_mesh_camera_points(gpu_device.handle, *args, i, C.c_void_p(idx.ctypes.data), C.c_void_p(xy.ctypes.data), 10,
                                          C.byref(cnt)), "cvhip_mesh_camera_points")
    assert np.array_equal(idx, ref_mesh.camera_points(s.surface, i)[0][:10])


def test_reconstruct_perspective_mesh_512(gpu_device):
    """Config 5's scene at 512^2 through reconstruction.reconstruct_perspective_mesh with mesh.delaunay_scipy: camera 0's
    flags and the depth image agree with the restatement run on the surface the device returned, outside what
    near_threshold lists - at most 0.1 % of the polygons (a condition of the scene); the merged list's camera-0 group is
    camera 0's kept polygons."""
    pytest.importorskip("scipy")
    size = 512
    views, K, _ = synth.make_sfm_views(size)
    steps = synth.optimal_scale_steps(size, size)
    pyrs = [synth.box_pyramid(v, steps) for v in views]
    out = reconstruction.reconstruct_perspective_mesh(gpu_device, pyrs, K, project_to_image=0, bundle_adjustment=False, seed=3)
    surface, shapes = out["surface"], out["mesh_image_shapes"]
    assert len(surface.cameras) == 3 and len(surface.points) > 20000
    ref = ref_mesh.Surface.from_device(surface, shapes)
    idx, xy = mesh.camera_points(gpu_device, surface, shapes, 0)
    want_idx, want_xy = ref_mesh.camera_points(ref, 0)
    assert np.array_equal(idx, want_idx) and same_bytes(xy, want_xy)
    polys = idx[mesh.delaunay_scipy(xy)]
    keep, stats = mesh.cull(gpu_device, surface, shapes, 0, polys)
    near = ref_mesh.Near()
    want_keep, want_stats = ref_mesh.cull(ref, 0, polys, near=near)
    listed = np.zeros(len(polys), dtype=bool)
    listed[sorted(near.polygons)] = True
    print(f"mesh 512: {len(surface.points)} tracks, {len(polys)} polygons of camera 0, kept {int(keep.sum())}, "
          f"near_threshold lists {int(listed.sum())} polygons, {len(near.cells)} cells, {len(near.tracks)} tracks; stats {stats}")
    assert listed.mean() <= 0.001
    assert np.array_equal(keep[~listed], want_keep[~listed])
    assert 0 < keep.sum() < len(keep)
    for k in (1, 2):
        assert (stats[k]["width"], stats[k]["height"], stats[k]["occupied"]) == want_stats[k][:3]
    # the merged list: camera 0's group is its kept polygons, rotated and sorted
    got0 = out["mesh"]["polygons"][out["mesh"]["camera"] == 0]
    want0 = np.array(sorted({ref_mesh.rotate(p) for p in polys[keep].tolist()}), dtype=np.uint32).reshape(-1, 3)
    assert np.array_equal(got0, want0)
    assert out["mesh"]["per_camera"][0]["polygons"] == len(polys) and set(out["mesh"]["camera"].tolist()) == {0, 1, 2}
    # the depth image of the merged list
    img = out["depth_image"]
    near_img = ref_mesh.Near()
    want_map, want_origin, want_min, want_max = ref_mesh.depth_image(ref, 0, -1.0, out["mesh"]["polygons"], near=near_img)
    assert img["origin"] == want_origin and img["map"].shape == want_map.shape
    assert len(near_img.polygons) <= 0.001 * len(out["mesh"]["polygons"])
    skip = np.zeros(want_map.shape, dtype=bool)
    if near_img.polygons or near_img.tracks:  # the cells that a listed polygon or track can reach
        listed_p = out["mesh"]["polygons"][sorted(near_img.polygons)]
        sub = ref_mesh.depth_image(ref, 0, -1.0, listed_p)[0]
        none = ref_mesh.depth_image(ref, 0, -1.0, np.zeros((0, 3), dtype=np.uint32))[0]
        skip = ~(np.isnan(sub) & np.isnan(none)) & ~((sub == none) | (np.isnan(sub) & np.isnan(none)))
        assert not near_img.tracks
    got, want = np.where(skip, np.nan, img["map"]), np.where(skip, np.nan, want_map)
    assert close(got, want) and skip.mean() <= 0.001
    assert abs(img["min_depth"] - want_min) <= RTOL * abs(want_min) and abs(img["max_depth"] - want_max) <= RTOL * abs(want_max)


# ---- a K and an image size per camera (mesh_scenes.scene(m, mixed=True)) ---------------------------------------------------
MIXED_CASES = [(3, 0), (3, 1), (3, 2), (8, 5), (8, 6)]  # every camera of the 3-camera scene; 250 x 141 and 141 x 250 of the 8


@functools.lru_cache(maxsize=None)
def mixed_scene(m):
    s = mesh_scenes.scene(m, mixed=True)
    s.device = mesh_scenes.device_surface(s)
    return s


@pytest.mark.parametrize("m,i", MIXED_CASES)
def test_mixed_dims_match_restatement_on_both_paths(gpu_device, m, i):
    """test_cull_and_depth_image_match_restatement's comparisons - camera points, depth buffers, flags, statistics and the
    depth image: flags, masks and pixels equal, depths to 1e-9 - on scenes whose cameras each have their own K and their
    own (width, height), landscape and portrait, no two alike; with every polygon through the wave path, none, and the
    default threshold, as test_both_paths_give_the_same_flags_and_maps runs them.  near_threshold is empty for these
    cameras (tests/test_mesh_ref.py)."""
    s = mixed_scene(m)
    assert len(set(s.image_dims)) == m
    polys = mesh_scenes.polygons(s, i)
    near = ref_mesh.Near()
    want_idx, want_xy = ref_mesh.camera_points(s.surface, i, near=near)
    want_keep, want_stats = ref_mesh.cull(s.surface, i, polys, near=near)
    want_map, want_origin, want_min, want_max = ref_mesh.depth_image(s.surface, i, -1.0, polys, near=near)
    assert near.empty(), (near.polygons, near.cells, near.tracks)
    idx, xy = mesh.camera_points(gpu_device, s.device, s.image_dims, i)
    assert np.array_equal(idx, want_idx) and same_bytes(xy, want_xy) and len(idx) > 1000
    for j in ((i + 1) % m, (i + 2) % m):
        assert close(mesh.depth_buffer(gpu_device, s.device, s.image_dims, j), ref_mesh.depth_buffer(s.surface, j)), j
    try:
        for name, thr in (("all", mesh.WIDE_ALL), ("none", mesh.WIDE_NONE), ("default", mesh.WIDE_THRESHOLD_DEFAULT)):
            mesh.set_wide_threshold(gpu_device, thr)
            keep, stats = mesh.cull(gpu_device, s.device, s.image_dims, i, polys)
            assert np.array_equal(keep, want_keep), name
            for k in range(m):
                got = (stats[k]["width"], stats[k]["height"], stats[k]["occupied"], stats[k]["dropped"])
                assert got == want_stats[k], (name, k, got, want_stats[k])
                if k != i:
                    assert 0.05 * len(polys) <= stats[k]["dropped"] <= 0.95 * len(polys)
                    assert stats[k]["wide"] == {"all": len(polys), "none": 0}.get(name, stats[k]["wide"])
                    assert name != "default" or 0 < stats[k]["wide"] < len(polys)
            assert stats[i] == dict.fromkeys(mesh.STATS, 0)
            img = mesh.depth_image(gpu_device, s.device, s.image_dims, i, -1.0, polys)
            assert img["origin"] == want_origin and close(img["map"], want_map), name
            assert abs(img["min_depth"] - want_min) <= RTOL * abs(want_min) and abs(img["max_depth"] - want_max) <= RTOL * abs(want_max)
            assert img["wide"] == {"all": len(polys), "none": 0}.get(name, img["wide"])
            assert name != "default" or 0 < img["wide"] < len(polys)
    finally:
        mesh.set_wide_threshold(gpu_device, mesh.WIDE_THRESHOLD_DEFAULT)
