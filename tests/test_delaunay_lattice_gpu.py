"""The lattice path of cvhip_mesh_delaunay (LatticePolicy, exact integer predicates on the device for integer
coordinates within 2^24) on a real GPU: the faces are THE defined result (tests/ref_delaunay.py), the same bytes as the host
path gives, nearly every star stays on the device; and the affine surface through the mesh stage and reconstruct_affine_mesh.
The switch is off by default (the stats of a lattice input stay what they were); every test here sets it."""
import functools

import numpy as np
import pytest

import cases
import lattice_sets
import mesh_scenes
import ref_delaunay as rd
import ref_mesh
import ref_obj
import ref_ply
from cybervision_amd import correlation, mesh, reconstruction, triangulation

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def default_switches(gpu_device):
    yield
    mesh.set_delaunay_lattice(gpu_device, mesh.DELAUNAY_LATTICE_DEFAULT)
    mesh.set_delaunay_lane_cells(gpu_device, mesh.DELAUNAY_LANE_CELLS_DEFAULT)


def run(device, xy, lattice):
    """-> (faces, stats, lattice_stars) of one call with the switch at `lattice`"""
    mesh.set_delaunay_lattice(device, lattice)
    assert mesh.delaunay_lattice(device) is bool(lattice)
    stats = {}
    f = mesh.delaunay(device, xy, stats)
    return f, stats, mesh.delaunay_lattice_stars(device)


def defined(xy, faces):
    P = rd.Points(xy)
    f = np.asarray(faces, dtype=np.int64)
    assert rd.check(P, f) == []
    assert rd.as_set(rd.canonical(P, f)) == rd.as_set(f) and len(rd.as_set(f)) == len(f)
    return P


def test_default_is_off(gpu_device):
    """a fresh setting leaves a lattice where it was: every star meets a tie and goes to the host"""
    assert mesh.DELAUNAY_LATTICE_DEFAULT is False and mesh.delaunay_lattice(gpu_device) is False
    xy = rd.lattice()
    stats = {}
    mesh.delaunay(gpu_device, xy, stats)
    assert stats["host_stars"] == len(xy) and mesh.delaunay_lattice_stars(gpu_device) == 0


DEFINED = dict(lattice_sets.SETS, full_64=lambda: rd.lattice(64, 64), holes_64=lambda: lattice_sets.holes(64, 64, 64),
               k255=lambda: rd.lattice(17, 15), k256=lambda: rd.lattice(16, 16), k257=lambda: np.concatenate([rd.lattice(16, 16), [[16.0, 3.0]]]))
del DEFINED["holes_96"]  # (below, against the host path)


@pytest.mark.parametrize("name", sorted(DEFINED))
def test_defined_result(gpu_device, name):
    xy = DEFINED[name]()
    if name.startswith("k"):
        assert len(xy) == int(name[1:])
    f, stats, lattice_stars = run(gpu_device, xy, True)
    P = defined(xy, f)
    if len(xy) <= 40:
        assert rd.as_set(f) == rd.as_set(rd.brute(P))
    print(f"{name}: {len(xy)} points, {len(f)} faces, stats {stats}, lattice stars {lattice_stars}")
    assert stats["device_stars"] == lattice_stars and lattice_stars + stats["host_stars"] == len(xy) and stats["duplicates"] == 0
    assert stats["host_stars"] <= len(xy) // 10  # (only lane_cells can send a star away here: a few hull stars)


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_circle50_permutations(gpu_device, seed):
    xy = rd.circle50(seed)
    f, stats, lattice_stars = run(gpu_device, xy, True)
    assert rd.as_set(f) == rd.as_set(rd.brute(xy)) and len(rd.as_set(f)) == len(f)
    assert lattice_stars == len(xy) and stats["host_stars"] == 0


def beyond():
    xy = lattice_sets.holes(30, 20, 30)
    xy[7, 0] = lattice_sets.LIMIT + 1.0
    return xy


def half():
    xy = lattice_sets.holes(30, 20, 31)
    xy[11, 1] += 0.5
    return xy


SAME = {"holes_96": (lambda: lattice_sets.holes(96, 96, 96), True), "strip_3x2000": (lambda: rd.lattice(3, 2000), True),
        "transposed_strip": (lambda: rd.lattice(2000, 3), True), "duplicates": (lambda: lattice_sets.with_duplicates()[0], True),
        "beyond_2^24": (beyond, False), "half": (half, False)}


@pytest.mark.parametrize("name", sorted(SAME))
def test_same_bytes_as_the_host_path(gpu_device, name):
    make, qualifies = SAME[name]
    xy = make()
    on, st_on, lattice_stars = run(gpu_device, xy, True)
    off, st_off, off_stars = run(gpu_device, xy, False)
    print(f"{name}: {len(xy)} points, {len(on)} faces, on {st_on} ({lattice_stars} lattice stars), off {st_off}")
    assert len(on) > len(xy) and on.tobytes() == off.tobytes()
    assert off_stars == 0 and st_on["duplicates"] == st_off["duplicates"]
    assert st_on["device_stars"] + st_on["host_stars"] == len(xy) == st_off["device_stars"] + st_off["host_stars"]
    if qualifies:
        assert lattice_stars == st_on["device_stars"] > 0 and st_on["host_stars"] < st_off["host_stars"]
    else:
        assert lattice_stars == 0 and st_on == st_off
    if name == "duplicates":
        assert st_on["duplicates"] == lattice_sets.with_duplicates()[1]
        defined(xy, on)


def test_non_integer_input_is_untouched(gpu_device):
    xy = ref_mesh.camera_points(mesh_scenes.scene(2).surface, 0)[1]
    on, st_on, lattice_stars = run(gpu_device, xy, True)
    off, st_off, _ = run(gpu_device, xy, False)
    assert len(on) > len(xy) and on.tobytes() == off.tobytes()
    assert lattice_stars == 0 and set(st_on) == set(mesh.DELAUNAY_STATS)
    assert st_on == st_off, (st_on, st_off)
    assert st_on["device_stars"] + st_on["host_stars"] == len(xy) and st_on["device_stars"] > st_on["host_stars"]


def test_coverage(gpu_device):
    """256 x 256 with 10 % holes: with the lattice kernels only the stars past lane_cells leave the device (tests/cpp/delaunay_lattice_exact.cpp
    counts them, `over`: 26 of 59 003 for this seed); without them every star does"""
    xy = lattice_sets.holes(256, 256, 256)
    k = len(xy)
    on, st_on, lattice_stars = run(gpu_device, xy, True)
    print(f"coverage: {k} points, on {st_on}, lattice stars {lattice_stars}")
    assert st_on["host_stars"] * 100 <= k and lattice_stars + st_on["host_stars"] == k
    off, st_off, off_stars = run(gpu_device, xy, False)
    assert st_off["host_stars"] == k and off_stars == 0 and on.tobytes() == off.tobytes()


def test_past_one_launch(gpu_device):
    """513 x 513 lattice points: more than CVHIP_MESH_GRID_LANES"""
    xy = rd.lattice(513, 513)
    k = len(xy)
    assert k == 263169 > mesh.GRID_LANES
    a, st, lattice_stars = run(gpu_device, xy, True)
    b, _, _ = run(gpu_device, xy, True)
    print(f"513 x 513: {len(a)} faces, stats {st}, lattice stars {lattice_stars}")
    assert len(a) == 2 * k - 2 - 4 * 512  # (every lattice point of the boundary is a hull vertex of the triangulation: h = 2048)
    assert a.tobytes() == b.tobytes()
    assert lattice_stars + st["host_stars"] == k and st["host_stars"] * 100 <= k
    # rotated, counter-clockwise, unit right triangles: two per cell, every one with its right angle's legs along the axes
    p = xy[a.astype(np.int64)]
    e1, e2 = p[:, 1] - p[:, 0], p[:, 2] - p[:, 0]
    assert ((e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]) == 1.0).all() and (a[:, 0] < a[:, 1]).all() and (a[:, 0] < a[:, 2]).all()
    assert len(np.unique(np.sort(a, axis=1), axis=0)) == len(a)


# ---- the affine surface -------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def affine_scene():
    pts, p2 = lattice_sets.affine_points(64, 48, 64)
    surface = triangulation.affine_surface(pts, p2)
    return surface, [(64, 48), (64, 48)]


def test_mesh_of_an_affine_surface(gpu_device):
    surface, dims = affine_scene()
    n = len(surface.points)
    ref_surface = ref_mesh.Surface.from_device(surface, dims)
    got = mesh.create(gpu_device, surface, dims, mesh.delaunay_device(gpu_device, lattice=True))
    assert mesh.delaunay_lattice(gpu_device) is False  # (the triangulator puts the setting back)
    want_p, want_c, per = ref_mesh.create(ref_surface, mesh.delaunay_device(gpu_device, lattice=False))
    assert np.array_equal(got["polygons"], want_p) and np.array_equal(got["camera"], want_c)
    for cam, (idx, polys, keep) in zip(got["per_camera"], per):
        assert cam["points"] == n == len(idx) and cam["polygons"] == len(polys) == cam["kept"] and keep.all()
    assert len(got["polygons"]) == per[0][1].shape[0] > 2 * n - 300 and (got["camera"] == 0).all()
    # the depth image: the same mask, values to 1e-9, and at a vertex pixel the vertex's own depth, bit for bit
    img = mesh.depth_image(gpu_device, surface, dims, 0, -1.0, got["polygons"])
    want_map, want_origin, want_min, want_max = ref_mesh.depth_image(ref_surface, 0, -1.0, got["polygons"])
    assert img["origin"] == want_origin and img["map"].shape == want_map.shape
    assert np.array_equal(np.isnan(img["map"]), np.isnan(want_map))
    filled = ~np.isnan(want_map)
    assert np.abs(img["map"][filled] - want_map[filled]).max() <= 1e-9
    assert abs(img["min_depth"] - want_min) <= 1e-9 and abs(img["max_depth"] - want_max) <= 1e-9
    vx, vy = surface.tracks[:, 0, 0] - int(want_origin[0]), surface.tracks[:, 0, 1] - int(want_origin[1])
    assert img["map"][vy, vx].tobytes() == (surface.points[:, 2] * -1.0).tobytes()
    # the PLY
    polys = got["polygons"]
    assert mesh.ply(gpu_device, surface, polys).tobytes() == ref_ply.ply_bytes(surface.points, surface.tracks, None, ref_ply.PLAIN,
                                                                               (1.0, 1.0, 1.0), polys)


def test_reconstruct_affine_mesh(gpu_device, tmp_path):
    c = cases.make_case("tilt3_200x150")
    p1, p2 = cases.pyramids(c)
    h, w = c["img1"].shape
    pc = correlation.PointCorrelations(gpu_device, (w, h), (c["img2"].shape[1], c["img2"].shape[0]), c["F"])
    try:
        for i in range(c["steps"] + 1):
            k = c["steps"] - i
            pc.correlate_images(p1[k], p2[k], 1.0 / float(1 << k))
        want_pts, want_p2 = pc.triangulate_affine()
    finally:
        pc.close()
    scale = (1.0, 1.0, 0.5)
    out = reconstruction.reconstruct_affine_mesh(gpu_device, p1, p2, c["F"], project_to_image=0, ply_path=str(tmp_path / "s.ply"),
                                                 obj_path=str(tmp_path / "s.obj"), out_scale=scale)
    assert mesh.delaunay_lattice(gpu_device) is False
    s, polys, camera = out["surface"], out["mesh"]["polygons"], out["mesh"]["camera"]
    n = len(want_pts)
    assert n > 1000 and s.points.tobytes() == want_pts.tobytes() and np.array_equal(s.tracks[:, 1], want_p2.astype(np.int32))
    assert np.array_equal(s.tracks[:, 0], want_pts[:, :2].astype(np.int32)) and len(s.cameras) == 2
    assert len(polys) > n and (camera == 0).all()
    for cam in out["mesh"]["per_camera"]:
        assert cam["points"] == n and cam["kept"] == cam["polygons"] == len(polys)
    # every track is a camera point, in track order: a polygon's vertices are positions in xy (`check` alone: re-fanning 25 000
    # tie pairs takes `canonical` many seconds, and the smaller sets above pin the tie rule)
    assert rd.check(rd.Points(want_pts[:, :2]), polys.astype(np.int64)) == []
    assert set(out["timings_ms"]) >= {"dense", "triangulate", "mesh", "depth_image", "ply", "obj"}
    img = out["depth_image"]
    assert img is not None and img["map"].shape[0] <= h and img["map"].shape[1] <= w and np.isfinite(img["map"]).sum() >= n
    ply = (tmp_path / "s.ply").read_bytes()
    assert len(ply) == sum(out["ply_sections"]) and out["ply_sections"][1:] == (24 * n, 13 * len(polys))
    assert ply == ref_ply.ply_bytes(s.points, s.tracks, None, ref_ply.PLAIN, scale, polys)
    obj = (tmp_path / "s.obj").read_bytes()
    assert len(obj) == sum(out["obj_sections"]) and out["obj_sections"][0] == 0 and out["obj_sections"][2] == 0
    assert obj == ref_obj.obj_bytes(s.points, s.tracks, None, ref_obj.PLAIN, scale, polys, camera, "s")
    assert tuple(ref_obj.obj_sections(obj, ref_obj.PLAIN)) == tuple(out["obj_sections"])
