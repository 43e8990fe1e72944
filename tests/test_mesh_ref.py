"""The numpy restatement of the mesh stage (tests/ref_mesh.py) against hand-computed cases and against a scalar
transcription of ProjectedPolygon's iterator, and the conditions the GPU tests rely on (tests/mesh_scenes.py's seeds)."""
import math

import numpy as np
import pytest

import mesh_scenes
import ref_mesh
import ref_triangulation as rt

EPS = ref_mesh.EPS


def flat_surface(points, seen=None, m=2, dims=(100, 100)):
    """m identical cameras that project (X, Y, Z) to (X, Y) with depth Z: P = [e1; e2; (0, 0, 0, 1)], r = t = 0."""
    points = np.asarray(points, dtype=np.float64).reshape(-1, 3)
    n = len(points)
    tracks = np.full((n, m, 2), -1, dtype=np.int32)
    seen = np.ones((n, m), dtype=bool) if seen is None else np.asarray(seen, dtype=bool)
    tracks[seen] = 1
    P = np.array([[1.0, 0.0, 0.0, 0.0], [0.0, 1.0, 0.0, 0.0], [0.0, 0.0, 0.0, 1.0]])
    cams = [rt.Camera(np.eye(3), np.zeros(3), np.zeros(3)) for _ in range(m)]
    return ref_mesh.Surface(points, tracks, cams, [P] * m, [dims] * m)


def emitted(pts, max_x, max_y):
    out = []
    for p, xs, ys, v in ref_mesh.walk(np.asarray(pts, dtype=np.float64).reshape(-1, 3, 3), max_x, max_y):
        out += [(int(a), int(b), int(c), float(d)) for a, b, c, d in zip(p, xs, ys, v)]
    return sorted(out)


def scalar_walk(pts, max_x, max_y):
    """ProjectedPolygon::new and its iterator (output.rs:115-254) for ONE polygon, statement by statement (a Python loop over
    the pixels: an independent check of the vectorised restatement on tiny cases)."""
    def clamp(v, hi):
        c = 0.0 if v < 0.0 else (float(hi) if v > float(hi) else v)
        return 0 if math.isnan(c) else int(c)

    def div(a, b):
        with np.errstate(all="ignore"):
            return float(np.float64(a) / np.float64(b))

    key = [int(ref_mesh.total_key(np.array([p[1]]))[0]) for p in pts]
    a, b, c = (pts[i] for i in sorted(range(3), key=lambda i: key[i]))  # (sorted is stable)
    out = []
    for yi in range(clamp(math.floor(a[1]) if math.isfinite(a[1]) else a[1], max_y),
                    clamp(math.ceil(c[1] + 1.0) if math.isfinite(c[1] + 1.0) else c[1] + 1.0, max_y)):
        y = float(yi)
        if y < a[1] or y > c[1]:
            continue
        if y < b[1] or abs(div(b[1] - c[1], b[0] - c[0])) < EPS:
            k = div(y - a[1], b[1] - a[1])
            sx, sv = a[0] * (1.0 - k) + b[0] * k, a[2] * (1.0 - k) + b[2] * k
        else:
            k = div(y - b[1], c[1] - b[1])
            sx, sv = b[0] * (1.0 - k) + c[0] * k, b[2] * (1.0 - k) + c[2] * k
        k = div(y - a[1], c[1] - a[1])
        ex, ev = a[0] * (1.0 - k) + c[0] * k, a[2] * (1.0 - k) + c[2] * k
        if not sx < ex:
            sx, ex, sv, ev = ex, sx, ev, sv
        fl = math.floor(sx) if math.isfinite(sx) else sx
        ce = math.ceil(ex + 1.0) if math.isfinite(ex + 1.0) else ex + 1.0
        for xi in range(clamp(fl, max_x), clamp(ce, max_x)):
            xc = div(float(xi) - sx, ex - sx)
            if 0.0 <= xc <= 1.0:
                out.append((0, xi, yi, sv * (1.0 - xc) + xc * ev))
    return sorted(out)


def test_three_pixel_triangle():
    """a = (0.5, 0.5), b = (2.5, 0.5), c = (0.5, 2.5) with values 1, 2, 3: row 0 lies above a.y; row 1 runs from the a-c
    edge (x = 0.5, value 1.5) to the b-c edge (x = 2, value 2.25) and emits x = 1 (x_c = 1/3) and x = 2 (x_c = 1); row 2
    from 0.5 (2.5) to 1.0 (2.75) and emits x = 1 (x_c = 1); row 3 lies below c.y."""
    tri = [[0.5, 0.5, 1.0], [2.5, 0.5, 2.0], [0.5, 2.5, 3.0]]
    got = emitted(tri, 10, 10)
    assert [g[1:3] for g in got] == [(1, 1), (1, 2), (2, 1)]
    assert got[0][3] == pytest.approx(1.75, abs=1e-15) and got[1][3] == 2.75 and got[2][3] == 2.25
    assert got == scalar_walk(tri, 10, 10)
    # the vertex order does not matter beyond the stable sort of equal y (a and b here)
    assert [g[1:3] for g in emitted([tri[2], tri[0], tri[1]], 10, 10)] == [(1, 1), (1, 2), (2, 1)]


def test_walk_matches_scalar_transcription():
    """Random small triangles, among them ones that reach past every edge of the grid, with vertices left of and above 0,
    with equal y, equal x and repeated vertices (the NaN and infinity paths): the same pixels and the same bits."""
    rng = np.random.default_rng(5)
    tris = rng.uniform(-3.0, 12.0, (300, 3, 3))
    tris[:40, :, :2] = np.round(tris[:40, :, :2])          # integer coordinates: y at a.y / b.y / c.y, x_c at 0 and 1
    tris[40:60, 1, 1] = tris[40:60, 0, 1]                  # a horizontal edge
    tris[60:80, 1, 0] = tris[60:80, 2, 0]                  # a vertical edge
    tris[80:90, 1] = tris[80:90, 0]                        # [v, v, w]
    tris[90:100, 2] = tris[90:100, 1]                      # [v, w, w]
    tris[100:110, 1] = tris[100:110, 0]
    tris[100:110, 2] = tris[100:110, 0]                    # [v, v, v]
    tris[110:115, 0, 0] = np.inf
    tris[115:120, 1, 1] = np.nan
    for max_x, max_y in ((9, 7), (0, 0), (1, 12)):
        got = emitted(tris, max_x, max_y)
        want = sorted((k,) + e[1:] for k, t in enumerate(tris) for e in scalar_walk([list(v) for v in t], max_x, max_y))
        assert len(got) == len(want)
        assert [g[:3] for g in got] == [w[:3] for w in want]
        assert np.array_equal(np.array([g[3] for g in got]), np.array([w[3] for w in want]), equal_nan=True)
        if max_x:
            assert len(got) > 50


def test_repeated_vertex_polygons_emit_nothing():
    v, w = [2.3, 3.1, 1.0], [6.8, 5.2, 2.0]
    for tri in ([v, v, w], [v, w, w], [v, v, v]):
        assert emitted(tri, 20, 20) == [] and scalar_walk(tri, 20, 20) == []


def test_depth_buffer_saturating_round_and_minimum():
    """(-0.7, -3.2) and (-0.2, 0.4) land in cell (0, 0) - `as usize` saturates -, which keeps the smaller depth; (2.5, 1.5)
    rounds half away from zero to (3, 2); the grid is (ceil(3.2) + 1) x (ceil(2.1) + 1); a track without a point in the
    camera, and one out of range, are not in it."""
    pts = [[-0.7, -3.2, 7.0], [-0.2, 0.4, 5.0], [2.5, 1.5, 4.0], [3.2, 2.1, 9.0], [1.0, 1.0, 1.0], [460.0, 1.0, 1.0]]
    seen = np.ones((6, 2), dtype=bool)
    seen[4, 1] = False
    s = flat_surface(pts, seen)
    buf = ref_mesh.depth_buffer(s, 1)
    assert buf.shape == (4, 5)
    want = np.full((4, 5), np.nan)
    want[0, 0], want[2, 3] = 5.0, 4.0
    want[2, 3] = 4.0   # (3.2, 2.1) rounds to the same cell (3, 2): the minimum of 4 and 9
    assert np.array_equal(buf, want, equal_nan=True)
    assert ref_mesh.depth_buffer(s, 0)[1, 1] == 1.0
    idx, xy = ref_mesh.camera_points(s, 1)
    assert idx.tolist() == [0, 1, 2, 3] and np.array_equal(xy, np.array(pts)[:4, :2])
    assert ref_mesh.depth_buffer(flat_surface(pts, np.zeros((6, 2), dtype=bool)), 1).shape == (0, 0)


def test_obstructs_rule():
    """A polygon at depth 3 over a cell that holds 5 obstructs (5 - 3 > EPSILON); at the cell's own depth, or behind it, it
    does not; over empty cells it does not; a 0 x 0 buffer obstructs nothing."""
    pts = [[1.0, 1.0, 5.0], [8.0, 8.0, 5.0],                       # what the buffer of camera 1 holds
           [0.5, 0.5, 3.0], [2.5, 0.5, 3.0], [0.5, 2.5, 3.0],      # in front of (1, 1)
           [0.5, 0.5, 5.0], [2.5, 0.5, 5.0], [0.5, 2.5, 5.0],      # at its depth
           [0.5, 0.5, 6.0], [2.5, 0.5, 6.0], [0.5, 2.5, 6.0],      # behind it
           [4.5, 4.5, 3.0], [6.5, 4.5, 3.0], [4.5, 6.5, 3.0]]      # over empty cells
    seen = np.zeros((14, 2), dtype=bool)
    seen[:, 0] = True
    seen[:2, 1] = True
    s = flat_surface(pts, seen)
    polys = [[2, 3, 4], [5, 6, 7], [8, 9, 10], [11, 12, 13]]
    assert ref_mesh.obstructs(s, 1, polys).tolist() == [True, False, False, False]
    keep, stats = ref_mesh.cull(s, 0, polys)
    assert keep.tolist() == [False, True, True, True] and stats[1] == (9, 9, 2, 1) and stats[0] == (0, 0, 0, 0)
    seen[:, 1] = False
    assert ref_mesh.cull(flat_surface(pts, seen), 0, polys)[0].all()


def test_depth_image_maximum_and_skipped_last_row_and_column():
    """Vertices at (0, 0), (2, 0), (0, 2) and (3, 3) with depths 1, 2, 3, 8: the origin is (0, 0) and the map 4 x 4
    (ceil(3) - floor(0) + 1).  The face (0, 0), (2, 0), (0, 2) gives row 0: 1, 1.5, 2; row 1: 2, 2.5; row 2: nothing (start =
    end = 0: 0 / 0).  The face (2, 0), (3, 3), (0, 2) reaches x = 3 and y = 3, but is walked with max_x = max_y = 3: the last
    row and column take no face pixels.  Every cell is the maximum of what it receives; scale = -1 negates the depths."""
    pts = [[0.0, 0.0, 1.0], [2.0, 0.0, 2.0], [0.0, 2.0, 3.0], [3.0, 3.0, 8.0], [500.0, 0.0, 1.0]]
    s = flat_surface(pts, np.zeros((5, 2), dtype=bool))  # visibility is not required
    img, origin, lo, hi = ref_mesh.depth_image(s, 0, 1.0, [[0, 1, 2], [1, 3, 2], [0, 1, 4]])  # (the last: a None vertex)
    assert img.shape == (4, 4) and origin == (0.0, 0.0)
    assert img[0, :3].tolist() == [1.0, 1.5, 2.0] and img[1, :2].tolist() == [2.0, 2.5] and img[2, 0] == 3.0
    assert img[2, 2] == pytest.approx(5.25, abs=1e-12)                  # the second face, inside: 3 * 0.25 + 0.75 * 6
    assert img[3, 3] == 8.0 and np.isnan(img[3, :3]).all() and np.isnan(img[:3, 3]).all()  # the splat only
    assert (lo, hi) == (1.0, 8.0)
    neg, _, lo, hi = ref_mesh.depth_image(s, 0, -1.0, [[0, 1, 2]])
    assert neg[0, 0] == -1.0 and neg[1, 1] == -2.5 and (lo, hi) == (-8.0, -1.0)
    # two vertices in one cell: the larger stays
    two, _, _, _ = ref_mesh.depth_image(flat_surface([[0.2, 0.2, 1.0], [0.4, 0.3, 2.0], [5.0, 5.0, 0.0]]), 0, 1.0, [])
    assert two[0, 0] == 2.0
    assert ref_mesh.depth_image(flat_surface([[900.0, 0.0, 1.0]]), 0, 1.0, []) is None


def test_merge_rotation_and_deduplication():
    polys, cams = ref_mesh.merge([(0, [[5, 2, 9], [9, 5, 2], [7, 8, 3]]), (1, [[2, 9, 5], [1, 4, 6], [2, 5, 9]]), (2, [[6, 1, 4], [0, 1, 2]])])
    # (5, 2, 9), (9, 5, 2) and (2, 9, 5) are one polygon (2, 9, 5): camera 0 keeps it; (2, 5, 9) has the other orientation
    assert polys.tolist() == [[2, 9, 5], [3, 7, 8], [1, 4, 6], [2, 5, 9], [0, 1, 2]]
    assert cams.tolist() == [0, 0, 1, 1, 2]
    assert ref_mesh.rotate([4, 4, 1]) == (1, 4, 4) and ref_mesh.rotate([3, 3, 3]) == (3, 3, 3) and ref_mesh.rotate([1, 1, 2]) == (2, 1, 1)


@pytest.mark.parametrize("m", [2, 3, 4, 8])
def test_scene_seeds_meet_the_gpu_tests_conditions(m):
    """What tests/test_mesh_gpu.py assumes of mesh_scenes.scene(m): near_threshold is empty for every camera_i (culling and
    the depth image), every other camera both drops and keeps at least 5 % of the polygons, the long triangles are there,
    some polygons have vertices left of or above 0 and past the buffer's edge, and some are dropped through the foreground."""
    s = mesh_scenes.scene(m)
    outside = np.zeros(4, dtype=bool)
    for i in range(m):
        polys = mesh_scenes.polygons(s, i)
        near = ref_mesh.near_threshold(s.surface, polys, camera_i=i, project_to_image=i)
        assert near.empty(), (i, near.polygons, near.cells, near.tracks)
        keep, stats = ref_mesh.cull(s.surface, i, polys)
        for j in range(m):
            if j != i:
                assert 0.05 * len(polys) <= stats[j][3] <= 0.95 * len(polys)
        assert 0.05 < keep.mean() < 0.95
        for j in range(m):
            if j == i:
                continue
            x, y = s.surface.project(j)
            px, py = x[polys.astype(np.int64)], y[polys.astype(np.int64)]
            w, h = stats[j][0], stats[j][1]
            outside |= np.array([(px < 0).any(), (py < 0).any(), ((px > w) | (py > h)).any(),
                                 ((px.max(axis=1) < 0) | (px.min(axis=1) > w)).any()])
    assert outside.all(), outside  # (over the scene's camera pairs: left of 0, above 0, past the right or lower edge, entirely outside)
    assert s.n_long >= 5 and len(s.surface.points) == 2 * 96 * 64


def test_create_with_delaunay_scipy():
    """mesh.delaunay_scipy's triangles through the restatement's create: every kept polygon is a Delaunay face of its
    camera's points, rotated; the list is grouped by camera and holds no vertex triple twice."""
    pytest.importorskip("scipy")
    from cybervision_amd import mesh

    s = mesh_scenes.scene(3)
    polys, cams, per = ref_mesh.create(s.surface, mesh.delaunay_scipy)
    assert len(polys) > 1000 and (np.diff(cams.astype(np.int64)) >= 0).all() and set(cams.tolist()) == {0, 1, 2}
    assert len({tuple(p) for p in polys.tolist()}) == len(polys)
    assert (polys[:, 0] <= polys[:, 1]).all() and (polys[:, 0] <= polys[:, 2]).all()
    for i, (idx, faces, keep) in enumerate(per):
        assert 0 < keep.sum() < len(keep)
        mine = {ref_mesh.rotate(f) for f in faces[keep].tolist()}
        assert {tuple(p) for p in polys[cams == i].tolist()} <= mine


def test_delaunay_scipy_reports_a_missing_scipy(monkeypatch):
    import builtins

    from cybervision_amd import mesh

    real = builtins.__import__

    def no_scipy(name, *a, **k):
        if name.startswith("scipy"):
            raise ImportError(name)
        return real(name, *a, **k)

    monkeypatch.setattr(builtins, "__import__", no_scipy)
    with pytest.raises(RuntimeError, match="scipy"):
        mesh.delaunay_scipy(np.zeros((4, 2)))


MIXED_CASES = [(3, 0), (3, 1), (3, 2), (8, 5), (8, 6)]  # (tests/test_mesh_gpu.py's)


@pytest.mark.parametrize("m,i", MIXED_CASES)
def test_mixed_scene_seeds_meet_the_gpu_tests_conditions(m, i):
    """What test_mixed_dims_match_restatement_on_both_paths assumes of mesh_scenes.scene(m, mixed=True): no two image
    sizes alike, landscape and portrait, a K per camera with fx != fy and skew; every track seen in a camera lies inside
    that camera's own image, and some only because the test is per axis (a pixel past the OTHER side's length); near_threshold is empty for camera_i; more than
    1000 camera points; every other camera drops between 5 % and 95 % of the polygons.  The plain scene is what it was."""
    s = mesh_scenes.scene(m, mixed=True)
    dims = s.image_dims
    assert dims == mesh_scenes.mixed_dims(m) and len(set(dims)) == m
    assert any(w > h for w, h in dims[:3]) and any(w < h for w, h in dims[:3])
    per_axis = 0
    for j, (w, h) in enumerate(dims):
        K = s.cams[j][0]
        assert K[0, 0] != K[1, 1] and K[0, 1] != 0.0 and K[0, 2] != K[1, 2]
        t = s.surface.tracks[s.surface.seen(j), j]
        assert t[:, 0].max() < w and t[:, 1].max() < h and t.min() >= 0
        per_axis += int(((t[:, 0] >= min(w, h)) | (t[:, 1] >= min(w, h))).sum())
    assert per_axis > 1000
    polys = mesh_scenes.polygons(s, i)
    near = ref_mesh.near_threshold(s.surface, polys, camera_i=i, project_to_image=i)
    assert near.empty(), (near.polygons, near.cells, near.tracks)
    assert len(ref_mesh.camera_points(s.surface, i)[0]) > 1000
    keep, stats = ref_mesh.cull(s.surface, i, polys)
    for j in range(m):
        if j != i:
            assert 0.05 * len(polys) <= stats[j][3] <= 0.95 * len(polys), (j, stats[j])
    plain = mesh_scenes.scene(m)
    assert plain.image_dims == [(mesh_scenes.SIZE, mesh_scenes.SIZE)] * m and np.array_equal(plain.cams[0][0], plain.cams[m - 1][0])
