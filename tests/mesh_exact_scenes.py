"""Scenes on which the mesh stage is exact (test_mesh_exact_ref.py, test_mesh_exact_gpu.py): three cameras with r = 0 -
matrix_r takes its identity branch on the host, no library function runs - and dyadic projections and t, points on the
quarter lattice and depths a few EPSILON apart.  Every projection and depth is then an exact IEEE result, the device and
the restatement (tests/ref_mesh.py) run the same operations, and every rule that hangs on a comparison - a vertex on an
integer row or column, x_c at 0 or 1, a projection at .5, a margin of exactly EPSILON, a projection on the range edge, a
horizontal or vertical edge, NaN, infinity, -0.0 - can be compared bit for bit.

This module restates nothing: it builds a ref_mesh.Surface (and through mesh_scenes.device_surface the device's) and
chooses polygons.

The cameras, as rows of the projection, and t:
  0: [e1; e2; (0, 0, 0, 1)], t = 0                          x = X,        y = Y,       depth = Z
  1: [(2, 0, 0, 1); (0, 2, 0, -1); (0, 0, 0, 2)], t.z = .25 x = X + 0.5,  y = Y - 0.5, depth = Z + 0.25 (quarter-lattice points land
                                                            on halves and integers)
  2: [(1, 0, 0, .25); e2; (0, 0, 0, 0)], t.z = -.5          x = X + 0.25, y = Y,       depth = Z - 0.5 (w = 0: the |w| < EPSILON branch)
e2 is written (-0.0, 1, -0.0, -0.0) - the same numbers.  With (+0, 1, +0, +0) the sum ((0 X + Y) + 0 Z) + 0 is +0.0 for
Y = -0.0 (a sum is -0.0 only if every term is), so no -0.0 would ever reach ProjectedPolygon's total_cmp sort; with the
signed zeros a track with Y = -0.0, X >= +0 and Z > 0 projects to y = -0.0, and every other y is unchanged.
"""
from __future__ import annotations

import functools

import numpy as np

import mesh_scenes
import ref_mesh
import ref_triangulation as rt

EPS = ref_mesh.EPS
SIZE = (40, 24)  # not square; img_range is [-140, 180) x [-84, 108)
E2 = (-0.0, 1.0, -0.0, -0.0)
PROJECTIONS = np.array([[(1.0, 0.0, 0.0, 0.0), E2, (0.0, 0.0, 0.0, 1.0)],
                        [(2.0, 0.0, 0.0, 1.0), (0.0, 2.0, 0.0, -1.0), (0.0, 0.0, 0.0, 2.0)],
                        [(1.0, 0.0, 0.0, 0.25), E2, (0.0, 0.0, 0.0, 0.0)]])
T = np.array([(0.0, 0.0, 0.0), (0.0, 0.0, 0.25), (0.0, 0.0, -0.5)])
OFFSET = [(0.0, 0.0), (0.5, -0.5), (0.25, 0.0)]  # (x - X, y - Y) per camera
# Margins of exactly EPSILON, and one step to either side of it, occur among these; none is 0 in any camera.  Camera 1 adds
# 0.25: the values next to 1 land in [1, 2), where depths are EPSILON apart, and the ones below 0.75 just below 1, where
# they are EPSILON / 2 apart - without them no margin of camera 1 would lie inside (0, EPSILON).
Z_VALUES = np.array([1.0, 1.0 - EPS / 2, 1.0 - EPS, 1.0 - 1.5 * EPS, 1.0 - 2 * EPS, 1.0 + EPS, 1.0 + 2 * EPS,
                     0.75, 0.75 - EPS / 2, 0.75 - EPS, 0.75 - 1.5 * EPS, 0.75 - 2 * EPS, 0.75 - 2.5 * EPS, 0.75 - 3 * EPS, 1.25, 1.5])
Z_WEIGHTS = np.array([2.0] * 7 + [3.0] * 7 + [4.0] * 2) / 43.0  # (the values next to 0.75 are the front, the last two the back)
EDGE_X = (-140.0, 180.0, -140.25, 179.75)  # on lo (in), on hi (out), below lo (out), below hi (in)
EDGE_Y = (-84.0, 108.0, 107.75)
N_RANDOM, N_LOCAL, N_LONG, SEEN = 1500, 1500, 12, 0.7
MIN_AWAY = 2.0  # of a local triple's second and third vertex from the first, in pixels: polygons that cover a few cells


def cameras():
    return [rt.Camera(np.eye(3), np.zeros(3), T[j]) for j in range(3)]


def surface(points, tracks, dims=None):
    return ref_mesh.Surface(points, tracks, cameras(), PROJECTIONS, [SIZE] * 3 if dims is None else dims)


def lattice_points(rng, n):
    """n points with X, Y random multiples of 1/4 that reach 3 pixels past the image on every side, Z from Z_VALUES."""
    X = rng.integers(-12, 4 * (SIZE[0] + 3) + 1, n) / 4.0
    Y = rng.integers(-12, 4 * (SIZE[1] + 3) + 1, n) / 4.0
    return np.stack([X, Y, rng.choice(Z_VALUES, n, p=Z_WEIGHTS)], axis=1)


def seen_tracks(mask):
    """tracks [n, m, 2]: (1, 1) where mask [n, m], (-1, -1) = None elsewhere"""
    tracks = np.full(mask.shape + (2,), -1, dtype=np.int32)
    tracks[mask] = 1
    return tracks


class Scene:
    pass


@functools.lru_cache(maxsize=None)
def scene(seed=7):
    """-> Scene: surface, image_dims, and the hand-placed tracks by name: edge[camera] = {"x": {x: track}, "y": {y: track}},
    inf, nan, neg_zero, far (lists of tracks), sort_cases (polygons whose flag hangs on the order of -0.0 and +0.0; the
    last two are controls that it does not move), hand (the tracks of the polygons worked by hand)."""
    rng = np.random.default_rng(seed)
    pts = [lattice_points(rng, N_RANDOM)]
    n = N_RANDOM
    s = Scene()

    def place(rows):
        nonlocal n
        rows = np.asarray(rows, dtype=np.float64).reshape(-1, 3)
        pts.append(rows)
        n += len(rows)
        return list(range(n - len(rows), n))

    # on and next to the range edge of every camera, on both axes (the other coordinate well inside)
    s.edge = []
    for dx, dy in OFFSET:
        ex = place([(x - dx, 10.0 - dy, 1.25) for x in EDGE_X])
        ey = place([(20.0 - dx, y - dy, 1.25) for y in EDGE_Y])
        s.edge.append({"x": dict(zip(EDGE_X, ex)), "y": dict(zip(EDGE_Y, ey))})
    inf, nan = np.inf, np.nan
    s.inf = place([(inf, 5.0, 1.0), (-inf, 6.0, 1.0), (7.0, inf, 1.0), (8.0, -inf, 1.0), (9.0, 9.0, inf), (9.0, 10.0, -inf)])
    s.nan = place([(nan, 5.0, 1.0), (6.0, nan, 1.0), (7.0, 7.0, nan)])
    s.neg_zero = place([(-0.0, -0.0, 1.0), (0.0, -0.0, 0.75), (3.0, -0.0, 0.75), (-0.0, 4.0, 1.0), (17.0, -0.0, 0.75), (30.25, -0.0, 1.0)])
    # Far to the right on the row y = +0.0 (not in range; culling does not ask for that): with a vertex at y = -0.0 and one
    # below, total_cmp makes the -0.0 vertex a and this one b; the b-c edge is then flat within EPSILON, the a-b edge
    # divides by b.y - a.y = 0 and the polygon emits nothing.  An order that takes -0.0 == +0.0 keeps the input order, this
    # vertex is a, and the rows from the b-c edge to the far a-c edge are emitted.
    s.far = place([(1e300, 0.0, 0.75), (-1e300, 0.0, 0.75)])
    low = place([(5.0, 4.0, 0.75), (20.0, 6.0, 0.75), (33.0, 3.0, 0.75)])
    s.sort_cases = np.array([[s.far[0], s.neg_zero[2], low[0]], [s.far[0], s.neg_zero[4], low[1]], [s.far[1], s.neg_zero[5], low[2]],
                             [s.neg_zero[2], s.far[0], low[0]], [low[1], s.far[0], s.neg_zero[4]]], dtype=np.int64)
    # the polygons that test_mesh_exact_ref.py works by hand: flat-topped and with a vertical b-c edge in camera 0; in
    # camera 1 the middle vertex of the third overflows to x = +inf (2 X), with y = 4 and a finite depth
    s.hand = {"flat_top": place([(10.0, 2.0, 1.0), (12.0, 2.0, 1.0), (10.0, 4.0, 1.5)]),
              "vertical": place([(20.0, 1.0, 1.0), (22.0, 3.0, 1.5), (22.0, 5.0, 0.75)]),
              "infinite": place([(9.5, 2.5, 0.75), (1.5e308, 4.5, 0.75), (9.5, 6.5, 0.75)])}
    points = np.concatenate(pts)
    mask = rng.random((n, 3)) < SEEN
    mask[N_RANDOM:] = True  # the hand-placed tracks are seen everywhere
    s.surface = surface(points, seen_tracks(mask))
    s.image_dims = [SIZE] * 3
    s.n_random = N_RANDOM
    return s


@functools.lru_cache(maxsize=None)
def polygons(camera_i, seed=7):
    """Camera_i's polygons [k, 3] uint32: N_LOCAL triples among camera points at most 3 pixels from the first (many share a
    row or a column, some repeat a vertex), N_LONG triples from anywhere (half of them across the whole buffer), and polygons that name the infinite, NaN, -0.0
    and far tracks (culling does not require a polygon's vertices to be in range or seen)."""
    s = scene(seed)
    rng = np.random.default_rng(100 * seed + camera_i)
    idx, xy = ref_mesh.camera_points(s.surface, camera_i)
    local = np.zeros((N_LOCAL, 3), dtype=np.int64)
    for k, first in enumerate(rng.integers(0, len(idx), N_LOCAL)):
        away = np.abs(xy - xy[first]).max(axis=1)
        around = np.nonzero((away <= 3.0) & ((away >= MIN_AWAY) | (k % 8 == 0)))[0]  # (every eighth: any, the first included)
        if len(around) == 0:  # (a lone track on the range edge)
            around = np.array([first])
        local[k] = idx[first], *idx[rng.choice(around, 2)]
    far_apart = idx[rng.integers(0, len(idx), (N_LONG, 3))]
    # half of them from the track a quarter below the range's right edge to the one a quarter below its lower edge: a box of
    # 160 x 98 cells, past the wave path's default threshold
    corners = [s.edge[camera_i]["x"][EDGE_X[3]], s.edge[camera_i]["y"][EDGE_Y[2]]]
    for k in range(N_LONG // 2):
        far_apart[k] = np.roll([corners[0], corners[1], far_apart[k, 2]], k)
    named = []
    for v in s.inf + s.nan + s.neg_zero + s.far:
        u, w = idx[rng.integers(0, len(idx), 2)]
        named += [(v, u, w), (u, v, w), (u, w, v)]
    named += [(s.inf[0], s.inf[1], idx[0]), (s.nan[0], s.nan[1], s.nan[2]), (s.neg_zero[0], s.neg_zero[1], s.neg_zero[3])]
    named += [tuple(v) for v in s.hand.values()]
    return np.concatenate([local, far_apart, np.array(named, dtype=np.int64), s.sort_cases]).astype(np.uint32)


def device(s):
    return mesh_scenes.device_surface(s)


# ---- img_range per camera and per axis ------------------------------------------------------------------------------------
# Landscape, portrait, and a third shape: img_range is [-1120, 1440) x [-700, 900), [-700, 900) x [-1120, 1440) and
# [-840, 1080) x [-1120, 1440).  With x held against the height's range or y against the width's - or with another
# camera's dims - tracks on these edges change sides.
EDGE_DIMS = [(320, 200), (200, 320), (240, 320)]
N_EDGE_RANDOM, N_EDGE_POLYGONS = 600, 24


def edge_values(size):
    """Per axis the coordinates (on lo: in, a quarter below lo: out, a quarter below hi: in, on hi: out) of img_range(size)."""
    lo, hi = ref_mesh.img_range(size)
    return [(lo[a], lo[a] - 0.25, hi[a] - 0.25, hi[a]) for a in range(2)]


@functools.lru_cache(maxsize=None)
def edge_scene(seed=13):
    """-> Scene over the exact cameras with EDGE_DIMS: N_EDGE_RANDOM lattice points, and for every camera and axis four
    hand-placed tracks on both sides of both ends of its img_range (edge_values), the other coordinate at 10, depth 1.25,
    seen everywhere.  edge[camera] = {"x": {x: track}, "y": {y: track}}."""
    rng = np.random.default_rng(seed)
    pts = [lattice_points(rng, N_EDGE_RANDOM)]
    n = N_EDGE_RANDOM
    s = Scene()
    s.edge = []
    for (dx, dy), size in zip(OFFSET, EDGE_DIMS):
        xs, ys = edge_values(size)
        pts.append(np.array([(x - dx, 10.0 - dy, 1.25) for x in xs] + [(10.0 - dx, y - dy, 1.25) for y in ys]))
        s.edge.append({"x": dict(zip(xs, range(n, n + 4))), "y": dict(zip(ys, range(n + 4, n + 8)))})
        n += 8
    mask = rng.random((n, 3)) < SEEN
    mask[N_EDGE_RANDOM:] = True
    s.surface = surface(np.concatenate(pts), seen_tracks(mask), EDGE_DIMS)
    s.image_dims = list(EDGE_DIMS)
    return s


@functools.lru_cache(maxsize=None)
def edge_polygons(camera_i, seed=13):
    """N_EDGE_POLYGONS triples for camera_i of edge_scene: half local ones among its lattice camera points (at most 3
    pixels from the first, as polygons()), half with one or two of the edge tracks that are in range (polygons that cross
    most of a buffer 1441 or 901 cells wide)."""
    s = edge_scene(seed)
    rng = np.random.default_rng(100 * seed + camera_i)
    idx, xy = ref_mesh.camera_points(s.surface, camera_i)
    small, far = idx[idx < N_EDGE_RANDOM], idx[idx >= N_EDGE_RANDOM]
    polys = small[rng.integers(0, len(small), (N_EDGE_POLYGONS, 3))]
    for k in range(N_EDGE_POLYGONS):
        away = np.abs(xy[:len(small)] - xy[np.nonzero(small == polys[k, 0])[0][0]]).max(axis=1)
        around = np.nonzero((away <= 3.0) & (away >= MIN_AWAY))[0]
        if len(around):
            polys[k, 1:] = small[rng.choice(around, 2)]
    half = N_EDGE_POLYGONS // 2
    polys[:half, 0] = far[rng.integers(0, len(far), half)]
    polys[:half // 2, 1] = far[rng.integers(0, len(far), half // 2)]
    return polys.astype(np.uint32)


@functools.lru_cache(maxsize=None)
def sized(n, seed=11):
    """-> Scene of n lattice points for the size tests.  Up to a few hundred points every track is seen in every camera (a
    single one projects to integers in camera 1);
    past that the selection is sparse and ragged: every 97th track, the first and the last are seen, and every eighth
    track lies out of range."""
    rng = np.random.default_rng(seed + n)
    points = lattice_points(rng, n)
    mask = np.ones((n, 3), dtype=bool)
    if n == 1:
        points[0, :2] = 5.5, 3.5  # (6, 3) in camera 1: a 1 x 1 depth image
    if n > 1000:
        points[::8, 0] += 1000.0
        mask[:] = False
        mask[::97] = True
        mask[[0, -1]] = True
        points[[0, -1], 0] = 5.0, 6.0
    s = Scene()
    s.surface = surface(points, seen_tracks(mask))
    s.image_dims = [SIZE] * 3
    return s


@functools.lru_cache(maxsize=None)
def wave_case():
    """-> Scene for the wave walk's column steps and its last row: the scene's tracks, two occupied cells of camera 0 at
    depth 1.5 in rows that are otherwise empty - (150, 60) and (165, 50) -, and camera 1's `polygons`, at depth 0.75 and seen
    nowhere: [0] a long thin one whose last emitted row, 60, runs from x = 2.5 to 170.5 (b lies ON the row, so the b-c edge
    starts there) - (150, 60) is its only occupied cell, in the third 64-lane step of the row, columns 130 to 193 -; [2] a
    small one whose last emitted row, 50, holds (165, 50); [1] and [3] their twins one row up, over empty cells only."""
    base = scene().surface
    cells = [(150.0, 60.0, 1.5), (165.0, 50.0, 1.5)]
    long_one = [(2.5, 45.5, 0.75), (170.5, 60.0, 0.75), (2.5, 60.5, 0.75)]
    small = [(160.5, 40.5, 0.75), (170.5, 50.0, 0.75), (160.5, 50.5, 0.75)]
    up = np.array([0.0, 1.0, 0.0])
    extra = np.concatenate([np.array(cells), np.array(long_one), np.array(long_one) - up, np.array(small), np.array(small) - up])
    n = len(base.points)
    tracks = np.concatenate([base.tracks, np.full((len(extra), 3, 2), -1, dtype=np.int32)])
    tracks[n:n + len(cells), 0] = 1
    s = Scene()
    s.surface = surface(np.concatenate([base.points, extra]), tracks)
    s.image_dims = [SIZE] * 3
    s.polygons = (n + len(cells) + np.arange(12).reshape(4, 3)).astype(np.uint32)
    s.cells = [(150, 60), (165, 50)]
    return s
