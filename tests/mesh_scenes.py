"""Scenes for the mesh-stage tests (test_mesh_ref.py, test_mesh_gpu.py): tri_scenes.rig(m) looking at a background plane
and a smaller foreground patch in front of it, so that in the other cameras the foreground's polygons lie in front of
background points those cameras see - real polygons are both culled and kept."""
from __future__ import annotations

import numpy as np

import mixed_scenes
import ref_mesh
import tri_scenes

SIZE = 320          # image size of the rig: buffers of ~350^2 cells, lattice cells of ~4 x 5 pixels
LATTICE = (96, 64)  # points per plane
# seeds per camera count for which ref_mesh.near_threshold is empty for every camera_i (checked by test_mesh_ref.py)
SEEDS = {2: 1, 3: 1, 4: 1, 8: 1}
# the same for scene(m, mixed=True)
MIXED_SEEDS = {3: 2, 8: 3}


class Scene:
    pass


def _plane(rng, x_half, y_half, z, jitter):
    """A jittered LATTICE[0] x LATTICE[1] lattice on the plane Z = z: the jitter (a fraction of the spacing in X and Y,
    `jitter` in Z) keeps the projections off integers and the depths of a cell apart."""
    nx, ny = LATTICE
    gx, gy = np.meshgrid(np.linspace(-x_half, x_half, nx), np.linspace(-y_half, y_half, ny))
    sx, sy = 2 * x_half / (nx - 1), 2 * y_half / (ny - 1)
    X = gx + rng.uniform(-0.3, 0.3, gx.shape) * sx
    Y = gy + rng.uniform(-0.3, 0.3, gy.shape) * sy
    Z = z + rng.uniform(-jitter, jitter, gx.shape)
    return np.stack([X.ravel(), Y.ravel(), Z.ravel()], axis=1)


def lattice_triangles(offset=0):
    """Two triangles per lattice cell (the split does not depend on scipy), as indices offset + row * nx + column."""
    nx, ny = LATTICE
    r, c = np.meshgrid(np.arange(ny - 1), np.arange(nx - 1), indexing="ij")
    v00 = (r * nx + c).ravel() + offset
    v01, v10, v11 = v00 + 1, v00 + nx, v00 + nx + 1
    return np.concatenate([np.stack([v00, v01, v11], axis=1), np.stack([v00, v11, v10], axis=1)])


def axis_angle(R):
    """The r with matrix_r(r) = R, for rotations by less than 180 degrees."""
    rho = np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]]) / 2.0
    s = np.linalg.norm(rho)
    if s == 0.0:
        return np.zeros(3)
    return rho / s * np.arctan2(s, (np.trace(R) - 1.0) / 2.0)


def facing_rig(m, size=SIZE):
    """tri_scenes.rig(m)'s cameras - K, and the same centres - with the cameras on the arc turned to face the scene centre
    (0, 0, 5): rig's own rotation rot_y(-theta) turns them the other way, so that the centre projects far outside their
    images; the transpose is the rotation its docstring describes."""
    cams = []
    for j, (K, R, t) in enumerate(tri_scenes.rig(m, size=size, near_duplicate=False)):
        if j >= 2:
            C = -R.T @ t
            R = R.T
            t = -R @ C
        cams.append((K, R, t))
    return cams


def mixed_dims(m):
    """mixed_scenes.DIMS at SIZE pixels on the longest side: (320, 200), (200, 320), (300, 225), (160, 240), (320, 320),
    (250, 141), (141, 250), (200, 160)."""
    return mixed_scenes.dims(m, 2048 / SIZE)


def scene(m, seed=None, size=SIZE, mixed=False):
    """-> Scene: cams (rig(m)), surface (ref_mesh.Surface over the true points), image_dims, triangles (all lattice
    triangles of both planes), n_background.  mixed: camera j has mixed_scenes' K for its own image size mixed_dims(m)[j]
    (no two alike, landscape and portrait), and a track is seen inside that image."""
    seed = (MIXED_SEEDS if mixed else SEEDS).get(m, 1) if seed is None else seed
    rng = np.random.default_rng(1000 * m + seed)
    cams = facing_rig(m, size)
    dims = [(size, size)] * m
    if mixed:
        dims = mixed_dims(m)
        cams = [(mixed_scenes.calibration(j, dims[j]), R, t) for j, (_, R, t) in enumerate(cams)]
    # the background reaches past the image on every side (projections left of and above 0, and past the buffers' edges:
    # a track is seen only inside an image); the foreground hides its middle
    back = _plane(rng, 5.9, 5.8, 5.5, 0.02)
    front = _plane(rng, 1.4, 1.0, 4.4, 0.02)
    X = np.concatenate([back, front])
    n = len(X)
    # every track in a random subset of the cameras, at least two
    k = rng.integers(2, m + 1, n)
    order = np.argsort(rng.random((n, m)), axis=1)
    mask = np.zeros((n, m), dtype=bool)
    np.put_along_axis(mask, order, np.arange(m)[None, :] < k[:, None], axis=1)
    tracks = tri_scenes.observe(cams, X, mask)
    tracks[(tracks >= np.array(dims)[None]).any(axis=2)] = -1  # (and what falls past the right or lower edge of an image)
    s = Scene()
    s.m, s.seed, s.size, s.cams = m, seed, size, cams
    s.image_dims = dims
    # (not Camera::from_matrix: as written it turns a camera by more than its R - ref_triangulation notes the factor 2 -,
    # and the scene's tracks were observed through R itself)
    s.surface = ref_mesh.Surface.from_poses(X, tracks, [(K, axis_angle(R), t) for K, R, t in cams], s.image_dims)
    s.n_background = len(back)
    s.triangles = np.concatenate([lattice_triangles(0), lattice_triangles(len(back))]).astype(np.int64)
    s.n_long = 6
    return s


def polygons(s, camera_i):
    """Camera_i's polygons: the lattice triangles whose three vertices are camera points of camera_i (seen there and in
    range), then s.n_long long triangles that join far-apart camera points - of the background, and across the two
    planes -, so that they span most of a buffer."""
    idx, _ = ref_mesh.camera_points(s.surface, camera_i)
    on = np.zeros(len(s.surface.points), dtype=bool)
    on[idx] = True
    b, f = idx[idx < s.n_background], idx[idx >= s.n_background]  # (track order is the lattice's row-major order)
    long_ones = np.array([[b[0], b[-1], b[len(b) // 2]], [b[0], b[len(b) // 3], f[len(f) // 2]], [b[-1], f[0], f[-1]],
                          [b[len(b) // 4], b[3 * len(b) // 4], b[-1]], [f[0], b[len(b) // 2], b[-2]], [b[1], b[-3], f[len(f) // 3]]])
    return np.concatenate([s.triangles[on[s.triangles].all(axis=1)], long_ones]).astype(np.uint32)


def lattice_triangulate(s, camera_i):
    """A `triangulate(xy)` for mesh.create / ref_mesh.create on this scene: the lattice split restricted to camera_i's
    points, as indices into them (the points come in track order)."""
    idx, _ = ref_mesh.camera_points(s.surface, camera_i)
    where = np.full(len(s.surface.points), -1, dtype=np.int64)
    where[idx] = np.arange(len(idx))
    faces = where[polygons(s, camera_i).astype(np.int64)]

    def triangulate(xy):
        assert len(xy) == len(idx)
        return faces

    return triangulate


def device_surface(s):
    """The scene's surface as cybervision_amd.triangulation.Surface (what the mesh entry points take)."""
    from cybervision_amd import triangulation

    sf = s.surface
    return triangulation.Surface(points=sf.points, track_index=np.arange(len(sf.points)), tracks=sf.tracks,
                                 cameras=[triangulation.Camera(c.r.copy(), c.t.copy(), sf.projections[j].copy())
                                          for j, c in enumerate(sf.cameras)])
