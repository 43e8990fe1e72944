"""The surface of the mesh-output tests (test_mesh_output_gpu.py, test_host_mesh_output_cpp_gpu.py): tests/mesh_scenes.py's
scene(3) - 12 288 tracks, camera 0's polygons - with random RGB images from a fixed seed.  527 of the scene's tracks have
lost every point to the image edges; Color mode refuses such a track, so they are given a point here.  The images are
narrower than the scene's 320^2 - (200, 280), (160, 200), (250, 320): the foreground patch, tracks 6144 .. 12287, projects
to x 90 .. 211, and only images this narrow cut it - so that every one of the 48 blocks of 256 tracks holds 24-byte and
27-byte records (test_whole_file_three_modes asserts it)."""
import functools

import numpy as np

import mesh_scenes
import ref_ply
from cybervision_amd import triangulation

SCALE = (1.5, -2.0, 0.75)
NARROW = [(200, 280), (160, 200), (250, 320)]  # (width, height) per image


def random_images(dims, seed=7):
    rng = np.random.default_rng(seed)
    return [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for w, h in dims]


def surface_of(points, tracks):
    return triangulation.Surface(points=np.ascontiguousarray(points), track_index=np.arange(len(points)),
                                 tracks=np.ascontiguousarray(tracks, dtype=np.int32), cameras=[])


@functools.lru_cache(maxsize=None)
def scene():
    """-> (points [n, 3], tracks [n, 3, 2] with a point in every track, polygons [p, 3], images)"""
    s = mesh_scenes.scene(3)
    points, tracks = s.surface.points.copy(), s.surface.tracks.copy()
    points[5, 1] = 0.0       # -0.0 in the file
    points[6] = [np.nan, np.inf, -np.inf]
    none = np.flatnonzero(ref_ply.first_points(tracks)[0] < 0)
    tracks[none, none % 3] = np.stack([(7 * none) % 320, (13 * none) % 320], axis=1)
    return points, tracks, mesh_scenes.polygons(s, 0), random_images(NARROW)
