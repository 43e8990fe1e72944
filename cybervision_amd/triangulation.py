"""PerspectiveTriangulation (src/triangulation.rs:604-1593) over the C ABI: the dense track table that
extend_tracks builds pair by pair, and triangulate_all (:817-865) - DLT points, filter_outliers and the bundle
adjustment - in one call of cvhip_triangulate_perspective.  The cameras are the caller's: pose recovery
(recover_pose / find_projection_matrix, :1033-1278) and merge_tracks (:1421-1540) are not part of this module.
No compute in Python - the track table's bookkeeping and the calls only.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass, field

import numpy as np

from . import _lib

MAX_CAMERAS = 8  # CVHIP_TRIANGULATE_MAX_CAMERAS
BUNDLE_ADJUSTMENT_MAX_ITERATIONS = 100  # triangulation.rs:15


@dataclass
class Camera:
    """The refined camera of a surface: axis-angle r, translation t and projection K [R | t] (Camera, :404-507)."""
    r: np.ndarray
    t: np.ndarray
    projection: np.ndarray


@dataclass
class Surface:
    """Surface (triangulation.rs:142-150) as the device returns it: points[i] belongs to track row track_index[i] of the
    table (tracks[i] is that row); one camera per image.  ba_*: what the bundle adjustment did (iterations, accept (1) /
    reject (0) per iteration, |residual| before and after; NaN without bundle adjustment)."""
    points: np.ndarray
    track_index: np.ndarray
    tracks: np.ndarray
    cameras: list
    ba_iterations: int = 0
    ba_history: list = field(default_factory=list)
    ba_residual_norms: tuple = (float("nan"), float("nan"))


class PerspectiveTriangulation:
    """The dense half of PerspectiveTriangulation: tracks [n, images_count, 2] int32, (-1, -1) = no point."""

    def __init__(self, images_count: int, image_shapes, bundle_adjustment: bool = True):
        """image_shapes: (width, height) per image (image_shapes, :604-617)."""
        self.images_count = int(images_count)
        self.image_shapes = [tuple(int(v) for v in s) for s in image_shapes]
        self.bundle_adjustment = bool(bundle_adjustment)
        self.tracks = np.full((0, self.images_count, 2), -1, dtype=np.int32)

    def add_image_pair_dense(self, image1_index: int, image2_index: int, pc):
        """extend_tracks (:1330-1419) with the completed grid of a pair's PointCorrelations `pc`: every track with a point
        in image 1 gets the nearest match - Track::add only fills an empty slot (:370-375) - and every remaining match
        becomes a new track, appended in scan order."""
        max_dimension = max(self.image_shapes[image2_index])
        tp2, new_p1, new_p2 = pc.extend_tracks(self.tracks[:, image1_index], max_dimension)
        fill = (self.tracks[:, image2_index, 0] < 0) & (tp2[:, 0] >= 0)
        self.tracks[fill, image2_index] = tp2[fill]
        new = np.full((len(new_p1), self.images_count, 2), -1, dtype=np.int32)
        new[:, image1_index] = new_p1.astype(np.int32)
        new[:, image2_index] = new_p2.astype(np.int32)
        self.tracks = np.concatenate([self.tracks, new])

    def prune_projections(self, cameras):
        """prune_projections (:913-938): images without a camera are dropped and the track columns remapped (kept in
        order).  -> (cameras, tracks) of the remaining images."""
        keep = [i for i, cam in enumerate(cameras) if cam is not None]
        return [cameras[i] for i in keep], np.ascontiguousarray(self.tracks[:, keep])

    def triangulate_all(self, device, cameras, progress=None) -> Surface:
        """triangulate_all (:817-865) with the given cameras [(K, R, t)] (None = no camera for that image).  max_points
        (a random subset in the reference) stays with the caller.  Raises CvhipError with the reference's
        TriangulationError message (CVHIP_ERR_NO_SURFACE) when the bundle adjustment fails."""
        cams, tracks = self.prune_projections(cameras)
        m = len(cams)
        n = len(tracks)
        K = np.ascontiguousarray(np.stack([np.asarray(c[0], dtype=np.float64).reshape(9) for c in cams]))
        R = np.ascontiguousarray(np.stack([np.asarray(c[1], dtype=np.float64).reshape(9) for c in cams]))
        t = np.ascontiguousarray(np.stack([np.asarray(c[2], dtype=np.float64).reshape(3) for c in cams]))
        pts = np.zeros((max(n, 1), 3), dtype=np.float64)
        idx = np.zeros(max(n, 1), dtype=np.uint64)
        out_r = np.zeros((m, 3))
        out_t = np.zeros((m, 3))
        out_p = np.zeros((m, 3, 4))
        out_n = C.c_uint64(0)
        iters = C.c_uint32(0)
        history = np.zeros(BUNDLE_ADJUSTMENT_MAX_ITERATIONS, dtype=np.uint8)
        norms = np.zeros(2)
        cb = _lib.PROGRESS_FN(lambda _user, pos: progress(pos)) if progress is not None else _lib.NULL_PROGRESS
        p = lambda a: C.c_void_p(a.ctypes.data)  # noqa: E731
        _lib.check(_lib.lib().cvhip_triangulate_perspective(
            device.handle, p(tracks) if n else None, n, m, p(K), p(R), p(t), int(self.bundle_adjustment), p(pts), p(idx),
            p(out_r), p(out_t), p(out_p), C.byref(out_n), C.byref(iters), p(history), p(norms), cb, None),
            "cvhip_triangulate_perspective")
        k = out_n.value
        index = idx[:k].astype(np.int64)
        return Surface(points=pts[:k].copy(), track_index=index, tracks=tracks[index],
                       cameras=[Camera(out_r[j].copy(), out_t[j].copy(), out_p[j].copy()) for j in range(m)],
                       ba_iterations=int(iters.value), ba_history=[int(h) for h in history[:iters.value]],
                       ba_residual_norms=(float(norms[0]), float(norms[1])))
