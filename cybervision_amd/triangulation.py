"""PerspectiveTriangulation (src/triangulation.rs:604-1593) over the C ABI: the dense track table that
extend_tracks builds pair by pair, and triangulate_all (:817-865) - DLT points, filter_outliers and the bundle
adjustment - in one call of cvhip_triangulate_perspective - and the sparse half that recovers the cameras
(add_image_pair_sparse, recover_next_cameras, :620-811): find_projection_matrix, triangulate_tracks and the P3P RANSAC of
recover_pose run on the device - and merge_tracks (:1421-1540, cvhip_merge_tracks), which reconstruct_dense runs after
each linked image's pairs.  `subset` is triangulate_all's max_points (:837-843, cvhip_surface_subset): a seeded random subset
of a surface's rows, selected and gathered on the device.
`DeviceTrackTable` is the dense table in device memory (cvhip_tracks): with resident_tracks=True the table
stays there from extend_tracks to the surface, whose points and tracks are device tensors.
`affine_surface` is the Surface of AffineTriangulation::triangulate (:268-330) around cvhip_triangulate_affine's points.
No compute in Python - the track table's bookkeeping and the calls only.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass, field

import numpy as np

from . import _lib

MAX_CAMERAS = 8  # CVHIP_TRIANGULATE_MAX_CAMERAS
BUNDLE_ADJUSTMENT_MAX_ITERATIONS = 100  # triangulation.rs:15
SUBSET_WG_ROWS = 1024      # CVHIP_SUBSET_WG_ROWS: rows of one workgroup trip of the subset's selection kernels
SUBSET_GRID_ROWS = 524288  # CVHIP_SUBSET_GRID_ROWS: rows of one trip of their whole grid


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
    reject (0) per iteration, |residual| before and after; NaN without bundle adjustment).  points and tracks are numpy
    arrays, or - from a resident track table - device tensors; track_index is always a host array."""
    points: np.ndarray
    track_index: np.ndarray
    tracks: np.ndarray
    cameras: list
    ba_iterations: int = 0
    ba_history: list = field(default_factory=list)
    ba_residual_norms: tuple = (float("nan"), float("nan"))


def affine_surface(points3d, p2) -> Surface:
    """The Surface that AffineTriangulation::triangulate returns (triangulation.rs:268-330) around the rows of
    PointCorrelations.triangulate_affine: `points` are the rows as given ((x, y, depth), x and y the pixel of image 1),
    track_index = arange, tracks [n, 2, 2] hold (x, y) of image 1 and the match `p2` in image 2, and both images get the
    reference's affine camera (:287-292): K = diag(1, 1, 0), R = I, t = 0, so r = t = 0 and the projection is
    [[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 0, 0]] - a point projects to (x, y) exactly and its depth is z.  The mesh stage
    (mesh.create, mesh.depth_image, mesh.ply, mesh.obj) takes it like any other surface."""
    pts = np.ascontiguousarray(points3d, dtype=np.float64).reshape(-1, 3)
    m2 = np.asarray(p2).reshape(-1, 2)
    if len(m2) != len(pts):
        raise ValueError("one image-2 point per 3D point")
    tracks = np.empty((len(pts), 2, 2), dtype=np.int32)
    tracks[:, 0] = pts[:, :2]  # (integer pixels: the conversion is exact)
    tracks[:, 1] = m2
    projection = np.zeros((3, 4))
    projection[0, 0] = projection[1, 1] = 1.0
    return Surface(points=pts, track_index=np.arange(len(pts), dtype=np.int64), tracks=tracks,
                   cameras=[Camera(np.zeros(3), np.zeros(3), projection.copy()) for _ in range(2)])


def _array_ptr(a):
    """The address of a numpy array or a device tensor (None stays NULL)."""
    if a is None:
        return None
    return C.c_void_p(a.data_ptr() if hasattr(a, "data_ptr") else a.ctypes.data)


def _empty_like_rows(a, rows: int):
    """Room for `rows` rows of `a`, where `a` lives: a numpy array, or a tensor on a's device."""
    shape = (max(int(rows), 1), *a.shape[1:])
    if hasattr(a, "data_ptr"):
        import torch

        return torch.empty(shape, dtype=a.dtype, device=a.device)
    return np.empty(shape, dtype=a.dtype)


def select_smallest(device, keys, m: int):
    """The rows of the m smallest (key, row) pairs of the uint64 `keys` - of equal keys the lower row -, ascending
    (cvhip_select_smallest_u64: a radix select and a stable compaction on the device).  keys: a numpy array, or
    a device tensor of 64-bit integers (its bits are the keys).  -> [min(n, m)] uint64."""
    if not hasattr(keys, "data_ptr"):
        keys = np.ascontiguousarray(keys, dtype=np.uint64).reshape(-1)
    elif not keys.is_contiguous() or keys.element_size() != 8 or keys.dim() != 1:
        raise ValueError("keys: a contiguous one-dimensional tensor of 64-bit integers")
    n = int(keys.shape[0])
    rows = np.empty(max(min(n, int(m)), 1), dtype=np.uint64)
    out_n = C.c_uint64(0)
    _lib.check(_lib.lib().cvhip_select_smallest_u64(device.handle, _array_ptr(keys) if n else None, n, int(m), _array_ptr(rows),
                                                    C.byref(out_n)), "cvhip_select_smallest_u64")
    return rows[:out_n.value]


def subset(device, surface: Surface, max_points: int, seed: int = 0):
    """max_points (triangulation.rs:837-843) on the device (cvhip_surface_subset): the Surface of the
    max_points rows of `surface` with the smallest keys key(seed, row), in ascending row order - every row when max_points >=
    len(surface.points).  The kept set is distributed as the reference's shuffle + truncate; its order is the surface's, not a
    random one.  points, track_index and tracks are those of the kept rows (points and tracks gathered on the device; they may
    be numpy arrays or device tensors, the results live where they do); the cameras and the ba_* fields are carried over.
    Perspective surfaces and affine_surface's alike.
    -> (Surface, info): info = {rows_in, rows_out, seed, rows (the kept rows, [rows_out] uint64)}."""
    max_points, seed = int(max_points), int(seed)
    if max_points < 0 or not 0 <= seed < 1 << 64:
        raise ValueError("max_points >= 0 and a 64-bit seed")
    on_dev = hasattr(surface.points, "data_ptr")
    points = surface.points.contiguous() if on_dev else np.ascontiguousarray(surface.points, dtype=np.float64)
    tracks = (surface.tracks.contiguous() if hasattr(surface.tracks, "data_ptr")
              else np.ascontiguousarray(surface.tracks, dtype=np.int32))
    n = int(points.shape[0])
    if int(tracks.shape[0]) != n or len(surface.track_index) != n:
        raise ValueError("one track row and one track index per point")
    m_cams = int(tracks.shape[1])
    k = min(n, max_points)
    rows = np.empty(max(k, 1), dtype=np.uint64)
    out_points, out_tracks = _empty_like_rows(points, k), _empty_like_rows(tracks, k)
    out_n = C.c_uint64(0)
    _lib.check(_lib.lib().cvhip_surface_subset(device.handle, n, max_points, seed, _array_ptr(points), _array_ptr(tracks), m_cams,
                                               _array_ptr(rows), _array_ptr(out_points), _array_ptr(out_tracks), C.byref(out_n)),
               "cvhip_surface_subset")
    k = out_n.value
    rows = rows[:k]
    index = surface.track_index[rows.astype(np.int64)]
    out = Surface(points=out_points[:k], track_index=index, tracks=out_tracks[:k], cameras=surface.cameras,
                  ba_iterations=surface.ba_iterations, ba_history=surface.ba_history, ba_residual_norms=surface.ba_residual_norms)
    return out, {"rows_in": n, "rows_out": k, "seed": seed, "rows": rows}


def _device_tensor(device, shape, dtype):
    """An uninitialised tensor on the GPU of the handle `device` (what the library writes a device output into)."""
    import torch

    ordinal = int(getattr(device, "ordinal", -1))
    return torch.empty(shape, dtype=dtype, device=torch.device("cuda", ordinal) if ordinal >= 0 else "cuda")


class DeviceTrackTable:
    """The dense track table in device memory (cvhip_tracks): [rows, m, 2] int32, (-1, -1) = no point, owned
    by a handle of the library - the table the existing entries take through `data_ptr`.  It belongs to `device`, works on its
    stream and is closed before it.  data_ptr is valid until the next call that changes the table (assign, extend, merge,
    close); a call that raises leaves the table as it was.  No arithmetic here: every method is one entry of the library."""

    def __init__(self, device, m: int, reserve_rows: int = 0, _handle=None):
        self.device = device
        self._h = C.c_void_p()
        if _handle is not None:
            self._h = _handle
        else:
            _lib.check(_lib.lib().cvhip_tracks_create(device.handle, int(m), int(reserve_rows), C.byref(self._h)),
                       "cvhip_tracks_create")

    def _info(self):
        rows, cap, m, ptr = C.c_uint64(0), C.c_uint64(0), C.c_uint32(0), C.c_void_p()
        _lib.check(_lib.lib().cvhip_tracks_info(self._h, C.byref(rows), C.byref(cap), C.byref(m), C.byref(ptr)), "cvhip_tracks_info")
        return int(rows.value), int(cap.value), int(m.value), int(ptr.value or 0)

    @property
    def handle(self):
        return self._h

    @property
    def rows(self) -> int:
        return self._info()[0]

    @property
    def capacity(self) -> int:
        return self._info()[1]

    @property
    def m(self) -> int:
        return self._info()[2]

    @property
    def data_ptr(self) -> int:
        """The device address of row 0 (0 while the table has no capacity)."""
        return self._info()[3]

    def __len__(self) -> int:
        return self.rows

    def numpy(self, first: int = 0, n=None) -> np.ndarray:
        """Rows [first, first + n) (to the last row by default) as a host array [n, m, 2] int32."""
        rows, _cap, m, _ptr = self._info()
        n = rows - int(first) if n is None else int(n)
        out = np.empty((max(n, 0), m, 2), dtype=np.int32)
        _lib.check(_lib.lib().cvhip_tracks_read(self._h, int(first), n, _array_ptr(out) if out.size else None), "cvhip_tracks_read")
        return out

    def assign(self, rows):
        """The table becomes `rows`: a numpy array or a contiguous int32 device tensor, [n, m, 2]."""
        if not hasattr(rows, "data_ptr"):
            rows = np.ascontiguousarray(rows, dtype=np.int32)
        elif not rows.is_contiguous():
            raise ValueError("rows: a contiguous tensor")
        if rows.ndim != 3 or tuple(rows.shape[1:]) != (self.m, 2):
            raise ValueError("rows: [n, m, 2]")
        n = int(rows.shape[0])
        _lib.check(_lib.lib().cvhip_tracks_assign(self._h, _array_ptr(rows) if n else None, n), "cvhip_tracks_assign")

    def extend(self, pc, image1_index: int, image2_index: int, max_dimension: int) -> dict:
        """extend_tracks (triangulation.rs:1330-1419) with the grid of the pair's PointCorrelations `pc`, fill rule and append
        included (cvhip_tracks_extend) -> {matched, filled, appended}."""
        counts = np.zeros(3, dtype=np.uint64)
        _lib.check(_lib.lib().cvhip_tracks_extend(self._h, pc._h, int(image1_index), int(image2_index), int(max_dimension),
                                                  _array_ptr(counts)), "cvhip_tracks_extend")
        return {"matched": int(counts[0]), "filled": int(counts[1]), "appended": int(counts[2])}

    def merge(self, image_index: int, width: int, height: int) -> dict:
        """merge_tracks for image `image_index` of width x height (cvhip_tracks_merge) -> PerspectiveTriangulation.merge_tracks'
        dict."""
        n = self.rows
        stats = np.zeros(4, dtype=np.uint64)
        _lib.check(_lib.lib().cvhip_tracks_merge(self._h, int(image_index), int(width), int(height), _array_ptr(stats)),
                   "cvhip_tracks_merge")
        return {"image": int(image_index), "rows_in": n, "rows_out": self.rows, "present": int(stats[0]), "cells": int(stats[1]),
                "rejected": int(stats[2]), "empty_area": int(stats[3])}

    def select_columns(self, columns) -> "DeviceTrackTable":
        """A new table of the listed columns (strictly increasing) of every row (prune_projections, :913-938)."""
        cols = np.ascontiguousarray(columns, dtype=np.uint32).reshape(-1)
        out = C.c_void_p()
        _lib.check(_lib.lib().cvhip_tracks_select_columns(self._h, _array_ptr(cols) if len(cols) else None, len(cols), C.byref(out)),
                   "cvhip_tracks_select_columns")
        return DeviceTrackTable(self.device, len(cols), _handle=out)

    def gather(self, rows, out=None):
        """out[j] = row rows[j].  rows: a numpy array or a contiguous device tensor of 64-bit integers; out: a numpy array or a
        contiguous int32 device tensor [k, m, 2] (by default a device tensor).  -> out."""
        if not hasattr(rows, "data_ptr"):
            rows = np.ascontiguousarray(rows, dtype=np.uint64).reshape(-1)
        elif not rows.is_contiguous() or rows.element_size() != 8 or rows.dim() != 1:
            raise ValueError("rows: a contiguous one-dimensional tensor of 64-bit integers")
        k = int(rows.shape[0])
        if out is None:
            import torch

            out = _device_tensor(self.device, (k, self.m, 2), torch.int32)
        elif (hasattr(out, "data_ptr") and not out.is_contiguous()) or tuple(out.shape) != (k, self.m, 2):
            raise ValueError("out: contiguous, [k, m, 2]")
        _lib.check(_lib.lib().cvhip_tracks_gather(self._h, _array_ptr(rows) if k else None, k, _array_ptr(out) if k else None),
                   "cvhip_tracks_gather")
        return out

    def close(self):
        if getattr(self, "_h", None):
            _lib.lib().cvhip_tracks_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class PerspectiveTriangulation:
    """PerspectiveTriangulation: tracks [n, images_count, 2] int32, (-1, -1) = no point; the sparse half places the cameras.
    resident_tracks=True: after complete_sparse_triangulation the dense table is a DeviceTrackTable - add_image_pair_dense,
    merge_tracks and triangulate_all[_recovered] work on it in device memory (they take the device handle then), and the
    Surface's points and tracks are device tensors.  The sparse half keeps its host table."""

    def __init__(self, images_count: int, image_shapes, bundle_adjustment: bool = True, calibration=None,
                 resident_tracks: bool = False):
        """image_shapes: (width, height) per image; calibration: K per image (set_image_data, :604-617, 700-703)."""
        self.images_count = int(images_count)
        self.image_shapes = [tuple(int(v) for v in s) for s in image_shapes]
        self.bundle_adjustment = bool(bundle_adjustment)
        self.resident_tracks = bool(resident_tracks)
        self.tracks = np.full((0, self.images_count, 2), -1, dtype=np.int32)
        n = self.images_count
        self.calibration = [None if calibration is None else np.ascontiguousarray(calibration[i], dtype=np.float64)
                            for i in range(n)]
        self.projections = [None] * n   # 3 x 4, calibrated
        self.cameras = [None] * n       # (K, r, t) per placed image: the Camera as the reference holds it
        self.points = np.zeros((0, 3))  # point3d of every track (valid where points_ok)
        self.points_ok = np.zeros(0, dtype=bool)
        self.best_initial_p2 = None
        self.best_initial_r2 = None     # Camera::from_matrix's r of best_initial_p2's rotation
        self.best_initial_kp2 = None    # k2 * best_initial_p2, as the library computed it
        self.best_initial_score = None
        self.best_initial_pair = None
        self.remaining_images = list(range(n))
        self.last_pose = None           # what the last recover_pose call returned (count, error, batches)

    # ---- sparse half ---------------------------------------------------------------------------------------------------
    def _extend_tracks_matches(self, device, image1_index, image2_index, inliers):
        """extend_tracks (:1330-1419) with add_image_pair_sparse's inlier grid (:628-638), on the device."""
        inl = np.ascontiguousarray(np.asarray(inliers, dtype=np.uint32).reshape(-1, 4))
        w1, h1 = self.image_shapes[image1_index]
        max_dimension = max(self.image_shapes[image2_index])
        tp1 = np.ascontiguousarray(self.tracks[:, image1_index])
        n = len(tp1)
        tp2 = np.full((max(n, 1), 2), -1, dtype=np.int32)
        cap = max(len(inl), 1)
        new_p1 = np.zeros((cap, 2), dtype=np.uint32)
        new_p2 = np.zeros((cap, 2), dtype=np.uint32)
        n_new = C.c_uint64(0)
        p = lambda a: C.c_void_p(a.ctypes.data)  # noqa: E731
        _lib.check(_lib.lib().cvhip_extend_tracks_matches(device.handle, p(inl), len(inl), w1, h1, p(tp1) if n else None, n,
                                                          max_dimension, p(tp2) if n else None, p(new_p1), p(new_p2), cap,
                                                          C.byref(n_new)), "cvhip_extend_tracks_matches")
        tp2 = tp2[:n]
        fill = (self.tracks[:, image2_index, 0] < 0) & (tp2[:, 0] >= 0)
        self.tracks[fill, image2_index] = tp2[fill]
        k = n_new.value
        new = np.full((k, self.images_count, 2), -1, dtype=np.int32)
        new[:, image1_index] = new_p1[:k].astype(np.int32)
        new[:, image2_index] = new_p2[:k].astype(np.int32)
        self.tracks = np.concatenate([self.tracks, new])
        self.points = np.concatenate([self.points, np.zeros((k, 3))])
        self.points_ok = np.concatenate([self.points_ok, np.zeros(k, dtype=bool)])

    def add_image_pair_sparse(self, device, image1_index: int, image2_index: int, f, inliers):
        """add_image_pair_sparse (:620-688): extend_tracks with the inliers ([k, 4] x1, y1, x2, y2), then
        find_projection_matrix over the tracks seen in both images; the first pair with a strictly higher score becomes the
        initial pair.  -> (p2 [3, 4] = [r | t], score)."""
        self._extend_tracks_matches(device, image1_index, image2_index, inliers)  # (before the calibration check, :628-655)
        k1, k2 = self.calibration[image1_index], self.calibration[image2_index]
        if k1 is None or k2 is None:
            raise _lib.CvhipError(-1, "add_image_pair_sparse", "Missing calibration matrix")
        both = (self.tracks[:, image1_index, 0] >= 0) & (self.tracks[:, image2_index, 0] >= 0)
        short = np.ascontiguousarray(self.tracks[both][:, [image1_index, image2_index]])
        self.last_short = short
        p2, r2, kp2 = np.zeros((3, 4)), np.zeros(3), np.zeros((3, 4))
        score = C.c_double(0.0)
        p = lambda a: C.c_void_p(a.ctypes.data)  # noqa: E731
        F = np.ascontiguousarray(f, dtype=np.float64)
        _lib.check(_lib.lib().cvhip_find_projection_matrix(device.handle, p(F), p(k1), p(k2), p(short) if len(short) else None,
                                                           len(short), p(p2), C.byref(score), p(r2), p(kp2)),
                   "cvhip_find_projection_matrix")
        if self.best_initial_score is None or score.value > self.best_initial_score:
            self.best_initial_p2 = p2
            self.best_initial_r2 = r2
            self.best_initial_kp2 = kp2
            self.best_initial_pair = (image1_index, image2_index)
            self.best_initial_score = score.value
        return p2, score.value

    def triangulate_tracks(self, device):
        """triangulate_tracks (:905-911): every track's point from the images that have a projection (device)."""
        n, m = len(self.tracks), self.images_count
        has = np.array([pr is not None for pr in self.projections], dtype=np.uint8)
        P = np.ascontiguousarray(np.stack([pr if pr is not None else np.zeros((3, 4)) for pr in self.projections]))
        pts = np.zeros((max(n, 1), 3))
        ok = np.zeros(max(n, 1), dtype=np.uint8)
        p = lambda a: C.c_void_p(a.ctypes.data)  # noqa: E731
        tr = np.ascontiguousarray(self.tracks)
        _lib.check(_lib.lib().cvhip_triangulate_tracks(device.handle, p(tr) if n else None, n, m, p(P), p(has),
                                                       p(pts) if n else None, p(ok) if n else None),
                   "cvhip_triangulate_tracks")
        self.points, self.points_ok = pts[:n], ok[:n].astype(bool)

    def recover_next_cameras(self, device, seed: int = 0, progress=None):
        """recover_next_cameras (:710-811) -> the images whose cameras were placed ([] when none is left).  The first call
        places the initial pair (camera 1 at the origin, camera 2 from best_initial_p2); every later call takes the
        remaining image seen by the most triangulated tracks - max_by_key keeps the LAST of equal counts - and runs
        recover_pose for it; the tracks are re-triangulated after every placed camera.  Raises CvhipError
        (CVHIP_ERR_NO_SURFACE, "Unable to find projection matrix") when recover_pose fails; that image stays unplaced."""
        self.last_pose = None
        if self.best_initial_pair is not None:
            i1, i2 = self.best_initial_pair
            k1, k2 = self.calibration[i1], self.calibration[i2]
            p2 = self.best_initial_p2
            # camera1 = from_matrix(k1, I, 0): r = 0, p1 = k1 [I | 0]; camera2 = from_matrix(k2, p2[:, :3], p2[:, 3]), whose r
            # and k2 p2 cvhip_find_projection_matrix returned (:720-752); k1 [I | 0] is k1 next to a zero column, no arithmetic
            self.projections[i1] = np.hstack([k1, np.zeros((3, 1))])
            self.cameras[i1] = (k1, np.zeros(3), np.zeros(3))
            self.projections[i2] = self.best_initial_kp2.copy()
            self.cameras[i2] = (k2, self.best_initial_r2.copy(), p2[:, 3].copy())
            self.triangulate_tracks(device)
            self.remaining_images = [i for i in self.remaining_images if i not in (i1, i2)]
            self.best_initial_pair = None
            return [i1, i2]
        seen = self.tracks[..., 0] >= 0
        linked = self.points_ok & seen[:, self.remaining_images].any(axis=1) if self.remaining_images else self.points_ok
        counts = {i: int((linked & seen[:, i]).sum()) for i in self.remaining_images}
        if not self.remaining_images:
            return []
        best = self.remaining_images[0]
        for i in self.remaining_images:  # max_by_key: the last maximum
            if counts[i] >= counts[best]:
                best = i
        self.remaining_images = [i for i in self.remaining_images if i != best]
        K = self.calibration[best]
        n, m = len(self.tracks), self.images_count
        has = np.array([pr is not None for pr in self.projections], dtype=np.uint8)
        P = np.ascontiguousarray(np.stack([pr if pr is not None else np.zeros((3, 4)) for pr in self.projections]))
        r, t, proj = np.zeros(3), np.zeros(3), np.zeros((3, 4))
        cnt, err, batches = C.c_uint32(0), C.c_double(0.0), C.c_uint32(0)
        winner = np.full(3, -1, dtype=np.int32)
        cb = _lib.PROGRESS_FN(lambda _user, pos: progress(pos)) if progress is not None else _lib.NULL_PROGRESS
        p = lambda a: C.c_void_p(a.ctypes.data)  # noqa: E731
        tr = np.ascontiguousarray(self.tracks)
        pts = np.ascontiguousarray(self.points)
        ok = np.ascontiguousarray(self.points_ok.astype(np.uint8))
        rc = _lib.lib().cvhip_recover_pose(device.handle, p(tr) if n else None, n, m, p(pts) if n else None,
                                           p(ok) if n else None, p(P), p(has), best, p(np.ascontiguousarray(K)),
                                           max(self.image_shapes[best]), int(seed), p(r), p(t), p(proj), C.byref(cnt),
                                           C.byref(err), C.byref(batches), p(winner), cb, None)
        self.last_pose = {"image": best, "count": int(cnt.value), "error": float(err.value), "batches": int(batches.value),
                          "linked": counts[best], "winner": tuple(int(v) for v in winner), "r": r.copy(), "t": t.copy(),
                          "projection": proj.copy()}
        _lib.check(rc, "cvhip_recover_pose")
        self.cameras[best] = (K, r, t)
        self.projections[best] = proj
        self.triangulate_tracks(device)
        return [best]

    def complete_sparse_triangulation(self, device=None):
        """complete_sparse_triangulation (:813-815): the tracks go, the cameras stay.  With resident_tracks the dense table
        that takes their place is a DeviceTrackTable of `device` (without a device here, the first dense call makes it)."""
        self.tracks = np.full((0, self.images_count, 2), -1, dtype=np.int32)
        self.points = np.zeros((0, 3))
        self.points_ok = np.zeros(0, dtype=bool)
        if self.resident_tracks and device is not None:
            self._resident_table(device)

    def _resident_table(self, device) -> DeviceTrackTable:
        """The dense table in device memory: made on first use, from the rows the host table holds then."""
        if not isinstance(self.tracks, DeviceTrackTable):
            table = DeviceTrackTable(device, self.images_count)
            if len(self.tracks):
                table.assign(self.tracks)
            self.tracks = table
        return self.tracks

    def _triangulate_resident(self, device, keep, call) -> Surface:
        """triangulate_all on the resident table: the kept columns selected on the device, the entry `call(tracks pointer, n,
        m, outputs...)` run on the table's device rows with device outputs, and the survivors' rows gathered on the device.
        The Surface's points and tracks are device tensors.  track_index stays a host array: it is bookkeeping that no kernel
        reads, and the one n_kept x 8 B array that still comes down."""
        import torch

        sel = self._resident_table(device).select_columns(keep)
        try:
            m, n = len(keep), sel.rows
            pts = _device_tensor(device, (max(n, 1), 3), torch.float64)
            idx = _device_tensor(device, (max(n, 1),), torch.int64)  # (the entry's uint64 rows: below 2^32)
            out_r, out_t, out_p = np.zeros((m, 3)), np.zeros((m, 3)), np.zeros((m, 3, 4))
            out_n, iters = C.c_uint64(0), C.c_uint32(0)
            history = np.zeros(BUNDLE_ADJUSTMENT_MAX_ITERATIONS, dtype=np.uint8)
            norms = np.zeros(2)
            p = lambda a: C.c_void_p(a.ctypes.data)  # noqa: E731
            call(C.c_void_p(sel.data_ptr) if n else None, n, m, _array_ptr(pts), _array_ptr(idx), p(out_r), p(out_t), p(out_p),
                 C.byref(out_n), C.byref(iters), p(history), p(norms))
            k = out_n.value
            index = idx[:k]
            tracks = sel.gather(index)
            return Surface(points=pts[:k], track_index=index.cpu().numpy(), tracks=tracks,
                           cameras=[Camera(out_r[j].copy(), out_t[j].copy(), out_p[j].copy()) for j in range(m)],
                           ba_iterations=int(iters.value), ba_history=[int(h) for h in history[:iters.value]],
                           ba_residual_norms=(float(norms[0]), float(norms[1])))
        finally:
            sel.close()

    def triangulate_all_recovered(self, device, progress=None) -> Surface:
        """triangulate_all (:817-865) with the recovered cameras and projections (cvhip_triangulate_perspective_cameras);
        images without a camera are pruned (prune_projections, :913-938).  With resident_tracks: _triangulate_resident."""
        keep = [i for i in range(self.images_count) if self.projections[i] is not None]
        if self.resident_tracks:
            K = np.ascontiguousarray(np.stack([self.cameras[i][0].reshape(9) for i in keep]))
            R = np.ascontiguousarray(np.stack([self.cameras[i][1].reshape(3) for i in keep]))
            t = np.ascontiguousarray(np.stack([self.cameras[i][2].reshape(3) for i in keep]))
            P = np.ascontiguousarray(np.stack([self.projections[i] for i in keep]))
            cb = _lib.PROGRESS_FN(lambda _user, pos: progress(pos)) if progress is not None else _lib.NULL_PROGRESS
            a = lambda v: C.c_void_p(v.ctypes.data)  # noqa: E731
            return self._triangulate_resident(device, keep, lambda tracks, n, m, *outs: _lib.check(
                _lib.lib().cvhip_triangulate_perspective_cameras(device.handle, tracks, n, m, a(K), a(R), a(t), a(P),
                                                                 int(self.bundle_adjustment), *outs, cb, None),
                "cvhip_triangulate_perspective_cameras"))
        tracks = np.ascontiguousarray(self.tracks[:, keep])
        m, n = len(keep), len(tracks)
        K = np.ascontiguousarray(np.stack([self.cameras[i][0].reshape(9) for i in keep]))
        R = np.ascontiguousarray(np.stack([self.cameras[i][1].reshape(3) for i in keep]))
        t = np.ascontiguousarray(np.stack([self.cameras[i][2].reshape(3) for i in keep]))
        P = np.ascontiguousarray(np.stack([self.projections[i] for i in keep]))
        pts = np.zeros((max(n, 1), 3), dtype=np.float64)
        idx = np.zeros(max(n, 1), dtype=np.uint64)
        out_r, out_t, out_p = np.zeros((m, 3)), np.zeros((m, 3)), np.zeros((m, 3, 4))
        out_n, iters = C.c_uint64(0), C.c_uint32(0)
        history = np.zeros(BUNDLE_ADJUSTMENT_MAX_ITERATIONS, dtype=np.uint8)
        norms = np.zeros(2)
        cb = _lib.PROGRESS_FN(lambda _user, pos: progress(pos)) if progress is not None else _lib.NULL_PROGRESS
        p = lambda a: C.c_void_p(a.ctypes.data)  # noqa: E731
        _lib.check(_lib.lib().cvhip_triangulate_perspective_cameras(
            device.handle, p(tracks) if n else None, n, m, p(K), p(R), p(t), p(P), int(self.bundle_adjustment), p(pts),
            p(idx), p(out_r), p(out_t), p(out_p), C.byref(out_n), C.byref(iters), p(history), p(norms), cb, None),
            "cvhip_triangulate_perspective_cameras")
        k = out_n.value
        index = idx[:k].astype(np.int64)
        return Surface(points=pts[:k].copy(), track_index=index, tracks=tracks[index],
                       cameras=[Camera(out_r[j].copy(), out_t[j].copy(), out_p[j].copy()) for j in range(m)],
                       ba_iterations=int(iters.value), ba_history=[int(h) for h in history[:iters.value]],
                       ba_residual_norms=(float(norms[0]), float(norms[1])))

    def add_image_pair_dense(self, image1_index: int, image2_index: int, pc):
        """extend_tracks (:1330-1419) with the completed grid of a pair's PointCorrelations `pc`: every track with a point
        in image 1 gets the nearest match - Track::add only fills an empty slot (:370-375) - and every remaining match
        becomes a new track, appended in scan order.  With resident_tracks all of it is one call on the table in device
        memory (DeviceTrackTable.extend, on pc's device), whose counts it returns."""
        max_dimension = max(self.image_shapes[image2_index])
        if self.resident_tracks:
            return self._resident_table(pc.device).extend(pc, image1_index, image2_index, max_dimension)
        tp2, new_p1, new_p2 = pc.extend_tracks(self.tracks[:, image1_index], max_dimension)
        fill = (self.tracks[:, image2_index, 0] < 0) & (tp2[:, 0] >= 0)
        self.tracks[fill, image2_index] = tp2[fill]
        new = np.full((len(new_p1), self.images_count, 2), -1, dtype=np.int32)
        new[:, image1_index] = new_p1.astype(np.int32)
        new[:, image2_index] = new_p2.astype(np.int32)
        self.tracks = np.concatenate([self.tracks, new])

    def merge_tracks(self, device, image_index: int) -> dict:
        """merge_tracks (:1421-1540) for image `image_index` on the device (cvhip_merge_tracks): the table
        becomes one copy of the highest row of every kept cell of that image, in row-major order of the cells; tracks
        without a point in the image are dropped.  The trailing triangulate_tracks (:1538) is not run: triangulate_all
        re-triangulates every track first (:822), and the dense stage keeps no points (`self.points` stays as it is).
        -> {image, rows_in, rows_out, present, cells, rejected, empty_area}.  With resident_tracks the table is merged in
        device memory (DeviceTrackTable.merge): the same dict."""
        n, m = len(self.tracks), self.images_count
        w, h = self.image_shapes[image_index]
        if self.resident_tracks:
            return self._resident_table(device).merge(image_index, w, h)
        tr = np.ascontiguousarray(self.tracks)
        out = np.empty((max(n, 1), m, 2), dtype=np.int32)
        out_n = C.c_uint64(0)
        stats = np.zeros(4, dtype=np.uint64)
        p = lambda a: C.c_void_p(a.ctypes.data)  # noqa: E731
        _lib.check(_lib.lib().cvhip_merge_tracks(device.handle, p(tr) if n else None, n, m, int(image_index), w, h, None,
                                                 p(out), C.byref(out_n), p(stats)), "cvhip_merge_tracks")
        k = out_n.value
        self.tracks = out[:k]
        return {"image": int(image_index), "rows_in": n, "rows_out": k, "present": int(stats[0]), "cells": int(stats[1]),
                "rejected": int(stats[2]), "empty_area": int(stats[3])}

    def prune_projections(self, cameras):
        """prune_projections (:913-938): images without a camera are dropped and the track columns remapped (kept in
        order).  -> (cameras, tracks) of the remaining images."""
        keep = [i for i, cam in enumerate(cameras) if cam is not None]
        return [cameras[i] for i in keep], np.ascontiguousarray(self.tracks[:, keep])

    def triangulate_all(self, device, cameras, progress=None) -> Surface:
        """triangulate_all (:817-865) with the given cameras [(K, R, t)] (None = no camera for that image).  max_points
        (:837-843, a random subset) is `subset`, applied to the surface this returns.  Raises CvhipError with the reference's
        TriangulationError message (CVHIP_ERR_NO_SURFACE) when the bundle adjustment fails.  With resident_tracks:
        _triangulate_resident."""
        if self.resident_tracks:
            keep = [i for i, cam in enumerate(cameras) if cam is not None]
            K = np.ascontiguousarray(np.stack([np.asarray(cameras[i][0], dtype=np.float64).reshape(9) for i in keep]))
            R = np.ascontiguousarray(np.stack([np.asarray(cameras[i][1], dtype=np.float64).reshape(9) for i in keep]))
            t = np.ascontiguousarray(np.stack([np.asarray(cameras[i][2], dtype=np.float64).reshape(3) for i in keep]))
            cb = _lib.PROGRESS_FN(lambda _user, pos: progress(pos)) if progress is not None else _lib.NULL_PROGRESS
            a = lambda v: C.c_void_p(v.ctypes.data)  # noqa: E731
            return self._triangulate_resident(device, keep, lambda tracks, n, m, *outs: _lib.check(
                _lib.lib().cvhip_triangulate_perspective(device.handle, tracks, n, m, a(K), a(R), a(t), int(self.bundle_adjustment),
                                                         *outs, cb, None), "cvhip_triangulate_perspective"))
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
