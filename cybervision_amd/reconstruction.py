"""The hot-path calls of ImageReconstruction (src/reconstruction.rs) in the order the reference makes them,
over the C ABI: match_keypoints (:400-500: per-level ORB on both images + KeypointMatching),
find_fundamental_matrix (:502-526), correlate_dense (:528-603) and the pair loops of reconstruct /
reconstruct_dense (:261-277, :680-730).  This is BASELINE config 5's workload ("3-image perspective SFM:
ORB + RANSAC F-matrix on GPU + pairwise dense correlation").  Everything between the calls that the
reference does on the CPU (image decode, Lanczos3 resize, triangulation, bundle adjustment) is outside
the boundary; images arrive here as prebuilt pyramids (pyr[k] = the 1/2^k level, host arrays or device
tensors).  No compute in Python - only the calls and their timing.
"""
from __future__ import annotations

import time

import numpy as np

from . import correlation, fundamentalmatrix, orb, pointmatching
from .fundamentalmatrix import ProjectionMode


class ImageReconstruction:
    def __init__(self, device, projection_mode: ProjectionMode = ProjectionMode.Perspective):
        self.device = device
        self.projection_mode = ProjectionMode(projection_mode)
        self.timings_ms: dict[str, float] = {}

    def _timed(self, key: str, fn):
        self.device.synchronize()
        t0 = time.perf_counter()
        out = fn()
        self.device.synchronize()
        self.timings_ms[key] = self.timings_ms.get(key, 0.0) + (time.perf_counter() - t0) * 1e3
        return out

    # reconstruction.rs:418-458 for ONE image: levels coarse to fine, coordinates mapped back, lists concatenated
    def extract_keypoints(self, pyramid):
        dims = (int(pyramid[0].shape[1]), int(pyramid[0].shape[0]))
        steps = orb.optimal_scale_steps(*dims)
        return self._timed("orb", lambda: orb.extract_points_multiscale(self.device, pyramid[:steps + 1]))

    # the same for every image of the set in ONE batched call (all levels of all images: cvhip_orb_extract_batch)
    def extract_keypoints_set(self, pyramids):
        trimmed = []
        for pyramid in pyramids:
            dims = (int(pyramid[0].shape[1]), int(pyramid[0].shape[0]))
            trimmed.append(pyramid[:orb.optimal_scale_steps(*dims) + 1])
        return self._timed("orb", lambda: orb.extract_points_multiscale_set(self.device, trimmed))

    # reconstruction.rs:400-500
    def match_keypoints(self, keypoints1, keypoints2):
        thr = (pointmatching.THRESHOLD_PERSPECTIVE if self.projection_mode == ProjectionMode.Perspective
               else pointmatching.THRESHOLD_AFFINE)
        m, _ = self._timed("match", lambda: pointmatching.match_points(self.device, keypoints1[0], keypoints1[1],
                                                                       keypoints2[0], keypoints2[1], thr))
        return m

    # reconstruction.rs:502-526
    def find_fundamental_matrix(self, img1_dimensions, img2_dimensions, point_matches, seed: int = 0, progress_listener=None):
        """progress_listener: the reference ALWAYS passes one (`Some(&pb)`, reconstruction.rs:510-518): an object with
        report_status(pos) / report_matches(count), both thunks of cvhip_find_ransac."""
        max_dimension = float(max(img1_dimensions[0], img1_dimensions[1], img2_dimensions[0], img2_dimensions[1]))
        fm = fundamentalmatrix.FundamentalMatrix(self.projection_mode, max_dimension)
        return self._timed("ransac", lambda: fm.find_ransac(self.device, point_matches, seed=seed, progress_listener=progress_listener))

    # reconstruction.rs:528-603 (up to complete(); triangulation is the next stage)
    def correlate_dense(self, pyr1, pyr2, f, out_xy=None, out_corr=None, borrow=False):
        """borrow: the pyramids are device tensors with 64 readable bytes behind every level and complete in memory
        (padded_pyramid below) - the library then uses them in place and computes their window statistics ahead of the
        levels' turn (cvhip_ctx_set_borrow_inputs / cvhip_ctx_set_stats_ahead)."""
        def dims(img):
            return (int(img.shape[1]), int(img.shape[0]))

        steps = correlation.optimal_scale_steps(*dims(pyr1[0]))
        mode = correlation.ProjectionMode(int(self.projection_mode))

        if out_xy is None and hasattr(pyr1[0], "data_ptr"):
            # device-resident pyramids: the grid stays in HBM too (the next stage - triangulation, track extension -
            # reads it there); a host copy is the caller's explicit choice (pass numpy outputs)
            import torch

            w, h = dims(pyr1[0])
            out_xy = torch.empty((h, w, 2), dtype=torch.int32, device=pyr1[0].device)
            out_corr = torch.empty((h, w), dtype=torch.float32, device=pyr1[0].device)

        def run():
            pc = correlation.PointCorrelations(self.device, dims(pyr1[0]), dims(pyr2[0]), f, mode)
            try:
                if borrow:
                    pc.set_borrow_inputs(True)
                    pc.set_stats_ahead(True)
                for i in range(steps + 1):
                    k = steps - i
                    pc.correlate_images(pyr1[k], pyr2[k], 1.0 / float(1 << k))
                return pc.complete(out_xy=out_xy, out_corr=out_corr)
            finally:
                pc.close()

        return self._timed("dense", run)


    def correlate_dense_set(self, jobs, borrow=False):
        """jobs: [(pyr1, pyr2, f)] - the pairs of reconstruct_dense's loop (reconstruction.rs:680-730), each a correlate_dense of
        its own -> [(xy, corr)].  The pairs are independent: with device-resident pyramids (borrow) every pair runs on a device
        handle - a stream - of its own, so that one pair's coarse levels (chains of small dependent launches that leave the
        chip idle) run under another pair's full-resolution levels.  Results are those of the calls one after the other."""
        if not borrow or len(jobs) < 2:
            return [self.correlate_dense(p1, p2, f, borrow=borrow) for p1, p2, f in jobs]
        import torch

        mode = correlation.ProjectionMode(int(self.projection_mode))
        devs = [self.device] + [self.device.side_handle(i) for i in range(len(jobs) - 1)]

        def dims(img):
            return (int(img.shape[1]), int(img.shape[0]))

        outs = []
        for p1, _, _ in jobs:
            w, h = dims(p1[0])
            outs.append((torch.empty((h, w, 2), dtype=torch.int32, device=p1[0].device),
                         torch.empty((h, w), dtype=torch.float32, device=p1[0].device)))
        torch.cuda.synchronize(jobs[0][0][0].device)  # (the outputs exist before a private stream writes them)

        def run():
            pcs = []
            try:
                for dev, (p1, p2, f) in zip(devs, jobs):
                    pc = correlation.PointCorrelations(dev, dims(p1[0]), dims(p2[0]), f, mode)
                    pcs.append(pc)
                    pc.set_borrow_inputs(True)
                    pc.set_stats_ahead(dev is self.device)  # (one statistics side stream: every further stream of the process
                    #                                          shares a hardware queue with one already in use)
                res = []
                for pc, (p1, p2, f), (oxy, ocorr) in zip(pcs, jobs, outs):
                    steps = correlation.optimal_scale_steps(*dims(p1[0]))
                    for i in range(steps + 1):
                        k = steps - i
                        pc.correlate_images(p1[k], p2[k], 1.0 / float(1 << k))
                    res.append(pc.complete(out_xy=oxy, out_corr=ocorr))
                for dev in devs:
                    dev.synchronize()
                return res
            finally:
                for pc in pcs:
                    pc.close()

        return self._timed("dense", run)


def padded_pyramid(pyr):
    """Device copies of a pyramid's levels with 64 readable bytes behind each (what cvhip_ctx_set_borrow_inputs asks
    for); host pyramids are returned as they are.  -> (pyramid, borrowable)."""
    if not hasattr(pyr[0], "data_ptr") or not pyr[0].is_cuda:
        return pyr, False
    import torch

    out = []
    for level in pyr:
        n = level.numel()
        buf = torch.zeros(n + 64, dtype=torch.uint8, device=level.device)
        buf[:n].copy_(level.reshape(-1))
        out.append(buf[:n].view(level.shape[0], level.shape[1]))
    torch.cuda.synchronize(pyr[0].device)  # complete in memory before any level is handed to the library
    return out, True


class ProgressBar:
    """Stand-in for the reference's indicatif bar (reconstruction.rs:840-863): both RANSAC thunks, nothing drawn."""

    def __init__(self):
        self.pos, self.matches, self.calls = 0.0, 0, 0

    def report_status(self, pos):
        self.pos = pos
        self.calls += 1

    def report_matches(self, count):
        self.matches = count
        self.calls += 1


def reconstruct_pairs(device, pyramids, projection_mode: ProjectionMode = ProjectionMode.Perspective, seed: int = 0,
                      dense: bool = True, borrow: bool = False, listener: bool = False, images=None, concurrent_pairs: bool = True):
    """The two pair loops of `reconstruct` (reconstruction.rs:261-277 sparse, :680-730 dense) over n images:
    for every i < j the sparse stage (ORB on both, matcher, RANSAC); then, for every pair that produced an F, the
    dense correlation.  The reference re-extracts an image's keypoints for every pair it takes part in; the result
    is a pure function of the image, so they are extracted once per image here.  concurrent_pairs (device-resident pyramids):
    the pairs' dense correlations - independent of each other - run side by side, each on a stream of its own
    (ImageReconstruction.correlate_dense_set); False: one after the other, as the reference's loop does.
    -> dict: keypoints [n], pairs {(i, j): {matches, f, inliers, (xy, corr)}}, timings_ms per stage."""
    rec = ImageReconstruction(device, projection_mode)
    if images is not None:
        # The reference's own pyramids: SourceImage::resize (Lanczos3, reconstruction.rs:146-162) per level, rebuilt by every
        # stage that needs them - match_keypoints for both images of a pair (:421-422; once per image here, like the
        # keypoints) and correlate_dense for both images of a pair (:567-568).  `pyramids` is ignored; the resizes run on the
        # device (cvhip_resize_lanczos3) and are timed as their own stage.
        pyramids = [rec._timed("resize", lambda im=im: correlation.lanczos_pyramid(
            device, im, orb.optimal_scale_steps(int(im.shape[1]), int(im.shape[0])))) for im in images]
    n = len(pyramids)
    keypoints = rec.extract_keypoints_set(pyramids)
    pairs = {}
    for i in range(n - 1):
        for j in range(i + 1, n):
            di = (int(pyramids[i][0].shape[1]), int(pyramids[i][0].shape[0]))
            dj = (int(pyramids[j][0].shape[1]), int(pyramids[j][0].shape[0]))
            matches = rec.match_keypoints(keypoints[i], keypoints[j])
            entry = {"matches": matches, "f": None, "inliers": None, "error": None}
            try:
                f, inliers, _ = rec.find_fundamental_matrix(di, dj, matches, seed=seed + 1000 * i + j,
                                                            progress_listener=ProgressBar() if listener else None)
                entry["f"], entry["inliers"] = f, inliers
            except Exception as exc:  # "Failed to match images" (reconstruction.rs:268-274): the pair is skipped
                entry["error"] = str(exc)
            pairs[(i, j)] = entry
    if dense and borrow and images is None and concurrent_pairs:
        todo = [(key, entry) for key, entry in pairs.items() if entry["f"] is not None]
        results = rec.correlate_dense_set([(pyramids[i], pyramids[j], entry["f"]) for (i, j), entry in todo], borrow=True)
        for (_, entry), (xy, corr) in zip(todo, results):
            entry["xy"], entry["corr"] = xy, corr
    elif dense:
        for (i, j), entry in pairs.items():
            if entry["f"] is None:
                continue
            pi, pj = pyramids[i], pyramids[j]
            if images is not None:
                dsteps = correlation.optimal_scale_steps(int(images[i].shape[1]), int(images[i].shape[0]))
                pi, pj = rec._timed("resize", lambda: (correlation.lanczos_pyramid(device, images[i], dsteps),
                                                       correlation.lanczos_pyramid(device, images[j], dsteps)))
            entry["xy"], entry["corr"] = rec.correlate_dense(pi, pj, entry["f"], borrow=borrow and images is None)
    return {"keypoints": keypoints, "pairs": pairs, "timings_ms": dict(rec.timings_ms)}


def _resident_grid(device, shape, resident: bool) -> dict:
    """complete()'s outputs for a pair of the perspective tail: none (host arrays) - or, with the resident track table, device
    tensors of the image-1 grid `shape` = (width, height), so that nothing of the grid crosses to the host."""
    if not resident:
        return {}
    import torch

    from .triangulation import _device_tensor

    w, h = shape
    return {"out_xy": _device_tensor(device, (h, w, 2), torch.int32), "out_corr": _device_tensor(device, (h, w), torch.float32)}


def match_count(xy) -> int:
    """Number of Some cells of a dense grid (host array or device tensor)."""
    if hasattr(xy, "data_ptr"):
        return int((xy[..., 0] >= 0).sum().item())
    return int((np.asarray(xy)[..., 0] >= 0).sum())


def reconstruct_perspective_surface(device, pyramids, pairs_result, cameras, bundle_adjustment: bool = True,
                                    progress=None, merge_tracks: bool = False, max_points=None, max_points_seed: int = 0,
                                    resident_tracks: bool = False):
    """The perspective tail of `reconstruct` for n views: reconstruct_dense's pair loop (reconstruction.rs:668-730) -
    for img1 in order, for every later img2 whose pair has an F in `pairs_result` (reconstruct_pairs' output; its
    dense grids are not needed, dense=False is enough), the dense correlation and extend_tracks into one track table
    (triangulation.rs:1330-1419) - then triangulate_all (:817-865) with the given cameras [(K, R, t)] per image: DLT
    points, filter_outliers and, unless bundle_adjustment is False (--no-bundle-adjustment), the bundle adjustment.
    merge_tracks=True is the reference's flow: merge_tracks (:1421-1540, run after every img1 at reconstruction.rs:726) after each
    image's pairs, every view counting as linked; False (the default) skips it.  Departures, as stated
    in DESIGN.md: the cameras come from the caller (no P3P / recover_pose).  max_points (not None): triangulate_all's random
    subset (:837-843) right behind it, on the device - triangulation.subset with max_points_seed.
    -> dict: surface (triangulation.Surface), tracks (the whole table), timings_ms per stage (dense,
    tracks, merge, triangulate); with merge_tracks, merges (per image: PerspectiveTriangulation.merge_tracks' counts); with
    max_points, surface is the subset, subset its info (triangulation.subset's) and timings_ms["subset"] its time.
    resident_tracks=True: as in reconstruct_perspective."""
    from . import triangulation

    rec = ImageReconstruction(device, ProjectionMode.Perspective)
    n = len(pyramids)
    shapes = [(int(p[0].shape[1]), int(p[0].shape[0])) for p in pyramids]
    tri = triangulation.PerspectiveTriangulation(n, shapes, bundle_adjustment=bundle_adjustment, resident_tracks=resident_tracks)
    if resident_tracks:
        tri.complete_sparse_triangulation(device)  # (no sparse half here: the empty dense table, in device memory)
    mode = correlation.ProjectionMode(int(ProjectionMode.Perspective))
    merges = []
    for i in range(n):
        for j in range(i + 1, n):
            entry = pairs_result["pairs"].get((i, j))
            if entry is None or entry["f"] is None:
                continue  # no matches between the images: no correlation (reconstruction.rs:702-707)
            pc = correlation.PointCorrelations(device, shapes[i], shapes[j], entry["f"], mode)
            try:
                def run(pc=pc, pi=pyramids[i], pj=pyramids[j]):
                    steps = correlation.optimal_scale_steps(*shapes[i])
                    for s in range(steps + 1):
                        k = steps - s
                        pc.correlate_images(pi[k], pj[k], 1.0 / float(1 << k))
                    return pc.complete(**_resident_grid(device, shapes[i], resident_tracks))

                rec._timed("dense", run)
                rec._timed("tracks", lambda pc=pc, i=i, j=j: tri.add_image_pair_dense(i, j, pc))
            finally:
                pc.close()
        if merge_tracks:
            merges.append(rec._timed("merge", lambda i=i: tri.merge_tracks(device, i)))
    surface = rec._timed("triangulate", lambda: tri.triangulate_all(device, cameras, progress=progress))
    if max_points is not None:
        surface, subset_info = rec._timed("subset", lambda: triangulation.subset(device, surface, max_points, max_points_seed))
    out = {"surface": surface, "tracks": tri.tracks, "timings_ms": dict(rec.timings_ms)}
    if merge_tracks:
        out["merges"] = merges
    if max_points is not None:
        out["subset"] = subset_info
    return out


def recover_camera_poses(device, tri, seed: int = 0, log=None):
    """recover_camera_poses (reconstruction.rs:627-666) over a PerspectiveTriangulation whose sparse pairs are in: calls
    recover_next_cameras until it places no more images; an image whose recover_pose fails is skipped (the reference prints
    the error and goes on).  Then complete_sparse_triangulation.  -> (camera_order, per-call info): "images" for a call
    that placed some, "failure" (the message) for one that failed, next to what recover_next_cameras left in last_pose."""
    from . import _lib

    order, info = [], []
    while True:
        try:
            images = tri.recover_next_cameras(device, seed=seed + len(info))
        except _lib.CvhipError as exc:  # "Failed to recover pose for next image"
            # (last_pose has an "error" of its own, recover_pose's residual, so the message gets a key that it cannot overwrite)
            info.append({**(tri.last_pose or {}), "failure": str(exc)})
            if log is not None:
                log(f"Failed to recover pose for next image: {exc}")
            continue
        if not images:
            break
        info.append({"images": images, **((tri.last_pose or {}) if len(images) == 1 else {})})
        order.extend(images)
    tri.complete_sparse_triangulation()
    return order, info


def reconstruct_perspective(device, pyramids, K, bundle_adjustment: bool = True, seed: int = 0, pairs_result=None,
                            progress=None, merge_tracks: bool = False, max_points=None, max_points_seed: int = 0,
                            resident_tracks: bool = False):
    """The perspective `reconstruct` in the reference's order for n views (reconstruction.rs:261-277, 380-395, 627-752):
    the sparse stage per pair (ORB, matcher, RANSAC - reconstruct_pairs with dense=False, or the caller's `pairs_result`),
    add_image_pair_sparse for every pair with an F (a pair that fails is skipped), recover_camera_poses, the dense
    correlation and extend_tracks of the pairs of linked images only, and triangulate_all with the recovered cameras.
    merge_tracks=True is the reference's flow: merge_tracks (triangulation.rs:1421-1540) after every linked image's
    pairs, the last linked image included (reconstruction.rs:726); False (the default) skips it.
    K: one 3 x 3 matrix for every view, or one per view.  max_points (not None; --max-points): triangulate_all's random subset
    (:837-843) right behind it, on the device - triangulation.subset with max_points_seed.
    -> dict: surface, camera_order, poses (per recover call), initial_pair, sparse ({pair: (p2, score, the short tracks scored)}), sparse_tracks (the
    table before complete_sparse_triangulation), tracks, cameras, projections, pairs, timings_ms; with merge_tracks, merges
    (per linked image: PerspectiveTriangulation.merge_tracks' counts); with max_points, surface is the subset, subset its info
    (triangulation.subset's) and timings_ms["subset"] its time.
    resident_tracks=True: the dense track table lives in device memory from extend_tracks to the surface - a
    pair's complete() writes into device tensors, extend_tracks' fill rule and append, merge_tracks, the column selection and the
    survivors' rows all run on a triangulation.DeviceTrackTable, which is out["tracks"] (`.numpy()` brings it down), and the
    surface's points and tracks are device tensors (its track_index a host array); every value equals the default path's."""
    from . import triangulation

    n = len(pyramids)
    Ks = [np.asarray(K[i] if np.ndim(K) == 3 else K, dtype=np.float64) for i in range(n)]
    if pairs_result is None:
        pairs_result = reconstruct_pairs(device, pyramids, ProjectionMode.Perspective, seed=seed, dense=False)
    rec = ImageReconstruction(device, ProjectionMode.Perspective)
    shapes = [(int(p[0].shape[1]), int(p[0].shape[0])) for p in pyramids]
    tri = triangulation.PerspectiveTriangulation(n, shapes, bundle_adjustment=bundle_adjustment, calibration=Ks,
                                                 resident_tracks=resident_tracks)
    from . import _lib

    sparse = {}
    for (i, j), entry in sorted(pairs_result["pairs"].items()):
        if entry["f"] is None:
            continue
        try:
            p2, score = rec._timed("sparse", lambda i=i, j=j, e=entry: tri.add_image_pair_sparse(device, i, j, e["f"],
                                                                                               e["inliers"]))
            sparse[(i, j)] = (p2, score, tri.last_short)
        except _lib.CvhipError:
            continue
    initial = tri.best_initial_pair
    sparse_tracks = tri.tracks.copy()
    order, poses = rec._timed("poses", lambda: recover_camera_poses(device, tri, seed=seed))
    if resident_tracks:
        tri.complete_sparse_triangulation(device)  # (the sparse table is gone: the empty dense table, in device memory)
    linked = set(order)
    mode = correlation.ProjectionMode(int(ProjectionMode.Perspective))
    merges = []
    for i in range(n):
        if i not in linked:
            continue
        for j in range(i + 1, n):
            entry = pairs_result["pairs"].get((i, j))
            if j not in linked or entry is None or entry["f"] is None:
                continue
            pc = correlation.PointCorrelations(device, shapes[i], shapes[j], entry["f"], mode)
            try:
                def run(pc=pc, pi=pyramids[i], pj=pyramids[j], i=i):
                    steps = correlation.optimal_scale_steps(*shapes[i])
                    for s in range(steps + 1):
                        k = steps - s
                        pc.correlate_images(pi[k], pj[k], 1.0 / float(1 << k))
                    return pc.complete(**_resident_grid(device, shapes[i], resident_tracks))

                rec._timed("dense", run)
                rec._timed("tracks", lambda pc=pc, i=i, j=j: tri.add_image_pair_dense(i, j, pc))
            finally:
                pc.close()
        if merge_tracks:
            merges.append(rec._timed("merge", lambda i=i: tri.merge_tracks(device, i)))
    surface = rec._timed("triangulate", lambda: tri.triangulate_all_recovered(device, progress=progress))
    if max_points is not None:
        surface, subset_info = rec._timed("subset", lambda: triangulation.subset(device, surface, max_points, max_points_seed))
    out = {"surface": surface, "camera_order": order, "poses": poses, "initial_pair": initial, "sparse": sparse,
           "sparse_tracks": sparse_tracks, "tracks": tri.tracks,
           "cameras": list(tri.cameras), "projections": list(tri.projections), "pairs": pairs_result,
           "timings_ms": dict(rec.timings_ms)}
    if merge_tracks:
        out["merges"] = merges
    if max_points is not None:
        out["subset"] = subset_info
    return out


def reconstruct_perspective_mesh(device, pyramids, K, triangulate=None, project_to_image=None, depth_scale: float = -1.0,
                                 ply_path=None, images=None, vertex_mode=0, out_scale=(1.0, 1.0, 1.0), colour_table=None,
                                 obj_path=None, save_textures=False, depth_png_path=None, depth_jpeg_path=None, jpeg_quality=75,
                                 depth_tiff_path=None, **kwargs):
    """reconstruct_perspective, then the mesh stage of output::output (output.rs:567-611) on its surface:
    mesh.create - per camera the Delaunay input, `triangulate(xy) -> [f, 3]` (the caller's Delaunay; default
    mesh.delaunay_scipy; mesh.delaunay_device(device) runs on the device and needs no scipy), the occlusion culling and the
    merged polygon list - and, when project_to_image is not None, ImageWriter's depth map of that camera (depth_scale = out_scale.2.signum()).  kwargs go to reconstruct_perspective.
    -> its dict with mesh (mesh.create's dict), depth_image (mesh.depth_image's dict or None) and timings_ms mesh /
    depth_image added.
    The output files' contents, each only when asked for: ply_path - the binary PLY of the surface and the
    merged list is written there (mesh.write_ply with images - one [h, w, 3] uint8 array per placed image, Color mode only -,
    vertex_mode, a mesh.VertexMode, and out_scale), its section sizes are out["ply_sections"], its time timings_ms["ply"];
    colour_table ([256, 3] uint8, with project_to_image) - out["depth_image"]["rgba"] is the depth map through
    mesh.colour_map; obj_path - the Wavefront OBJ of the surface and the merged list with its cameras is
    written there (mesh.write_obj with the same images, vertex_mode and out_scale; in Texture mode the .mtl goes next to it and
    the caller saves the {stem}-{i}.png images), its section sizes are out["obj_sections"], its time timings_ms["obj"].
    The PNG files, their time in timings_ms["png"]: save_textures - with obj_path, in Texture mode and with
    `images` given as arrays, the {stem}-{i}.png files the .mtl names are written next to it (mesh.write_obj_textures);
    depth_png_path - the depth map's RGBA is written there (mesh.write_depth_png, out["depth_png"] is its dict); it needs
    project_to_image and colour_table (ValueError otherwise).
    depth_jpeg_path - the depth map's RGB is written there as a baseline JPEG file of quality jpeg_quality
    (mesh.write_depth_jpeg, out["depth_jpeg"] is its dict, its time timings_ms["jpeg"]); the same two preconditions.
    depth_tiff_path - the depth map's RGBA is written there as an LZW TIFF file (mesh.write_depth_tiff,
    out["depth_tiff"] is its dict, its time timings_ms["tiff"]); the same two preconditions."""
    import time

    from . import mesh

    if depth_png_path is not None and (project_to_image is None or colour_table is None):
        raise ValueError("depth_png_path needs project_to_image and colour_table")
    if depth_jpeg_path is not None and (project_to_image is None or colour_table is None):
        raise ValueError("depth_jpeg_path needs project_to_image and colour_table")
    if depth_tiff_path is not None and (project_to_image is None or colour_table is None):
        raise ValueError("depth_tiff_path needs project_to_image and colour_table")
    out = reconstruct_perspective(device, pyramids, K, **kwargs)
    shapes = [(int(p[0].shape[1]), int(p[0].shape[0])) for p in pyramids]
    # (the surface's cameras are the placed images, in image order: prune_projections keeps the order)
    placed = [i for i in range(len(pyramids)) if out["projections"][i] is not None]
    shapes = [shapes[i] for i in placed]
    t0 = time.perf_counter()
    out["mesh"] = mesh.create(device, out["surface"], shapes, triangulate or mesh.delaunay_scipy)
    t1 = time.perf_counter()
    out["depth_image"] = None
    if project_to_image is not None:
        out["depth_image"] = mesh.depth_image(device, out["surface"], shapes, project_to_image, depth_scale, out["mesh"]["polygons"])
        if colour_table is not None:
            img = out["depth_image"]
            img["rgba"] = mesh.colour_map(device, img["map"], img["min_depth"], img["max_depth"], colour_table)
    out["mesh_image_shapes"] = shapes
    out["timings_ms"]["mesh"] = (t1 - t0) * 1e3
    out["timings_ms"]["depth_image"] = (time.perf_counter() - t1) * 1e3
    if ply_path is not None:
        t2 = time.perf_counter()
        out["ply_sections"] = mesh.write_ply(ply_path, device, out["surface"], out["mesh"]["polygons"], images,
                                             mesh.VertexMode(int(vertex_mode)), out_scale)
        out["timings_ms"]["ply"] = (time.perf_counter() - t2) * 1e3
    if obj_path is not None:
        t3 = time.perf_counter()
        out["obj_sections"] = mesh.write_obj(obj_path, device, out["surface"], out["mesh"]["polygons"], out["mesh"]["camera"],
                                             shapes if images is None and int(vertex_mode) == mesh.VertexMode.Texture else images,
                                             mesh.VertexMode(int(vertex_mode)), out_scale)
        out["timings_ms"]["obj"] = (time.perf_counter() - t3) * 1e3
    t4 = time.perf_counter()
    textures = obj_path is not None and save_textures and int(vertex_mode) == mesh.VertexMode.Texture
    if textures:
        mesh.write_obj_textures(obj_path, device, images)
    if depth_png_path is not None:
        out["depth_png"] = mesh.write_depth_png(depth_png_path, device, out["surface"], shapes, project_to_image, depth_scale,
                                                out["mesh"]["polygons"], colour_table)
    if textures or depth_png_path is not None:
        out["timings_ms"]["png"] = (time.perf_counter() - t4) * 1e3
    if depth_jpeg_path is not None:
        t5 = time.perf_counter()
        out["depth_jpeg"] = mesh.write_depth_jpeg(depth_jpeg_path, device, out["surface"], shapes, project_to_image, depth_scale,
                                                  out["mesh"]["polygons"], colour_table, quality=jpeg_quality)
        out["timings_ms"]["jpeg"] = (time.perf_counter() - t5) * 1e3
    if depth_tiff_path is not None:
        t6 = time.perf_counter()
        out["depth_tiff"] = mesh.write_depth_tiff(depth_tiff_path, device, out["surface"], shapes, project_to_image, depth_scale,
                                                  out["mesh"]["polygons"], colour_table)
        out["timings_ms"]["tiff"] = (time.perf_counter() - t6) * 1e3
    return out


def reconstruct_affine_mesh(device, pyramid1, pyramid2, f, triangulate=None, project_to_image=None, depth_scale: float = -1.0,
                            ply_path=None, obj_path=None, images=None, vertex_mode=0, out_scale=(1.0, 1.0, 1.0), colour_table=None,
                            save_textures=False, depth_png_path=None, depth_jpeg_path=None, jpeg_quality=75, depth_tiff_path=None):
    """The affine `reconstruct` of one pair, through to the mesh and its outputs: the dense correlation of the two pyramids
    with the affine F, AffineTriangulation::triangulate straight from the device grid (PointCorrelations.triangulate_affine),
    its Surface (triangulation.affine_surface: two cameras with K = diag(1, 1, 0)), mesh.create - both cameras are
    triangulated and culled as the reference does; the second camera's triangles are the first's, and the merge leaves them
    with camera 0 - and the outputs of reconstruct_perspective_mesh, each only when asked for: project_to_image (with
    depth_scale, colour_table), ply_path, obj_path (with images - one per image of the pair -, vertex_mode, out_scale),
    save_textures and depth_png_path (the PNG files; timings_ms["png"]), depth_jpeg_path and jpeg_quality (the JPEG file of
    the depth map; out["depth_jpeg"], timings_ms["jpeg"]), depth_tiff_path (the TIFF file of the depth map's RGBA;
    out["depth_tiff"], timings_ms["tiff"]).
    triangulate: the Delaunay of a camera's points; the default is mesh.delaunay_device(device, lattice=True) - the camera
    points are integer pixels, every star is an exact tie, and cvhip_mesh_delaunay decides those as defined, on the device
    (scipy's tie choices are not the defined ones).
    -> dict: surface, mesh, depth_image (or None), timings_ms (dense, triangulate, mesh, depth_image, ply, obj), and
    ply_sections / obj_sections when those files were written."""
    from . import mesh, triangulation

    if depth_png_path is not None and (project_to_image is None or colour_table is None):
        raise ValueError("depth_png_path needs project_to_image and colour_table")
    if depth_jpeg_path is not None and (project_to_image is None or colour_table is None):
        raise ValueError("depth_jpeg_path needs project_to_image and colour_table")
    if depth_tiff_path is not None and (project_to_image is None or colour_table is None):
        raise ValueError("depth_tiff_path needs project_to_image and colour_table")
    rec = ImageReconstruction(device, ProjectionMode.Affine)
    shapes = [(int(p[0].shape[1]), int(p[0].shape[0])) for p in (pyramid1, pyramid2)]
    pc = correlation.PointCorrelations(device, shapes[0], shapes[1], f, correlation.ProjectionMode(int(ProjectionMode.Affine)))
    try:
        def run():
            steps = correlation.optimal_scale_steps(*shapes[0])
            for s in range(steps + 1):
                k = steps - s
                pc.correlate_images(pyramid1[k], pyramid2[k], 1.0 / float(1 << k))

        rec._timed("dense", run)
        points3d, p2 = rec._timed("triangulate", pc.triangulate_affine)
    finally:
        pc.close()
    out = {"surface": triangulation.affine_surface(points3d, p2), "depth_image": None}
    out["mesh"] = rec._timed("mesh", lambda: mesh.create(device, out["surface"], shapes,
                                                         triangulate or mesh.delaunay_device(device, lattice=True)))
    polygons = out["mesh"]["polygons"]

    def image():
        img = mesh.depth_image(device, out["surface"], shapes, project_to_image, depth_scale, polygons)
        if colour_table is not None:
            img["rgba"] = mesh.colour_map(device, img["map"], img["min_depth"], img["max_depth"], colour_table)
        return img

    if project_to_image is not None:
        out["depth_image"] = rec._timed("depth_image", image)
    out["mesh_image_shapes"] = shapes
    if ply_path is not None:
        out["ply_sections"] = rec._timed("ply", lambda: mesh.write_ply(ply_path, device, out["surface"], polygons, images,
                                                                      mesh.VertexMode(int(vertex_mode)), out_scale))
    if obj_path is not None:
        dims = shapes if images is None and int(vertex_mode) == mesh.VertexMode.Texture else images
        out["obj_sections"] = rec._timed("obj", lambda: mesh.write_obj(obj_path, device, out["surface"], polygons, out["mesh"]["camera"],
                                                                      dims, mesh.VertexMode(int(vertex_mode)), out_scale))
        if save_textures and int(vertex_mode) == mesh.VertexMode.Texture:
            rec._timed("png", lambda: mesh.write_obj_textures(obj_path, device, images))
    if depth_png_path is not None:
        out["depth_png"] = rec._timed("png", lambda: mesh.write_depth_png(depth_png_path, device, out["surface"], shapes, project_to_image,
                                                                         depth_scale, polygons, colour_table))
    if depth_jpeg_path is not None:
        out["depth_jpeg"] = rec._timed("jpeg", lambda: mesh.write_depth_jpeg(depth_jpeg_path, device, out["surface"], shapes, project_to_image,
                                                                            depth_scale, polygons, colour_table, quality=jpeg_quality))
    if depth_tiff_path is not None:
        out["depth_tiff"] = rec._timed("tiff", lambda: mesh.write_depth_tiff(depth_tiff_path, device, out["surface"], shapes, project_to_image,
                                                                            depth_scale, polygons, colour_table))
    out["timings_ms"] = dict(rec.timings_ms)
    return out


def reconstruct_perspective_files(device, paths, focal_length_35mm=None, mesh=True, drop_rows: int = 0, on_device: bool = True, **kwargs):
    """The perspective `reconstruct` from image FILES (reconstruction.rs:39-60, 164-185, 261-277): image.load
    of every path - its Luma8 decoded on the device (JPEG, TIFF or PNG: cvhip_jpeg_decode, cvhip_tiff_decode, cvhip_png_decode), its EXIF FocalLengthIn35mmFilm -, K per image
    by image.calibration_matrix (focal_length_35mm, when given, overrides the files' values, as `:170` does; neither: 1),
    the Lanczos3 pyramids (correlation.lanczos_pyramid with correlation.optimal_scale_steps levels), then
    reconstruct_perspective_mesh (mesh=True) or reconstruct_perspective with kwargs.  With a vertex_mode of Color or Texture
    and no `images=`, the files' decoded RGB8 is passed.  on_device: the decoded Luma8 and the pyramids stay in device
    memory (torch tensors); False: numpy arrays.  drop_rows: the reference's databar_height (its SEM tag is not read).
    -> that call's dict with source_images (the image.SourceImage list), K and timings_ms["decode"] added."""
    import time

    from . import image
    from . import mesh as mesh_mod

    t0 = time.perf_counter()
    mode = int(kwargs.get("vertex_mode", 0))
    want_rgb = bool(mesh) and kwargs.get("images") is None and mode in (int(mesh_mod.VertexMode.Color), int(mesh_mod.VertexMode.Texture))
    sources = [image.load(device, p, rgb=want_rgb, drop_rows=drop_rows, out="device" if on_device else None) for p in paths]
    decode_ms = (time.perf_counter() - t0) * 1e3
    Ks = np.stack([s.calibration_matrix(focal_length_35mm) for s in sources]) if sources else np.zeros((0, 3, 3))
    pyramids = [correlation.lanczos_pyramid(device, s.img, correlation.optimal_scale_steps(int(s.img.shape[1]), int(s.img.shape[0])))
                for s in sources]
    if mesh:
        if want_rgb:
            kwargs = {**kwargs, "images": [s.rgb for s in sources]}
        out = reconstruct_perspective_mesh(device, pyramids, Ks, **kwargs)
    else:
        out = reconstruct_perspective(device, pyramids, Ks, **kwargs)
    out["source_images"], out["K"] = sources, Ks
    out["timings_ms"]["decode"] = decode_ms
    return out


def reconstruct_affine_files(device, path1, path2, f=None, seed: int = 0, on_device: bool = True, depth_scale: float = -1.0, **kwargs):
    """The affine `reconstruct` (--projection=parallel) of an SEM pair from its two FILES (reconstruction.rs:39-60, 80-144,
    223-231, 261-277, 358-362): image.load of both paths - TIFF, PNG or JPEG, the Luma8 decoded on the device
    with the file's own DatabarHeight cut, the SEM block's scale and tilt angle read -, the Lanczos3 pyramids
    (correlation.lanczos_pyramid with correlation.optimal_scale_steps levels), the sparse stage when no `f` is given
    (reconstruct_pairs in ProjectionMode.Affine with dense=False and `seed`; a pair without an F raises the reference's
    "Failed to match images"), then reconstruct_affine_mesh with kwargs and out_scale = (1, 1, depth_scale * 1): the
    reference resets the image scale to 1 (:223-231), so the files' scales are reported, not applied.  With a vertex_mode of
    Color or Texture and no `images=`, the files' decoded RGB8 is passed.  on_device: the decoded Luma8 and the pyramids stay
    in device memory (torch tensors); False: numpy arrays.
    -> that call's dict with source_images (the two image.SourceImage), f, relative_tilt_angle (the second file's tilt angle
    minus the first's, None unless both have one) and timings_ms["decode"] added."""
    import time

    from . import image
    from . import mesh as mesh_mod

    t0 = time.perf_counter()
    mode = int(kwargs.get("vertex_mode", 0))
    want_rgb = kwargs.get("images") is None and mode in (int(mesh_mod.VertexMode.Color), int(mesh_mod.VertexMode.Texture))
    sources = [image.load(device, p, rgb=want_rgb, out="device" if on_device else None) for p in (path1, path2)]
    decode_ms = (time.perf_counter() - t0) * 1e3
    pyramids = [correlation.lanczos_pyramid(device, s.img, correlation.optimal_scale_steps(int(s.img.shape[1]), int(s.img.shape[0])))
                for s in sources]
    if f is None:
        entry = reconstruct_pairs(device, pyramids, ProjectionMode.Affine, dense=False, seed=seed)["pairs"][(0, 1)]
        if entry["f"] is None:
            raise RuntimeError("Failed to match images")
        f = entry["f"]
    if want_rgb:
        kwargs = {**kwargs, "images": [s.rgb for s in sources]}
    out = reconstruct_affine_mesh(device, pyramids[0], pyramids[1], f, depth_scale=depth_scale, out_scale=(1.0, 1.0, depth_scale * 1.0), **kwargs)
    a1, a2 = sources[0].tilt_angle, sources[1].tilt_angle
    out["source_images"], out["f"] = sources, f
    out["relative_tilt_angle"] = a2 - a1 if a1 is not None and a2 is not None else None
    out["timings_ms"]["decode"] = decode_ms
    return out
