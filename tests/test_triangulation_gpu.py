"""Perspective triangulation on the device (cvhip_triangulate_perspective, cybervision_amd/triangulation.py) against the
CPU restatement (tests/ref_triangulation.py): DLT + filter_outliers on analytic track tables, the bundle adjustment, the
determinism of its reductions, the errors, and config 5's scene end to end at 512^2 and 2048^2."""
import time

import numpy as np
import pytest

import mixed_scenes
import ref_triangulation as rt
import tri_scenes
from cybervision_amd import _lib, reconstruction, synth, triangulation


def run_device(dev, tracks, cams, bundle_adjustment, image_shapes=None):
    m = tracks.shape[1]
    tri = triangulation.PerspectiveTriangulation(m, image_shapes or [(2048, 2048)] * m, bundle_adjustment=bundle_adjustment)
    tri.tracks = np.ascontiguousarray(tracks, dtype=np.int32)
    return tri.triangulate_all(dev, cams)


def rel_err(a, b):
    return np.linalg.norm(np.asarray(a) - np.asarray(b), axis=-1) / np.maximum(np.linalg.norm(np.asarray(b), axis=-1), 1e-300)


@pytest.mark.gpu
@pytest.mark.parametrize("m", [2, 3, 4, 5, 6, 7, 8])
def test_triangulate_and_filter_match_restatement(gpu_device, m):
    """triangulate_track + filter_outliers (triangulation.rs:867-911, 1559-1593), no bundle adjustment, ~100 k tracks with
    1-view tracks, parallel rays (|w| ~ 0), points behind a camera and near-duplicate views: the same kept set in the
    same order, points to 1e-9.  No track's deciding quantity lies within 1e-9 of its threshold (listed otherwise)."""
    cams = tri_scenes.rig(m, near_duplicate=m > 2)
    tracks = tri_scenes.track_table(cams, 100_000, seed=m)
    close = tri_scenes.near_threshold(tracks, cams)
    assert len(close) == 0, f"tracks at a threshold: {close[:20].tolist()}"
    ref_idx, ref_pts, _, _ = rt.triangulate_all(tracks, cams, bundle_adjustment=False)
    surf = run_device(gpu_device, tracks, cams, False)
    # every branch is exercised and decides some tracks
    k = (tracks[..., 0] >= 0).sum(axis=1)
    kept = np.zeros(len(tracks), dtype=bool)
    kept[ref_idx] = True
    assert (k < 2).any() and not kept[k < 2].any()
    assert 0.3 * len(tracks) < len(ref_idx) < 0.9 * len(tracks)
    assert np.array_equal(surf.track_index, ref_idx)
    assert (rel_err(surf.points, ref_pts) <= 1e-9).all(), rel_err(surf.points, ref_pts).max()
    assert surf.ba_iterations == 0 and np.isnan(surf.ba_residual_norms[0])


def _ba_case(dev):
    _, pert, tracks = tri_scenes.ba_scene(20_000)
    return pert, tracks, run_device(dev, tracks, pert, True)


@pytest.mark.gpu
def test_bundle_adjustment_matches_restatement(gpu_device):
    """BundleAdjustment::optimize (:2042-2147) on 20 k tracks, 3 cameras with perturbed poses and integer (sub-pixel
    noisy) observations: the same number of LM iterations, the same accept / reject sequence, cameras and points to
    1e-6, the final residual norm to 1e-9.  (As the reference writes the update every step is rejected - see
    tests/test_triangulation_ref.py - so the sequence is all rejections until the delta test ends the loop.)"""
    pert, tracks, surf = _ba_case(gpu_device)
    idx, pts, cams, ba = rt.triangulate_all(tracks, pert, bundle_adjustment=True)
    assert np.array_equal(surf.track_index, idx)
    assert surf.ba_iterations == len(ba.history)
    assert surf.ba_history == [int(h) for h in ba.history]
    assert (rel_err(surf.points, pts) <= 1e-6).all()
    for dc, rc in zip(surf.cameras, cams):
        assert np.allclose(dc.r, rc.r, rtol=1e-6, atol=1e-12)
        assert np.allclose(dc.t, rc.t, rtol=1e-6, atol=1e-12)
        assert np.allclose(dc.projection, rc.projection(), rtol=1e-6, atol=1e-9)
    assert abs(surf.ba_residual_norms[1] - ba.final_residual_norm) <= 1e-9 * ba.final_residual_norm


@pytest.mark.gpu
def test_bundle_adjustment_is_deterministic(gpu_device):
    """Two runs of the bundle adjustment case give the same bits (fixed-order reductions)."""
    _, _, a = _ba_case(gpu_device)
    _, _, b = _ba_case(gpu_device)
    assert np.array_equal(a.track_index, b.track_index)
    assert a.points.tobytes() == b.points.tobytes()
    assert a.ba_history == b.ba_history and a.ba_residual_norms == b.ba_residual_norms
    for ca, cb in zip(a.cameras, b.cameras):
        assert ca.r.tobytes() == cb.r.tobytes() and ca.t.tobytes() == cb.t.tobytes()


@pytest.mark.gpu
def test_errors(gpu_device):
    """Fewer than two views everywhere: every track is rejected (:881-883) and, as in the reference (an empty
    bundle adjustment returns at :2050), the surface is empty - not an error; the cameras are from_matrix's.  More than
    CVHIP_TRIANGULATE_MAX_CAMERAS cameras: CVHIP_ERR_UNSUPPORTED.  A progress listener sees iter / 100 (:2054-2056)."""
    cams = tri_scenes.rig(3)
    tracks = tri_scenes.track_table(cams, 10_000, seed=9)
    single = tracks.copy()
    single[:, 1:] = -1
    surf = run_device(gpu_device, single, cams, True)
    assert len(surf.points) == 0 and surf.ba_iterations == 0
    for dc, (K, R, t) in zip(surf.cameras, cams):
        rc = rt.Camera.from_matrix(K, R, t)
        assert np.allclose(dc.r, rc.r, atol=1e-15) and np.allclose(dc.projection, rc.projection(), rtol=1e-14)
    cams9 = tri_scenes.rig(9)
    with pytest.raises(_lib.CvhipError) as err:
        run_device(gpu_device, tri_scenes.track_table(cams9, 1000, seed=1), cams9, False)
    assert err.value.code == -3
    pert, btracks = tri_scenes.ba_scene(2000)[1:]
    seen = []
    tri = triangulation.PerspectiveTriangulation(3, [(2048, 2048)] * 3)
    tri.tracks = btracks
    surf = tri.triangulate_all(gpu_device, pert, progress=seen.append)
    # one report per pass of the loop: the decided steps, and the last pass, which the delta test ends (:2079-2083)
    assert seen == [np.float32(i / 100.0) for i in range(surf.ba_iterations + 1)]


def _call_perspective(dev, tracks, cams, bundle_adjustment, pts, idx):
    """cvhip_triangulate_perspective with the table and the two per-track outputs wherever the caller keeps them (numpy
    arrays or CUDA tensors) -> (out_n, the small host outputs' bytes)."""
    import ctypes as C

    def ptr(a):
        return C.c_void_p(a.data_ptr() if hasattr(a, "data_ptr") else a.ctypes.data)

    n, m = tracks.shape[:2]
    K = np.ascontiguousarray(np.stack([np.asarray(c[0], dtype=np.float64).reshape(9) for c in cams]))
    R = np.ascontiguousarray(np.stack([np.asarray(c[1], dtype=np.float64).reshape(9) for c in cams]))
    t = np.ascontiguousarray(np.stack([np.asarray(c[2], dtype=np.float64).reshape(3) for c in cams]))
    out_r, out_t, out_p = np.zeros((m, 3)), np.zeros((m, 3)), np.zeros((m, 3, 4))
    out_n, iters = C.c_uint64(0), C.c_uint32(0)
    history, norms = np.zeros(triangulation.BUNDLE_ADJUSTMENT_MAX_ITERATIONS, dtype=np.uint8), np.zeros(2)
    _lib.check(_lib.lib().cvhip_triangulate_perspective(
        dev.handle, ptr(tracks), n, m, ptr(K), ptr(R), ptr(t), int(bundle_adjustment), ptr(pts), ptr(idx), ptr(out_r),
        ptr(out_t), ptr(out_p), C.byref(out_n), C.byref(iters), ptr(history), ptr(norms), _lib.NULL_PROGRESS, None),
        "cvhip_triangulate_perspective")
    return out_n.value, (out_r.tobytes(), out_t.tobytes(), out_p.tobytes(), iters.value, history.tobytes(), norms.tobytes())


@pytest.mark.gpu
@pytest.mark.parametrize("bundle_adjustment", [False, True])
def test_device_resident_table_and_outputs(gpu_device, bundle_adjustment):
    """The table, out_points and out_index in device memory, all of them or some: out_n, the points, the index and the
    cameras are the host call's bytes, rows from out_n on keep what they held, and the caller's table is not written -
    the bundle adjustment compacts a copy of it.  600 tracks without the bundle adjustment (past two blocks, no multiple
    of 256), the 2000-track scene of test_errors with it."""
    import torch

    if bundle_adjustment:
        _, cams, tracks = tri_scenes.ba_scene(2000)
    else:
        cams = tri_scenes.rig(3)
        tracks = tri_scenes.track_table(cams, 600, seed=5)
    tracks = np.ascontiguousarray(tracks, dtype=np.int32)
    n = len(tracks)
    POINT, INDEX = -7.25, 0x5A5A5A5A5A5A5A5A

    def host_outputs():
        return np.full((n, 3), POINT), np.full(n, INDEX, dtype=np.uint64)

    def device_outputs():
        return (torch.full((n, 3), POINT, dtype=torch.float64, device="cuda"),
                torch.full((n,), INDEX, dtype=torch.int64, device="cuda"))

    def host(a):
        return a.cpu().numpy() if hasattr(a, "cpu") else a

    d_tracks = torch.from_numpy(tracks).cuda()
    torch.cuda.synchronize()
    want_pts, want_idx = host_outputs()
    k, want_small = _call_perspective(gpu_device, tracks, cams, bundle_adjustment, want_pts, want_idx)
    assert 0 < k and (bundle_adjustment or k < n)
    assert (want_pts[k:] == POINT).all() and (want_idx[k:] == INDEX).all()
    for tracks_dev, pts_dev, idx_dev in ((True, True, True), (True, False, True), (False, True, False)):
        pts, idx = (device_outputs() if pts_dev else host_outputs())[0], (device_outputs() if idx_dev else host_outputs())[1]
        torch.cuda.synchronize()
        got_k, small = _call_perspective(gpu_device, d_tracks if tracks_dev else tracks, cams, bundle_adjustment, pts, idx)
        assert got_k == k and small == want_small
        assert host(pts).tobytes() == want_pts.tobytes()  # (the rows from k on: the fill value, as in want_pts)
        assert host(idx).view(np.uint64).tobytes() == want_idx.tobytes()
    assert d_tracks.cpu().numpy().tobytes() == tracks.tobytes()


def _compare_ba(surf, idx, pts, cams, ba, tol, tol_res):
    """The device's bundle adjustment against the restatement's: the kept set, the iteration count, the exact accept /
    reject sequence, both residual norms to tol_res, points, and each camera's r, t and projection to tol (relative to
    the largest element: a step moves every component, the small ones by as much as the large)."""
    assert np.array_equal(surf.track_index, idx)
    assert surf.ba_iterations == len(ba.history)
    assert surf.ba_history == [int(h) for h in ba.history]
    for dn, rn in zip(surf.ba_residual_norms, (ba.initial_residual_norm, ba.final_residual_norm)):
        assert abs(dn - rn) <= tol_res * rn, (dn, rn)
    assert (rel_err(surf.points, pts) <= tol).all(), rel_err(surf.points, pts).max()
    for j, (dc, rc) in enumerate(zip(surf.cameras, cams)):
        assert tri_scenes.vec_close(dc.r, rc.r, tol, 1e-12), j
        assert tri_scenes.vec_close(dc.t, rc.t, tol, 1e-12), j
        assert tri_scenes.vec_close(dc.projection, rc.projection(), tol, 1e-9), j


def _case_id(case):
    m, n, seed, far, accepts = case
    return f"m{m}-n{n}-seed{seed}-{'accepts' if accepts else 'rejects'}" + ("-mixed" if isinstance(case, tri_scenes.MixedCase) else "")


@pytest.mark.gpu
@pytest.mark.parametrize("case", tri_scenes.BA_RIG_CASES, ids=_case_id)
def test_bundle_adjustment_every_camera_count(gpu_device, case):
    """BundleAdjustment::optimize (:2042-2147) with every camera count the kernels are instantiated for (M = 2..8),
    ~20 k tracks over tri_scenes.ba_rig_scene: each track seen in 2..m views, the rest missing (the obs.x < 0 residual,
    V summed over every view, seen or not), the cameras 1..m-1 perturbed.  M >= 5 runs the second camera group of
    ba_jtr_kernel; M = 8 the 48 x 48 LU.  Compared as test_bundle_adjustment_matches_restatement: the kept set, the
    iteration count, the exact accept / reject sequence, both residual norms, points and cameras, at that test's 1e-6
    (points, cameras) and 1e-9 (residual norms).  Every scene is all-rejected (tri_scenes.BA_RIG_CASES says why); every
    rho is at least 0.1 away from 0 and keeps its sign under a reversed summation order (tests/test_triangulation_ref.py)."""
    m, n, seed, far, accepts = case
    _, given, tracks = tri_scenes.ba_case_scene(case)
    idx, pts, cams, ba = tri_scenes.ba_restatement(given, tracks)
    assert any(ba.history) == accepts
    surf = run_device(gpu_device, tracks, given, True)
    print(f"m={m}: {len(idx)} kept, history {surf.ba_history}")
    _compare_ba(surf, idx, pts, cams, ba, 1e-6, 1e-9)


@pytest.mark.gpu
def test_bundle_adjustment_past_one_grid(gpu_device):
    """The bundle adjustment with more than MAX_GRID = 1024 blocks of 256 kept tracks, so every thread of
    ba_schur_kernel, ba_step_kernel and ba_jtr_kernel walks its grid-stride loop more than once: 3 cameras, 270 k
    tracks, all-rejected.  Compared with the restatement as above (1e-6, 1e-9).  Two device runs give the same bits."""
    case = tri_scenes.BA_GRID_CASE
    _, given, tracks = tri_scenes.ba_case_scene(case)
    idx, pts, cams, ba = tri_scenes.ba_restatement(given, tracks)
    assert len(idx) > tri_scenes.GRID_STRIDE_TRACKS and any(ba.history) == case[4]
    a = run_device(gpu_device, tracks, given, True)
    print(f"{len(idx)} kept, history {a.ba_history}")
    _compare_ba(a, idx, pts, cams, ba, 1e-6, 1e-9)
    b = run_device(gpu_device, tracks, given, True)
    assert np.array_equal(a.track_index, b.track_index)
    assert a.points.tobytes() == b.points.tobytes()
    assert a.ba_history == b.ba_history and a.ba_residual_norms == b.ba_residual_norms
    for ca, cb in zip(a.cameras, b.cameras):
        assert ca.r.tobytes() == cb.r.tobytes() and ca.t.tobytes() == cb.t.tobytes()
        assert ca.projection.tobytes() == cb.projection.tobytes()


def ground_truth_depth_error(points, K, size):
    """|z - Z0(p0)| / Z0(p0) per point, p0 = the point's pixel in view 0 (camera 0 is the identity: z is its depth)."""
    q = points @ K.T
    x, y = q[:, 0] / q[:, 2], q[:, 1] / q[:, 2]
    inside = (x >= 0) & (x < size) & (y >= 0) & (y < size)
    z0 = synth._sfm_depth(x[inside], y[inside], size)
    return np.abs(points[inside, 2] - z0) / z0


@pytest.mark.gpu
def test_sfm3_surface_512_matches_restatement(gpu_device):
    """Config 5 at 512^2: reconstruct_pairs' sparse stage, then reconstruct_perspective_surface with the true cameras
    and bundle adjustment on; the same track table through the restatement gives the same surface: the same kept set
    and accept / reject sequence, the final residual norm to 1e-6, points and cameras to 1e-4.  (The reference's
    update is uphill - tests/test_triangulation_ref.py - and its first step is so large that, on this scene, it lands
    lower and is accepted: it carries the points ~2000 scene units away, and the rounding of the 18 x 18 solve with
    them - measured 3.2e-5 at most on the points, 2.5e-7 on the residual - so the bounds here are looser than the
    1e-6 / 1e-9 of the all-rejected case above.)  The triangulation itself (no bundle adjustment) against the scene's
    ground truth: median relative depth error below 3 %."""
    size = 512
    views, K, poses = synth.make_sfm_views(size)
    steps = synth.optimal_scale_steps(size, size)
    pyrs = [synth.box_pyramid(v, steps) for v in views]
    pairs = reconstruction.reconstruct_pairs(gpu_device, pyrs, dense=False)
    cams = [(K, R, t) for R, t in poses]
    out = reconstruction.reconstruct_perspective_surface(gpu_device, pyrs, pairs, cams, bundle_adjustment=True)
    surf, table = out["surface"], out["tracks"]
    assert len(table) > 50_000 and len(surf.points) > 0.5 * len(table)
    idx, pts, rcams, ba = rt.triangulate_all(table, cams, bundle_adjustment=True)
    assert np.array_equal(surf.track_index, idx)
    assert surf.ba_history == [int(h) for h in ba.history]
    assert abs(surf.ba_residual_norms[1] - ba.final_residual_norm) <= 1e-6 * ba.final_residual_norm
    assert (rel_err(surf.points, pts) <= 1e-4).all(), rel_err(surf.points, pts).max()
    for dc, rc in zip(surf.cameras, rcams):
        assert np.allclose(dc.r, rc.r, rtol=1e-4, atol=1e-12) and np.allclose(dc.t, rc.t, rtol=1e-4, atol=1e-12)
    plain = run_device(gpu_device, table, cams, False)
    assert np.array_equal(plain.track_index, surf.track_index)
    err = ground_truth_depth_error(plain.points, K, size)
    err_ba = ground_truth_depth_error(surf.points, K, size)
    print(f"512^2: {len(table)} tracks, {len(surf.points)} kept, median depth error {np.median(err):.4f} "
          f"({np.median(err_ba):.4f} after the bundle adjustment, history {surf.ba_history}), timings {out['timings_ms']}")
    assert np.median(err) < 0.03


@pytest.mark.gpu
def test_sfm3_surface_2048_properties(gpu_device):
    """Config 5 at 2048^2 (no restatement: size-independent properties): most tracks kept, the reprojection RMS after
    the bundle adjustment not above the one before, the median relative depth error of the triangulation (no bundle
    adjustment) against the ground truth below 2 %; wall time reported.  The RMS is the bundle adjustment's own, taken
    with Camera::from_matrix's cameras, whose rotation angle is atan2(2 sin, cos) of the given one
    (tests/test_triangulation_ref.py): ~1.7 px before, so no sub-pixel bound holds for the reference's residual."""
    size = 2048
    views, K, poses = synth.make_sfm_views(size)
    steps = synth.optimal_scale_steps(size, size)
    pyrs = [synth.box_pyramid(v, steps) for v in views]
    pairs = reconstruction.reconstruct_pairs(gpu_device, pyrs, dense=False)
    cams = [(K, R, t) for R, t in poses]
    t0 = time.perf_counter()
    out = reconstruction.reconstruct_perspective_surface(gpu_device, pyrs, pairs, cams, bundle_adjustment=True)
    wall = time.perf_counter() - t0
    surf, table = out["surface"], out["tracks"]
    n_obs = int((surf.tracks[..., 0] >= 0).sum())
    rms_before, rms_after = (v / np.sqrt(n_obs) for v in surf.ba_residual_norms)
    plain = run_device(gpu_device, table, cams, False)
    err = ground_truth_depth_error(plain.points, K, size)
    err_ba = ground_truth_depth_error(surf.points, K, size)
    print(f"2048^2: {len(table)} tracks, {len(surf.points)} kept ({len(surf.points) / len(table):.3f}), reprojection RMS "
          f"{rms_before:.4f} -> {rms_after:.4f} px over {n_obs} observations, LM history {surf.ba_history}, median depth "
          f"error {np.median(err):.4f} ({np.median(err_ba):.4f} after the bundle adjustment), wall {wall:.2f} s, "
          f"timings {out['timings_ms']}")
    assert len(surf.points) > 0.5 * len(table)
    assert rms_after <= rms_before
    assert np.median(err) < 0.02


# ---- the mixed rig: a K per camera (fx != fy, skew, off-centre principal point), no two images of one size ---------------
@pytest.mark.gpu
@pytest.mark.parametrize("m", [2, 3, 8])
def test_triangulate_and_filter_match_restatement_on_the_mixed_rig(gpu_device, m):
    """test_triangulate_and_filter_match_restatement's comparison on tri_scenes.mixed_rig(m) - every camera's K its own,
    images of mixed_scenes.DIMS -, 20 k tracks (~78 blocks of 256): the same kept set in the same order, points to 1e-9,
    every branch deciding some tracks.  With one shared, symmetric K a kernel that takes camera j's K from camera 0, or
    K[1] for K[3], computes the same numbers; here it does not (tests/test_triangulation_ref.py)."""
    cams = tri_scenes.mixed_rig(m, near_duplicate=m > 2)
    tracks = tri_scenes.track_table(cams, 20_000, seed=m)
    close = tri_scenes.near_threshold(tracks, cams)
    assert len(close) == 0, f"tracks at a threshold: {close[:20].tolist()}"
    ref_idx, ref_pts, _, _ = rt.triangulate_all(tracks, cams, bundle_adjustment=False)
    surf = run_device(gpu_device, tracks, cams, False, image_shapes=mixed_scenes.DIMS[:m])
    k = (tracks[..., 0] >= 0).sum(axis=1)
    kept = np.zeros(len(tracks), dtype=bool)
    kept[ref_idx] = True
    assert (k < 2).any() and not kept[k < 2].any()
    assert 0.3 * len(tracks) < len(ref_idx) < 0.9 * len(tracks)
    assert np.array_equal(surf.track_index, ref_idx)
    assert (rel_err(surf.points, ref_pts) <= 1e-9).all(), rel_err(surf.points, ref_pts).max()
    assert surf.ba_iterations == 0 and np.isnan(surf.ba_residual_norms[0])


@pytest.mark.gpu
@pytest.mark.parametrize("case", tri_scenes.BA_MIXED_CASES, ids=_case_id)
def test_bundle_adjustment_on_the_mixed_rig(gpu_device, case):
    """test_bundle_adjustment_every_camera_count's comparison (1e-6 points and cameras, 1e-9 residual norms, the exact
    accept / reject sequence) with a K per camera: d * K of the Jacobians uses all nine entries of the camera's own K.
    m = 6 and m = 8 run the second camera group of ba_jtr_kernel.  The scenes' claims: tests/test_triangulation_ref.py's
    test_ba_scene_claims, as for BA_RIG_CASES, and test_ba_mixed_scene_keeps_its_history_however_v_is_inverted."""
    m, n, seed, far, accepts = case
    _, given, tracks = tri_scenes.ba_case_scene(case)
    idx, pts, cams, ba = tri_scenes.ba_restatement(given, tracks)
    assert any(ba.history) == accepts
    surf = run_device(gpu_device, tracks, given, True, image_shapes=mixed_scenes.DIMS[:m])
    print(f"mixed m={m}: {len(idx)} kept, history {surf.ba_history}")
    _compare_ba(surf, idx, pts, cams, ba, 1e-6, 1e-9)


@pytest.mark.gpu
def test_perspective_cameras_on_the_mixed_rig(gpu_device):
    """cvhip_triangulate_perspective_cameras with three mixed cameras given as pose recovery leaves them: r =
    from_matrix's, and the projection K_j [matrix_r(r) | t] of a P3P camera - not K_j [R | t] -, which is where such a
    projection and a K of its own meet.  No bundle adjustment, 5 k tracks: the restatement's kept set in order and points
    to 1e-9 (no track at a threshold: tests/test_triangulation_ref.py); then the device-resident test's comparison:
    table and outputs in device memory give the host call's bytes, rows from out_n on keep what they held."""
    import ctypes as C

    import torch

    given, cams, P, tracks = tri_scenes.mixed_p3p_case()
    n, m = tracks.shape[:2]
    K = np.ascontiguousarray(np.stack([c.k.reshape(9) for c in cams]))
    r = np.ascontiguousarray(np.stack([c.r for c in cams]))
    t = np.ascontiguousarray(np.stack([c.t for c in cams]))
    Pc = np.ascontiguousarray(P)
    POINT, INDEX = -7.25, 0x5A5A5A5A5A5A5A5A

    def ptr(a):
        return C.c_void_p(a.data_ptr() if hasattr(a, "data_ptr") else a.ctypes.data)

    def call(table, pts, idx):
        out_r, out_t, out_p = np.zeros((m, 3)), np.zeros((m, 3)), np.zeros((m, 3, 4))
        out_n = C.c_uint64(0)
        _lib.check(_lib.lib().cvhip_triangulate_perspective_cameras(
            gpu_device.handle, ptr(table), n, m, ptr(K), ptr(r), ptr(t), ptr(Pc), 0, ptr(pts), ptr(idx), ptr(out_r),
            ptr(out_t), ptr(out_p), C.byref(out_n), None, None, None, _lib.NULL_PROGRESS, None),
            "cvhip_triangulate_perspective_cameras")
        return out_n.value, out_r, out_t, out_p

    want_idx, want_pts = rt.triangulate_and_filter(tracks, cams, P)
    pts, idx = np.full((n, 3), POINT), np.full(n, INDEX, dtype=np.uint64)
    k, out_r, out_t, out_p = call(tracks, pts, idx)
    assert 0.3 * n < k < 0.9 * n and np.array_equal(idx[:k].astype(np.int64), want_idx)
    assert (rel_err(pts[:k], want_pts) <= 1e-9).all(), rel_err(pts[:k], want_pts).max()
    assert (pts[k:] == POINT).all() and (idx[k:] == INDEX).all()
    for j, c in enumerate(cams):  # the cameras come back as given
        assert np.array_equal(out_r[j], c.r) and np.array_equal(out_t[j], c.t)
        assert np.allclose(out_p[j], c.projection(), rtol=1e-9, atol=1e-9)
    d_tracks = torch.from_numpy(tracks).cuda()
    d_pts = torch.full((n, 3), POINT, dtype=torch.float64, device="cuda")
    d_idx = torch.full((n,), INDEX, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    got_k, got_r, got_t, got_p = call(d_tracks, d_pts, d_idx)
    assert got_k == k and got_r.tobytes() == out_r.tobytes() and got_p.tobytes() == out_p.tobytes()
    assert d_pts.cpu().numpy().tobytes() == pts.tobytes() and d_idx.cpu().numpy().view(np.uint64).tobytes() == idx.tobytes()
    assert d_tracks.cpu().numpy().tobytes() == tracks.tobytes()
