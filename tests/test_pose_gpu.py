"""Pose recovery on the device against the restatement (tests/ref_pose.py) and the planted geometry."""
import numpy as np
import pytest

import mixed_scenes
import pose_checks
import pose_scenes
import ref_pose as rp
import ref_triangulation as rt
from cybervision_amd import _lib, reconstruction, synth, triangulation

pytestmark = pytest.mark.gpu


def _p(a):
    import ctypes as C
    return C.c_void_p(a.ctypes.data)


def _known(K, poses):
    P = np.ascontiguousarray(np.stack([pose_scenes.projection(K, *poses[0]), pose_scenes.projection(K, *poses[1]),
                                       np.zeros((3, 4))]))
    return P, np.array([1, 1, 0], dtype=np.uint8)


def device_triangulate(dev, tracks, P, has):
    n, m = tracks.shape[:2]
    pts, ok = np.zeros((n, 3)), np.zeros(n, dtype=np.uint8)
    tr = np.ascontiguousarray(tracks)
    _lib.check(_lib.lib().cvhip_triangulate_tracks(dev.handle, _p(tr), n, m, _p(P), _p(has), _p(pts), _p(ok)), "tt")
    return pts, ok.astype(bool)


def test_triangulate_tracks_matches_restatement(gpu_device):
    tracks, K, poses, _ = pose_scenes.scene(n=2000)
    tracks[::7, 0] = -1
    allP = [pose_scenes.projection(K, R, t) for R, t in poses]
    for has in ([1, 1, 0], [1, 0, 1], [0, 1, 1], [1, 1, 1]):
        has = np.array(has, dtype=np.uint8)
        P = np.ascontiguousarray(np.stack([allP[j] if has[j] else np.zeros((3, 4)) for j in range(3)]))
        pts, ok = device_triangulate(gpu_device, tracks, P, has)
        masked = tracks.copy()
        masked[:, has == 0] = -1
        wpts, wok, _ = rt.triangulate_tracks(masked, list(P))
        assert np.array_equal(ok, wok)
        assert np.allclose(pts[ok], wpts[ok], rtol=1e-9, atol=1e-12)


def test_triangulate_tracks_device_resident_table(gpu_device):
    """cvhip_triangulate_tracks with the table in device memory (600 tracks, 3 views: past two blocks, no multiple of
    256) reads it in place: the host call's bytes, into host and into device outputs, and the table is unchanged."""
    import ctypes as C

    import torch

    tracks, K, poses, _ = pose_scenes.scene(n=600)
    tracks[::7, 0] = -1
    tracks = np.ascontiguousarray(tracks)
    has = np.array([1, 1, 1], dtype=np.uint8)
    P = np.ascontiguousarray(np.stack([pose_scenes.projection(K, R, t) for R, t in poses]))
    n, m = tracks.shape[:2]
    assert (n, m) == (600, 3)
    want_pts, want_ok = np.zeros((n, 3)), np.zeros(n, dtype=np.uint8)
    call = _lib.lib().cvhip_triangulate_tracks
    _lib.check(call(gpu_device.handle, _p(tracks), n, m, _p(P), _p(has), _p(want_pts), _p(want_ok)), "tt")
    assert 0 < want_ok.sum()
    d_tracks = torch.from_numpy(tracks).cuda()
    dp = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    pts, ok = np.zeros((n, 3)), np.zeros(n, dtype=np.uint8)
    _lib.check(call(gpu_device.handle, dp(d_tracks), n, m, _p(P), _p(has), _p(pts), _p(ok)), "tt")
    assert pts.tobytes() == want_pts.tobytes() and ok.tobytes() == want_ok.tobytes()
    d_pts = torch.zeros((n, 3), dtype=torch.float64, device="cuda")
    d_ok = torch.zeros(n, dtype=torch.uint8, device="cuda")
    _lib.check(call(gpu_device.handle, dp(d_tracks), n, m, _p(P), _p(has), dp(d_pts), dp(d_ok)), "tt")
    assert d_pts.cpu().numpy().tobytes() == want_pts.tobytes() and d_ok.cpu().numpy().tobytes() == want_ok.tobytes()
    assert d_tracks.cpu().numpy().tobytes() == tracks.tobytes()


def test_find_projection_matrix_matches_restatement(gpu_device):
    tracks, K, poses, _ = pose_scenes.scene(n=3000)
    for i, j in [(0, 1), (0, 2), (1, 2)]:
        F = synth.sfm_true_f(K, poses[i], poses[j])
        short = np.ascontiguousarray(tracks[:, [i, j]])
        p2, r2 = np.zeros((3, 4)), np.zeros(3)
        import ctypes as C
        score = C.c_double(0)
        _lib.check(_lib.lib().cvhip_find_projection_matrix(gpu_device.handle, _p(np.ascontiguousarray(F)), _p(K), _p(K),
                                                           _p(short), len(short), _p(p2), C.byref(score), _p(r2), None), "fpm")
        wp2, wcount, counts = rp.find_projection_matrix(F, K, K, short)
        assert score.value == wcount and sorted(counts)[-2] < wcount
        assert np.allclose(p2, wp2, rtol=1e-9, atol=1e-9)
        assert np.allclose(r2, rt.Camera.from_matrix(K, p2[:, :3], p2[:, 3]).r, rtol=1e-9, atol=1e-12)


def test_pose_models_match_restatement_per_sample(gpu_device):
    """recover_pose's hot path per sample (cvhip_recover_pose_models) against ref_pose.pose_candidates on 3000 triples, with
    duplicate indices and near-collinear triples: the same root slots in order, R, t, the Camera's r and projection to
    1e-9 (1e-6 for at most 1 % of the poses, those of ill-conditioned triples), the same 3-sample verdicts; counts exact and the largest residual to 1e-9 of the image size once the tracks whose error lies within
    that distance of the threshold are set aside (as tri_scenes.near_threshold does): the count may differ by at most their number, and
    the error is compared where there is none."""
    tracks, K, poses, X = pose_scenes.scene(n=1500)
    P, has = _known(K, poses)
    pts, ok = device_triangulate(gpu_device, tracks, P, has)
    lt, lp = rp.linked(tracks, pts, ok, 2)
    # (noise_triples: this test's samples stay as drawn, as they always were)
    samples = pose_checks.sample_triples(lp, 3000, seed=9, noise_triples=True)
    got = pose_checks.device_models(gpu_device, tracks, pts, ok, P, has, 2, K, 512, samples)
    pose_checks.check_models(got, lt, lp, [P[0], P[1], None], 2, K, 512, samples)


def test_extend_tracks_matches_is_bit_exact(gpu_device, oracle):
    """cvhip_extend_tracks_matches against oracle.cvref.extend_tracks on add_image_pair_sparse's inlier grid: duplicate
    image-1 points (the later one wins), inliers on the grid's edges, existing tracks near and far from inliers, none."""
    w, h = 300, 200
    rng = np.random.default_rng(11)
    k = 4000
    # (image-2 points inside the image-1 grid: the reference indexes that grid with them when it clears a merged match)
    inl = np.stack([rng.integers(0, w, k), rng.integers(0, h, k), rng.integers(0, w, k), rng.integers(0, h, k)], axis=1)
    inl[:50, :2] = inl[50:100, :2]  # duplicates of image-1 points
    inl[100:110] = [[0, 0, 5, 5], [w - 1, 0, 6, 6], [0, h - 1, 7, 7], [w - 1, h - 1, 8, 8], [w - 1, 50, 0, 0],
                    [3, h - 1, w - 1, h - 1], [w // 2, 0, 1, 2], [0, h // 2, 3, 4], [w - 1, h // 2, 9, 9], [w // 2, h - 1, 2, 1]]
    inl = np.ascontiguousarray(inl.astype(np.uint32))
    grid = np.full((h, w, 2), -1, dtype=np.int32)
    for x1, y1, x2, y2 in inl:
        grid[y1, x1] = (x2, y2)
    near = inl[200:400, :2].astype(np.int32) + rng.integers(-2, 3, size=(200, 2)).astype(np.int32)
    far = np.full((50, 2), -1, dtype=np.int32)
    edge = np.array([[0, 0], [w - 1, h - 1], [w + 5, 3], [2, h + 9]], dtype=np.int32)
    for tracks in (np.zeros((0, 2), dtype=np.int32), np.ascontiguousarray(np.concatenate([near, far, edge]))):
        for max_dim2 in (320, 2048):
            wtp2, wn1, wn2 = oracle.extend_tracks(grid, tracks, max_dim2)
            n = len(tracks)
            tp2 = np.full((max(n, 1), 2), -1, dtype=np.int32)
            n1, n2 = np.zeros((k, 2), dtype=np.uint32), np.zeros((k, 2), dtype=np.uint32)
            import ctypes as C
            n_new = C.c_uint64(0)
            _lib.check(_lib.lib().cvhip_extend_tracks_matches(gpu_device.handle, _p(inl), k, w, h, _p(tracks) if n else None,
                                                              n, max_dim2, _p(tp2) if n else None, _p(n1), _p(n2), k,
                                                              C.byref(n_new)), "etm")
            m = n_new.value
            assert np.array_equal(tp2[:n], wtp2)
            assert m == len(wn1) and np.array_equal(n1[:m], wn1) and np.array_equal(n2[:m], wn2)
    bad = np.ascontiguousarray(np.array([[1, 1, 65535, 65535]], dtype=np.uint32))
    import ctypes as C
    n_new = C.c_uint64(0)
    rc = _lib.lib().cvhip_extend_tracks_matches(gpu_device.handle, _p(bad), 1, w, h, None, 0, 320, None, _p(n1), _p(n2), k,
                                                C.byref(n_new))
    assert rc == -1


def test_recover_pose_finds_the_third_camera_deterministically(gpu_device):
    tracks, K, poses, _ = pose_scenes.scene(n=3000)
    tri = triangulation.PerspectiveTriangulation(3, [(512, 512)] * 3, calibration=[K] * 3)
    tri.tracks = tracks.copy()
    tri.projections = [pose_scenes.projection(K, *poses[0]), pose_scenes.projection(K, *poses[1]), None]
    tri.cameras = [(K, np.zeros(3), np.zeros(3)), (K, np.zeros(3), poses[1][1]), None]
    tri.remaining_images = [2]
    tri.triangulate_tracks(gpu_device)
    runs = []
    for _ in range(2):
        t2 = triangulation.PerspectiveTriangulation(3, [(512, 512)] * 3, calibration=[K] * 3)
        t2.tracks, t2.points, t2.points_ok = tri.tracks.copy(), tri.points.copy(), tri.points_ok.copy()
        t2.projections, t2.cameras, t2.remaining_images = list(tri.projections), list(tri.cameras), [2]
        assert t2.recover_next_cameras(gpu_device, seed=17) == [2]
        runs.append((t2.projections[2].copy(), t2.cameras[2][1].copy(), t2.last_pose))
    assert np.array_equal(runs[0][0], runs[1][0])
    info = runs[0][2]
    assert all(info[k] == runs[1][2][k] for k in ("count", "error", "batches", "winner"))
    assert info["count"] >= rp.RANSAC_D_PERCENT_EARLY_EXIT * info["linked"] // 100 and info["batches"] == 1
    Pt = pose_scenes.projection(K, *poses[2])
    assert np.abs(runs[0][0] / np.linalg.norm(runs[0][0]) - Pt / np.linalg.norm(Pt)).max() < 1e-2


def test_recover_pose_errors(gpu_device):
    tracks, K, poses, _ = pose_scenes.scene(n=600)
    P, has = _known(K, poses)
    for n_keep, scramble in ((2, False), (600, True)):
        tr = tracks[:n_keep].copy()
        if scramble:
            tr[:, 2] = np.random.default_rng(1).integers(0, 512, size=(n_keep, 2))
        pts, ok = device_triangulate(gpu_device, tr, P, has)
        import ctypes as C
        r, t, pr = np.zeros(3), np.zeros(3), np.zeros(12)
        cnt, err, bat = C.c_uint32(0), C.c_double(0), C.c_uint32(0)
        okb = ok.astype(np.uint8)
        rc = _lib.lib().cvhip_recover_pose(gpu_device.handle, _p(tr), n_keep, 3, _p(pts), _p(okb), _p(P), _p(has), 2, _p(K),
                                           512, 3, _p(r), _p(t), _p(pr), C.byref(cnt), C.byref(err), C.byref(bat), None,
                                           _lib.NULL_PROGRESS, None)
        assert rc == -6 and b"Unable to find projection matrix" in _lib.lib().cvhip_last_error()


def _sparse_restatement(oracle, out, K, size, seed):
    """The restated sparse stage on the device run's pairs (its RANSAC F and inliers): SparseTriangulation with the oracle's
    extend_tracks, ref_pose.find_projection_matrix and recover_pose (fed with the device generator's stream)."""
    st = rp.SparseTriangulation(3, [(size, size)] * 3, [K] * 3, oracle.extend_tracks)
    for (i, j), e in sorted(out["pairs"]["pairs"].items()):
        if e["f"] is not None:
            wp2, wscore = st.add_image_pair_sparse(i, j, e["f"], e["inliers"])
            p2, score, _ = out["sparse"][(i, j)]
            assert score == wscore and np.allclose(p2, wp2, rtol=1e-9, atol=1e-9), (i, j)
    assert np.array_equal(out["sparse_tracks"], st.tracks)
    order, calls = [], 0
    while True:  # recover_camera_poses passes seed + the number of earlier calls
        placed = st.recover_next_cameras(seed=seed + calls)
        calls += 1
        if not placed:
            break
        order.extend(placed)
    return st, order


def _similarity_error(points, truth):
    mp, mt = points.mean(0), truth.mean(0)
    a, b = points - mp, truth - mt
    u, sv, vt = np.linalg.svd(b.T @ a)
    d = np.sign(np.linalg.det(u @ vt))
    S = np.diag([1.0, 1.0, d])
    R = u @ S @ vt
    s = (sv * np.diag(S)).sum() / (a ** 2).sum()
    aligned = s * a @ R.T + mt
    return np.abs(aligned[:, 2] - truth[:, 2]) / truth[:, 2]


def _truth_points(tracks, K, size):
    """The scene point behind each track's view-0 pixel (synth's depth bump; camera 0 is the identity)."""
    x, y = tracks[:, 0, 0].astype(np.float64), tracks[:, 0, 1].astype(np.float64)
    z = synth._sfm_depth(x, y, size)
    return ((np.linalg.inv(K) @ np.stack([x, y, np.ones_like(x)])) * z).T


def test_recover_pose_512_matches_restatement(gpu_device, oracle):
    """Config 5 at 512^2 through reconstruct_perspective (no bundle adjustment) against the restated sparse stage on the
    same pairs: the same find_projection_matrix result per pair, the same sparse track table, the same order; then the
    third camera's cvhip_recover_pose fed with the DEVICE's table and points against ref_pose.recover_pose on the same
    inputs: the same winner (batch, hypothesis, root), count and batches, error, r, t and projection to 1e-9.  A second call
    gives the same bits."""
    size = 512
    views, K, poses = synth.make_sfm_views(size)
    steps = synth.optimal_scale_steps(size, size)
    pyrs = [synth.box_pyramid(v, steps) for v in views]
    pairs = reconstruction.reconstruct_pairs(gpu_device, pyrs, dense=False, seed=3)
    out = reconstruction.reconstruct_perspective(gpu_device, pyrs, K, bundle_adjustment=False, seed=3, pairs_result=pairs)
    st, order = _sparse_restatement(oracle, out, K, size, 3)
    assert out["camera_order"] == order and tuple(order[:2]) == out["initial_pair"]
    # the driver alone: the device's table after the initial pair, both implementations on identical inputs
    tri = triangulation.PerspectiveTriangulation(3, [(size, size)] * 3, bundle_adjustment=False, calibration=[K] * 3)
    for (i, j), e in sorted(pairs["pairs"].items()):
        tri.add_image_pair_sparse(gpu_device, i, j, e["f"], e["inliers"])
    tri.recover_next_cameras(gpu_device)
    image = tri.remaining_images[-1]
    snapshot = (tri.tracks.copy(), tri.points.copy(), tri.points_ok.copy(), list(tri.projections), list(tri.cameras))
    runs = []
    for _ in range(2):
        tri.tracks, tri.points, tri.points_ok = snapshot[0].copy(), snapshot[1].copy(), snapshot[2].copy()
        tri.projections, tri.cameras, tri.remaining_images = list(snapshot[3]), list(snapshot[4]), [image]
        assert tri.recover_next_cameras(gpu_device, seed=5) == [image]
        runs.append(tri.last_pose)
    a, b = runs
    assert a["winner"] == b["winner"] and a["count"] == b["count"] and a["error"] == b["error"]
    assert np.array_equal(a["projection"], b["projection"]) and np.array_equal(a["r"], b["r"])
    want = rp.recover_pose(snapshot[0], snapshot[1], snapshot[2], snapshot[3], image, K, size, 5)
    print("512^2 third camera", image, a["winner"], a["count"], a["linked"], a["batches"], "restated", want["winner"],
          want["count"], want["batches"])
    assert a["linked"] == want["linked"] and a["winner"] == want["winner"]
    assert a["count"] == want["count"] and a["batches"] == want["batches"]
    assert np.isclose(a["error"], want["error"], rtol=1e-9, atol=0)
    r, t, P = want["camera"]
    assert np.allclose(a["r"], r, rtol=1e-9, atol=1e-12) and np.allclose(a["t"], t, rtol=1e-9, atol=1e-12)
    assert np.allclose(a["projection"], P, rtol=1e-9, atol=1e-9)


def test_reconstruct_perspective_512_bundle_adjustment_matches_restatement(gpu_device, oracle):
    """bundle_adjustment=True at 512^2: the surface of cvhip_triangulate_perspective_cameras (the initial pair's cameras
    from find_projection_matrix, the third camera's P3P projection K [matrix_r(r) | t]) against
    ref_triangulation's triangulate_and_filter + BundleAdjustment fed with the restatement's recovered cameras and
    projections, at the tolerances of test_sfm3_surface_512_matches_restatement: the same kept set and accept / reject
    history, the final residual norm to 1e-6, points and cameras to 1e-4."""
    size = 512
    views, K, poses = synth.make_sfm_views(size)
    steps = synth.optimal_scale_steps(size, size)
    pyrs = [synth.box_pyramid(v, steps) for v in views]
    pairs = reconstruction.reconstruct_pairs(gpu_device, pyrs, dense=False, seed=3)
    out = reconstruction.reconstruct_perspective(gpu_device, pyrs, K, bundle_adjustment=True, seed=3, pairs_result=pairs)
    st, order = _sparse_restatement(oracle, out, K, size, 3)
    keep = [i for i in range(3) if st.projections[i] is not None]
    for i in keep:
        assert np.allclose(out["projections"][i], st.projections[i], rtol=1e-9, atol=1e-9), i
    table = out["tracks"]
    surf = out["surface"]
    cams = [st.cameras[i].copy() for i in keep]
    idx, pts = rt.triangulate_and_filter(table, cams, [st.projections[i] for i in keep])
    ba = rt.BundleAdjustment(cams, np.asarray(table)[idx], pts)
    rcams = ba.optimize()
    assert np.array_equal(surf.track_index, idx)
    assert surf.ba_history == [int(h) for h in ba.history]
    assert abs(surf.ba_residual_norms[1] - ba.final_residual_norm) <= 1e-6 * ba.final_residual_norm
    rel = np.linalg.norm(surf.points - ba.points, axis=1) / np.linalg.norm(ba.points, axis=1)
    assert (rel <= 1e-4).all(), rel.max()
    for dc, rc in zip(surf.cameras, rcams):
        assert np.allclose(dc.r, rc.r, rtol=1e-4, atol=1e-12) and np.allclose(dc.t, rc.t, rtol=1e-4, atol=1e-12)


def test_reconstruct_perspective_2048(gpu_device):
    """Config 5 at 2048^2, no bundle adjustment: find_projection_matrix per pair equal to the restatement on the device's
    short tracks; the order is the initial pair, then the third view; the initial pair's rotation against the truth and
    its translation direction; the third camera's count at the early-exit level; the surface's depth error against synth
    after a similarity alignment.  Bounds: DESIGN.md 4.9."""
    size = 2048
    views, K, poses = synth.make_sfm_views(size)
    steps = synth.optimal_scale_steps(size, size)
    pyrs = [synth.box_pyramid(v, steps) for v in views]
    out = reconstruction.reconstruct_perspective(gpu_device, pyrs, K, bundle_adjustment=False, seed=3)
    for (i, j), (p2, score, short) in out["sparse"].items():
        e = out["pairs"]["pairs"][(i, j)]
        wp2, wscore, _ = rp.find_projection_matrix(e["f"], K, K, short)
        assert score == wscore and np.allclose(p2, wp2, rtol=1e-9, atol=1e-9), (i, j)
    i1, i2 = out["initial_pair"]
    assert out["camera_order"][:2] == [i1, i2] and sorted(out["camera_order"]) == [0, 1, 2]
    p2 = out["sparse"][(i1, i2)][0]
    R_rel = poses[i2][0] @ poses[i1][0].T
    t_rel = poses[i2][1] - R_rel @ poses[i1][1]
    rot_err = np.linalg.norm(p2[:, :3] - R_rel)
    cos_t = abs(p2[:, 3] @ t_rel) / np.linalg.norm(t_rel) / np.linalg.norm(p2[:, 3])
    third = [p for p in out["poses"] if p.get("images") and len(p["images"]) == 1][0]
    surf = out["surface"]
    err = np.array([np.nan])
    if i1 == 0:
        err = _similarity_error(surf.points, _truth_points(surf.tracks, K, size))
    print(f"2048^2: order {out['camera_order']}, rotation error {rot_err:.3e}, |cos t| {cos_t:.9f}, third {third['count']} of "
          f"{third['linked']} in {third['batches']} batch(es), {len(surf.points)} points, median depth error "
          f"{np.nanmedian(err):.4f}, timings {out['timings_ms']}")
    # find_projection_matrix equals the restatement above, so these are the restatement's values on this scene (measured
    # 3.46e-3, 0.99864 and 4.9 %: the RANSAC F's deviation from the planted one), with a 1.5x margin
    assert rot_err < 5.2e-3
    assert cos_t > 0.998
    assert third["count"] >= rp.RANSAC_D_PERCENT_EARLY_EXIT * third["linked"] // 100
    assert i1 != 0 or np.median(err) < 0.074


def test_find_projection_matrix_with_two_calibrations(gpu_device):
    """cvhip_find_projection_matrix with K1 != K2 on every ordered pair (i, j) of a 3-camera mixed scene (3000 tracks, a
    K and an image size per camera) and the pair's two-K true F, as test_find_projection_matrix_matches_restatement
    compares: the restatement's score, the runner-up strictly lower, out_P2 and out_r2 to 1e-9 - and out_KP2 against
    K_j P2.  E = K2^T F K1: with the two K exchanged the restatement finds another winner or a strictly lower score on
    every one of these pairs (tests/test_pose_ref.py), which one shared K cannot show."""
    import ctypes as C

    tracks, Ks, poses, _, _ = pose_scenes.mixed_multiview_scene(3, 3000, seed=3, miss=0.0)
    for i, j in [(0, 1), (1, 0), (0, 2), (2, 0), (1, 2), (2, 1)]:
        F = np.ascontiguousarray(mixed_scenes.true_f(Ks[i], Ks[j], poses[i], poses[j]))
        short = np.ascontiguousarray(tracks[:, [i, j]])
        k1, k2 = np.ascontiguousarray(Ks[i]), np.ascontiguousarray(Ks[j])
        p2, r2, kp2 = np.zeros((3, 4)), np.zeros(3), np.zeros((3, 4))
        score = C.c_double(0)
        _lib.check(_lib.lib().cvhip_find_projection_matrix(gpu_device.handle, _p(F), _p(k1), _p(k2), _p(short), len(short),
                                                           _p(p2), C.byref(score), _p(r2), _p(kp2)), "fpm")
        wp2, wcount, counts = rp.find_projection_matrix(F, k1, k2, short)
        assert score.value == wcount and sorted(counts)[-2] < wcount, (i, j)
        assert np.allclose(p2, wp2, rtol=1e-9, atol=1e-9), (i, j)
        assert np.allclose(r2, rt.Camera.from_matrix(k2, p2[:, :3], p2[:, 3]).r, rtol=1e-9, atol=1e-12), (i, j)
        assert np.allclose(kp2, k2 @ wp2, rtol=1e-9, atol=1e-9), (i, j)
