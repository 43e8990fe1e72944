"""The CPU restatement of the perspective triangulation stage (tests/ref_triangulation.py) on its own: DLT recovery, the
Rodrigues round trip of Camera::from_matrix and the bundle adjustment's behaviour as the reference writes it."""
import math

import numpy as np
import pytest

import ref_triangulation as rt
import tri_scenes


def test_dlt_recovers_noise_free_points():
    """triangulate_track (triangulation.rs:867-911) on exact (float) projections: the points come back to ~1e-9."""
    from cybervision_amd import synth

    K, poses = synth.sfm_cameras(2048)
    cams = [rt.Camera.from_matrix(K, R, t) for R, t in poses]
    P = np.stack([c.projection() for c in cams])
    rng = np.random.default_rng(3)
    X = np.stack([rng.uniform(-0.4, 0.4, 2000), rng.uniform(-0.4, 0.4, 2000), rng.uniform(0.85, 1.0, 2000)], axis=1)
    tracks = np.zeros((2000, 3, 2))
    for j in range(3):
        q = X @ P[j][:, :3].T + P[j][:, 3]
        tracks[:, j] = q[:, :2] / q[:, 2:3]
    tracks[:500, 2] = -1.0  # two views only
    pts, ok, _ = rt.triangulate_tracks(tracks, P)
    assert ok.all()
    rel = np.linalg.norm(pts - X, axis=1) / np.linalg.norm(X, axis=1)
    assert rel.max() < 1e-9, rel.max()


AXES = [(0, 0, 1), (1, 0, 0), (0, 1, 0), (1, 1, 0), (1, -2, 3), (0, -1, 1)]
# 180 degrees only about axes whose matrix_r is exactly symmetric in f64 (s = 0): elsewhere s is ~1e-16, not below
# f64::EPSILON, and the reference's general branch divides rounding noise by it - no axis to recover
CASES = [(a, t) for a in AXES for t in (0.0, 1e-3, 0.7, 2.5)] + [(a, math.pi) for a in AXES[:4]]


@pytest.mark.parametrize("axis,angle", CASES)
def test_from_matrix_of_matrix_r(axis, angle):
    """Camera::from_matrix (:414-466) of matrix_r(theta u) (:475-485).  As the reference writes it, rho (:419-423) is the
    DIFFERENCE a21 - a12 = 2 sin(theta) u, so the axis comes back but the angle is atan2(2 sin(theta), cos(theta)): the
    round trip is exact at 0 and at 180 degrees (the branch of :433-461 and its sign convention), not in between."""
    u = np.asarray(axis, dtype=np.float64)
    u = u / np.linalg.norm(u)
    R = rt.matrix_r(u * angle)
    cam = rt.Camera.from_matrix(np.eye(3), R, np.zeros(3))
    if angle == 0.0:
        assert (cam.r == 0).all()
    elif angle == math.pi:
        assert abs(np.linalg.norm(cam.r) - math.pi) < 1e-12
        expected = u * math.pi
        if expected[0] < 0 or (abs(expected[0]) < rt.EPS and expected[1] < 0) or \
                (abs(expected[0]) < rt.EPS and abs(expected[1]) < rt.EPS and expected[2] < 0):
            expected = -expected
        assert np.allclose(cam.r, expected, atol=1e-12)
        assert np.allclose(rt.matrix_r(cam.r), R, atol=1e-12)
    else:
        assert np.allclose(cam.r, u * math.atan2(2.0 * math.sin(angle), math.cos(angle)), atol=1e-12)


def test_exact_180_degree_rotation_takes_its_branch():
    """diag(1, -1, -1) is exactly 180 degrees about x: s = 0 and c = -1, so from_matrix takes the branch of :433-461."""
    cam = rt.Camera.from_matrix(np.eye(3), np.diag([1.0, -1.0, -1.0]), np.zeros(3))
    assert np.allclose(cam.r, [math.pi, 0.0, 0.0], atol=0)
    assert np.allclose(rt.matrix_r(cam.r), np.diag([1.0, -1.0, -1.0]), atol=1e-15)


def test_bundle_adjustment_as_written_reaches_found_without_raising_the_residual():
    """BundleAdjustment::optimize (:2042-2147) on a perturbed scene: it reaches "found" and never raises the residual.
    As the reference writes it the step is ADDED (update_params, :2012-2040) although delta = (J^T J + mu I)^-1 J^T r with
    r = projected - observed (:1781-1786) points uphill, so every step is rejected and mu grows until the delta test
    (:2079-2083) ends the loop - the surface keeps the input points and cameras.  The same loop with the step's sign
    turned does lower the residual, which is what pins the diagnosis."""
    _, pert, tracks = tri_scenes.ba_scene(1500)
    cams = tri_scenes.ref_cameras(pert)
    idx, pts = rt.triangulate_and_filter(tracks, cams, [rt.given_projection(*c) for c in pert])
    assert len(idx) > 1000
    ba = rt.BundleAdjustment(cams, tracks[idx], pts)
    before = ba.residual_norm_squared()
    ba.optimize()
    assert ba.final_residual_norm ** 2 <= before
    assert len(ba.history) > 0 and not any(ba.history)  # all rejected
    assert np.array_equal(ba.points, pts)

    turned = rt.BundleAdjustment(cams, tracks[idx], pts)
    step = turned.delta_step

    def downhill():
        da, db = step()
        return -da, -db

    turned.delta_step = downhill
    try:
        turned.optimize()
    except rt.TriangulationError:
        pass  # (100 iterations are not always enough for the turned loop; only its residual matters here)
    assert any(turned.history)
    assert turned.residual_norm_squared() < 0.5 * before


SCENE_CASES = tri_scenes.BA_RIG_CASES + [tri_scenes.BA_GRID_CASE] + tri_scenes.BA_MIXED_CASES


@pytest.mark.parametrize("case", SCENE_CASES,
                         ids=lambda c: f"m{c[0]}-n{c[1]}-seed{c[2]}" + ("-mixed" if isinstance(c, tri_scenes.MixedCase) else ""))
def test_ba_scene_claims(case, monkeypatch):
    """What the device tests rely on for each bundle-adjustment scene: no track's DLT / filter decision lies within 1e-9
    of its threshold, the restatement reaches "found", every V it pseudo-inverts keeps its singular values far above the
    f64::EPSILON cut-off, the history has accepted steps exactly where the case claims
    them, every rho is at least RHO_MARGIN away from 0, the grid-stride case keeps more than 1024 * 256 tracks, and - so that the device's other summation order
    cannot tip any decision - the restatement with its reductions over the kept tracks in reversed order gives the same
    accept / reject sequence, with points, cameras and residual norm within a fifth of the device test's bound."""
    m, n, seed, far, accepts = case
    _, given, tracks = tri_scenes.ba_case_scene(case)
    close = tri_scenes.near_threshold(tracks, given)
    assert len(close) == 0, f"tracks at a threshold: {close[:20].tolist()}"
    smallest = []  # the smallest singular value of every V the loop pseudo-inverts (:1797)
    pinv3 = rt._pinv3

    def recording_pinv3(v):
        smallest.append(float(np.linalg.svd(v, compute_uv=False)[:, -1].min()))
        return pinv3(v)

    monkeypatch.setattr(rt, "_pinv3", recording_pinv3)
    idx, pts, cams, ba = tri_scenes.ba_restatement(given, tracks)  # raises unless "found"
    monkeypatch.setattr(rt, "_pinv3", pinv3)
    # the f64::EPSILON cut-off never engages, so the device's adjugate inverse is the pseudo-inverse
    assert min(smallest) > 1e6 * rt.EPS, min(smallest)
    assert any(ba.history) == accepts, ba.history
    assert min(abs(r) for r in ba.rhos) >= tri_scenes.RHO_MARGIN, ba.rhos
    if case == tri_scenes.BA_GRID_CASE:
        assert len(idx) > tri_scenes.GRID_STRIDE_TRACKS
    tol, tol_res = 1e-6, 1e-9  # the device test's bounds
    _, rpts, rcams, rba = tri_scenes.ba_restatement(given, tracks, order=np.arange(len(idx))[::-1])
    assert rba.history == ba.history
    assert abs(rba.final_residual_norm - ba.final_residual_norm) <= 0.2 * tol_res * ba.final_residual_norm
    rel = np.linalg.norm(rpts - pts, axis=1) / np.linalg.norm(pts, axis=1)
    assert rel.max() <= 0.2 * tol, rel.max()
    for a, b in zip(rcams, cams):
        assert tri_scenes.vec_close(a.r, b.r, 0.2 * tol, 1e-12) and tri_scenes.vec_close(a.t, b.t, 0.2 * tol, 1e-12)
        assert tri_scenes.vec_close(a.projection(), b.projection(), 0.2 * tol, 1e-9)


@pytest.mark.parametrize("case", tri_scenes.BA_MIXED_CASES, ids=lambda c: f"m{c[0]}-n{c[1]}-seed{c[2]}-mixed")
def test_ba_mixed_scene_keeps_its_history_however_v_is_inverted(case, monkeypatch):
    """A further claim for the mixed bundle-adjustment scenes (tri_scenes.BA_MIXED_CASES says why): with V inverted as the
    device inverts it - adjugate over determinant - in place of the SVD pseudo-inverse, the restatement runs the same
    accept / reject sequence, every rho stays RHO_MARGIN away from 0, and points, cameras and the residual norm stay
    within a fifth of the device test's bounds."""
    _, given, tracks = tri_scenes.ba_case_scene(case)
    idx, pts, cams, ba = tri_scenes.ba_restatement(given, tracks)
    monkeypatch.setattr(rt, "_pinv3", tri_scenes.adjugate_inverse)
    _, apts, acams, aba = tri_scenes.ba_restatement(given, tracks)
    assert aba.history == ba.history, (aba.history, aba.rhos)
    assert min(abs(r) for r in aba.rhos) >= tri_scenes.RHO_MARGIN, aba.rhos
    tol, tol_res = 1e-6, 1e-9
    assert abs(aba.final_residual_norm - ba.final_residual_norm) <= 0.2 * tol_res * ba.final_residual_norm
    assert (np.linalg.norm(apts - pts, axis=1) <= 0.2 * tol * np.linalg.norm(pts, axis=1)).all()
    for a, b in zip(acams, cams):
        assert tri_scenes.vec_close(a.r, b.r, 0.2 * tol, 1e-12) and tri_scenes.vec_close(a.t, b.t, 0.2 * tol, 1e-12)
        assert tri_scenes.vec_close(a.projection(), b.projection(), 0.2 * tol, 1e-9)


# ---- the mixed rig (tests/mixed_scenes.py): what the device tests on it rely on, and what they can tell apart -------------
def test_mixed_calibrations_are_general_and_all_different():
    """Every K of the mixed rig has fx != fy (ratio 0.8 or 1.25), skew of ~1.5 % of fx with either sign among the first
    two, a principal point off the centre by a different (signed) number of pixels in x and y, last row (0, 0, 1); no two K and no two image
    sizes are alike, and landscape and portrait both occur among the first three."""
    import mixed_scenes

    Ks = mixed_scenes.calibrations(mixed_scenes.DIMS)
    for j, (K, (w, h)) in enumerate(zip(Ks, mixed_scenes.DIMS)):
        assert K[1, 1] / K[0, 0] == pytest.approx(1.25 if j % 2 else 0.8) and abs(K[0, 1]) == pytest.approx(0.015 * K[0, 0])
        assert (K[0, 1] < 0) == bool(j % 2) and K[1, 0] == 0.0 and K[2].tolist() == [0.0, 0.0, 1.0]
        dx, dy = K[0, 2] - w / 2.0, K[1, 2] - h / 2.0
        assert dx != dy and dx != 0.0 and dy != 0.0 and K[0, 2] != K[1, 2]
    assert len({K.tobytes() for K in Ks}) == 8 and len(set(mixed_scenes.DIMS)) == 8
    assert len({(w, h) for w, h in mixed_scenes.DIMS} & {(h, w) for w, h in mixed_scenes.DIMS if w != h}) >= 4
    shapes = [w > h for w, h in mixed_scenes.DIMS[:3]]
    assert any(shapes) and not all(shapes)
    # rig's poses and track tables are what they were
    for a, b in zip(tri_scenes.rig(8), tri_scenes.mixed_rig(8)):
        assert np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])


def _with_k(cams, change):
    return [(change(j, K), R, t) for j, (K, R, t) in enumerate(cams)]


@pytest.mark.parametrize("m", [2, 3, 8])
def test_mixed_rig_table_claims(m):
    """What test_triangulate_and_filter_match_restatement_on_the_mixed_rig relies on: no track at a threshold, 30 % to
    90 % of the tracks kept, 1-view tracks present.  And what the scene tells apart - each of these changes of the
    cameras given to the restatement, which one shared symmetric K would hide, moves the kept points by far more than the
    device test's 1e-9 (and changes the kept set or not): every camera with camera 0's K; K[0][1] and K[1][0] exchanged
    (the skew read from the other side of the diagonal); fx and fy exchanged; cx and cy exchanged."""
    cams = tri_scenes.mixed_rig(m, near_duplicate=m > 2)
    tracks = tri_scenes.track_table(cams, 20_000, seed=m)
    assert len(tri_scenes.near_threshold(tracks, cams)) == 0
    idx, pts, _, _ = rt.triangulate_all(tracks, cams, bundle_adjustment=False)
    k = (tracks[..., 0] >= 0).sum(axis=1)
    assert (k < 2).any() and 0.3 * len(tracks) < len(idx) < 0.9 * len(tracks)
    print(f"m={m}: {len(idx)} of {len(tracks)} kept")

    def swap(a, b):
        def change(j, K):
            K = K.copy()
            K[a], K[b] = K[b], K[a]
            return K
        return change

    k0 = cams[0][0]
    for name, change in (("camera 0's K for every camera", lambda j, K: k0), ("K[1] read for K[3]", swap((0, 1), (1, 0))),
                         ("fx and fy exchanged", swap((0, 0), (1, 1))), ("cx and cy exchanged", swap((0, 2), (1, 2)))):
        idx2, pts2, _, _ = rt.triangulate_all(tracks, _with_k(cams, change), bundle_adjustment=False)
        both = np.intersect1d(idx, idx2)
        a, b = pts[np.searchsorted(idx, both)], pts2[np.searchsorted(idx2, both)]
        moved = np.linalg.norm(a - b, axis=1) / np.linalg.norm(a, axis=1)
        assert not np.array_equal(idx, idx2) or moved.max() > 1e-3, name
        assert len(both) == 0 or moved.max() > 1e-3, (name, moved.max())


def test_mixed_p3p_case_claims():
    """test_perspective_cameras_on_the_mixed_rig's scene: no track at a threshold with the P3P-style projections, 30 % to
    90 % kept, and the projections are not K [R | t] of the given matrices - the DLT with those keeps other points."""
    given, cams, P, tracks = tri_scenes.mixed_p3p_case()
    assert len(tri_scenes.near_threshold(tracks, given, projections=P)) == 0
    idx, pts = rt.triangulate_and_filter(tracks, cams, P)
    assert 0.3 * len(tracks) < len(idx) < 0.9 * len(tracks)
    idx2, pts2 = rt.triangulate_and_filter(tracks, cams, [rt.given_projection(*c) for c in given])
    assert not np.array_equal(idx, idx2) or np.abs(pts - pts2).max() > 1e-3
