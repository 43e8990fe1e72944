"""Analytic scenes for the perspective triangulation tests: cameras (K, R, t) and integer track tables that exercise every
branch of triangulate_track / filter_outliers (triangulation.rs:867-911, 1559-1593)."""
from __future__ import annotations

import math

import numpy as np

import mixed_scenes
import ref_triangulation as rt


def rot_y(a):
    c, s = math.cos(a), math.sin(a)
    return np.array([[c, 0.0, s], [0.0, 1.0, 0.0], [-s, 0.0, c]])


def rig(m, size=2048, near_duplicate=True):
    """m cameras [(K, R, t)] looking at (0, 0, 5): camera 0 at the origin (R = I); camera 1 with R = I too, 0.01 to the
    side (near-duplicate: its rays and camera 0's are within 0.5 degrees at the scene) or 0.5 when near_duplicate is off;
    the others on an arc of radius 5 around the scene centre, 12 to 40 degrees to either side."""
    f = 0.5 * size
    K = np.array([[f, 0.0, size / 2.0], [0.0, f, size / 2.0], [0.0, 0.0, 1.0]])
    cams = [(K, np.eye(3), np.zeros(3)), (K, np.eye(3), np.array([-0.01 if near_duplicate else -0.5, 0.0, 0.0]))]
    for j in range(2, m):
        theta = math.radians((12.0 + 28.0 * (j - 2) / max(m - 3, 1)) * (1 if j % 2 else -1))
        C = np.array([5.0 * math.sin(theta), 0.2 * (j % 3 - 1), 5.0 - 5.0 * math.cos(theta)])
        R = rot_y(-theta)
        cams.append((K, R, -R @ C))
    return cams


def mixed_rig(m, near_duplicate=True):
    """rig(m)'s poses with mixed_scenes' cameras: camera j has its own K (fx != fy, skew, an off-centre principal point)
    for its own image size mixed_scenes.DIMS[j] - the scene centre still projects near the middle of every image."""
    return [(mixed_scenes.calibration(j, mixed_scenes.DIMS[j]), R, t)
            for j, (_, R, t) in enumerate(rig(m, near_duplicate=near_duplicate))]


def project(cam, X):
    K, R, t = cam
    q = (X @ R.T + t) @ K.T
    return q[:, :2] / q[:, 2:3]


def observe(cams, X, mask):
    """Rounded projections where mask (and the projection is a valid non-negative pixel), else (-1, -1)."""
    n, m = len(X), len(cams)
    out = np.full((n, m, 2), -1, dtype=np.int32)
    for j, cam in enumerate(cams):
        with np.errstate(all="ignore"):
            p = np.round(project(cam, X))
        good = mask[:, j] & np.all(np.isfinite(p), axis=1) & np.all((p >= 0) & (p < 1e6), axis=1)
        out[good, j] = p[good].astype(np.int32)
    return out


def track_table(cams, n, seed):
    """~n tracks: 60 % regular points seen in a random subset of >= 2 views, 10 % seen in one view only, 10 % the same
    pixel in cameras 0 and 1 (parallel rays: |w| ~ 0), 10 % scattered through a large box (many behind a camera),
    10 % seen by cameras 0 and 1 only (near-duplicate views: the ray-angle test).  Rows shuffled."""
    rng = np.random.default_rng(seed)
    m = len(cams)
    parts = []
    n_reg = int(0.6 * n)
    X = np.stack([rng.uniform(-1.5, 1.5, n_reg), rng.uniform(-1.5, 1.5, n_reg), rng.uniform(3.5, 6.5, n_reg)], axis=1)
    mask = rng.random((n_reg, m)) < 0.7
    mask[np.arange(n_reg), rng.integers(0, m, n_reg)] = True
    mask[np.arange(n_reg), (rng.integers(1, m, n_reg) + rng.integers(0, m, n_reg)) % m] = True
    parts.append(observe(cams, X, mask))
    n10 = n // 10
    X = np.stack([rng.uniform(-1.5, 1.5, n10), rng.uniform(-1.5, 1.5, n10), rng.uniform(3.5, 6.5, n10)], axis=1)
    mask = np.zeros((n10, m), dtype=bool)
    mask[np.arange(n10), rng.integers(0, m, n10)] = True
    parts.append(observe(cams, X, mask))
    pix = np.stack([rng.integers(0, 2048, n10), rng.integers(0, 2048, n10)], axis=1).astype(np.int32)
    t = np.full((n10, m, 2), -1, dtype=np.int32)
    t[:, 0] = pix
    t[:, 1] = pix
    parts.append(t)
    X = np.stack([rng.uniform(-8, 8, n10), rng.uniform(-3, 3, n10), rng.uniform(-4, 10, n10)], axis=1)
    parts.append(observe(cams, X, np.ones((n10, m), dtype=bool)))
    X = np.stack([rng.uniform(-1.5, 1.5, n10), rng.uniform(-1.5, 1.5, n10), rng.uniform(3.5, 6.5, n10)], axis=1)
    mask = np.zeros((n10, m), dtype=bool)
    mask[:, :2] = True
    parts.append(observe(cams, X, mask))
    table = np.concatenate(parts)
    return np.ascontiguousarray(table[rng.permutation(len(table))])


def ref_cameras(cams):
    return [rt.Camera.from_matrix(K, R, t) for K, R, t in cams]


def near_threshold(tracks, cams, tol=1e-9, projections=None):
    """Rows whose deciding quantity lies within tol (relative) of its threshold: |w| vs 1e-4, the smallest depth of a seen
    view vs 0, the smallest |cos| between rays vs cos(0.5 deg).  projections: what the DLT projects with, when it is not
    K [R | t] as given."""
    rc = ref_cameras(cams)
    P = np.stack([rt.given_projection(*c) for c in cams]) if projections is None else np.asarray(projections)
    pts, ok, w_abs = rt.triangulate_tracks(tracks, P)
    _, depth_min, min_cos = rt.filter_decisions(tracks, pts, ok, rc)
    thr = math.cos(rt.MIN_ANGLE_BETWEEN_RAYS)
    close = np.abs(w_abs - rt.PERSPECTIVE_SCALE_THRESHOLD) <= tol * rt.PERSPECTIVE_SCALE_THRESHOLD
    close |= ok & (np.abs(depth_min) <= tol * np.maximum(1.0, np.linalg.norm(np.where(ok[:, None], pts, 0.0), axis=1)))
    close |= ok & (np.abs(min_cos - thr) <= tol)
    return np.nonzero(close)[0]


def ba_scene(n, seed=5, size=2048):
    """n tracks over synth.sfm_cameras-like cameras (3 views), every track seen in 2 or 3 views with integer (so
    sub-pixel-noisy) observations, and the cameras 2 and 3 perturbed by ~1e-3 in r and t.  -> (true cams, perturbed
    cams, tracks)."""
    from cybervision_amd import synth

    rng = np.random.default_rng(seed)
    K, poses = synth.sfm_cameras(size)
    cams = [(K, R, t) for R, t in poses]
    X = np.stack([rng.uniform(-0.4, 0.4, n), rng.uniform(-0.4, 0.4, n), rng.uniform(0.85, 1.0, n)], axis=1)
    mask = np.ones((n, 3), dtype=bool)
    mask[np.arange(n), rng.integers(0, 3, n)] = rng.random(n) < 0.5
    tracks = observe(cams, X, mask)
    pert = [cams[0]]
    for K_, R, t in cams[1:]:
        dR = rt.matrix_r(rng.normal(0.0, 1e-3, 3))
        pert.append((K_, dR @ R, t + rng.normal(0.0, 1e-3, 3)))
    return cams, pert, tracks


def ba_rig_scene(m, n, seed, perturb=True, far=0.1, mixed=False):
    """n tracks over rig(m, near_duplicate=False) (no camera pair the ray-angle test drops whole; with `mixed`,
    mixed_rig's cameras: the same poses, a K per camera): points of the box
    [-1.5, 1.5]^2 x [3.5, 6.5], a fraction `far` of them scattered through track_table's large box instead (some far
    or behind a camera: the tracks that can make the reference's uphill first step land lower), each seen in a uniform
    number of 2..m views (a random subset; the others (-1, -1)) with integer observations; with perturb, the cameras
    1..m-1 perturbed by ~1e-3 in r and t as ba_scene's.  -> (true cams, cams given to the triangulation, tracks)."""
    rng = np.random.default_rng(seed)
    cams = mixed_rig(m, near_duplicate=False) if mixed else rig(m, near_duplicate=False)
    n_far = int(far * n)
    X = np.stack([rng.uniform(-1.5, 1.5, n), rng.uniform(-1.5, 1.5, n), rng.uniform(3.5, 6.5, n)], axis=1)
    X[:n_far] = np.stack([rng.uniform(-8, 8, n_far), rng.uniform(-3, 3, n_far), rng.uniform(-4, 10, n_far)], axis=1)
    k = rng.integers(2, m + 1, n)
    order = np.argsort(rng.random((n, m)), axis=1)
    mask = np.zeros((n, m), dtype=bool)
    np.put_along_axis(mask, order, np.arange(m)[None, :] < k[:, None], axis=1)
    tracks = observe(cams, X, mask)
    given = [cams[0]]
    for K, R, t in cams[1:]:
        if perturb:
            dR = rt.matrix_r(rng.normal(0.0, 1e-3, 3))
            given.append((K, dR @ R, t + rng.normal(0.0, 1e-3, 3)))
        else:
            given.append((K, R, t))
    return cams, given, np.ascontiguousarray(tracks[rng.permutation(n)])


# The bundle-adjustment scenes of tests/test_triangulation_gpu.py, (m, n, seed, far, accepts): ba_rig_scene(m, n, seed,
# far=far), and whether its LM history holds accepted steps.  Seeds picked on the CPU; tests/test_triangulation_ref.py
# checks each scene's claims.  Every scene here is all-rejected: no scene tried has an accepted step that the
# restatement reproduces when only its rounding changes (reductions in reversed track order, or V inverted by
# np.linalg.inv instead of the SVD pseudo-inverse) - the history itself changes, or the points move by O(1).  Tried:
# ba_rig_scene with m = 2..8, seeds 1..16, far 0 / 0.01 / 0.02 / 0.03 / 0.05 / 0.1, n = 20 k and 270 k; rig(m,
# near_duplicate=False) with track_table(cams, 20 k, seed), true cameras, m = 3..8, seeds 1, 2, 3, 5, 8 (among them the
# 8-camera seed-8 scene with 3 accepts: reversed order moves its points by 54x their norm); rig sizes 16, 64, 256.  The
# accepts come from tracks whose V is ill-conditioned (condition numbers up to 4.5e12) and, with 4 or more cameras, from
# S + mu I solved at mu = 1e-3 against entries ~1e10 in its near-null directions.
BA_RIG_CASES = [
    (2, 20_000, 11, 0.0, False),
    (3, 20_000, 3, 0.0, False),
    (4, 20_000, 1, 0.0, False),
    (5, 20_000, 8, 0.0, False),
    (6, 20_000, 1, 0.1, False),
    (7, 20_000, 3, 0.0, False),
    (8, 20_000, 5, 0.0, False),
]


class MixedCase(tuple):
    """A case (m, n, seed, far, accepts) of ba_rig_scene(..., mixed=True): mixed_rig's cameras."""


# The bundle-adjustment scenes on mixed_rig, n = 6000, picked on the CPU like BA_RIG_CASES; tests/test_triangulation_ref.py
# checks their claims with the same test.  All-rejected, like every scene above.  Tried with mixed cameras, far = 0,
# n = 6000: m = 2, seeds 1..32 - all rejected everywhere, but the smallest |rho| is below RHO_MARGIN (0.002 .. 0.0999) except
# for seeds 12 (0.109) and 30 (0.179); m = 3, seeds 1..8 - seeds 1, 3, 4, 5, 7, 8 qualify (seed 4: every rho is 1), seeds 2
# and 6 have a rho ~1e-3.
# m >= 5 (the second camera group of ba_jtr_kernel), seeds 1..16 x far 0 / 0.01 / 0.05 / 0.1 at n = 6000: no scene has an
# accepted step, and 26 of the 256 pass test_ba_scene_claims as all-rejected scenes (the others miss RHO_MARGIN or change
# under reversed order).  That test does not suffice here: on the mixed rig with 5 or more cameras some track's V (summed
# over every view, seen or not) has a condition number of 1e14 .. 1e17, and the restatement's rhos then follow the way V
# is inverted - the SVD pseudo-inverse, or the device's adjugate / determinant (adjugate_inverse below).  m = 5 seed 1
# (smallest |rho| 0.139, condition 3.8e15) passes every claim of test_ba_scene_claims, yet with the adjugate the
# restatement itself accepts steps 6 and 10 and runs 22 iterations for 14; the device accepted steps 4 and 8 of 21.
# m = 5 seed 11 at n = 20 k and m = 7 seed 3 change their history the same way.  So a mixed scene must also keep its
# history under adjugate_inverse (test_ba_mixed_scene_keeps_its_history_however_v_is_inverted); m = 6 seed 10 and
# m = 8 seed 1 do, with every rho <= -1 both ways, and are taken.  No m = 5 scene was found that does.
BA_MIXED_CASES = [
    MixedCase((2, 6000, 30, 0.0, False)),
    MixedCase((3, 6000, 4, 0.0, False)),
    MixedCase((6, 6000, 10, 0.0, False)),
    MixedCase((8, 6000, 1, 0.0, False)),
]


def adjugate_inverse(v):
    """The inverse of [..., 3, 3] symmetric matrices as the device forms it (v_inverse, csrc/triangulation_kernels.hip):
    adjugate over determinant, in its order of operations - a stand-in for ref_triangulation._pinv3."""
    v = np.asarray(v, dtype=np.float64)
    V = np.moveaxis(v.reshape(-1, 9), 1, 0)
    c00, c01, c02 = V[4] * V[8] - V[5] * V[7], V[5] * V[6] - V[3] * V[8], V[3] * V[7] - V[4] * V[6]
    inv = 1.0 / (V[0] * c00 + V[1] * c01 + V[2] * c02)
    out = np.stack([c00 * inv, (V[2] * V[7] - V[1] * V[8]) * inv, (V[1] * V[5] - V[2] * V[4]) * inv,
                    c01 * inv, (V[0] * V[8] - V[2] * V[6]) * inv, (V[2] * V[3] - V[0] * V[5]) * inv,
                    c02 * inv, (V[1] * V[6] - V[0] * V[7]) * inv, (V[0] * V[4] - V[1] * V[3]) * inv], axis=1)
    return out.reshape(v.shape)


# more than MAX_GRID (1024) blocks of 256 kept tracks: the grid-stride loops of the bundle-adjustment kernels
BA_GRID_CASE = (3, 270_000, 2, 0.0, False)
GRID_STRIDE_TRACKS = 1024 * 256
# every rho of a scene at least this far from 0: the decisions then do not hang on the rounding of rho itself (an
# all-rejected scene's rhos are O(1) or larger; a scene whose rho was 2e-3 at one step took the other branch on the device)
RHO_MARGIN = 0.1


def mixed_p3p_case(n=5000, seed=3):
    """Three mixed cameras as pose recovery leaves them, for cvhip_triangulate_perspective_cameras: the Camera that
    from_matrix makes of mixed_rig(3)'s (K_j, R, t), and ITS projection K_j [matrix_r(r) | t] - a P3P camera's; as the
    reference writes from_matrix that is a rotation by atan2(2 sin, cos) of R's angle, so the tracks are observed
    through these projections.  -> (given [(K, R, t)], cameras, projections [3, 3, 4], tracks of track_table)."""
    given = mixed_rig(3)
    cams = ref_cameras(given)
    seen_through = [(c.k, c.r_matrix, c.t) for c in cams]
    tracks = np.ascontiguousarray(track_table(seen_through, n, seed), dtype=np.int32)
    return given, cams, np.stack([c.projection() for c in cams]), tracks


def vec_close(a, b, rtol, atol):
    """max |a - b| <= rtol max |b| + atol (relative to the largest element of b)."""
    a, b = np.asarray(a), np.asarray(b)
    return float(np.abs(a - b).max()) <= rtol * float(np.abs(b).max()) + atol


def ba_case_scene(case):
    m, n, seed, far, _ = case
    return ba_rig_scene(m, n, seed, far=far, mixed=isinstance(case, MixedCase))


def ba_restatement(given, tracks, order=None):
    """triangulate_all with the bundle adjustment on, its reductions run over the kept tracks in `order` (a permutation
    of them; None = track order) -> (kept indices, points, cameras, BundleAdjustment), points in track order."""
    cams = ref_cameras(given)
    idx, pts = rt.triangulate_and_filter(tracks, cams, [rt.given_projection(*c) for c in given])
    order = np.arange(len(idx)) if order is None else np.asarray(order)
    ba = rt.BundleAdjustment(cams, np.asarray(tracks)[idx][order], pts[order])
    out = ba.optimize()
    points = np.empty_like(ba.points)
    points[order] = ba.points
    return idx, points, out, ba
