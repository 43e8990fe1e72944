"""CPU restatement (numpy, f64) of the reference's pose recovery - test infrastructure only.

Transcribes, citing zlogic/cybervision v0.20.3 src/triangulation.rs:
  - find_projection_matrix                                                    :940-994
  - recover_pose (driven by an injected sample stream), recover_pose_from_points, choose_inliers' role,
    tracks_reprojection_error, point_reprojection_error                       :1033-1210, 1296-1328
  - solve_quartic, polish_roots                                               :1595-1673
  - add_image_pair_sparse, recover_next_cameras, triangulate_tracks's bookkeeping (SparseTriangulation) :620-811
  - recover_camera_poses' loop over a SparseTriangulation                     src/reconstruction.rs:627-666
plus the device's sample generator (csrc/pose_kernels.hip draw_samples), so that the restatement can be fed the same
index stream.  Unpinned: nalgebra's SVD signs (np.linalg.svd here) - they change find_projection_matrix's candidate
order, which matters only on a tie of counts.  Nothing in cybervision_amd/ may import this module.
"""
from __future__ import annotations

import math

import numpy as np

import ref_triangulation as rt

EPS = np.finfo(np.float64).eps
RANSAC_N = 3
RANSAC_K = 100_000
RANSAC_INLIERS_T = 50.0 / 1000.0
RANSAC_T = 50.0 / 1000.0
RANSAC_D_PERCENT = 70
RANSAC_D_PERCENT_EARLY_EXIT = 95
RANSAC_CHECK_INTERVAL = 1000
M64 = (1 << 64) - 1


def mix64(z):
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def device_samples(seed, batch, h, length):
    """The device's three draws for hypothesis h of a batch (with replacement, 0..length)."""
    state = mix64((seed ^ mix64(((batch << 32) | h) & M64)) & M64)
    out = []
    for _ in range(3):
        state = mix64((state + 0x9E3779B97F4A7C15) & M64)
        out.append(((state >> 32) * length) >> 32)
    return out


def solve_quartic(h):
    """:1595-1638, NaN where Rust's powf / sqrt give NaN."""
    a, b, c, d, e = (np.float64(v) for v in h)  # (IEEE division: 0 / 0 and x / 0 as in Rust)
    with np.errstate(all="ignore"):
        a2, b2 = a * a, b * b
        a3, b3 = a2 * a, b2 * b
        a4, b4 = a3 * a, b3 * b
        alpha = -3.0 * b2 / (8.0 * a2) + c / a
        beta = b3 / (8.0 * a3) - b * c / (2.0 * a2) + d / a
        gamma = -3.0 * b4 / (256.0 * a4) + b2 * c / (16.0 * a3) - b * d / (4.0 * a2) + e / a
        al2 = alpha * alpha
        al3 = al2 * alpha
        p = -al2 / 12.0 - gamma
        q = -al3 / 108.0 + alpha * gamma / 3.0 - beta * beta / 8.0
        r = -q / 2.0 + np.sqrt(np.float64(q * q / 4.0 + p * p * p / 27.0))
        u = np.power(np.float64(r), 1.0 / 3.0)
        y = -5.0 * alpha / 6.0 - np.power(np.float64(q), 1.0 / 3.0) if abs(u) < EPS else -5.0 * alpha / 6.0 - p / (3.0 * u) + u
        w = np.sqrt(np.float64(alpha + 2.0 * y))
        s1 = np.sqrt(np.float64(-(3.0 * alpha + 2.0 * y + 2.0 * beta / w)))
        s2 = np.sqrt(np.float64(-(3.0 * alpha + 2.0 * y - 2.0 * beta / w)))
        base = -b / (4.0 * a)
        return [base + 0.5 * (w + s1), base + 0.5 * (w - s1), base + 0.5 * (-w + s2), base + 0.5 * (-w - s2)]


def polish_roots(f, g, xy):
    """:1640-1673, in place on a list of [x, y]."""
    with np.errstate(all="ignore"):
        for _ in range(5):
            stable = True
            for v in xy:
                x, y = v
                fv = f[0] * x * x + f[1] * x * y + f[3] * x + f[4] * y + f[5]
                gv = g[0] * x * x - y * y + g[3] * x + g[4] * y + g[5]
                if abs(fv) < EPS and abs(gv) < EPS:
                    continue
                stable = False
                dfdx = 2.0 * f[0] * x + f[1] * y + f[3]
                dfdy = f[1] * x + f[4]
                dgdx = 2.0 * g[0] * x + g[3]
                dgdy = -2.0 * y + g[4]
                inv = np.float64(1.0) / (dfdx * dgdy - dfdy * dgdx)
                v[0] = x - (dgdy * fv - dfdy * gv) * inv
                v[1] = y - (-dgdx * fv + dfdx * gv) * inv
            if stable:
                break


def _normalize(v):
    return v / np.linalg.norm(v)


def recover_pose_from_points(k_inv, samples):
    """:1146-1290.  samples: 3 x (pixel (x, y), point3d) -> [(root slot, R, t)] (slot = solve_quartic's root index)."""
    with np.errstate(all="ignore"):
        inl = [(_normalize(k_inv @ np.array([float(px[0]), float(px[1]), 1.0])), np.asarray(X, dtype=np.float64))
               for px, X in samples]
        d01 = np.linalg.norm(inl[0][1] - inl[1][1])
        d12 = np.linalg.norm(inl[1][1] - inl[2][1])
        d02 = np.linalg.norm(inl[0][1] - inl[2][1])
        if d12 > d01 and d12 > d02:
            inl = inl[1:] + inl[:1]
        elif d02 > d01 and d02 > d12:
            inl = [inl[0], inl[2], inl[1]]
        x10 = inl[1][1] - inl[0][1]
        x20 = inl[2][1] - inl[0][1]
        nx = _normalize(x10)
        nz = _normalize(np.cross(nx, x20))
        ny = _normalize(np.cross(nz, nx))
        N = np.stack([nx, ny, nz], axis=1)
        a, b, c = nx @ x10, nx @ x20, ny @ x20
        m01, m02, m12 = inl[0][0] @ inl[1][0], inl[0][0] @ inl[2][0], inl[1][0] @ inl[2][0]
        p = b / a
        q = (b * b + c * c) / (a * a)
        f = [p, -m12, 0.0, -m01 * (2.0 * p - 1.0), m02, p - 1.0]
        g = [q, 0.0, -1.0, -2.0 * m01 * q, 2.0 * m02, q - 1.0]
        h = [-f[0] * f[0] + g[0] * f[1] * f[1],
             f[1] * f[1] * g[3] - 2.0 * f[0] * f[3] - 2.0 * f[0] * f[1] * f[4] + 2.0 * f[1] * f[4] * g[0],
             f[4] * f[4] * g[0] - 2.0 * f[0] * f[4] * f[4] - 2.0 * f[0] * f[5] + f[1] * f[1] * g[5] - f[3] * f[3]
             - 2.0 * f[1] * f[3] * f[4] + 2.0 * f[1] * f[4] * g[3],
             f[4] * f[4] * g[3] - 2.0 * f[3] * f[4] * f[4] - 2.0 * f[3] * f[5] - 2.0 * f[1] * f[4] * f[5]
             + 2.0 * f[1] * f[4] * g[5],
             -2.0 * f[4] * f[4] * f[5] + g[5] * f[4] * f[4] - f[5] * f[5]]
        roots = solve_quartic(h)
        slots, xy = [], []
        for k, x in enumerate(roots):
            if not np.isfinite(x):
                continue
            y = -((f[0] * x + f[3]) * x + f[5]) / (f[4] + f[1] * x)
            slots.append(k)
            xy.append([x, y])
        polish_roots(f, g, xy)
        A = np.stack([-inl[0][0], inl[1][0], np.zeros(3)], axis=1)
        B = np.stack([-inl[0][0], np.zeros(3), inl[2][0]], axis=1)
        Cv = B - p * A
        out = []
        for k, (x, y) in zip(slots, xy):
            lam = np.array([1.0, x, y])
            s = np.linalg.norm(A @ lam) / a
            d = lam / s
            r1 = (A @ d) / a
            r2 = (Cv @ d) / c
            rc = np.stack([r1, r2, np.cross(r1, r2)], axis=1)
            R = rc @ N.T
            t = d[0] * inl[0][0] - R @ inl[0][1]
            if not np.isfinite(np.linalg.norm(R)) or not np.isfinite(np.linalg.norm(t)):
                continue
            out.append((k, R, t))
        return out


def point_reprojection_errors(tracks, projections, include):
    """point_reprojection_error (:1296-1328) of every track at once: the DLT with every projection given (rt's batched SVD,
    as triangulate_track), then the largest error over the views in `include` the track sees - f64::max, so NaN is ignored.
    -> errors [n] (NaN where the DLT gives None)."""
    tracks = np.asarray(tracks)
    m = tracks.shape[1]
    masked = tracks.copy()
    for j in range(m):
        if projections[j] is None:
            masked[:, j] = -1
    P = [pr if pr is not None else np.zeros((3, 4)) for pr in projections]
    pts, ok, _ = rt.triangulate_tracks(masked, P)
    err = np.full(len(tracks), np.nan)
    with np.errstate(all="ignore"):
        Xh = np.hstack([pts, np.ones((len(tracks), 1))])
        for j in include:
            if projections[j] is None:
                continue
            q = Xh @ projections[j].T
            e = np.sqrt((q[:, 0] / q[:, 2] - tracks[:, j, 0]) ** 2 + (q[:, 1] / q[:, 2] - tracks[:, j, 1]) ** 2)
            e = np.where(tracks[:, j, 0] >= 0, e, np.nan)
            err = np.fmax(err, e)
    err[~ok] = np.nan
    return err


def tracks_reprojection_error(tracks, projections, include, threshold, per_track=False):
    """:1193-1210 -> (count, largest error below the threshold) (and the per-track errors)."""
    errs = point_reprojection_errors(tracks, projections, include)
    below = errs < threshold
    count = int(below.sum())
    error = float(errs[below].max()) if count else 0.0
    return (count, error, errs) if per_track else (count, error)


def pose_candidates(linked_tracks, linked_points, projections, image, K, max_dimension, triple, per_track=False, score=True):
    """One hypothesis of recover_pose (:1091-1121) on a given sample triple
    -> [(slot, R, t, r, P, passed, count, error, per-track errors or None)]; score=False stops after the 3-sample check
    (count and error None for a pose that passed)."""
    k_inv = np.linalg.pinv(K, rcond=0.0)
    samples = [(linked_tracks[i][image], linked_points[i]) for i in triple]
    validate = [i for i, pr in enumerate(projections) if pr is not None or i == image]
    out = []
    for slot, R, t in recover_pose_from_points(k_inv, samples):
        cam = rt.Camera.from_matrix(K, R, t)
        P = cam.projection()
        prj = list(projections)
        prj[image] = P
        cnt, _ = tracks_reprojection_error(np.asarray(linked_tracks)[list(triple)], prj, [image],
                                           RANSAC_INLIERS_T * max_dimension)
        if cnt != RANSAC_N:
            out.append((slot, R, t, cam.r, P, False, 0, np.nan, None))
            continue
        if not score:
            out.append((slot, R, t, cam.r, P, True, None, None, None))
            continue
        count, error, errs = tracks_reprojection_error(linked_tracks, prj, validate, RANSAC_T * max_dimension, per_track=True)
        with np.errstate(all="ignore"):
            out.append((slot, R, t, cam.r, P, True, count, np.float64(error) / count, errs if per_track else None))
    return out


def linked(tracks, points, ok, image):
    """recover_pose's linked tracks (:1057-1062): seen in the image and triangulated, in table order."""
    sel = np.nonzero(np.asarray(ok, dtype=bool) & (np.asarray(tracks)[:, image, 0] >= 0))[0]
    return np.asarray(tracks)[sel], np.asarray(points)[sel]


def recover_pose_batch(lt, lp, projections, image, K, max_dimension, seed, batch, samples=device_samples, observe=None):
    """The hypotheses of one batch (:1091-1121) scanned in (hypothesis, root) order from the empty result
    -> (camera (r, t, P) or None, count, error, winner (batch, hyp, slot) or None).  observe(batch, hyp, slot, count, error,
    per-track errors) is called for every scored pose."""
    best = (None, 0, np.finfo(np.float64).max, None)
    for h in range(RANSAC_CHECK_INTERVAL):
        for slot, R, t, r, P, passed, count, error, errs in pose_candidates(
                lt, lp, projections, image, K, max_dimension, samples(seed, batch, h, len(lt)), per_track=observe is not None):
            if not passed:
                continue
            if observe is not None:
                observe(batch, h, slot, count, error, errs)
            if count > best[1] or (count == best[1] and error < best[2]):
                best = ((r, t, P), count, error, (batch, h, slot))
    return best


def recover_pose(tracks, points, ok, projections, image, K, max_dimension, seed, samples=device_samples, observe=None,
                 batch_results=None):
    """recover_pose (:1033-1144) fed with an index stream (the device's by default); reduce_best_result applied as a scan
    in (batch, hypothesis, root) order after the carried result (the device's convention): a batch's own best replaces the
    carried result when it is strictly better, which is the same scan.  batch_results: {batch: recover_pose_batch's result}
    computed elsewhere (the fixture generator's workers).
    -> dict(camera (r, t, P) or None when not accepted, best (the carried camera, accepted or not), count, error, batches,
    winner (batch, hyp, slot) or None, linked, ransac_d, history [(count, error, winner) after every batch])."""
    lt, lp = linked(tracks, points, ok, image)
    d = RANSAC_D_PERCENT * len(lt) // 100
    res = {"camera": None, "best": None, "count": 0, "error": 0.0, "batches": 0, "winner": None, "linked": len(lt),
           "ransac_d": d, "history": []}
    if len(lt) < RANSAC_N:
        return res
    best = (None, 0, np.finfo(np.float64).max, None)
    d_early = RANSAC_D_PERCENT_EARLY_EXIT * len(lt) // 100
    batches = 0
    for batch in range(RANSAC_K // RANSAC_CHECK_INTERVAL):
        b = batch_results[batch] if batch_results is not None else recover_pose_batch(
            lt, lp, projections, image, K, max_dimension, seed, batch, samples, observe)
        if b[1] > best[1] or (b[1] == best[1] and b[2] < best[2]):
            best = b
        res["history"].append((best[1], best[2], best[3]))
        batches = batch + 1
        if best[1] >= d_early:
            break
    res.update(camera=best[0] if best[1] > d else None, best=best[0], count=best[1], error=best[2], batches=batches,
               winner=best[3])
    return res


class SparseTriangulation:
    """The sparse half of PerspectiveTriangulation (:604-815) over numpy tables: add_image_pair_sparse (extend_tracks is
    passed in - the oracle's - with the inlier grid built here), recover_next_cameras and the re-triangulation."""

    def __init__(self, images_count, image_shapes, calibration, extend_tracks):
        self.n = images_count
        self.shapes = list(image_shapes)
        self.K = list(calibration)
        self.extend = extend_tracks
        self.tracks = np.full((0, images_count, 2), -1, dtype=np.int32)
        self.projections = [None] * images_count
        self.cameras = [None] * images_count
        self.best = None  # (score, pair, p2)
        self.remaining = list(range(images_count))
        self.points, self.ok = np.zeros((0, 3)), np.zeros(0, dtype=bool)
        self.last = self.last_image = self.last_counts = None

    def add_image_pair_sparse(self, i, j, F, inliers):
        w, h = self.shapes[i]
        grid = np.full((h, w, 2), -1, dtype=np.int32)
        for x1, y1, x2, y2 in np.asarray(inliers):  # later duplicates overwrite (:632-635)
            grid[y1, x1] = (x2, y2)
        tp2, n1, n2 = self.extend(grid, self.tracks[:, i], max(self.shapes[j]))
        fill = (self.tracks[:, j, 0] < 0) & (tp2[:, 0] >= 0)
        self.tracks[fill, j] = tp2[fill]
        new = np.full((len(n1), self.n, 2), -1, dtype=np.int32)
        new[:, i], new[:, j] = n1.astype(np.int32), n2.astype(np.int32)
        self.tracks = np.concatenate([self.tracks, new])
        both = (self.tracks[:, i, 0] >= 0) & (self.tracks[:, j, 0] >= 0)
        p2, score, _ = find_projection_matrix(F, self.K[i], self.K[j], self.tracks[both][:, [i, j]])
        if self.best is None or score > self.best[0]:
            self.best = (score, (i, j), p2)
        return p2, score

    def triangulate_tracks(self):
        masked = self.tracks.copy()
        for j in range(self.n):
            if self.projections[j] is None:
                masked[:, j] = -1
        P = [pr if pr is not None else np.zeros((3, 4)) for pr in self.projections]
        self.points, self.ok, _ = rt.triangulate_tracks(masked, P)

    def recover_next_cameras(self, seed=0, recover=None):
        """:710-811 -> the images placed ([] when none is left); raises TriangulationError when recover_pose fails.
        recover: stands in for recover_pose (same arguments and result), for a run recorded in tests/golden/."""
        self.last = self.last_image = self.last_counts = None
        if self.best is not None:
            _, (i1, i2), p2 = self.best
            self.projections[i1] = self.K[i1] @ np.eye(3, 4)
            self.cameras[i1] = rt.Camera.from_matrix(self.K[i1], np.eye(3), np.zeros(3))
            self.projections[i2] = self.K[i2] @ p2
            self.cameras[i2] = rt.Camera.from_matrix(self.K[i2], p2[:, :3], p2[:, 3])
            self.triangulate_tracks()
            self.remaining = [k for k in self.remaining if k not in (i1, i2)]
            self.best = None
            return [i1, i2]
        seen = self.tracks[..., 0] >= 0
        if not self.remaining:
            return []
        linked_any = self.ok & seen[:, self.remaining].any(axis=1)
        counts = {k: int((linked_any & seen[:, k]).sum()) for k in self.remaining}
        best = self.remaining[0]
        for k in self.remaining:  # max_by_key: the last maximum
            if counts[k] >= counts[best]:
                best = k
        self.remaining = [k for k in self.remaining if k != best]
        self.last_image, self.last_counts = best, counts
        res = (recover or recover_pose)(self.tracks, self.points, self.ok, self.projections, best, self.K[best],
                                        max(self.shapes[best]), seed)
        self.last = res
        if res["camera"] is None:
            raise rt.TriangulationError("Unable to find projection matrix")
        r, t, P = res["camera"]
        self.cameras[best] = rt.Camera(self.K[best], r, t)
        self.projections[best] = P
        self.triangulate_tracks()
        return [best]


def recover_camera_poses(st, seed=0, recover=None):
    """recover_camera_poses (reconstruction.rs:627-666) over a SparseTriangulation whose pairs are in: recover_next_cameras
    with seed + the number of earlier calls until it places nothing; a failed image is skipped and the loop goes on.
    -> (order, calls): per call that tried something {images | failure, image, counts, pose (recover_pose's result), and
    the state after it: points, ok, projections, cameras}."""
    order, calls = [], []
    while True:
        entry = {}
        try:
            placed = st.recover_next_cameras(seed=seed + len(calls), recover=recover)
        except rt.TriangulationError as exc:
            entry["failure"] = str(exc)
            placed = None
        if placed is not None and not placed:
            break
        entry.update(images=placed, image=st.last_image, counts=st.last_counts, pose=st.last, points=st.points.copy(),
                     ok=st.ok.copy(), projections=list(st.projections), cameras=list(st.cameras))
        calls.append(entry)
        order.extend(placed or [])
    return order, calls


def find_projection_matrix(F, k1, k2, short_tracks):
    """:940-994 -> (p2 [3, 4], count, counts of the four candidates)."""
    E = k2.T @ F @ k1
    u, _, vt = np.linalg.svd(E)
    E = u @ np.diag([1.0, 1.0, 0.0]) @ vt
    u, _, vt = np.linalg.svd(E)
    u3 = u[:, 2]
    W = np.array([[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]])
    r1 = u @ W @ vt
    r2 = u @ W.T @ vt
    r1 = r1 * np.sign(np.linalg.det(r1))
    r2 = r2 * np.sign(np.linalg.det(r2))
    p1 = k1 @ np.eye(3, 4)
    best, counts = None, []
    for r, t in [(r1, u3), (r1, -u3), (r2, u3), (r2, -u3)]:
        p2 = np.hstack([r, t[:, None]])
        cam2 = rt.Camera.from_matrix(k2, r, t)
        pts, ok, _ = rt.triangulate_tracks(short_tracks, [p1, k2 @ p2])
        good = ok.copy()
        good[ok] = (pts[ok, 2] > 0.0) & (cam2.point_depth(pts[ok]) > 0.0)
        count = int(good.sum())
        counts.append(count)
        if best is None or count >= best[1]:  # max_by: the last maximum
            best = (p2, count)
    return best[0], best[1], counts
