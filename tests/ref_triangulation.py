"""CPU restatement (numpy, f64) of the reference's perspective triangulation stage - test infrastructure only.

Transcribes, citing zlogic/cybervision v0.20.3 src/triangulation.rs line by line:
  - Camera::{from_matrix, update_params, matrix_r, center, point_depth, projection}   :414-500
  - PerspectiveTriangulation::triangulate_track / triangulate_tracks                     :867-911
  - min_ray_angle_cos                                                                    :996-1031
  - filter_outliers                                                                      :1559-1593
  - BundleAdjustment (jacobian_a/b, residual, v_inv, residual vector, J^T r, Schur step,
    update_params, optimize)                                                             :1675-2148
Vectorised over tracks where the reference's order cannot matter (per-track work; the reductions run in track order).

Unpinned assumptions (nalgebra 0.35 calls replaced by numpy):
  - `a.svd(false, true)` -> np.linalg.svd: the singular values come out sorted in decreasing order in both (nalgebra's
    `SVD::new` sorts them, `svd_unordered` does not), so `v_t.row(nrows - 1)` is the right singular vector of the smallest
    one.  Its sign differs between libraries; the point is xyz / w, which does not depend on it.
  - `v.pseudo_inverse(f64::EPSILON)` -> np.linalg.pinv(v, rcond) with the absolute cut-off eps (V = mu I + sum B^T B is
    symmetric positive definite, so no singular value is cut and the result is the inverse either way).
  - `s.lu().solve(&e)` (partial pivoting) -> scipy-free LU with partial pivoting below (numpy's solve is LAPACK getrf /
    getrs, the same algorithm; the pivot order may differ on ties).  `None` when a pivot is exactly zero, as nalgebra's.
Nothing in cybervision_amd/ may import this module.
"""
from __future__ import annotations

import math

import numpy as np

EPS = np.finfo(np.float64).eps
PERSPECTIVE_SCALE_THRESHOLD = 0.0001            # triangulation.rs:20
MIN_ANGLE_BETWEEN_RAYS = 0.5 * math.pi / 180.0  # triangulation.rs (0.5 degrees, to_radians)
BUNDLE_ADJUSTMENT_MAX_ITERATIONS = 100          # triangulation.rs:15
INITIAL_MU = 1e-3                               # :1687
GRADIENT_EPSILON = 1e-12                        # :1688
DELTA_EPSILON = 1e-12                           # :1689
RESIDUAL_EPSILON = 1e-12                        # :1690
RESIDUAL_REDUCTION_EPSILON = 0.0                # :1691


class TriangulationError(RuntimeError):
    """TriangulationError (triangulation.rs:2150-2166): a static message."""


def skew(u):
    """nalgebra's cross_matrix."""
    return np.array([[0.0, -u[2], u[1]], [u[2], 0.0, -u[0]], [-u[1], u[0], 0.0]])


class Camera:
    """Camera (:404-500)."""

    def __init__(self, k, r, t):
        self.k = np.array(k, dtype=np.float64)
        self.r = np.array(r, dtype=np.float64)
        self.t = np.array(t, dtype=np.float64)
        self.r_matrix = matrix_r(self.r)
        self.center = center(self.r_matrix, self.t)

    @staticmethod
    def from_matrix(k, r, t):
        """:414-466 - Rodrigues via Tomasi, with the 180 degree branch."""
        r = np.asarray(r, dtype=np.float64)
        a = (r - r.T) / 2.0
        rho = np.array([a[2, 1] - a[1, 2], a[0, 2] - a[2, 0], a[1, 0] - a[0, 1]])
        s = np.linalg.norm(rho)
        c = (np.trace(r) - 1.0) / 2.0
        # (sic: rho is 2 sin(theta) u, so the angle below is atan2(2 sin(theta), cos(theta)), not theta)
        if abs(s) < EPS and abs(c - 1.0) < EPS:
            rv = np.zeros(3)
        elif abs(s) < EPS and abs(c + 1.0) < EPS:
            v_i, v_norm = 0, 0.0
            r_i = r + np.eye(3)
            for cand in range(3):  # column_iter, first strict maximum
                n = np.linalg.norm(r_i[:, cand])
                if n > v_norm:
                    v_i, v_norm = cand, n
            v = r_i[:, v_i]
            u = v / np.linalg.norm(v)
            rv = u * math.pi
            if abs(np.linalg.norm(rv) - math.pi) < EPS and (
                    (abs(rv[0]) < EPS and abs(rv[1]) < EPS and rv[2] < 0.0) or (abs(rv[0]) < EPS and rv[1] < 0.0)
                    or rv[0] < 0.0):
                rv = -rv
        else:
            u = rho / s
            theta = math.atan2(s, c)
            rv = u * theta
        return Camera(k, rv, t)

    def update_params(self, delta_r, delta_t):
        """:468-473"""
        self.r = self.r + delta_r
        self.t = self.t + delta_t
        self.r_matrix = matrix_r(self.r)
        self.center = center(self.r_matrix, self.t)

    def point_depth(self, X):
        """:492-496, X: [n, 3] -> [n] (OpenMVG's form)."""
        R = self.r_matrix
        q = X + (R.T @ self.t)[None, :]
        return q @ R[2]

    def projection(self):
        """:503-507"""
        p = np.zeros((3, 4))
        p[:, :3] = self.r_matrix
        p[:, 3] = self.t
        return self.k @ p

    def copy(self):
        c = Camera.__new__(Camera)
        c.k, c.r, c.t, c.r_matrix, c.center = self.k, self.r.copy(), self.t.copy(), self.r_matrix.copy(), self.center.copy()
        return c


def matrix_r(r):
    """:475-485"""
    theta = np.linalg.norm(r)
    if abs(theta) < EPS:
        return np.eye(3)
    u = r / theta
    return np.eye(3) * math.cos(theta) + (1.0 - math.cos(theta)) * np.outer(u, u) + skew(u) * math.sin(theta)


def center(r_matrix, t):
    """:487-489"""
    return -(r_matrix.T @ t)


# ---- triangulate_track / triangulate_tracks (:867-911) ----------------------------------------------------------------
def _dlt_systems(tracks, projections, sel, kk):
    """A (:885-890) of the tracks `sel`, which all have kk seen views: rows P.row(2) x - P.row(0), P.row(2) y - P.row(1)
    over the seen views in camera order (:873-880)."""
    seen = tracks[sel, :, 0] >= 0
    views = np.argsort(~seen, axis=1, kind="stable")[:, :kk]  # seen views first, in camera order
    P = np.asarray(projections)[views]  # [s, kk, 3, 4]
    xy = np.take_along_axis(tracks[sel].astype(np.float64), views[:, :, None], axis=1)  # [s, kk, 2]
    a = np.empty((len(sel), kk, 2, 4))
    a[:, :, 0] = P[:, :, 2] * xy[:, :, 0:1] - P[:, :, 0]
    a[:, :, 1] = P[:, :, 2] * xy[:, :, 1:2] - P[:, :, 1]
    return a.reshape(len(sel), 2 * kk, 4)


def triangulate_tracks(tracks, projections):
    """tracks: [n, m, 2] ((-1, -1) = None; int32, or float for noise-free tests), projections: [m, 3, 4]
    -> (points [n, 3], ok [n] bool, |w| [n] - the deciding quantity of :896, NaN for k < 2)."""
    tracks = np.asarray(tracks)
    n = tracks.shape[0]
    k = (tracks[..., 0] >= 0).sum(axis=1)
    pts = np.full((n, 3), np.nan)
    ok = np.zeros(n, dtype=bool)
    w_abs = np.full(n, np.nan)
    for kk in np.unique(k):
        if kk < 2:  # :881-883
            continue
        sel = np.nonzero(k == kk)[0]
        _, _, vt = np.linalg.svd(_dlt_systems(tracks, projections, sel, kk), full_matrices=False)  # :892-894
        p4 = vt[:, -1, :]  # v_t.row(nrows - 1): singular values descending
        w_abs[sel] = np.abs(p4[:, 3])
        good = ~(np.abs(p4[:, 3]) < PERSPECTIVE_SCALE_THRESHOLD)  # :896-898
        pts[sel[good]] = p4[good, :3] / p4[good, 3:4]  # :906-907 remove_row(3).unscale(w)
        ok[sel[good]] = True
    return pts, ok, w_abs


# ---- filter_outliers (:1559-1593), min_ray_angle_cos (:996-1031) -------------------------------------------------------
def filter_decisions(tracks, points, ok, cameras):
    """-> (keep [n] bool, depth_min [n], min_cos [n]): the deciding quantities of every triangulated track."""
    tracks = np.asarray(tracks)
    n, m, _ = tracks.shape
    seen = tracks[..., 0] >= 0
    threshold = math.cos(MIN_ANGLE_BETWEEN_RAYS)
    X = np.where(ok[:, None], points, 0.0)
    depth_min = np.full(n, np.inf)
    for j, cam in enumerate(cameras):
        d = cam.point_depth(X)
        depth_min = np.where(seen[:, j], np.minimum(depth_min, d), depth_min)
    front = depth_min > 0.0  # any(seen && !point_in_front) (:1568-1578)
    rays = np.zeros((n, m, 3))
    has = np.zeros((n, m), dtype=bool)
    for j, cam in enumerate(cameras):
        ray = X - cam.center[None, :]
        norm = np.linalg.norm(ray, axis=1)
        good = seen[:, j] & (norm >= EPS)  # ray.norm() < EPS -> skipped (:1009-1011)
        rays[good, j] = ray[good] / norm[good, None]
        has[:, j] = good
    min_cos = np.full(n, np.nan)
    for i in range(m):
        for j in range(i + 1, m):
            both = has[:, i] & has[:, j]
            c = np.abs(np.einsum("nk,nk->n", rays[:, i], rays[:, j]))
            upd = both & (np.isnan(min_cos) | (c < min_cos))
            min_cos = np.where(upd, c, min_cos)
    keep = ok & front & ~np.isnan(min_cos) & ~(min_cos > threshold)  # :1580-1587
    return keep, depth_min, min_cos


def given_projection(k, r, t):
    """k * [R | t] of a camera given as matrices - the projection triangulate_tracks uses for the initial pair
    (:737-740), next to the Camera that from_matrix makes of the same matrices."""
    p = np.zeros((3, 4))
    p[:, :3] = r
    p[:, 3] = t
    return np.asarray(k, dtype=np.float64) @ p


def triangulate_and_filter(tracks, cameras, projections):
    """triangulate_tracks with `projections`, then filter_outliers with `cameras` and retain (:1590):
    -> (kept indices, points [n_kept, 3])."""
    projections = np.asarray(projections)
    pts, ok, _ = triangulate_tracks(tracks, projections)
    keep, _, _ = filter_decisions(tracks, pts, ok, cameras)
    idx = np.nonzero(keep)[0]
    return idx, pts[idx]


# ---- BundleAdjustment (:1675-2148) ---------------------------------------------------------------------------------------
def lu_solve(a, b):
    """nalgebra `lu().solve` (partial pivoting; None when U has a zero on its diagonal)."""
    a = a.copy()
    b = b.copy()
    n = a.shape[0]
    for c in range(n):
        p = c + int(np.argmax(np.abs(a[c:, c])))
        if a[p, c] == 0.0:
            return None
        if p != c:
            a[[c, p]] = a[[p, c]]
            b[[c, p]] = b[[p, c]]
        f = a[c + 1:, c] / a[c, c]
        a[c + 1:, c:] -= np.outer(f, a[c, c:])
        b[c + 1:] -= f * b[c]
    x = np.zeros(n)
    for r in range(n - 1, -1, -1):
        x[r] = (b[r] - a[r, r + 1:] @ x[r + 1:]) / a[r, r]
    return x


class BundleAdjustment:
    CAMERA_PARAMETERS = 6

    def __init__(self, cameras, tracks, points):
        """cameras: [Camera], tracks: [n, m, 2] int32 (all with a point), points: [n, 3]."""
        self.cameras = [c.copy() for c in cameras]
        self.projections = [c.projection() for c in self.cameras]
        self.tracks = np.asarray(tracks)
        self.seen = self.tracks[..., 0] >= 0
        self.points = np.array(points, dtype=np.float64)
        self.covariance = 1.0
        self.mu = INITIAL_MU
        self.history = []  # accept (True) / reject (False) per finished iteration
        self.rhos = []  # the rho that decided each of them

    def _d_projection(self, X, j):
        """point_projected and d_projection_hpoint (:1698-1704), [n, 2, 3]."""
        P = self.projections[j]
        q = X @ P[:, :3].T + P[:, 3][None, :]
        u, v, w = q[:, 0], q[:, 1], q[:, 2]
        d = np.zeros((len(X), 2, 3))
        d[:, 0, 0] = 1.0 / w
        d[:, 0, 2] = -u / (w * w)
        d[:, 1, 1] = 1.0 / w
        d[:, 1, 2] = -v / (w * w)
        return d

    def jacobian_a(self, X, j):
        """:1694-1748 -> [n, 2, 6]"""
        cam = self.cameras[j]
        d = self._d_projection(X, j)
        u = cam.r
        u_skew = skew(u)
        dt = np.zeros((len(X), 3, 6))
        if np.linalg.norm(u) > EPS:
            for i in range(3):
                e_i = np.zeros(3)
                e_i[i] = 1.0
                d_r_i = (u[i] * u_skew + skew(np.cross(u, (np.eye(3) - cam.r_matrix) @ e_i))) @ cam.r_matrix / (u @ u)
                dt[:, :, i] = X @ d_r_i.T
        else:
            dt[:, :, :3] = -u_skew[None]  # (sic: the constant -[u]x, :1739-1743)
        dt[:, :, 3:] = np.eye(3)[None]
        return (d @ cam.k) @ dt

    def jacobian_b(self, X, j):
        """:1750-1766 -> [n, 2, 3]"""
        cam = self.cameras[j]
        d = self._d_projection(X, j)
        return (d @ cam.k) @ cam.r_matrix

    def residuals(self, X=None):
        """residual (:1768-1788) for every (track, view): [n, m, 2], zero where the view has no point."""
        X = self.points if X is None else X
        n, m = self.seen.shape
        out = np.zeros((n, m, 2))
        for j in range(m):
            P = self.projections[j]
            q = X @ P[:, :3].T + P[:, 3][None, :]
            q = q / q[:, 2:3]
            r = np.stack([q[:, 0] - self.tracks[:, j, 0], q[:, 1] - self.tracks[:, j, 1]], axis=1)
            out[:, j] = np.where(self.seen[:, j, None], r, 0.0)
        return out

    def residual_norm_squared(self):
        """calculate_residual_vector (:1800-1838) .norm_squared(), summed in vector order."""
        r = self.residuals().reshape(-1)
        return float(np.sum(r * r)) if len(r) < 2 else float(np.dot(r, r))

    def v_inv(self, X):
        """calculate_v_inv (:1790-1798) -> [n, 3, 3]"""
        v = np.broadcast_to(np.eye(3) * self.mu, (len(X), 3, 3)).copy()
        for j in range(len(self.cameras)):
            b = self.jacobian_b(X, j)
            v += np.swapaxes(b, 1, 2) @ b * self.covariance
        return _pinv3(v)

    def jt_residual(self):
        """calculate_jt_residual (:1840-1895) -> (camera part [6m], point part [n, 3])."""
        X = self.points
        res = self.residuals()
        m = len(self.cameras)
        g_a = np.zeros(6 * m)
        g_b = np.zeros((len(X), 3))
        ca = []
        for j in range(m):
            ja = self.jacobian_a(X, j)
            jb = self.jacobian_b(X, j)
            ca.append(np.einsum("nki,nk->ni", ja, res[:, j]))
            g_b += np.einsum("nki,nk->ni", jb, res[:, j])
        for j in range(m):  # track order, view order within a track (:1880-1892)
            g_a[6 * j:6 * j + 6] = ca[j].sum(axis=0)
        return g_a, g_b

    def delta_step(self):
        """calculate_delta_step (:1897-2010) -> (delta_a [6m], delta_b [n, 3]) or None (LU failure)."""
        X = self.points
        m = len(self.cameras)
        res = self.residuals()
        v_inv = self.v_inv(X)
        ja = [self.jacobian_a(X, j) for j in range(m)]
        jb = [self.jacobian_b(X, j) for j in range(m)]
        w = [np.swapaxes(ja[j], 1, 2) @ jb[j] * self.covariance for j in range(m)]  # [n, 6, 3]
        y = [w[j] @ v_inv for j in range(m)]
        s = np.zeros((6 * m, 6 * m))
        e = np.zeros(6 * m)
        for j in range(m):
            u_j = np.swapaxes(ja[j], 1, 2) @ ja[j] * self.covariance
            for k in range(m):
                blk = -(y[j] @ np.swapaxes(w[k], 1, 2))
                if j == k:
                    blk = blk + u_j
                s[6 * j:6 * j + 6, 6 * k:6 * k + 6] += blk.sum(axis=0)
            ra = np.einsum("nki,nk->ni", ja[j], res[:, j]) * self.covariance
            rb = np.einsum("nki,nk->ni", jb[j], res[:, j]) * self.covariance
            e[6 * j:6 * j + 6] += (ra - np.einsum("nij,nj->ni", y[j], rb)).sum(axis=0)
        for j in range(m):
            s[6 * j:6 * j + 6, 6 * j:6 * j + 6] += np.eye(6) * self.mu
        delta_a = lu_solve(s, e)
        if delta_a is None or not np.all(np.isfinite(delta_a)):
            return None
        delta_b = np.zeros((len(X), 3))
        for j in range(m):
            rb = np.einsum("nki,nk->ni", jb[j], res[:, j]) * self.covariance
            wt_da = np.einsum("nij,i->nj", w[j], delta_a[6 * j:6 * j + 6])
            delta_b += np.einsum("nij,nj->ni", v_inv, rb) - np.einsum("nij,nj->ni", v_inv, wt_da)
        return delta_a, delta_b

    def update_params(self, delta_a, delta_b):
        """:2012-2040"""
        for j, cam in enumerate(self.cameras):
            cam.update_params(delta_a[6 * j:6 * j + 3], delta_a[6 * j + 3:6 * j + 6])
        self.projections = [c.projection() for c in self.cameras]
        self.points = self.points + delta_b

    def optimize(self, progress=None):
        """:2042-2147 -> refined cameras; raises TriangulationError."""
        residual_ns = self.residual_norm_squared()
        g_a, g_b = self.jt_residual()
        self.initial_residual_norm = self.final_residual_norm = math.sqrt(residual_ns)
        if abs(max(g_a.max(), g_b.max())) <= GRADIENT_EPSILON:  # .max().abs() (:2050)
            return self.cameras
        self.mu = INITIAL_MU
        nu = 2.0
        found = False
        for it in range(BUNDLE_ADJUSTMENT_MAX_ITERATIONS):
            if progress is not None:
                progress(it / BUNDLE_ADJUSTMENT_MAX_ITERATIONS)
            step = self.delta_step()
            if step is None:
                raise TriangulationError("Failed to compute delta vector")
            delta_a, delta_b = step
            sum_cameras = sum(float(c.r @ c.r + c.t @ c.t) for c in self.cameras)
            sum_points = float(np.sum(self.points * self.points))
            params_norm = math.sqrt(sum_cameras + sum_points)
            delta_norm = math.sqrt(float(delta_a @ delta_a) + float(np.sum(delta_b * delta_b)))
            if delta_norm <= DELTA_EPSILON * (params_norm + DELTA_EPSILON):
                found = True
                break
            saved = ([c.copy() for c in self.cameras], list(self.projections), self.points.copy())
            self.update_params(delta_a, delta_b)
            new_ns = self.residual_norm_squared()
            rho_den = float(delta_a @ (delta_a * self.mu + g_a)) + float(np.sum(delta_b * (delta_b * self.mu + g_b)))
            rho = (residual_ns - new_ns) / rho_den
            self.rhos.append(rho)
            if rho > 0.0:
                self.history.append(True)
                converged = math.sqrt(residual_ns) - math.sqrt(new_ns) < RESIDUAL_REDUCTION_EPSILON * math.sqrt(residual_ns)
                residual_ns = new_ns
                g_a, g_b = self.jt_residual()
                if converged or abs(max(g_a.max(), g_b.max())) <= GRADIENT_EPSILON:
                    found = True
                    break
                self.mu *= max(1.0 / 3.0, 1.0 - (2.0 * rho - 1.0) ** 3.0)
                nu = 2.0
            else:
                self.history.append(False)
                self.cameras, self.projections, self.points = saved
                self.mu *= nu
                nu *= 2.0
            if math.sqrt(residual_ns) <= RESIDUAL_EPSILON:
                found = True
                break
        self.final_residual_norm = math.sqrt(residual_ns)
        if not found:
            raise TriangulationError("Levenberg-Marquardt failed to converge")
        return self.cameras


def _pinv3(v):
    """pseudo_inverse of a batch of 3x3 matrices (np.linalg.pinv, absolute cut-off f64::EPSILON as in :1797)."""
    u, s, vt = np.linalg.svd(v)
    s_inv = np.where(s > EPS, 1.0 / np.where(s > EPS, s, 1.0), 0.0)
    return np.swapaxes(vt, 1, 2) @ (s_inv[:, :, None] * np.swapaxes(u, 1, 2))


def triangulate_all(tracks, given, bundle_adjustment=True):
    """triangulate_all (:817-865) for cameras given as matrices [(K, R, t)] - projections k [R | t], cameras
    Camera::from_matrix, as for the initial pair (:727-740) - without pose recovery, merge_tracks or max_points:
    -> (kept indices, points, cameras, BundleAdjustment or None)."""
    cameras = [Camera.from_matrix(K, R, t) for K, R, t in given]
    idx, pts = triangulate_and_filter(tracks, cameras, [given_projection(K, R, t) for K, R, t in given])
    if not bundle_adjustment:
        return idx, pts, cameras, None
    ba = BundleAdjustment(cameras, np.asarray(tracks)[idx], pts)
    cams = ba.optimize()
    return idx, ba.points, cams, ba
