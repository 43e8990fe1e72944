// tri_common.hpp — what the perspective triangulation (triangulation_kernels.hip) and the pose recovery
// (pose_kernels.hip) share: Camera::matrix_r / from_matrix, the given projection k [R | t], and the DLT of
// triangulate_track (src/triangulation.rs:414-507, 867-911).  All f64; the common flag set keeps every product and sum
// unfused, so moving a function here changes no bit of its callers.
#pragma once

#include <hip/hip_runtime.h>

#include <cmath>

namespace {

constexpr double F64_EPS = 2.220446049250313e-16;         // f64::EPSILON
constexpr double PERSPECTIVE_SCALE_THRESHOLD = 0.0001;    // triangulation.rs:20

// Camera::matrix_r (:475-485)
__host__ __device__ inline void matrix_r(const double r[3], double R[9])
{
    double theta = sqrt(r[0] * r[0] + r[1] * r[1] + r[2] * r[2]);
    if (fabs(theta) < F64_EPS) {
        for (int i = 0; i < 9; i++) R[i] = (i % 4 == 0) ? 1.0 : 0.0;
        return;
    }
    double u[3] = {r[0] / theta, r[1] / theta, r[2] / theta};
    double c = cos(theta), s = sin(theta);
    double ux[9] = {0.0, -u[2], u[1], u[2], 0.0, -u[0], -u[1], u[0], 0.0};
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) R[3 * i + j] = ((i == j ? c : 0.0) + (1.0 - c) * u[i] * u[j]) + ux[3 * i + j] * s;
}

// Camera::from_matrix (:414-466): Rodrigues after Tomasi, with its 180 degree branch.  As written, rho = (a21 - a12, ..)
// is 2 sin(theta) u (Tomasi's is sin(theta) u), so the angle comes out as atan2(2 sin(theta), cos(theta)): a camera
// built from R rotates by more than R unless theta is 0 or 180 degrees.  Kept: the reference's cameras are these.
__host__ __device__ inline void from_matrix(const double *Rm, double r[3])
{
    auto R = [&](int i, int j) { return Rm[3 * i + j]; };
    double a[9];
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) a[3 * i + j] = (R(i, j) - R(j, i)) / 2.0;
    double rho[3] = {a[7] - a[5], a[2] - a[6], a[3] - a[1]};
    double s = sqrt(rho[0] * rho[0] + rho[1] * rho[1] + rho[2] * rho[2]);
    double c = ((R(0, 0) + R(1, 1)) + R(2, 2) - 1.0) / 2.0;
    if (fabs(s) < F64_EPS && fabs(c - 1.0) < F64_EPS) {
        r[0] = r[1] = r[2] = 0.0;
    } else if (fabs(s) < F64_EPS && fabs(c + 1.0) < F64_EPS) {
        int v_i = 0;
        double v_norm = 0.0;
        for (int col = 0; col < 3; col++) {
            double x = R(0, col) + (col == 0), y = R(1, col) + (col == 1), z = R(2, col) + (col == 2);
            double nn = sqrt(x * x + y * y + z * z);
            if (nn > v_norm) v_i = col, v_norm = nn;
        }
        double v[3]; // column v_i of R + I (selects: no indexed load of a private array on the device)
        for (int k = 0; k < 3; k++) v[k] = (v_i == 0 ? R(k, 0) : (v_i == 1 ? R(k, 1) : R(k, 2))) + (v_i == k);
        double vn = sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
        for (int k = 0; k < 3; k++) r[k] = (v[k] / vn) * M_PI;
        double rn = sqrt(r[0] * r[0] + r[1] * r[1] + r[2] * r[2]);
        if (fabs(rn - M_PI) < F64_EPS &&
            ((fabs(r[0]) < F64_EPS && fabs(r[1]) < F64_EPS && r[2] < 0.0) || (fabs(r[0]) < F64_EPS && r[1] < 0.0) ||
             r[0] < 0.0))
            for (int k = 0; k < 3; k++) r[k] = -r[k];
    } else {
        double theta = atan2(s, c);
        for (int k = 0; k < 3; k++) r[k] = (rho[k] / s) * theta;
    }
}

// k * [R | t] (:737-740): the projection triangulate_tracks uses for a camera given as matrices
__host__ __device__ inline void given_projection(const double *K, const double *R, const double *t, double P[12])
{
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 4; j++) {
            double a0 = j < 3 ? R[j] : t[0], a1 = j < 3 ? R[3 + j] : t[1], a2 = j < 3 ? R[6 + j] : t[2];
            P[4 * i + j] = K[3 * i] * a0 + K[3 * i + 1] * a1 + K[3 * i + 2] * a2;
        }
}

// ---- triangulate_track (:867-911) ---------------------------------------------------------------------------------------
// A (2k x 4, rows P.row(2) x - P.row(0), P.row(2) y - P.row(1) over the seen views in camera order) is reduced to the 4 x 4
// triangular R of its QR decomposition by Givens rotations (same right singular vectors and singular values, A^T A is
// never formed), then a one-sided Jacobi SVD of R gives V; the right singular vector of the smallest singular value is
// the point.  dlt_init / dlt_fold_view / dlt_solve are that computation in three steps.
__device__ inline void dlt_init(double R[16])
{
    for (int k = 0; k < 16; k++) R[k] = 0.0;
}

// the two rows of one seen view (observation x, y; projection P, 12 row-major) folded into R
__device__ inline void dlt_fold_view(double R[16], const double *P, double x, double y)
{
    for (int rr = 0; rr < 2; rr++) {
        double xv = rr == 0 ? x : y;
        double a[4];
        for (int c = 0; c < 4; c++) a[c] = P[8 + c] * xv - P[4 * rr + c];
        for (int c = 0; c < 4; c++) {
            double h = hypot(R[5 * c], a[c]);
            if (h == 0.0) continue;
            double cs = R[5 * c] / h, sn = a[c] / h;
            for (int l = c; l < 4; l++) {
                double t1 = cs * R[4 * c + l] + sn * a[l];
                a[l] = cs * a[l] - sn * R[4 * c + l];
                R[4 * c + l] = t1;
            }
            a[c] = 0.0;
        }
    }
}

// the right singular vector of the smallest singular value of R as a unit 4-vector (v4, the reference's point4d up to its
// sign) and the point xyz / w; false when |w| < 1e-4 (:896-898).  R is overwritten.
__device__ inline bool dlt_solve(double R[16], double v4[4], double X[3])
{
    double V[16];
    for (int k = 0; k < 16; k++) V[k] = (k % 5 == 0) ? 1.0 : 0.0;
    for (int sweep = 0; sweep < 40; sweep++) {
        bool rotated = false;
        for (int p = 0; p < 3; p++)
            for (int q = p + 1; q < 4; q++) {
                double al = 0.0, be = 0.0, ga = 0.0;
                for (int r = 0; r < 4; r++) {
                    al += R[4 * r + p] * R[4 * r + p];
                    be += R[4 * r + q] * R[4 * r + q];
                    ga += R[4 * r + p] * R[4 * r + q];
                }
                if (ga == 0.0 || fabs(ga) <= 1e-17 * sqrt(al * be)) continue;
                rotated = true;
                double zeta = (be - al) / (2.0 * ga);
                double t = (zeta >= 0.0 ? 1.0 : -1.0) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
                double c = 1.0 / sqrt(1.0 + t * t), s = c * t;
                for (int r = 0; r < 4; r++) {
                    double rp = R[4 * r + p], rq = R[4 * r + q];
                    R[4 * r + p] = c * rp - s * rq;
                    R[4 * r + q] = s * rp + c * rq;
                    double vp = V[4 * r + p], vq = V[4 * r + q];
                    V[4 * r + p] = c * vp - s * vq;
                    V[4 * r + q] = s * vp + c * vq;
                }
            }
        if (!rotated) break;
    }
    int best = 0;
    double best_n = INFINITY;
    for (int c = 0; c < 4; c++) {
        double s2 = 0.0;
        for (int r = 0; r < 4; r++) s2 += R[4 * r + c] * R[4 * r + c];
        if (s2 < best_n) best_n = s2, best = c;
    }
    double u[4];
    for (int r = 0; r < 4; r++) u[r] = V[4 * r + best];
    double nv = sqrt(u[0] * u[0] + u[1] * u[1] + u[2] * u[2] + u[3] * u[3]);
    for (int r = 0; r < 4; r++) v4[r] = u[r] / nv;
    double w = u[3] / nv;
    if (fabs(w) < PERSPECTIVE_SCALE_THRESHOLD) return false; // :896-898
    for (int k = 0; k < 3; k++) X[k] = (u[k] / nv) / w;     // remove_row(3).unscale(w) (:906-907)
    return true;
}

} // namespace
