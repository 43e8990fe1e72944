// pose_kernels.hip — camera pose recovery of the perspective pipeline on the device: PerspectiveTriangulation's
// triangulate_tracks over the images that have a projection, find_projection_matrix's cheirality count, and recover_pose's
// P3P RANSAC (src/triangulation.rs:867-911, 940-994, 1033-1328, 1595-1673).  All arithmetic is f64, as in the reference.
// Counts are integer sums and the error of a candidate is a maximum, so no result depends on the order of a reduction; the
// best candidate of a batch is taken by a scan in (hypothesis, root) order (pose_best_kernel), so two runs give the same bits.
#include "cvhip_internal.hpp"
#include "tri_common.hpp"

#include <cmath>
#include <cstring>
#include <string>
#include <vector>

namespace {

constexpr int MAXC = CVHIP_TRIANGULATE_MAX_CAMERAS;
constexpr int BLOCK = 256;
constexpr uint32_t RANSAC_N = 3;                 // triangulation.rs:21
constexpr uint32_t RANSAC_K = 100000;            // :22
constexpr double RANSAC_INLIERS_T = 50.0 / 1000.0; // :23
constexpr double RANSAC_T = 50.0 / 1000.0;       // :24
constexpr uint32_t RANSAC_D_PERCENT = 70;        // :25
constexpr uint32_t RANSAC_D_PERCENT_EARLY_EXIT = 95; // :26
constexpr uint32_t RANSAC_CHECK_INTERVAL = 1000; // :27
constexpr int ROOTS = 4;                         // solve_quartic's roots, one pose each at most

// the known projections (has bit j set) of the m images, the image whose pose is sought, its K and K^-1
struct PoseViews {
    double P[MAXC][12];
    double K[9], Kinv[9];
    uint32_t m, has, image;
};

// one candidate pose: the P3P rotation R and t, the Camera::from_matrix(k, R, t) the reference scores (r, and its
// projection K [matrix_r(r) | t]); status 0 = no pose in this root slot, 1 = rejected by the 3-sample check, 2 = scored
struct PoseCand {
    double R[9], t[3], rv[3], P[12];
    int status;
};

struct PoseScore {
    uint32_t count;
    double error;
};

struct PoseBest {
    uint32_t count;
    double error;
    int32_t batch, hyp, root; // -1: the initial result (identity camera, 0, f64::MAX) is still carried
    double R[9], t[3], rv[3], P[12];
};

__device__ __forceinline__ unsigned long long mix64(unsigned long long z)
{
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

// choose_inliers (:1181-1191) for hypothesis h of a batch: three draws with replacement from 0..len by a counter-based
// generator (the scheme of ransac_kernels.hip): state = mix64(seed ^ mix64(batch << 32 | h)), then per draw
// state = mix64(state + 0x9E3779B97F4A7C15) and index = ((state >> 32) * len) >> 32.
__device__ inline void draw_samples(unsigned long long seed, uint32_t batch, uint32_t h, uint32_t len, uint32_t idx[3])
{
    unsigned long long state = mix64(seed ^ mix64(((unsigned long long)batch << 32) | h));
    for (int i = 0; i < 3; i++) {
        state = mix64(state + 0x9E3779B97F4A7C15ull);
        idx[i] = (uint32_t)(((state >> 32) * (unsigned long long)len) >> 32);
    }
}

// triangulate_track (:867-883) with the known projections plus `cand` in the image's slot -> unit 4-vector, false = None
__device__ inline bool tri_with(const int2 *__restrict__ row, const PoseViews &pv, const double *cand, double v4[4])
{
    double R[16], X[3];
    dlt_init(R);
    uint32_t seen = 0;
    for (uint32_t j = 0; j < pv.m; j++) {
        const bool isc = cand && j == pv.image;
        if (!isc && !((pv.has >> j) & 1u)) continue;
        const int2 o = row[j];
        if (o.x < 0) continue;
        seen++;
        dlt_fold_view(R, isc ? cand : pv.P[j], (double)o.x, (double)o.y);
    }
    if (seen < 2) return false;
    return dlt_solve(R, v4, X);
}

// point_reprojection_error's term (:1311-1320) of one view
__device__ inline double reproj(const double *P, const double v4[4], int2 o)
{
    double q[3];
    for (int i = 0; i < 3; i++) q[i] = ((P[4 * i] * v4[0] + P[4 * i + 1] * v4[1]) + P[4 * i + 2] * v4[2]) + P[4 * i + 3] * v4[3];
    const double x = q[0] / q[2], y = q[1] / q[2];
    const double dx = x - (double)o.x, dy = y - (double)o.y;
    return sqrt(dx * dx + dy * dy);
}

// ---- triangulate_tracks (:905-911) with the images that have a projection --------------------------------------------
__global__ __launch_bounds__(BLOCK) void pose_triangulate_kernel(const int2 *__restrict__ tracks, uint64_t n, const PoseViews *__restrict__ pvp,
                                                                 double *__restrict__ pts, uint8_t *__restrict__ ok)
{
    const uint64_t i = (uint64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n) return;
    const PoseViews &pv = *pvp;
    double v4[4], R[16], X[3] = {NAN, NAN, NAN};
    dlt_init(R);
    uint32_t seen = 0;
    for (uint32_t j = 0; j < pv.m; j++) {
        const int2 o = tracks[i * pv.m + j];
        if (!((pv.has >> j) & 1u) || o.x < 0) continue;
        seen++;
        dlt_fold_view(R, pv.P[j], (double)o.x, (double)o.y);
    }
    const bool good = seen >= 2 && dlt_solve(R, v4, X);
    for (int k = 0; k < 3; k++) pts[3 * i + k] = good ? X[k] : NAN;
    ok[i] = good ? 1 : 0;
}

// ---- find_projection_matrix's cheirality count (:970-991), the four candidates at once --------------------------------
struct Cheirality {
    double P1[12];
    double P2[4][12]; // k2 [r | t]
    double R2[4][9];  // camera2 = Camera::from_matrix(k2, r, t): its r_matrix and r_matrix^T t (point_depth, :492-500)
    double Rtt[4][3];
};

__global__ __launch_bounds__(BLOCK) void pose_cheirality_kernel(const int2 *__restrict__ short_tracks, uint64_t n,
                                                                Cheirality ch, uint32_t *__restrict__ block_counts)
{
    const uint64_t i = (uint64_t)blockIdx.x * BLOCK + threadIdx.x;
    int hit[4] = {0, 0, 0, 0};
    if (i < n) {
        const int2 o1 = short_tracks[2 * i], o2 = short_tracks[2 * i + 1];
        if (o1.x >= 0 && o2.x >= 0) {
            for (int c = 0; c < 4; c++) {
                double R[16], v4[4], X[3];
                dlt_init(R);
                dlt_fold_view(R, ch.P1, (double)o1.x, (double)o1.y);
                dlt_fold_view(R, ch.P2[c], (double)o2.x, (double)o2.y);
                if (!dlt_solve(R, v4, X)) continue;
                const double q0 = X[0] + ch.Rtt[c][0], q1 = X[1] + ch.Rtt[c][1], q2 = X[2] + ch.Rtt[c][2];
                const double depth = (ch.R2[c][6] * q0 + ch.R2[c][7] * q1) + ch.R2[c][8] * q2;
                hit[c] = X[2] > 0.0 && depth > 0.0;
            }
        }
    }
    for (int c = 0; c < 4; c++) {
        const uint32_t cnt = __syncthreads_count(hit[c]);
        if (threadIdx.x == 0) block_counts[(size_t)c * gridDim.x + blockIdx.x] = cnt;
    }
}

// ---- recover_pose_from_points (:1146-1179, 1193-1290), solve_quartic, polish_roots (:1595-1673) ------------------------
__device__ inline void normalize3(double v[3])
{
    const double n = sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
    for (int k = 0; k < 3; k++) v[k] = v[k] / n;
}

__device__ inline void cross3(const double a[3], const double b[3], double c[3])
{
    c[0] = a[1] * b[2] - a[2] * b[1];
    c[1] = a[2] * b[0] - a[0] * b[2];
    c[2] = a[0] * b[1] - a[1] * b[0];
}

__device__ inline double dot3(const double a[3], const double b[3]) { return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]; }

__device__ inline double dist3(const double a[3], const double b[3])
{
    const double d0 = a[0] - b[0], d1 = a[1] - b[1], d2 = a[2] - b[2];
    return sqrt((d0 * d0 + d1 * d1) + d2 * d2);
}

// solve_quartic (:1595-1638) as written: powf(1/3) of a negative number and sqrt of a negative number are NaN
__device__ inline void solve_quartic(const double h[5], double out[4])
{
    const double a = h[0], b = h[1], c = h[2], d = h[3], e = h[4];
    const double a_pw2 = a * a, b_pw2 = b * b, a_pw3 = a_pw2 * a, b_pw3 = b_pw2 * b, a_pw4 = a_pw3 * a, b_pw4 = b_pw3 * b;
    const double alpha = -3.0 * b_pw2 / (8.0 * a_pw2) + c / a;
    const double beta = b_pw3 / (8.0 * a_pw3) - b * c / (2.0 * a_pw2) + d / a;
    const double gamma = -3.0 * b_pw4 / (256.0 * a_pw4) + b_pw2 * c / (16.0 * a_pw3) - b * d / (4.0 * a_pw2) + e / a;
    const double alpha_pw2 = alpha * alpha, alpha_pw3 = alpha_pw2 * alpha;
    const double p = -alpha_pw2 / 12.0 - gamma;
    const double q = -alpha_pw3 / 108.0 + alpha * gamma / 3.0 - beta * beta / 8.0;
    const double r = -q / 2.0 + sqrt(q * q / 4.0 + p * p * p / 27.0);
    const double u = pow(r, 1.0 / 3.0);
    const double y = fabs(u) < F64_EPS ? -5.0 * alpha / 6.0 - pow(q, 1.0 / 3.0) : -5.0 * alpha / 6.0 - p / (3.0 * u) + u;
    const double w = sqrt(alpha + 2.0 * y);
    const double base = -b / (4.0 * a);
    const double s1 = sqrt(-(3.0 * alpha + 2.0 * y + 2.0 * beta / w)), s2 = sqrt(-(3.0 * alpha + 2.0 * y - 2.0 * beta / w));
    out[0] = base + 0.5 * (w + s1);
    out[1] = base + 0.5 * (w - s1);
    out[2] = base + 0.5 * (-w + s2);
    out[3] = base + 0.5 * (-w - s2);
}

// polish_roots (:1640-1673): 5 Newton passes over all roots, ending early when every root is stable
__device__ inline void polish_roots(const double f[6], const double g[6], double x[4], double y[4], const bool valid[4])
{
#pragma unroll
    for (int it = 0; it < 5; it++) {
        bool stable = true;
#pragma unroll
        for (int k = 0; k < ROOTS; k++) {
            if (!valid[k]) continue;
            const double xv = x[k], yv = y[k], x2 = xv * xv, y2 = yv * yv, x_y = xv * yv;
            const double fv = f[0] * x2 + f[1] * x_y + f[3] * xv + f[4] * yv + f[5];
            const double gv = g[0] * x2 - y2 + g[3] * xv + g[4] * yv + g[5];
            if (fabs(fv) < F64_EPS && fabs(gv) < F64_EPS) continue;
            stable = false;
            const double dfdx = 2.0 * f[0] * xv + f[1] * yv + f[3], dfdy = f[1] * xv + f[4];
            const double dgdx = 2.0 * g[0] * xv + g[3], dgdy = -2.0 * yv + g[4];
            const double inv_det_j = 1.0 / (dfdx * dgdy - dfdy * dgdx);
            const double dx = (dgdy * fv - dfdy * gv) * inv_det_j, dy = (-dgdx * fv + dfdx * gv) * inv_det_j;
            x[k] -= dx;
            y[k] -= dy;
        }
        if (stable) break;
    }
}

// One hypothesis per lane: its three samples, the P3P poses of recover_pose_from_points, each pose's scoring camera and the
// 3-sample check of recover_pose (:1102-1112).  Writes ROOTS candidates per hypothesis (slot = quartic root).
__global__ __launch_bounds__(64) void pose_hypothesis_kernel(const int2 *__restrict__ tracks, const double *__restrict__ pts,
                                                             uint32_t len, const PoseViews *__restrict__ pvp, unsigned long long seed, uint32_t batch,
                                                             uint32_t H, const uint32_t *__restrict__ sample_idx,
                                                             double inliers_threshold, PoseCand *__restrict__ out)
{
    const uint32_t h = blockIdx.x * 64 + threadIdx.x;
    if (h >= H) return;
    const PoseViews &pv = *pvp;
    uint32_t idx[3];
    if (sample_idx) {
#pragma unroll
        for (int i = 0; i < 3; i++) idx[i] = sample_idx[(size_t)3 * h + i];
    }
    else draw_samples(seed, batch, h, len, idx);
    // (p2 = normalize(K^-1 (x, y, 1)), point3d) per sample (:1151-1160)
    double b[3][3], X[3][3];
#pragma unroll
    for (int i = 0; i < 3; i++) {
        const int2 o = tracks[(size_t)idx[i] * pv.m + pv.image];
        const double v[3] = {(double)o.x, (double)o.y, 1.0};
#pragma unroll
        for (int r = 0; r < 3; r++) b[i][r] = (pv.Kinv[3 * r] * v[0] + pv.Kinv[3 * r + 1] * v[1]) + pv.Kinv[3 * r + 2] * v[2];
        normalize3(b[i]);
#pragma unroll
        for (int r = 0; r < 3; r++) X[i][r] = pts[(size_t)3 * idx[i] + r];
    }
    // rearrange so that 0-1 has the largest distance (:1162-1172); whole-array moves under the branch, so no private array
    // is indexed by a runtime value
    double b0[3], b1[3], b2[3], X0[3], X1[3], X2[3];
#pragma unroll
    for (int r = 0; r < 3; r++) b0[r] = b[0][r], b1[r] = b[1][r], b2[r] = b[2][r], X0[r] = X[0][r], X1[r] = X[1][r], X2[r] = X[2][r];
    {
        const double d01 = dist3(X0, X1), d12 = dist3(X1, X2), d02 = dist3(X0, X2);
        if (d12 > d01 && d12 > d02) { // rotate_left(1)
#pragma unroll
            for (int r = 0; r < 3; r++) {
                const double tb = b0[r], tx = X0[r];
                b0[r] = b1[r], b1[r] = b2[r], b2[r] = tb;
                X0[r] = X1[r], X1[r] = X2[r], X2[r] = tx;
            }
        } else if (d02 > d01 && d02 > d12) { // swap(1, 2)
#pragma unroll
            for (int r = 0; r < 3; r++) {
                const double tb = b1[r], tx = X1[r];
                b1[r] = b2[r], b2[r] = tb;
                X1[r] = X2[r], X2[r] = tx;
            }
        }
    }
    double x10[3], x20[3], nx[3], nz[3], ny[3];
#pragma unroll
    for (int k = 0; k < 3; k++) x10[k] = X1[k] - X0[k], x20[k] = X2[k] - X0[k];
#pragma unroll
    for (int k = 0; k < 3; k++) nx[k] = x10[k];
    normalize3(nx);
    cross3(nx, x20, nz);
    normalize3(nz);
    cross3(nz, nx, ny);
    normalize3(ny);
    const double a = dot3(nx, x10), bb = dot3(nx, x20), c = dot3(ny, x20);
    const double m01 = dot3(b0, b1), m02 = dot3(b0, b2), m12 = dot3(b1, b2);
    const double p = bb / a, q = (bb * bb + c * c) / (a * a);
    const double f[6] = {p, -m12, 0.0, -m01 * (2.0 * p - 1.0), m02, p - 1.0};
    const double g[6] = {q, 0.0, -1.0, -2.0 * m01 * q, 2.0 * m02, q - 1.0};
    const double hq[5] = {
        -f[0] * f[0] + g[0] * f[1] * f[1],
        f[1] * f[1] * g[3] - 2.0 * f[0] * f[3] - 2.0 * f[0] * f[1] * f[4] + 2.0 * f[1] * f[4] * g[0],
        f[4] * f[4] * g[0] - 2.0 * f[0] * f[4] * f[4] - 2.0 * f[0] * f[5] + f[1] * f[1] * g[5] - f[3] * f[3] -
            2.0 * f[1] * f[3] * f[4] + 2.0 * f[1] * f[4] * g[3],
        f[4] * f[4] * g[3] - 2.0 * f[3] * f[4] * f[4] - 2.0 * f[3] * f[5] - 2.0 * f[1] * f[4] * f[5] + 2.0 * f[1] * f[4] * g[5],
        -2.0 * f[4] * f[4] * f[5] + g[5] * f[4] * f[4] - f[5] * f[5],
    };
    double xs[4], ys[4];
    bool valid[4];
    solve_quartic(hq, xs);
#pragma unroll
    for (int k = 0; k < ROOTS; k++) {
        valid[k] = isfinite(xs[k]);
        ys[k] = valid[k] ? -((f[0] * xs[k] + f[3]) * xs[k] + f[5]) / (f[4] + f[1] * xs[k]) : 0.0;
    }
    polish_roots(f, g, xs, ys, valid);
    // a_vector = [-b0 | b1 | 0], b_vector = [-b0 | 0 | b2] (columns), c_vector = b_vector - p a_vector
    // the polished roots go through memory (this lane's own candidate slots), so the pose loop below stays rolled and
    // indexes no private array
#pragma unroll
    for (int k = 0; k < ROOTS; k++) {
        PoseCand &slot = out[(size_t)ROOTS * h + k];
        slot.t[0] = xs[k];
        slot.t[1] = ys[k];
        slot.status = valid[k] ? -1 : 0;
    }
#pragma unroll 1
    for (int k = 0; k < ROOTS; k++) {
        if (out[(size_t)ROOTS * h + k].status == 0) continue;
        const double lam[3] = {1.0, out[(size_t)ROOTS * h + k].t[0], out[(size_t)ROOTS * h + k].t[1]};
        double av[3];
#pragma unroll
        for (int r = 0; r < 3; r++) av[r] = (-b0[r] * lam[0] + b1[r] * lam[1]) + 0.0 * lam[2];
        const double s = sqrt((av[0] * av[0] + av[1] * av[1]) + av[2] * av[2]) / a;
        const double d[3] = {lam[0] / s, lam[1] / s, lam[2] / s};
        double r1[3], r2[3], r3[3];
#pragma unroll
        for (int r = 0; r < 3; r++) {
            const double A0 = -b0[r], A1 = b1[r], A2 = 0.0;
            const double C0 = -b0[r] - p * A0, C1 = 0.0 - p * A1, C2 = b2[r] - p * A2;
            r1[r] = ((A0 * d[0] + A1 * d[1]) + A2 * d[2]) / a;
            r2[r] = ((C0 * d[0] + C1 * d[1]) + C2 * d[2]) / c;
        }
        cross3(r1, r2, r3);
        // r = rc n^T, t = d0 b0 - r X0 (rc columns r1 r2 r3, n columns nx ny nz)
        double Rm[9], t[3];
#pragma unroll
        for (int i = 0; i < 3; i++)
#pragma unroll
            for (int j = 0; j < 3; j++) Rm[3 * i + j] = (r1[i] * nx[j] + r2[i] * ny[j]) + r3[i] * nz[j];
#pragma unroll
        for (int i = 0; i < 3; i++) t[i] = d[0] * b0[i] - ((Rm[3 * i] * X0[0] + Rm[3 * i + 1] * X0[1]) + Rm[3 * i + 2] * X0[2]);
        double rn = 0.0, tn = 0.0;
#pragma unroll
        for (int i = 0; i < 9; i++) rn += Rm[i] * Rm[i];
#pragma unroll
        for (int i = 0; i < 3; i++) tn += t[i] * t[i];
        if (!isfinite(sqrt(rn)) || !isfinite(sqrt(tn))) { // :1281-1284
            out[(size_t)ROOTS * h + k].status = 0;
            continue;
        }
        PoseCand &cand = out[(size_t)ROOTS * h + k];
#pragma unroll
        for (int i = 0; i < 9; i++) cand.R[i] = Rm[i];
#pragma unroll
        for (int i = 0; i < 3; i++) cand.t[i] = t[i];
        // Camera::from_matrix(k, &r, &t).projection() (:1096-1097)
        double rv[3], Rc[9], P[12];
        from_matrix(Rm, rv);
        matrix_r(rv, Rc);
        given_projection(pv.K, Rc, t, P);
#pragma unroll
        for (int i = 0; i < 3; i++) cand.rv[i] = rv[i];
#pragma unroll
        for (int i = 0; i < 12; i++) cand.P[i] = P[i];
        // the 3-sample check (:1102-1112): each sample re-triangulated with the candidate, its error in this image
        uint32_t cnt = 0;
#pragma unroll 1
        for (int i = 0; i < 3; i++) {
            const uint32_t ti = i == 0 ? idx[0] : (i == 1 ? idx[1] : idx[2]);
            const int2 *row = tracks + (size_t)ti * pv.m;
            double v4[4];
            if (!tri_with(row, pv, cand.P, v4)) continue;
            if (reproj(cand.P, v4, row[pv.image]) < inliers_threshold) cnt++;
        }
        cand.status = cnt == RANSAC_N ? 2 : 1;
    }
}

// tracks_reprojection_error (:1193-1210) of every candidate that passed the 3-sample check against all linked tracks: one
// block per candidate.  The track's error is the f64::max (NaN-ignoring, = fmax) of its views in validate_projections; the
// count and the largest error below the threshold are order-independent, so the block's reduction order does not matter.
__global__ __launch_bounds__(BLOCK) void pose_score_kernel(const int2 *__restrict__ tracks, uint32_t len, const PoseViews *__restrict__ pvp,
                                                           const PoseCand *__restrict__ cands, double threshold,
                                                           PoseScore *__restrict__ scores)
{
    __shared__ uint32_t cnt_w[BLOCK / 64];
    __shared__ double max_w[BLOCK / 64];
    const PoseCand &cand = cands[blockIdx.x];
    if (cand.status != 2) return; // (uniform over the block)
    const PoseViews &pv = *pvp;
    const double *P = cand.P;
    uint32_t cnt = 0;
    double mx = 0.0;
    for (uint32_t i = threadIdx.x; i < len; i += BLOCK) {
        const int2 *row = tracks + (size_t)i * pv.m;
        double v4[4];
        if (!tri_with(row, pv, P, v4)) continue;
        double err = NAN;
        for (uint32_t j = 0; j < pv.m; j++) {
            const bool isc = j == pv.image;
            if (!isc && !((pv.has >> j) & 1u)) continue;
            const int2 o = row[j];
            if (o.x < 0) continue;
            err = fmax(err, reproj(isc ? P : pv.P[j], v4, o));
        }
        if (err < threshold) {
            cnt++;
            mx = fmax(mx, err);
        }
    }
    for (int off = 32; off > 0; off >>= 1) {
        cnt += __shfl_down(cnt, off, 64);
        mx = fmax(mx, __shfl_down(mx, off, 64));
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) cnt_w[wave] = cnt, max_w[wave] = mx;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t c = 0;
        double m = 0.0;
        for (int w = 0; w < BLOCK / 64; w++) c += cnt_w[w], m = fmax(m, max_w[w]);
        scores[blockIdx.x].count = c;
        scores[blockIdx.x].error = m / (double)c; // error / count as written (NaN for 0 / 0)
    }
}

// reduce_best_result (:1078-1084) as a scan: b replaces a when it has a higher count, or the same count and a lower error
__device__ inline bool better(uint32_t cb, double eb, uint32_t ca, double ea) { return cb > ca || (cb == ca && eb < ea); }

// The best of a batch in (hypothesis, root) order, after the result carried from the earlier batches: each thread scans a
// contiguous chunk, thread 0 the chunk winners in order.  For this relation the chunked scan equals the one scan of all.
__global__ __launch_bounds__(BLOCK) void pose_best_kernel(const PoseCand *__restrict__ cands, const PoseScore *__restrict__ scores,
                                                          uint32_t nc, uint32_t batch, PoseBest *__restrict__ best)
{
    __shared__ int win[BLOCK];
    const uint32_t chunk = (nc + BLOCK - 1) / BLOCK;
    const uint32_t c0 = threadIdx.x * chunk, c1 = min(nc, c0 + chunk);
    int w = -1;
    for (uint32_t c = c0; c < c1; c++) {
        if (cands[c].status != 2) continue;
        if (w < 0 || better(scores[c].count, scores[c].error, scores[w].count, scores[w].error)) w = (int)c;
    }
    win[threadIdx.x] = w;
    __syncthreads();
    if (threadIdx.x != 0) return;
    PoseBest b = *best;
    for (int i = 0; i < BLOCK; i++) {
        const int c = win[i];
        if (c < 0 || !better(scores[c].count, scores[c].error, b.count, b.error)) continue;
        b.count = scores[c].count;
        b.error = scores[c].error;
        b.batch = (int32_t)batch;
        b.hyp = c / ROOTS;
        b.root = c % ROOTS;
        for (int k = 0; k < 9; k++) b.R[k] = cands[c].R[k];
        for (int k = 0; k < 3; k++) b.t[k] = cands[c].t[k], b.rv[k] = cands[c].rv[k];
        for (int k = 0; k < 12; k++) b.P[k] = cands[c].P[k];
    }
    *best = b;
}

// ---- host ----------------------------------------------------------------------------------------------------------------
// 3 x 3 SVD by one-sided Jacobi on the columns: A V = U S, singular values in decreasing order (as nalgebra's `svd`
// returns them).  A column whose singular value is below 1e-300 gets U's column from the cross product of the other two.
void svd3(const double A[9], double U[9], double S[3], double V[9])
{
    double a[9], v[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
    std::memcpy(a, A, 72);
    for (int sweep = 0; sweep < 60; sweep++) {
        bool rotated = false;
        for (int p = 0; p < 2; p++)
            for (int q = p + 1; q < 3; q++) {
                double al = 0.0, be = 0.0, ga = 0.0;
                for (int r = 0; r < 3; r++) {
                    al += a[3 * r + p] * a[3 * r + p];
                    be += a[3 * r + q] * a[3 * r + q];
                    ga += a[3 * r + p] * a[3 * r + q];
                }
                if (ga == 0.0 || std::fabs(ga) <= 1e-17 * std::sqrt(al * be)) continue;
                rotated = true;
                const double zeta = (be - al) / (2.0 * ga);
                const double t = (zeta >= 0.0 ? 1.0 : -1.0) / (std::fabs(zeta) + std::sqrt(1.0 + zeta * zeta));
                const double c = 1.0 / std::sqrt(1.0 + t * t), s = c * t;
                for (int r = 0; r < 3; r++) {
                    const double ap = a[3 * r + p], aq = a[3 * r + q];
                    a[3 * r + p] = c * ap - s * aq;
                    a[3 * r + q] = s * ap + c * aq;
                    const double vp = v[3 * r + p], vq = v[3 * r + q];
                    v[3 * r + p] = c * vp - s * vq;
                    v[3 * r + q] = s * vp + c * vq;
                }
            }
        if (!rotated) break;
    }
    double nrm[3];
    int ord[3] = {0, 1, 2};
    for (int c = 0; c < 3; c++) nrm[c] = std::sqrt(a[c] * a[c] + a[3 + c] * a[3 + c] + a[6 + c] * a[6 + c]);
    for (int i = 0; i < 3; i++) // stable sort, decreasing
        for (int j = i + 1; j < 3; j++)
            if (nrm[ord[j]] > nrm[ord[i]]) std::swap(ord[i], ord[j]);
    for (int k = 0; k < 3; k++) {
        const int c = ord[k];
        S[k] = nrm[c];
        for (int r = 0; r < 3; r++) {
            V[3 * r + k] = v[3 * r + c];
            U[3 * r + k] = nrm[c] > 1e-300 ? a[3 * r + c] / nrm[c] : 0.0;
        }
    }
    for (int k = 0; k < 3; k++) {
        if (S[k] > 1e-300) continue;
        const int i = (k + 1) % 3, j = (k + 2) % 3;
        U[k] = U[3 + i] * U[6 + j] - U[6 + i] * U[3 + j];
        U[3 + k] = U[6 + i] * U[j] - U[i] * U[6 + j];
        U[6 + k] = U[i] * U[3 + j] - U[3 + i] * U[j];
    }
}

void mul3(const double A[9], const double B[9], double C[9])
{
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) C[3 * i + j] = (A[3 * i] * B[j] + A[3 * i + 1] * B[3 + j]) + A[3 * i + 2] * B[6 + j];
}

double det3(const double A[9])
{
    return A[0] * (A[4] * A[8] - A[5] * A[7]) - A[1] * (A[3] * A[8] - A[5] * A[6]) + A[2] * (A[3] * A[7] - A[4] * A[6]);
}

// nalgebra's pseudo_inverse(f64::EPSILON) of a 3 x 3: V S^+ U^T, singular values at or below eps dropped
void pinv3(const double A[9], double Ai[9])
{
    double U[9], S[3], V[9];
    svd3(A, U, S, V);
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) {
            double s = 0.0;
            for (int k = 0; k < 3; k++)
                if (S[k] > F64_EPS) s += V[3 * i + k] * (1.0 / S[k]) * U[3 * j + k];
            Ai[3 * i + j] = s;
        }
}

int set_views(PoseViews &pv, uint32_t m, const double *projections, const uint8_t *has_projection, uint32_t image,
              const double *K)
{
    std::memset(&pv, 0, sizeof(pv));
    pv.m = m;
    pv.image = image;
    for (uint32_t j = 0; j < m; j++) {
        if (!has_projection[j]) continue;
        pv.has |= 1u << j;
        std::memcpy(pv.P[j], projections + 12 * j, 96);
    }
    if (K) {
        std::memcpy(pv.K, K, 72);
        pinv3(K, pv.Kinv);
    }
    return CVHIP_OK;
}

int check_common(cvhip_device *dev, uint64_t n, uint32_t m, const char *what)
{
    if (!dev) return cvhip::fail(CVHIP_ERR_INVALID, "null argument");
    if (m < 1 || m > CVHIP_TRIANGULATE_MAX_CAMERAS)
        return cvhip::fail(m < 1 ? CVHIP_ERR_INVALID : CVHIP_ERR_UNSUPPORTED,
                           std::string(what) + ": 1 to " + std::to_string(CVHIP_TRIANGULATE_MAX_CAMERAS) + " images");
    if (n >= 0xFFFFFFFFull) return cvhip::fail(CVHIP_ERR_UNSUPPORTED, std::string(what) + ": 2^32 - 1 tracks or more");
    hipError_t e = hipSetDevice(dev->d.ordinal);
    if (e != hipSuccess) return cvhip::fail(CVHIP_ERR_DEVICE, std::string("hipSetDevice: ") + hipGetErrorString(e));
    return CVHIP_OK;
}

// the linked tracks of recover_pose (:1057-1062): seen in the image and triangulated, in table order
void linked_tracks(const int32_t *tracks, uint64_t n, uint32_t m, const double *points, const uint8_t *ok, uint32_t image,
                   std::vector<int2> &lt, std::vector<double> &lp)
{
    for (uint64_t i = 0; i < n; i++) {
        if (!ok[i] || tracks[(i * m + image) * 2] < 0) continue;
        for (uint32_t j = 0; j < m; j++) lt.push_back(make_int2(tracks[(i * m + j) * 2], tracks[(i * m + j) * 2 + 1]));
        for (int k = 0; k < 3; k++) lp.push_back(points[3 * i + k]);
    }
}

} // namespace

extern "C" int cvhip_triangulate_tracks(cvhip_device *dev, const int32_t *tracks, uint64_t n, uint32_t m,
                                        const double *projections, const uint8_t *has_projection, double *out_points,
                                        uint8_t *out_ok)
{
    int rc = check_common(dev, n, m, "triangulate_tracks");
    if (rc) return rc;
    if (!projections || !has_projection || (n && (!tracks || !out_points || !out_ok)))
        return cvhip::fail(CVHIP_ERR_INVALID, "null argument");
    if (n == 0) return CVHIP_OK;
    PoseViews pv;
    set_views(pv, m, projections, has_projection, 0, nullptr);
    hipStream_t s = dev->d.stream;
    cvhip::CallScratch sc;
    const int2 *d_tr = nullptr;
    double *d_pts = nullptr;
    uint8_t *d_ok = nullptr;
    PoseViews *d_pv = nullptr;
    const char *const what = "triangulate_tracks";
    CVHIP_TRY_HIP_AT(what, sc.alloc(&d_pv, 1));
    CVHIP_TRY_HIP_AT(what, hipMemcpyAsync(d_pv, &pv, sizeof(pv), hipMemcpyHostToDevice, s));
    CVHIP_TRY_HIP_AT(what, sc.input(reinterpret_cast<const int2 *>(tracks), (size_t)n * m, &d_tr, s));
    CVHIP_TRY_HIP_AT(what, sc.output(out_points, (size_t)n * 3, &d_pts));
    CVHIP_TRY_HIP_AT(what, sc.output(out_ok, (size_t)n, &d_ok));
    hipLaunchKernelGGL(pose_triangulate_kernel, dim3((unsigned)((n + BLOCK - 1) / BLOCK)), dim3(BLOCK), 0, s, d_tr, n, d_pv, d_pts, d_ok);
    CVHIP_TRY_HIP_AT(what, hipGetLastError());
    CVHIP_TRY_HIP_AT(what, sc.copy_out(out_points, d_pts, (size_t)n * 3, s));
    CVHIP_TRY_HIP_AT(what, sc.copy_out(out_ok, d_ok, (size_t)n, s));
    CVHIP_TRY_HIP_AT(what, hipStreamSynchronize(s));
    return CVHIP_OK;
}

extern "C" int cvhip_find_projection_matrix(cvhip_device *dev, const double *F, const double *K1, const double *K2,
                                            const int32_t *short_tracks, uint64_t n, double *out_P2, double *out_score,
                                            double *out_r2, double *out_KP2)
{
    int rc = check_common(dev, n, 2, "find_projection_matrix");
    if (rc) return rc;
    if (!F || !K1 || !K2 || !out_P2 || !out_score || (n && !short_tracks)) return cvhip::fail(CVHIP_ERR_INVALID, "null argument");
    // E = k2^T F k1, projected onto diag(1, 1, 0), decomposed again (:946-958)
    double K2t[9], tmp[9], E[9], U[9], S[3], V[9];
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) K2t[3 * i + j] = K2[3 * j + i];
    mul3(K2t, F, tmp);
    mul3(tmp, K1, E);
    svd3(E, U, S, V);
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) E[3 * i + j] = U[3 * i] * V[3 * j] + U[3 * i + 1] * V[3 * j + 1];
    svd3(E, U, S, V);
    double Vt[9];
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) Vt[3 * i + j] = V[3 * j + i];
    const double W[9] = {0.0, -1.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 1.0}, Wt[9] = {0.0, 1.0, 0.0, -1.0, 0.0, 0.0, 0.0, 0.0, 1.0};
    double r1[9], r2[9];
    mul3(U, W, tmp);
    mul3(tmp, Vt, r1);
    mul3(U, Wt, tmp);
    mul3(tmp, Vt, r2);
    for (double *r : {r1, r2}) {
        const double d = det3(r), sg = std::isnan(d) ? d : (std::signbit(d) ? -1.0 : 1.0); // f64::signum
        for (int k = 0; k < 9; k++) r[k] *= sg;
    }
    const double u3[3] = {U[2], U[5], U[8]};
    // candidates in the reference's order: (r1, u3), (r1, -u3), (r2, u3), (r2, -u3) (:968-969)
    Cheirality ch;
    const double Id[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, z3[3] = {0, 0, 0};
    given_projection(K1, Id, z3, ch.P1);
    double cand_r[4][9], cand_t[4][3];
    for (int c = 0; c < 4; c++) {
        std::memcpy(cand_r[c], c < 2 ? r1 : r2, 72);
        for (int k = 0; k < 3; k++) cand_t[c][k] = (c % 2) ? -u3[k] : u3[k];
        given_projection(K2, cand_r[c], cand_t[c], ch.P2[c]);
        double rv[3];
        from_matrix(cand_r[c], rv);
        matrix_r(rv, ch.R2[c]);
        for (int i = 0; i < 3; i++)
            ch.Rtt[c][i] = (ch.R2[c][i] * cand_t[c][0] + ch.R2[c][3 + i] * cand_t[c][1]) + ch.R2[c][6 + i] * cand_t[c][2];
    }
    uint64_t counts[4] = {0, 0, 0, 0};
    if (n) {
        hipStream_t s = dev->d.stream;
        cvhip::CallScratch sc;
        const uint32_t nb = (uint32_t)((n + BLOCK - 1) / BLOCK);
        const int2 *d_tr = nullptr;
        uint32_t *d_cnt = nullptr;
        CVHIP_TRY_HIP_AT("find_projection_matrix", sc.input(reinterpret_cast<const int2 *>(short_tracks), (size_t)n * 2, &d_tr, s));
        CVHIP_TRY_HIP_AT("find_projection_matrix", sc.alloc(&d_cnt, (size_t)nb * 4));
        hipLaunchKernelGGL(pose_cheirality_kernel, dim3(nb), dim3(BLOCK), 0, s, d_tr, n, ch, d_cnt);
        CVHIP_TRY_HIP_AT("find_projection_matrix", hipGetLastError());
        std::vector<uint32_t> h((size_t)nb * 4);
        CVHIP_TRY_HIP_AT("find_projection_matrix", hipMemcpyAsync(h.data(), d_cnt, h.size() * 4, hipMemcpyDeviceToHost, s));
        CVHIP_TRY_HIP_AT("find_projection_matrix", hipStreamSynchronize(s));
        for (int c = 0; c < 4; c++)
            for (uint32_t b = 0; b < nb; b++) counts[c] += h[(size_t)c * nb + b];
    }
    int best = 0; // max_by keeps the LAST maximum
    for (int c = 1; c < 4; c++)
        if (counts[c] >= counts[best]) best = c;
    for (int i = 0; i < 3; i++) {
        for (int j = 0; j < 3; j++) out_P2[4 * i + j] = cand_r[best][3 * i + j];
        out_P2[4 * i + 3] = cand_t[best][i];
    }
    *out_score = (double)counts[best];
    if (out_r2) from_matrix(cand_r[best], out_r2);
    if (out_KP2) std::memcpy(out_KP2, ch.P2[best], 96); // k2 * p2 (:737-740)
    return CVHIP_OK;
}

namespace {

struct PoseRun {
    cvhip::CallScratch mem;
    int2 *tr = nullptr;
    double *pts = nullptr;
    uint32_t len = 0;
    PoseViews pv;
    PoseViews *d_pv = nullptr;
};

int pose_setup(PoseRun &r, cvhip_device *dev, const int32_t *tracks, uint64_t n, uint32_t m, const double *points,
               const uint8_t *ok, const double *projections, const uint8_t *has_projection, uint32_t image_index,
               const double *K, const char *what)
{
    int rc = check_common(dev, n, m, what);
    if (rc) return rc;
    if (!projections || !has_projection || !K || (n && (!tracks || !points || !ok)))
        return cvhip::fail(CVHIP_ERR_INVALID, "null argument");
    if (image_index >= m) return cvhip::fail(CVHIP_ERR_INVALID, std::string(what) + ": image_index out of range");
    std::vector<int2> lt;
    std::vector<double> lp;
    linked_tracks(tracks, n, m, points, ok, image_index, lt, lp);
    r.len = (uint32_t)(lp.size() / 3);
    set_views(r.pv, m, projections, has_projection, image_index, K);
    r.pv.has &= ~(1u << image_index); // the image's own slot is the candidate's
    hipStream_t s = dev->d.stream;
    CVHIP_TRY_HIP_AT(what, r.mem.alloc(&r.d_pv, 1));
    CVHIP_TRY_HIP_AT(what, hipMemcpyAsync(r.d_pv, &r.pv, sizeof(PoseViews), hipMemcpyHostToDevice, s));
    CVHIP_TRY_HIP_AT(what, r.mem.alloc(&r.tr, lt.size()));
    CVHIP_TRY_HIP_AT(what, r.mem.alloc(&r.pts, lp.size()));
    if (r.len) {
        CVHIP_TRY_HIP_AT(what, hipMemcpyAsync(r.tr, lt.data(), lt.size() * sizeof(int2), hipMemcpyHostToDevice, s));
        CVHIP_TRY_HIP_AT(what, hipMemcpyAsync(r.pts, lp.data(), lp.size() * 8, hipMemcpyHostToDevice, s));
    }
    CVHIP_TRY_HIP_AT(what, hipStreamSynchronize(s)); // (the host vectors and r.pv's copy are read before they go)
    return CVHIP_OK;
}

} // namespace

extern "C" int cvhip_recover_pose(cvhip_device *dev, const int32_t *tracks, uint64_t n, uint32_t m, const double *points,
                                  const uint8_t *ok, const double *projections, const uint8_t *has_projection,
                                  uint32_t image_index, const double *K, uint32_t max_dimension, uint64_t seed, double *out_r,
                                  double *out_t, double *out_projection, uint32_t *out_count, double *out_error,
                                  uint32_t *out_batches, int32_t *out_winner, cvhip_progress_fn progress, void *user)
{
    PoseRun r;
    int rc = pose_setup(r, dev, tracks, n, m, points, ok, projections, has_projection, image_index, K, "recover_pose");
    if (rc) return rc;
    if (out_count) *out_count = 0;
    if (out_batches) *out_batches = 0;
    if (out_winner) out_winner[0] = out_winner[1] = out_winner[2] = -1;
    if (r.len < RANSAC_N) return cvhip::fail(CVHIP_ERR_NO_SURFACE, "Unable to find projection matrix");
    const uint32_t H = RANSAC_CHECK_INTERVAL, NC = H * ROOTS;
    const uint32_t ransac_d = (uint32_t)((uint64_t)RANSAC_D_PERCENT * r.len / 100);
    const uint32_t ransac_d_early_exit = (uint32_t)((uint64_t)RANSAC_D_PERCENT_EARLY_EXIT * r.len / 100);
    hipStream_t s = dev->d.stream;
    PoseCand *cands;
    PoseScore *scores;
    PoseBest *best;
    CVHIP_TRY_HIP_AT("recover_pose", r.mem.alloc(&cands, NC));
    CVHIP_TRY_HIP_AT("recover_pose", r.mem.alloc(&scores, NC));
    CVHIP_TRY_HIP_AT("recover_pose", r.mem.alloc(&best, 1));
    // best_result = (Camera::from_matrix(k, I, 0), 0, f64::MAX) (:1072-1076)
    PoseBest hb;
    std::memset(&hb, 0, sizeof(hb));
    hb.count = 0;
    hb.error = 1.7976931348623157e308;
    hb.batch = hb.hyp = hb.root = -1;
    const double Id[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, z3[3] = {0, 0, 0};
    std::memcpy(hb.R, Id, 72);
    given_projection(K, Id, z3, hb.P);
    CVHIP_TRY_HIP_AT("recover_pose", hipMemcpyAsync(best, &hb, sizeof(hb), hipMemcpyHostToDevice, s));
    const uint32_t max_dim = max_dimension;
    const double inl_t = RANSAC_INLIERS_T * (double)max_dim, pts_t = RANSAC_T * (double)max_dim;
    uint32_t batches = 0;
    for (uint32_t batch = 0; batch < RANSAC_K / RANSAC_CHECK_INTERVAL; batch++) {
        hipLaunchKernelGGL(pose_hypothesis_kernel, dim3((H + 63) / 64), dim3(64), 0, s, r.tr, r.pts, r.len, r.d_pv,
                           (unsigned long long)seed, batch, H, (const uint32_t *)nullptr, inl_t, cands);
        hipLaunchKernelGGL(pose_score_kernel, dim3(NC), dim3(BLOCK), 0, s, r.tr, r.len, r.d_pv, cands, pts_t, scores);
        hipLaunchKernelGGL(pose_best_kernel, dim3(1), dim3(BLOCK), 0, s, cands, scores, NC, batch, best);
        CVHIP_TRY_HIP_AT("recover_pose", hipGetLastError());
        CVHIP_TRY_HIP_AT("recover_pose", hipMemcpyAsync(&hb, best, sizeof(hb), hipMemcpyDeviceToHost, s));
        CVHIP_TRY_HIP_AT("recover_pose", hipStreamSynchronize(s));
        batches = batch + 1;
        if (progress) progress(user, 0.02f + 0.98f * ((float)(batches * H) / (float)RANSAC_K));
        if (hb.count >= ransac_d_early_exit) break; // :1126-1129
    }
    if (out_count) *out_count = hb.count;
    if (out_error) *out_error = hb.error;
    if (out_batches) *out_batches = batches;
    if (out_winner) out_winner[0] = hb.batch, out_winner[1] = hb.hyp, out_winner[2] = hb.root;
    if (out_r) std::memcpy(out_r, hb.rv, 24);
    if (out_t) std::memcpy(out_t, hb.t, 24);
    if (out_projection) std::memcpy(out_projection, hb.P, 96);
    if (!(hb.count > ransac_d)) return cvhip::fail(CVHIP_ERR_NO_SURFACE, "Unable to find projection matrix"); // :1132-1137
    return CVHIP_OK;
}

extern "C" int cvhip_recover_pose_models(cvhip_device *dev, const int32_t *tracks, uint64_t n, uint32_t m,
                                         const double *points, const uint8_t *ok, const double *projections,
                                         const uint8_t *has_projection, uint32_t image_index, const double *K,
                                         uint32_t max_dimension, const uint32_t *sample_idx, uint32_t B, double *out_pose,
                                         int8_t *out_status, uint32_t *out_count, double *out_error)
{
    PoseRun r;
    int rc = pose_setup(r, dev, tracks, n, m, points, ok, projections, has_projection, image_index, K, "recover_pose_models");
    if (rc) return rc;
    if (!sample_idx || !out_pose || !out_status || !out_count || !out_error) return cvhip::fail(CVHIP_ERR_INVALID, "null argument");
    for (uint64_t i = 0; i < 3ull * B; i++)
        if (sample_idx[i] >= r.len) return cvhip::fail(CVHIP_ERR_INVALID, "recover_pose_models: sample index out of range");
    if (B == 0) return CVHIP_OK;
    const uint32_t NC = B * ROOTS;
    hipStream_t s = dev->d.stream;
    PoseCand *cands;
    PoseScore *scores;
    uint32_t *d_idx;
    CVHIP_TRY_HIP_AT("recover_pose_models", r.mem.alloc(&cands, NC));
    CVHIP_TRY_HIP_AT("recover_pose_models", r.mem.alloc(&scores, NC));
    CVHIP_TRY_HIP_AT("recover_pose_models", r.mem.alloc(&d_idx, 3 * (size_t)B));
    CVHIP_TRY_HIP_AT("recover_pose_models", hipMemcpyAsync(d_idx, sample_idx, 12ull * B, hipMemcpyHostToDevice, s));
    const double inl_t = RANSAC_INLIERS_T * (double)max_dimension, pts_t = RANSAC_T * (double)max_dimension;
    hipLaunchKernelGGL(pose_hypothesis_kernel, dim3((B + 63) / 64), dim3(64), 0, s, r.tr, r.pts, r.len, r.d_pv, 0ull, 0u, B,
                       (const uint32_t *)d_idx, inl_t, cands);
    hipLaunchKernelGGL(pose_score_kernel, dim3(NC), dim3(BLOCK), 0, s, r.tr, r.len, r.d_pv, cands, pts_t, scores);
    CVHIP_TRY_HIP_AT("recover_pose_models", hipGetLastError());
    std::vector<PoseCand> hc(NC);
    std::vector<PoseScore> hs(NC);
    CVHIP_TRY_HIP_AT("recover_pose_models", hipMemcpyAsync(hc.data(), cands, sizeof(PoseCand) * NC, hipMemcpyDeviceToHost, s));
    CVHIP_TRY_HIP_AT("recover_pose_models", hipMemcpyAsync(hs.data(), scores, sizeof(PoseScore) * NC, hipMemcpyDeviceToHost, s));
    CVHIP_TRY_HIP_AT("recover_pose_models", hipStreamSynchronize(s));
    for (uint32_t c = 0; c < NC; c++) {
        double *o = out_pose + 27ull * c;
        const bool any = hc[c].status != 0;
        out_status[c] = (int8_t)hc[c].status;
        std::memcpy(o, hc[c].R, 72);
        std::memcpy(o + 9, hc[c].t, 24);
        std::memcpy(o + 12, hc[c].rv, 24);
        std::memcpy(o + 15, hc[c].P, 96);
        if (!any)
            for (int k = 0; k < 27; k++) o[k] = NAN;
        out_count[c] = hc[c].status == 2 ? hs[c].count : 0;
        out_error[c] = hc[c].status == 2 ? hs[c].error : NAN;
    }
    return CVHIP_OK;
}
