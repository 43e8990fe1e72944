// triangulation_kernels.hip — perspective triangulation of the dense tracks on the device: PerspectiveTriangulation's
// triangulate_tracks + filter_outliers + BundleAdjustment (src/triangulation.rs:817-865, 867-911, 1559-1593, 1675-2148).
// All arithmetic is f64, as in the reference.  Every reduction runs in a fixed order (fixed grid, per-thread sums in
// track order, wave shuffles, LDS, then the per-block partials in block order), so two runs are bit-identical.
#include "cvhip_internal.hpp"
#include "tri_common.hpp"

#include <cmath>
#include <cstring>

namespace {

constexpr int MAXC = CVHIP_TRIANGULATE_MAX_CAMERAS;
constexpr int BA_MAX_ITERATIONS = 100;                    // :15 BUNDLE_ADJUSTMENT_MAX_ITERATIONS
constexpr double BA_INITIAL_MU = 1e-3;                    // :1687
constexpr double BA_GRADIENT_EPSILON = 1e-12;             // :1688
constexpr double BA_DELTA_EPSILON = 1e-12;                // :1689
constexpr double BA_RESIDUAL_EPSILON = 1e-12;             // :1690
constexpr double BA_RESIDUAL_REDUCTION_EPSILON = 0.0;     // :1691
constexpr int BLOCK = 256;
constexpr int MAX_GRID = 1024;

// Camera (:404-500) with what the kernels read: the projection, K, R, t, the centre, R^T t (point_depth), and the
// rotation-derivative terms of jacobian_a (:1706-1743): column i of d_translation_camerapose[:, 0:3] = Dr[i] * X + cr[i].
struct TriCam {
    double r[3], t[3];
    double K[9], R[9], C[3], Rt_t[3];
    double P[12];
    double Pg[12]; // K [R | t] of the caller's R: what triangulate_tracks projects with (the initial pair's p2, :737-740)
    double Dr[3][9];
    double cr[3][3];
};

// Camera::{matrix_r, center, projection} (:475-507) and the camera-only parts of jacobian_a (:1706-1743)
__host__ __device__ inline void cam_setup(TriCam &c, const double K[9], const double r[3], const double t[3])
{
    for (int i = 0; i < 3; i++) c.r[i] = r[i], c.t[i] = t[i];
    for (int i = 0; i < 9; i++) c.K[i] = K[i];
    matrix_r(r, c.R);
    for (int i = 0; i < 3; i++) {
        c.Rt_t[i] = c.R[i] * t[0] + c.R[3 + i] * t[1] + c.R[6 + i] * t[2]; // r_matrix.tr_mul(t)
        c.C[i] = -c.Rt_t[i];                                               // center (:487-489)
    }
    for (int i = 0; i < 3; i++) // projection = K [R | t] (:503-507)
        for (int j = 0; j < 4; j++) {
            double a0 = j < 3 ? c.R[j] : t[0], a1 = j < 3 ? c.R[3 + j] : t[1], a2 = j < 3 ? c.R[6 + j] : t[2];
            c.P[4 * i + j] = K[3 * i] * a0 + K[3 * i + 1] * a1 + K[3 * i + 2] * a2;
        }
    double un2 = r[0] * r[0] + r[1] * r[1] + r[2] * r[2];
    double ux[9] = {0.0, -r[2], r[1], r[2], 0.0, -r[0], -r[1], r[0], 0.0};
    if (sqrt(un2) > F64_EPS) {
        for (int i = 0; i < 3; i++) {
            // d_r_i = (u_i [u]x + [u x ((I - R) e_i)]x) R / |u|^2
            double v[3] = {(i == 0 ? 1.0 : 0.0) - c.R[i], (i == 1 ? 1.0 : 0.0) - c.R[3 + i], (i == 2 ? 1.0 : 0.0) - c.R[6 + i]};
            double w[3] = {r[1] * v[2] - r[2] * v[1], r[2] * v[0] - r[0] * v[2], r[0] * v[1] - r[1] * v[0]};
            double wx[9] = {0.0, -w[2], w[1], w[2], 0.0, -w[0], -w[1], w[0], 0.0};
            double m[9];
            for (int k = 0; k < 9; k++) m[k] = r[i] * ux[k] + wx[k];
            for (int a = 0; a < 3; a++)
                for (int b = 0; b < 3; b++)
                    c.Dr[i][3 * a + b] = (m[3 * a] * c.R[b] + m[3 * a + 1] * c.R[3 + b] + m[3 * a + 2] * c.R[6 + b]) / un2;
            c.cr[i][0] = c.cr[i][1] = c.cr[i][2] = 0.0;
        }
    } else {
        // near zero the reference copies -[u]x itself into the rotation columns (:1739-1743), independent of X
        for (int i = 0; i < 3; i++) {
            for (int k = 0; k < 9; k++) c.Dr[i][k] = 0.0;
            for (int a = 0; a < 3; a++) c.cr[i][a] = -ux[3 * a + i];
        }
    }
}

// ---- one track's view j: residual (:1768-1788), jacobian_b (:1750-1766), jacobian_a (:1694-1748) ----------------------
struct ViewJac {
    double dk[6]; // d_projection_hpoint * K (2 x 3)
    double q[3];
};

__device__ inline void view_dk(const TriCam &c, const double X[3], ViewJac &v)
{
    for (int i = 0; i < 3; i++) v.q[i] = ((c.P[4 * i] * X[0] + c.P[4 * i + 1] * X[1]) + c.P[4 * i + 2] * X[2]) + c.P[4 * i + 3];
    double u = v.q[0], vv = v.q[1], w = v.q[2];
    double d[6] = {1.0 / w, 0.0, -u / (w * w), 0.0, 1.0 / w, -vv / (w * w)};
    for (int a = 0; a < 2; a++)
        for (int b = 0; b < 3; b++) v.dk[3 * a + b] = (d[3 * a] * c.K[b] + d[3 * a + 1] * c.K[3 + b]) + d[3 * a + 2] * c.K[6 + b];
}

__device__ inline void jac_b(const TriCam &c, const ViewJac &v, double B[6])
{
    for (int a = 0; a < 2; a++)
        for (int b = 0; b < 3; b++) B[3 * a + b] = (v.dk[3 * a] * c.R[b] + v.dk[3 * a + 1] * c.R[3 + b]) + v.dk[3 * a + 2] * c.R[6 + b];
}

__device__ inline void jac_a(const TriCam &c, const ViewJac &v, const double X[3], double A[12])
{
    for (int i = 0; i < 3; i++) {
        double col[3];
        for (int a = 0; a < 3; a++)
            col[a] = ((c.Dr[i][3 * a] * X[0] + c.Dr[i][3 * a + 1] * X[1]) + c.Dr[i][3 * a + 2] * X[2]) + c.cr[i][a];
        for (int a = 0; a < 2; a++) A[6 * a + i] = (v.dk[3 * a] * col[0] + v.dk[3 * a + 1] * col[1]) + v.dk[3 * a + 2] * col[2];
    }
    for (int a = 0; a < 2; a++)
        for (int i = 0; i < 3; i++) A[6 * a + 3 + i] = v.dk[3 * a + i];
}

__device__ inline void residual(const ViewJac &v, int2 obs, double r[2])
{
    if (obs.x < 0) {
        r[0] = r[1] = 0.0;
        return;
    }
    r[0] = v.q[0] / v.q[2] - (double)obs.x;
    r[1] = v.q[1] / v.q[2] - (double)obs.y;
}

// V^-1 of calculate_v_inv (:1790-1798): V = mu I + sum over ALL views of B^T B (seen or not)
template <int M>
__device__ inline void v_inverse(const TriCam *cams, const double X[3], double mu, double Vi[9])
{
    double V[9] = {mu, 0.0, 0.0, 0.0, mu, 0.0, 0.0, 0.0, mu};
#pragma unroll
    for (int j = 0; j < M; j++) {
        ViewJac vj;
        view_dk(cams[j], X, vj);
        double B[6];
        jac_b(cams[j], vj, B);
        for (int a = 0; a < 3; a++)
            for (int b = 0; b < 3; b++) V[3 * a + b] += B[a] * B[b] + B[3 + a] * B[3 + b];
    }
    // symmetric positive definite: the pseudo-inverse is the inverse (adjugate / determinant)
    double c00 = V[4] * V[8] - V[5] * V[7], c01 = V[5] * V[6] - V[3] * V[8], c02 = V[3] * V[7] - V[4] * V[6];
    double det = V[0] * c00 + V[1] * c01 + V[2] * c02;
    double id = 1.0 / det;
    Vi[0] = c00 * id;
    Vi[1] = (V[2] * V[7] - V[1] * V[8]) * id;
    Vi[2] = (V[1] * V[5] - V[2] * V[4]) * id;
    Vi[3] = c01 * id;
    Vi[4] = (V[0] * V[8] - V[2] * V[6]) * id;
    Vi[5] = (V[2] * V[3] - V[0] * V[5]) * id;
    Vi[6] = c02 * id;
    Vi[7] = (V[1] * V[6] - V[0] * V[7]) * id;
    Vi[8] = (V[0] * V[4] - V[1] * V[3]) * id;
}

// W = A^T B (6 x 3)
__device__ inline void w_block(const double A[12], const double B[6], double W[18])
{
    for (int a = 0; a < 6; a++)
        for (int b = 0; b < 3; b++) W[3 * a + b] = A[a] * B[b] + A[6 + a] * B[3 + b];
}

// ---- fixed-order block reduction ----------------------------------------------------------------------------------------
__device__ inline double block_sum(double v, double *lds)
{
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    __syncthreads();
    if (lane == 0) lds[wave] = v;
    __syncthreads();
    double s = 0.0;
    if (threadIdx.x == 0)
        for (int w = 0; w < BLOCK / 64; w++) s += lds[w];
    return s;
}

__device__ inline double block_max(double v, double *lds)
{
    for (int off = 32; off > 0; off >>= 1) v = fmax(v, __shfl_down(v, off, 64));
    int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    __syncthreads();
    if (lane == 0) lds[wave] = v;
    __syncthreads();
    double s = -INFINITY;
    if (threadIdx.x == 0)
        for (int w = 0; w < BLOCK / 64; w++) s = fmax(s, lds[w]);
    return s;
}

// ---- triangulate_track (:867-911) + filter_outliers (:1559-1593), one track per lane ----------------------------------
// The DLT (Givens QR of the 2k x 4 system, one-sided Jacobi SVD of its R) is tri_common.hpp's, shared with pose recovery.
template <int M>
__global__ __launch_bounds__(BLOCK) void tri_dlt_filter_kernel(const int2 *__restrict__ tracks, uint64_t n,
                                                               const TriCam *__restrict__ cams, double cos_threshold,
                                                               double *__restrict__ pts, uint8_t *__restrict__ keep,
                                                               uint32_t *__restrict__ block_count)
{
    uint64_t i = (uint64_t)blockIdx.x * BLOCK + threadIdx.x;
    int ok = 0;
    double X[3] = {0.0, 0.0, 0.0};
    if (i < n) {
        double R[16];
        dlt_init(R);
        int seen = 0;
#pragma unroll
        for (int j = 0; j < M; j++) {
            int2 o = tracks[i * M + j];
            if (o.x < 0) continue;
            seen++;
            dlt_fold_view(R, cams[j].Pg, (double)o.x, (double)o.y);
        }
        if (seen >= 2) {
            double v4[4];
            ok = dlt_solve(R, v4, X) ? 1 : 0;
        }
        if (ok) {
            // filter_outliers: every seen view has the point in front (point_depth, :492-500; :1568-1578)
#pragma unroll
            for (int j = 0; j < M; j++) {
                if (tracks[i * M + j].x < 0) continue;
                const TriCam &c = cams[j];
                double q0 = X[0] + c.Rt_t[0], q1 = X[1] + c.Rt_t[1], q2 = X[2] + c.Rt_t[2];
                double depth = (c.R[6] * q0 + c.R[7] * q1) + c.R[8] * q2;
                if (!(depth > 0.0)) ok = 0;
            }
        }
        if (ok) {
            // min_ray_angle_cos (:996-1031): rays of the seen views, shorter than f64::EPSILON skipped; min |cos| of pairs
            double rays[M][3];
            bool has[M];
#pragma unroll
            for (int j = 0; j < M; j++) {
                has[j] = false;
                if (tracks[i * M + j].x < 0) continue;
                double d[3] = {X[0] - cams[j].C[0], X[1] - cams[j].C[1], X[2] - cams[j].C[2]};
                double nr = sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]);
                if (nr < F64_EPS) continue;
                for (int k = 0; k < 3; k++) rays[j][k] = d[k] / nr;
                has[j] = true;
            }
            bool any = false;
            double min_cos = 0.0;
#pragma unroll
            for (int a = 0; a < M; a++)
#pragma unroll
                for (int b = a + 1; b < M; b++) {
                    if (!has[a] || !has[b]) continue;
                    double c = fabs(rays[a][0] * rays[b][0] + rays[a][1] * rays[b][1] + rays[a][2] * rays[b][2]);
                    min_cos = any ? fmin(min_cos, c) : c;
                    any = true;
                }
            if (!any || min_cos > cos_threshold) ok = 0; // :1580-1587
        }
        for (int k = 0; k < 3; k++) pts[3 * i + k] = X[k];
        keep[i] = (uint8_t)ok;
    }
    uint32_t cnt = __syncthreads_count(ok);
    if (threadIdx.x == 0) block_count[blockIdx.x] = cnt;
}

// exclusive scan of the block counts, one block: each thread scans a contiguous chunk
__global__ __launch_bounds__(BLOCK) void tri_scan_kernel(uint32_t *__restrict__ counts, uint32_t nb, uint64_t *__restrict__ total)
{
    __shared__ uint64_t part[BLOCK];
    uint32_t chunk = (nb + BLOCK - 1) / BLOCK;
    uint32_t b0 = threadIdx.x * chunk, b1 = min(nb, b0 + chunk);
    uint64_t s = 0;
    for (uint32_t b = b0; b < b1; b++) s += counts[b];
    part[threadIdx.x] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint64_t acc = 0;
        for (int t = 0; t < BLOCK; t++) {
            uint64_t v = part[t];
            part[t] = acc;
            acc += v;
        }
        *total = acc;
    }
    __syncthreads();
    uint64_t acc = part[threadIdx.x];
    for (uint32_t b = b0; b < b1; b++) {
        uint32_t v = counts[b];
        counts[b] = (uint32_t)acc; // < 2^32: n is limited to 2^32 - 1 tracks
        acc += v;
    }
}

// retain in track order (:1590)
__global__ __launch_bounds__(BLOCK) void tri_compact_kernel(const uint8_t *__restrict__ keep, const double *__restrict__ pts,
                                                            uint64_t n, const uint32_t *__restrict__ offsets,
                                                            double *__restrict__ out_pts, uint64_t *__restrict__ out_idx)
{
    __shared__ uint32_t wave_cnt[BLOCK / 64];
    uint64_t i = (uint64_t)blockIdx.x * BLOCK + threadIdx.x;
    int k = i < n ? keep[i] : 0;
    uint64_t bal = __ballot(k);
    int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint32_t below = __popcll(bal & ((lane == 0) ? 0ull : (~0ull >> (64 - lane))));
    if (lane == 0) wave_cnt[wave] = __popcll(bal);
    __syncthreads();
    uint32_t off = offsets[blockIdx.x];
    for (int w = 0; w < wave; w++) off += wave_cnt[w];
    if (k) {
        uint64_t o = off + below;
        for (int c = 0; c < 3; c++) out_pts[3 * o + c] = pts[3 * i + c];
        out_idx[o] = i;
    }
}

// ---- BundleAdjustment::optimize (:2042-2147) on the device ---------------------------------------------------------------
enum { BA_RUNNING = 0, BA_FOUND = 1, BA_DELTA_FAILED = 2 };

struct BaState {
    double mu, nu;
    double residual_ns, new_ns, rho;
    double ga[6 * MAXC];
    double gmax;
    double da[6 * MAXC];
    double da_sq, da_rho, cam_sq;
    int status, accepted, converged, iterations;
    uint8_t history[BA_MAX_ITERATIONS];
};

// calculate_delta_step's reduction (:1903-1962): blockIdx.y = 2 (j M + k) + h for rows 3h..3h+2 of the camera block (j, k)
// of S (18 entries), or M * M * 2 + j for e_j (6) - half a block per slice keeps the accumulators in registers.  Each
// thread sums its tracks (grid stride, track order), the block sums its threads (wave shuffles, then 4 waves).
template <int M>
__global__ __launch_bounds__(BLOCK) void ba_schur_kernel(const int2 *__restrict__ tracks, const double *__restrict__ X_,
                                                         uint64_t n, const TriCam *__restrict__ cams,
                                                         const BaState *__restrict__ st, double *__restrict__ part)
{
    __shared__ double lds[BLOCK / 64];
    if (st->status != BA_RUNNING) return;
    const double mu = st->mu;
    const int y = blockIdx.y;
    const bool is_e = y >= 2 * M * M;
    const int blk = y / 2, h = y % 2;
    const int j = is_e ? y - 2 * M * M : blk / M, k = is_e ? j : blk % M;
    double acc[18];
    for (int a = 0; a < 18; a++) acc[a] = 0.0;
    for (uint64_t i = (uint64_t)blockIdx.x * BLOCK + threadIdx.x; i < n; i += (uint64_t)gridDim.x * BLOCK) {
        double X[3] = {X_[3 * i], X_[3 * i + 1], X_[3 * i + 2]};
        double Vi[9];
        v_inverse<M>(cams, X, mu, Vi);
        ViewJac vj;
        view_dk(cams[j], X, vj);
        double Aj[12], Bj[6], Wj[18];
        jac_a(cams[j], vj, X, Aj);
        jac_b(cams[j], vj, Bj);
        w_block(Aj, Bj, Wj);
        if (is_e) {
            // e_j += A_j^T r_j - Y_j (B_j^T r_j), Y_j = W_j V^-1   (:1953-1958)
            double r[2];
            residual(vj, tracks[i * M + j], r);
            double rb[3];
            for (int b = 0; b < 3; b++) rb[b] = Bj[b] * r[0] + Bj[3 + b] * r[1];
            for (int a = 0; a < 6; a++) {
                double ya[3];
                for (int b = 0; b < 3; b++) ya[b] = (Wj[3 * a] * Vi[b] + Wj[3 * a + 1] * Vi[3 + b]) + Wj[3 * a + 2] * Vi[6 + b];
                double ra = Aj[a] * r[0] + Aj[6 + a] * r[1];
                acc[a] += ra - ((ya[0] * rb[0] + ya[1] * rb[1]) + ya[2] * rb[2]);
            }
        } else {
            // S_jk += [j == k] U_j - Y_j W_k^T   (:1925-1950), rows a0..a0+2
            // (rows picked by selects between compile-time indices: a register array indexed at run time goes to scratch)
            double Y[9], Ar[6];
            for (int a = 0; a < 3; a++) {
                double w0 = h ? Wj[3 * (a + 3)] : Wj[3 * a], w1 = h ? Wj[3 * (a + 3) + 1] : Wj[3 * a + 1];
                double w2 = h ? Wj[3 * (a + 3) + 2] : Wj[3 * a + 2];
                for (int b = 0; b < 3; b++) Y[3 * a + b] = (w0 * Vi[b] + w1 * Vi[3 + b]) + w2 * Vi[6 + b];
                Ar[a] = h ? Aj[a + 3] : Aj[a];
                Ar[3 + a] = h ? Aj[9 + a] : Aj[6 + a];
            }
            double Wk[18];
            if (k == j) {
                for (int a = 0; a < 18; a++) Wk[a] = Wj[a];
            } else {
                ViewJac vk;
                view_dk(cams[k], X, vk);
                double Ak[12], Bk[6];
                jac_a(cams[k], vk, X, Ak);
                jac_b(cams[k], vk, Bk);
                w_block(Ak, Bk, Wk);
            }
            for (int a = 0; a < 3; a++)
                for (int b = 0; b < 6; b++) {
                    double u = k == j ? Ar[a] * Aj[b] + Ar[3 + a] * Aj[6 + b] : 0.0;
                    double yw = (Y[3 * a] * Wk[3 * b] + Y[3 * a + 1] * Wk[3 * b + 1]) + Y[3 * a + 2] * Wk[3 * b + 2];
                    acc[6 * a + b] += u - yw;
                }
        }
    }
    const int nv = is_e ? 6 : 18;
    const size_t base = is_e ? (size_t)M * M * 36 + (size_t)j * 6 : (size_t)blk * 36 + (size_t)h * 18;
#pragma unroll
    for (int a = 0; a < 18; a++) {
        if (a < nv) { // (uniform over the block)
            double s = block_sum(acc[a], lds);
            if (threadIdx.x == 0) part[(base + a) * gridDim.x + blockIdx.x] = s;
        }
    }
}

// sum of the per-block partials of quantity q in block order -> out[q]
__global__ void ba_reduce_kernel(const double *__restrict__ part, uint32_t nq, uint32_t nb, double *__restrict__ out)
{
    uint32_t q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= nq) return;
    double s = 0.0;
    for (uint32_t b = 0; b < nb; b++) s += part[(size_t)q * nb + b];
    out[q] = s;
}

// S + mu I, s.lu().solve(&e) (partial pivoting; None when U has a zero pivot) (:1964-1973), then the camera part of the
// step's sums and the candidate cameras (update_params, :2012-2024).  One thread; S is 6m x 6m.
template <int M>
__global__ void ba_solve_kernel(double *__restrict__ se, BaState *__restrict__ st, const TriCam *__restrict__ cams,
                                TriCam *__restrict__ cand)
{
    if (st->status != BA_RUNNING) return;
    constexpr int N = 6 * M;
    // se holds S as its camera blocks (j, k), 36 entries each (row-major within the block), then e
    auto S = [&](int r, int c) -> double & { return se[((r / 6) * M + (c / 6)) * 36 + (r % 6) * 6 + (c % 6)]; };
    double *e = se + (size_t)M * M * 36;
    for (int d = 0; d < N; d++) S(d, d) += st->mu;
    double *b = st->da; // solved in place: delta_a
    for (int r = 0; r < N; r++) b[r] = e[r];
    bool ok = true;
    for (int c = 0; c < N && ok; c++) {
        int p = c;
        double pv = fabs(S(c, c));
        for (int r = c + 1; r < N; r++)
            if (fabs(S(r, c)) > pv) pv = fabs(S(r, c)), p = r;
        if (pv == 0.0) {
            ok = false;
            break;
        }
        if (p != c) {
            for (int l = 0; l < N; l++) {
                double t = S(c, l);
                S(c, l) = S(p, l);
                S(p, l) = t;
            }
            double t = b[c];
            b[c] = b[p];
            b[p] = t;
        }
        for (int r = c + 1; r < N; r++) {
            double f = S(r, c) / S(c, c);
            for (int l = c + 1; l < N; l++) S(r, l) -= f * S(c, l);
            b[r] -= f * b[c];
        }
    }
    if (ok)
        for (int r = N - 1; r >= 0; r--) {
            double s = b[r];
            for (int l = r + 1; l < N; l++) s -= S(r, l) * b[l];
            b[r] = s / S(r, r);
            if (!isfinite(b[r])) ok = false;
        }
    if (!ok) {
        st->status = BA_DELTA_FAILED;
        return;
    }
    double da_sq = 0.0, da_rho = 0.0, cam_sq = 0.0;
    for (int r = 0; r < N; r++) {
        da_sq += b[r] * b[r];
        da_rho += b[r] * (b[r] * st->mu + st->ga[r]);
    }
    for (int j = 0; j < M; j++) {
        const TriCam &c = cams[j];
        cam_sq += (c.r[0] * c.r[0] + c.r[1] * c.r[1] + c.r[2] * c.r[2]) + (c.t[0] * c.t[0] + c.t[1] * c.t[1] + c.t[2] * c.t[2]);
        double r[3] = {c.r[0] + b[6 * j], c.r[1] + b[6 * j + 1], c.r[2] + b[6 * j + 2]};
        double t[3] = {c.t[0] + b[6 * j + 3], c.t[1] + b[6 * j + 4], c.t[2] + b[6 * j + 5]};
        cam_setup(cand[j], c.K, r, t);
    }
    st->da_sq = da_sq;
    st->da_rho = da_rho;
    st->cam_sq = cam_sq;
}

// delta_b per track (:1975-2007), its sums (||delta||, rho's denominator), params_norm's point part, the updated point
// (kept apart: the old one stays for a rejected step) and the new residual under the candidate cameras (:2076-2086).
template <int M>
__global__ __launch_bounds__(BLOCK) void ba_step_kernel(const int2 *__restrict__ tracks, const double *__restrict__ X_,
                                                        double *__restrict__ Xn_, const double *__restrict__ gb, uint64_t n,
                                                        const TriCam *__restrict__ cams, const TriCam *__restrict__ cand,
                                                        const BaState *__restrict__ st, double *__restrict__ part)
{
    __shared__ double lds[BLOCK / 64];
    if (st->status != BA_RUNNING) return;
    const double mu = st->mu;
    double s_db = 0.0, s_rho = 0.0, s_x = 0.0, s_res = 0.0;
    for (uint64_t i = (uint64_t)blockIdx.x * BLOCK + threadIdx.x; i < n; i += (uint64_t)gridDim.x * BLOCK) {
        double X[3] = {X_[3 * i], X_[3 * i + 1], X_[3 * i + 2]};
        double Vi[9];
        v_inverse<M>(cams, X, mu, Vi);
        double db[3] = {0.0, 0.0, 0.0};
#pragma unroll
        for (int j = 0; j < M; j++) {
            ViewJac vj;
            view_dk(cams[j], X, vj);
            double A[12], B[6], W[18], r[2];
            jac_a(cams[j], vj, X, A);
            jac_b(cams[j], vj, B);
            w_block(A, B, W);
            residual(vj, tracks[i * M + j], r);
            double rb[3], wd[3];
            for (int b = 0; b < 3; b++) {
                rb[b] = B[b] * r[0] + B[3 + b] * r[1];
                double s = 0.0;
                for (int a = 0; a < 6; a++) s += W[3 * a + b] * st->da[6 * j + a];
                wd[b] = s;
            }
            for (int a = 0; a < 3; a++) {
                double v1 = (Vi[3 * a] * rb[0] + Vi[3 * a + 1] * rb[1]) + Vi[3 * a + 2] * rb[2];
                double v2 = (Vi[3 * a] * wd[0] + Vi[3 * a + 1] * wd[1]) + Vi[3 * a + 2] * wd[2];
                db[a] += v1 - v2;
            }
        }
        double Xn[3];
        for (int a = 0; a < 3; a++) {
            s_db += db[a] * db[a];
            s_rho += db[a] * (db[a] * mu + gb[3 * i + a]);
            s_x += X[a] * X[a];
            Xn[a] = X[a] + db[a];
            Xn_[3 * i + a] = Xn[a];
        }
#pragma unroll
        for (int j = 0; j < M; j++) {
            ViewJac vj;
            view_dk(cand[j], Xn, vj);
            double r[2];
            residual(vj, tracks[i * M + j], r);
            s_res += r[0] * r[0] + r[1] * r[1];
        }
    }
    double v[4] = {s_db, s_rho, s_x, s_res};
    for (int q = 0; q < 4; q++) {
        double s = block_sum(v[q], lds);
        if (threadIdx.x == 0) part[(size_t)q * gridDim.x + blockIdx.x] = s;
    }
}

// the delta test, rho and the accept / reject decision (:2058-2127).  One thread.
template <int M>
__global__ void ba_decide_kernel(const double *__restrict__ part, uint32_t nb, BaState *__restrict__ st,
                                 TriCam *__restrict__ cams, const TriCam *__restrict__ cand)
{
    if (st->status != BA_RUNNING) return;
    double s[4];
    for (int q = 0; q < 4; q++) {
        double a = 0.0;
        for (uint32_t b = 0; b < nb; b++) a += part[(size_t)q * nb + b];
        s[q] = a;
    }
    double params_norm = sqrt(st->cam_sq + s[2]);
    double delta_norm = sqrt(st->da_sq + s[0]);
    st->accepted = 0;
    if (delta_norm <= BA_DELTA_EPSILON * (params_norm + BA_DELTA_EPSILON)) {
        st->status = BA_FOUND;
        return;
    }
    double old_ns = st->residual_ns, new_ns = s[3];
    double rho = (old_ns - new_ns) / (st->da_rho + s[1]);
    st->rho = rho;
    st->new_ns = new_ns;
    st->history[st->iterations] = rho > 0.0 ? 1 : 0;
    if (rho > 0.0) {
        st->accepted = 1;
        st->converged = sqrt(old_ns) - sqrt(new_ns) < BA_RESIDUAL_REDUCTION_EPSILON * sqrt(old_ns);
        for (int j = 0; j < M; j++) cams[j] = cand[j];
    } else {
        st->mu *= st->nu;
        st->nu *= 2.0;
    }
}

// calculate_jt_residual (:1840-1895) and calculate_residual_vector's norm (:1800-1838).  init = 1: the first evaluation;
// otherwise only after an accepted step, which it commits (the new points become the current ones).  blockIdx.y = a group
// of up to JTR_GROUP cameras whose part of J^T r the slice sums; slice 0 also commits, and writes the point part (per
// track), its largest element and the residual norm.
constexpr int JTR_GROUP = 4;
template <int M>
__global__ __launch_bounds__(BLOCK) void ba_jtr_kernel(const int2 *__restrict__ tracks, double *__restrict__ X_,
                                                       const double *__restrict__ Xn_, double *__restrict__ gb, uint64_t n,
                                                       const TriCam *__restrict__ cams, const BaState *__restrict__ st,
                                                       int init, double *__restrict__ part, double *__restrict__ part_max)
{
    __shared__ double lds[BLOCK / 64];
    if (!init && (st->status != BA_RUNNING || !st->accepted)) return;
    const bool first = blockIdx.y == 0;
    const int j0 = blockIdx.y * JTR_GROUP;
    double acc[6 * JTR_GROUP];
    for (int a = 0; a < 6 * JTR_GROUP; a++) acc[a] = 0.0;
    double s_res = 0.0, gmax = -INFINITY;
    for (uint64_t i = (uint64_t)blockIdx.x * BLOCK + threadIdx.x; i < n; i += (uint64_t)gridDim.x * BLOCK) {
        double X[3];
        for (int a = 0; a < 3; a++) X[a] = init ? X_[3 * i + a] : Xn_[3 * i + a];
        if (first) {
            double g[3] = {0.0, 0.0, 0.0};
#pragma unroll
            for (int j = 0; j < M; j++) {
                ViewJac vj;
                view_dk(cams[j], X, vj);
                double B[6], r[2];
                jac_b(cams[j], vj, B);
                residual(vj, tracks[i * M + j], r);
                s_res += r[0] * r[0] + r[1] * r[1];
                for (int b = 0; b < 3; b++) g[b] += B[b] * r[0] + B[3 + b] * r[1];
            }
            for (int b = 0; b < 3; b++) {
                gb[3 * i + b] = g[b];
                gmax = fmax(gmax, g[b]);
                if (!init) X_[3 * i + b] = X[b];
            }
        }
#pragma unroll
        for (int jj = 0; jj < JTR_GROUP; jj++) {
            const int j = j0 + jj;
            if (j >= M) continue;
            ViewJac vj;
            view_dk(cams[j], X, vj);
            double A[12], r[2];
            jac_a(cams[j], vj, X, A);
            residual(vj, tracks[i * M + j], r);
            for (int a = 0; a < 6; a++) acc[6 * jj + a] += A[a] * r[0] + A[6 + a] * r[1];
        }
    }
#pragma unroll
    for (int a = 0; a < 6 * JTR_GROUP; a++) {
        if (j0 * 6 + a < 6 * M) { // (uniform over the block)
            double s = block_sum(acc[a], lds);
            if (threadIdx.x == 0) part[(size_t)(6 * j0 + a) * gridDim.x + blockIdx.x] = s;
        }
    }
    if (first) {
        double s = block_sum(s_res, lds);
        if (threadIdx.x == 0) part[(size_t)(6 * M) * gridDim.x + blockIdx.x] = s;
        double mx = block_max(gmax, lds);
        if (threadIdx.x == 0) part_max[blockIdx.x] = mx;
    }
}

// after the (re)evaluation of J^T r: the gradient test, mu / nu (:2048-2052, :2101-2116), the residual test (:2130-2133)
template <int M>
__global__ void ba_finish_kernel(const double *__restrict__ sums, const double *__restrict__ part_max, uint32_t nb,
                                 BaState *__restrict__ st, int init)
{
    if (!init && st->status != BA_RUNNING) return;
    bool fresh = init || st->accepted;
    if (fresh) {
        double gmax = -INFINITY;
        for (int a = 0; a < 6 * M; a++) {
            st->ga[a] = sums[a];
            gmax = fmax(gmax, sums[a]);
        }
        for (uint32_t b = 0; b < nb; b++) gmax = fmax(gmax, part_max[b]);
        st->gmax = gmax;
        st->residual_ns = sums[6 * M];
    }
    if (init) {
        st->mu = BA_INITIAL_MU;
        st->nu = 2.0;
        st->iterations = 0;
        st->status = fabs(st->gmax) <= BA_GRADIENT_EPSILON ? BA_FOUND : BA_RUNNING;
        return;
    }
    st->iterations += 1;
    if (st->accepted) {
        if (st->converged || fabs(st->gmax) <= BA_GRADIENT_EPSILON) {
            st->status = BA_FOUND;
            return;
        }
        double rho = st->rho;
        st->mu *= fmax(1.0 / 3.0, 1.0 - pow(2.0 * rho - 1.0, 3.0));
        st->nu = 2.0;
    }
    if (sqrt(st->residual_ns) <= BA_RESIDUAL_EPSILON) st->status = BA_FOUND;
}

struct Args {
    cvhip_device *dev;
    const int32_t *tracks;
    uint64_t n;
    uint32_t m;
    const double *K, *R, *t;
    const double *rv, *P; // cvhip_triangulate_perspective_cameras: the cameras' r and projections as held (else NULL)
    int bundle_adjustment;
    double *out_points;
    uint64_t *out_index;
    double *out_r, *out_t, *out_projection;
    uint64_t *out_n;
    uint32_t *out_iterations;
    uint8_t *out_history;
    double *out_residual_norms;
    cvhip_progress_fn progress;
    void *user;
};

const char what[] = "triangulate_perspective";

template <int M>
int run(const Args &a)
{
    using namespace cvhip;
    hipStream_t s = a.dev->d.stream;
    const uint64_t n = a.n;
    CallScratch sc;
    int2 *d_tracks = nullptr;
    double *d_pts = nullptr, *d_Xn = nullptr, *d_gb = nullptr, *d_kept = nullptr, *d_part = nullptr, *d_part_max = nullptr, *d_sums = nullptr;
    uint8_t *d_keep = nullptr;
    uint32_t *d_counts = nullptr;
    uint64_t *d_idx = nullptr, *d_total = nullptr;
    TriCam *d_cams = nullptr, *d_cand = nullptr;
    BaState *d_st = nullptr;
    const uint32_t nb = (uint32_t)((n + BLOCK - 1) / BLOCK);
    TriCam hc[M];
    for (int j = 0; j < M; j++) {
        if (a.rv) { // a camera as the reference holds it: r and the projection the DLT uses, both given
            cam_setup(hc[j], a.K + 9 * j, a.rv + 3 * j, a.t + 3 * j);
            std::memcpy(hc[j].Pg, a.P + 12 * j, 96);
            continue;
        }
        double r[3];
        from_matrix(a.R + 9 * j, r);
        cam_setup(hc[j], a.K + 9 * j, r, a.t + 3 * j);
        given_projection(a.K + 9 * j, a.R + 9 * j, a.t + 3 * j, hc[j].Pg);
    }
    const size_t tb = (size_t)n * M * sizeof(int2);
    // an owned copy of the table, whoever holds it: the bundle adjustment compacts it in place
    CVHIP_TRY_HIP_AT(what, sc.copy_in(reinterpret_cast<const int2 *>(a.tracks), (size_t)n * M, &d_tracks, s));
    CVHIP_TRY_HIP_AT(what, sc.alloc(&d_pts, (size_t)n * 3));
    CVHIP_TRY_HIP_AT(what, sc.alloc(&d_kept, (size_t)n * 3));
    CVHIP_TRY_HIP_AT(what, sc.alloc(&d_idx, (size_t)n));
    CVHIP_TRY_HIP_AT(what, sc.alloc(&d_keep, (size_t)n));
    CVHIP_TRY_HIP_AT(what, sc.alloc(&d_counts, (size_t)nb));
    CVHIP_TRY_HIP_AT(what, sc.alloc(&d_total, 1));
    CVHIP_TRY_HIP_AT(what, sc.alloc(&d_cams, M));
    CVHIP_TRY_HIP_AT(what, sc.alloc(&d_cand, M));
    CVHIP_TRY_HIP_AT(what, hipMemcpyAsync(d_cams, hc, sizeof(TriCam) * M, hipMemcpyHostToDevice, s));
    // triangulate_tracks + filter_outliers (:821, :832)
    const double cos_threshold = std::cos(0.5 * M_PI / 180.0); // MIN_ANGLE_BETWEEN_RAYS.cos()
    hipLaunchKernelGGL(tri_dlt_filter_kernel<M>, dim3(nb), dim3(BLOCK), 0, s, d_tracks, n, d_cams, cos_threshold, d_pts,
                       d_keep, d_counts);
    CVHIP_TRY_HIP_AT(what, hipGetLastError());
    hipLaunchKernelGGL(tri_scan_kernel, dim3(1), dim3(BLOCK), 0, s, d_counts, nb, d_total);
    CVHIP_TRY_HIP_AT(what, hipGetLastError());
    hipLaunchKernelGGL(tri_compact_kernel, dim3(nb), dim3(BLOCK), 0, s, d_keep, d_pts, n, d_counts, d_kept, d_idx);
    CVHIP_TRY_HIP_AT(what, hipGetLastError());
    uint64_t kept = 0;
    CVHIP_TRY_HIP_AT(what, hipMemcpyAsync(&kept, d_total, 8, hipMemcpyDeviceToHost, s));
    CVHIP_TRY_HIP_AT(what, hipStreamSynchronize(s));

    BaState hs;
    std::memset(&hs, 0, sizeof(hs));
    std::memset(hs.history, 0xFF, sizeof(hs.history));
    double norms[2] = {NAN, NAN};
    if (a.bundle_adjustment && kept > 0) {
        // BundleAdjustment over the surviving tracks (:1544-1556): compact the track table the same way
        const uint64_t nk = kept;
        int2 *ktracks = nullptr;
        {
            std::vector<uint64_t> hidx(nk);
            std::vector<int2> htr(n * M), hk(nk * M);
            CVHIP_TRY_HIP_AT(what, hipMemcpyAsync(hidx.data(), d_idx, nk * 8, hipMemcpyDeviceToHost, s));
            CVHIP_TRY_HIP_AT(what, hipMemcpyAsync(htr.data(), d_tracks, tb, hipMemcpyDeviceToHost, s));
            CVHIP_TRY_HIP_AT(what, hipStreamSynchronize(s));
            for (uint64_t i = 0; i < nk; i++)
                for (int j = 0; j < M; j++) hk[i * M + j] = htr[hidx[i] * M + j];
            CVHIP_TRY_HIP_AT(what, hipMemcpyAsync(d_tracks, hk.data(), nk * M * sizeof(int2), hipMemcpyHostToDevice, s));
            CVHIP_TRY_HIP_AT(what, hipStreamSynchronize(s));
            ktracks = d_tracks;
        }
        const uint32_t G = (uint32_t)std::min<uint64_t>((nk + BLOCK - 1) / BLOCK, MAX_GRID);
        const uint32_t nq_s = 36 * M * M + 6 * M, nq_j = 6 * M + 1;
        CVHIP_TRY_HIP_AT(what, sc.alloc(&d_Xn, (size_t)nk * 3));
        CVHIP_TRY_HIP_AT(what, sc.alloc(&d_gb, (size_t)nk * 3));
        CVHIP_TRY_HIP_AT(what, sc.alloc(&d_part, (size_t)std::max(nq_s, nq_j) * G));
        CVHIP_TRY_HIP_AT(what, sc.alloc(&d_part_max, (size_t)G));
        CVHIP_TRY_HIP_AT(what, sc.alloc(&d_sums, (size_t)nq_s));
        CVHIP_TRY_HIP_AT(what, sc.alloc(&d_st, 1));
        CVHIP_TRY_HIP_AT(what, hipMemcpyAsync(d_st, &hs, sizeof(hs), hipMemcpyHostToDevice, s));
        double *X = d_kept;
        // initial residual and J^T r (:2045-2052)
        hipLaunchKernelGGL(ba_jtr_kernel<M>, dim3(G, (M + JTR_GROUP - 1) / JTR_GROUP), dim3(BLOCK), 0, s, ktracks, X, d_Xn, d_gb, nk, d_cams, d_st, 1, d_part, d_part_max);
        hipLaunchKernelGGL(ba_reduce_kernel, dim3((nq_j + 63) / 64), dim3(64), 0, s, d_part, nq_j, G, d_sums);
        hipLaunchKernelGGL(ba_finish_kernel<M>, dim3(1), dim3(1), 0, s, d_sums, d_part_max, G, d_st, 1);
        CVHIP_TRY_HIP_AT(what, hipGetLastError());
        CVHIP_TRY_HIP_AT(what, hipMemcpyAsync(&hs, d_st, sizeof(hs), hipMemcpyDeviceToHost, s));
        CVHIP_TRY_HIP_AT(what, hipStreamSynchronize(s));
        norms[0] = std::sqrt(hs.residual_ns);
        int it = 0;
        for (; hs.status == BA_RUNNING && it < BA_MAX_ITERATIONS; it++) {
            if (a.progress) a.progress(a.user, (float)it / (float)BA_MAX_ITERATIONS); // :2054-2056
            hipLaunchKernelGGL(ba_schur_kernel<M>, dim3(G, 2 * M * M + M), dim3(BLOCK), 0, s, ktracks, X, nk, d_cams, d_st, d_part);
            hipLaunchKernelGGL(ba_reduce_kernel, dim3((nq_s + 63) / 64), dim3(64), 0, s, d_part, nq_s, G, d_sums);
            hipLaunchKernelGGL(ba_solve_kernel<M>, dim3(1), dim3(1), 0, s, d_sums, d_st, d_cams, d_cand);
            hipLaunchKernelGGL(ba_step_kernel<M>, dim3(G), dim3(BLOCK), 0, s, ktracks, X, d_Xn, d_gb, nk, d_cams, d_cand, d_st, d_part);
            hipLaunchKernelGGL(ba_decide_kernel<M>, dim3(1), dim3(1), 0, s, d_part, G, d_st, d_cams, d_cand);
            hipLaunchKernelGGL(ba_jtr_kernel<M>, dim3(G, (M + JTR_GROUP - 1) / JTR_GROUP), dim3(BLOCK), 0, s, ktracks, X, d_Xn, d_gb, nk, d_cams, d_st, 0, d_part, d_part_max);
            hipLaunchKernelGGL(ba_reduce_kernel, dim3((nq_j + 63) / 64), dim3(64), 0, s, d_part, nq_j, G, d_sums);
            hipLaunchKernelGGL(ba_finish_kernel<M>, dim3(1), dim3(1), 0, s, d_sums, d_part_max, G, d_st, 0);
            CVHIP_TRY_HIP_AT(what, hipGetLastError());
            // one small readback per iteration: the loop's state word
            CVHIP_TRY_HIP_AT(what, hipMemcpyAsync(&hs.status, (const char *)d_st + offsetof(BaState, status), sizeof(int), hipMemcpyDeviceToHost, s));
            CVHIP_TRY_HIP_AT(what, hipStreamSynchronize(s));
        }
        CVHIP_TRY_HIP_AT(what, hipMemcpyAsync(&hs, d_st, sizeof(hs), hipMemcpyDeviceToHost, s));
        CVHIP_TRY_HIP_AT(what, hipMemcpyAsync(hc, d_cams, sizeof(TriCam) * M, hipMemcpyDeviceToHost, s));
        CVHIP_TRY_HIP_AT(what, hipStreamSynchronize(s));
        norms[1] = std::sqrt(hs.residual_ns);
        if (a.out_iterations) *a.out_iterations = (uint32_t)hs.iterations;
        if (a.out_history) std::memcpy(a.out_history, hs.history, BA_MAX_ITERATIONS);
        if (a.out_residual_norms) std::memcpy(a.out_residual_norms, norms, sizeof(norms));
        if (hs.status == BA_DELTA_FAILED) return fail(CVHIP_ERR_NO_SURFACE, "Failed to compute delta vector");
        if (hs.status != BA_FOUND) return fail(CVHIP_ERR_NO_SURFACE, "Levenberg-Marquardt failed to converge");
    } else {
        if (a.out_iterations) *a.out_iterations = 0;
        if (a.out_history) std::memcpy(a.out_history, hs.history, BA_MAX_ITERATIONS);
        if (a.out_residual_norms) std::memcpy(a.out_residual_norms, norms, sizeof(norms));
    }
    if (kept) {
        CVHIP_TRY_HIP_AT(what, sc.copy_out(a.out_points, d_kept, (size_t)kept * 3, s));
        CVHIP_TRY_HIP_AT(what, sc.copy_out(a.out_index, d_idx, (size_t)kept, s));
    }
    CVHIP_TRY_HIP_AT(what, hipStreamSynchronize(s));
    for (int j = 0; j < M; j++) {
        if (a.out_r) std::memcpy(a.out_r + 3 * j, hc[j].r, 24);
        if (a.out_t) std::memcpy(a.out_t + 3 * j, hc[j].t, 24);
        if (a.out_projection) std::memcpy(a.out_projection + 12 * j, hc[j].P, 96);
    }
    *a.out_n = kept;
    return CVHIP_OK;
}

} // namespace

namespace {
int triangulate_perspective(cvhip_device *dev, const int32_t *tracks, uint64_t n, uint32_t m, const double *K,
                            const double *R, const double *rv, const double *P, const double *t, int bundle_adjustment,
                            double *out_points, uint64_t *out_index, double *out_r, double *out_t, double *out_projection,
                            uint64_t *out_n, uint32_t *out_iterations, uint8_t *out_history, double *out_residual_norms,
                            cvhip_progress_fn progress, void *user)
{
    using cvhip::fail;
    if (!dev || !K || (!R && !(rv && P)) || !t || !out_n || (n && (!tracks || !out_points || !out_index)))
        return fail(CVHIP_ERR_INVALID, "null argument");
    if (m < 2) return fail(CVHIP_ERR_INVALID, "triangulate_perspective: at least two cameras are needed");
    if (m > CVHIP_TRIANGULATE_MAX_CAMERAS)
        return fail(CVHIP_ERR_UNSUPPORTED, "triangulate_perspective: more than " + std::to_string(CVHIP_TRIANGULATE_MAX_CAMERAS) + " cameras");
    if (n >= 0xFFFFFFFFull) return fail(CVHIP_ERR_UNSUPPORTED, "triangulate_perspective: 2^32 - 1 tracks or more");
    *out_n = 0;
    if (n == 0) { // nothing to triangulate: an empty surface with the cameras as given (BundleAdjustment returns at :2050)
        for (uint32_t j = 0; j < m; j++) {
            double r[3];
            TriCam c;
            if (rv) std::memcpy(r, rv + 3 * j, 24);
            else from_matrix(R + 9 * j, r);
            cam_setup(c, K + 9 * j, r, t + 3 * j);
            if (out_r) std::memcpy(out_r + 3 * j, c.r, 24);
            if (out_t) std::memcpy(out_t + 3 * j, c.t, 24);
            if (out_projection) std::memcpy(out_projection + 12 * j, c.P, 96);
        }
        if (out_iterations) *out_iterations = 0;
        if (out_history) std::memset(out_history, 0xFF, BA_MAX_ITERATIONS);
        if (out_residual_norms) out_residual_norms[0] = out_residual_norms[1] = NAN;
        return CVHIP_OK;
    }
    hipError_t e = hipSetDevice(dev->d.ordinal);
    if (e != hipSuccess) return fail(CVHIP_ERR_DEVICE, std::string("hipSetDevice: ") + hipGetErrorString(e));
    Args a{dev, tracks, n, m, K, R, t, rv, P, bundle_adjustment, out_points, out_index, out_r, out_t, out_projection, out_n,
           out_iterations, out_history, out_residual_norms, progress, user};
    switch (m) {
    case 2: return run<2>(a);
    case 3: return run<3>(a);
    case 4: return run<4>(a);
    case 5: return run<5>(a);
    case 6: return run<6>(a);
    case 7: return run<7>(a);
    default: return run<8>(a);
    }
}
} // namespace

extern "C" int cvhip_triangulate_perspective(cvhip_device *dev, const int32_t *tracks, uint64_t n, uint32_t m, const double *K,
                                             const double *R, const double *t, int bundle_adjustment, double *out_points,
                                             uint64_t *out_index, double *out_r, double *out_t, double *out_projection,
                                             uint64_t *out_n, uint32_t *out_iterations, uint8_t *out_history,
                                             double *out_residual_norms, cvhip_progress_fn progress, void *user)
{
    if (!R) return cvhip::fail(CVHIP_ERR_INVALID, "null argument");
    return triangulate_perspective(dev, tracks, n, m, K, R, nullptr, nullptr, t, bundle_adjustment, out_points, out_index,
                                   out_r, out_t, out_projection, out_n, out_iterations, out_history, out_residual_norms,
                                   progress, user);
}

extern "C" int cvhip_triangulate_perspective_cameras(cvhip_device *dev, const int32_t *tracks, uint64_t n, uint32_t m,
                                                     const double *K, const double *r, const double *t,
                                                     const double *projection, int bundle_adjustment, double *out_points,
                                                     uint64_t *out_index, double *out_r, double *out_t,
                                                     double *out_projection, uint64_t *out_n, uint32_t *out_iterations,
                                                     uint8_t *out_history, double *out_residual_norms,
                                                     cvhip_progress_fn progress, void *user)
{
    if (!r || !projection) return cvhip::fail(CVHIP_ERR_INVALID, "null argument");
    return triangulate_perspective(dev, tracks, n, m, K, nullptr, r, projection, t, bundle_adjustment, out_points,
                                   out_index, out_r, out_t, out_projection, out_n, out_iterations, out_history,
                                   out_residual_norms, progress, user);
}
