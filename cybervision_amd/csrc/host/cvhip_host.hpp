// cvhip_host.hpp — C++ host layer above the C ABI (include/cvhip.h).
//
// The reference's host code is Rust; its toolchain is absent here, so this header is the compiled
// host side that mirrors the reference's interface for the accelerated path — same names,
// argument meaning and error behaviour — and is what a C++ consumer (or a cxx-bridge) would use:
//
//   create_gpu_context(HardwareMode)                       src/correlation/mod.rs:145-147
//   PointCorrelations::{new, correlate_images, complete,   src/correlation/mod.rs:150-245, 542-550
//                       optimal_scale_steps, get_selected_hardware}, .correlated_points
//   orb::extract_points, orb::optimal_scale_steps          src/orb.rs:50-84, 407-415
//   KeypointMatching::new(...).matches                     src/pointmatching.rs:29-77
//   FundamentalMatrix::{new, find_ransac}                  src/fundamentalmatrix.rs:72-147
//   mesh::Mesh::create, mesh::depth_image                  src/output.rs:363-387, 1016-1143 (Delaunay: the caller's)
//
// Header-only, no dependencies beyond the C ABI and the C++17 standard library.  Nothing here does
// arithmetic on the dense/ORB/matcher path: it only calls libcvhip.so.  RANSAC keeps the reference's
// split: hypotheses are sampled and fitted on the host (as fundamentalmatrix.rs:155-190, 260-286
// do), every batch is scored on the GPU (cvhip_ransac_score), the best is chosen with the reference's
// ordering (:623-649).  Errors surface as exceptions carrying cvhip_last_error(), the analogue of
// Result<_, GpuError>; a failed GpuDevice construction is what makes the reference fall back to its
// CPU path (mod.rs:170-173) — here it simply throws, there is no CPU fallback in this library.
#pragma once

#include <algorithm>
#include <array>
#include <cmath>
#include <cstdint>
#include <optional>
#include <random>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include "../../../include/cvhip.h"

namespace cvhip_host {

struct GpuError : std::runtime_error { // GpuError (correlation/gpu/vulkan.rs:1204-1272)
    int code;
    GpuError(int c, const std::string &where)
        : std::runtime_error(where + ": " + cvhip_last_error()), code(c) {}
};
inline void check(int rc, const char *where)
{
    if (rc != CVHIP_OK) throw GpuError(rc, where);
}

enum class HardwareMode { Gpu, GpuLowPower, Cpu }; // correlation/mod.rs:49-54
enum class ProjectionMode { Affine, Perspective }; // correlation/mod.rs:43-47

template <typename T> struct Point2D { // data.rs:8-19
    T x, y;
};

template <typename T> class Grid { // data.rs:22-64: row-major, index = width*y + x
  public:
    Grid() = default;
    Grid(size_t width, size_t height, T v) : width_(width), height_(height), data_(width * height, v) {}
    size_t width() const { return width_; }
    size_t height() const { return height_; }
    const T &val(size_t x, size_t y) const { return data_.at(width_ * y + x); }
    T &val_mut(size_t x, size_t y) { return data_.at(width_ * y + x); }
    const T *data() const { return data_.data(); }
    T *data() { return data_.data(); }

  private:
    size_t width_ = 0, height_ = 0;
    std::vector<T> data_;
};

using Match = std::pair<Point2D<uint32_t>, float>; // correlation/mod.rs:33

class GpuDevice { // GpuDevice = DefaultDeviceContext (correlation/mod.rs:35)
  public:
    explicit GpuDevice(HardwareMode mode, int ordinal = -1)
    {
        if (mode == HardwareMode::Cpu) throw std::invalid_argument("HardwareMode::Cpu has no GPU device");
        check(cvhip_device_create(mode == HardwareMode::GpuLowPower ? 1 : 0, ordinal, &dev_), "cvhip_device_create");
    }
    ~GpuDevice() { cvhip_device_destroy(dev_); }
    GpuDevice(const GpuDevice &) = delete;
    GpuDevice &operator=(const GpuDevice &) = delete;
    cvhip_device *handle() const { return dev_; }
    std::string name() const { return cvhip_device_name(dev_); }

  private:
    cvhip_device *dev_ = nullptr;
};
inline GpuDevice create_gpu_context(HardwareMode mode) { return GpuDevice(mode); } // mod.rs:145-147 (guaranteed elision)

class PointCorrelations { // correlation/mod.rs:63-245, GPU branch
  public:
    Grid<std::optional<Match>> correlated_points;

    PointCorrelations(GpuDevice &dev, std::pair<uint32_t, uint32_t> img1_dimensions,
                      std::pair<uint32_t, uint32_t> img2_dimensions, const std::array<double, 9> &fundamental_matrix,
                      ProjectionMode projection_mode)
        : dims1_(img1_dimensions), selected_hardware_("GPU " + dev.name())
    {
        check(cvhip_ctx_create(dev.handle(), img1_dimensions.first, img1_dimensions.second, img2_dimensions.first,
                               img2_dimensions.second, projection_mode == ProjectionMode::Perspective ? 1 : 0,
                               fundamental_matrix.data(), &ctx_),
              "cvhip_ctx_create");
        // complete() always lands in host memory: the last level goes out in row bands, each crossing PCIe under the
        // search of the next (same grid)
        check(cvhip_ctx_set_result_bands(ctx_, 0), "cvhip_ctx_set_result_bands"); // (0: the library's choice by size)
    }
    ~PointCorrelations() { cvhip_ctx_destroy(ctx_); }
    PointCorrelations(const PointCorrelations &) = delete;
    PointCorrelations &operator=(const PointCorrelations &) = delete;

    const std::string &get_selected_hardware() const { return selected_hardware_; }
    cvhip_ctx *handle() const { return ctx_; } // (for the entries that read the device-resident grid: mesh::TrackTable::extend)

    // correlate_images (mod.rs:217-245): forward, reverse, cross-check x2, first_pass = false
    void correlate_images(const Grid<uint8_t> &img1, const Grid<uint8_t> &img2, float scale)
    {
        check(cvhip_correlate_level(ctx_, img1.data(), (uint32_t)img1.width(), (uint32_t)img1.height(), img2.data(),
                                    (uint32_t)img2.width(), (uint32_t)img2.height(), scale, first_pass_ ? 1 : 0,
                                    nullptr, nullptr),
              "cvhip_correlate_level");
        first_pass_ = false;
    }

    // complete (mod.rs:208-215): pulls the forward grid into `correlated_points`
    void complete()
    {
        const size_t w = dims1_.first, h = dims1_.second;
        std::vector<uint32_t> cells(w * h); // y2 << 16 | x2, all ones = None: 8 bytes per cell over PCIe with the score
        std::vector<float> corr(w * h);
        check(cvhip_complete_packed(ctx_, 0, cells.data(), corr.data()), "cvhip_complete_packed");
        correlated_points = Grid<std::optional<Match>>(w, h, std::nullopt);
        for (size_t i = 0; i < w * h; i++)
            if (cells[i] != 0xFFFFFFFFu) correlated_points.data()[i] = Match{{cells[i] & 0xFFFFu, cells[i] >> 16}, corr[i]};
    }

    static size_t optimal_scale_steps(std::pair<uint32_t, uint32_t> dimensions) // mod.rs:542-550
    {
        const size_t min_dimension = std::min(dimensions.first, dimensions.second);
        if (min_dimension <= 64) return 0;
        return (size_t)std::floor(std::log2((double)min_dimension / 64.0));
    }

  private:
    cvhip_ctx *ctx_ = nullptr;
    std::pair<uint32_t, uint32_t> dims1_;
    bool first_pass_ = true;
    std::string selected_hardware_;
};

// The dense stage of ImageReconstruction::correlate_dense (reconstruction.rs:554-588) over prebuilt
// pyramids: pyr[k] is the 1/2^k image; levels run coarse to fine.
inline Grid<std::optional<Match>> correlate_dense(GpuDevice &dev, const std::vector<Grid<uint8_t>> &pyr1,
                                                  const std::vector<Grid<uint8_t>> &pyr2,
                                                  const std::array<double, 9> &f, ProjectionMode mode)
{
    PointCorrelations pc(dev, {(uint32_t)pyr1[0].width(), (uint32_t)pyr1[0].height()},
                         {(uint32_t)pyr2[0].width(), (uint32_t)pyr2[0].height()}, f, mode);
    const size_t steps = pyr1.size() - 1;
    for (size_t i = 0; i <= steps; i++) {
        const size_t k = steps - i;
        pc.correlate_images(pyr1[k], pyr2[k], 1.0f / (float)(1u << k));
    }
    pc.complete();
    return std::move(pc.correlated_points);
}

namespace orb {
using Keypoint = std::pair<Point2D<size_t>, std::array<uint32_t, 8>>; // orb.rs:9
constexpr uint32_t MAX_KEYPOINTS = 10000;                            // orb.rs:41

// orb.rs:43-48: `Option<&PL>` becomes a nullable pointer; report_status is called on the calling thread
struct ProgressListener {
    virtual void report_status(float pos) const = 0;
    virtual ~ProgressListener() = default;
};
inline std::vector<Keypoint> extract_points(GpuDevice &dev, const Grid<uint8_t> &img,
                                            const ProgressListener *progress_listener = nullptr) // orb.rs:50-84
{
    std::vector<uint32_t> xy(2 * MAX_KEYPOINTS), desc(8 * MAX_KEYPOINTS);
    uint32_t n = 0;
    const auto thunk = [](void *user, float pos) { static_cast<const ProgressListener *>(user)->report_status(pos); };
    check(cvhip_orb_extract(dev.handle(), img.data(), (uint32_t)img.width(), (uint32_t)img.height(), MAX_KEYPOINTS,
                            xy.data(), desc.data(), &n, progress_listener ? +thunk : nullptr,
                            const_cast<ProgressListener *>(progress_listener)),
          "cvhip_orb_extract");
    std::vector<Keypoint> out(n);
    for (uint32_t i = 0; i < n; i++) {
        out[i].first = {xy[2 * i], xy[2 * i + 1]};
        std::copy_n(&desc[8 * i], 8, out[i].second.begin());
    }
    return out;
}
inline size_t optimal_scale_steps(std::pair<uint32_t, uint32_t> dimensions) // orb.rs:407-415
{
    const size_t min_dimension = std::min(dimensions.first, dimensions.second);
    if (min_dimension <= 256) return 0;
    return (size_t)std::floor(std::log2((double)min_dimension / 256.0));
}
} // namespace orb

using PointMatch = std::pair<Point2D<size_t>, Point2D<size_t>>; // fundamentalmatrix.rs:33, pointmatching.rs

struct KeypointMatching { // pointmatching.rs:17-77
    std::vector<PointMatch> matches;
    KeypointMatching(GpuDevice &dev, const std::vector<orb::Keypoint> &points1,
                     const std::vector<orb::Keypoint> &points2, ProjectionMode mode)
    {
        const uint32_t threshold = mode == ProjectionMode::Affine ? 32 : 48; // pointmatching.rs:8-9
        auto flatten = [](const std::vector<orb::Keypoint> &kp, std::vector<uint32_t> &xy, std::vector<uint32_t> &d) {
            xy.resize(2 * kp.size());
            d.resize(8 * kp.size());
            for (size_t i = 0; i < kp.size(); i++) {
                xy[2 * i] = (uint32_t)kp[i].first.x;
                xy[2 * i + 1] = (uint32_t)kp[i].first.y;
                std::copy(kp[i].second.begin(), kp[i].second.end(), &d[8 * i]);
            }
        };
        std::vector<uint32_t> xy1, d1, xy2, d2;
        flatten(points1, xy1, d1);
        flatten(points2, xy2, d2);
        std::vector<uint32_t> out(4 * std::max<size_t>(points1.size(), 1));
        uint32_t n = 0;
        check(cvhip_match_points(dev.handle(), xy1.data(), d1.data(), (uint32_t)points1.size(), xy2.data(), d2.data(),
                                 (uint32_t)points2.size(), threshold, out.data(), nullptr, &n),
              "cvhip_match_points");
        matches.resize(n);
        for (uint32_t i = 0; i < n; i++)
            matches[i] = {{out[4 * i], out[4 * i + 1]}, {out[4 * i + 2], out[4 * i + 3]}};
    }
};

struct RansacError : std::runtime_error { // fundamentalmatrix.rs:665-682
    using std::runtime_error::runtime_error;
};

struct FundamentalMatrixResult { // fundamentalmatrix.rs:57-61
    std::array<double, 9> f;     // row-major
    std::vector<PointMatch> inliers;
};

// FundamentalMatrix (fundamentalmatrix.rs:63-257) for the affine model.  Sampling and the 4-point fit
// run on the host exactly as in the reference (rejection sampling from the top 5000 matches, >= 10 px
// apart; mean-centred 4x4 smallest right-singular vector); all hypotheses of one check interval are
// scored on the GPU in one call.  The perspective model (7-point, fundamentalmatrix.rs:289-389) runs
// entirely on the device (cvhip_ransac_perspective); its final LM refit (:391-426, 515-621) is
// cvhip_optimize_perspective_f.
class FundamentalMatrix {
  public:
    FundamentalMatrix(ProjectionMode projection, double max_dimension) : projection_(projection), max_dimension_(max_dimension)
    {
        // fundamentalmatrix.rs:16-30, 72-101
        ransac_k_ = 1000000;
        if (projection == ProjectionMode::Affine) {
            ransac_n_ = 4;
            ransac_t_ = 0.1;
            ransac_d_ = 10;
            ransac_d_early_exit_ = 1000;
        } else {
            ransac_n_ = 7;
            ransac_t_ = 10.0 / 1000.0 * max_dimension;
            ransac_d_ = 200;
            ransac_d_early_exit_ = 50000;
        }
    }

    FundamentalMatrixResult find_ransac(GpuDevice &dev, const std::vector<PointMatch> &point_matches,
                                        uint64_t seed = std::random_device{}()) const
    {
        if (point_matches.size() < ransac_d_ + ransac_n_) throw RansacError("Not enough matches");
        std::vector<uint32_t> flat(4 * point_matches.size());
        for (size_t i = 0; i < point_matches.size(); i++) {
            flat[4 * i] = (uint32_t)point_matches[i].first.x;
            flat[4 * i + 1] = (uint32_t)point_matches[i].first.y;
            flat[4 * i + 2] = (uint32_t)point_matches[i].second.x;
            flat[4 * i + 3] = (uint32_t)point_matches[i].second.y;
        }
        if (projection_ != ProjectionMode::Affine) {
            // Perspective: sampling, the 7-point model and its checks, scoring and best-pick all run on the device
            // (cvhip_ransac_perspective); optimize_result (:231-257) then refits the winner on its inliers with the
            // reference's own LM loop (cvhip_optimize_perspective_f, host arithmetic) and re-selects the inliers.
            FundamentalMatrixResult res;
            std::vector<uint8_t> mask(point_matches.size());
            uint32_t cnt = 0;
            const int rc = cvhip_ransac_perspective(dev.handle(), flat.data(), (uint32_t)point_matches.size(), max_dimension_,
                                                    seed, 0, res.f.data(), &cnt, mask.data());
            if (rc == CVHIP_ERR_NO_MODEL) throw RansacError(cvhip_last_error());
            check(rc, "cvhip_ransac_perspective");
            std::vector<uint32_t> inl;
            inl.reserve(4 * (size_t)cnt);
            for (size_t i = 0; i < point_matches.size(); i++)
                if (mask[i]) inl.insert(inl.end(), flat.begin() + 4 * i, flat.begin() + 4 * i + 4);
            std::array<double, 9> refit{};
            int refined = 0;
            check(cvhip_optimize_perspective_f(res.f.data(), inl.data(), (uint32_t)(inl.size() / 4), refit.data(), &refined),
                  "cvhip_optimize_perspective_f");
            res.f = refit; // .unwrap_or(res.f): the call returns F itself when the refit is rejected
            for (size_t i = 0; i < point_matches.size(); i++)
                if (fits(res.f, point_matches[i])) res.inliers.push_back(point_matches[i]); // :248-254
            return res;
        }
        std::mt19937_64 rng(seed); // the reference seeds SmallRng from the OS: runs are not reproducible there
        const size_t check_interval = 50000, outer = ransac_k_ / check_interval;
        bool have = false;
        Best best{};
        std::vector<double> fs;
        std::vector<uint32_t> counts;
        std::vector<double> errs;
        for (size_t round = 0; round < outer; round++) {
            fs.clear();
            for (size_t it = 0; it < check_interval; it++) { // ransac_iteration, :177-190
                std::array<PointMatch, 4> sample;
                choose_inliers(point_matches, rng, sample);
                std::array<double, 9> f;
                if (!calculate_model_affine(sample, f)) continue;
                bool finite = true, sample_fits = true;
                for (double v : f) finite = finite && std::isfinite(v);
                if (!finite) continue; // validate_f, :197-199
                for (const auto &m : sample) sample_fits = sample_fits && fits(f, m); // :206-209
                if (!sample_fits) continue;
                fs.insert(fs.end(), f.begin(), f.end());
            }
            const uint32_t H = (uint32_t)(fs.size() / 9);
            counts.assign(H, 0);
            errs.assign(H, 0.0);
            check(cvhip_ransac_score(dev.handle(), fs.data(), H, flat.data(), (uint32_t)point_matches.size(), ransac_t_,
                                     counts.data(), errs.data()),
                  "cvhip_ransac_score");
            for (uint32_t h = 0; h < H; h++) {
                if (counts[h] < ransac_d_ + ransac_n_) continue; // :218-220
                Best cand;
                std::copy_n(&fs[9 * (size_t)h], 9, cand.f.begin());
                cand.matches_count = counts[h];
                cand.best_error = errs[h] / (double)counts[h];
                if (!have || better(cand, best)) {
                    best = cand;
                    have = true;
                }
            }
            if (have && best.matches_count > ransac_d_early_exit_) break; // :135-141
        }
        if (!have) throw RansacError("No reliable matches found");
        FundamentalMatrixResult res; // optimize_result, affine branch (:231-239)
        res.f = best.f;
        for (const auto &m : point_matches)
            if (fits(best.f, m)) res.inliers.push_back(m);
        return res;
    }

    // reprojection_error (fundamentalmatrix.rs:461-471), nalgebra evaluation order
    static double reprojection_error(const std::array<double, 9> &F, const PointMatch &m)
    {
        const double p1x = (double)m.first.x, p1y = (double)m.first.y, p2x = (double)m.second.x, p2y = (double)m.second.y;
        const double r0 = (p2x * F[0] + p2y * F[3]) + F[6], r1 = (p2x * F[1] + p2y * F[4]) + F[7],
                     r2 = (p2x * F[2] + p2y * F[5]) + F[8];
        double n = r0 * p1x;
        n = r1 * p1y + n;
        n = r2 + n;
        double a0 = F[0] * p1x;
        a0 = F[1] * p1y + a0;
        a0 = F[2] + a0;
        double a1 = F[3] * p1x;
        a1 = F[4] * p1y + a1;
        a1 = F[5] + a1;
        const double b0 = (F[0] * p2x + F[3] * p2y) + F[6], b1 = (F[1] * p2x + F[4] * p2y) + F[7];
        return (n * n) / (a0 * a0 + a1 * a1 + b0 * b0 + b1 * b1);
    }

  private:
    struct Best {
        std::array<double, 9> f;
        size_t matches_count;
        double best_error;
    };
    // Ord for RansacIterationResult (fundamentalmatrix.rs:623-649): more matches, then finite and lower error
    static bool better(const Best &a, const Best &b)
    {
        if (a.matches_count != b.matches_count) return a.matches_count > b.matches_count;
        const bool af = std::isfinite(a.best_error), bf = std::isfinite(b.best_error);
        if (af != bf) return af;
        if (!af) return false;
        return a.best_error < b.best_error;
    }
    bool fits(const std::array<double, 9> &f, const PointMatch &m) const // fits_model, :452-458
    {
        const double err = reprojection_error(f, m);
        return std::isfinite(err) && !(std::fabs(err) > ransac_t_);
    }
    static size_t dist(size_t x, size_t y) { return x > y ? x - y : y - x; }
    template <typename Rng>
    static void choose_inliers(const std::vector<PointMatch> &pm, Rng &rng, std::array<PointMatch, 4> &out) // :155-175
    {
        const size_t limit = std::min<size_t>(pm.size(), 5000);
        std::uniform_int_distribution<size_t> pick(0, limit - 1);
        size_t have = 0;
        while (have < 4) {
            const PointMatch &next = pm[pick(rng)];
            bool close = false;
            for (size_t i = 0; i < have; i++) {
                const PointMatch &c = out[i];
                close = close || dist(next.first.x, c.first.x) < 10 || dist(next.first.y, c.first.y) < 10 ||
                        dist(next.second.x, c.second.x) < 10 || dist(next.second.y, c.second.y) < 10;
            }
            if (!close) out[have++] = next;
        }
    }
    // calculate_model_affine (fundamentalmatrix.rs:260-286): rows (x2, y2, x1, y1), mean-centred; the
    // right-singular vector of the smallest singular value via Jacobi eigen-decomposition of A^T A.
    static bool calculate_model_affine(const std::array<PointMatch, 4> &s, std::array<double, 9> &f)
    {
        double a[4][4], mean[4] = {0, 0, 0, 0};
        for (int i = 0; i < 4; i++) {
            a[i][0] = (double)s[i].second.x;
            a[i][1] = (double)s[i].second.y;
            a[i][2] = (double)s[i].first.x;
            a[i][3] = (double)s[i].first.y;
            for (int j = 0; j < 4; j++) mean[j] += a[i][j] / 4.0;
        }
        for (int i = 0; i < 4; i++)
            for (int j = 0; j < 4; j++) a[i][j] -= mean[j];
        double m[4][4], v[4][4];
        for (int i = 0; i < 4; i++)
            for (int j = 0; j < 4; j++) {
                m[i][j] = 0;
                for (int k = 0; k < 4; k++) m[i][j] += a[k][i] * a[k][j];
                v[i][j] = i == j ? 1.0 : 0.0;
            }
        for (int sweep = 0; sweep < 60; sweep++) { // cyclic Jacobi
            double off = 0;
            for (int p = 0; p < 4; p++)
                for (int q = p + 1; q < 4; q++) off += m[p][q] * m[p][q];
            if (off < 1e-300) break;
            for (int p = 0; p < 4; p++)
                for (int q = p + 1; q < 4; q++) {
                    if (std::fabs(m[p][q]) < 1e-300) continue;
                    const double theta = (m[q][q] - m[p][p]) / (2.0 * m[p][q]);
                    const double t = (theta >= 0 ? 1.0 : -1.0) / (std::fabs(theta) + std::sqrt(theta * theta + 1.0));
                    const double c = 1.0 / std::sqrt(t * t + 1.0), sn = t * c;
                    for (int k = 0; k < 4; k++) {
                        const double mkp = m[k][p], mkq = m[k][q];
                        m[k][p] = c * mkp - sn * mkq;
                        m[k][q] = sn * mkp + c * mkq;
                    }
                    for (int k = 0; k < 4; k++) {
                        const double mpk = m[p][k], mqk = m[q][k];
                        m[p][k] = c * mpk - sn * mqk;
                        m[q][k] = sn * mpk + c * mqk;
                    }
                    for (int k = 0; k < 4; k++) {
                        const double vkp = v[k][p], vkq = v[k][q];
                        v[k][p] = c * vkp - sn * vkq;
                        v[k][q] = sn * vkp + c * vkq;
                    }
                }
        }
        int order[4] = {0, 1, 2, 3};
        std::sort(order, order + 4, [&](int x, int y) { return m[x][x] > m[y][y]; });
        // singular values = sqrt(eigenvalues); reject rank-deficient samples: s[1] < 1e-3 (:272-275)
        if (std::sqrt(std::max(m[order[1]][order[1]], 0.0)) < 0.001) return false;
        const int last = order[3];
        const double vt[4] = {v[0][last], v[1][last], v[2][last], v[3][last]};
        const double e = vt[0] * mean[0] + vt[1] * mean[1] + vt[2] * mean[2] + vt[3] * mean[3];
        const double raw[9] = {0, 0, vt[0], 0, 0, vt[1], vt[2], vt[3], -e};
        for (int i = 0; i < 9; i++) f[i] = raw[i] / raw[8];
        return true;
    }

    ProjectionMode projection_;
    double max_dimension_;
    size_t ransac_k_, ransac_n_, ransac_d_, ransac_d_early_exit_;
    double ransac_t_;
};

// ---- the mesh stage of output::output (src/output.rs:567-611) ------------------------------------------------
namespace mesh {

struct Surface { // triangulation::Surface (triangulation.rs:142-150) as the cvhip_mesh_* entries take it
    std::vector<double> points;       // n x 3
    std::vector<int32_t> tracks;      // n x m x 2, (-1, -1) = None
    std::vector<double> projection;   // m x 12
    std::vector<double> r, t;         // m x 3 each
    std::vector<uint32_t> image_dims; // m x 2: width, height
    uint64_t tracks_len() const { return points.size() / 3; }
    uint32_t cameras_len() const { return (uint32_t)(projection.size() / 12); }
};

// max_points (triangulation.rs:837-843) on the device -> the surface of the max_points rows of `s` with the
// smallest keys of `seed` (the binding passes rand::random()), in ascending row order; every row when max_points >= the
// surface's length.  Cameras and image dimensions are carried over.  rows (optional): the kept rows, for the caller's own
// per-track data.
inline Surface surface_subset(GpuDevice &dev, const Surface &s, uint64_t max_points, uint64_t seed, std::vector<uint64_t> *rows = nullptr)
{
    const uint64_t n = s.tracks_len(), k = n < max_points ? n : max_points;
    Surface out = s;
    out.points.assign(3 * k, 0.0);
    out.tracks.assign(2 * k * s.cameras_len(), 0);
    std::vector<uint64_t> kept(k);
    uint64_t out_n = 0;
    check(cvhip_surface_subset(dev.handle(), n, max_points, seed, s.points.data(), s.tracks.data(), s.cameras_len(), kept.data(),
                               out.points.data(), out.tracks.data(), &out_n),
          "cvhip_surface_subset");
    if (rows) *rows = std::move(kept);
    return out;
}

// The dense track table in device memory (cvhip_tracks): n x m x 2 int32, (-1, -1) = None - what
// PerspectiveTriangulation keeps in `tracks` (triangulation.rs:604-617), owned by the library, so that extend_tracks, merge_tracks
// and the survivors' rows never cross to the host.  It belongs to the GpuDevice it was made with and is destroyed before it.
// device_rows() is valid until the next call that changes the table (assign, extend, merge); a call that throws leaves the
// table as it was.
class TrackTable {
  public:
    struct ExtendCounts {
        uint64_t matched, filled, appended;
    };
    struct MergeStats { // cvhip_merge_tracks' out_stats
        uint64_t present, cells, rejected, empty_area;
    };
    TrackTable(GpuDevice &dev, uint32_t m, uint64_t reserve_rows = 0) { check(cvhip_tracks_create(dev.handle(), m, reserve_rows, &t_), "cvhip_tracks_create"); }
    ~TrackTable() { cvhip_tracks_destroy(t_); }
    TrackTable(const TrackTable &) = delete;
    TrackTable &operator=(const TrackTable &) = delete;
    TrackTable(TrackTable &&o) noexcept : t_(o.t_) { o.t_ = nullptr; }
    cvhip_tracks *handle() const { return t_; }
    uint64_t rows() const { return info().rows; }
    uint64_t capacity() const { return info().capacity; }
    uint32_t m() const { return info().m; }
    const int32_t *device_rows() const { return info().device_rows; }
    void assign(const std::vector<int32_t> &rows) { check(cvhip_tracks_assign(t_, rows.data(), rows.size() / (2 * (size_t)m())), "cvhip_tracks_assign"); }
    // rows [first, first + n) on the host (n = UINT64_MAX: to the last row)
    std::vector<int32_t> read(uint64_t first = 0, uint64_t n = UINT64_MAX) const
    {
        const Info i = info();
        if (n == UINT64_MAX) n = i.rows > first ? i.rows - first : 0;
        std::vector<int32_t> out((size_t)n * i.m * 2);
        check(cvhip_tracks_read(t_, first, n, out.data()), "cvhip_tracks_read");
        return out;
    }
    // extend_tracks (triangulation.rs:1330-1419) with the device-resident grid of `pc`, fill rule and append included
    ExtendCounts extend(PointCorrelations &pc, uint32_t image1, uint32_t image2, uint32_t max_dimension2)
    {
        uint64_t c[3] = {0, 0, 0};
        check(cvhip_tracks_extend(t_, pc.handle(), image1, image2, max_dimension2, c), "cvhip_tracks_extend");
        return {c[0], c[1], c[2]};
    }
    MergeStats merge(uint32_t image_index, uint32_t width, uint32_t height) // merge_tracks (:1421-1540)
    {
        uint64_t s[4] = {0, 0, 0, 0};
        check(cvhip_tracks_merge(t_, image_index, width, height, s), "cvhip_tracks_merge");
        return {s[0], s[1], s[2], s[3]};
    }
    TrackTable select_columns(const std::vector<uint32_t> &columns) const // prune_projections (:913-938)
    {
        cvhip_tracks *out = nullptr;
        check(cvhip_tracks_select_columns(t_, columns.data(), (uint32_t)columns.size(), &out), "cvhip_tracks_select_columns");
        return TrackTable(out);
    }
    std::vector<int32_t> gather(const std::vector<uint64_t> &rows) const // out[j] = row rows[j]
    {
        std::vector<int32_t> out(rows.size() * (size_t)m() * 2);
        check(cvhip_tracks_gather(t_, rows.data(), rows.size(), out.data()), "cvhip_tracks_gather");
        return out;
    }

  private:
    struct Info {
        uint64_t rows = 0, capacity = 0;
        uint32_t m = 0;
        const int32_t *device_rows = nullptr;
    };
    explicit TrackTable(cvhip_tracks *t) : t_(t) {}
    Info info() const
    {
        Info i;
        check(cvhip_tracks_info(t_, &i.rows, &i.capacity, &i.m, &i.device_rows), "cvhip_tracks_info");
        return i;
    }
    cvhip_tracks *t_ = nullptr;
};

struct Polygon { // output.rs:49-53
    uint32_t camera_i;
    std::array<uint32_t, 3> vertices;
};

struct CameraPoints { // Mesh::process_camera's Delaunay input (:401-423), in track order
    std::vector<uint32_t> track_i;
    std::vector<double> xy; // 2 per point
};

inline CameraPoints camera_points(GpuDevice &dev, const Surface &s, uint32_t camera_i)
{
    uint64_t n = 0;
    check(cvhip_mesh_camera_points(dev.handle(), s.points.data(), s.tracks.data(), s.tracks_len(), s.cameras_len(), s.projection.data(),
                                   s.r.data(), s.t.data(), s.image_dims.data(), camera_i, nullptr, nullptr, 0, &n),
          "cvhip_mesh_camera_points");
    CameraPoints out;
    out.track_i.resize(n);
    out.xy.resize(2 * n);
    if (n)
        check(cvhip_mesh_camera_points(dev.handle(), s.points.data(), s.tracks.data(), s.tracks_len(), s.cameras_len(),
                                       s.projection.data(), s.r.data(), s.t.data(), s.image_dims.data(), camera_i, out.track_i.data(),
                                       out.xy.data(), n, &n),
              "cvhip_mesh_camera_points");
    return out;
}

struct DelaunayStats { // CVHIP_DELAUNAY_STAT_*
    uint64_t grid_width = 0, grid_height = 0, device_stars = 0, host_stars = 0, duplicates = 0, most_cells = 0;
};

// DelaunayTriangulation::bulk_load of a camera's points (:425) on the device -> the faces, 3 indices into the
// points each, counter-clockwise, the smallest first (cvhip.h has the definition); a `triangulate` for Mesh::create:
//   Mesh::create(dev, s, [&](const CameraPoints &cp) { return mesh::delaunay(dev, cp); })
inline std::vector<uint32_t> delaunay(GpuDevice &dev, const std::vector<double> &xy, DelaunayStats *stats = nullptr)
{
    const uint64_t k = xy.size() / 2;
    std::vector<uint32_t> faces(6 * k); // (2 k faces are always enough)
    uint64_t n = 0, st[CVHIP_DELAUNAY_STATS] = {0};
    check(cvhip_mesh_delaunay(dev.handle(), xy.data(), k, faces.data(), 2 * k, &n, st), "cvhip_mesh_delaunay");
    faces.resize(3 * n);
    if (stats) *stats = DelaunayStats{st[0], st[1], st[2], st[3], st[4], st[5]};
    return faces;
}
inline std::vector<uint32_t> delaunay(GpuDevice &dev, const CameraPoints &cp, DelaunayStats *stats = nullptr) { return delaunay(dev, cp.xy, stats); }

inline void set_delaunay_lane_cells(GpuDevice &dev, uint32_t cells)
{
    check(cvhip_mesh_delaunay_set_lane_cells(dev.handle(), cells), "cvhip_mesh_delaunay_set_lane_cells");
}

// integer coordinates within 2^24 (an affine surface's camera points): exact integer predicates on the device (off by default)
inline void set_delaunay_lattice(GpuDevice &dev, bool on)
{
    check(cvhip_mesh_delaunay_set_lattice(dev.handle(), on ? 1 : 0), "cvhip_mesh_delaunay_set_lattice");
}
inline bool delaunay_lattice(GpuDevice &dev)
{
    int on = 0;
    check(cvhip_mesh_delaunay_get_lattice(dev.handle(), &on), "cvhip_mesh_delaunay_get_lattice");
    return on != 0;
}
// the stars of the last mesh::delaunay call that the lattice kernels finished (0: the call did not qualify)
inline uint64_t delaunay_lattice_stars(GpuDevice &dev)
{
    uint64_t n = 0;
    check(cvhip_mesh_delaunay_get_lattice_stars(dev.handle(), &n), "cvhip_mesh_delaunay_get_lattice_stars");
    return n;
}

// the culling loop of process_camera (:457-508): keep[p] = 0 iff polygon p obstructs in another camera
inline std::vector<uint8_t> cull(GpuDevice &dev, const Surface &s, uint32_t camera_i, const std::vector<uint32_t> &polygons)
{
    std::vector<uint8_t> keep(polygons.size() / 3);
    check(cvhip_mesh_cull(dev.handle(), s.points.data(), s.tracks.data(), s.tracks_len(), s.cameras_len(), s.projection.data(),
                          s.r.data(), s.t.data(), s.image_dims.data(), camera_i, polygons.data(), keep.size(), keep.data(), nullptr),
          "cvhip_mesh_cull");
    return keep;
}

class Mesh { // output.rs:356-387
  public:
    std::vector<Polygon> polygons;

    // Mesh::create: `triangulate(xy) -> faces` (3 indices into the camera's points each) is the caller's Delaunay
    // (mesh::delaunay is one, on the device)
    template <typename Triangulate> static Mesh create(GpuDevice &dev, const Surface &s, Triangulate triangulate)
    {
        std::vector<uint32_t> kept, cams;
        for (uint32_t i = 0; i < s.cameras_len(); i++) {
            const CameraPoints cp = camera_points(dev, s, i);
            const std::vector<uint32_t> faces = triangulate(cp);
            std::vector<uint32_t> polys(faces.size());
            for (size_t k = 0; k < faces.size(); k++) polys[k] = cp.track_i.at(faces[k]);
            const std::vector<uint8_t> keep = cull(dev, s, i, polys);
            for (size_t p = 0; p < keep.size(); p++)
                if (keep[p]) {
                    kept.insert(kept.end(), polys.begin() + 3 * p, polys.begin() + 3 * p + 3);
                    cams.push_back(i);
                }
        }
        std::vector<uint32_t> out_p(kept.size()), out_c(cams.size());
        uint64_t n = 0;
        check(cvhip_mesh_merge(dev.handle(), kept.data(), cams.data(), cams.size(), out_p.data(), out_c.data(), &n), "cvhip_mesh_merge");
        Mesh mesh;
        for (uint64_t p = 0; p < n; p++) mesh.polygons.push_back(Polygon{out_c[p], {out_p[3 * p], out_p[3 * p + 1], out_p[3 * p + 2]}});
        return mesh;
    }
};

struct DepthImage { // ImageWriter's output_map (:1009-1013) with its origin and depth range
    Grid<double> map; // NaN = None
    double min_x = 0, min_y = 0, min_depth = 0, max_depth = 0;
};

inline DepthImage depth_image(GpuDevice &dev, const Surface &s, uint32_t project_to_image, double scale, const std::vector<Polygon> &polygons)
{
    std::vector<uint32_t> flat;
    for (const Polygon &p : polygons) flat.insert(flat.end(), p.vertices.begin(), p.vertices.end());
    uint64_t w = 0, h = 0;
    double origin[2] = {0, 0}, minmax[2] = {0, 0};
    check(cvhip_mesh_depth_image(dev.handle(), s.points.data(), s.tracks.data(), s.tracks_len(), s.cameras_len(), s.projection.data(),
                                 s.r.data(), s.t.data(), s.image_dims.data(), project_to_image, scale, flat.data(), polygons.size(),
                                 nullptr, 0, &w, &h, origin, nullptr, nullptr),
          "cvhip_mesh_depth_image");
    DepthImage out;
    out.map = Grid<double>(w, h, 0.0);
    check(cvhip_mesh_depth_image(dev.handle(), s.points.data(), s.tracks.data(), s.tracks_len(), s.cameras_len(), s.projection.data(),
                                 s.r.data(), s.t.data(), s.image_dims.data(), project_to_image, scale, flat.data(), polygons.size(),
                                 out.map.data(), w * h, &w, &h, origin, minmax, nullptr),
          "cvhip_mesh_depth_image");
    out.min_x = origin[0], out.min_y = origin[1], out.min_depth = minmax[0], out.max_depth = minmax[1];
    return out;
}

// ---- the mesh output: PlyWriter's file image (:648-772) and ImageWriter::complete's colours (:1117-1229) ------
enum class VertexMode : uint32_t { Plain = CVHIP_VERTEX_PLAIN, Color = CVHIP_VERTEX_COLOR, Texture = CVHIP_VERTEX_TEXTURE };

struct RgbImage { // image::RgbImage: row-major, 3 bytes per pixel
    uint32_t width = 0, height = 0;
    std::vector<uint8_t> pixels;
};

struct PlySections {
    uint64_t header = 0, vertices = 0, faces = 0;
};

namespace detail {
// the arrays of cvhip_mesh_ply and cvhip_mesh_obj: the polygons and their cameras, flattened, and the images, concatenated
struct WriterArrays {
    std::vector<uint32_t> polygons, cameras, dims;
    std::vector<uint8_t> pixels;
    std::vector<uint64_t> offsets{0};
    uint64_t n = 0;
    uint32_t m = 0;    // images per track (an affine surface has no cameras: the number of images then)
    bool with_dims = false; // one image per image of a track
};
inline WriterArrays writer_arrays(const Surface &s, const std::vector<Polygon> &polygons, const std::vector<RgbImage> &images, bool with_pixels)
{
    WriterArrays a;
    for (const Polygon &p : polygons) a.polygons.insert(a.polygons.end(), p.vertices.begin(), p.vertices.end()), a.cameras.push_back(p.camera_i);
    a.n = s.tracks_len();
    a.m = a.n ? (uint32_t)(s.tracks.size() / (2 * a.n)) : (uint32_t)images.size();
    for (const RgbImage &im : images) {
        if (with_pixels) a.pixels.insert(a.pixels.end(), im.pixels.begin(), im.pixels.end());
        a.offsets.push_back(a.pixels.size());
        a.dims.push_back(im.width), a.dims.push_back(im.height);
    }
    a.with_dims = images.size() == a.m && a.m > 0;
    return a;
}
// call(out, cap, &size) twice: for the size, then into a vector of that size
template <typename Call> inline std::vector<uint8_t> size_then_fill(Call &&call)
{
    uint64_t size = 0;
    call(nullptr, 0, &size);
    std::vector<uint8_t> out(size);
    call(out.data(), size, &size);
    return out;
}
} // namespace detail

// Mesh::output with a PlyWriter -> the file's bytes.  images: one per image of a track, read in Color mode only; the surface
// may be affine (no cameras): `m` is then the number of images.
inline std::vector<uint8_t> ply(GpuDevice &dev, const Surface &s, const std::vector<Polygon> &polygons, const std::vector<RgbImage> &images,
                                VertexMode mode, const std::array<double, 3> &out_scale, PlySections *sections = nullptr)
{
    const detail::WriterArrays a = detail::writer_arrays(s, polygons, images, true);
    const bool with_images = mode == VertexMode::Color && a.with_dims;
    uint64_t sec[3] = {0, 0, 0};
    std::vector<uint8_t> out = detail::size_then_fill([&](uint8_t *dst, uint64_t cap, uint64_t *size) {
        check(cvhip_mesh_ply(dev.handle(), s.points.data(), s.tracks.data(), a.n, a.m, with_images ? a.pixels.data() : nullptr,
                             with_images ? a.offsets.data() : nullptr, with_images ? a.dims.data() : nullptr, (uint32_t)mode, out_scale.data(),
                             a.polygons.data(), polygons.size(), dst, cap, size, sec),
              "cvhip_mesh_ply");
    });
    if (sections) *sections = PlySections{sec[0], sec[1], sec[2]};
    return out;
}

// ---- the OBJ writer: ObjWriter's file image (:774-1007) and its .mtl text ------------------------------------------
struct ObjSections {
    uint64_t header = 0, v = 0, vt = 0, f = 0;
};

// Mesh::output with an ObjWriter -> the file's bytes.  images: one per image of a track - their pixels are read in Color mode,
// only their sizes in Texture mode (pixels may be empty there); each polygon's camera_i is read in Texture mode; stem: the
// output path's file stem.  The {stem}-{i}.png images the .mtl names: png_encode of each image.
inline std::vector<uint8_t> mesh_obj(GpuDevice &dev, const Surface &s, const std::vector<Polygon> &polygons, const std::vector<RgbImage> &images,
                                     VertexMode mode, const std::array<double, 3> &out_scale, const std::string &stem,
                                     ObjSections *sections = nullptr)
{
    const detail::WriterArrays a = detail::writer_arrays(s, polygons, images, mode == VertexMode::Color);
    const bool with_dims = mode != VertexMode::Plain && a.with_dims, with_images = with_dims && mode == VertexMode::Color;
    uint64_t sec[4] = {0, 0, 0, 0};
    std::vector<uint8_t> out = detail::size_then_fill([&](uint8_t *dst, uint64_t cap, uint64_t *size) {
        check(cvhip_mesh_obj(dev.handle(), s.points.data(), s.tracks.data(), a.n, a.m, with_images ? a.pixels.data() : nullptr,
                             with_images ? a.offsets.data() : nullptr, with_dims ? a.dims.data() : nullptr, (uint32_t)mode, out_scale.data(),
                             a.polygons.data(), a.cameras.data(), polygons.size(), stem.c_str(), dst, cap, size, sec),
              "cvhip_mesh_obj");
    });
    if (sections) *sections = ObjSections{sec[0], sec[1], sec[2], sec[3]};
    return out;
}

// ObjWriter::write_materials' text (:856-868) for m images
inline std::string mesh_obj_mtl(const std::string &stem, uint32_t m)
{
    uint64_t size = 0;
    check(cvhip_mesh_obj_mtl(stem.c_str(), m, nullptr, 0, &size), "cvhip_mesh_obj_mtl");
    std::string out(size, '\0');
    check(cvhip_mesh_obj_mtl(stem.c_str(), m, out.data(), size, &size), "cvhip_mesh_obj_mtl");
    return out;
}

// ---- the PNG encoder: what img.save writes for the textures (:845-875) and the depth map (:1141) -----------------
struct PngSections {
    uint64_t before = 0, idat = 0, after = 0; // the bytes before the IDAT data, the IDAT data, the bytes after it
};
enum class PngFilter : uint32_t { None = 0, Sub = 1, Up = 2, Average = 3, Paeth = 4, Adaptive = 5 };

// The PNG file's bytes of width x height pixels of `channels` (1: grey, 2: grey and alpha, 3: RGB, 4: RGBA) bytes each.
inline std::vector<uint8_t> png_encode(GpuDevice &dev, const uint8_t *pixels, uint32_t width, uint32_t height, uint32_t channels,
                                       PngFilter filter = PngFilter::Adaptive, PngSections *sections = nullptr)
{
    uint64_t sec[3] = {0, 0, 0};
    std::vector<uint8_t> out = detail::size_then_fill([&](uint8_t *dst, uint64_t cap, uint64_t *size) {
        check(cvhip_png_encode(dev.handle(), pixels, width, height, channels, (uint32_t)filter, dst, cap, size, sec), "cvhip_png_encode");
    });
    if (sections) *sections = PngSections{sec[0], sec[1], sec[2]};
    return out;
}

// ---- the JPEG encoder: what img.save writes for a depth map whose path ends in .jpg (:1141) ---------------------
struct JpegSections {
    uint64_t before = 0, data = 0, after = 0; // the bytes before the scan's data, the data, the bytes after it
};
enum class JpegSampling : uint32_t { S444 = 0, S422 = 1, S420 = 2 };
struct JpegEncodeStats {
    uint64_t blocks = 0, dummy_blocks = 0, bits = 0, stuffed = 0;
};

// The baseline JPEG file's bytes, libjpeg's file, of width x height pixels of `channels` (1: grey, 2: grey and alpha, 3: RGB,
// 4: RGBA; alpha is dropped) bytes each.  The OBJ writer's textures stay PNG.
inline std::vector<uint8_t> jpeg_encode(GpuDevice &dev, const uint8_t *pixels, uint32_t width, uint32_t height, uint32_t channels,
                                        uint32_t quality = 75, JpegSampling sampling = JpegSampling::S420, bool optimize = false,
                                        JpegSections *sections = nullptr)
{
    uint64_t sec[3] = {0, 0, 0};
    std::vector<uint8_t> out = detail::size_then_fill([&](uint8_t *dst, uint64_t cap, uint64_t *size) {
        check(cvhip_jpeg_encode(dev.handle(), pixels, width, height, channels, quality, (uint32_t)sampling, optimize ? 1u : 0u, dst, cap, size, sec),
              "cvhip_jpeg_encode");
    });
    if (sections) *sections = JpegSections{sec[0], sec[1], sec[2]};
    return out;
}

// of this thread's last jpeg_encode
inline JpegEncodeStats jpeg_encode_last_stats()
{
    uint64_t st[4] = {0, 0, 0, 0};
    check(cvhip_jpeg_encode_last_stats(st), "cvhip_jpeg_encode_last_stats");
    return JpegEncodeStats{st[0], st[1], st[2], st[3]};
}

// ---- the TIFF encoder: what img.save writes for a depth map whose path ends in .tif (:1141) ---------------------
struct TiffSections {
    uint64_t before = 0, strips = 0, after = 0; // the bytes before the first strip, the strips with their padding, the bytes after
};
enum class TiffCompression : uint32_t { None = 1, Lzw = 5, PackBits = 32773 };
struct TiffEncodeStats {
    uint64_t strips = 0, codes = 0, clears = 0, packets = 0;
};

// The classic little-endian TIFF file's bytes of width x height pixels of `channels` (1: grey, 2: grey and alpha, 3: RGB, 4:
// RGBA) bytes each.  predictor 0: 2 with LZW, 1 otherwise.  rows_per_strip 0: about 8 KB a strip.
inline std::vector<uint8_t> tiff_encode(GpuDevice &dev, const uint8_t *pixels, uint32_t width, uint32_t height, uint32_t channels,
                                        TiffCompression compression = TiffCompression::Lzw, uint32_t predictor = 0, uint32_t rows_per_strip = 0,
                                        TiffSections *sections = nullptr)
{
    uint64_t sec[3] = {0, 0, 0};
    if (!predictor) predictor = compression == TiffCompression::Lzw ? 2u : 1u;
    std::vector<uint8_t> out = detail::size_then_fill([&](uint8_t *dst, uint64_t cap, uint64_t *size) {
        check(cvhip_tiff_encode(dev.handle(), pixels, width, height, channels, (uint32_t)compression, predictor, rows_per_strip, dst, cap, size, sec),
              "cvhip_tiff_encode");
    });
    if (sections) *sections = TiffSections{sec[0], sec[1], sec[2]};
    return out;
}

// of this thread's last tiff_encode
inline TiffEncodeStats tiff_encode_last_stats()
{
    uint64_t st[4] = {0, 0, 0, 0};
    check(cvhip_tiff_encode_last_stats(st), "cvhip_tiff_encode_last_stats");
    return TiffEncodeStats{st[0], st[1], st[2], st[3]};
}

// ImageWriter::complete: the depth map through `table` (256 x R, G, B) -> width x height x RGBA
inline std::vector<uint8_t> colour_map(GpuDevice &dev, const DepthImage &img, const std::array<uint8_t, 768> &table)
{
    std::vector<uint8_t> rgba(img.map.width() * img.map.height() * 4);
    check(cvhip_mesh_colour_map(dev.handle(), img.map.data(), img.map.width(), img.map.height(), img.min_depth, img.max_depth, table.data(),
                                rgba.data()),
          "cvhip_mesh_colour_map");
    return rgba;
}

} // namespace mesh

// ---- image files in: SourceImage::load / load_rgb (reconstruction.rs:40-60) for baseline JPEG, strip TIFF and PNG ---
namespace image {

struct JpegInfo {
    uint32_t width = 0, height = 0, components = 0, h = 0, v = 0; // h, v: the luma sampling factors
    uint32_t focal_length_35mm = 0;                               // EXIF FocalLengthIn35mmFilm (:138-142), 0 = none
};
enum class Format : uint32_t { Luma8 = CVHIP_IMAGE_LUMA8, Rgb8 = CVHIP_IMAGE_RGB8 };

// the frame and the EXIF focal length of a JPEG file's bytes (host only)
inline JpegInfo jpeg_info(const uint8_t *file, uint64_t size)
{
    uint32_t v[6] = {0, 0, 0, 0, 0, 0};
    check(cvhip_jpeg_info(file, size, v), "cvhip_jpeg_info");
    JpegInfo info;
    info.width = v[0], info.height = v[1], info.components = v[2], info.h = v[3], info.v = v[4], info.focal_length_35mm = v[5];
    return info;
}

// image::open(path)?.into_luma8() / into_rgb8() of the file's bytes, drop_rows (databar_height) rows cut from the bottom ->
// width x (height - drop_rows) pixels of 1 or 3 bytes
inline std::vector<uint8_t> jpeg_decode(GpuDevice &dev, const uint8_t *file, uint64_t size, Format format = Format::Luma8, uint32_t drop_rows = 0)
{
    return mesh::detail::size_then_fill([&](uint8_t *dst, uint64_t cap, uint64_t *out_size) {
        check(cvhip_jpeg_decode(dev.handle(), file, size, (uint32_t)format, drop_rows, dst, cap, out_size), "cvhip_jpeg_decode");
    });
}

// ---- progressive JPEG: the SOF2 files jpeg_decode refuses
struct JpegProgressiveInfo : JpegInfo {
    uint32_t scans = 0;
};

// the frame, the EXIF focal length and the number of scans of a progressive file's bytes (host only; the whole file is walked)
inline JpegProgressiveInfo jpeg_progressive_info(const uint8_t *file, uint64_t size)
{
    uint32_t v[7] = {0, 0, 0, 0, 0, 0, 0};
    check(cvhip_jpeg_progressive_info(file, size, v), "cvhip_jpeg_progressive_info");
    JpegProgressiveInfo info;
    info.width = v[0], info.height = v[1], info.components = v[2], info.h = v[3], info.v = v[4], info.focal_length_35mm = v[5], info.scans = v[6];
    return info;
}

// as jpeg_decode, of a progressive file
inline std::vector<uint8_t> jpeg_progressive_decode(GpuDevice &dev, const uint8_t *file, uint64_t size, Format format = Format::Luma8,
                                                    uint32_t drop_rows = 0)
{
    return mesh::detail::size_then_fill([&](uint8_t *dst, uint64_t cap, uint64_t *out_size) {
        check(cvhip_jpeg_progressive_decode(dev.handle(), file, size, (uint32_t)format, drop_rows, dst, cap, out_size), "cvhip_jpeg_progressive_decode");
    });
}

// ---- TIFF: the SEM pairs of --projection=parallel, with the metadata of reconstruction.rs:80-144
struct TiffInfo {
    uint32_t width = 0, height = 0, samples = 0, bits = 0, compression = 0, photometric = 0, predictor = 0, strips = 0, rows_per_strip = 0;
    uint32_t focal_length_35mm = 0; // EXIF FocalLengthIn35mmFilm, 0 = none
    uint32_t databar_height = 0;    // [PrivateFei] DatabarHeight of the SEM block (tag 34683 or 34682), 0 = none
    bool sem = false;               // an SEM block was found
    bool has_tilt_angle = false;    // tilt_angle is Some
    float scale[2] = {1.0f, 1.0f}, tilt_angle = 0.0f;
};
constexpr uint32_t DROP_DATABAR = CVHIP_TIFF_DROP_DATABAR; // as drop_rows: the file's own databar_height

// the first IFD, the EXIF focal length and the SEM block of a TIFF file's bytes (host only)
inline TiffInfo tiff_info(const uint8_t *file, uint64_t size)
{
    uint32_t v[12] = {0};
    float s[3] = {0.0f, 0.0f, 0.0f};
    check(cvhip_tiff_info(file, size, v, s), "cvhip_tiff_info");
    TiffInfo info;
    info.width = v[0], info.height = v[1], info.samples = v[2], info.bits = v[3], info.compression = v[4], info.photometric = v[5];
    info.predictor = v[6], info.strips = v[7], info.rows_per_strip = v[8], info.focal_length_35mm = v[9], info.databar_height = v[10];
    info.sem = (v[11] & 1u) != 0, info.has_tilt_angle = (v[11] & 2u) != 0;
    info.scale[0] = s[0], info.scale[1] = s[1], info.tilt_angle = s[2];
    return info;
}

// as jpeg_decode, of a TIFF file; drop_rows = DROP_DATABAR (the default) cuts the file's own databar_height, as SourceImage::load does
inline std::vector<uint8_t> tiff_decode(GpuDevice &dev, const uint8_t *file, uint64_t size, Format format = Format::Luma8, uint32_t drop_rows = DROP_DATABAR)
{
    return mesh::detail::size_then_fill([&](uint8_t *dst, uint64_t cap, uint64_t *out_size) {
        check(cvhip_tiff_decode(dev.handle(), file, size, (uint32_t)format, drop_rows, dst, cap, out_size), "cvhip_tiff_decode");
    });
}

// ---- TIFF, Deflate strips and tiled layout: a superset of tiff_info / tiff_decode, which answer as they always did
struct TiffExtInfo : TiffInfo {                                 // of a tiled file strips is the number of tiles, rows_per_strip TileLength
    uint32_t tile_width = 0, tile_length = 0, tiles_across = 0; // all 0: strips
};

inline TiffExtInfo tiff_ext_info(const uint8_t *file, uint64_t size)
{
    uint32_t v[16] = {0};
    float s[3] = {0.0f, 0.0f, 0.0f};
    check(cvhip_tiff_ext_info(file, size, v, s), "cvhip_tiff_ext_info");
    TiffExtInfo info;
    info.width = v[0], info.height = v[1], info.samples = v[2], info.bits = v[3], info.compression = v[4], info.photometric = v[5];
    info.predictor = v[6], info.strips = v[7], info.rows_per_strip = v[8], info.focal_length_35mm = v[9], info.databar_height = v[10];
    info.sem = (v[11] & 1u) != 0, info.has_tilt_angle = (v[11] & 2u) != 0;
    info.scale[0] = s[0], info.scale[1] = s[1], info.tilt_angle = s[2];
    info.tile_width = v[12], info.tile_length = v[13], info.tiles_across = v[14];
    return info;
}

// as tiff_decode, of a file that may hold Deflate streams or tiles
inline std::vector<uint8_t> tiff_ext_decode(GpuDevice &dev, const uint8_t *file, uint64_t size, Format format = Format::Luma8, uint32_t drop_rows = DROP_DATABAR)
{
    return mesh::detail::size_then_fill([&](uint8_t *dst, uint64_t cap, uint64_t *out_size) {
        check(cvhip_tiff_ext_decode(dev.handle(), file, size, (uint32_t)format, drop_rows, dst, cap, out_size), "cvhip_tiff_ext_decode");
    });
}

// ---- PNG: every colour type and bit depth, not interlaced; the SEM fields keep their defaults
struct PngInfo {
    uint32_t width = 0, height = 0, colour_type = 0, bit_depth = 0, interlace = 0, idat_chunks = 0;
    uint32_t focal_length_35mm = 0; // the eXIf chunk's FocalLengthIn35mmFilm, 0 = none
    bool plte = false, trns = false; // such a chunk was read
};

// IHDR, the chunks counted and the eXIf focal length of a PNG file's bytes (host only)
inline PngInfo png_info(const uint8_t *file, uint64_t size)
{
    uint32_t v[8] = {0};
    check(cvhip_png_info(file, size, v), "cvhip_png_info");
    PngInfo info;
    info.width = v[0], info.height = v[1], info.colour_type = v[2], info.bit_depth = v[3], info.interlace = v[4], info.idat_chunks = v[5];
    info.focal_length_35mm = v[6], info.plte = (v[7] & 1u) != 0, info.trns = (v[7] & 2u) != 0;
    return info;
}

// as jpeg_decode, of a PNG file
inline std::vector<uint8_t> png_decode(GpuDevice &dev, const uint8_t *file, uint64_t size, Format format = Format::Luma8, uint32_t drop_rows = 0)
{
    return mesh::detail::size_then_fill([&](uint8_t *dst, uint64_t cap, uint64_t *out_size) {
        check(cvhip_png_decode(dev.handle(), file, size, (uint32_t)format, drop_rows, dst, cap, out_size), "cvhip_png_decode");
    });
}

// ---- PNG, Adam7 interlaced files too: what png_info / png_decode take, and interlace method 1
inline PngInfo png_ext_info(const uint8_t *file, uint64_t size)
{
    uint32_t v[8] = {0};
    check(cvhip_png_ext_info(file, size, v), "cvhip_png_ext_info");
    PngInfo info;
    info.width = v[0], info.height = v[1], info.colour_type = v[2], info.bit_depth = v[3], info.interlace = v[4], info.idat_chunks = v[5];
    info.focal_length_35mm = v[6], info.plte = (v[7] & 1u) != 0, info.trns = (v[7] & 2u) != 0;
    return info;
}

// as png_decode
inline std::vector<uint8_t> png_ext_decode(GpuDevice &dev, const uint8_t *file, uint64_t size, Format format = Format::Luma8, uint32_t drop_rows = 0)
{
    return mesh::detail::size_then_fill([&](uint8_t *dst, uint64_t cap, uint64_t *out_size) {
        check(cvhip_png_ext_decode(dev.handle(), file, size, (uint32_t)format, drop_rows, dst, cap, out_size), "cvhip_png_ext_decode");
    });
}

// SourceImage::calibration_matrix (:164-185), row-major; focal_length_35mm 0 = none: 1
inline std::array<double, 9> calibration_matrix(uint32_t width, uint32_t height, uint32_t focal_length_35mm)
{
    const double diagonal_35mm = std::sqrt(24.0 * 24.0 + 36.0 * 36.0);
    const double w = (double)width, h = (double)height, diagonal = std::sqrt(w * w + h * h);
    const double focal = (double)(focal_length_35mm ? focal_length_35mm : 1u) * diagonal / diagonal_35mm;
    return {focal, 0.0, w / 2.0, 0.0, focal, h / 2.0, 0.0, 0.0, 1.0};
}

} // namespace image

} // namespace cvhip_host
