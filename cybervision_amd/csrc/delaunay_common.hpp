// delaunay_common.hpp — the Delaunay triangulation of a camera's points, one star at a time.
//
// Written once for every path of cvhip_mesh_delaunay: the device lanes (delaunay_kernels.hip; FilterPolicy, and LatticePolicy
// when every coordinate is an integer within 2^24) and the exact host path inside the library (ExactPolicy).  Compiles
// without HIP (tests/cpp/delaunay_host_exact.cpp, tests/cpp/delaunay_lattice_exact.cpp).
//
// The star of point a is built by WRAPPING over a uniform grid of the points:
//   - the start is a's nearest point (a nearest point is a Delaunay neighbour whatever else is co-circular: the disc on
//     the segment a-j as diameter lies inside the disc around a through j, which holds no point);
//   - the neighbour after j (counter-clockwise) is the point k left of a->j with no point inside circle(a, j, k): over the
//     candidates p left of a->j, p replaces k iff in_circle(a, j, k, p) > 0.  Any point inside circle(a, j, k) and left of
//     a->j lies in the LUNE of every earlier k, so scanning the cells that cover the lune of the current k is enough;
//   - no candidate left of a->j: a->j is a hull edge, and the wrap goes on clockwise from the start.
// Every decision is the sign of an exact determinant.  FilterPolicy evaluates it in f64 with Shewchuk's stage-A forward
// error bounds and answers UNSURE below them - the caller then abandons the star; ExactPolicy goes on with floating-point
// expansions (error-free two-sum, FMA two-product) and never answers UNSURE.  Both need -ffp-contract=off.
// The cells searched are computed in CELL SPACE ((x - min_x) / s) in rounded arithmetic and inflated by more than their
// error (DESIGN.md 4.13 has the bounds); a circle too flat to bound (|det| 2^20 < L^2) counts as the half-plane.
//
// LatticePolicy is exact as well and runs on the device: for integer-valued coordinates the determinants are plain integer
// arithmetic (its bound is stated at the policy).  It skips no duplicates: a candidate at the position of j, of the current k
// or of the tie polygon's first or last vertex flags the star instead, and the host path applies the duplicate rule.
//
// Exact ties (ExactPolicy and LatticePolicy): the points left of a->j on the empty circle through a and j form, with a and j, a convex
// polygon that is fanned from its lowest index m: the next neighbour is the polygon's first vertex after j when m = a, its
// last when m = j, and m otherwise.  Of several indices at one position the lowest is the vertex.
// The exactness holds while no product of coordinate differences over- or underflows (|differences| within 2^+-240).
#pragma once

#include <cmath>
#include <cstdint>

#if defined(__HIPCC__)
#define CVHIP_DLN_HD __host__ __device__
#else
#define CVHIP_DLN_HD
#endif

namespace cvhip {
namespace delaunay {

constexpr uint32_t NONE = 0xFFFFFFFFu; // no neighbour: a hull edge, or no other position at all
constexpr uint32_t FLAG = 0xFFFFFFFEu; // the star leaves this path (an undecided sign, or too many cells)
constexpr int UNSURE = 2;
constexpr double EPS = 1.1102230246251565e-16;            // 2^-53
constexpr double ORIENT_BOUND = (3.0 + 16.0 * EPS) * EPS;  // Shewchuk's ccwerrboundA
constexpr double CIRCLE_BOUND = (10.0 + 96.0 * EPS) * EPS; // Shewchuk's iccerrboundA
constexpr double DIST_BOUND = 1.0 - 3.552713678800501e-15; // 1 - 2^-48: two rounded squared distances (relative error < 4 EPS each) in certain order
constexpr double TINY = 1e-280;                            // below it a product may have underflowed: never certain
constexpr double FLAT = 1048576.0;                         // a circle with |det| FLAT < L^2 is not bounded (the half-plane is searched)

// the points and their uniform grid: square cells of side s over the bounding box, cell (cx, cy) holds cell_pts[cell_start[c]
// .. cell_start[c + 1]), c = cy * gw + cx, in any order
struct Grid {
    const double *xy;
    uint32_t k;
    double min_x, min_y, s, inv_s;
    uint32_t gw, gh;
    const uint32_t *cell_start, *cell_pts;
};

// the grid over an extent: about 2 points per cell, at most k / 2 + 1 cells along one axis.  A point extent (or one whose
// size overflows) gives one cell.
CVHIP_DLN_HD inline void grid_dims(double min_x, double max_x, double min_y, double max_y, uint64_t k, double *s, double *inv_s,
                                   uint32_t *gw, uint32_t *gh)
{
    const double w = max_x - min_x, h = max_y - min_y, T = (double)(k / 2 > 1 ? k / 2 : 1);
    double side = sqrt((w / T) * h);
    if (w / T > side) side = w / T;
    if (h / T > side) side = h / T;
    *s = 1.0, *inv_s = 0.0, *gw = 1, *gh = 1;
    if (!(side > 0.0) || !(side < INFINITY) || !(1.0 / side < INFINITY)) return;
    const double cw = floor(w / side) + 1.0, ch = floor(h / side) + 1.0;
    *s = side, *inv_s = 1.0 / side;
    *gw = (uint32_t)(cw < T + 1.0 ? cw : T + 1.0), *gh = (uint32_t)(ch < T + 1.0 ? ch : T + 1.0);
}

// cell-space coordinate -> cell index, monotone; NaN and anything below 1 -> 0
CVHIP_DLN_HD inline uint32_t cell_index(double u, uint32_t n) { return u >= 1.0 ? (u < (double)n ? (uint32_t)u : n - 1) : 0; }
CVHIP_DLN_HD inline uint32_t cell_of(const Grid &g, double x, double y)
{
    return cell_index((y - g.min_y) * g.inv_s, g.gh) * g.gw + cell_index((x - g.min_x) * g.inv_s, g.gw);
}

// ---- the filtered predicates: -1 / +1 when the sign is certain, UNSURE otherwise (zero included) ----------------------------
// sign of (bx - ax)(cy - ay) - (by - ay)(cx - ax): +1 = c left of a->b
CVHIP_DLN_HD inline int orient_filter(double ax, double ay, double bx, double by, double cx, double cy)
{
    const double l = (bx - ax) * (cy - ay), r = (by - ay) * (cx - ax);
    const double det = l - r, bound = ORIENT_BOUND * (fabs(l) + fabs(r));
    if (det > bound && det > TINY) return 1;
    if (-det > bound && -det > TINY) return -1;
    return UNSURE;
}

// +1 = d strictly inside the circle through a, b, c when those are counter-clockwise (the sign flips when they are clockwise)
CVHIP_DLN_HD inline int circle_filter(double ax, double ay, double bx, double by, double cx, double cy, double dx, double dy)
{
    const double adx = ax - dx, ady = ay - dy, bdx = bx - dx, bdy = by - dy, cdx = cx - dx, cdy = cy - dy;
    const double bdxcdy = bdx * cdy, cdxbdy = cdx * bdy, cdxady = cdx * ady, adxcdy = adx * cdy, adxbdy = adx * bdy, bdxady = bdx * ady;
    const double alift = adx * adx + ady * ady, blift = bdx * bdx + bdy * bdy, clift = cdx * cdx + cdy * cdy;
    const double det = alift * (bdxcdy - cdxbdy) + blift * (cdxady - adxcdy) + clift * (adxbdy - bdxady);
    const double permanent = (fabs(bdxcdy) + fabs(cdxbdy)) * alift + (fabs(cdxady) + fabs(adxcdy)) * blift + (fabs(adxbdy) + fabs(bdxady)) * clift;
    const double bound = CIRCLE_BOUND * permanent;
    if (det > bound && det > TINY) return 1;
    if (-det > bound && -det > TINY) return -1;
    return UNSURE;
}

CVHIP_DLN_HD inline double dist2(double ax, double ay, double px, double py)
{
    const double dx = px - ax, dy = py - ay;
    return dx * dx + dy * dy;
}

// sign of |p - a|^2 - |q - a|^2
CVHIP_DLN_HD inline int dist_filter(double ax, double ay, double px, double py, double qx, double qy)
{
    const double dp = dist2(ax, ay, px, py), dq = dist2(ax, ay, qx, qy);
    if (dp < dq * DIST_BOUND && dq > TINY && dp > TINY) return -1;
    if (dq < dp * DIST_BOUND && dq > TINY && dp > TINY) return 1;
    return UNSURE;
}

// the device lanes' policy: the filter alone
struct FilterPolicy {
    CVHIP_DLN_HD int orient(double ax, double ay, double bx, double by, double cx, double cy) const { return orient_filter(ax, ay, bx, by, cx, cy); }
    CVHIP_DLN_HD int circle(double ax, double ay, double bx, double by, double cx, double cy, double dx, double dy) const
    {
        return circle_filter(ax, ay, bx, by, cx, cy, dx, dy);
    }
    CVHIP_DLN_HD int dist(double ax, double ay, double px, double py, double qx, double qy) const { return dist_filter(ax, ay, px, py, qx, qy); }
    CVHIP_DLN_HD bool skip(uint32_t) const { return false; } // a duplicate is never skipped: its zero determinant flags the star
    CVHIP_DLN_HD bool same_position(double, double, double, double) const { return false; } // (that zero comes first)
};

// ---- the lattice policy: exact signs of integer-valued coordinates, on the device as on the host -----------------------------
// Valid when every coordinate is an integer with |v| <= LATTICE_MAX = 2^24 (the caller checks all of them before it picks this
// policy).  Then every coordinate difference is an integer below 2^25 in magnitude, and
//   orient: the two products are below 2^50, their difference below 2^51                                  - 64-bit integers;
//   dist:   the four squares are below 2^50, each sum below 2^51, their difference below 2^52             - 64-bit integers;
//   circle: the lifts (sums of two squares) and the 2 x 2 minors (differences of two products) are below 2^51, a lift times
//           a minor below 2^102, the sum of the three below 2^104                                         - 128-bit signed.
// The f64 filter runs first, as in ExactPolicy, and the integers only where it is UNSURE; the policy never answers UNSURE.
constexpr double LATTICE_MAX = 16777216.0; // 2^24

CVHIP_DLN_HD inline bool on_lattice(double v) { return fabs(v) <= LATTICE_MAX && v == rint(v); } // (false for NaN and infinity)

CVHIP_DLN_HD inline int orient_lattice(double ax, double ay, double bx, double by, double cx, double cy)
{
    const int64_t iax = (int64_t)ax, iay = (int64_t)ay;
    const int64_t l = ((int64_t)bx - iax) * ((int64_t)cy - iay), r = ((int64_t)by - iay) * ((int64_t)cx - iax);
    return (l > r) - (l < r);
}

CVHIP_DLN_HD inline int circle_lattice(double ax, double ay, double bx, double by, double cx, double cy, double dx, double dy)
{
    const int64_t idx = (int64_t)dx, idy = (int64_t)dy;
    const int64_t adx = (int64_t)ax - idx, ady = (int64_t)ay - idy, bdx = (int64_t)bx - idx, bdy = (int64_t)by - idy,
                  cdx = (int64_t)cx - idx, cdy = (int64_t)cy - idy;
    const int64_t alift = adx * adx + ady * ady, blift = bdx * bdx + bdy * bdy, clift = cdx * cdx + cdy * cdy;
    const __int128 det = (__int128)alift * (bdx * cdy - cdx * bdy) + (__int128)blift * (cdx * ady - adx * cdy) +
                         (__int128)clift * (adx * bdy - bdx * ady);
    return (det > 0) - (det < 0);
}

CVHIP_DLN_HD inline int dist_lattice(double ax, double ay, double px, double py, double qx, double qy)
{
    const int64_t iax = (int64_t)ax, iay = (int64_t)ay;
    const int64_t pdx = (int64_t)px - iax, pdy = (int64_t)py - iay, qdx = (int64_t)qx - iax, qdy = (int64_t)qy - iay;
    const int64_t dp = pdx * pdx + pdy * pdy, dq = qdx * qdx + qdy * qdy;
    return (dp > dq) - (dp < dq);
}

struct LatticePolicy {
    CVHIP_DLN_HD int orient(double ax, double ay, double bx, double by, double cx, double cy) const
    {
        const int s = orient_filter(ax, ay, bx, by, cx, cy);
        return s != UNSURE ? s : orient_lattice(ax, ay, bx, by, cx, cy);
    }
    CVHIP_DLN_HD int circle(double ax, double ay, double bx, double by, double cx, double cy, double dx, double dy) const
    {
        const int s = circle_filter(ax, ay, bx, by, cx, cy, dx, dy);
        return s != UNSURE ? s : circle_lattice(ax, ay, bx, by, cx, cy, dx, dy);
    }
    CVHIP_DLN_HD int dist(double ax, double ay, double px, double py, double qx, double qy) const
    {
        const int s = dist_filter(ax, ay, px, py, qx, qy);
        return s != UNSURE ? s : dist_lattice(ax, ay, px, py, qx, qy);
    }
    CVHIP_DLN_HD bool skip(uint32_t) const { return false; } // duplicates stay with the host: same_position flags the star
    CVHIP_DLN_HD bool same_position(double px, double py, double qx, double qy) const { return px == qx && py == qy; }
};

// ---- one star ---------------------------------------------------------------------------------------------------------------
struct StarWork {
    uint64_t cells = 0;  // grid cells visited so far
    uint64_t lane_cells; // more than this many: FLAG
};

// a's nearest point (Pol::dist decides; of exactly equidistant ones the lowest index), NONE when no other position exists
template <class Pol> CVHIP_DLN_HD uint32_t nearest(const Grid &g, const Pol &pol, uint32_t a, StarWork &w)
{
    const double ax = g.xy[2 * a], ay = g.xy[2 * a + 1];
    const uint32_t cax = cell_index((ax - g.min_x) * g.inv_s, g.gw), cay = cell_index((ay - g.min_y) * g.inv_s, g.gh);
    uint32_t best = NONE;
    for (uint32_t R = 1;; R++) {
        const uint32_t x0 = cax > R ? cax - R : 0, y0 = cay > R ? cay - R : 0;
        const uint32_t x1 = g.gw - 1 - cax > R ? cax + R : g.gw - 1, y1 = g.gh - 1 - cay > R ? cay + R : g.gh - 1;
        for (uint32_t cy = y0; cy <= y1; cy++) {
            // the block's new ring: its first and last row whole, of the rows between them the two end cells
            const bool whole = R == 1 || (cy > cay ? cy - cay : cay - cy) == R;
            const uint32_t stride = whole || cax < R ? 1 : 2 * R; // (cax < R: the left end lies outside the grid)
            for (uint32_t cx = whole || cax < R ? x0 : cax - R; cx <= x1; cx += stride) {
                if (!whole && (cx > cax ? cx - cax : cax - cx) != R) continue; // (within the ring's sides only on a clipped block)
                if (++w.cells > w.lane_cells) return FLAG;
                const uint32_t c = cy * g.gw + cx;
                for (uint32_t q = g.cell_start[c], end = g.cell_start[c + 1]; q < end; q++) {
                    const uint32_t p = g.cell_pts[q];
                    if (p == a || p >= g.k || pol.skip(p)) continue;
                    if (g.xy[2 * p] == ax && g.xy[2 * p + 1] == ay) return FLAG; // (a duplicate: the exact policy skips them)
                    if (best == NONE) {
                        best = p;
                        continue;
                    }
                    const int o = pol.dist(ax, ay, g.xy[2 * p], g.xy[2 * p + 1], g.xy[2 * best], g.xy[2 * best + 1]);
                    if (o == UNSURE) return FLAG;
                    if (o < 0 || (o == 0 && p < best)) best = p;
                }
            }
        }
        if (x0 == 0 && y0 == 0 && x1 == g.gw - 1 && y1 == g.gh - 1) break;
        // a point outside the block is more than R - 1e-3 cells away (the cell coordinates are within 1e-6 cells of exact)
        if (best != NONE) {
            const double reach = ((double)R - 1e-3) * g.s;
            if (dist2(ax, ay, g.xy[2 * best], g.xy[2 * best + 1]) <= reach * reach * (1.0 - 1e-9)) break;
        }
    }
    return best;
}

// the neighbour after j around a, counter-clockwise (dir = +1) or clockwise (dir = -1); NONE at a hull edge
template <class Pol> CVHIP_DLN_HD uint32_t wrap_step(const Grid &g, const Pol &pol, uint32_t a, uint32_t j, int dir, StarWork &w)
{
    const double ax = g.xy[2 * a], ay = g.xy[2 * a + 1], jx = g.xy[2 * j], jy = g.xy[2 * j + 1];
    // cell space: a's position, and dir * (j - a) from the doubles themselves (relative error 2 EPS)
    const double ua = (ax - g.min_x) * g.inv_s, va = (ay - g.min_y) * g.inv_s;
    const double bu = (jx - ax) * g.inv_s, bv = (jy - ay) * g.inv_s;
    const double eu = dir > 0 ? bu : -bu, ev = dir > 0 ? bv : -bv; // searched: eu (v - va) - ev (u - ua) > 0
    const double b2 = bu * bu + bv * bv;
    uint32_t k = NONE, kmin = NONE, kfirst = NONE, klast = NONE; // the best candidate; of those tied with it the lowest, first and last
    double kx = 0, ky = 0;
    bool bounded = false; // the current circle in cell space, inflated: centre (cu, cv), radius R
    double cu = 0, cv = 0, R = 0;

    auto circle_of = [&]() {
        const double du = (kx - ax) * g.inv_s, dv = (ky - ay) * g.inv_s, c2 = du * du + dv * dv;
        const double det = bu * dv - bv * du, L2 = b2 > c2 ? b2 : c2;
        bounded = false;
        if (!(fabs(det) * FLAT >= L2) || !(L2 > 0.0)) return;
        const double ou = (dv * b2 - bv * c2) / (2.0 * det), ov = (bu * c2 - du * b2) / (2.0 * det);
        cu = ua + ou, cv = va + ov;
        R = sqrt(ou * ou + ov * ov) * (1.0 + 1e-6) + 1e-6 * sqrt(L2) + 1e-3;
        bounded = R < INFINITY && cu - cu == 0.0 && cv - cv == 0.0;
    };
    // -> false: the star leaves this path
    auto scan_cell = [&](uint32_t cx, uint32_t cy) -> bool {
        if (++w.cells > w.lane_cells) return false;
        const uint32_t c = cy * g.gw + cx;
        for (uint32_t q = g.cell_start[c], end = g.cell_start[c + 1]; q < end; q++) {
            const uint32_t p = g.cell_pts[q];
            if (p == a || p == j || p == k || p >= g.k || pol.skip(p)) continue;
            const double px = g.xy[2 * p], py = g.xy[2 * p + 1];
            if (pol.same_position(px, py, jx, jy) || (k != NONE && pol.same_position(px, py, kx, ky))) return false; // (a duplicate)
            const int o = pol.orient(ax, ay, jx, jy, px, py);
            if (o == UNSURE) return false;
            if (o * dir <= 0) continue;
            int s = 1;
            if (k != NONE) {
                s = pol.circle(ax, ay, jx, jy, kx, ky, px, py);
                if (s == UNSURE) return false;
                s *= dir;
            }
            if (s > 0) {
                k = kmin = kfirst = klast = p, kx = px, ky = py;
                circle_of();
            } else if (s == 0) { // (exact policies only) p lies on the circle: one more vertex of the polygon
                if ((p != kfirst && pol.same_position(px, py, g.xy[2 * kfirst], g.xy[2 * kfirst + 1])) ||
                    (p != klast && pol.same_position(px, py, g.xy[2 * klast], g.xy[2 * klast + 1])))
                    return false; // (a duplicate of a vertex that may be returned; a cell can be scanned twice, so p may be that vertex)
                if (p < kmin) kmin = p;
                const int of = pol.orient(ax, ay, g.xy[2 * kfirst], g.xy[2 * kfirst + 1], px, py);
                const int ol = pol.orient(ax, ay, g.xy[2 * klast], g.xy[2 * klast + 1], px, py);
                if (of == UNSURE || ol == UNSURE) return false;
                if (of * dir < 0) kfirst = p;
                if (ol * dir > 0) klast = p;
            }
        }
        return true;
    };

    // the 3 x 3 block around a: a first candidate, near
    const uint32_t cax = cell_index(ua, g.gw), cay = cell_index(va, g.gh);
    for (uint32_t cy = cay ? cay - 1 : 0; cy <= (cay + 1 < g.gh ? cay + 1 : g.gh - 1); cy++)
        for (uint32_t cx = cax ? cax - 1 : 0; cx <= (cax + 1 < g.gw ? cax + 1 : g.gw - 1); cx++)
            if (!scan_cell(cx, cy)) return FLAG;

    // the rows that the lune of the current candidate can touch: its circle's rows, and the half-plane's over u in [0, gw]
    double vlo = -INFINITY, vhi = INFINITY;
    if (bounded) vlo = cv - R, vhi = cv + R;
    if (eu != 0.0) {
        const double t0 = ev * (0.0 - ua) / eu, t1 = ev * ((double)g.gw - ua) / eu;
        if (eu > 0.0) {
            const double t = t0 < t1 ? t0 : t1, lim = va + t - (1e-3 + 1e-9 * fabs(t));
            if (lim > vlo) vlo = lim;
        } else {
            const double t = t0 > t1 ? t0 : t1, lim = va + t + (1e-3 + 1e-9 * fabs(t));
            if (lim < vhi) vhi = lim;
        }
    }
    if (!(vlo <= vhi)) vlo = -INFINITY, vhi = INFINITY; // (NaN: everything)
    const uint32_t r0 = cell_index(vlo, g.gh), r1 = cell_index(vhi, g.gh);
    const bool none = vhi < 0.0 || vlo > (double)g.gh + 1.0; // the half-plane misses the grid
    for (uint32_t r = r0; r <= r1 && !none; r++) {
        const double y0 = (double)r, y1 = (double)r + 1.0;
        double ulo = -INFINITY, uhi = INFINITY;
        if (bounded) { // (the circle only shrinks on this side of a->j while k improves)
            if (y0 > cv + R) break;
            if (y1 < cv - R) continue;
            const double d = cv < y0 ? y0 - cv : (cv > y1 ? cv - y1 : 0.0); // the row's chord (1e-9 R^2 is far above its rounding)
            const double rr = R * R * (1.0 + 1e-9) - d * d, hw = rr > 0.0 ? sqrt(rr) : 0.0;
            ulo = cu - hw, uhi = cu + hw;
        }
        if (ev != 0.0) {
            const double t0 = eu * (y0 - va) / ev, t1 = eu * (y1 - va) / ev;
            if (ev > 0.0) {
                const double t = t0 > t1 ? t0 : t1, lim = ua + t + (1e-3 + 1e-9 * fabs(t));
                if (lim < uhi) uhi = lim;
            } else {
                const double t = t0 < t1 ? t0 : t1, lim = ua + t - (1e-3 + 1e-9 * fabs(t));
                if (lim > ulo) ulo = lim;
            }
        } else if (eu > 0.0) {
            if (y1 < va - 1e-3) continue;
        } else if (eu < 0.0) {
            if (y0 > va + 1e-3) continue;
        }
        if (ulo > uhi || uhi < 0.0 || ulo > (double)g.gw + 1.0) continue;
        const uint32_t c0 = cell_index(ulo, g.gw), c1 = cell_index(uhi, g.gw);
        for (uint32_t c = c0; c <= c1; c++)
            if (!scan_cell(c, r)) return FLAG;
    }
    if (k == NONE) return NONE;
    if (kmin < a && kmin < j) return kmin;
    return a < j ? kfirst : klast;
}

// The star of a: emit(a, b, c) for its faces in counter-clockwise order, in the order of the wrap (counter-clockwise from
// the nearest point; at a hull point then clockwise from it).  -> false: the star leaves this path (what was emitted is void).
template <class Pol, class Emit>
CVHIP_DLN_HD bool build_star(const Grid &g, const Pol &pol, uint32_t a, uint64_t lane_cells, uint32_t max_neighbours, Emit &emit, uint64_t *cells)
{
    StarWork w;
    w.lane_cells = lane_cells;
    *cells = 0;
    if (pol.skip(a)) return true; // a higher index at a lower one's position: in no face
    const uint32_t j0 = nearest(g, pol, a, w);
    *cells = w.cells;
    if (j0 == FLAG) return false;
    if (j0 == NONE) return true;
    uint32_t j = j0, steps = 0;
    bool closed = false;
    for (;; steps++) {
        if (steps >= max_neighbours) return false;
        const uint32_t n = wrap_step(g, pol, a, j, 1, w);
        *cells = w.cells;
        if (n == FLAG) return false;
        if (n == NONE) break;
        emit(a, j, n);
        if (n == j0) {
            closed = true;
            break;
        }
        j = n;
    }
    if (closed) return true;
    j = j0;
    for (;; steps++) {
        if (steps >= max_neighbours) return false;
        const uint32_t n = wrap_step(g, pol, a, j, -1, w);
        *cells = w.cells;
        if (n == FLAG) return false;
        if (n == NONE) break;
        emit(a, n, j);
        j = n;
    }
    return true;
}

} // namespace delaunay
} // namespace cvhip

// ---- the exact policy: host code only (unannotated, so hipcc never compiles it for the device) -------------------------------
#include <algorithm>
#include <vector>

namespace cvhip {
namespace delaunay {

// A floating-point expansion (Shewchuk 1997): non-overlapping components in increasing magnitude, zeros dropped (empty = 0)
typedef std::vector<double> Expansion;

inline void two_sum(double a, double b, double &x, double &y)
{
    x = a + b;
    const double bv = x - a, av = x - bv;
    y = (a - av) + (b - bv);
}
inline void fast_two_sum(double a, double b, double &x, double &y) // |a| >= |b|
{
    x = a + b;
    y = b - (x - a);
}
inline void two_product(double a, double b, double &x, double &y)
{
    x = a * b;
    y = std::fma(a, b, -x);
}

inline Expansion ex_diff(double a, double b) // a - b
{
    const double x = a - b, bv = a - x, av = x + bv, y = (a - av) + (bv - b);
    Expansion e;
    if (y != 0.0) e.push_back(y);
    if (x != 0.0) e.push_back(x);
    return e;
}

// e + f in one merge (fast_expansion_sum with zero elimination)
inline Expansion ex_sum(const Expansion &e, const Expansion &f)
{
    if (e.empty()) return f;
    if (f.empty()) return e;
    Expansion h;
    h.reserve(e.size() + f.size());
    size_t ei = 0, fi = 0;
    auto take = [&]() { // the next component of the merge by magnitude
        if (fi >= f.size() || (ei < e.size() && std::fabs(e[ei]) <= std::fabs(f[fi]))) return e[ei++];
        return f[fi++];
    };
    double Q = take(), x, y;
    if (ei < e.size() || fi < f.size()) {
        const double g = take();
        fast_two_sum(g, Q, x, y);
        Q = x;
        if (y != 0.0) h.push_back(y);
    }
    while (ei < e.size() || fi < f.size()) {
        two_sum(Q, take(), x, y);
        Q = x;
        if (y != 0.0) h.push_back(y);
    }
    if (Q != 0.0) h.push_back(Q);
    return h;
}

inline Expansion ex_scale(const Expansion &e, double b)
{
    Expansion h;
    if (e.empty() || b == 0.0) return h;
    h.reserve(2 * e.size());
    double Q, lo, p1, p0, sum;
    two_product(e[0], b, Q, lo);
    if (lo != 0.0) h.push_back(lo);
    for (size_t i = 1; i < e.size(); i++) {
        two_product(e[i], b, p1, p0);
        two_sum(Q, p0, sum, lo);
        if (lo != 0.0) h.push_back(lo);
        fast_two_sum(p1, sum, Q, lo);
        if (lo != 0.0) h.push_back(lo);
    }
    if (Q != 0.0) h.push_back(Q);
    return h;
}

inline Expansion ex_mul(const Expansion &e, const Expansion &f)
{
    Expansion acc;
    for (double b : f) acc = ex_sum(acc, ex_scale(e, b));
    return acc;
}
inline Expansion ex_neg(Expansion e)
{
    for (double &v : e) v = -v;
    return e;
}
inline Expansion ex_sub(const Expansion &e, const Expansion &f) { return ex_sum(e, ex_neg(f)); }
inline int ex_sign(const Expansion &e) { return e.empty() ? 0 : (e.back() > 0.0 ? 1 : -1); }

inline int orient_exact(double ax, double ay, double bx, double by, double cx, double cy)
{
    return ex_sign(ex_sub(ex_mul(ex_diff(bx, ax), ex_diff(cy, ay)), ex_mul(ex_diff(by, ay), ex_diff(cx, ax))));
}
inline int circle_exact(double ax, double ay, double bx, double by, double cx, double cy, double dx, double dy)
{
    const Expansion adx = ex_diff(ax, dx), ady = ex_diff(ay, dy), bdx = ex_diff(bx, dx), bdy = ex_diff(by, dy), cdx = ex_diff(cx, dx),
                    cdy = ex_diff(cy, dy);
    const Expansion alift = ex_sum(ex_mul(adx, adx), ex_mul(ady, ady)), blift = ex_sum(ex_mul(bdx, bdx), ex_mul(bdy, bdy)),
                    clift = ex_sum(ex_mul(cdx, cdx), ex_mul(cdy, cdy));
    const Expansion ta = ex_mul(alift, ex_sub(ex_mul(bdx, cdy), ex_mul(cdx, bdy))), tb = ex_mul(blift, ex_sub(ex_mul(cdx, ady), ex_mul(adx, cdy))),
                    tc = ex_mul(clift, ex_sub(ex_mul(adx, bdy), ex_mul(bdx, ady)));
    return ex_sign(ex_sum(ex_sum(ta, tb), tc));
}
inline int dist_exact(double ax, double ay, double px, double py, double qx, double qy)
{
    const Expansion pdx = ex_diff(px, ax), pdy = ex_diff(py, ay), qdx = ex_diff(qx, ax), qdy = ex_diff(qy, ay);
    return ex_sign(ex_sub(ex_sum(ex_mul(pdx, pdx), ex_mul(pdy, pdy)), ex_sum(ex_mul(qdx, qdx), ex_mul(qdy, qdy))));
}

// which points are a higher index at a lower one's position - found cell by cell, when a cell is first asked about
class Duplicates {
  public:
    explicit Duplicates(const Grid &g) : g_(g), dup_(g.k, 0), done_((size_t)g.gw * g.gh, 0) {}
    bool is_duplicate(uint32_t p)
    {
        const uint32_t c = cell_of(g_, g_.xy[2 * p], g_.xy[2 * p + 1]);
        if (!done_[c]) mark(c);
        return dup_[p] != 0;
    }
    uint64_t count_all() // every cell
    {
        uint64_t n = 0;
        for (size_t c = 0; c < done_.size(); c++)
            if (!done_[c]) mark((uint32_t)c);
        for (uint8_t d : dup_) n += d;
        return n;
    }

  private:
    void mark(uint32_t c)
    {
        done_[c] = 1;
        std::vector<uint32_t> pts(g_.cell_pts + g_.cell_start[c], g_.cell_pts + g_.cell_start[c + 1]);
        const double *xy = g_.xy;
        std::sort(pts.begin(), pts.end(), [xy](uint32_t p, uint32_t q) {
            if (xy[2 * p] != xy[2 * q]) return xy[2 * p] < xy[2 * q];
            if (xy[2 * p + 1] != xy[2 * q + 1]) return xy[2 * p + 1] < xy[2 * q + 1];
            return p < q;
        });
        for (size_t i = 1; i < pts.size(); i++)
            if (xy[2 * pts[i]] == xy[2 * pts[i - 1]] && xy[2 * pts[i] + 1] == xy[2 * pts[i - 1] + 1]) dup_[pts[i]] = 1;
    }
    const Grid &g_;
    std::vector<uint8_t> dup_, done_;
};

// the host path's policy: the filter, then the expansions - never UNSURE
struct ExactPolicy {
    Duplicates *dups;
    int orient(double ax, double ay, double bx, double by, double cx, double cy) const
    {
        const int s = orient_filter(ax, ay, bx, by, cx, cy);
        return s != UNSURE ? s : orient_exact(ax, ay, bx, by, cx, cy);
    }
    int circle(double ax, double ay, double bx, double by, double cx, double cy, double dx, double dy) const
    {
        const int s = circle_filter(ax, ay, bx, by, cx, cy, dx, dy);
        return s != UNSURE ? s : circle_exact(ax, ay, bx, by, cx, cy, dx, dy);
    }
    int dist(double ax, double ay, double px, double py, double qx, double qy) const
    {
        const int s = dist_filter(ax, ay, px, py, qx, qy);
        return s != UNSURE ? s : dist_exact(ax, ay, px, py, qx, qy);
    }
    bool skip(uint32_t p) const { return dups->is_duplicate(p); }
    bool same_position(double, double, double, double) const { return false; } // (a duplicate never gets that far)
};

// the grid built on the host (the library downloads the device's instead): cell_start and cell_pts are filled
inline Grid host_grid(const double *xy, uint32_t k, std::vector<uint32_t> &cell_start, std::vector<uint32_t> &cell_pts)
{
    Grid g{xy, k, 0.0, 0.0, 1.0, 0.0, 1, 1, nullptr, nullptr};
    double max_x = 0.0, max_y = 0.0;
    for (uint32_t i = 0; i < k; i++) {
        const double x = xy[2 * i], y = xy[2 * i + 1];
        if (!i || x < g.min_x) g.min_x = x;
        if (!i || x > max_x) max_x = x;
        if (!i || y < g.min_y) g.min_y = y;
        if (!i || y > max_y) max_y = y;
    }
    grid_dims(g.min_x, max_x, g.min_y, max_y, k, &g.s, &g.inv_s, &g.gw, &g.gh);
    const size_t cells = (size_t)g.gw * g.gh;
    cell_start.assign(cells + 1, 0);
    cell_pts.assign(k, 0);
    for (uint32_t i = 0; i < k; i++) cell_start[cell_of(g, xy[2 * i], xy[2 * i + 1]) + 1]++;
    for (size_t c = 0; c < cells; c++) cell_start[c + 1] += cell_start[c];
    std::vector<uint32_t> cursor(cell_start.begin(), cell_start.end() - 1);
    for (uint32_t i = 0; i < k; i++) cell_pts[cursor[cell_of(g, xy[2 * i], xy[2 * i + 1])]++] = i;
    g.cell_start = cell_start.data(), g.cell_pts = cell_pts.data();
    return g;
}

} // namespace delaunay
} // namespace cvhip
