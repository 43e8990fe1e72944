// mesh_kernels.hip — the mesh stage of output::output (src/output.rs:567-611) on the device: the camera points that feed
// the Delaunay triangulation (Mesh::process_camera, :401-423), DepthBuffer::new and polygon_obstructs (:256-353), the
// polygon list's merge (:50-105, :384, :510-516) and ImageWriter's depth map (:1009-1143).  DESIGN.md 4.11.
//
// All f64, one IEEE operation per written operation in the written order (-ffp-contract=off).  The Delaunay construction
// is delaunay_kernels.hip (a caller may supply triangles of its own just as well); the PLY writer and the colour
// mapping are mesh_output_kernels.hip, the OBJ writer is mesh_obj_kernels.hip; the colour table and the PNG encoder stay out.
//
// Two results of the reference depend on its thread order; here they are defined:
//   - DepthBuffer::new keeps a new depth iff the cell is empty or cur - new > f64::EPSILON, folding the points in
//     par_bridge's arbitrary order.  Here the cell is the MINIMUM of its depths (the depth image: the MAXIMUM) - one of
//     the reference's outcomes whenever no two depths of a cell differ by a non-zero amount <= EPSILON.
//   - process_camera sorts the list with sort_unstable and de-duplicates it by vertices alone, so which camera's copy of
//     a triple produced by two cameras survives is not determined.  Here the LOWEST camera wins.
#include <cmath>
#include <cstring>

#include "cvhip_internal.hpp"
#include "tri_common.hpp"

namespace cvhip {
namespace {

constexpr int BLOCK = 256;
constexpr int MAX_GRID = CVHIP_MESH_GRID_LANES / BLOCK; // blocks of a grid-stride launch
constexpr unsigned long long KEY_NONE_MIN = ~0ull;      // empty cell of a minimum buffer
constexpr unsigned long long KEY_NONE_MAX = 0ull;       // empty cell of a maximum map
constexpr uint32_t FLAG_RANGE = 1u, FLAG_SEEN = 2u;

// what the kernels read of one camera: the projection (Surface::project_point, triangulation.rs:63-74), row 2 of
// r_matrix and r_matrix^T t (Camera::point_depth, :492-495) and img_range (output.rs:613-624)
struct MeshCam {
    double P[12];
    double R2[3], Rtt[3];
    double lo[2], hi[2];
};

struct Extent {
    double min_x, max_x, min_y, max_y;
    unsigned long long count;
};

// the order-preserving map f64 -> u64 (negative depths order correctly too) and back
__device__ __forceinline__ unsigned long long key_of(double d)
{
    const unsigned long long b = (unsigned long long)__double_as_longlong(d);
    return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}
__device__ __forceinline__ double value_of(unsigned long long k)
{
    const unsigned long long b = (k >> 63) ? (k & 0x7FFFFFFFFFFFFFFFull) : ~k;
    return __longlong_as_double((long long)b);
}

// f64::round (half away from zero) `as usize` (saturating: negative and NaN -> 0), capped at `cap`
__device__ __forceinline__ unsigned long long round_usize(double v, unsigned long long cap)
{
    const double r = round(v);
    if (!(r > 0.0)) return 0;
    return r >= (double)cap ? cap : (unsigned long long)r;
}

// f64::clamp(0.0, max as f64) as usize (:132-135, 219-220): NaN stays NaN and converts to 0
__device__ __forceinline__ uint32_t clamp_usize(double v, uint32_t mx)
{
    const double m = (double)mx;
    const double c = v < 0.0 ? 0.0 : (v > m ? m : v);
    return c == c ? (uint32_t)c : 0u;
}

// ---- project: one lane per track ------------------------------------------------------------------------------------------
// plane[i] = (x, y, depth, flags) of track i in the camera; partial[block] = the extent of the tracks whose flags hold
// every bit of `sel`, reduced in a fixed order (tree over the block's lanes; extent_final_kernel folds the blocks in order)
__global__ __launch_bounds__(BLOCK) void mesh_project_kernel(const double *__restrict__ points, const int2 *__restrict__ tracks,
                                                             unsigned long long n, uint32_t m, uint32_t cam, MeshCam c,
                                                             uint32_t sel, double4 *__restrict__ plane, Extent *__restrict__ partial)
{
    __shared__ double s_v[4][BLOCK];
    __shared__ unsigned long long s_n[BLOCK];
    double mnx = INFINITY, mxx = -INFINITY, mny = INFINITY, mxy = -INFINITY;
    unsigned long long cnt = 0;
    for (unsigned long long i = (unsigned long long)blockIdx.x * BLOCK + threadIdx.x; i < n; i += (unsigned long long)gridDim.x * BLOCK) {
        const double X = points[3 * i], Y = points[3 * i + 1], Z = points[3 * i + 2];
        double p[3];
        for (int k = 0; k < 3; k++) p[k] = ((c.P[4 * k] * X + c.P[4 * k + 1] * Y) + c.P[4 * k + 2] * Z) + c.P[4 * k + 3];
        const double scale = fabs(p[2]) < F64_EPS ? 1.0 : p[2];
        const double x = p[0] / scale, y = p[1] / scale;
        const double q0 = X + c.Rtt[0], q1 = Y + c.Rtt[1], q2 = Z + c.Rtt[2];
        const double depth = (c.R2[0] * q0 + c.R2[1] * q1) + c.R2[2] * q2;
        uint32_t f = 0;
        if (c.lo[0] <= x && x < c.hi[0] && c.lo[1] <= y && y < c.hi[1]) f |= FLAG_RANGE;
        if (tracks[i * m + cam].x >= 0) f |= FLAG_SEEN;
        plane[i] = make_double4(x, y, depth, (double)f);
        if ((f & sel) == sel) {
            mnx = fmin(mnx, x), mxx = fmax(mxx, x), mny = fmin(mny, y), mxy = fmax(mxy, y);
            cnt++;
        }
    }
    const int t = threadIdx.x;
    s_v[0][t] = mnx, s_v[1][t] = mxx, s_v[2][t] = mny, s_v[3][t] = mxy, s_n[t] = cnt;
    __syncthreads();
    for (int w = BLOCK / 2; w > 0; w >>= 1) {
        if (t < w) {
            s_v[0][t] = fmin(s_v[0][t], s_v[0][t + w]), s_v[1][t] = fmax(s_v[1][t], s_v[1][t + w]);
            s_v[2][t] = fmin(s_v[2][t], s_v[2][t + w]), s_v[3][t] = fmax(s_v[3][t], s_v[3][t + w]);
            s_n[t] += s_n[t + w];
        }
        __syncthreads();
    }
    if (t == 0) partial[blockIdx.x] = Extent{s_v[0][0], s_v[1][0], s_v[2][0], s_v[3][0], s_n[0]};
}

__global__ void extent_final_kernel(const Extent *__restrict__ partial, uint32_t blocks, Extent *__restrict__ out)
{
    if (threadIdx.x || blockIdx.x) return;
    Extent e{INFINITY, -INFINITY, INFINITY, -INFINITY, 0};
    for (uint32_t b = 0; b < blocks; b++) {
        const Extent p = partial[b];
        e.min_x = fmin(e.min_x, p.min_x), e.max_x = fmax(e.max_x, p.max_x);
        e.min_y = fmin(e.min_y, p.min_y), e.max_y = fmax(e.max_y, p.max_y);
        e.count += p.count;
    }
    *out = e;
}

__global__ __launch_bounds__(BLOCK) void fill_u64_kernel(unsigned long long *__restrict__ p, unsigned long long v, unsigned long long n)
{
    for (unsigned long long i = (unsigned long long)blockIdx.x * BLOCK + threadIdx.x; i < n; i += (unsigned long long)gridDim.x * BLOCK) p[i] = v;
}

// ---- depth-buffer scatter -------------------------------------------------------------------------------------------------
// DepthBuffer::new (:298-312): cell (round(x), round(y)) takes the minimum depth of its points.
// ImageWriter::new (:1052-1072, MAXIMUM): the point moves to (x - ox, y - oy), its depth is scaled, the rounded position is
// clamped into the map, the cell takes the maximum.
template <bool MAXIMUM>
__global__ __launch_bounds__(BLOCK) void mesh_scatter_kernel(const double4 *__restrict__ plane, unsigned long long n, uint32_t sel,
                                                             double ox, double oy, double scale, uint32_t w, uint32_t h,
                                                             unsigned long long *__restrict__ buf)
{
    for (unsigned long long i = (unsigned long long)blockIdx.x * BLOCK + threadIdx.x; i < n; i += (unsigned long long)gridDim.x * BLOCK) {
        const double4 v = plane[i];
        if (((uint32_t)v.w & sel) != sel) continue;
        if (MAXIMUM) {
            const unsigned long long x = round_usize(v.x - ox, w - 1), y = round_usize(v.y - oy, h - 1);
            atomicMax(&buf[y * w + x], key_of(v.z * scale));
        } else {
            const unsigned long long x = round_usize(v.x, w), y = round_usize(v.y, h);
            if (x < w && y < h) atomicMin(&buf[y * w + x], key_of(v.z)); // (always: w = ceil(max x) + 1)
        }
    }
}

// ---- the scanline walk of ProjectedPolygon (:107-254), quirks included ---------------------------------------------------------
struct Tri {
    double x[3], y[3], v[3]; // a, b, c: stably sorted by y with total_cmp (:116)
};

__device__ __forceinline__ long long total_key(double d)
{
    long long b = __double_as_longlong(d);
    return b ^ (long long)((unsigned long long)(b >> 63) >> 1);
}

__device__ __forceinline__ void tri_swap(Tri &t, int i, int j)
{
    double a;
    a = t.x[i], t.x[i] = t.x[j], t.x[j] = a;
    a = t.y[i], t.y[i] = t.y[j], t.y[j] = a;
    a = t.v[i], t.v[i] = t.v[j], t.v[j] = a;
}

__device__ __forceinline__ void tri_sort(Tri &t)
{
    if (total_key(t.y[1]) < total_key(t.y[0])) tri_swap(t, 0, 1);
    if (total_key(t.y[2]) < total_key(t.y[1])) {
        tri_swap(t, 1, 2);
        if (total_key(t.y[1]) < total_key(t.y[0])) tri_swap(t, 0, 1);
    }
}

struct Scanline {
    double start_x, end_x, start_v, end_v;
    uint32_t x0, x1;
};

// update_scanline (:168-223); false = the row is skipped
__device__ __forceinline__ bool scanline(const Tri &t, uint32_t yi, uint32_t max_x, Scanline &s)
{
    const double y = (double)yi;
    if (y < t.y[0] || y > t.y[2]) return false;
    double sx, sv;
    if (y < t.y[1] || fabs((t.y[1] - t.y[2]) / (t.x[1] - t.x[2])) < F64_EPS) {
        const double k = (y - t.y[0]) / (t.y[1] - t.y[0]);
        sx = t.x[0] * (1.0 - k) + t.x[1] * k;
        sv = t.v[0] * (1.0 - k) + t.v[1] * k;
    } else {
        const double k = (y - t.y[1]) / (t.y[2] - t.y[1]);
        sx = t.x[1] * (1.0 - k) + t.x[2] * k;
        sv = t.v[1] * (1.0 - k) + t.v[2] * k;
    }
    const double k = (y - t.y[0]) / (t.y[2] - t.y[0]);
    const double ex = t.x[0] * (1.0 - k) + t.x[2] * k;
    const double ev = t.v[0] * (1.0 - k) + t.v[2] * k;
    if (sx < ex)
        s.start_x = sx, s.end_x = ex, s.start_v = sv, s.end_v = ev;
    else
        s.start_x = ex, s.end_x = sx, s.start_v = ev, s.end_v = sv;
    s.x0 = clamp_usize(floor(s.start_x), max_x);
    s.x1 = clamp_usize(ceil(s.end_x + 1.0), max_x);
    return true;
}

// scanline_value (:225-232)
__device__ __forceinline__ bool scanline_value(const Scanline &s, uint32_t xi, double &value)
{
    const double xc = ((double)xi - s.start_x) / (s.end_x - s.start_x);
    if (!(0.0 <= xc && xc <= 1.0)) return false;
    value = s.start_v * (1.0 - xc) + xc * s.end_v;
    return true;
}

__device__ __forceinline__ void row_bounds(const Tri &t, uint32_t max_y, uint32_t &y0, uint32_t &y1)
{
    y0 = clamp_usize(floor(t.y[0]), max_y);
    y1 = clamp_usize(ceil(t.y[2] + 1.0), max_y);
}

// rows x columns of the polygon's bounding box inside the grid: what decides between the lane walk and the wave walk
__device__ __forceinline__ unsigned long long box_pixels(const Tri &t, uint32_t max_x, uint32_t max_y)
{
    uint32_t y0, y1;
    row_bounds(t, max_y, y0, y1);
    // (a vertex at infinity or NaN: the rows' ends are what the formulas give - count whole rows)
    const bool finite = isfinite(t.x[0]) && isfinite(t.x[1]) && isfinite(t.x[2]);
    const uint32_t x0 = finite ? clamp_usize(floor(fmin(fmin(t.x[0], t.x[1]), t.x[2])), max_x) : 0u;
    const uint32_t x1 = finite ? clamp_usize(ceil(fmax(fmax(t.x[0], t.x[1]), t.x[2]) + 1.0), max_x) : max_x;
    return (unsigned long long)(y1 > y0 ? y1 - y0 : 0) * (x1 > x0 ? x1 - x0 : 0);
}

__device__ __forceinline__ bool goes_wide(unsigned long long pixels, uint32_t threshold)
{
    return threshold != 0xFFFFFFFFu && pixels >= threshold;
}

// polygon_obstructs' test of one emitted pixel (:345-352)
__device__ __forceinline__ bool cell_hit(const unsigned long long *__restrict__ buf, uint32_t w, uint32_t x, uint32_t y, double depth)
{
    const unsigned long long c = buf[(size_t)y * w + x];
    return c != KEY_NONE_MIN && value_of(c) - depth > F64_EPS;
}

__device__ __forceinline__ Tri load_tri(const double4 *__restrict__ plane, const uint32_t *__restrict__ poly, bool &all_range)
{
    Tri t;
    all_range = true;
    for (int k = 0; k < 3; k++) {
        const double4 v = plane[poly[k]];
        t.x[k] = v.x, t.y[k] = v.y, t.v[k] = v.z;
        all_range = all_range && ((uint32_t)v.w & FLAG_RANGE);
    }
    return t;
}

// ---- cull -----------------------------------------------------------------------------------------------------------------------
// counters: [0] polygons that obstruct in this camera, [1] queue length (polygons sent to the wave path)
__global__ __launch_bounds__(BLOCK) void mesh_cull_kernel(const double4 *__restrict__ plane, const uint32_t *__restrict__ polygons,
                                                          unsigned long long n_poly, const unsigned long long *__restrict__ buf,
                                                          uint32_t w, uint32_t h, uint32_t threshold, uint8_t *__restrict__ keep,
                                                          uint32_t *__restrict__ queue, uint32_t *__restrict__ counters)
{
    uint32_t dropped = 0;
    for (unsigned long long p = (unsigned long long)blockIdx.x * BLOCK + threadIdx.x; p < n_poly; p += (unsigned long long)gridDim.x * BLOCK) {
        bool in_range;
        Tri t = load_tri(plane, polygons + 3 * p, in_range);
        tri_sort(t);
        if (goes_wide(box_pixels(t, w, h), threshold)) {
            queue[atomicAdd(&counters[1], 1u)] = (uint32_t)p;
            continue;
        }
        uint32_t y0, y1;
        row_bounds(t, h, y0, y1);
        bool hit = false;
        for (uint32_t y = y0; y < y1 && !hit; y++) {
            Scanline s;
            if (!scanline(t, y, w, s)) continue;
            for (uint32_t x = s.x0; x < s.x1; x++) {
                double depth;
                if (scanline_value(s, x, depth) && cell_hit(buf, w, x, y, depth)) {
                    hit = true;
                    break;
                }
            }
        }
        if (hit) keep[p] = 0, dropped++;
    }
    if (dropped) atomicAdd(&counters[0], dropped);
}

// one wave per queued polygon: its lanes take consecutive x of a row, a ballot ends the wave at the first hit
__global__ __launch_bounds__(BLOCK) void mesh_cull_wide_kernel(const double4 *__restrict__ plane, const uint32_t *__restrict__ polygons,
                                                               const unsigned long long *__restrict__ buf, uint32_t w, uint32_t h,
                                                               uint8_t *__restrict__ keep, const uint32_t *__restrict__ queue,
                                                               uint32_t *__restrict__ counters)
{
    const uint32_t lane = threadIdx.x & 63u, waves = gridDim.x * (BLOCK / 64), n_queue = counters[1];
    for (uint32_t q = blockIdx.x * (BLOCK / 64) + (threadIdx.x >> 6); q < n_queue; q += waves) {
        const uint32_t p = queue[q];
        bool in_range;
        Tri t = load_tri(plane, polygons + 3 * (size_t)p, in_range);
        tri_sort(t);
        uint32_t y0, y1;
        row_bounds(t, h, y0, y1);
        bool hit = false;
        for (uint32_t y = y0; y < y1 && !hit; y++) {
            Scanline s;
            if (!scanline(t, y, w, s)) continue;
            for (uint32_t xb = s.x0; xb < s.x1 && !hit; xb += 64) {
                const uint32_t x = xb + lane; // (x1 <= w <= 2^32 - 2: the sum can wrap only past x1 - see the test below)
                double depth;
                const bool mine = x >= xb && x < s.x1 && scanline_value(s, x, depth) && cell_hit(buf, w, x, y, depth);
                hit = __ballot(mine) != 0ull;
            }
        }
        if (hit && lane == 0) {
            keep[p] = 0;
            atomicAdd(&counters[0], 1u);
        }
    }
}

// ---- depth-image raster (ImageWriter::output_face, :1088-1115) ------------------------------------------------------------------
// A polygon is drawn iff its three vertices are in range (`Some` in point_projections); each emitted pixel takes the maximum.
__device__ __forceinline__ Tri place_tri(Tri t, double ox, double oy, double scale)
{
    for (int k = 0; k < 3; k++) t.x[k] = t.x[k] - ox, t.y[k] = t.y[k] - oy, t.v[k] = t.v[k] * scale;
    return t;
}

__global__ __launch_bounds__(BLOCK) void mesh_raster_kernel(const double4 *__restrict__ plane, const uint32_t *__restrict__ polygons,
                                                            unsigned long long n_poly, double ox, double oy, double scale, uint32_t w,
                                                            uint32_t h, uint32_t threshold, unsigned long long *__restrict__ map,
                                                            uint32_t *__restrict__ queue, uint32_t *__restrict__ counters)
{
    for (unsigned long long p = (unsigned long long)blockIdx.x * BLOCK + threadIdx.x; p < n_poly; p += (unsigned long long)gridDim.x * BLOCK) {
        bool in_range;
        Tri t = load_tri(plane, polygons + 3 * p, in_range);
        if (!in_range) continue;
        t = place_tri(t, ox, oy, scale);
        tri_sort(t);
        if (goes_wide(box_pixels(t, w - 1, h - 1), threshold)) {
            queue[atomicAdd(&counters[1], 1u)] = (uint32_t)p;
            continue;
        }
        uint32_t y0, y1;
        row_bounds(t, h - 1, y0, y1);
        for (uint32_t y = y0; y < y1; y++) {
            Scanline s;
            if (!scanline(t, y, w - 1, s)) continue;
            for (uint32_t x = s.x0; x < s.x1; x++) {
                double depth;
                if (scanline_value(s, x, depth)) atomicMax(&map[(size_t)y * w + x], key_of(depth));
            }
        }
    }
}

__global__ __launch_bounds__(BLOCK) void mesh_raster_wide_kernel(const double4 *__restrict__ plane, const uint32_t *__restrict__ polygons,
                                                                 double ox, double oy, double scale, uint32_t w, uint32_t h,
                                                                 unsigned long long *__restrict__ map, const uint32_t *__restrict__ queue,
                                                                 const uint32_t *__restrict__ counters)
{
    const uint32_t lane = threadIdx.x & 63u, waves = gridDim.x * (BLOCK / 64), n_queue = counters[1];
    for (uint32_t q = blockIdx.x * (BLOCK / 64) + (threadIdx.x >> 6); q < n_queue; q += waves) {
        bool in_range;
        Tri t = load_tri(plane, polygons + 3 * (size_t)queue[q], in_range);
        t = place_tri(t, ox, oy, scale);
        tri_sort(t);
        uint32_t y0, y1;
        row_bounds(t, h - 1, y0, y1);
        for (uint32_t y = y0; y < y1; y++) {
            Scanline s;
            if (!scanline(t, y, w - 1, s)) continue;
            for (uint32_t xb = s.x0; xb < s.x1; xb += 64) {
                const uint32_t x = xb + lane;
                double depth;
                if (x >= xb && x < s.x1 && scanline_value(s, x, depth)) atomicMax(&map[(size_t)y * w + x], key_of(depth));
            }
        }
    }
}

// ---- reading a buffer back ----------------------------------------------------------------------------------------------------
// out[i] = the cell's depth, NaN where it is empty; partial[block] = (min, max, ., ., occupied cells) in a fixed order
__global__ __launch_bounds__(BLOCK) void mesh_decode_kernel(const unsigned long long *__restrict__ buf, unsigned long long cells,
                                                            unsigned long long none, double *__restrict__ out, Extent *__restrict__ partial)
{
    __shared__ double s_v[2][BLOCK];
    __shared__ unsigned long long s_n[BLOCK];
    double mn = INFINITY, mx = -INFINITY;
    unsigned long long cnt = 0;
    for (unsigned long long i = (unsigned long long)blockIdx.x * BLOCK + threadIdx.x; i < cells; i += (unsigned long long)gridDim.x * BLOCK) {
        const unsigned long long k = buf[i];
        const double v = k == none ? NAN : value_of(k);
        if (out) out[i] = v;
        if (k != none) mn = fmin(mn, v), mx = fmax(mx, v), cnt++;
    }
    const int t = threadIdx.x;
    s_v[0][t] = mn, s_v[1][t] = mx, s_n[t] = cnt;
    __syncthreads();
    for (int w = BLOCK / 2; w > 0; w >>= 1) {
        if (t < w) s_v[0][t] = fmin(s_v[0][t], s_v[0][t + w]), s_v[1][t] = fmax(s_v[1][t], s_v[1][t + w]), s_n[t] += s_n[t + w];
        __syncthreads();
    }
    if (t == 0) partial[blockIdx.x] = Extent{s_v[0][0], s_v[1][0], INFINITY, -INFINITY, s_n[0]};
}

// ---- camera points: the selected tracks in track order ------------------------------------------------------------------------
__global__ __launch_bounds__(BLOCK) void mesh_select_count_kernel(const double4 *__restrict__ plane, unsigned long long n, uint32_t sel,
                                                                  uint32_t *__restrict__ block_counts)
{
    const unsigned long long i = (unsigned long long)blockIdx.x * BLOCK + threadIdx.x;
    const bool on = i < n && ((uint32_t)plane[i].w & sel) == sel;
    const uint32_t c = __syncthreads_count(on);
    if (threadIdx.x == 0) block_counts[blockIdx.x] = c;
}

__global__ __launch_bounds__(BLOCK) void mesh_select_write_kernel(const double4 *__restrict__ plane, unsigned long long n, uint32_t sel,
                                                                  const uint32_t *__restrict__ block_offsets, unsigned long long cap,
                                                                  uint32_t *__restrict__ out_index, double *__restrict__ out_xy)
{
    __shared__ uint32_t s_wave[BLOCK / 64];
    const unsigned long long i = (unsigned long long)blockIdx.x * BLOCK + threadIdx.x;
    const double4 v = i < n ? plane[i] : make_double4(0.0, 0.0, 0.0, 0.0);
    const bool on = i < n && ((uint32_t)v.w & sel) == sel;
    const unsigned long long mask = __ballot(on);
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    if (lane == 0) s_wave[wave] = (uint32_t)__popcll(mask);
    __syncthreads();
    uint32_t before = 0;
    for (uint32_t k = 0; k < wave; k++) before += s_wave[k];
    if (!on) return;
    const unsigned long long at = (unsigned long long)block_offsets[blockIdx.x] + before + __popcll(mask & ((1ull << lane) - 1ull));
    if (at >= cap) return;
    out_index[at] = (uint32_t)i;
    out_xy[2 * at] = v.x, out_xy[2 * at + 1] = v.y;
}

// polygons with a vertex >= n: counted (nothing else runs when there is one)
__global__ __launch_bounds__(BLOCK) void mesh_check_polygons_kernel(const uint32_t *__restrict__ polygons, unsigned long long n_poly,
                                                                    unsigned long long n, uint32_t *__restrict__ bad)
{
    uint32_t mine = 0;
    for (unsigned long long p = (unsigned long long)blockIdx.x * BLOCK + threadIdx.x; p < n_poly; p += (unsigned long long)gridDim.x * BLOCK)
        if (polygons[3 * p] >= n || polygons[3 * p + 1] >= n || polygons[3 * p + 2] >= n) mine = 1;
    if (mine) atomicOr(bad, 1u);
}

// ---- host side ------------------------------------------------------------------------------------------------------------------
} // namespace

void launch_mesh_check_polygons(const uint32_t *polygons, unsigned long long n_poly, unsigned long long n, uint32_t *bad, hipStream_t s)
{
    hipLaunchKernelGGL(mesh_check_polygons_kernel, dim3(grid_for(n_poly)), dim3(BLOCK), 0, s, polygons, n_poly, n, bad);
}

namespace {

// the surface as every entry point takes it, checked and staged on the device
struct SurfaceArgs {
    const double *points;
    const int32_t *tracks;
    uint64_t n;
    uint32_t m;
    const double *projection, *r, *t;
    const uint32_t *image_dims;
};

struct DeviceSurface {
    const double *points = nullptr;
    const int2 *tracks = nullptr;
    double4 *plane = nullptr;
    Extent *partial = nullptr, *extent = nullptr;
    uint32_t blocks = 1;
};

int check_surface(const char *what, cvhip_device *dev, const SurfaceArgs &a, uint32_t camera)
{
    const std::string w(what);
    if (!dev || !a.projection || !a.r || !a.t || !a.image_dims || (a.n && (!a.points || !a.tracks)))
        return fail(CVHIP_ERR_INVALID, w + ": null argument");
    if (a.m == 0) return fail(CVHIP_ERR_INVALID, w + ": no cameras (an affine surface has no mesh culling and no depth image)");
    if (a.m > CVHIP_TRIANGULATE_MAX_CAMERAS) return fail(CVHIP_ERR_UNSUPPORTED, w + ": more than CVHIP_TRIANGULATE_MAX_CAMERAS cameras");
    if (camera >= a.m) return fail(CVHIP_ERR_INVALID, w + ": camera index >= m");
    if (a.n >= 0xFFFFFFFFull) return fail(CVHIP_ERR_UNSUPPORTED, w + ": 2^32 - 1 or more tracks");
    return CVHIP_OK;
}

MeshCam make_cam(const SurfaceArgs &a, uint32_t j)
{
    MeshCam c;
    for (int k = 0; k < 12; k++) c.P[k] = a.projection[12 * j + k];
    double R[9];
    matrix_r(a.r + 3 * j, R);
    const double *t = a.t + 3 * j;
    for (int k = 0; k < 3; k++) {
        c.Rtt[k] = R[k] * t[0] + R[3 + k] * t[1] + R[6 + k] * t[2]; // r_matrix.tr_mul(t)
        c.R2[k] = R[6 + k];
    }
    for (int k = 0; k < 2; k++) { // img_range (:613-624), MAX_CENTER_DISTANCE = 4
        const double size = (double)a.image_dims[2 * j + k], centre = size / 2.0;
        c.lo[k] = centre - size * 4.0;
        c.hi[k] = centre + size * 4.0;
    }
    return c;
}

hipError_t stage_surface(CallScratch &sc, const SurfaceArgs &a, DeviceSurface &d, hipStream_t s)
{
    const int32_t *tr = nullptr;
    hipError_t e = sc.input(a.points, (size_t)a.n * 3, &d.points, s);
    if (e == hipSuccess) e = sc.input(a.tracks, (size_t)a.n * a.m * 2, &tr, s);
    d.tracks = reinterpret_cast<const int2 *>(tr);
    d.blocks = grid_for(a.n);
    if (e == hipSuccess) e = sc.alloc(&d.plane, (size_t)a.n);
    if (e == hipSuccess) e = sc.alloc(&d.partial, (size_t)MAX_GRID);
    if (e == hipSuccess) e = sc.alloc(&d.extent, 1);
    return e;
}

// project every track into camera j and read the extent of the tracks selected by `sel` back (one synchronisation)
hipError_t project(const SurfaceArgs &a, const DeviceSurface &d, uint32_t j, uint32_t sel, Extent *h_extent, hipStream_t s)
{
    hipLaunchKernelGGL(mesh_project_kernel, dim3(d.blocks), dim3(BLOCK), 0, s, d.points, d.tracks, (unsigned long long)a.n, a.m, j,
                       make_cam(a, j), sel, d.plane, d.partial);
    hipLaunchKernelGGL(extent_final_kernel, dim3(1), dim3(64), 0, s, d.partial, d.blocks, d.extent);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipMemcpyAsync(h_extent, d.extent, sizeof(Extent), hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    return e;
}

// DepthBuffer::new's grid (:285-299): (ceil(max_x) + 1) x (ceil(max_y) + 1), 0 x 0 without points
void buffer_dims(const Extent &e, uint64_t *w, uint64_t *h)
{
    *w = *h = 0;
    if (!e.count) return;
    *w = (uint64_t)std::max(0.0, std::ceil(e.max_x)) + 1;
    *h = (uint64_t)std::max(0.0, std::ceil(e.max_y)) + 1;
}

// the minimum buffer of camera j from the projected plane
hipError_t build_buffer(CallScratch &sc, const SurfaceArgs &a, const DeviceSurface &d, uint32_t w, uint32_t h, unsigned long long **buf,
                        hipStream_t s)
{
    const unsigned long long cells = (unsigned long long)w * h;
    hipError_t e = sc.alloc(buf, (size_t)cells);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(fill_u64_kernel, dim3(grid_for(cells)), dim3(BLOCK), 0, s, *buf, KEY_NONE_MIN, cells);
    hipLaunchKernelGGL((mesh_scatter_kernel<false>), dim3(d.blocks), dim3(BLOCK), 0, s, d.plane, (unsigned long long)a.n,
                       FLAG_RANGE | FLAG_SEEN, 0.0, 0.0, 1.0, w, h, *buf);
    return hipGetLastError();
}

// decode a buffer into `out` (host or device, may be NULL) and fold (min, max, occupied) into *h_stats
hipError_t decode(CallScratch &sc, const DeviceSurface &d, const unsigned long long *buf, unsigned long long cells, unsigned long long none,
                  double *out, Extent *h_stats, hipStream_t s)
{
    double *d_out = nullptr;
    hipError_t e = sc.output(out, (size_t)cells, &d_out);
    if (e != hipSuccess) return e;
    const uint32_t blocks = grid_for(cells);
    hipLaunchKernelGGL(mesh_decode_kernel, dim3(blocks), dim3(BLOCK), 0, s, buf, cells, none, d_out, d.partial);
    hipLaunchKernelGGL(extent_final_kernel, dim3(1), dim3(64), 0, s, d.partial, blocks, d.extent);
    e = hipGetLastError();
    if (e == hipSuccess) e = hipMemcpyAsync(h_stats, d.extent, sizeof(Extent), hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = sc.copy_out(out, d_out, (size_t)cells, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    return e;
}

} // namespace
} // namespace cvhip

using namespace cvhip;

extern "C" int cvhip_mesh_set_wide_threshold(cvhip_device *dev, uint32_t pixels)
{
    if (!dev) return fail(CVHIP_ERR_INVALID, "cvhip_mesh_set_wide_threshold: null device");
    dev->d.mesh_wide_threshold = pixels;
    return CVHIP_OK;
}

extern "C" int cvhip_mesh_camera_points(cvhip_device *dev, const double *points, const int32_t *tracks, uint64_t n, uint32_t m,
                                        const double *projection, const double *r, const double *t, const uint32_t *image_dims,
                                        uint32_t camera_i, uint32_t *out_index, double *out_xy, uint64_t cap, uint64_t *out_n)
{
    const SurfaceArgs a{points, tracks, n, m, projection, r, t, image_dims};
    CVHIP_TRY(check_surface("mesh_camera_points", dev, a, camera_i));
    if (!out_n || (cap && (!out_index || !out_xy))) return fail(CVHIP_ERR_INVALID, "mesh_camera_points: null output");
    CVHIP_TRY_HIP(hipSetDevice(dev->d.ordinal));
    hipStream_t s = dev->d.stream;
    CallScratch sc;
    DeviceSurface d;
    Extent ext{};
    hipError_t e = stage_surface(sc, a, d, s);
    if (e == hipSuccess) e = project(a, d, camera_i, FLAG_RANGE | FLAG_SEEN, &ext, s);
    if (e != hipSuccess) return device_error("mesh_camera_points", e);
    *out_n = ext.count;
    const uint64_t k = std::min<uint64_t>(cap, ext.count);
    if (!k) return CVHIP_OK;
    // one block per 256 consecutive tracks (not a grid-stride loop: the blocks' counts are scanned into their offsets)
    const uint32_t blocks = (uint32_t)((n + BLOCK - 1) / BLOCK);
    uint32_t *counts = nullptr, *d_index = nullptr;
    double *d_xy = nullptr;
    e = sc.alloc(&counts, (size_t)blocks + 1);
    if (e == hipSuccess) e = sc.output(out_index, (size_t)k, &d_index);
    if (e == hipSuccess) e = sc.output(out_xy, (size_t)k * 2, &d_xy);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(mesh_select_count_kernel, dim3(blocks), dim3(BLOCK), 0, s, d.plane, (unsigned long long)n, FLAG_RANGE | FLAG_SEEN, counts);
        launch_scan_u32(counts, blocks, counts + blocks, s);
        hipLaunchKernelGGL(mesh_select_write_kernel, dim3(blocks), dim3(BLOCK), 0, s, d.plane, (unsigned long long)n, FLAG_RANGE | FLAG_SEEN,
                           counts, (unsigned long long)k, d_index, d_xy);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = sc.copy_out(out_index, d_index, (size_t)k, s);
    if (e == hipSuccess) e = sc.copy_out(out_xy, d_xy, (size_t)k * 2, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) return device_error("mesh_camera_points", e);
    return CVHIP_OK;
}

extern "C" int cvhip_mesh_depth_buffer(cvhip_device *dev, const double *points, const int32_t *tracks, uint64_t n, uint32_t m,
                                       const double *projection, const double *r, const double *t, const uint32_t *image_dims,
                                       uint32_t camera_j, double *out_buffer, uint64_t cap_cells, uint64_t *out_width,
                                       uint64_t *out_height)
{
    const SurfaceArgs a{points, tracks, n, m, projection, r, t, image_dims};
    CVHIP_TRY(check_surface("mesh_depth_buffer", dev, a, camera_j));
    if (!out_width || !out_height || (cap_cells && !out_buffer)) return fail(CVHIP_ERR_INVALID, "mesh_depth_buffer: null output");
    CVHIP_TRY_HIP(hipSetDevice(dev->d.ordinal));
    hipStream_t s = dev->d.stream;
    CallScratch sc;
    DeviceSurface d;
    Extent ext{};
    hipError_t e = stage_surface(sc, a, d, s);
    if (e == hipSuccess) e = project(a, d, camera_j, FLAG_RANGE | FLAG_SEEN, &ext, s);
    if (e != hipSuccess) return device_error("mesh_depth_buffer", e);
    uint64_t w, h;
    buffer_dims(ext, &w, &h);
    if (w * h >= 0xFFFFFFFFull) return fail(CVHIP_ERR_UNSUPPORTED, "mesh_depth_buffer: 2^32 - 1 or more cells");
    *out_width = w, *out_height = h;
    if (!cap_cells || !(w * h)) return CVHIP_OK;
    if (cap_cells < w * h) return fail(CVHIP_ERR_INVALID, "mesh_depth_buffer: the buffer is smaller than width x height");
    unsigned long long *buf = nullptr;
    Extent stats{};
    e = build_buffer(sc, a, d, (uint32_t)w, (uint32_t)h, &buf, s);
    if (e == hipSuccess) e = decode(sc, d, buf, w * h, KEY_NONE_MIN, out_buffer, &stats, s);
    if (e != hipSuccess) return device_error("mesh_depth_buffer", e);
    return CVHIP_OK;
}

extern "C" int cvhip_mesh_cull(cvhip_device *dev, const double *points, const int32_t *tracks, uint64_t n, uint32_t m,
                               const double *projection, const double *r, const double *t, const uint32_t *image_dims,
                               uint32_t camera_i, const uint32_t *polygons, uint64_t n_poly, uint8_t *out_keep, uint64_t *out_stats)
{
    const SurfaceArgs a{points, tracks, n, m, projection, r, t, image_dims};
    CVHIP_TRY(check_surface("mesh_cull", dev, a, camera_i));
    if (n_poly && (!polygons || !out_keep)) return fail(CVHIP_ERR_INVALID, "mesh_cull: null argument");
    if (n_poly >= 0xFFFFFFFFull) return fail(CVHIP_ERR_UNSUPPORTED, "mesh_cull: 2^32 - 1 or more polygons");
    CVHIP_TRY_HIP(hipSetDevice(dev->d.ordinal));
    hipStream_t s = dev->d.stream;
    CallScratch sc;
    DeviceSurface d;
    const uint32_t *d_poly = nullptr;
    uint32_t *queue = nullptr, *counters = nullptr; // counters: per camera {obstructing, queued}, then the bad-vertex flag
    uint8_t *d_keep = nullptr;
    const uint32_t pblocks = grid_for(n_poly), threshold = dev->d.mesh_wide_threshold;
    uint32_t h_counters[2 * CVHIP_TRIANGULATE_MAX_CAMERAS + 1] = {};
    uint64_t stats[CVHIP_TRIANGULATE_MAX_CAMERAS][5] = {};
    hipError_t e = stage_surface(sc, a, d, s);
    if (e == hipSuccess) e = sc.input(polygons, (size_t)n_poly * 3, &d_poly, s);
    if (e == hipSuccess) e = sc.alloc(&queue, (size_t)n_poly);
    if (e == hipSuccess) e = sc.alloc(&counters, 2 * (size_t)m + 1);
    if (e == hipSuccess) e = sc.output(out_keep, (size_t)n_poly, &d_keep);
    if (e == hipSuccess) e = hipMemsetAsync(counters, 0, (2 * (size_t)m + 1) * sizeof(uint32_t), s);
    if (e == hipSuccess && n_poly) {
        hipLaunchKernelGGL(mesh_check_polygons_kernel, dim3(pblocks), dim3(BLOCK), 0, s, d_poly, (unsigned long long)n_poly,
                           (unsigned long long)n, counters + 2 * m);
        e = hipGetLastError();
        if (e == hipSuccess) e = hipMemcpyAsync(h_counters + 2 * m, counters + 2 * m, sizeof(uint32_t), hipMemcpyDeviceToHost, s);
        if (e == hipSuccess) e = hipStreamSynchronize(s);
    }
    if (e != hipSuccess) return device_error("mesh_cull", e);
    if (h_counters[2 * m]) return fail(CVHIP_ERR_INVALID, "mesh_cull: a polygon names a track >= n");
    if (n_poly) e = hipMemsetAsync(d_keep, 1, (size_t)n_poly, s);
    for (uint32_t j = 0; j < m && e == hipSuccess; j++) {
        if (j == camera_i) continue;
        Extent ext{}, occ{};
        e = project(a, d, j, FLAG_RANGE | FLAG_SEEN, &ext, s);
        if (e != hipSuccess) break;
        uint64_t w, h;
        buffer_dims(ext, &w, &h);
        if (w * h >= 0xFFFFFFFFull) return fail(CVHIP_ERR_UNSUPPORTED, "mesh_cull: 2^32 - 1 or more cells");
        stats[j][0] = w, stats[j][1] = h;
        if (!(w * h)) continue; // a 0 x 0 buffer: nothing obstructs (:292-296)
        unsigned long long *buf = nullptr;
        e = build_buffer(sc, a, d, (uint32_t)w, (uint32_t)h, &buf, s);
        if (e == hipSuccess && n_poly) {
            hipLaunchKernelGGL(mesh_cull_kernel, dim3(pblocks), dim3(BLOCK), 0, s, d.plane, d_poly, (unsigned long long)n_poly, buf,
                               (uint32_t)w, (uint32_t)h, threshold, d_keep, queue, counters + 2 * j);
            hipLaunchKernelGGL(mesh_cull_wide_kernel, dim3(MAX_GRID), dim3(BLOCK), 0, s, d.plane, d_poly, buf, (uint32_t)w, (uint32_t)h,
                               d_keep, queue, counters + 2 * j);
            e = hipGetLastError();
        }
        if (e == hipSuccess) e = decode(sc, d, buf, w * h, KEY_NONE_MIN, nullptr, &occ, s); // (synchronises: buf can go)
        stats[j][2] = occ.count;
        sc.release(buf); // before the next camera's
    }
    if (e == hipSuccess) e = hipMemcpyAsync(h_counters, counters, 2 * (size_t)m * sizeof(uint32_t), hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = sc.copy_out(out_keep, d_keep, (size_t)n_poly, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) return device_error("mesh_cull", e);
    if (out_stats)
        for (uint32_t j = 0; j < m; j++) {
            stats[j][3] = h_counters[2 * j], stats[j][4] = h_counters[2 * j + 1];
            std::memcpy(out_stats + 5 * j, stats[j], sizeof(stats[j]));
        }
    return CVHIP_OK;
}

extern "C" int cvhip_mesh_depth_image(cvhip_device *dev, const double *points, const int32_t *tracks, uint64_t n, uint32_t m,
                                      const double *projection, const double *r, const double *t, const uint32_t *image_dims,
                                      uint32_t project_to_image, double scale, const uint32_t *polygons, uint64_t n_poly,
                                      double *out_map, uint64_t cap_cells, uint64_t *out_width, uint64_t *out_height,
                                      double *out_origin, double *out_minmax, uint64_t *out_wide)
{
    const SurfaceArgs a{points, tracks, n, m, projection, r, t, image_dims};
    CVHIP_TRY(check_surface("mesh_depth_image", dev, a, project_to_image));
    if (!out_width || !out_height || (cap_cells && !out_map) || (n_poly && !polygons))
        return fail(CVHIP_ERR_INVALID, "mesh_depth_image: null argument");
    if (n_poly >= 0xFFFFFFFFull) return fail(CVHIP_ERR_UNSUPPORTED, "mesh_depth_image: 2^32 - 1 or more polygons");
    CVHIP_TRY_HIP(hipSetDevice(dev->d.ordinal));
    hipStream_t s = dev->d.stream;
    CallScratch sc;
    DeviceSurface d;
    Extent ext{};
    hipError_t e = stage_surface(sc, a, d, s);
    if (e == hipSuccess) e = project(a, d, project_to_image, FLAG_RANGE, &ext, s); // visibility is not required (:1025-1037)
    if (e != hipSuccess) return device_error("mesh_depth_image", e);
    if (!ext.count) return fail(CVHIP_ERR_NO_SURFACE, "No point projections found"); // :1046
    const uint64_t w = (uint64_t)(std::ceil(ext.max_x) - std::floor(ext.min_x)) + 1; // :1048-1049
    const uint64_t h = (uint64_t)(std::ceil(ext.max_y) - std::floor(ext.min_y)) + 1;
    if (w * h >= 0xFFFFFFFFull) return fail(CVHIP_ERR_UNSUPPORTED, "mesh_depth_image: 2^32 - 1 or more cells");
    *out_width = w, *out_height = h;
    if (out_origin) out_origin[0] = ext.min_x, out_origin[1] = ext.min_y;
    if (!cap_cells) return CVHIP_OK;
    if (cap_cells < w * h) return fail(CVHIP_ERR_INVALID, "mesh_depth_image: the map is smaller than width x height");
    const uint32_t *d_poly = nullptr;
    uint32_t *queue = nullptr, *counters = nullptr;
    unsigned long long *map = nullptr;
    uint32_t h_counters[3] = {};
    const uint32_t pblocks = grid_for(n_poly), threshold = dev->d.mesh_wide_threshold;
    e = sc.input(polygons, (size_t)n_poly * 3, &d_poly, s);
    if (e == hipSuccess) e = sc.alloc(&queue, (size_t)n_poly);
    if (e == hipSuccess) e = sc.alloc(&counters, 3);
    if (e == hipSuccess) e = sc.alloc(&map, (size_t)(w * h));
    if (e == hipSuccess) e = hipMemsetAsync(counters, 0, 3 * sizeof(uint32_t), s);
    if (e == hipSuccess && n_poly) {
        hipLaunchKernelGGL(mesh_check_polygons_kernel, dim3(pblocks), dim3(BLOCK), 0, s, d_poly, (unsigned long long)n_poly,
                           (unsigned long long)n, counters + 2);
        e = hipGetLastError();
        if (e == hipSuccess) e = hipMemcpyAsync(h_counters + 2, counters + 2, sizeof(uint32_t), hipMemcpyDeviceToHost, s);
        if (e == hipSuccess) e = hipStreamSynchronize(s);
    }
    if (e != hipSuccess) return device_error("mesh_depth_image", e);
    if (h_counters[2]) return fail(CVHIP_ERR_INVALID, "mesh_depth_image: a polygon names a track >= n");
    Extent stats{};
    hipLaunchKernelGGL(fill_u64_kernel, dim3(grid_for(w * h)), dim3(BLOCK), 0, s, map, KEY_NONE_MAX, (unsigned long long)(w * h));
    hipLaunchKernelGGL((mesh_scatter_kernel<true>), dim3(d.blocks), dim3(BLOCK), 0, s, d.plane, (unsigned long long)n, FLAG_RANGE, ext.min_x,
                       ext.min_y, scale, (uint32_t)w, (uint32_t)h, map);
    if (n_poly) {
        hipLaunchKernelGGL(mesh_raster_kernel, dim3(pblocks), dim3(BLOCK), 0, s, d.plane, d_poly, (unsigned long long)n_poly, ext.min_x,
                           ext.min_y, scale, (uint32_t)w, (uint32_t)h, threshold, map, queue, counters);
        hipLaunchKernelGGL(mesh_raster_wide_kernel, dim3(MAX_GRID), dim3(BLOCK), 0, s, d.plane, d_poly, ext.min_x, ext.min_y, scale,
                           (uint32_t)w, (uint32_t)h, map, queue, counters);
    }
    e = hipGetLastError();
    if (e == hipSuccess) e = hipMemcpyAsync(h_counters, counters, 2 * sizeof(uint32_t), hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = decode(sc, d, map, w * h, KEY_NONE_MAX, out_map, &stats, s);
    if (e != hipSuccess) return device_error("mesh_depth_image", e);
    if (out_minmax) out_minmax[0] = stats.min_x, out_minmax[1] = stats.max_x;
    if (out_wide) *out_wide = h_counters[1];
    return CVHIP_OK;
}

// Polygon::new's rotation (:56-67), the per-camera sort + dedup by vertices (:510-516) and the final stable sort by camera
// (:384) in one pass: sort by (vertices, camera), keep the first of equal vertices - the lowest camera -, sort by camera.
// Host C++: not the hot path; its purpose is that the callers do no arithmetic.
extern "C" int cvhip_mesh_merge(cvhip_device *dev, const uint32_t *polygons, const uint32_t *camera, uint64_t n_poly,
                                uint32_t *out_polygons, uint32_t *out_camera, uint64_t *out_n)
{
    if (!dev || !out_n || (n_poly && (!polygons || !camera || !out_polygons || !out_camera)))
        return fail(CVHIP_ERR_INVALID, "mesh_merge: null argument");
    if (n_poly >= 0xFFFFFFFFull) return fail(CVHIP_ERR_UNSUPPORTED, "mesh_merge: 2^32 - 1 or more polygons");
    CVHIP_TRY_HIP(hipSetDevice(dev->d.ordinal));
    struct Poly {
        uint32_t v[3], camera;
    };
    std::vector<uint32_t> h_poly((size_t)n_poly * 3), h_cam((size_t)n_poly);
    if (n_poly) {
        CVHIP_TRY_HIP(hipStreamSynchronize(dev->d.stream));
        CVHIP_TRY_HIP(hipMemcpy(h_poly.data(), polygons, h_poly.size() * 4, hipMemcpyDefault));
        CVHIP_TRY_HIP(hipMemcpy(h_cam.data(), camera, h_cam.size() * 4, hipMemcpyDefault));
    }
    std::vector<Poly> list((size_t)n_poly);
    for (size_t i = 0; i < list.size(); i++) {
        const uint32_t *v = &h_poly[3 * i];
        Poly &p = list[i];
        p.camera = h_cam[i];
        if (v[0] < v[1] && v[0] < v[2])
            p.v[0] = v[0], p.v[1] = v[1], p.v[2] = v[2];
        else if (v[1] < v[0] && v[1] < v[2])
            p.v[0] = v[1], p.v[1] = v[2], p.v[2] = v[0];
        else
            p.v[0] = v[2], p.v[1] = v[0], p.v[2] = v[1];
    }
    auto same = [](const Poly &a, const Poly &b) { return a.v[0] == b.v[0] && a.v[1] == b.v[1] && a.v[2] == b.v[2]; };
    std::sort(list.begin(), list.end(), [](const Poly &a, const Poly &b) {
        for (int k = 0; k < 3; k++)
            if (a.v[k] != b.v[k]) return a.v[k] < b.v[k];
        return a.camera < b.camera;
    });
    list.erase(std::unique(list.begin(), list.end(), same), list.end());
    std::stable_sort(list.begin(), list.end(), [](const Poly &a, const Poly &b) { return a.camera < b.camera; });
    for (size_t i = 0; i < list.size(); i++) {
        for (int k = 0; k < 3; k++) h_poly[3 * i + k] = list[i].v[k];
        h_cam[i] = list[i].camera;
    }
    if (!list.empty()) {
        CVHIP_TRY_HIP(hipMemcpy(out_polygons, h_poly.data(), list.size() * 12, hipMemcpyDefault));
        CVHIP_TRY_HIP(hipMemcpy(out_camera, h_cam.data(), list.size() * 4, hipMemcpyDefault));
    }
    *out_n = list.size();
    return CVHIP_OK;
}
