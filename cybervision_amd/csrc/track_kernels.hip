// track_kernels.hip — the dense consumer's track extension on the device-resident forward grid.
//
// Replaces Triangulation::extend_tracks (zlogic/cybervision src/triangulation.rs:1330-1419), the first thing the
// perspective pipeline does with a finished dense correlation (triangulation.rs:638, 697): every existing track
// that has a point in image 1 looks for the nearest dense match within `search_radius` of it (squared distance,
// FIRST minimum in row-major scan order, :1362-1382) and takes that match's image-2 point; the merged points are
// then cleared from the remaining grid - at the MATCHED point's coordinates, as the reference does (:1391-1393) -
// and every remaining Some cell starts a new track, in scan order (:1397-1416).  Integer only: bit-exact.
// Also PerspectiveTriangulation::merge_tracks (:1421-1540), the pass that reconstruct_dense runs after each image's pairs.
#include "cvhip_internal.hpp"

#include <algorithm>
#include <string>
#include <vector>

namespace cvhip {

__global__ __launch_bounds__(256) void extend_tracks_match_kernel(const uint32_t *__restrict__ cells, uint32_t lw, uint32_t lh,
                                                                   uint32_t k, uint32_t gw, uint32_t gh,
                                                                   const int2 *__restrict__ track_p1, uint32_t stride,
                                                                   unsigned long long n_tracks, uint32_t radius,
                                                                   int2 *__restrict__ out_p2, uint8_t *__restrict__ removed,
                                                                   uint32_t *__restrict__ oob)
{
    const unsigned long long t = (unsigned long long)blockIdx.x * 256 + threadIdx.x;
    if (t >= n_tracks) return;
    // track t's image-1 point: a column of its own (stride 1), or column image1 of the n x m table in place (stride m)
    const int2 p = track_p1[t * stride];
    int2 res = make_int2(-1, -1);
    if (p.x >= 0 && p.y >= 0) { // track.get(image1_index)?
        const uint32_t px = (uint32_t)p.x, py = (uint32_t)p.y;
        // :1358-1361 - saturating_sub below, min(.., width/height) above: [p - r, p + r) clipped
        const uint32_t min_x = px > radius ? px - radius : 0u, min_y = py > radius ? py - radius : 0u;
        const uint32_t max_x = min(px + radius, gw), max_y = min(py + radius, gh);
        bool have = false;
        unsigned long long best = 0;
        for (uint32_t y = min_y; y < max_y; y++)
            for (uint32_t x = min_x; x < max_x; x++) {
                uint32_t mx, my;
                if (!full_res_match(cells, lw, lh, k, x, y, mx, my)) continue;
                const unsigned long long dx = x > px ? x - px : px - x, dy = y > py ? y - py : py - y;
                const unsigned long long d = dx * dx + dy * dy;
                if (!have || d < best) { // is_none_or(distance < min_distance): the first minimum wins
                    have = true;
                    best = d;
                    res = make_int2((int)mx, (int)my);
                }
            }
        if (have) {
            // :1391-1393: *remaining_points.val_mut(track_point.x, track_point.y) = None - the image-1 grid indexed
            // with the image-2 point; Grid::val_mut asserts the bounds (data.rs:61-64)
            if ((uint32_t)res.x < gw && (uint32_t)res.y < gh) removed[(size_t)res.y * gw + res.x] = 1;
            else atomicAdd(oob, 1u);
        }
    }
    out_p2[t] = res;
}

__device__ __forceinline__ bool remaining_cell(const uint32_t *__restrict__ cells, uint32_t lw, uint32_t lh, uint32_t k,
                                               uint32_t gw, uint32_t gh, const uint8_t *__restrict__ removed, size_t i,
                                               uint32_t &gx, uint32_t &gy, uint32_t &mx, uint32_t &my)
{
    if (i >= (size_t)gw * gh) return false;
    gx = (uint32_t)(i % gw);
    gy = (uint32_t)(i / gw);
    return full_res_match(cells, lw, lh, k, gx, gy, mx, my) && !removed[i];
}

__global__ __launch_bounds__(256) void extend_tracks_count_kernel(const uint32_t *__restrict__ cells, uint32_t lw, uint32_t lh,
                                                                   uint32_t k, uint32_t gw, uint32_t gh,
                                                                   const uint8_t *__restrict__ removed,
                                                                   uint32_t *__restrict__ block_counts)
{
    uint32_t gx, gy, mx, my;
    const bool f = remaining_cell(cells, lw, lh, k, gw, gh, removed, (size_t)blockIdx.x * 256 + threadIdx.x, gx, gy, mx, my);
    __shared__ uint32_t wsum[4];
    const unsigned long long b = __ballot(f);
    if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = (uint32_t)__popcll(b);
    __syncthreads();
    if (threadIdx.x == 0) block_counts[blockIdx.x] = wsum[0] + wsum[1] + wsum[2] + wsum[3];
}

__global__ __launch_bounds__(256) void extend_tracks_write_kernel(const uint32_t *__restrict__ cells, uint32_t lw, uint32_t lh,
                                                                   uint32_t k, uint32_t gw, uint32_t gh,
                                                                   const uint8_t *__restrict__ removed,
                                                                   const uint32_t *__restrict__ block_offsets,
                                                                   unsigned long long cap, uint32_t *__restrict__ out_new_p1,
                                                                   uint32_t *__restrict__ out_new_p2)
{
    uint32_t gx = 0, gy = 0, mx = 0, my = 0;
    const bool f = remaining_cell(cells, lw, lh, k, gw, gh, removed, (size_t)blockIdx.x * 256 + threadIdx.x, gx, gy, mx, my);
    __shared__ uint32_t wsum[4];
    const unsigned long long b = __ballot(f);
    const uint32_t lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    if (lane == 0) wsum[wv] = (uint32_t)__popcll(b);
    __syncthreads();
    if (f) {
        unsigned long long off = block_offsets[blockIdx.x];
        for (uint32_t w = 0; w < wv; w++) off += wsum[w];
        off += (unsigned long long)__popcll(b & ((1ull << lane) - 1ull));
        if (off < cap) {
            reinterpret_cast<uint2 *>(out_new_p1)[off] = make_uint2(gx, gy);
            reinterpret_cast<uint2 *>(out_new_p2)[off] = make_uint2(mx, my);
        }
    }
}

void launch_extend_tracks_match(const uint32_t *cells, uint32_t lw, uint32_t lh, uint32_t k, uint32_t gw, uint32_t gh,
                                const int2 *track_p1, unsigned long long n_tracks, uint32_t radius, int2 *out_p2,
                                uint8_t *removed, uint32_t *oob, hipStream_t s, uint32_t stride)
{
    if (!n_tracks) return;
    hipLaunchKernelGGL(extend_tracks_match_kernel, dim3((unsigned)((n_tracks + 255) / 256)), dim3(256), 0, s, cells, lw, lh, k,
                       gw, gh, track_p1, stride, n_tracks, radius, out_p2, removed, oob);
}

void launch_extend_tracks_new(const uint32_t *cells, uint32_t lw, uint32_t lh, uint32_t k, uint32_t gw, uint32_t gh,
                              const uint8_t *removed, uint32_t *block_counts, uint32_t *total, uint32_t *out_new_p1,
                              uint32_t *out_new_p2, unsigned long long cap, hipStream_t s)
{
    const uint32_t nblocks = (uint32_t)(((size_t)gw * gh + 255) / 256);
    hipLaunchKernelGGL(extend_tracks_count_kernel, dim3(nblocks), dim3(256), 0, s, cells, lw, lh, k, gw, gh, removed,
                       block_counts);
    launch_scan_u32(block_counts, nblocks, total, s);
    if (cap)
        hipLaunchKernelGGL(extend_tracks_write_kernel, dim3(nblocks), dim3(256), 0, s, cells, lw, lh, k, gw, gh, removed,
                           block_counts, cap, out_new_p1, out_new_p2);
}

// ---- merge_tracks (triangulation.rs:1421-1540), DESIGN.md 4.10 ---------------------------------------------------------
// The reference's AverageTrack folds start every step from a fresh vector (:523-583), so each fold returns the points of
// the LAST element it folded: the "average" of a cell is its highest row, the vertical window's is the last track of its
// bottom cell (row yhi - 1), and the area track A of cell p is last[x*, yhi - 1] with x* the highest column of
// [px - r, min(px + r, w)) that has any track in rows [py - r, yhi).  A cell is kept iff every track in it can_merge
// (:347-368) with A, and then yields a copy of its highest row; cells in row-major order.  Integer only: bit-exact.
// Counters (MergeCounters): tracks with a point in image i, occupied cells, cells whose A is empty, invalid point.
struct MergeCounters {
    uint32_t present, cells, empty_area, bad, total;
};

// the number of true `f` in a block of 256 lanes (every lane of the block calls it)
__device__ __forceinline__ uint32_t block_count_256(bool f, uint32_t *wsum)
{
    const unsigned long long b = __ballot(f);
    if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = (uint32_t)__popcll(b);
    __syncthreads();
    return wsum[0] + wsum[1] + wsum[2] + wsum[3];
}

// one lane per track: validate the row (a point is present iff x >= 0 and y >= 0; exactly one negative coordinate, or an
// image-i point outside w x h, is an error) and scatter row + 1 into its image-i cell; the highest row wins (0 = empty).
// present_part[block] = the block's tracks with a point in image i (summed by merge_tracks_sum_kernel: a counter shared
// by every wave would serialise the kernel on one address)
__global__ __launch_bounds__(256) void merge_tracks_scatter_kernel(const int2 *__restrict__ tracks, unsigned long long n, uint32_t m,
                                                                   uint32_t image_index, uint32_t w, uint32_t h,
                                                                   uint32_t *__restrict__ last, uint32_t *__restrict__ present_part,
                                                                   MergeCounters *__restrict__ cnt)
{
    const unsigned long long t = (unsigned long long)blockIdx.x * 256 + threadIdx.x;
    bool present = false;
    if (t < n) {
        const int2 *row = tracks + t * m;
        bool bad = false;
        for (uint32_t j = 0; j < m; j++) {
            const int2 p = row[j];
            bad |= (p.x < 0) != (p.y < 0);
        }
        const int2 p = row[image_index];
        if (p.x >= 0 && p.y >= 0) {
            if ((uint32_t)p.x < w && (uint32_t)p.y < h) {
                atomicMax(&last[(size_t)p.y * w + p.x], (uint32_t)t + 1u);
                present = true;
            } else {
                bad = true;
            }
        }
        if (bad) atomicOr(&cnt->bad, 1u);
    }
    __shared__ uint32_t wsum[4];
    const uint32_t c = block_count_256(present, wsum);
    if (threadIdx.x == 0) present_part[blockIdx.x] = c;
}

// column occupancy: occ[y, x] = 1 iff a cell of column x in rows [max(y - r, 0), min(y + r, h)) holds a track.  One lane
// per (column, chunk of MERGE_ROWS rows): neighbouring lanes read neighbouring cells, and the window slides down the chunk
constexpr uint32_t MERGE_ROWS = 64;
__global__ __launch_bounds__(256) void merge_tracks_column_kernel(const uint32_t *__restrict__ last, uint32_t w, uint32_t h,
                                                                  uint32_t r, uint8_t *__restrict__ occ)
{
    const size_t g = (size_t)blockIdx.x * 256 + threadIdx.x;
    const uint32_t chunks = (h + MERGE_ROWS - 1) / MERGE_ROWS;
    if (g >= (size_t)w * chunks) return;
    const uint32_t x = (uint32_t)(g % w), y0 = (uint32_t)(g / w) * MERGE_ROWS, y1 = min(y0 + MERGE_ROWS, h);
    uint32_t count = 0;
    for (uint32_t y = y0 > r ? y0 - r : 0u, hi = min(y0 + r, h); y < hi; y++) count += last[(size_t)y * w + x] != 0;
    for (uint32_t y = y0; y < y1; y++) {
        occ[(size_t)y * w + x] = count != 0;
        if (y + r < h) count += last[(size_t)(y + r) * w + x] != 0;
        if (y >= r) count -= last[(size_t)(y - r) * w + x] != 0;
    }
}

// one lane per cell: area[c] = A (row + 1 of the area track, 0 = empty) and keep[c] = occupied; per block the occupied
// cells and those whose A is empty
__global__ __launch_bounds__(256) void merge_tracks_area_kernel(const uint32_t *__restrict__ last, const uint8_t *__restrict__ occ,
                                                                uint32_t w, uint32_t h, uint32_t r, uint32_t *__restrict__ area,
                                                                uint8_t *__restrict__ keep, uint32_t *__restrict__ cells_part,
                                                                uint32_t *__restrict__ empty_part)
{
    const size_t c = (size_t)blockIdx.x * 256 + threadIdx.x;
    bool occupied = false, empty = false;
    if (c < (size_t)w * h) {
        occupied = last[c] != 0;
        keep[c] = occupied;
        if (occupied) {
            const uint32_t px = (uint32_t)(c % w), py = (uint32_t)(c / w);
            const uint32_t xlo = px > r ? px - r : 0u, xhi = min(px + r, w), yhi = min(py + r, h);
            const uint8_t *orow = occ + (size_t)py * w;
            uint32_t xs = xhi - 1;
            while (xs > xlo && !orow[xs]) xs--; // column px itself qualifies (r >= 2), so the walk ends by px
            const uint32_t a = last[(size_t)(yhi - 1) * w + xs];
            area[c] = a;
            empty = a == 0;
        }
    }
    __shared__ uint32_t wsum[8];
    const uint32_t nc = block_count_256(occupied, wsum);
    const uint32_t ne = block_count_256(empty, wsum + 4);
    if (threadIdx.x == 0) {
        cells_part[blockIdx.x] = nc;
        empty_part[blockIdx.x] = ne;
    }
}

// one block: the per-block counts of the scatter and area kernels into MergeCounters, in a fixed order
__global__ __launch_bounds__(1024) void merge_tracks_sum_kernel(const uint32_t *__restrict__ present_part, uint32_t tblocks,
                                                                const uint32_t *__restrict__ cells_part,
                                                                const uint32_t *__restrict__ empty_part, uint32_t cblocks,
                                                                MergeCounters *__restrict__ cnt)
{
    uint32_t v[3] = {0, 0, 0};
    for (uint32_t i = threadIdx.x; i < tblocks; i += 1024) v[0] += present_part[i];
    for (uint32_t i = threadIdx.x; i < cblocks; i += 1024) {
        v[1] += cells_part[i];
        v[2] += empty_part[i];
    }
    __shared__ uint32_t part[3][16];
    for (int k = 0; k < 3; k++) {
        for (int s = 32; s > 0; s >>= 1) v[k] += __shfl_down(v[k], s, 64);
        if ((threadIdx.x & 63) == 0) part[k][threadIdx.x >> 6] = v[k];
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t sum[3] = {0, 0, 0};
        for (int k = 0; k < 3; k++)
            for (int wv = 0; wv < 16; wv++) sum[k] += part[k][wv];
        cnt->present = sum[0];
        cnt->cells = sum[1];
        cnt->empty_area = sum[2];
    }
}

// one lane per track with a point in image i: can_merge with its cell's area track over the m images, or keep[c] = 0
__global__ __launch_bounds__(256) void merge_tracks_check_kernel(const int2 *__restrict__ tracks, unsigned long long n, uint32_t m,
                                                                 uint32_t image_index, uint32_t w, uint32_t h,
                                                                 unsigned long long max_distance_sqr,
                                                                 const uint32_t *__restrict__ area, uint8_t *__restrict__ keep)
{
    const unsigned long long t = (unsigned long long)blockIdx.x * 256 + threadIdx.x;
    if (t >= n) return;
    const int2 *row = tracks + t * m;
    const int2 p = row[image_index];
    if (p.x < 0 || p.y < 0 || (uint32_t)p.x >= w || (uint32_t)p.y >= h) return;
    const size_t c = (size_t)p.y * w + p.x;
    const uint32_t a = area[c];
    if (!a) return; // an empty area track has no point in any image: can_merge holds
    const int2 *arow = tracks + (unsigned long long)(a - 1) * m;
    for (uint32_t j = 0; j < m; j++) {
        const int2 p1 = row[j], p2 = arow[j];
        if (p1.x < 0 || p1.y < 0 || p2.x < 0 || p2.y < 0) continue;
        const unsigned long long dx = (unsigned long long)(p1.x > p2.x ? p1.x - p2.x : p2.x - p1.x);
        const unsigned long long dy = (unsigned long long)(p1.y > p2.y ? p1.y - p2.y : p2.y - p1.y);
        if (dx * dx + dy * dy > max_distance_sqr) {
            keep[c] = 0;
            return;
        }
    }
}

__global__ __launch_bounds__(256) void merge_tracks_count_kernel(const uint8_t *__restrict__ keep, size_t cells,
                                                                 uint32_t *__restrict__ block_counts)
{
    const size_t c = (size_t)blockIdx.x * 256 + threadIdx.x;
    const bool f = c < cells && keep[c];
    __shared__ uint32_t wsum[4];
    const unsigned long long b = __ballot(f);
    if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = (uint32_t)__popcll(b);
    __syncthreads();
    if (threadIdx.x == 0) block_counts[blockIdx.x] = wsum[0] + wsum[1] + wsum[2] + wsum[3];
}

// kept cells in row-major order: out_rows[k] = the cell's highest row, out_tracks[k] = that row (either may be null).
// Nothing is written when the scatter found an invalid point.
__global__ __launch_bounds__(256) void merge_tracks_write_kernel(const int2 *__restrict__ tracks, uint32_t m,
                                                                 const uint32_t *__restrict__ last,
                                                                 const uint8_t *__restrict__ keep, size_t cells,
                                                                 const uint32_t *__restrict__ block_offsets,
                                                                 const MergeCounters *__restrict__ cnt,
                                                                 unsigned long long *__restrict__ out_rows,
                                                                 int2 *__restrict__ out_tracks)
{
    const size_t c = (size_t)blockIdx.x * 256 + threadIdx.x;
    const bool f = c < cells && keep[c];
    __shared__ uint32_t wsum[4];
    const unsigned long long b = __ballot(f);
    const uint32_t lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    if (lane == 0) wsum[wv] = (uint32_t)__popcll(b);
    __syncthreads();
    if (!f || cnt->bad) return;
    unsigned long long off = block_offsets[blockIdx.x];
    for (uint32_t v = 0; v < wv; v++) off += wsum[v];
    off += (unsigned long long)__popcll(b & ((1ull << lane) - 1ull));
    const unsigned long long src = last[c] - 1u;
    if (out_rows) out_rows[off] = src;
    if (out_tracks)
        for (uint32_t j = 0; j < m; j++) out_tracks[off * m + j] = tracks[src * m + j];
}

void launch_merge_tracks(const int2 *tracks, unsigned long long n, uint32_t m, uint32_t image_index, uint32_t w, uint32_t h,
                         uint32_t r, unsigned long long max_distance_sqr, uint32_t *last, uint8_t *occ, uint32_t *area,
                         uint8_t *keep, uint32_t *block_counts, uint32_t *present_part, uint32_t *cells_part,
                         uint32_t *empty_part, MergeCounters *cnt, unsigned long long *out_rows, int2 *out_tracks,
                         hipStream_t s)
{
    const size_t cells = (size_t)w * h;
    const uint32_t cblocks = (uint32_t)((cells + 255) / 256);
    const unsigned tblocks = (unsigned)((n + 255) / 256);
    const size_t col_lanes = (size_t)w * ((h + MERGE_ROWS - 1) / MERGE_ROWS);
    if (n) {
        hipLaunchKernelGGL(merge_tracks_scatter_kernel, dim3(tblocks), dim3(256), 0, s, tracks, n, m, image_index, w, h, last,
                           present_part, cnt);
    }
    hipLaunchKernelGGL(merge_tracks_column_kernel, dim3((unsigned)((col_lanes + 255) / 256)), dim3(256), 0, s, last, w, h, r, occ);
    hipLaunchKernelGGL(merge_tracks_area_kernel, dim3(cblocks), dim3(256), 0, s, last, occ, w, h, r, area, keep, cells_part,
                       empty_part);
    hipLaunchKernelGGL(merge_tracks_sum_kernel, dim3(1), dim3(1024), 0, s, present_part, (uint32_t)tblocks, cells_part, empty_part,
                       cblocks, cnt);
    if (n) {
        hipLaunchKernelGGL(merge_tracks_check_kernel, dim3(tblocks), dim3(256), 0, s, tracks, n, m, image_index, w, h,
                           max_distance_sqr, area, keep);
    }
    hipLaunchKernelGGL(merge_tracks_count_kernel, dim3(cblocks), dim3(256), 0, s, keep, cells, block_counts);
    launch_scan_u32(block_counts, cblocks, &cnt->total, s);
    if (out_rows || out_tracks)
        hipLaunchKernelGGL(merge_tracks_write_kernel, dim3(cblocks), dim3(256), 0, s, tracks, m, last, keep, cells, block_counts,
                           cnt, out_rows, out_tracks);
}

} // namespace cvhip

using namespace cvhip;

extern "C" int cvhip_extend_tracks(cvhip_ctx *ctx, const int32_t *track_p1, uint64_t n_tracks, uint32_t max_dimension2,
                                   int32_t *out_track_p2, uint32_t *out_new_p1, uint32_t *out_new_p2, uint64_t cap,
                                   uint64_t *out_n_new)
{
    if (!ctx || !out_n_new) return fail(CVHIP_ERR_INVALID, "null argument");
    CVHIP_TRY(cvhip::flush_level_calls(ctx));
    if (n_tracks && (!track_p1 || !out_track_p2)) return fail(CVHIP_ERR_INVALID, "track arrays are null");
    if (cap && (!out_new_p1 || !out_new_p2)) return fail(CVHIP_ERR_INVALID, "new-track arrays are null");
    CVHIP_TRY_HIP(hipSetDevice(ctx->dev->d.ordinal));
    CVHIP_TRY(cvhip::flush_forward_cross_check(ctx));
    hipStream_t s = ctx->dev->d.stream;
    DirState &ds = ctx->dir[0];
    *out_n_new = 0;
    if (!ds.valid) { // nothing correlated: no matches to merge, no new tracks
        if (n_tracks && !on_device(out_track_p2))
            for (uint64_t i = 0; i < 2 * n_tracks; i++) out_track_p2[i] = -1;
        else if (n_tracks)
            CVHIP_TRY_HIP(hipMemsetAsync(out_track_p2, 0xFF, n_tracks * 2 * sizeof(int32_t), s));
        return CVHIP_OK;
    }
    const size_t n = (size_t)ds.gw * ds.gh;
    const uint32_t nblocks = (uint32_t)((n + 255) / 256);
    // scratch that is free between pairs: the contender words (8 B per pixel) hold the removal map, the
    // search-interval buffer the block counts (+ total, + the out-of-bounds flag)
    if ((size_t)nblocks + 2 > ctx->max_px || n > ctx->max_px * sizeof(unsigned long long))
        return fail(CVHIP_ERR_INVALID, "image too small for the scratch buffers");
    uint8_t *removed = reinterpret_cast<uint8_t *>(ctx->contenders);
    uint32_t *counts = ctx->range, *total = ctx->range + nblocks, *oob = ctx->range + nblocks + 1;
    // EXTEND_TRACKS_SEARCH_RADIUS = 3, TRACKS_RADIUS_DENOMINATOR = 1000 (triangulation.rs:16, 19, 1346-1350)
    const uint32_t radius = max_dimension2 > 1000 ? (uint32_t)((uint64_t)3 * max_dimension2 / 1000) : 3u;
    CallScratch sc;
    const int2 *d_tp1 = nullptr;
    int2 *const tp2 = reinterpret_cast<int2 *>(out_track_p2), *d_tp2 = nullptr;
    uint32_t *d_n1 = nullptr, *d_n2 = nullptr;
    uint32_t h_total = 0, h_oob = 0;
    hipError_t e = hipMemsetAsync(removed, 0, n, s);
    if (e == hipSuccess) e = hipMemsetAsync(oob, 0, sizeof(uint32_t), s);
    if (e == hipSuccess) e = sc.input(reinterpret_cast<const int2 *>(track_p1), (size_t)n_tracks, &d_tp1, s);
    if (e == hipSuccess) e = sc.output(tp2, (size_t)n_tracks, &d_tp2);
    if (e == hipSuccess) e = sc.output(out_new_p1, (size_t)cap * 2, &d_n1);
    if (e == hipSuccess) e = sc.output(out_new_p2, (size_t)cap * 2, &d_n2);
    if (e == hipSuccess) {
        launch_extend_tracks_match(ds.cells[ds.cur], ds.lw, ds.lh, ds.k, ds.gw, ds.gh, d_tp1, n_tracks, radius, d_tp2, removed,
                                   oob, s);
        launch_extend_tracks_new(ds.cells[ds.cur], ds.lw, ds.lh, ds.k, ds.gw, ds.gh, removed, counts, total, d_n1, d_n2, cap, s);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpyAsync(&h_total, total, sizeof(uint32_t), hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipMemcpyAsync(&h_oob, oob, sizeof(uint32_t), hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = sc.copy_out(tp2, d_tp2, (size_t)n_tracks, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    const size_t written = (size_t)std::min<uint64_t>(h_total, cap);
    if (e == hipSuccess) e = sc.copy_out(out_new_p1, d_n1, written * 2, s);
    if (e == hipSuccess) e = sc.copy_out(out_new_p2, d_n2, written * 2, s);
    if (e == hipSuccess) e = sc.drain(s);
    if (e != hipSuccess) return device_error("extend_tracks", e);
    if (h_oob) return fail(CVHIP_ERR_INVALID, "Index out of bounds (a merged match lies outside the image-1 grid; the reference panics here, data.rs:61-64)");
    *out_n_new = h_total;
    return CVHIP_OK;
}

// extend_tracks (triangulation.rs:1330-1419) with the grid add_image_pair_sparse builds from a pair's RANSAC inliers
// (:628-633): image-1 shape w1 x h1, cell (x1, y1) = Some(x2, y2), a later duplicate of a point overwriting an earlier one.
// The grid is uploaded as full-resolution cells and runs through the dense path's kernels above.
extern "C" int cvhip_extend_tracks_matches(cvhip_device *dev, const uint32_t *inliers, uint64_t n_inliers, uint32_t w1,
                                           uint32_t h1, const int32_t *track_p1, uint64_t n_tracks, uint32_t max_dimension2,
                                           int32_t *out_track_p2, uint32_t *out_new_p1, uint32_t *out_new_p2, uint64_t cap,
                                           uint64_t *out_n_new)
{
    if (!dev || !out_n_new || (n_inliers && !inliers)) return fail(CVHIP_ERR_INVALID, "null argument");
    if (n_tracks && (!track_p1 || !out_track_p2)) return fail(CVHIP_ERR_INVALID, "track arrays are null");
    if (cap && (!out_new_p1 || !out_new_p2)) return fail(CVHIP_ERR_INVALID, "new-track arrays are null");
    if (w1 == 0 || h1 == 0 || w1 > 65535 || h1 > 65535) return fail(CVHIP_ERR_INVALID, "extend_tracks_matches: image size");
    std::vector<uint32_t> cells((size_t)w1 * h1, CELL_NONE);
    for (uint64_t i = 0; i < n_inliers; i++) {
        const uint32_t *m = inliers + 4 * i;
        // (x2, y2) are packed in 16 bits each, and 0xFFFF / 0xFFFF would read as the empty cell: 65535 is rejected too
        if (m[0] >= w1 || m[1] >= h1 || m[2] >= 65535 || m[3] >= 65535)
            return fail(CVHIP_ERR_INVALID, "extend_tracks_matches: an inlier lies outside the image-1 grid");
        cells[(size_t)m[1] * w1 + m[0]] = m[2] | (m[3] << 16);
    }
    CVHIP_TRY_HIP(hipSetDevice(dev->d.ordinal));
    hipStream_t s = dev->d.stream;
    const size_t n = (size_t)w1 * h1;
    const uint32_t nblocks = (uint32_t)((n + 255) / 256);
    CallScratch sc;
    uint32_t *d_cells = nullptr, *d_counts = nullptr, *d_n1 = nullptr, *d_n2 = nullptr;
    uint8_t *d_removed = nullptr;
    const int2 *d_tp1 = nullptr;
    int2 *const tp2 = reinterpret_cast<int2 *>(out_track_p2), *d_tp2 = nullptr;
    hipError_t e = sc.copy_in(cells.data(), n, &d_cells, s);
    if (e == hipSuccess) e = sc.alloc(&d_removed, n);
    if (e == hipSuccess) e = sc.alloc(&d_counts, (size_t)nblocks + 2);
    if (e == hipSuccess) e = sc.input(reinterpret_cast<const int2 *>(track_p1), (size_t)n_tracks, &d_tp1, s);
    if (e == hipSuccess) e = sc.output(tp2, (size_t)n_tracks, &d_tp2);
    if (e == hipSuccess) e = sc.output(out_new_p1, (size_t)cap * 2, &d_n1);
    if (e == hipSuccess) e = sc.output(out_new_p2, (size_t)cap * 2, &d_n2);
    uint32_t *total = d_counts + nblocks, *oob = d_counts + nblocks + 1;
    if (e == hipSuccess) e = hipMemsetAsync(d_removed, 0, n, s);
    if (e == hipSuccess) e = hipMemsetAsync(oob, 0, 4, s);
    // EXTEND_TRACKS_SEARCH_RADIUS = 3, TRACKS_RADIUS_DENOMINATOR = 1000 (triangulation.rs:16, 19, 1346-1350)
    const uint32_t radius = max_dimension2 > 1000 ? (uint32_t)((uint64_t)3 * max_dimension2 / 1000) : 3u;
    uint32_t h_total = 0, h_oob = 0;
    if (e == hipSuccess) {
        launch_extend_tracks_match(d_cells, w1, h1, 0, w1, h1, d_tp1, n_tracks, radius, d_tp2, d_removed, oob, s);
        launch_extend_tracks_new(d_cells, w1, h1, 0, w1, h1, d_removed, d_counts, total, d_n1, d_n2, cap, s);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpyAsync(&h_total, total, 4, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipMemcpyAsync(&h_oob, oob, 4, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = sc.copy_out(tp2, d_tp2, (size_t)n_tracks, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    const size_t written = (size_t)std::min<uint64_t>(h_total, cap);
    if (e == hipSuccess) e = sc.copy_out(out_new_p1, d_n1, written * 2, s);
    if (e == hipSuccess) e = sc.copy_out(out_new_p2, d_n2, written * 2, s);
    if (e == hipSuccess) e = sc.drain(s);
    if (e != hipSuccess) return device_error("extend_tracks_matches", e);
    if (h_oob) return fail(CVHIP_ERR_INVALID, "Index out of bounds (a merged match lies outside the image-1 grid; the reference panics here, data.rs:61-64)");
    *out_n_new = h_total;
    return CVHIP_OK;
}

// merge_tracks (triangulation.rs:1421-1540) for image `image_index` of shape width x height over the n x m x 2 table;
// kernels above.
extern "C" int cvhip_merge_tracks(cvhip_device *dev, const int32_t *tracks, uint64_t n, uint32_t m, uint32_t image_index,
                                  uint32_t width, uint32_t height, uint64_t *out_rows, int32_t *out_tracks, uint64_t *out_n,
                                  uint64_t *out_stats)
{
    if (!dev || !out_n || (n && !tracks)) return fail(CVHIP_ERR_INVALID, "null argument");
    if (image_index >= m) return fail(CVHIP_ERR_INVALID, "merge_tracks: image_index >= m");
    if (m > CVHIP_TRIANGULATE_MAX_CAMERAS) return fail(CVHIP_ERR_UNSUPPORTED, "merge_tracks: more than CVHIP_TRIANGULATE_MAX_CAMERAS images");
    if (width == 0 || height == 0) return fail(CVHIP_ERR_INVALID, "merge_tracks: image size");
    // row + 1 and the cell offsets are 32-bit
    if (n >= 0xFFFFFFFFull || (uint64_t)width * height >= 0xFFFFFFFFull)
        return fail(CVHIP_ERR_UNSUPPORTED, "merge_tracks: more than 2^32 - 2 tracks or cells");
    CVHIP_TRY_HIP(hipSetDevice(dev->d.ordinal));
    hipStream_t s = dev->d.stream;
    // MERGE_TRACKS_SEARCH_RADIUS = 2, MERGE_TRACKS_MAX_DISTANCE = 10, TRACKS_RADIUS_DENOMINATOR = 1000 (:17-19, 1431-1443)
    const uint64_t md = std::max(width, height);
    const uint32_t r = md > 1000 ? (uint32_t)(2 * md / 1000) : 2u;
    const unsigned long long d2 = md > 1000 ? 10ull * 10ull * md / 1000 : 100ull;
    const size_t cells = (size_t)width * height;
    const uint32_t cblocks = (uint32_t)((cells + 255) / 256);
    const size_t tblocks = (size_t)((n + 255) / 256);
    CallScratch sc;
    uint32_t *d_last = nullptr, *d_area = nullptr, *d_counts = nullptr, *d_parts = nullptr;
    uint8_t *d_occ = nullptr, *d_keep = nullptr;
    MergeCounters *d_cnt = nullptr, h_cnt{};
    // the table and the outputs as rows of m points (out_rows: one index per kept row)
    const int2 *d_tr = nullptr;
    int2 *const otr = reinterpret_cast<int2 *>(out_tracks), *d_otr = nullptr;
    unsigned long long *const rows = reinterpret_cast<unsigned long long *>(out_rows), *d_rows = nullptr;
    hipError_t e = sc.alloc(&d_last, cells);
    if (e == hipSuccess) e = sc.alloc(&d_area, cells);
    if (e == hipSuccess) e = sc.alloc(&d_occ, cells);
    if (e == hipSuccess) e = sc.alloc(&d_keep, cells);
    if (e == hipSuccess) e = sc.alloc(&d_counts, (size_t)cblocks);
    if (e == hipSuccess) e = sc.alloc(&d_parts, tblocks + 2 * (size_t)cblocks);
    if (e == hipSuccess) e = sc.alloc(&d_cnt, 1);
    if (e == hipSuccess) e = sc.input(reinterpret_cast<const int2 *>(tracks), (size_t)n * m, &d_tr, s);
    if (e == hipSuccess) e = sc.output(rows, (size_t)n, &d_rows);
    if (e == hipSuccess) e = sc.output(otr, (size_t)n * m, &d_otr);
    if (e == hipSuccess) e = hipMemsetAsync(d_last, 0, cells * 4, s);
    if (e == hipSuccess) e = hipMemsetAsync(d_cnt, 0, sizeof(MergeCounters), s);
    if (e == hipSuccess) {
        launch_merge_tracks(d_tr, n, m, image_index, width, height, r, d2, d_last, d_occ, d_area, d_keep, d_counts, d_parts + 2 * cblocks,
                            d_parts, d_parts + cblocks, d_cnt, d_rows, d_otr, s);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpyAsync(&h_cnt, d_cnt, sizeof(MergeCounters), hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    const uint64_t k = h_cnt.total;
    if (e == hipSuccess && !h_cnt.bad) e = sc.copy_out(rows, d_rows, (size_t)k, s);
    if (e == hipSuccess && !h_cnt.bad) e = sc.copy_out(otr, d_otr, (size_t)k * m, s);
    if (e == hipSuccess) e = sc.drain(s);
    if (e != hipSuccess) return device_error("merge_tracks", e);
    if (h_cnt.bad)
        return fail(CVHIP_ERR_INVALID, "merge_tracks: a point has exactly one negative coordinate, or an image-i point lies "
                                       "outside the image (the reference panics here, data.rs:61-64)");
    *out_n = k;
    if (out_stats) {
        out_stats[0] = h_cnt.present;
        out_stats[1] = h_cnt.cells;
        out_stats[2] = (uint64_t)h_cnt.cells - k;
        out_stats[3] = h_cnt.empty_area;
    }
    return CVHIP_OK;
}
