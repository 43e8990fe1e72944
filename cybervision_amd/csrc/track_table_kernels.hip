// track_table_kernels.hip — the dense track table in device memory (cvhip_tracks).
//
// PerspectiveTriangulation's table (zlogic/cybervision src/triangulation.rs:604-617: tracks, n x m points) owned by a handle
// in HBM, with the three pieces of bookkeeping a host table needs around the device entries: Track::add's fill rule
// (:370-375) and the append of extend_tracks' new tracks (:1397-1416), prune_projections' column selection (:913-938) and the
// row gather of triangulate_all's survivors (:817-865).  The search, the removal map and the scan of the new cells are
// track_kernels.hip's, unchanged; merge_tracks is cvhip_merge_tracks on the table's own device pointers.  Integer only.
#include "cvhip_internal.hpp"

#include <algorithm>
#include <utility>

struct cvhip_tracks {
    cvhip_device *dev = nullptr;
    int ordinal = 0;
    hipStream_t stream = nullptr;
    uint32_t m = 0;
    uint64_t rows = 0, cap = 0; // rows in use / rows `data` has room for
    int2 *data = nullptr;       // cap x m points
    int2 *spare = nullptr;      // merge's output buffer, exchanged with `data` (spare_cap rows; kept for the next merge)
    uint64_t spare_cap = 0;
    int2 *match = nullptr;      // extend's scratch column: the match of every existing track (match_cap points)
    uint64_t match_cap = 0;
};

namespace cvhip {

constexpr uint64_t TRACKS_MAX_ROWS = 0xFFFFFFFFull; // row + 1 is 32-bit in merge_tracks: fewer rows than this

// the tracks whose search found a match and, of those, the ones whose slot image2 is empty: counts[0] += matched,
// counts[1] += filled.  Reads only - the table is written by tracks_extend_apply_kernel, once the host has seen the flag.
__global__ __launch_bounds__(256) void tracks_extend_tally_kernel(const int2 *__restrict__ table, uint32_t m, uint32_t image2,
                                                                   const int2 *__restrict__ match, unsigned long long n,
                                                                   uint32_t *__restrict__ counts)
{
    const unsigned long long t = (unsigned long long)blockIdx.x * 256 + threadIdx.x;
    bool matched = false, filled = false;
    if (t < n) {
        matched = match[t].x >= 0;
        filled = matched && table[t * m + image2].x < 0;
    }
    __shared__ uint32_t wsum[8];
    const unsigned long long bm = __ballot(matched), bf = __ballot(filled);
    if ((threadIdx.x & 63) == 0) {
        wsum[threadIdx.x >> 6] = (uint32_t)__popcll(bm);
        wsum[4 + (threadIdx.x >> 6)] = (uint32_t)__popcll(bf);
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        const uint32_t nm = wsum[0] + wsum[1] + wsum[2] + wsum[3], nf = wsum[4] + wsum[5] + wsum[6] + wsum[7];
        if (nm) atomicAdd(&counts[0], nm);
        if (nf) atomicAdd(&counts[1], nf);
    }
}

// The fill and the append in one launch.  Blocks [0, tblocks): one lane per existing track - its match goes into slot image2
// if that slot is empty (x < 0).  Blocks [tblocks, tblocks + cblocks): one lane per image-1 cell, as
// extend_tracks_write_kernel - every remaining Some cell becomes row n + (its rank in scan order): the cell in slot image1,
// its match in slot image2, (-1, -1) elsewhere.  The two halves touch disjoint rows.
__global__ __launch_bounds__(256) void tracks_extend_apply_kernel(const uint32_t *__restrict__ cells, uint32_t lw, uint32_t lh,
                                                                   uint32_t k, uint32_t gw, uint32_t gh,
                                                                   const uint8_t *__restrict__ removed,
                                                                   const uint32_t *__restrict__ block_offsets, uint32_t tblocks,
                                                                   int2 *__restrict__ table, uint32_t m, uint32_t image1,
                                                                   uint32_t image2, const int2 *__restrict__ match,
                                                                   unsigned long long n, unsigned long long cap)
{
    if (blockIdx.x < tblocks) {
        const unsigned long long t = (unsigned long long)blockIdx.x * 256 + threadIdx.x;
        if (t >= n) return;
        const int2 p2 = match[t];
        int2 *slot = table + t * m + image2;
        if (p2.x >= 0 && slot->x < 0) *slot = p2;
        return;
    }
    const uint32_t cb = blockIdx.x - tblocks;
    const size_t i = (size_t)cb * 256 + threadIdx.x;
    uint32_t gx = 0, gy = 0, mx = 0, my = 0;
    bool f = false;
    if (i < (size_t)gw * gh) {
        gx = (uint32_t)(i % gw);
        gy = (uint32_t)(i / gw);
        f = full_res_match(cells, lw, lh, k, gx, gy, mx, my) && !removed[i];
    }
    __shared__ uint32_t wsum[4];
    const unsigned long long b = __ballot(f);
    const uint32_t lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    if (lane == 0) wsum[wv] = (uint32_t)__popcll(b);
    __syncthreads();
    if (!f) return;
    unsigned long long row = n + block_offsets[cb];
    for (uint32_t w = 0; w < wv; w++) row += wsum[w];
    row += (unsigned long long)__popcll(b & ((1ull << lane) - 1ull));
    if (row >= cap) return; // (the capacity was grown to n + total before the launch)
    int2 *out = table + row * m;
    for (uint32_t j = 0; j < m; j++)
        out[j] = j == image1 ? make_int2((int)gx, (int)gy) : j == image2 ? make_int2((int)mx, (int)my) : make_int2(-1, -1);
}

struct TrackColumns {
    uint32_t c[CVHIP_TRIANGULATE_MAX_CAMERAS];
};

// out[r, j] = src[r, cols.c[j]]: one lane per point of the output
__global__ __launch_bounds__(256) void tracks_select_columns_kernel(const int2 *__restrict__ src, uint32_t m, TrackColumns cols,
                                                                     uint32_t k, unsigned long long n, int2 *__restrict__ out)
{
    const unsigned long long i = (unsigned long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n * k) return;
    const unsigned long long r = i / k;
    out[i] = src[r * m + cols.c[i % k]];
}

// *bad |= 1 when a row of the list is not a row of the table
__global__ __launch_bounds__(256) void tracks_check_rows_kernel(const unsigned long long *__restrict__ rows, unsigned long long k,
                                                                 unsigned long long n, uint32_t *__restrict__ bad)
{
    const unsigned long long j = (unsigned long long)blockIdx.x * 256 + threadIdx.x;
    if (j < k && rows[j] >= n) atomicOr(bad, 1u);
}

// out[j] = row rows[j]: one lane per point of the output (every row was checked before)
__global__ __launch_bounds__(256) void tracks_gather_kernel(const int2 *__restrict__ table, uint32_t m,
                                                             const unsigned long long *__restrict__ rows, unsigned long long k,
                                                             int2 *__restrict__ out)
{
    const unsigned long long i = (unsigned long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= k * m) return;
    out[i] = table[rows[i / m] * m + i % m];
}

// room for `need` rows, the rows in use kept: at least twice the old capacity when it grows
static hipError_t tracks_reserve(cvhip_tracks *t, uint64_t need)
{
    if (need <= t->cap) return hipSuccess;
    const uint64_t cap = std::max<uint64_t>(need, 2 * t->cap);
    void *p = nullptr;
    hipError_t e = hipMalloc(&p, (size_t)cap * t->m * sizeof(int2));
    if (e != hipSuccess) return e;
    if (t->rows) {
        e = hipMemcpyAsync(p, t->data, (size_t)t->rows * t->m * sizeof(int2), hipMemcpyDeviceToDevice, t->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(t->stream);
        if (e != hipSuccess) {
            (void)hipFree(p);
            return e;
        }
    }
    if (t->data) (void)hipFree(t->data);
    t->data = static_cast<int2 *>(p);
    t->cap = cap;
    return hipSuccess;
}

// a device buffer of at least `need` elements (its contents are not kept)
static hipError_t tracks_buffer(int2 **buf, uint64_t *have, uint64_t need)
{
    if (*buf && need <= *have) return hipSuccess;
    if (*buf) (void)hipFree(*buf);
    *buf = nullptr;
    *have = 0;
    void *p = nullptr;
    const hipError_t e = hipMalloc(&p, (size_t)std::max<uint64_t>(need, 1) * sizeof(int2));
    if (e != hipSuccess) return e;
    *buf = static_cast<int2 *>(p);
    *have = std::max<uint64_t>(need, 1);
    return hipSuccess;
}

} // namespace cvhip

using namespace cvhip;

extern "C" int cvhip_tracks_create(cvhip_device *dev, uint32_t m, uint64_t reserve_rows, cvhip_tracks **out)
{
    if (!dev || !out) return fail(CVHIP_ERR_INVALID, "null argument");
    if (m == 0) return fail(CVHIP_ERR_INVALID, "tracks_create: m = 0");
    if (m > CVHIP_TRIANGULATE_MAX_CAMERAS) return fail(CVHIP_ERR_UNSUPPORTED, "tracks_create: more than CVHIP_TRIANGULATE_MAX_CAMERAS images");
    if (reserve_rows >= TRACKS_MAX_ROWS) return fail(CVHIP_ERR_UNSUPPORTED, "tracks_create: 2^32 - 1 or more rows");
    CVHIP_TRY_HIP(hipSetDevice(dev->d.ordinal));
    cvhip_tracks *t = new cvhip_tracks();
    t->dev = dev;
    t->ordinal = dev->d.ordinal;
    t->stream = dev->d.stream;
    t->m = m;
    const hipError_t e = tracks_reserve(t, reserve_rows);
    if (e != hipSuccess) {
        delete t;
        return device_error("tracks_create", e);
    }
    *out = t;
    return CVHIP_OK;
}

extern "C" void cvhip_tracks_destroy(cvhip_tracks *t)
{
    if (!t) return;
    (void)hipSetDevice(t->ordinal);
    if (t->data) (void)hipFree(t->data); // (hipFree waits for the work that still reads it)
    if (t->spare) (void)hipFree(t->spare);
    if (t->match) (void)hipFree(t->match);
    delete t;
}

extern "C" int cvhip_tracks_info(const cvhip_tracks *t, uint64_t *out_rows, uint64_t *out_capacity, uint32_t *out_m,
                                 const int32_t **out_device_rows)
{
    if (!t) return fail(CVHIP_ERR_INVALID, "null argument");
    if (out_rows) *out_rows = t->rows;
    if (out_capacity) *out_capacity = t->cap;
    if (out_m) *out_m = t->m;
    if (out_device_rows) *out_device_rows = reinterpret_cast<const int32_t *>(t->data);
    return CVHIP_OK;
}

extern "C" int cvhip_tracks_assign(cvhip_tracks *t, const int32_t *rows, uint64_t n)
{
    if (!t || (n && !rows)) return fail(CVHIP_ERR_INVALID, "null argument");
    if (n >= TRACKS_MAX_ROWS) return fail(CVHIP_ERR_UNSUPPORTED, "tracks_assign: 2^32 - 1 or more rows");
    CVHIP_TRY_HIP(hipSetDevice(t->ordinal));
    const size_t bytes = (size_t)n * t->m * sizeof(int2);
    const hipMemcpyKind kind = n && on_device(rows) ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
    if (n > t->cap) { // into a buffer of its own, which replaces the table's once the copy is in
        const uint64_t cap = std::max<uint64_t>(n, 2 * t->cap);
        void *p = nullptr;
        CVHIP_TRY_HIP_AT("tracks_assign", hipMalloc(&p, (size_t)cap * t->m * sizeof(int2)));
        hipError_t e = hipMemcpyAsync(p, rows, bytes, kind, t->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(t->stream);
        if (e != hipSuccess) {
            (void)hipFree(p);
            return device_error("tracks_assign", e);
        }
        if (t->data) (void)hipFree(t->data);
        t->data = static_cast<int2 *>(p);
        t->cap = cap;
    } else if (n) {
        CVHIP_TRY_HIP_AT("tracks_assign", hipMemcpyAsync(t->data, rows, bytes, kind, t->stream));
        CVHIP_TRY_HIP_AT("tracks_assign", hipStreamSynchronize(t->stream));
    }
    t->rows = n;
    return CVHIP_OK;
}

extern "C" int cvhip_tracks_read(const cvhip_tracks *t, uint64_t first, uint64_t n, int32_t *out)
{
    if (!t || (n && !out)) return fail(CVHIP_ERR_INVALID, "null argument");
    if (first > t->rows || n > t->rows - first) return fail(CVHIP_ERR_INVALID, "tracks_read: the range passes the last row");
    if (!n) return CVHIP_OK;
    CVHIP_TRY_HIP(hipSetDevice(t->ordinal));
    CVHIP_TRY_HIP_AT("tracks_read", hipMemcpyAsync(out, t->data + first * t->m, (size_t)n * t->m * sizeof(int2),
                                                   on_device(out) ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, t->stream));
    CVHIP_TRY_HIP_AT("tracks_read", hipStreamSynchronize(t->stream));
    return CVHIP_OK;
}

extern "C" int cvhip_tracks_extend(cvhip_tracks *t, cvhip_ctx *ctx, uint32_t image1, uint32_t image2, uint32_t max_dimension2,
                                   uint64_t *out_counts)
{
    if (!t || !ctx) return fail(CVHIP_ERR_INVALID, "null argument");
    if (image1 == image2 || image1 >= t->m || image2 >= t->m)
        return fail(CVHIP_ERR_INVALID, "tracks_extend: two different images below m");
    if (ctx->dev != t->dev) return fail(CVHIP_ERR_INVALID, "tracks_extend: the context belongs to another device handle");
    CVHIP_TRY(cvhip::flush_level_calls(ctx));
    CVHIP_TRY_HIP(hipSetDevice(t->ordinal));
    CVHIP_TRY(cvhip::flush_forward_cross_check(ctx));
    hipStream_t s = t->stream;
    DirState &ds = ctx->dir[0];
    if (out_counts) out_counts[0] = out_counts[1] = out_counts[2] = 0;
    if (!ds.valid) return CVHIP_OK; // nothing correlated: no matches to merge, no new tracks
    const size_t cells = (size_t)ds.gw * ds.gh;
    const uint32_t cblocks = (uint32_t)((cells + 255) / 256);
    const uint64_t n = t->rows;
    const uint32_t tblocks = (uint32_t)((n + 255) / 256);
    // the context's scratch that is free between pairs, as cvhip_extend_tracks uses it: the contender words hold the removal
    // map, the search-interval buffer the block counts and behind them {total, out-of-bounds flag, matched, filled}
    if ((size_t)cblocks + 4 > ctx->max_px || cells > ctx->max_px * sizeof(unsigned long long))
        return fail(CVHIP_ERR_INVALID, "image too small for the scratch buffers");
    uint8_t *removed = reinterpret_cast<uint8_t *>(ctx->contenders);
    uint32_t *counts = ctx->range, *tail = ctx->range + cblocks; // tail: total, oob, matched, filled
    // EXTEND_TRACKS_SEARCH_RADIUS = 3, TRACKS_RADIUS_DENOMINATOR = 1000 (triangulation.rs:16, 19, 1346-1350)
    const uint32_t radius = max_dimension2 > 1000 ? (uint32_t)((uint64_t)3 * max_dimension2 / 1000) : 3u;
    const uint32_t *grid = ds.cells[ds.cur];
    uint32_t h_tail[4] = {0, 0, 0, 0};
    hipError_t e = tracks_buffer(&t->match, &t->match_cap, n);
    if (e == hipSuccess) e = hipMemsetAsync(removed, 0, cells, s);
    if (e == hipSuccess) e = hipMemsetAsync(tail, 0, 4 * sizeof(uint32_t), s);
    if (e == hipSuccess) {
        // the search, once: column image1 of the table in place, the matches into the scratch column
        launch_extend_tracks_match(grid, ds.lw, ds.lh, ds.k, ds.gw, ds.gh, t->data + image1, n, radius, t->match, removed, tail + 1,
                                   s, t->m);
        // (cap = 0: the counts and their scan only - counts[] become the blocks' offsets, tail[0] the number of new rows)
        launch_extend_tracks_new(grid, ds.lw, ds.lh, ds.k, ds.gw, ds.gh, removed, counts, tail, nullptr, nullptr, 0, s);
        if (n)
            hipLaunchKernelGGL(tracks_extend_tally_kernel, dim3(tblocks), dim3(256), 0, s, t->data, t->m, image2, t->match, n,
                               tail + 2);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpyAsync(h_tail, tail, sizeof(h_tail), hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) return device_error("tracks_extend", e);
    if (h_tail[1])
        return fail(CVHIP_ERR_INVALID, "Index out of bounds (a merged match lies outside the image-1 grid; the reference panics here, data.rs:61-64)");
    const uint64_t total = h_tail[0];
    if (n + total >= TRACKS_MAX_ROWS) return fail(CVHIP_ERR_UNSUPPORTED, "tracks_extend: 2^32 - 1 or more rows");
    e = tracks_reserve(t, n + total);
    if (e != hipSuccess) return device_error("tracks_extend", e);
    if (h_tail[2] || total) {
        hipLaunchKernelGGL(tracks_extend_apply_kernel, dim3(tblocks + cblocks), dim3(256), 0, s, grid, ds.lw, ds.lh, ds.k, ds.gw,
                           ds.gh, removed, counts, tblocks, t->data, t->m, image1, image2, t->match, n, t->cap);
        e = hipGetLastError();
        if (e != hipSuccess) return device_error("tracks_extend", e);
    }
    t->rows = n + total;
    if (out_counts) {
        out_counts[0] = h_tail[2];
        out_counts[1] = h_tail[3];
        out_counts[2] = total;
    }
    return CVHIP_OK;
}

extern "C" int cvhip_tracks_merge(cvhip_tracks *t, uint32_t image_index, uint32_t width, uint32_t height, uint64_t *out_stats)
{
    if (!t) return fail(CVHIP_ERR_INVALID, "null argument");
    CVHIP_TRY_HIP(hipSetDevice(t->ordinal));
    // the second buffer has the table's capacity, so the exchange leaves the capacity as it is
    const uint64_t want = std::max<uint64_t>(t->cap, 1);
    if (!t->spare || t->spare_cap != want) {
        if (t->spare) (void)hipFree(t->spare);
        t->spare = nullptr;
        t->spare_cap = 0;
        void *p = nullptr;
        CVHIP_TRY_HIP_AT("tracks_merge", hipMalloc(&p, (size_t)want * t->m * sizeof(int2)));
        t->spare = static_cast<int2 *>(p);
        t->spare_cap = want;
    }
    uint64_t k = 0;
    // device pointers both: cvhip_merge_tracks reads the table and writes the second buffer in place, and writes nothing
    // when it returns an error
    CVHIP_TRY(cvhip_merge_tracks(t->dev, t->rows ? reinterpret_cast<const int32_t *>(t->data) : nullptr, t->rows, t->m, image_index,
                                 width, height, nullptr, reinterpret_cast<int32_t *>(t->spare), &k, out_stats));
    if (t->cap) std::swap(t->data, t->spare); // (no capacity: no rows, and none come out)
    t->rows = k;
    return CVHIP_OK;
}

extern "C" int cvhip_tracks_select_columns(const cvhip_tracks *src, const uint32_t *columns, uint32_t k, cvhip_tracks **out)
{
    if (!src || !columns || !out) return fail(CVHIP_ERR_INVALID, "null argument");
    if (k == 0 || k > src->m) return fail(CVHIP_ERR_INVALID, "tracks_select_columns: 1 to m columns");
    TrackColumns cols{};
    for (uint32_t j = 0; j < k; j++) {
        if (columns[j] >= src->m || (j && columns[j] <= columns[j - 1]))
            return fail(CVHIP_ERR_INVALID, "tracks_select_columns: the columns are strictly increasing and below m");
        cols.c[j] = columns[j];
    }
    cvhip_tracks *t = nullptr;
    CVHIP_TRY(cvhip_tracks_create(src->dev, k, src->rows, &t));
    const uint64_t n = src->rows;
    if (n) {
        hipLaunchKernelGGL(tracks_select_columns_kernel, dim3((unsigned)((n * k + 255) / 256)), dim3(256), 0, src->stream, src->data,
                           src->m, cols, k, n, t->data);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) {
            cvhip_tracks_destroy(t);
            return device_error("tracks_select_columns", e);
        }
    }
    t->rows = n;
    *out = t;
    return CVHIP_OK;
}

extern "C" int cvhip_tracks_gather(const cvhip_tracks *t, const uint64_t *rows, uint64_t k, int32_t *out)
{
    if (!t || (k && (!rows || !out))) return fail(CVHIP_ERR_INVALID, "null argument");
    if (k >= TRACKS_MAX_ROWS) return fail(CVHIP_ERR_UNSUPPORTED, "tracks_gather: 2^32 - 1 or more rows");
    if (!k) return CVHIP_OK;
    CVHIP_TRY_HIP(hipSetDevice(t->ordinal));
    hipStream_t s = t->stream;
    CallScratch sc;
    const unsigned long long *d_rows = nullptr;
    int2 *const o = reinterpret_cast<int2 *>(out), *d_out = nullptr;
    uint32_t *d_bad = nullptr, h_bad = 0;
    const unsigned kblocks = (unsigned)((k + 255) / 256);
    hipError_t e = sc.input(reinterpret_cast<const unsigned long long *>(rows), (size_t)k, &d_rows, s);
    if (e == hipSuccess) e = sc.output(o, (size_t)k * t->m, &d_out);
    if (e == hipSuccess) e = sc.alloc(&d_bad, 1);
    if (e == hipSuccess) e = hipMemsetAsync(d_bad, 0, sizeof(uint32_t), s);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(tracks_check_rows_kernel, dim3(kblocks), dim3(256), 0, s, d_rows, k, t->rows, d_bad);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpyAsync(&h_bad, d_bad, sizeof(uint32_t), hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) return device_error("tracks_gather", e);
    if (h_bad) return fail(CVHIP_ERR_INVALID, "tracks_gather: a row is not a row of the table");
    hipLaunchKernelGGL(tracks_gather_kernel, dim3((unsigned)((k * t->m + 255) / 256)), dim3(256), 0, s, t->data, t->m, d_rows, k,
                       d_out);
    e = hipGetLastError();
    if (e == hipSuccess) e = sc.copy_out(o, d_out, (size_t)k * t->m, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s); // (the rows' stand-in is freed when the call returns)
    if (e != hipSuccess) return device_error("tracks_gather", e);
    return CVHIP_OK;
}
