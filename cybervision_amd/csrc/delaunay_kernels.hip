// delaunay_kernels.hip — cvhip_mesh_delaunay: the Delaunay triangulation of a camera's points (DelaunayTriangulation::
// bulk_load in Mesh::process_camera, output.rs:425) on the device.  DESIGN.md 4.13.
//
// A uniform grid over the points (counting sort), then one lane per point: the lane builds the star of its point by
// wrapping (delaunay_common.hpp) with filtered f64 predicates and counts the faces of which its point is the lowest index;
// a lane that meets a sign it cannot certify, more than lane_cells grid cells or more than MAX_NEIGHBOURS neighbours flags
// its point instead, and the library finishes the flagged stars on the host with exact predicates - the same routine, so
// the faces fit together as they are.  Count / scan / write: the faces come out grouped by their lowest index, ascending,
// in the order of the wrap - the same bytes on every call.  No lane keeps its star: the write pass wraps again.
// When every coordinate is an integer within 2^24 (counted with the extent) and cvhip_mesh_delaunay_set_lattice is on, the
// count and write kernels run as their LatticePolicy instantiations: exact integer signs, ties included, on the device; what
// still flags (duplicates, lane_cells, more than MAX_NEIGHBOURS neighbours) goes to the host as before.
#include <cmath>
#include <cstring>
#include <vector>

#include "cvhip_internal.hpp"
#include "delaunay_common.hpp"

namespace cvhip {
using namespace delaunay;
namespace {

constexpr int BLOCK = 256;
constexpr int MAX_GRID = CVHIP_MESH_GRID_LANES / BLOCK;
constexpr uint32_t MAX_NEIGHBOURS = 64; // a device star with more leaves for the host path (the loops' bound)

struct Extent {
    double min_x, max_x, min_y, max_y;
    unsigned long long bad;         // non-finite coordinates
    unsigned long long off_lattice; // finite coordinates that are no integer within 2^24 (LatticePolicy needs 0)
};

struct DeviceStats {
    unsigned long long device_stars;
    unsigned int most_cells;
};

// the extent of the points, reduced in a fixed order (tree over the block's lanes; extent_final_kernel folds the blocks in order)
__global__ __launch_bounds__(BLOCK) void dln_extent_kernel(const double2 *__restrict__ xy, unsigned long long k, Extent *__restrict__ partial)
{
    __shared__ double s_v[4][BLOCK];
    __shared__ unsigned long long s_n[BLOCK], s_off[BLOCK];
    double mnx = INFINITY, mxx = -INFINITY, mny = INFINITY, mxy = -INFINITY;
    unsigned long long bad = 0, off = 0;
    for (unsigned long long i = (unsigned long long)blockIdx.x * BLOCK + threadIdx.x; i < k; i += (unsigned long long)gridDim.x * BLOCK) {
        const double2 p = xy[i];
        if (!(fabs(p.x) < INFINITY) || !(fabs(p.y) < INFINITY)) {
            bad++;
            continue;
        }
        off += (on_lattice(p.x) ? 0u : 1u) + (on_lattice(p.y) ? 0u : 1u);
        mnx = fmin(mnx, p.x), mxx = fmax(mxx, p.x), mny = fmin(mny, p.y), mxy = fmax(mxy, p.y);
    }
    const int t = threadIdx.x;
    s_v[0][t] = mnx, s_v[1][t] = mxx, s_v[2][t] = mny, s_v[3][t] = mxy, s_n[t] = bad, s_off[t] = off;
    __syncthreads();
    for (int w = BLOCK / 2; w > 0; w >>= 1) {
        if (t < w) {
            s_v[0][t] = fmin(s_v[0][t], s_v[0][t + w]), s_v[1][t] = fmax(s_v[1][t], s_v[1][t + w]);
            s_v[2][t] = fmin(s_v[2][t], s_v[2][t + w]), s_v[3][t] = fmax(s_v[3][t], s_v[3][t + w]);
            s_n[t] += s_n[t + w], s_off[t] += s_off[t + w];
        }
        __syncthreads();
    }
    if (t == 0) partial[blockIdx.x] = Extent{s_v[0][0], s_v[1][0], s_v[2][0], s_v[3][0], s_n[0], s_off[0]};
}

__global__ void dln_extent_final_kernel(const Extent *__restrict__ partial, uint32_t blocks, Extent *__restrict__ out)
{
    if (threadIdx.x || blockIdx.x) return;
    Extent e{INFINITY, -INFINITY, INFINITY, -INFINITY, 0, 0};
    for (uint32_t b = 0; b < blocks; b++) {
        const Extent p = partial[b];
        e.min_x = fmin(e.min_x, p.min_x), e.max_x = fmax(e.max_x, p.max_x);
        e.min_y = fmin(e.min_y, p.min_y), e.max_y = fmax(e.max_y, p.max_y);
        e.bad += p.bad, e.off_lattice += p.off_lattice;
    }
    *out = e;
}

// ---- the grid: counting sort by cell (the order within a cell is that of the atomics: nothing depends on it) ----------------
__global__ __launch_bounds__(BLOCK) void dln_cell_count_kernel(Grid g, uint32_t *__restrict__ counts)
{
    for (unsigned long long i = (unsigned long long)blockIdx.x * BLOCK + threadIdx.x; i < g.k; i += (unsigned long long)gridDim.x * BLOCK)
        atomicAdd(&counts[cell_of(g, g.xy[2 * i], g.xy[2 * i + 1])], 1u); // (cell_of clamps into the grid)
}

__global__ __launch_bounds__(BLOCK) void dln_cell_fill_kernel(Grid g, uint32_t *__restrict__ cursor, uint32_t *__restrict__ cell_pts)
{
    for (unsigned long long i = (unsigned long long)blockIdx.x * BLOCK + threadIdx.x; i < g.k; i += (unsigned long long)gridDim.x * BLOCK) {
        const uint32_t pos = atomicAdd(&cursor[cell_of(g, g.xy[2 * i], g.xy[2 * i + 1])], 1u);
        if (pos < g.k) cell_pts[pos] = (uint32_t)i;
    }
}

// ---- the stars ----------------------------------------------------------------------------------------------------------------
struct CountFaces {
    uint32_t n = 0;
    __device__ void operator()(uint32_t a, uint32_t b, uint32_t c)
    {
        if (a < b && a < c) n++;
    }
};

struct WriteFaces {
    uint32_t *out; // this point's faces
    uint32_t n, room;
    __device__ void operator()(uint32_t a, uint32_t b, uint32_t c)
    {
        if (a < b && a < c && n < room) {
            out[3 * n] = a, out[3 * n + 1] = b, out[3 * n + 2] = c;
            n++;
        }
    }
};

// one lane per point: count[a] = the faces of which a is the lowest index, status[a] = 0; or status[a] = 1: the host path
// (Pol: FilterPolicy, or LatticePolicy on integer coordinates - an instantiation each, so neither pays for the other)
template <class Pol>
__global__ __launch_bounds__(BLOCK) void dln_count_kernel(Grid g, unsigned long long lane_cells, uint32_t *__restrict__ count,
                                                          uint8_t *__restrict__ status, DeviceStats *__restrict__ stats)
{
    const Pol pol;
    unsigned long long done = 0, most = 0;
    for (unsigned long long i = (unsigned long long)blockIdx.x * BLOCK + threadIdx.x; i < g.k; i += (unsigned long long)gridDim.x * BLOCK) {
        CountFaces emit;
        uint64_t cells = 0;
        const bool ok = build_star(g, pol, (uint32_t)i, lane_cells, MAX_NEIGHBOURS, emit, &cells);
        count[i] = ok ? emit.n : 0u;
        status[i] = ok ? 0 : 1;
        if (ok) {
            done++;
            if (cells > most) most = cells;
        }
    }
    // (a sum and a maximum of integers: the order of the atomics does not show)
    if (done) atomicAdd(&stats->device_stars, done);
    if (most) atomicMax(&stats->most_cells, (unsigned int)(most < 0xFFFFFFFFull ? most : 0xFFFFFFFFull));
}

// the host path's stars: their counts, and where their faces start in host_faces
__global__ __launch_bounds__(BLOCK) void dln_patch_kernel(const uint32_t *__restrict__ host_point, const uint32_t *__restrict__ host_count,
                                                          const uint32_t *__restrict__ host_offset, uint32_t n_host, uint32_t k,
                                                          uint32_t *__restrict__ count, uint32_t *__restrict__ offset_of)
{
    for (uint32_t i = blockIdx.x * BLOCK + threadIdx.x; i < n_host; i += gridDim.x * BLOCK) {
        const uint32_t a = host_point[i];
        if (a < k) count[a] = host_count[i], offset_of[a] = host_offset[i];
    }
}

// block_counts[b] = the faces of points [256 b, 256 b + 256)
__global__ __launch_bounds__(BLOCK) void dln_block_sum_kernel(const uint32_t *__restrict__ count, uint32_t k, uint32_t blocks,
                                                              uint32_t *__restrict__ block_counts)
{
    __shared__ uint32_t s_n[BLOCK];
    for (uint32_t b = blockIdx.x; b < blocks; b += gridDim.x) {
        const unsigned long long i = (unsigned long long)b * BLOCK + threadIdx.x;
        s_n[threadIdx.x] = i < k ? count[i] : 0u;
        __syncthreads();
        for (int w = BLOCK / 2; w > 0; w >>= 1) {
            if ((int)threadIdx.x < w) s_n[threadIdx.x] += s_n[threadIdx.x + w];
            __syncthreads();
        }
        if (threadIdx.x == 0) block_counts[b] = s_n[0];
        __syncthreads();
    }
}

// the faces of point a start at block_offsets[a / 256] + the counts of the block's earlier points; a device star is wrapped
// again (with the policy that counted it), a host star's faces are copied from host_faces
template <class Pol>
__global__ __launch_bounds__(BLOCK) void dln_write_kernel(Grid g, unsigned long long lane_cells, const uint32_t *__restrict__ count,
                                                          const uint8_t *__restrict__ status, const uint32_t *__restrict__ offset_of,
                                                          const uint32_t *__restrict__ host_faces, uint32_t n_host_faces,
                                                          const uint32_t *__restrict__ block_offsets, uint32_t blocks,
                                                          unsigned long long n_faces, uint32_t *__restrict__ out)
{
    __shared__ uint32_t s_n[BLOCK];
    const Pol pol;
    for (uint32_t b = blockIdx.x; b < blocks; b += gridDim.x) {
        const unsigned long long i = (unsigned long long)b * BLOCK + threadIdx.x;
        const uint32_t mine = i < g.k ? count[i] : 0u;
        s_n[threadIdx.x] = mine;
        __syncthreads();
        for (int w = 1; w < BLOCK; w <<= 1) { // inclusive scan
            const uint32_t v = (int)threadIdx.x >= w ? s_n[threadIdx.x - w] : 0u;
            __syncthreads();
            s_n[threadIdx.x] += v;
            __syncthreads();
        }
        const unsigned long long first = (unsigned long long)block_offsets[b] + s_n[threadIdx.x] - mine;
        __syncthreads();
        if (i < g.k && mine && first + mine <= n_faces) {
            if (status[i]) {
                const uint32_t src = offset_of[i];
                if ((unsigned long long)src + mine <= n_host_faces)
                    for (uint32_t q = 0; q < 3 * mine; q++) out[3 * first + q] = host_faces[3ull * src + q];
            } else {
                WriteFaces emit{out + 3 * first, 0, mine};
                uint64_t cells = 0;
                (void)build_star(g, pol, (uint32_t)i, lane_cells, MAX_NEIGHBOURS, emit, &cells);
            }
        }
    }
}

struct CollectFaces {
    std::vector<uint32_t> *faces;
    uint32_t n = 0;
    void operator()(uint32_t a, uint32_t b, uint32_t c)
    {
        if (a < b && a < c) {
            faces->insert(faces->end(), {a, b, c});
            n++;
        }
    }
};

} // namespace

int mesh_delaunay_run(Device &d, const double *xy, uint64_t k, uint32_t *out_faces, uint64_t cap_faces, uint64_t *out_n_faces,
                      uint64_t *out_stats)
{
    hipStream_t s = d.stream;
    CallScratch sc;
    d.mesh_delaunay_lattice_stars = 0; // (of this call, once its lattice kernels have run)
    uint64_t stats[6] = {0, 0, 0, 0, 0, 0};
    auto finish = [&](uint64_t n) {
        *out_n_faces = n;
        if (out_stats) std::memcpy(out_stats, stats, sizeof(stats));
        return CVHIP_OK;
    };
    if (!k) return finish(0);
    const double *d_xy = nullptr;
    Extent *partial = nullptr, *d_extent = nullptr, ext{};
    const uint32_t lanes = grid_for(k);
    hipError_t e = sc.input(xy, (size_t)k * 2, &d_xy, s);
    if (e == hipSuccess) e = sc.alloc(&partial, (size_t)MAX_GRID);
    if (e == hipSuccess) e = sc.alloc(&d_extent, 1);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(dln_extent_kernel, dim3(lanes), dim3(BLOCK), 0, s, reinterpret_cast<const double2 *>(d_xy), (unsigned long long)k, partial);
        hipLaunchKernelGGL(dln_extent_final_kernel, dim3(1), dim3(64), 0, s, partial, lanes, d_extent);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpyAsync(&ext, d_extent, sizeof(Extent), hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) return device_error("mesh_delaunay", e);
    if (ext.bad) return fail(CVHIP_ERR_INVALID, "mesh_delaunay: a coordinate is not finite");
    if (k < 3) return finish(0);
    const bool lattice = d.mesh_delaunay_lattice && ext.off_lattice == 0; // integer coordinates: the exact signs on the device

    Grid g{d_xy, (uint32_t)k, ext.min_x, ext.min_y, 1.0, 0.0, 1, 1, nullptr, nullptr};
    grid_dims(ext.min_x, ext.max_x, ext.min_y, ext.max_y, k, &g.s, &g.inv_s, &g.gw, &g.gh);
    const uint64_t cells = (uint64_t)g.gw * g.gh;
    if (cells >= 0xFFFFFFFFull) return fail(CVHIP_ERR_UNSUPPORTED, "mesh_delaunay: 2^32 - 1 or more grid cells");
    stats[0] = g.gw, stats[1] = g.gh;
    const uint32_t blocks = (uint32_t)((k + BLOCK - 1) / BLOCK);
    const unsigned long long lane_cells = d.mesh_delaunay_lane_cells == 0xFFFFFFFFu ? ~0ull : d.mesh_delaunay_lane_cells;
    uint32_t *cell_start = nullptr, *cursor = nullptr, *cell_pts = nullptr, *count = nullptr, *offset_of = nullptr, *block_counts = nullptr;
    uint8_t *status = nullptr;
    DeviceStats *d_stats = nullptr, h_stats{0, 0};
    e = sc.alloc(&cell_start, (size_t)cells + 1);
    if (e == hipSuccess) e = sc.alloc(&cursor, (size_t)cells);
    if (e == hipSuccess) e = sc.alloc(&cell_pts, (size_t)k);
    if (e == hipSuccess) e = sc.alloc(&count, (size_t)k);
    if (e == hipSuccess) e = sc.alloc(&offset_of, (size_t)k);
    if (e == hipSuccess) e = sc.alloc(&status, (size_t)k);
    if (e == hipSuccess) e = sc.alloc(&block_counts, (size_t)blocks + 1);
    if (e == hipSuccess) e = sc.alloc(&d_stats, 1);
    if (e == hipSuccess) e = hipMemsetAsync(cell_start, 0, ((size_t)cells + 1) * sizeof(uint32_t), s);
    if (e == hipSuccess) e = hipMemsetAsync(cell_pts, 0, (size_t)k * sizeof(uint32_t), s);
    if (e == hipSuccess) e = hipMemsetAsync(d_stats, 0, sizeof(DeviceStats), s);
    if (e != hipSuccess) return device_error("mesh_delaunay", e);
    hipLaunchKernelGGL(dln_cell_count_kernel, dim3(lanes), dim3(BLOCK), 0, s, g, cell_start);
    launch_scan_u32(cell_start, (uint32_t)cells, cell_start + cells, s);
    e = hipGetLastError();
    if (e == hipSuccess) e = hipMemcpyAsync(cursor, cell_start, (size_t)cells * sizeof(uint32_t), hipMemcpyDeviceToDevice, s);
    if (e != hipSuccess) return device_error("mesh_delaunay", e);
    hipLaunchKernelGGL(dln_cell_fill_kernel, dim3(lanes), dim3(BLOCK), 0, s, g, cursor, cell_pts);
    g.cell_start = cell_start, g.cell_pts = cell_pts;
    if (lattice)
        hipLaunchKernelGGL(dln_count_kernel<LatticePolicy>, dim3(lanes), dim3(BLOCK), 0, s, g, lane_cells, count, status, d_stats);
    else
        hipLaunchKernelGGL(dln_count_kernel<FilterPolicy>, dim3(lanes), dim3(BLOCK), 0, s, g, lane_cells, count, status, d_stats);
    e = hipGetLastError();
    std::vector<uint8_t> h_status((size_t)k);
    if (e == hipSuccess) e = hipMemcpyAsync(h_status.data(), status, (size_t)k, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipMemcpyAsync(&h_stats, d_stats, sizeof(DeviceStats), hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) return device_error("mesh_delaunay", e);
    stats[2] = h_stats.device_stars, stats[5] = h_stats.most_cells;
    if (lattice) d.mesh_delaunay_lattice_stars = h_stats.device_stars;

    // the flagged stars, on the host: the same routine with the exact predicates, on the device's grid
    std::vector<uint32_t> host_point, host_count, host_offset, host_faces;
    for (uint64_t a = 0; a < k; a++)
        if (h_status[a]) host_point.push_back((uint32_t)a);
    stats[3] = host_point.size();
    const uint32_t *d_host_faces = nullptr;
    if (!host_point.empty()) {
        std::vector<uint32_t> h_start((size_t)cells + 1), h_pts((size_t)k);
        std::vector<double> h_xy;
        e = hipMemcpyAsync(h_start.data(), cell_start, h_start.size() * sizeof(uint32_t), hipMemcpyDeviceToHost, s);
        if (e == hipSuccess) e = hipMemcpyAsync(h_pts.data(), cell_pts, h_pts.size() * sizeof(uint32_t), hipMemcpyDeviceToHost, s);
        if (e == hipSuccess && on_device(xy)) {
            h_xy.resize((size_t)k * 2);
            e = hipMemcpyAsync(h_xy.data(), d_xy, h_xy.size() * sizeof(double), hipMemcpyDeviceToHost, s);
        }
        if (e == hipSuccess) e = hipStreamSynchronize(s);
        if (e != hipSuccess) return device_error("mesh_delaunay", e);
        // (the grid is the device's own; a start past k or a point past k would only be the device's fault, and is refused)
        for (size_t c = 0; c + 1 < h_start.size(); c++)
            if (h_start[c] > h_start[c + 1] || h_start[c + 1] > k) return fail(CVHIP_ERR_DEVICE, "mesh_delaunay: the grid is inconsistent");
        Grid hg = g;
        hg.xy = h_xy.empty() ? xy : h_xy.data(), hg.cell_start = h_start.data(), hg.cell_pts = h_pts.data();
        Duplicates dups(hg);
        const ExactPolicy pol{&dups};
        for (const uint32_t a : host_point) {
            CollectFaces emit{&host_faces};
            const size_t before = host_faces.size();
            uint64_t visited = 0;
            if (!build_star(hg, pol, a, ~0ull, (uint32_t)k, emit, &visited)) { // (only arithmetic out of its range can do this)
                host_faces.resize(before);
                emit.n = 0;
            }
            if (dups.is_duplicate(a)) stats[4]++;
            host_count.push_back(emit.n);
            host_offset.push_back((uint32_t)(before / 3));
        }
        const uint32_t *d_point = nullptr, *d_count = nullptr, *d_offset = nullptr;
        const size_t nh = host_point.size();
        e = sc.input(host_point.data(), nh, &d_point, s);
        if (e == hipSuccess) e = sc.input(host_count.data(), nh, &d_count, s);
        if (e == hipSuccess) e = sc.input(host_offset.data(), nh, &d_offset, s);
        if (e == hipSuccess) e = sc.input(host_faces.data(), host_faces.size(), &d_host_faces, s);
        if (e != hipSuccess) return device_error("mesh_delaunay", e);
        hipLaunchKernelGGL(dln_patch_kernel, dim3(grid_for(nh)), dim3(BLOCK), 0, s, d_point, d_count, d_offset, (uint32_t)nh, (uint32_t)k, count, offset_of);
    }
    uint32_t total = 0;
    hipLaunchKernelGGL(dln_block_sum_kernel, dim3(grid_for((unsigned long long)blocks * BLOCK)), dim3(BLOCK), 0, s, count, (uint32_t)k, blocks, block_counts);
    launch_scan_u32(block_counts, blocks, block_counts + blocks, s);
    e = hipGetLastError();
    if (e == hipSuccess) e = hipMemcpyAsync(&total, block_counts + blocks, sizeof(uint32_t), hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s); // (the host arrays the patch was uploaded from live until here)
    if (e != hipSuccess) return device_error("mesh_delaunay", e);
    if (!cap_faces || !total) return finish(total);
    if (cap_faces < total) return fail(CVHIP_ERR_INVALID, "mesh_delaunay: the buffer is smaller than the face count");
    uint32_t *d_out = nullptr;
    e = sc.output(out_faces, (size_t)total * 3, &d_out);
    if (e != hipSuccess) return device_error("mesh_delaunay", e);
    const dim3 write_grid(grid_for((unsigned long long)blocks * BLOCK));
    if (lattice)
        hipLaunchKernelGGL(dln_write_kernel<LatticePolicy>, write_grid, dim3(BLOCK), 0, s, g, lane_cells, count, status, offset_of, d_host_faces,
                           (uint32_t)(host_faces.size() / 3), block_counts, blocks, (unsigned long long)total, d_out);
    else
        hipLaunchKernelGGL(dln_write_kernel<FilterPolicy>, write_grid, dim3(BLOCK), 0, s, g, lane_cells, count, status, offset_of, d_host_faces,
                           (uint32_t)(host_faces.size() / 3), block_counts, blocks, (unsigned long long)total, d_out);
    e = hipGetLastError();
    if (e == hipSuccess) e = sc.copy_out(out_faces, d_out, (size_t)total * 3, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) return device_error("mesh_delaunay", e);
    return finish(total);
}

} // namespace cvhip
