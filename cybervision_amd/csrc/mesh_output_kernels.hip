// mesh_output_kernels.hip — what output::output (src/output.rs:567-611) writes, on the device: PlyWriter's binary file image
// (:648-772, Mesh::output :521-559) and ImageWriter::complete's colour mapping (map_depth / map_color, :1117-1229).
// DESIGN.md 4.12.
//
// The file image is header, one record per track in track order, one record per polygon in list order:
//   vertex: x * sx, (-y) * sy, z * sz as 8 big-endian bytes each (negation first, one multiply: y = 0 gives -0.0); in Color
//           mode the 3 RGB bytes of the track's first present point follow iff get_pixel_checked succeeds - a point past its
//           image's right or lower edge gets none, so records are 24 or 27 bytes and their offsets a prefix sum;
//   face:   0x03, then big-endian u32 of vertices[2], vertices[1], vertices[0].
// The colour map is f64, one IEEE operation per written operation in the written order (-ffp-contract=off).
// The records are placed and stored by the writer the OBJ shares (mesh_records.hpp; the OBJ is mesh_obj_kernels.hip).
// Not here: the colour table (an argument).  The RGBA's PNG file is cvhip_png_encode's (png_kernels.hip).
#include <cmath>
#include <cstdio>
#include <string>

#include "mesh_records.hpp"

namespace cvhip {
namespace {

constexpr uint32_t VERTEX_BYTES = 24, COLOUR_BYTES = 3, FACE_BYTES = 13;
// a block's records (at most 256 x 27 = 6912 and 256 x 13 bytes) behind up to 3 bytes that stand for the rest of its first dword
constexpr uint32_t VERTEX_STAGE_BYTES = (BLOCK * (VERTEX_BYTES + COLOUR_BYTES) + 3 + 3) / 4 * 4;
constexpr uint32_t FACE_STAGE_BYTES = (BLOCK * FACE_BYTES + 3 + 3) / 4 * 4;

__device__ __forceinline__ void put_be64(uint8_t *r, double v)
{
    const unsigned long long be = __builtin_bswap64((unsigned long long)__double_as_longlong(v));
    for (int j = 0; j < 8; j++) r[j] = (uint8_t)(be >> (8 * j));
}

// ---- vertices (:712-750) ----------------------------------------------------------------------------------------------------------
// One block per 256 consecutive tracks (in a grid-stride loop over such blocks).  Plain records are 24 bytes: track i's is at
// 24 i, and there is no length pass.  COLOR records are 24 or 27 bytes: <true, false> leaves per block the bytes of its records
// in sums[blk] and *no_point |= 1 for a track without a present point (the reference's "Track has no images"); <true, true>
// finds its block's first byte in the scanned sums.  section = the vertex section's first byte.
template <bool COLOR, bool WRITE>
__global__ __launch_bounds__(BLOCK) void mesh_ply_vertex_kernel(const double *__restrict__ points, const int2 *__restrict__ tracks,
                                                                unsigned long long n, uint32_t m, TrackImages img, double sx, double sy,
                                                                double sz, unsigned long long n_blocks, unsigned long long *__restrict__ sums,
                                                                uint32_t *__restrict__ no_point, uint8_t *__restrict__ section,
                                                                unsigned long long section_bytes)
{
    __shared__ uint32_t s_stage[WRITE ? VERTEX_STAGE_BYTES / 4 : 1];
    __shared__ uint32_t s_wave[BLOCK / 64];
    const uint32_t t = threadIdx.x;
    for (unsigned long long blk = blockIdx.x; blk < n_blocks; blk += gridDim.x) {
        const unsigned long long i = blk * BLOCK + t, left = n - blk * BLOCK;
        const bool on = i < n;
        const uint8_t *px = nullptr; // the vertex's colour bytes, if it gets any
        uint32_t len = on ? VERTEX_BYTES : 0, before = t * VERTEX_BYTES, total = (left < BLOCK ? (uint32_t)left : BLOCK) * VERTEX_BYTES;
        unsigned long long start = blk * BLOCK * VERTEX_BYTES;
        if (COLOR) {
            unsigned long long pixel = 0;
            const int kind = on ? first_point(tracks, i, m, img.dims, pixel) : POINT_NO_PIXEL;
            if ((kind & 3) == POINT_PIXEL) len += COLOUR_BYTES;
            if (WRITE && (kind & 3) == POINT_PIXEL) px = img.pixels + img.offsets[(uint32_t)kind >> 2] + pixel;
            if (!WRITE && kind == POINT_NONE) atomicOr(no_point, 1u);
            before = block_scan(len, s_wave, total);
            if (!WRITE) {
                if (t == 0) sums[blk] = total;
                continue;
            }
            start = sums[blk];
        }
        write_records<VERTEX_STAGE_BYTES>(
            len, before, total,
            [&](uint8_t *r) {
                put_be64(r, points[3 * i] * sx);
                put_be64(r + 8, (-points[3 * i + 1]) * sy);
                put_be64(r + 16, points[3 * i + 2] * sz);
                if (px) r[24] = px[0], r[25] = px[1], r[26] = px[2];
            },
            start, section, section_bytes, s_stage);
    }
}

// ---- faces (:752-763): 13-byte records, polygon p's at 13 p ----------------------------------------------------------------------
__global__ __launch_bounds__(BLOCK) void mesh_ply_face_kernel(const uint32_t *__restrict__ polygons, unsigned long long n_poly,
                                                              unsigned long long n_blocks, uint8_t *__restrict__ section,
                                                              unsigned long long section_bytes)
{
    __shared__ uint32_t s_stage[FACE_STAGE_BYTES / 4];
    const uint32_t t = threadIdx.x;
    for (unsigned long long blk = blockIdx.x; blk < n_blocks; blk += gridDim.x) {
        const unsigned long long p = blk * BLOCK + t, left = n_poly - blk * BLOCK;
        write_records<FACE_STAGE_BYTES>(
            p < n_poly ? FACE_BYTES : 0, t * FACE_BYTES, (left < BLOCK ? (uint32_t)left : BLOCK) * FACE_BYTES,
            [&](uint8_t *r) {
                r[0] = 3;
                for (int k = 0; k < 3; k++) {
                    const uint32_t be = __builtin_bswap32(polygons[3 * p + (2 - k)]);
                    for (int j = 0; j < 4; j++) r[1 + 4 * k + j] = (uint8_t)(be >> (8 * j));
                }
            },
            blk * BLOCK * FACE_BYTES, section, section_bytes, s_stage);
    }
}

// ---- colour map (ImageWriter::complete, map_depth, map_color: :1117-1229) -------------------------------------------------------
// table: 256 x (R, G, B).  `as usize` and `as u8` saturate and send NaN to 0; round is half away from zero.
__device__ __forceinline__ uint8_t map_color(const uint8_t *table, double value)
{
    if (value >= 1.0) return table[3 * 255];
    const double step = 1.0 / 255.0;
    const double q = floor(value / step);
    const uint32_t box = q > 0.0 ? (q >= 254.0 ? 254u : (uint32_t)q) : 0u; // (as usize).clamp(0, 254)
    const double ratio = (value - step * (double)box) / step;
    const double c1 = (double)table[3 * box], c2 = (double)table[3 * (box + 1)];
    const double r = round(c2 * ratio + c1 * (1.0 - ratio));
    return r > 0.0 ? (r >= 255.0 ? (uint8_t)255 : (uint8_t)r) : (uint8_t)0;
}

// one lane per cell; a NaN cell is None: (0, 0, 0, 0)
__global__ __launch_bounds__(BLOCK) void mesh_colour_kernel(const double *__restrict__ map, unsigned long long cells, double min_depth,
                                                            double max_depth, const uint8_t *__restrict__ table, uchar4 *__restrict__ out)
{
    __shared__ uint8_t s_table[768];
    for (uint32_t k = threadIdx.x; k < 768; k += BLOCK) s_table[k] = table[k];
    __syncthreads();
    for (unsigned long long i = (unsigned long long)blockIdx.x * BLOCK + threadIdx.x; i < cells; i += (unsigned long long)gridDim.x * BLOCK) {
        const double depth = map[i];
        uchar4 px = make_uchar4(0, 0, 0, 0);
        if (depth == depth) {
            const double value = (depth - min_depth) / (max_depth - min_depth);
            px = make_uchar4(map_color(s_table, value), map_color(s_table + 1, value), map_color(s_table + 2, value), 255);
        }
        out[i] = px;
    }
}

// PlyWriter::output_header (:687-710)
std::string ply_header(uint64_t n, uint64_t n_poly, bool color)
{
    std::string h = "ply\nformat binary_big_endian 1.0\ncomment Cybervision 3D surface\n";
    h += "element vertex " + std::to_string(n) + "\nproperty double x\nproperty double y\nproperty double z\n";
    if (color) h += "property uchar red\nproperty uchar green\nproperty uchar blue\n";
    h += "element face " + std::to_string(n_poly) + "\nproperty list uchar int vertex_indices\nend_header\n";
    return h;
}

} // namespace
} // namespace cvhip

using namespace cvhip;

extern "C" int cvhip_mesh_ply(cvhip_device *dev, const double *points, const int32_t *tracks, uint64_t n, uint32_t m, const uint8_t *images,
                              const uint64_t *image_offsets, const uint32_t *image_dims, uint32_t vertex_mode, const double *out_scale,
                              const uint32_t *polygons, uint64_t n_poly, uint8_t *out, uint64_t cap, uint64_t *out_size,
                              uint64_t *out_sections)
{
    int rc = check_writer_args("mesh_ply", dev, points, n, vertex_mode, out_scale, polygons, n_poly, out, cap, out_size);
    if (rc != CVHIP_OK) return rc;
    const bool color = vertex_mode == MODE_COLOR && n;
    if (color) {
        if (m == 0) return fail(CVHIP_ERR_INVALID, "Track has no images"); // :726
        if ((rc = check_track_images("mesh_ply", tracks, m, images, image_offsets, image_dims)) != CVHIP_OK) return rc;
    }
    CVHIP_TRY_HIP(hipSetDevice(dev->d.ordinal));
    hipStream_t s = dev->d.stream;
    CallScratch sc;
    const std::string header = ply_header(n, n_poly, vertex_mode == MODE_COLOR);
    const unsigned long long v_blocks = (n + BLOCK - 1) / BLOCK, f_blocks = (n_poly + BLOCK - 1) / BLOCK;
    const double *d_points = nullptr;
    const int2 *d_tracks = nullptr;
    TrackImages img{nullptr, nullptr, nullptr};
    // Color mode: per block of tracks the bytes of its records, then their total, then (in its low word) the no-point flag
    unsigned long long *sums = nullptr, h_tail[2] = {n * VERTEX_BYTES, 0};
    uint32_t *no_point = nullptr;
    const dim3 v_grid(grid_for(n)), block(BLOCK);
    hipError_t e = hipSuccess;
    if (color) {
        e = upload_track_images(sc, tracks, n, m, images, image_offsets, image_dims, true, &d_tracks, &img, s);
        if (e == hipSuccess) e = sc.alloc(&sums, (size_t)v_blocks + 2);
        if (e == hipSuccess) e = hipMemsetAsync(sums + v_blocks, 0, sizeof(h_tail), s);
        if (e == hipSuccess) {
            no_point = reinterpret_cast<uint32_t *>(sums + v_blocks + 1);
            hipLaunchKernelGGL((mesh_ply_vertex_kernel<true, false>), v_grid, block, 0, s, d_points, d_tracks, (unsigned long long)n, m, img,
                               0.0, 0.0, 0.0, v_blocks, sums, no_point, static_cast<uint8_t *>(nullptr), 0ull);
            launch_scan_u64(sums, v_blocks, sums + v_blocks, s);
            e = hipGetLastError();
        }
        if (e == hipSuccess) e = hipMemcpyAsync(h_tail, sums + v_blocks, sizeof(h_tail), hipMemcpyDeviceToHost, s);
        if (e == hipSuccess) e = hipStreamSynchronize(s);
        if (e != hipSuccess) return device_error("mesh_ply", e);
        if (h_tail[1]) return fail(CVHIP_ERR_INVALID, "Track has no images"); // :726
    }
    const uint64_t vertex_bytes = h_tail[0], face_bytes = n_poly * FACE_BYTES;
    const uint64_t size = header.size() + vertex_bytes + face_bytes;
    *out_size = size;
    if (out_sections) out_sections[0] = header.size(), out_sections[1] = vertex_bytes, out_sections[2] = face_bytes;
    if (!cap) return CVHIP_OK;
    if (cap < size) return fail(CVHIP_ERR_INVALID, "mesh_ply: the buffer is smaller than the file image");
    const uint32_t *d_poly = nullptr;
    uint32_t *bad = nullptr, h_bad = 0;
    uint8_t *d_out = nullptr;
    e = sc.input(points, (size_t)n * 3, &d_points, s);
    if (e == hipSuccess) e = sc.input(polygons, (size_t)n_poly * 3, &d_poly, s);
    if (e == hipSuccess && n_poly) {
        e = sc.alloc(&bad, 1);
        if (e == hipSuccess) e = hipMemsetAsync(bad, 0, sizeof(uint32_t), s);
        if (e == hipSuccess) {
            launch_mesh_check_polygons(d_poly, n_poly, n, bad, s);
            e = hipGetLastError();
        }
        if (e == hipSuccess) e = hipMemcpyAsync(&h_bad, bad, sizeof(uint32_t), hipMemcpyDeviceToHost, s);
        if (e == hipSuccess) e = hipStreamSynchronize(s);
    }
    if (e != hipSuccess) return device_error("mesh_ply", e);
    if (h_bad) return fail(CVHIP_ERR_INVALID, "mesh_ply: a polygon names a track >= n");
    e = sc.output(out, (size_t)size, &d_out); // (a stand-in has the same offsets as `out`: the body starts behind the header's length)
    if (e != hipSuccess) return device_error("mesh_ply", e);
    uint8_t *d_vertices = d_out + header.size(), *d_faces = d_vertices + vertex_bytes;
    if (color)
        hipLaunchKernelGGL((mesh_ply_vertex_kernel<true, true>), v_grid, block, 0, s, d_points, d_tracks, (unsigned long long)n, m, img,
                           out_scale[0], out_scale[1], out_scale[2], v_blocks, sums, no_point, d_vertices, (unsigned long long)vertex_bytes);
    else if (n)
        hipLaunchKernelGGL((mesh_ply_vertex_kernel<false, true>), v_grid, block, 0, s, d_points, d_tracks, (unsigned long long)n, m, img,
                           out_scale[0], out_scale[1], out_scale[2], v_blocks, sums, no_point, d_vertices, (unsigned long long)vertex_bytes);
    if (n_poly)
        hipLaunchKernelGGL(mesh_ply_face_kernel, dim3(grid_for(n_poly)), block, 0, s, d_poly, (unsigned long long)n_poly, f_blocks, d_faces,
                           (unsigned long long)face_bytes);
    return finish_file_image("mesh_ply", sc, header, out, d_out, size, hipGetLastError(), s);
}

extern "C" int cvhip_mesh_colour_map(cvhip_device *dev, const double *map, uint64_t width, uint64_t height, double min_depth,
                                     double max_depth, const uint8_t *table, uint8_t *out_rgba)
{
    if (!dev || !table) return fail(CVHIP_ERR_INVALID, "mesh_colour_map: null argument");
    if (width && height && width > 0xFFFFFFFEull / height) return fail(CVHIP_ERR_UNSUPPORTED, "mesh_colour_map: 2^32 - 1 or more cells");
    const unsigned long long cells = width * height;
    if (!cells) return CVHIP_OK;
    if (!map || !out_rgba) return fail(CVHIP_ERR_INVALID, "mesh_colour_map: null argument");
    CVHIP_TRY_HIP(hipSetDevice(dev->d.ordinal));
    hipStream_t s = dev->d.stream;
    CallScratch sc;
    const double *d_map = nullptr;
    uint8_t *d_table = nullptr, *d_out = nullptr;
    hipError_t e = sc.input(map, (size_t)cells, &d_map, s);
    if (e == hipSuccess) e = sc.alloc(&d_table, 768);
    if (e == hipSuccess) e = hipMemcpyAsync(d_table, table, 768, hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = sc.output(out_rgba, (size_t)cells * 4, &d_out);
    if (e == hipSuccess && (reinterpret_cast<uintptr_t>(d_out) & 3u)) return fail(CVHIP_ERR_INVALID, "mesh_colour_map: out_rgba is not 4-byte aligned");
    if (e == hipSuccess) {
        hipLaunchKernelGGL(mesh_colour_kernel, dim3(grid_for(cells)), dim3(BLOCK), 0, s, d_map, cells, min_depth,
                           max_depth, d_table, reinterpret_cast<uchar4 *>(d_out));
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = sc.copy_out(out_rgba, d_out, (size_t)cells * 4, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) return device_error("mesh_colour_map", e);
    return CVHIP_OK;
}
