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
// The OBJ writer is mesh_obj_kernels.hip.  Not here: the colour table (an argument) and the PNG encoder.
#include <cmath>
#include <cstdio>
#include <cstring>

#include "cvhip_internal.hpp"

namespace cvhip {
namespace {

constexpr int BLOCK = 256;
constexpr uint32_t VERTEX_BYTES = 24, COLOUR_BYTES = 3, FACE_BYTES = 13;
// a block's records (at most 256 x 27 = 6912 bytes) behind up to 3 bytes that stand for the rest of its first dword
constexpr uint32_t STAGE_DWORDS = (BLOCK * (VERTEX_BYTES + COLOUR_BYTES) + 3 + 3) / 4;
enum { MODE_PLAIN = 0, MODE_COLOR = 1, MODE_TEXTURE = 2 };
enum { POINT_NONE = 0, POINT_NO_PIXEL = 1, POINT_PIXEL = 2 };

// the m RGB8 images, concatenated: image c is dims[c].x x dims[c].y pixels at pixels + offsets[c]
struct PlyImages {
    const uint8_t *pixels;
    const unsigned long long *offsets;
    const uint2 *dims;
};

// The track's first present point - the lowest image c with tracks[i][c].x >= 0, the presence test mesh_project_kernel
// uses (:716-720) - and whether get_pixel_checked finds its pixel (:723): x < width and y < height of that image.
__device__ __forceinline__ int first_point(const int2 *__restrict__ tracks, unsigned long long i, uint32_t m, const uint2 *__restrict__ dims,
                                           unsigned long long &pixel)
{
    for (uint32_t c = 0; c < m; c++) {
        const int2 p = tracks[i * m + c];
        if (p.x < 0) continue;
        const uint2 d = dims[c];
        if ((uint32_t)p.x >= d.x || (uint32_t)p.y >= d.y) return POINT_NO_PIXEL;
        pixel = ((unsigned long long)(uint32_t)p.y * d.x + (uint32_t)p.x) * 3ull;
        return POINT_PIXEL | (int)(c << 2);
    }
    return POINT_NONE;
}

// ---- count: per block of 256 consecutive tracks, the vertices that get colour bytes ------------------------------------------
// *no_point |= 1 when a track has no present point (the reference's "Track has no images")
__global__ __launch_bounds__(BLOCK) void mesh_ply_count_kernel(const int2 *__restrict__ tracks, unsigned long long n, uint32_t m,
                                                               const uint2 *__restrict__ dims, unsigned long long n_blocks,
                                                               uint32_t *__restrict__ block_counts, uint32_t *__restrict__ no_point)
{
    for (unsigned long long blk = blockIdx.x; blk < n_blocks; blk += gridDim.x) {
        const unsigned long long i = blk * BLOCK + threadIdx.x;
        unsigned long long pixel;
        const int kind = i < n ? (first_point(tracks, i, m, dims, pixel) & 3) : POINT_NO_PIXEL;
        const uint32_t coloured = __syncthreads_count(kind == POINT_PIXEL);
        const uint32_t none = __syncthreads_or(kind == POINT_NONE);
        if (threadIdx.x == 0) {
            block_counts[blk] = coloured;
            if (none) atomicOr(no_point, 1u);
        }
    }
}

__device__ __forceinline__ void put_be64(uint8_t *r, double v)
{
    const unsigned long long be = __builtin_bswap64((unsigned long long)__double_as_longlong(v));
    for (int j = 0; j < 8; j++) r[j] = (uint8_t)(be >> (8 * j));
}

// ---- vertices (:712-750) ----------------------------------------------------------------------------------------------------------
// One block per 256 consecutive tracks (in a grid-stride loop over such blocks): the lanes build their records in LDS at
// 24 t + 3 (coloured lanes before t), the block copies them out.  out = the vertex section's first byte, section_bytes its
// length; block_offsets = the exclusive scan of mesh_ply_count_kernel's counts (COLOR only).
template <bool COLOR>
__global__ __launch_bounds__(BLOCK) void mesh_ply_vertex_kernel(const double *__restrict__ points, const int2 *__restrict__ tracks,
                                                                unsigned long long n, uint32_t m, PlyImages img, double sx, double sy,
                                                                double sz, const uint32_t *__restrict__ block_offsets,
                                                                unsigned long long n_blocks, uint8_t *__restrict__ out,
                                                                unsigned long long section_bytes)
{
    __shared__ uint32_t s_rec[STAGE_DWORDS];
    __shared__ uint32_t s_wave[BLOCK / 64];
    uint8_t *s_bytes = reinterpret_cast<uint8_t *>(s_rec);
    const uint32_t t = threadIdx.x, lane = t & 63u, wave = t >> 6;
    for (unsigned long long blk = blockIdx.x; blk < n_blocks; blk += gridDim.x) {
        const unsigned long long i = blk * BLOCK + t;
        const bool on = i < n;
        bool coloured = false;
        uint8_t rgb[3] = {0, 0, 0};
        uint32_t before = 0, block_coloured = 0;
        if (COLOR) {
            unsigned long long pixel = 0;
            const int kind = on ? first_point(tracks, i, m, img.dims, pixel) : POINT_NONE;
            coloured = (kind & 3) == POINT_PIXEL;
            if (coloured) {
                const uint8_t *px = img.pixels + img.offsets[(uint32_t)kind >> 2] + pixel;
                rgb[0] = px[0], rgb[1] = px[1], rgb[2] = px[2];
            }
            const unsigned long long mask = __ballot(coloured);
            if (lane == 0) s_wave[wave] = (uint32_t)__popcll(mask);
            __syncthreads();
            for (uint32_t k = 0; k < BLOCK / 64; k++) {
                if (k < wave) before += s_wave[k];
                block_coloured += s_wave[k];
            }
            before += (uint32_t)__popcll(mask & ((1ull << lane) - 1ull));
        }
        const unsigned long long left = n - blk * BLOCK;
        const uint32_t in_block = left < BLOCK ? (uint32_t)left : BLOCK;
        const unsigned long long start = blk * BLOCK * VERTEX_BYTES + (COLOR ? (unsigned long long)block_offsets[blk] * COLOUR_BYTES : 0ull);
        uint32_t len = in_block * VERTEX_BYTES + block_coloured * COLOUR_BYTES;
        if (start + len > section_bytes) len = 0; // (the tracks changed since they were counted: write nothing out of place)
        uint8_t *dst = out + start;
        const uint32_t pad = (uint32_t)(reinterpret_cast<uintptr_t>(dst) & 3u);
        if (on) {
            uint8_t *r = s_bytes + pad + t * VERTEX_BYTES + before * COLOUR_BYTES;
            put_be64(r, points[3 * i] * sx);
            put_be64(r + 8, (-points[3 * i + 1]) * sy);
            put_be64(r + 16, points[3 * i + 2] * sz);
            if (coloured) r[24] = rgb[0], r[25] = rgb[1], r[26] = rgb[2];
        }
        __syncthreads();
        stage_out<BLOCK>(s_rec, pad, len, dst - pad);
        __syncthreads();
    }
}

// ---- faces (:752-763): the same staging with 13-byte records --------------------------------------------------------------------
__global__ __launch_bounds__(BLOCK) void mesh_ply_face_kernel(const uint32_t *__restrict__ polygons, unsigned long long n_poly,
                                                              unsigned long long n_blocks, uint8_t *__restrict__ out)
{
    __shared__ uint32_t s_rec[(BLOCK * FACE_BYTES + 3 + 3) / 4];
    uint8_t *s_bytes = reinterpret_cast<uint8_t *>(s_rec);
    const uint32_t t = threadIdx.x;
    for (unsigned long long blk = blockIdx.x; blk < n_blocks; blk += gridDim.x) {
        const unsigned long long p = blk * BLOCK + t, left = n_poly - blk * BLOCK;
        const uint32_t len = (left < BLOCK ? (uint32_t)left : BLOCK) * FACE_BYTES;
        uint8_t *dst = out + blk * BLOCK * FACE_BYTES;
        const uint32_t pad = (uint32_t)(reinterpret_cast<uintptr_t>(dst) & 3u);
        if (p < n_poly) {
            uint8_t *r = s_bytes + pad + t * FACE_BYTES;
            r[0] = 3;
            for (int k = 0; k < 3; k++) {
                const uint32_t be = __builtin_bswap32(polygons[3 * p + (2 - k)]);
                for (int j = 0; j < 4; j++) r[1 + 4 * k + j] = (uint8_t)(be >> (8 * j));
            }
        }
        __syncthreads();
        stage_out<BLOCK>(s_rec, pad, len, dst - pad);
        __syncthreads();
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
    if (vertex_mode > MODE_TEXTURE) return fail(CVHIP_ERR_INVALID, "mesh_ply: vertex_mode is not 0 (Plain), 1 (Color) or 2 (Texture)");
    const bool color = vertex_mode == MODE_COLOR;
    if (!dev || !out_size || !out_scale || (n && !points) || (n_poly && !polygons) || (cap && !out))
        return fail(CVHIP_ERR_INVALID, "mesh_ply: null argument");
    if (n >= 0xFFFFFFFFull) return fail(CVHIP_ERR_UNSUPPORTED, "mesh_ply: 2^32 - 1 or more tracks");
    if (n_poly >= 0xFFFFFFFFull) return fail(CVHIP_ERR_UNSUPPORTED, "mesh_ply: 2^32 - 1 or more polygons");
    if (color && n) {
        if (m == 0) return fail(CVHIP_ERR_INVALID, "Track has no images"); // :726
        if (!images || !image_offsets || !image_dims || !tracks) return fail(CVHIP_ERR_INVALID, "mesh_ply: Color mode without images");
        for (uint32_t c = 0; c < m; c++) { // every pixel the kernels may read lies inside `images`
            if (image_offsets[c + 1] < image_offsets[c]) return fail(CVHIP_ERR_INVALID, "mesh_ply: image_offsets decrease");
            const uint64_t pixels = (uint64_t)image_dims[2 * c] * image_dims[2 * c + 1];
            if (pixels > (image_offsets[c + 1] - image_offsets[c]) / 3)
                return fail(CVHIP_ERR_INVALID, "mesh_ply: an image is smaller than width x height x 3 bytes");
        }
    }
    CVHIP_TRY_HIP(hipSetDevice(dev->d.ordinal));
    hipStream_t s = dev->d.stream;
    CallScratch sc;
    const std::string header = ply_header(n, n_poly, color);
    const unsigned long long v_blocks = (n + BLOCK - 1) / BLOCK, f_blocks = (n_poly + BLOCK - 1) / BLOCK;
    const int32_t *d_tracks = nullptr;
    PlyImages img{nullptr, nullptr, nullptr};
    uint32_t *counts = nullptr; // per block of tracks, then the total, then the no-point flag
    uint32_t h_tail[2] = {0, 0};
    hipError_t e = hipSuccess;
    if (color && n) {
        const uint32_t *d_dims = nullptr;
        const unsigned long long *d_offsets = nullptr;
        e = sc.input(tracks, (size_t)n * m * 2, &d_tracks, s);
        if (e == hipSuccess) e = sc.input(images, (size_t)image_offsets[m], &img.pixels, s);
        if (e == hipSuccess) e = sc.input(reinterpret_cast<const unsigned long long *>(image_offsets), (size_t)m + 1, &d_offsets, s);
        if (e == hipSuccess) e = sc.input(image_dims, (size_t)m * 2, &d_dims, s);
        img.offsets = d_offsets, img.dims = reinterpret_cast<const uint2 *>(d_dims);
        if (e == hipSuccess) e = sc.alloc(&counts, (size_t)v_blocks + 2);
        if (e == hipSuccess) e = hipMemsetAsync(counts + v_blocks, 0, 2 * sizeof(uint32_t), s);
        if (e == hipSuccess) {
            hipLaunchKernelGGL(mesh_ply_count_kernel, dim3(grid_for(n)), dim3(BLOCK), 0, s, reinterpret_cast<const int2 *>(d_tracks),
                               (unsigned long long)n, m, img.dims, v_blocks, counts, counts + v_blocks + 1);
            launch_scan_u32(counts, (uint32_t)v_blocks, counts + v_blocks, s);
            e = hipGetLastError();
        }
        if (e == hipSuccess) e = hipMemcpyAsync(h_tail, counts + v_blocks, sizeof(h_tail), hipMemcpyDeviceToHost, s);
        if (e == hipSuccess) e = hipStreamSynchronize(s);
        if (e != hipSuccess) return device_error("mesh_ply", e);
        if (h_tail[1]) return fail(CVHIP_ERR_INVALID, "Track has no images"); // :726
    }
    const uint64_t vertex_bytes = n * VERTEX_BYTES + (uint64_t)h_tail[0] * COLOUR_BYTES, face_bytes = n_poly * FACE_BYTES;
    const uint64_t size = header.size() + vertex_bytes + face_bytes;
    *out_size = size;
    if (out_sections) out_sections[0] = header.size(), out_sections[1] = vertex_bytes, out_sections[2] = face_bytes;
    if (!cap) return CVHIP_OK;
    if (cap < size) return fail(CVHIP_ERR_INVALID, "mesh_ply: the buffer is smaller than the file image");
    const double *d_points = nullptr;
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
    if (n) {
        if (color)
            hipLaunchKernelGGL((mesh_ply_vertex_kernel<true>), dim3(grid_for(n)), dim3(BLOCK), 0, s, d_points,
                               reinterpret_cast<const int2 *>(d_tracks), (unsigned long long)n, m, img, out_scale[0], out_scale[1],
                               out_scale[2], counts, v_blocks, d_vertices, (unsigned long long)vertex_bytes);
        else
            hipLaunchKernelGGL((mesh_ply_vertex_kernel<false>), dim3(grid_for(n)), dim3(BLOCK), 0, s, d_points,
                               static_cast<const int2 *>(nullptr), (unsigned long long)n, m, img, out_scale[0], out_scale[1], out_scale[2],
                               static_cast<const uint32_t *>(nullptr), v_blocks, d_vertices, (unsigned long long)vertex_bytes);
    }
    if (n_poly)
        hipLaunchKernelGGL(mesh_ply_face_kernel, dim3(grid_for(n_poly)), dim3(BLOCK), 0, s, d_poly, (unsigned long long)n_poly, f_blocks,
                           d_faces);
    e = hipGetLastError();
    if (d_out != out) { // the body from the stand-in, the header from here
        if (e == hipSuccess) e = sc.copy_out(out + header.size(), d_vertices, (size_t)(size - header.size()), s);
        if (e == hipSuccess) e = hipStreamSynchronize(s);
        if (e == hipSuccess) std::memcpy(out, header.data(), header.size());
    } else {
        if (e == hipSuccess) e = hipMemcpyAsync(out, header.data(), header.size(), hipMemcpyHostToDevice, s);
        if (e == hipSuccess) e = hipStreamSynchronize(s);
    }
    if (e != hipSuccess) return device_error("mesh_ply", e);
    return CVHIP_OK;
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
