// mesh_obj_kernels.hip — Mesh::output with an ObjWriter (src/output.rs:521-559, 774-1007) on the device: the Wavefront OBJ
// file image, byte for byte, and the public f64 -> text primitive it rests on (f64_display.hpp).  DESIGN.md 4.14.
//
// The file image is, every line ended by '\n':
//   header  (Texture mode only)  mtllib {stem}.mtl                                                            composed on the host
//   v       one per track:       v {x * sx} {(-y) * sy} {z * sz}, in Color mode " {r / 255} {g / 255} {b / 255}" of the track's
//                                first present point iff get_pixel_checked finds its pixel
//   vt      (Texture mode only)  per track and per present point, in image order: vt {x / width} {1 - y / height}, no bounds test
//   f       one per polygon:     f, then for i in 2, 1, 0: " {vertex + 1}" or, in Texture mode, " {vertex + 1}/{uv + 1}" with
//                                uv = uv_index[vertex] + the track's present points among the images below the polygon's camera;
//                                in Texture mode "usemtl Textured{camera}" in front of polygon 0 and of every polygon whose
//                                camera differs from its predecessor's
// Records have data-dependent lengths (a v line is 8 to ~990 bytes), so the file is made in two passes over the same kernels
// (WRITE = false / true): the length pass leaves per block of 256 records the bytes of its records, a 64-bit exclusive scan
// places the blocks, the host learns the section sizes; the write pass runs the formatter again (nothing is kept between the
// passes but 8 bytes per block) and hands its records to the writer the PLY shares (mesh_records.hpp): placed by an in-block
// scan, assembled in LDS and copied out as aligned dwords.  A block with more bytes than the staging buffer (a block of
// subnormals is ~250 KB) stores its records directly.
// The {stem}-{i}.png images the .mtl names are cvhip_png_encode's (png_kernels.hip), one call per image.
#include <cstdio>
#include <cstring>
#include <string>

#include "mesh_records.hpp"

#include "f64_display.hpp"

namespace cvhip {
namespace {

namespace fd = f64_display;

constexpr uint32_t STAGE_BYTES = 40 * 1024; // a block of 256 v lines of the usual kind is ~15 KB, ~29 KB with colours

// single-block exclusive scan of n u64 in place, total to *total (launch_scan_u32 would wrap at 4 GB of text)
__global__ __launch_bounds__(1024) void obj_scan_u64_kernel(unsigned long long *__restrict__ data, unsigned long long n,
                                                            unsigned long long *__restrict__ total)
{
    __shared__ unsigned long long wtot[16];
    __shared__ unsigned long long carry_s;
    if (threadIdx.x == 0) carry_s = 0;
    __syncthreads();
    for (unsigned long long base = 0; base < n; base += 1024) {
        const unsigned long long i = base + threadIdx.x;
        const unsigned long long v = i < n ? data[i] : 0;
        unsigned long long incl = v;
#pragma unroll
        for (int s = 1; s < 64; s <<= 1) {
            const unsigned long long t = __shfl_up(incl, s, 64);
            if ((int)(threadIdx.x & 63) >= s) incl += t;
        }
        if ((threadIdx.x & 63) == 63) wtot[threadIdx.x >> 6] = incl;
        __syncthreads();
        unsigned long long woff = 0;
        for (uint32_t w = 0; w < (threadIdx.x >> 6); w++) woff += wtot[w];
        const unsigned long long carry = carry_s;
        if (i < n) data[i] = carry + woff + incl - v;
        __syncthreads();
        if (threadIdx.x == 1023) carry_s = carry + woff + incl;
        __syncthreads();
    }
    if (threadIdx.x == 0) *total = carry_s;
}

// What every kernel does with its lane's record of `len` bytes (0: none), which `write(dst)` writes.
// WRITE = false: sums[blk] = the block's bytes.  WRITE = true: write_records puts it at section + sums[blk] + (the bytes of
// the lanes before it); *record_offset = that offset.
template <bool WRITE, typename Writer>
__device__ __forceinline__ void emit(uint32_t len, Writer &&write, unsigned long long blk, unsigned long long *__restrict__ sums,
                                     uint8_t *__restrict__ section, unsigned long long section_bytes, uint32_t *s_stage, uint32_t *s_wave,
                                     unsigned long long *record_offset = nullptr)
{
    uint32_t total;
    const uint32_t before = block_scan(len, s_wave, total);
    if (!WRITE) {
        if (threadIdx.x == 0) sums[blk] = total;
        return;
    }
    const unsigned long long start = sums[blk];
    if (record_offset) *record_offset = start + before;
    write_records<STAGE_BYTES>(len, before, total, write, start, section, section_bytes, s_stage);
}

// ---- tracks: present points ---------------------------------------------------------------------------------------------------------
// Per track its number of present points (tracks[i][c].x >= 0) -> counts[i] when counts != nullptr, per block their sum ->
// sums[blk]; *no_point |= 1 for a track without one (the reference's "Track has no images", :908 and :961).
__global__ __launch_bounds__(BLOCK) void mesh_obj_count_kernel(const int2 *__restrict__ tracks, unsigned long long n, uint32_t m,
                                                               unsigned long long n_blocks, uint32_t *__restrict__ counts,
                                                               unsigned long long *__restrict__ sums, uint32_t *__restrict__ no_point)
{
    __shared__ uint32_t s_wave[BLOCK / 64];
    for (unsigned long long blk = blockIdx.x; blk < n_blocks; blk += gridDim.x) {
        const unsigned long long i = blk * BLOCK + threadIdx.x;
        uint32_t count = 0;
        if (i < n)
            for (uint32_t c = 0; c < m; c++) count += tracks[i * m + c].x >= 0 ? 1u : 0u;
        if (i < n && counts) counts[i] = count;
        if (i < n && count == 0) atomicOr(no_point, 1u);
        uint32_t total;
        block_scan(count, s_wave, total);
        if (threadIdx.x == 0) sums[blk] = total;
    }
}

// counts[i] -> uv_index[i], in place: the present points of the tracks before i (sums: the scanned block sums)
__global__ __launch_bounds__(BLOCK) void mesh_obj_uv_index_kernel(uint32_t *__restrict__ counts, unsigned long long n,
                                                                  unsigned long long n_blocks, const unsigned long long *__restrict__ sums)
{
    __shared__ uint32_t s_wave[BLOCK / 64];
    for (unsigned long long blk = blockIdx.x; blk < n_blocks; blk += gridDim.x) {
        const unsigned long long i = blk * BLOCK + threadIdx.x;
        uint32_t total;
        const uint32_t before = block_scan(i < n ? counts[i] : 0u, s_wave, total);
        if (i < n) counts[i] = (uint32_t)sums[blk] + before; // (n * m < 2^32 - 1)
    }
}

// ---- v lines (:891-936) -------------------------------------------------------------------------------------------------------------
template <bool COLOR, bool WRITE>
__global__ __launch_bounds__(BLOCK) void mesh_obj_vertex_kernel(const double *__restrict__ points, const int2 *__restrict__ tracks,
                                                                unsigned long long n, uint32_t m, TrackImages img, double sx, double sy,
                                                                double sz, unsigned long long n_blocks, unsigned long long *__restrict__ sums,
                                                                uint8_t *__restrict__ section, unsigned long long section_bytes)
{
    __shared__ uint32_t s_stage[WRITE ? STAGE_BYTES / 4 : 1];
    __shared__ uint32_t s_wave[BLOCK / 64];
    for (unsigned long long blk = blockIdx.x; blk < n_blocks; blk += gridDim.x) {
        const unsigned long long i = blk * BLOCK + threadIdx.x;
        fd::Decimal d[COLOR ? 6 : 3];
        uint32_t values = 0, len = 0;
        if (i < n) {
            d[0] = fd::shortest(points[3 * i] * sx);
            d[1] = fd::shortest((-points[3 * i + 1]) * sy);
            d[2] = fd::shortest(points[3 * i + 2] * sz);
            values = 3;
            if (COLOR) {
                unsigned long long pixel = 0;
                const int kind = first_point(tracks, i, m, img.dims, pixel); // (:898-906)
                if ((kind & 3) == POINT_PIXEL) {
                    const uint8_t *px = img.pixels + img.offsets[(uint32_t)kind >> 2] + pixel;
                    for (int k = 0; k < 3; k++) d[(COLOR ? 3 : 0) + k] = fd::shortest((double)px[k] / 255.0);
                    values = 6;
                }
            }
            len = 2; // 'v' and '\n'
#pragma unroll
            for (uint32_t k = 0; k < (COLOR ? 6u : 3u); k++)
                if (k < values) len += 1 + fd::display_len(d[k]);
        }
        emit<WRITE>(
            len,
            [&](uint8_t *dst) {
                *dst++ = 'v';
#pragma unroll
                for (uint32_t k = 0; k < (COLOR ? 6u : 3u); k++)
                    if (k < values) *dst++ = ' ', dst += fd::display_write(dst, d[k]);
                *dst = '\n';
            },
            blk, sums, section, section_bytes, s_stage, s_wave);
    }
}

// ---- vt lines (:938-969): one lane per (track, image) cell, in the file's order; an absent point is a record of no bytes -------------
template <bool WRITE>
__global__ __launch_bounds__(BLOCK) void mesh_obj_uv_kernel(const int2 *__restrict__ tracks, unsigned long long cells, uint32_t m,
                                                            const uint2 *__restrict__ dims, unsigned long long n_blocks,
                                                            unsigned long long *__restrict__ sums, uint8_t *__restrict__ section,
                                                            unsigned long long section_bytes)
{
    __shared__ uint32_t s_stage[WRITE ? STAGE_BYTES / 4 : 1];
    __shared__ uint32_t s_wave[BLOCK / 64];
    for (unsigned long long blk = blockIdx.x; blk < n_blocks; blk += gridDim.x) {
        const unsigned long long j = blk * BLOCK + threadIdx.x;
        fd::Decimal u{}, v{};
        uint32_t len = 0;
        if (j < cells) {
            const int2 p = tracks[j];
            if (p.x >= 0) {
                const uint2 dim = dims[j % m];
                u = fd::shortest((double)(uint32_t)p.x / (double)dim.x);
                v = fd::shortest(1.0 - (double)(uint32_t)p.y / (double)dim.y);
                len = 3 + fd::display_len(u) + 1 + fd::display_len(v) + 1;
            }
        }
        emit<WRITE>(
            len,
            [&](uint8_t *dst) {
                dst[0] = 'v', dst[1] = 't', dst[2] = ' ';
                dst += 3;
                dst += fd::display_write(dst, u);
                *dst++ = ' ';
                dst += fd::display_write(dst, v);
                *dst = '\n';
            },
            blk, sums, section, section_bytes, s_stage, s_wave);
    }
}

// ---- f lines (:971-997) -------------------------------------------------------------------------------------------------------------
// TEXTURE: cameras[p] = the polygon's camera, uv_index[i] = the vt lines in front of track i's.
template <bool TEXTURE, bool WRITE>
__global__ __launch_bounds__(BLOCK) void mesh_obj_face_kernel(const uint32_t *__restrict__ polygons, const uint32_t *__restrict__ cameras,
                                                              unsigned long long n_poly, const int2 *__restrict__ tracks, uint32_t m,
                                                              const uint32_t *__restrict__ uv_index, unsigned long long n_blocks,
                                                              unsigned long long *__restrict__ sums, uint8_t *__restrict__ section,
                                                              unsigned long long section_bytes)
{
    __shared__ uint32_t s_stage[WRITE ? STAGE_BYTES / 4 : 1];
    __shared__ uint32_t s_wave[BLOCK / 64];
    for (unsigned long long blk = blockIdx.x; blk < n_blocks; blk += gridDim.x) {
        const unsigned long long p = blk * BLOCK + threadIdx.x;
        unsigned long long index[3] = {0, 0, 0}, uv[3] = {0, 0, 0};
        uint32_t camera = 0, len = 0;
        bool material = false;
        if (p < n_poly) {
            if (TEXTURE) {
                camera = cameras[p];
                material = p == 0 || cameras[p - 1] != camera; // Some(camera_i) != current_image (:975)
                if (material) len += 16 + fd::u64_len(camera);  // "usemtl Textured", the number, '\n'
            }
            len += 2; // 'f' and '\n'
            for (int k = 0; k < 3; k++) {
                const uint32_t vertex = polygons[3 * p + (2 - k)];
                index[k] = (unsigned long long)vertex + 1;
                len += 1 + fd::u64_len(index[k]);
                if (TEXTURE) {
                    unsigned long long below = 0; // get_uv_index (:822-830): take(camera) past the track's end takes all of it
                    for (uint32_t c = 0; c < m && c < camera; c++) below += tracks[(unsigned long long)vertex * m + c].x >= 0 ? 1u : 0u;
                    uv[k] = (unsigned long long)uv_index[vertex] + below + 1;
                    len += 1 + fd::u64_len(uv[k]);
                }
            }
        }
        emit<WRITE>(
            len,
            [&](uint8_t *dst) {
                if (TEXTURE && material) {
                    const char word[] = "usemtl Textured";
                    for (int k = 0; k < 15; k++) dst[k] = (uint8_t)word[k];
                    dst += 15;
                    dst += fd::u64_write(dst, camera);
                    *dst++ = '\n';
                }
                *dst++ = 'f';
                for (int k = 0; k < 3; k++) {
                    *dst++ = ' ';
                    dst += fd::u64_write(dst, index[k]);
                    if (TEXTURE) *dst++ = '/', dst += fd::u64_write(dst, uv[k]);
                }
                *dst = '\n';
            },
            blk, sums, section, section_bytes, s_stage, s_wave);
    }
}

// ---- cvhip_f64_display: `{}` of each value, concatenated; offsets[i] = where value i's text begins, offsets[n] = the size -----------
template <bool WRITE>
__global__ __launch_bounds__(BLOCK) void f64_display_kernel(const double *__restrict__ values, unsigned long long n, unsigned long long n_blocks,
                                                            unsigned long long *__restrict__ sums, uint8_t *__restrict__ out,
                                                            unsigned long long out_bytes, unsigned long long *__restrict__ offsets)
{
    __shared__ uint32_t s_stage[WRITE ? STAGE_BYTES / 4 : 1];
    __shared__ uint32_t s_wave[BLOCK / 64];
    for (unsigned long long blk = blockIdx.x; blk < n_blocks; blk += gridDim.x) {
        const unsigned long long i = blk * BLOCK + threadIdx.x;
        fd::Decimal d{};
        uint32_t len = 0;
        if (i < n) d = fd::shortest(values[i]), len = fd::display_len(d);
        unsigned long long offset = 0;
        emit<WRITE>(len, [&](uint8_t *dst) { fd::display_write(dst, d); }, blk, sums, out, out_bytes, s_stage, s_wave, &offset);
        if (WRITE && offsets && i < n) {
            offsets[i] = offset;
            if (i == n - 1) offsets[n] = offset + len;
        }
    }
}

} // namespace

void launch_scan_u64(unsigned long long *data, unsigned long long n, unsigned long long *total, hipStream_t s)
{
    hipLaunchKernelGGL(obj_scan_u64_kernel, dim3(1), dim3(1024), 0, s, data, n, total);
}

} // namespace cvhip

using namespace cvhip;

extern "C" int cvhip_mesh_obj(cvhip_device *dev, const double *points, const int32_t *tracks, uint64_t n, uint32_t m, const uint8_t *images,
                              const uint64_t *image_offsets, const uint32_t *image_dims, uint32_t vertex_mode, const double *out_scale,
                              const uint32_t *polygons, const uint32_t *polygon_cameras, uint64_t n_poly, const char *stem, uint8_t *out,
                              uint64_t cap, uint64_t *out_size, uint64_t *out_sections)
{
    const bool color = vertex_mode == MODE_COLOR, texture = vertex_mode == MODE_TEXTURE;
    int rc = check_writer_args("mesh_obj", dev, points, n, vertex_mode, out_scale, polygons, n_poly, out, cap, out_size,
                               texture && !stem                         ? "mesh_obj: Texture mode without a stem"
                               : texture && n_poly && !polygon_cameras ? "mesh_obj: Texture mode without polygon_cameras"
                                                                       : nullptr);
    if (rc != CVHIP_OK) return rc;
    const bool with_tracks = (color || texture) && n;
    if (with_tracks) {
        if (m == 0) return fail(CVHIP_ERR_INVALID, "Track has no images"); // :908, :961
        if (n > 0xFFFFFFFEull / m) return fail(CVHIP_ERR_UNSUPPORTED, "mesh_obj: 2^32 - 1 or more points of tracks");
        if (texture && (!tracks || !image_dims)) return fail(CVHIP_ERR_INVALID, "mesh_obj: Texture mode without image_dims");
        if (color && (rc = check_track_images("mesh_obj", tracks, m, images, image_offsets, image_dims)) != CVHIP_OK) return rc;
    }
    CVHIP_TRY_HIP(hipSetDevice(dev->d.ordinal));
    hipStream_t s = dev->d.stream;
    CallScratch sc;
    const std::string header = texture ? "mtllib " + std::string(stem) + ".mtl\n" : std::string();
    const unsigned long long cells = with_tracks && texture ? n * m : 0;
    const unsigned long long v_blocks = (n + BLOCK - 1) / BLOCK, uv_blocks = (cells + BLOCK - 1) / BLOCK, f_blocks = (n_poly + BLOCK - 1) / BLOCK;
    const double *d_points = nullptr;
    const int2 *t2 = nullptr;
    const uint32_t *d_poly = nullptr, *d_cameras = nullptr;
    TrackImages img{nullptr, nullptr, nullptr};
    // per-block bytes of the v, vt and f records and present points of the tracks, then the four totals
    unsigned long long *sums = nullptr, h_totals[4] = {0, 0, 0, 0};
    uint32_t *flags = nullptr, h_flags[2] = {0, 0}; // a vertex >= n; a track without a point
    uint32_t *uv_index = nullptr;
    const size_t n_sums = (size_t)(2 * v_blocks + uv_blocks + f_blocks);
    hipError_t e = sc.input(points, (size_t)n * 3, &d_points, s);
    if (e == hipSuccess) e = sc.input(polygons, (size_t)n_poly * 3, &d_poly, s);
    if (e == hipSuccess && texture) e = sc.input(polygon_cameras, (size_t)n_poly, &d_cameras, s);
    if (e == hipSuccess && with_tracks) e = upload_track_images(sc, tracks, n, m, images, image_offsets, image_dims, color, &t2, &img, s);
    if (e == hipSuccess && with_tracks && texture) e = sc.alloc(&uv_index, (size_t)n);
    if (e == hipSuccess) e = sc.alloc(&sums, n_sums + 4);
    if (e == hipSuccess) e = sc.alloc(&flags, 2);
    if (e == hipSuccess) e = hipMemsetAsync(flags, 0, 2 * sizeof(uint32_t), s);
    if (e == hipSuccess) e = hipMemsetAsync(sums + n_sums, 0, 4 * sizeof(unsigned long long), s);
    if (e != hipSuccess) return device_error("mesh_obj", e);
    unsigned long long *v_sums = sums, *count_sums = sums + v_blocks, *uv_sums = count_sums + v_blocks, *f_sums = uv_sums + uv_blocks;
    unsigned long long *totals = sums + n_sums; // v, vt, f bytes; present points
    // ---- what must hold before a face is measured: vertices < n, and in Color and Texture mode a point in every track
    if (n_poly) launch_mesh_check_polygons(d_poly, n_poly, n, flags, s);
    if (with_tracks)
        hipLaunchKernelGGL(mesh_obj_count_kernel, dim3(grid_for(n)), dim3(BLOCK), 0, s, t2, (unsigned long long)n, m, v_blocks, uv_index, count_sums,
                           flags + 1);
    e = hipGetLastError();
    if (e == hipSuccess) e = hipMemcpyAsync(h_flags, flags, sizeof(h_flags), hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) return device_error("mesh_obj", e);
    if (h_flags[1]) return fail(CVHIP_ERR_INVALID, "Track has no images");
    if (h_flags[0]) return fail(CVHIP_ERR_INVALID, "mesh_obj: a polygon names a track >= n");
    // ---- the length pass
    auto vertex_pass = [&](bool write, uint8_t *section, unsigned long long bytes) {
        if (!n) return;
        const dim3 grid(grid_for(n)), block(BLOCK);
#define CVHIP_OBJ_VERTEX(COLOR, WRITE)                                                                                                 \
    hipLaunchKernelGGL((mesh_obj_vertex_kernel<COLOR, WRITE>), grid, block, 0, s, d_points, t2, (unsigned long long)n, m, img, out_scale[0], \
                       out_scale[1], out_scale[2], v_blocks, v_sums, section, bytes)
        if (color && write) CVHIP_OBJ_VERTEX(true, true);
        else if (color) CVHIP_OBJ_VERTEX(true, false);
        else if (write) CVHIP_OBJ_VERTEX(false, true);
        else CVHIP_OBJ_VERTEX(false, false);
#undef CVHIP_OBJ_VERTEX
    };
    auto uv_pass = [&](bool write, uint8_t *section, unsigned long long bytes) {
        if (!cells) return;
        const dim3 grid(grid_for(cells)), block(BLOCK);
        if (write)
            hipLaunchKernelGGL((mesh_obj_uv_kernel<true>), grid, block, 0, s, t2, cells, m, img.dims, uv_blocks, uv_sums, section, bytes);
        else
            hipLaunchKernelGGL((mesh_obj_uv_kernel<false>), grid, block, 0, s, t2, cells, m, img.dims, uv_blocks, uv_sums, section, bytes);
    };
    auto face_pass = [&](bool write, uint8_t *section, unsigned long long bytes) {
        if (!n_poly) return;
        const dim3 grid(grid_for(n_poly)), block(BLOCK);
#define CVHIP_OBJ_FACE(TEXTURE, WRITE)                                                                                                \
    hipLaunchKernelGGL((mesh_obj_face_kernel<TEXTURE, WRITE>), grid, block, 0, s, d_poly, d_cameras, (unsigned long long)n_poly, t2, m, uv_index, \
                       f_blocks, f_sums, section, bytes)
        if (texture && write) CVHIP_OBJ_FACE(true, true);
        else if (texture) CVHIP_OBJ_FACE(true, false);
        else if (write) CVHIP_OBJ_FACE(false, true);
        else CVHIP_OBJ_FACE(false, false);
#undef CVHIP_OBJ_FACE
    };
    if (cells) { // uv_index before the faces
        launch_scan_u64(count_sums, v_blocks, totals + 3, s);
        hipLaunchKernelGGL(mesh_obj_uv_index_kernel, dim3(grid_for(n)), dim3(BLOCK), 0, s, uv_index, (unsigned long long)n, v_blocks, count_sums);
    }
    vertex_pass(false, nullptr, 0);
    uv_pass(false, nullptr, 0);
    face_pass(false, nullptr, 0);
    if (n) launch_scan_u64(v_sums, v_blocks, totals, s);
    if (cells) launch_scan_u64(uv_sums, uv_blocks, totals + 1, s);
    if (n_poly) launch_scan_u64(f_sums, f_blocks, totals + 2, s);
    e = hipGetLastError();
    if (e == hipSuccess) e = hipMemcpyAsync(h_totals, totals, sizeof(h_totals), hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) return device_error("mesh_obj", e);
    const uint64_t v_bytes = h_totals[0], uv_bytes = h_totals[1], f_bytes = h_totals[2];
    const uint64_t size = header.size() + v_bytes + uv_bytes + f_bytes;
    *out_size = size;
    if (out_sections) out_sections[0] = header.size(), out_sections[1] = v_bytes, out_sections[2] = uv_bytes, out_sections[3] = f_bytes;
    if (!cap) return CVHIP_OK;
    if (cap < size) return fail(CVHIP_ERR_INVALID, "mesh_obj: the buffer is smaller than the file image");
    if (!size) return CVHIP_OK;
    // ---- the write pass
    uint8_t *d_out = nullptr;
    e = sc.output(out, (size_t)size, &d_out); // (a stand-in has the same offsets as `out`: the body starts behind the header's length)
    if (e != hipSuccess) return device_error("mesh_obj", e);
    uint8_t *d_v = d_out + header.size(), *d_uv = d_v + v_bytes, *d_f = d_uv + uv_bytes;
    vertex_pass(true, d_v, v_bytes);
    uv_pass(true, d_uv, uv_bytes);
    face_pass(true, d_f, f_bytes);
    return finish_file_image("mesh_obj", sc, header, out, d_out, size, hipGetLastError(), s);
}

extern "C" int cvhip_mesh_obj_mtl(const char *stem, uint32_t m, char *out, uint64_t cap, uint64_t *out_size)
{
    if (!stem || !out_size || (cap && !out)) return fail(CVHIP_ERR_INVALID, "mesh_obj_mtl: null argument");
    std::string text; // write_materials (:856-868)
    for (uint32_t i = 0; i < m; i++) {
        const std::string number = std::to_string(i), image = std::string(stem) + "-" + number + ".png";
        text += "newmtl Textured" + number + "\nKa 0.2 0.2 0.2\nKd 0.8 0.8 0.8\nKs 1.0 1.0 1.0\nillum 2\nNs 0.000500\n";
        text += "map_Ka " + image + "\nmap_Kd " + image + "\n\n";
    }
    *out_size = text.size();
    if (!cap) return CVHIP_OK;
    if (cap < text.size()) return fail(CVHIP_ERR_INVALID, "mesh_obj_mtl: the buffer is smaller than the text");
    std::memcpy(out, text.data(), text.size());
    return CVHIP_OK;
}

extern "C" int cvhip_f64_display(cvhip_device *dev, const double *values, uint64_t n, uint8_t *out, uint64_t cap, uint64_t *out_size,
                                 uint64_t *offsets)
{
    if (!dev || !out_size || (n && !values) || (cap && !out)) return fail(CVHIP_ERR_INVALID, "f64_display: null argument");
    if (n >= 0xFFFFFFFFull) return fail(CVHIP_ERR_UNSUPPORTED, "f64_display: 2^32 - 1 or more values");
    CVHIP_TRY_HIP(hipSetDevice(dev->d.ordinal));
    hipStream_t s = dev->d.stream;
    CallScratch sc;
    const unsigned long long blocks = (n + BLOCK - 1) / BLOCK;
    const double *d_values = nullptr;
    unsigned long long *sums = nullptr, h_total = 0, *d_offsets = nullptr;
    uint8_t *d_out = nullptr;
    hipError_t e = sc.input(values, (size_t)n, &d_values, s);
    if (e == hipSuccess) e = sc.alloc(&sums, (size_t)blocks + 1);
    if (e == hipSuccess) e = hipMemsetAsync(sums + blocks, 0, sizeof(unsigned long long), s);
    if (e == hipSuccess && n) {
        hipLaunchKernelGGL((f64_display_kernel<false>), dim3(grid_for(n)), dim3(BLOCK), 0, s, d_values, (unsigned long long)n, blocks, sums,
                           static_cast<uint8_t *>(nullptr), 0ull, static_cast<unsigned long long *>(nullptr));
        launch_scan_u64(sums, blocks, sums + blocks, s);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpyAsync(&h_total, sums + blocks, sizeof(h_total), hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) return device_error("f64_display", e);
    *out_size = h_total;
    if (!cap && h_total) return CVHIP_OK;
    if (cap < h_total) return fail(CVHIP_ERR_INVALID, "f64_display: the buffer is smaller than the text");
    e = sc.output(out, (size_t)h_total, &d_out);
    if (e == hipSuccess) e = sc.output(reinterpret_cast<unsigned long long *>(offsets), (size_t)n + 1, &d_offsets);
    if (e == hipSuccess && n) {
        hipLaunchKernelGGL((f64_display_kernel<true>), dim3(grid_for(n)), dim3(BLOCK), 0, s, d_values, (unsigned long long)n, blocks, sums, d_out,
                           h_total, d_offsets);
        e = hipGetLastError();
    } else if (e == hipSuccess && d_offsets)
        e = hipMemsetAsync(d_offsets, 0, sizeof(unsigned long long), s);
    if (e == hipSuccess) e = sc.copy_out(out, d_out, (size_t)h_total, s);
    if (e == hipSuccess && offsets) e = sc.copy_out(reinterpret_cast<unsigned long long *>(offsets), d_offsets, (size_t)n + 1, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) return device_error("f64_display", e);
    return CVHIP_OK;
}
