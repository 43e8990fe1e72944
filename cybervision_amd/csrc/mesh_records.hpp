// mesh_records.hpp — the one record writer behind the file images of Mesh::output: the binary PLY (mesh_output_kernels.hip,
// DESIGN.md 4.12) and the Wavefront OBJ (mesh_obj_kernels.hip).  Both lay per-track and per-polygon records
// of data-dependent length into a byte buffer, behind a header composed on the host, at any alignment, in device or host
// memory.  Included by those two sources only.
#pragma once

#include <cstring>

#include "cvhip_internal.hpp"

namespace cvhip {

constexpr int BLOCK = 256; // lanes of a block = records of a block
enum { MODE_PLAIN = 0, MODE_COLOR = 1, MODE_TEXTURE = 2 };
enum { POINT_NONE = 0, POINT_NO_PIXEL = 1, POINT_PIXEL = 2 };

// the m RGB8 images, concatenated: image c is dims[c].x x dims[c].y pixels at pixels + offsets[c]
struct TrackImages {
    const uint8_t *pixels;
    const unsigned long long *offsets;
    const uint2 *dims;
};

// The track's first present point - the lowest image c with tracks[i][c].x >= 0, the presence test mesh_project_kernel
// uses (:716-720, :898-906) - and whether get_pixel_checked finds its pixel (:723): x < width and y < height of that image.
// -> POINT_NONE, POINT_NO_PIXEL, or POINT_PIXEL | c << 2 with `pixel` = the pixel's byte in image c
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

// exclusive scan of v over the block's 256 lanes; total = the block's sum.  s_wave: BLOCK / 64 words of LDS.
__device__ __forceinline__ uint32_t block_scan(uint32_t v, uint32_t *s_wave, uint32_t &total)
{
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    uint32_t incl = v;
#pragma unroll
    for (int s = 1; s < 64; s <<= 1) {
        const uint32_t t = __shfl_up(incl, s, 64);
        if ((int)lane >= s) incl += t;
    }
    __syncthreads(); // (the previous round's readers are done with s_wave)
    if (lane == 63) s_wave[wave] = incl;
    __syncthreads();
    uint32_t before = 0;
    total = 0;
    for (uint32_t k = 0; k < BLOCK / 64; k++) {
        if (k < wave) before += s_wave[k];
        total += s_wave[k];
    }
    return before + incl - v;
}

// The block's `len` staged bytes, which begin `pad` bytes into `stage`, go to dst + pad .. dst + pad + len (dst is 4-byte
// aligned): lanes take consecutive dwords; a dword whose four bytes are all the block's is one store, the others - the
// block's unaligned head and tail, whose remaining bytes belong to the neighbouring blocks or the header - go byte by byte.
template <int BLOCK>
__device__ __forceinline__ void stage_out(const uint32_t *stage, uint32_t pad, uint32_t len, uint8_t *__restrict__ dst)
{
    const uint8_t *bytes = reinterpret_cast<const uint8_t *>(stage);
    const uint32_t end = pad + len;
    for (uint32_t k = threadIdx.x; 4 * k < end; k += BLOCK) {
        const uint32_t lo = 4 * k < pad ? pad : 4 * k, hi = 4 * k + 4 > end ? end : 4 * k + 4;
        if (hi - lo == 4)
            reinterpret_cast<uint32_t *>(dst)[k] = stage[k];
        else
            for (uint32_t b = lo; b < hi; b++) dst[b] = bytes[b];
    }
}

// The lane's record of `len` bytes (0: none), which `write(dst)` writes, goes to section + start + before: `start` = where
// the block's records begin in the section, `before` = the bytes of the lanes before this one, `total` = the block's bytes
// (the three from block_scan and the scanned block sums, or computed where the records have one length).  The block
// assembles its records in s_stage (STAGE_BYTES of LDS) behind pad = address & 3 bytes and copies them out with stage_out,
// or, when its bytes do not fit in the buffer, every lane stores its own record directly; a block that would end past the
// section (the inputs changed since they were measured) writes nothing.  Called by all lanes of the block.
template <uint32_t STAGE_BYTES, typename Writer>
__device__ __forceinline__ void write_records(uint32_t len, uint32_t before, uint32_t total, Writer &&write, unsigned long long start,
                                              uint8_t *__restrict__ section, unsigned long long section_bytes, uint32_t *s_stage)
{
    if (start + total > section_bytes || total == 0) return;
    uint8_t *dst = section + start;
    if (total + 3 <= STAGE_BYTES) {
        const uint32_t pad = (uint32_t)(reinterpret_cast<uintptr_t>(dst) & 3u);
        if (len) write(reinterpret_cast<uint8_t *>(s_stage) + pad + before);
        __syncthreads();
        stage_out<BLOCK>(s_stage, pad, total, dst - pad);
        __syncthreads();
    } else if (len)
        write(dst + before);
}

// ---- the host side of a writer's entry point; `what` = "mesh_ply" or "mesh_obj", the prefix of its messages ------------------

// What both entries check first.  own_error: what the format's own arguments lack (it ranks between a null argument and the
// counts), or nullptr.
inline int check_writer_args(const std::string &what, const cvhip_device *dev, const double *points, uint64_t n, uint32_t vertex_mode,
                             const double *out_scale, const uint32_t *polygons, uint64_t n_poly, const uint8_t *out, uint64_t cap,
                             const uint64_t *out_size, const char *own_error = nullptr)
{
    if (vertex_mode > MODE_TEXTURE) return fail(CVHIP_ERR_INVALID, what + ": vertex_mode is not 0 (Plain), 1 (Color) or 2 (Texture)");
    if (!dev || !out_size || !out_scale || (n && !points) || (n_poly && !polygons) || (cap && !out))
        return fail(CVHIP_ERR_INVALID, what + ": null argument");
    if (own_error) return fail(CVHIP_ERR_INVALID, own_error);
    if (n >= 0xFFFFFFFFull) return fail(CVHIP_ERR_UNSUPPORTED, what + ": 2^32 - 1 or more tracks");
    if (n_poly >= 0xFFFFFFFFull) return fail(CVHIP_ERR_UNSUPPORTED, what + ": 2^32 - 1 or more polygons");
    return CVHIP_OK;
}

// Color mode's arrays: every pixel the kernels may read lies inside `images`
inline int check_track_images(const std::string &what, const int32_t *tracks, uint32_t m, const uint8_t *images, const uint64_t *image_offsets,
                              const uint32_t *image_dims)
{
    if (!images || !image_offsets || !image_dims || !tracks) return fail(CVHIP_ERR_INVALID, what + ": Color mode without images");
    for (uint32_t c = 0; c < m; c++) {
        if (image_offsets[c + 1] < image_offsets[c]) return fail(CVHIP_ERR_INVALID, what + ": image_offsets decrease");
        const uint64_t pixels = (uint64_t)image_dims[2 * c] * image_dims[2 * c + 1];
        if (pixels > (image_offsets[c + 1] - image_offsets[c]) / 3)
            return fail(CVHIP_ERR_INVALID, what + ": an image is smaller than width x height x 3 bytes");
    }
    return CVHIP_OK;
}

// the tracks and the images' sizes on the device, with_pixels (Color mode): their pixels and offsets too
inline hipError_t upload_track_images(CallScratch &sc, const int32_t *tracks, uint64_t n, uint32_t m, const uint8_t *images,
                                      const uint64_t *image_offsets, const uint32_t *image_dims, bool with_pixels, const int2 **d_tracks,
                                      TrackImages *img, hipStream_t s)
{
    const int32_t *t = nullptr;
    const uint32_t *dims = nullptr;
    const unsigned long long *offsets = nullptr;
    hipError_t e = sc.input(tracks, (size_t)n * m * 2, &t, s);
    if (e == hipSuccess) e = sc.input(image_dims, (size_t)m * 2, &dims, s);
    if (e == hipSuccess && with_pixels) e = sc.input(images, (size_t)image_offsets[m], &img->pixels, s);
    if (e == hipSuccess && with_pixels) e = sc.input(reinterpret_cast<const unsigned long long *>(image_offsets), (size_t)m + 1, &offsets, s);
    *d_tracks = reinterpret_cast<const int2 *>(t);
    img->offsets = offsets, img->dims = reinterpret_cast<const uint2 *>(dims);
    return e;
}

// The end of a call whose kernels wrote the body to d_out + header.size() (e: the launches' error): the body from the
// stand-in and the header from here, or, in the caller's device memory, the header by hipMemcpyAsync.
inline int finish_file_image(const char *what, CallScratch &sc, const std::string &header, uint8_t *out, uint8_t *d_out, uint64_t size,
                             hipError_t e, hipStream_t s)
{
    if (d_out != out) {
        if (e == hipSuccess) e = sc.copy_out(out + header.size(), d_out + header.size(), (size_t)(size - header.size()), s);
        if (e == hipSuccess) e = hipStreamSynchronize(s);
        if (e == hipSuccess) std::memcpy(out, header.data(), header.size());
    } else {
        if (e == hipSuccess && !header.empty()) e = hipMemcpyAsync(out, header.data(), header.size(), hipMemcpyHostToDevice, s);
        if (e == hipSuccess) e = hipStreamSynchronize(s);
    }
    if (e != hipSuccess) return device_error(what, e);
    return CVHIP_OK;
}

} // namespace cvhip
