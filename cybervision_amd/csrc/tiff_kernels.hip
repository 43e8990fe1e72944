// tiff_kernels.hip — cvhip_tiff_info / cvhip_tiff_decode: a strip TIFF file to Luma8 or RGB8 pixels, everything behind the IFD
// walk on the device.  The reference opens its SEM pairs with image::open(path)?.into_luma8() and cuts
// DatabarHeight rows (src/reconstruction.rs:40-60, 80-144); the pixels are DEFINED by tests/ref_tiff.py, whose decompressed
// samples are pinned to libtiff.  The host (tiff_common.hpp) walks the IFD and uploads the file's bytes up to the last
// strip's end and the strip table.
//
//   tiff_packbits_kernel  a wave per strip: the header chain is walked by every lane alike, 64 packets at a time, a lane
//                         keeping the packet of its number; then the wave expands packet after packet, a lane per byte
//   tiff_lzw_kernel       a wave per strip, 64 codes at a time.  Between two Clears the width of the c-th code depends on c
//                         alone, so a lane finds its code's bits by a closed form; a ballot finds the first Clear, EOI, end
//                         of input or code above the next entry.  The string of entry 258 + j is the earlier output of the
//                         j-th code since the Clear plus the byte behind it, so a code is a (distance, length) copy:
//                         lengths of codes that name entries of earlier batches come from a table in LDS, those that name
//                         entries of their own batch by pointer doubling over the lanes (6 shuffles); a wave prefix sum
//                         places them.  Then a lane per output byte follows its distances back to a literal of the batch
//                         or a byte of an earlier batch (the self-overlapping case j = c - 1 is one more step)
//   tiff_convert_kernel   a workgroup per result row: Predictor 2 undone by a scan per sample channel (wave scans, the
//                         waves' sums through LDS, a carry from chunk to chunk), then the row's bytes - WhiteIsZero,
//                         16 -> 8 bits, luma, the fourth sample dropped - as aligned dwords with single bytes at its ends
// An uncompressed file has no first pass: the convert kernel reads the strips where they lie.
#include <algorithm>
#include <cstring>
#include <vector>

#include "cvhip_internal.hpp"

#include "tiff_common.hpp"

namespace cvhip {
namespace {

namespace tc = tiff_common;

#include "tiff_decompress.inc"

// where row y of the file's rows lies: in the decompressed rows, or in its strip of the file
__device__ __forceinline__ const uint8_t *source_row(const TiffParams &P, const uint8_t *__restrict__ file, const uint32_t *__restrict__ offsets,
                                                     const uint8_t *raw, uint32_t y)
{
    if (P.compressed) return raw + (unsigned long long)y * P.row_bytes;
    return file + offsets[y / P.rps] + (unsigned long long)(y % P.rps) * P.row_bytes;
}

__global__ __launch_bounds__(BLOCK) void tiff_convert_kernel(const uint8_t *__restrict__ file, const uint32_t *__restrict__ offsets, TiffParams P,
                                                             const uint8_t *raw, uint8_t *summed, uint32_t channels, uint8_t *__restrict__ out,
                                                             const uint32_t *__restrict__ flags)
{
    __shared__ uint32_t wave_sum[BLOCK / WAVE][4];
    if (flags[FLAG_ERR]) return;
    const uint32_t y = blockIdx.x, tid = threadIdx.x, lane = tid % WAVE, wave = tid / WAVE;
    const uint8_t *row = source_row(P, file, offsets, raw, y);
    if (P.predictor == 2) {
        // horizontal differencing undone: per sample channel the running sum along the row, modulo 2^8 or 2^16
        uint8_t *to = summed + (unsigned long long)y * P.row_bytes;
        uint32_t carry[4] = {0, 0, 0, 0};
        for (uint32_t base = 0; base < P.width; base += BLOCK) {
            const uint32_t x = base + tid;
            uint32_t v[4] = {0, 0, 0, 0};
#pragma unroll
            for (uint32_t ch = 0; ch < 4; ch++)
                if (x < P.width && ch < P.spp) v[ch] = sample_at(P, row, x * P.spp + ch);
#pragma unroll
            for (int d = 1; d < WAVE; d <<= 1) {
#pragma unroll
                for (uint32_t ch = 0; ch < 4; ch++) {
                    const uint32_t t = __shfl_up(v[ch], d);
                    if ((int)lane >= d) v[ch] += t;
                }
            }
            if (lane == WAVE - 1) {
#pragma unroll
                for (uint32_t ch = 0; ch < 4; ch++) wave_sum[wave][ch] = v[ch];
            }
            __syncthreads();
#pragma unroll
            for (uint32_t ch = 0; ch < 4; ch++) {
                uint32_t before = carry[ch], all = carry[ch];
#pragma unroll
                for (uint32_t k = 0; k < BLOCK / WAVE; k++) {
                    if (k < wave) before += wave_sum[k][ch];
                    all += wave_sum[k][ch];
                }
                v[ch] += before, carry[ch] = all;
            }
            if (x < P.width) {
#pragma unroll
                for (uint32_t ch = 0; ch < 4; ch++) {
                    if (ch >= P.spp) continue;
                    const uint32_t e = x * P.spp + ch;
                    if (P.sample_bytes == 1) to[e] = (uint8_t)v[ch];
                    else to[2u * e] = (uint8_t)(P.little ? v[ch] : v[ch] >> 8), to[2u * e + 1u] = (uint8_t)(P.little ? v[ch] >> 8 : v[ch]);
                }
            }
            __syncthreads();
        }
        row = to;
    }
    // the row's bytes: single bytes up to the first 4-byte aligned address, whole dwords, single bytes behind the last
    const uint32_t bytes = P.width * channels;
    uint8_t *dst = out + (unsigned long long)y * bytes;
    const uint32_t lead = min(bytes, (uint32_t)((4u - (uint32_t)(reinterpret_cast<uintptr_t>(dst) & 3u)) & 3u));
    const uint32_t dwords = (bytes - lead) / 4u, tail = bytes - lead - 4u * dwords;
    for (uint32_t t = tid; t < dwords; t += BLOCK) {
        const uint32_t at = lead + 4u * t;
        uint32_t word = 0;
#pragma unroll
        for (uint32_t k = 0; k < 4; k++) word |= row_byte(P, row, channels, at + k) << (8u * k);
        *reinterpret_cast<uint32_t *>(dst + at) = word;
    }
    if (tid < lead + tail) {
        const uint32_t at = tid < lead ? tid : lead + 4u * dwords + (tid - lead);
        dst[at] = (uint8_t)row_byte(P, row, channels, at);
    }
}

thread_local uint64_t t_stats[4] = {0, 0, 0, 0}; // of the thread's last decode: strips, LZW codes read, Clears met, the longest string

} // namespace
} // namespace cvhip

using namespace cvhip;

extern "C" int cvhip_tiff_info(const uint8_t *file, uint64_t size, uint32_t *out_info, float *out_scale)
{
    if (!file || !out_info || !out_scale) return fail(CVHIP_ERR_INVALID, "tiff_info: null argument");
    tc::Header h;
    const int rc = tc::parse(file, (size_t)size, h);
    if (rc != tc::OK) return refused("tiff_info", rc == tc::UNSUPPORTED, h.error);
    out_info[0] = h.width, out_info[1] = h.height, out_info[2] = h.samples, out_info[3] = h.bits, out_info[4] = h.compression;
    out_info[5] = h.photometric, out_info[6] = h.predictor, out_info[7] = (uint32_t)h.strips.size(), out_info[8] = h.rows_per_strip;
    out_info[9] = h.focal_length_35mm, out_info[10] = h.databar_height, out_info[11] = (h.sem ? 1u : 0u) | (h.have_tilt ? 2u : 0u);
    out_scale[0] = h.scale[0], out_scale[1] = h.scale[1], out_scale[2] = h.tilt_angle;
    return CVHIP_OK;
}

extern "C" int cvhip_tiff_last_stats(uint64_t *out_stats)
{
    if (!out_stats) return fail(CVHIP_ERR_INVALID, "tiff_last_stats: null argument");
    for (int k = 0; k < 4; k++) out_stats[k] = t_stats[k];
    return CVHIP_OK;
}

extern "C" int cvhip_tiff_decode(cvhip_device *dev, const uint8_t *file, uint64_t size, uint32_t format, uint32_t drop_rows, uint8_t *out,
                                 uint64_t cap, uint64_t *out_size)
{
    if (!dev || !file || !out_size || (cap && !out)) return fail(CVHIP_ERR_INVALID, "tiff_decode: null argument");
    if (format != CVHIP_IMAGE_LUMA8 && format != CVHIP_IMAGE_RGB8) return fail(CVHIP_ERR_INVALID, "tiff_decode: format is not CVHIP_IMAGE_LUMA8 or CVHIP_IMAGE_RGB8");
    tc::Header h;
    const int rc = tc::parse(file, (size_t)size, h);
    if (rc != tc::OK) return refused("tiff_decode", rc == tc::UNSUPPORTED, h.error);
    if (drop_rows == CVHIP_TIFF_DROP_DATABAR) drop_rows = h.databar_height;
    if (drop_rows >= h.height) return fail(CVHIP_ERR_INVALID, "tiff_decode: drop_rows leaves no row");
    const uint32_t channels = format == CVHIP_IMAGE_RGB8 ? 3u : 1u;
    const unsigned long long bytes = (unsigned long long)h.width * (h.height - drop_rows) * channels;
    *out_size = bytes;
    if (!cap) return CVHIP_OK;
    if (cap < bytes) return fail(CVHIP_ERR_INVALID, "tiff_decode: the buffer is smaller than the image");

    const uint32_t nstrips = (uint32_t)h.strips.size();
    TiffParams P{};
    P.width = h.width, P.height = h.height, P.rows_out = h.height - drop_rows, P.spp = h.samples, P.sample_bytes = h.bits / 8;
    P.little = h.little ? 1u : 0u, P.invert = h.photometric == 0 ? 1u : 0u, P.predictor = h.predictor, P.rps = h.rows_per_strip;
    P.compressed = h.compression != tc::COMPRESSION_NONE ? 1u : 0u, P.row_bytes = (uint32_t)h.row_bytes;
    // ---- the one upload: the strip table, then the file's bytes up to the last strip's end
    unsigned long long file_bytes = 0;
    for (const tc::Strip &strip : h.strips) file_bytes = std::max<unsigned long long>(file_bytes, (unsigned long long)strip.offset + strip.count);
    const size_t table_bytes = ((size_t)nstrips * 2 * sizeof(uint32_t) + 15) / 16 * 16;
    std::vector<uint8_t> blob(table_bytes + (size_t)file_bytes);
    uint32_t *table = reinterpret_cast<uint32_t *>(blob.data());
    for (uint32_t s = 0; s < nstrips; s++) table[s] = h.strips[s].offset, table[nstrips + s] = h.strips[s].count;
    std::memcpy(blob.data() + table_bytes, file, (size_t)file_bytes);

    CVHIP_TRY_HIP(hipSetDevice(dev->d.ordinal));
    hipStream_t s = dev->d.stream;
    CallScratch sc;
    const size_t raw_bytes = (size_t)h.row_bytes * h.height; // the decompressed rows, or the rows with Predictor 2 undone
    const bool need_raw = P.compressed || P.predictor == 2;
    Carver carve;
    const size_t at_blob = carve.reserve(blob.size()), at_flags = carve.reserve(FLAGS * sizeof(uint32_t)), at_raw = carve.reserve(need_raw ? raw_bytes : 0);
    uint8_t *arena = nullptr, *d_out = nullptr;
    hipError_t e = sc.alloc(&arena, carve.total);
    if (e == hipSuccess) e = sc.output(out, (size_t)bytes, &d_out);
    if (e != hipSuccess) return device_error("tiff_decode", e);
    uint32_t *flags = reinterpret_cast<uint32_t *>(arena + at_flags), h_flags[FLAGS] = {0, 0, 0, 0};
    const uint32_t *d_offsets = reinterpret_cast<const uint32_t *>(arena + at_blob), *d_counts = d_offsets + nstrips;
    const uint8_t *d_file = arena + at_blob + table_bytes;
    uint8_t *raw = arena + at_raw;
    e = hipMemcpyAsync(arena + at_blob, blob.data(), blob.size(), hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipMemsetAsync(flags, 0, FLAGS * sizeof(uint32_t), s);
    if (e != hipSuccess) return device_error("tiff_decode", e);
    if (h.compression == tc::COMPRESSION_LZW)
        hipLaunchKernelGGL(tiff_lzw_kernel, dim3(nstrips), dim3(WAVE), 0, s, d_file, d_offsets, d_counts, P, raw, flags);
    else if (h.compression == tc::COMPRESSION_PACKBITS)
        hipLaunchKernelGGL(tiff_packbits_kernel, dim3(nstrips), dim3(WAVE), 0, s, d_file, d_offsets, d_counts, P, raw, flags);
    hipLaunchKernelGGL(tiff_convert_kernel, dim3(P.rows_out), dim3(BLOCK), 0, s, d_file, d_offsets, P, raw, raw, channels, d_out, flags);
    e = hipGetLastError();
    if (e == hipSuccess) e = hipMemcpyAsync(h_flags, flags, sizeof(h_flags), hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) return device_error("tiff_decode", e);
    t_stats[0] = nstrips, t_stats[1] = h_flags[FLAG_CODES], t_stats[2] = h_flags[FLAG_CLEARS], t_stats[3] = h_flags[FLAG_LONGEST];
    if (h_flags[FLAG_ERR])
        return fail(CVHIP_ERR_INVALID, h.compression == tc::COMPRESSION_LZW
                                           ? "tiff_decode: LZW: a code above the next entry, or EOI or the end of the input before the rows are full"
                                           : "tiff_decode: PackBits: the input ends before the rows are full");
    e = sc.copy_out(out, d_out, (size_t)bytes, s);
    if (e == hipSuccess) e = sc.drain(s);
    if (e != hipSuccess) return device_error("tiff_decode", e);
    return CVHIP_OK;
}
