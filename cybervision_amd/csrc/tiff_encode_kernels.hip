// tiff_encode_kernels.hip — cvhip_tiff_encode: the classic little-endian TIFF file of an 8-bit image with 1 to 4 channels, made
// on the device.  The reference saves its depth map with img.save (src/output.rs:1141), and a path that ends in
// .tif makes that a TIFF file.  The file is defined by tests/ref_tiff_out.py: strips of RowsPerStrip rows, uncompressed, TIFF 6.0
// LZW as libtiff writes it (pinned to Pillow byte for byte by tests/test_tiff_out_ref.py) or PackBits row by row; Predictor 2
// with LZW.  The host composes the 8-byte header and the IFD (tiff_encode_common.hpp).
//
//   tiff_lzw_kernel      a wave a strip.  The strip is taken LZW_CHUNK bytes at a time: all lanes load the bytes into LDS with
//                        Predictor 2 applied; lane 0 walks them against the (prefix, byte) -> code hash table in LDS and writes
//                        the codes with their widths to LDS - the table and the pending string carry over from chunk to chunk;
//                        all lanes empty the table when a Clear left; then all lanes pack the codes, 64 at a time: a wave scan
//                        of the widths gives the bit offsets, the bits are ORed into LDS words and whole dwords leave to the
//                        strip's scratch.  Every loop is bounded by the chunk's bytes, its codes or the table's slots.
//   tiff_packbits_kernel a lane a row, the greedy walk of tiff_encode_common.hpp into the row's scratch
//   tiff_sizes_kernel    a lane a strip: its bytes (the rows' sum for PackBits, with each row's place in its strip) and its
//                        bytes with the padding to an even offset of the next strip
//   (launch_scan_u64)    places the strips
//   tiff_table_kernel    a lane a strip: its StripOffsets and StripByteCounts values and its padding byte
//   tiff_copy_kernel     a workgroup a unit (a strip; a row for PackBits): its bytes to their place in `out`, at any
//                        alignment: aligned dwords, bytes at the two ends
#include <cstring>

#include "cvhip_internal.hpp"

#include "tiff_encode_common.hpp"

namespace cvhip {
namespace {

namespace te = tiff_encode_common;

constexpr int WG = 256;
constexpr int WAVE = 64;
constexpr uint32_t OUT_WORDS = (te::LZW_CHUNK_CODES * 12 + 31) / 32 + 2; // a chunk's codes and the word carried over

struct Shape {
    uint32_t row_bytes, channels, predictor, rows_per_strip, height, strips, compression;
};
__device__ __forceinline__ uint32_t rows_of(const Shape &g, uint32_t strip) { return min(g.rows_per_strip, g.height - strip * g.rows_per_strip); }

// counters[0] += codes, counters[1] += Clears, counters[3 .. 5] += the ticks (wall_clock64, 100 MHz) this wave spent loading,
// walking and packing.  sizes[strip] = the bytes of the strip's stream at scratch + strip * stride
// (stride: a multiple of 4 that holds worst_strip() rounded up to whole dwords).
__global__ __launch_bounds__(WAVE) void tiff_lzw_kernel(const uint8_t *__restrict__ pixels, Shape g, uint8_t *__restrict__ scratch,
                                                        unsigned long long stride, uint32_t *__restrict__ sizes,
                                                        unsigned long long *__restrict__ counters)
{
    __shared__ uint32_t s_table[te::LZW_SLOTS];
    __shared__ uint32_t s_out[OUT_WORDS];
    __shared__ uint16_t s_codes[te::LZW_CHUNK_CODES]; // code | (width - 9) << 12
    __shared__ uint8_t s_bytes[te::LZW_CHUNK];
    __shared__ uint32_t s_walk[3]; // lane 0 -> all: where the walk stands, whether a Clear left, the chunk's codes
    const uint32_t lane = threadIdx.x;
    for (uint32_t strip = blockIdx.x; strip < g.strips; strip += gridDim.x) {
        const unsigned long long first = (unsigned long long)strip * g.rows_per_strip * g.row_bytes;
        const uint32_t n = rows_of(g, strip) * g.row_bytes; // < 2^31
        uint32_t *dst = reinterpret_cast<uint32_t *>(scratch + strip * stride);
        for (uint32_t k = lane; k < te::LZW_SLOTS; k += WAVE) s_table[k] = te::LZW_EMPTY;
        for (uint32_t k = lane; k < OUT_WORDS; k += WAVE) s_out[k] = 0;
        te::LzwState st;
        unsigned long long words_out = 0; // dwords of the strip's stream that have left
        uint32_t carry_bits = 0;          // bits of s_out[0] that are taken
        uint32_t n_codes = 0, n_clears = 0;
        unsigned long long ticks_load = 0, ticks_walk = 0, ticks_pack = 0;
        const uint32_t chunks = (n + te::LZW_CHUNK - 1) / te::LZW_CHUNK; // >= 1
        for (uint32_t chunk = 0; chunk < chunks; chunk++) {
            const uint32_t begin = chunk * te::LZW_CHUNK, len = min(te::LZW_CHUNK, n - begin);
            __syncthreads();
            const unsigned long long t0 = wall_clock64();
            for (uint32_t k = lane; k < len; k += WAVE) {
                const unsigned long long at = first + begin + k;
                uint32_t v = pixels[at];
                if (g.predictor == 2 && (begin + k) % g.row_bytes >= g.channels) v -= pixels[at - g.channels];
                s_bytes[k] = (uint8_t)v;
            }
            __syncthreads();
            const unsigned long long t1 = wall_clock64();
            // ---- the walk: lane 0, interrupted where the table is to be emptied (at most len + 1 rounds: each takes a byte)
            uint32_t pos = 0, codes = 0;
            auto put = [&](uint32_t code, uint32_t width) {
                if (codes < te::LZW_CHUNK_CODES) s_codes[codes] = (uint16_t)(code | (width - 9u) << 12);
                codes++;
                n_codes++;
                if (code == te::LZW_CLEAR) n_clears++;
            };
            if (lane == 0 && chunk == 0) put(te::LZW_CLEAR, 9);
            for (uint32_t round = 0; round <= len; round++) {
                if (lane == 0) {
                    bool clear = false;
                    for (; pos < len && !clear; pos++) clear = te::lzw_byte(s_table, st, s_bytes[pos], put);
                    s_walk[0] = pos, s_walk[1] = clear ? 1u : 0u;
                }
                __syncthreads();
                pos = s_walk[0];
                const bool clear = s_walk[1] != 0;
                __syncthreads();
                if (clear) {
                    for (uint32_t k = lane; k < te::LZW_SLOTS; k += WAVE) s_table[k] = te::LZW_EMPTY;
                    __syncthreads();
                }
                if (pos >= len) break;
            }
            if (lane == 0) {
                if (chunk + 1 == chunks) te::lzw_finish(st, put);
                s_walk[2] = codes;
            }
            __syncthreads();
            codes = s_walk[2];
            codes = min(codes, te::LZW_CHUNK_CODES);
            const unsigned long long t2 = wall_clock64();
            // ---- the packing: bit b of the stream is bit 31 - b % 32 of word b / 32 (swapped into byte order when it leaves)
            uint32_t bit = carry_bits;
            for (uint32_t base = 0; base < codes; base += WAVE) {
                const uint32_t k = base + lane;
                const uint32_t entry = k < codes ? s_codes[k] : 0u;
                const uint32_t width = k < codes ? 9u + (entry >> 12) : 0u, code = entry & 0xFFFu;
                uint32_t incl = width;
#pragma unroll
                for (int s = 1; s < WAVE; s <<= 1) {
                    const uint32_t t = __shfl_up(incl, s, WAVE);
                    if ((int)lane >= s) incl += t;
                }
                if (width) {
                    const uint32_t at = bit + incl - width, word = at >> 5, off = at & 31u;
                    if (off + width <= 32)
                        atomicOr(&s_out[word], code << (32u - off - width));
                    else {
                        atomicOr(&s_out[word], code >> (off + width - 32u));
                        atomicOr(&s_out[word + 1], code << (64u - off - width));
                    }
                }
                bit += __shfl(incl, WAVE - 1, WAVE);
            }
            __syncthreads();
            const bool last = chunk + 1 == chunks;
            const uint32_t whole = bit >> 5, leaving = last ? (bit + 31u) >> 5 : whole;
            for (uint32_t k = lane; k < leaving; k += WAVE) dst[words_out + k] = __builtin_bswap32(s_out[k]);
            __syncthreads();
            const uint32_t kept = s_out[whole < OUT_WORDS ? whole : 0];
            __syncthreads();
            for (uint32_t k = lane; k <= whole && k < OUT_WORDS; k += WAVE) s_out[k] = 0;
            __syncthreads();
            if (lane == 0 && !last) s_out[0] = kept;
            words_out += whole;
            carry_bits = bit & 31u;
            ticks_load += t1 - t0, ticks_walk += t2 - t1, ticks_pack += wall_clock64() - t2;
            if (last && lane == 0) {
                sizes[strip] = (uint32_t)(words_out * 4 + (carry_bits + 7u) / 8u);
                atomicAdd(&counters[0], (unsigned long long)n_codes);
                atomicAdd(&counters[1], (unsigned long long)n_clears);
                atomicAdd(&counters[3], ticks_load);
                atomicAdd(&counters[4], ticks_walk);
                atomicAdd(&counters[5], ticks_pack);
            }
        }
        __syncthreads();
    }
}

// sizes[row] = the bytes of the row's packets at scratch + row * stride; counters[2] += the packets
__global__ __launch_bounds__(WG) void tiff_packbits_kernel(const uint8_t *__restrict__ pixels, Shape g, uint8_t *__restrict__ scratch,
                                                           unsigned long long stride, uint32_t *__restrict__ sizes,
                                                           unsigned long long *__restrict__ counters)
{
    for (uint32_t row = blockIdx.x * WG + threadIdx.x; row < g.height; row += gridDim.x * WG) {
        uint32_t packets = 0;
        sizes[row] = te::packbits_row(pixels + (unsigned long long)row * g.row_bytes, g.row_bytes, scratch + row * stride, packets);
        atomicAdd(&counters[2], (unsigned long long)packets);
    }
}

// unit_sizes: of the strips (LZW) or of the rows (PackBits; row_at[row] = the bytes of its strip's rows before it).
// strip_sizes[s] = the strip's bytes; padded[s] = with the byte that brings the next strip to an even offset.
__global__ __launch_bounds__(WG) void tiff_sizes_kernel(Shape g, const uint32_t *__restrict__ unit_sizes, uint32_t *__restrict__ row_at,
                                                        uint32_t *__restrict__ strip_sizes, unsigned long long *__restrict__ padded)
{
    for (uint32_t s = blockIdx.x * WG + threadIdx.x; s < g.strips; s += gridDim.x * WG) {
        uint32_t size;
        if (g.compression == te::COMPRESSION_NONE)
            size = rows_of(g, s) * g.row_bytes;
        else if (g.compression == te::COMPRESSION_LZW)
            size = unit_sizes[s];
        else {
            size = 0;
            const uint32_t row0 = s * g.rows_per_strip, rows = rows_of(g, s);
            for (uint32_t r = 0; r < rows; r++) row_at[row0 + r] = size, size += unit_sizes[row0 + r];
        }
        strip_sizes[s] = size;
        padded[s] = (unsigned long long)size + (s + 1 < g.strips ? size & 1u : 0u);
    }
}

__device__ __forceinline__ void store_le32(uint8_t *p, uint32_t v)
{
    p[0] = (uint8_t)v, p[1] = (uint8_t)(v >> 8), p[2] = (uint8_t)(v >> 16), p[3] = (uint8_t)(v >> 24);
}
// starts[s]: where strip s begins behind data_at.  The two arrays (strips > 1) and the padding bytes.
__global__ __launch_bounds__(WG) void tiff_table_kernel(Shape g, const uint32_t *__restrict__ strip_sizes, const unsigned long long *__restrict__ starts,
                                                        uint32_t data_at, uint32_t offsets_at, uint32_t counts_at, uint8_t *__restrict__ out)
{
    for (uint32_t s = blockIdx.x * WG + threadIdx.x; s < g.strips; s += gridDim.x * WG) {
        const unsigned long long at = data_at + starts[s];
        const uint32_t size = strip_sizes[s];
        if (g.strips > 1) {
            store_le32(out + offsets_at + 4ull * s, (uint32_t)at);
            store_le32(out + counts_at + 4ull * s, size);
        }
        if (s + 1 < g.strips && (size & 1u)) out[at + size] = 0;
    }
}

// Unit u (a strip; with PackBits a row): `size` bytes from src to dst, dst at any alignment.
__global__ __launch_bounds__(WG) void tiff_copy_kernel(Shape g, const uint8_t *__restrict__ source, unsigned long long stride,
                                                       const uint32_t *__restrict__ unit_sizes, const uint32_t *__restrict__ row_at,
                                                       const uint32_t *__restrict__ strip_sizes, const unsigned long long *__restrict__ starts,
                                                       uint8_t *__restrict__ data)
{
    const bool rows = g.compression == te::COMPRESSION_PACKBITS;
    const uint32_t units = rows ? g.height : g.strips;
    for (uint32_t u = blockIdx.x; u < units; u += gridDim.x) {
        const uint8_t *src = source + u * stride;
        const uint32_t size = rows ? unit_sizes[u] : strip_sizes[u];
        uint8_t *dst = data + (rows ? starts[u / g.rows_per_strip] + row_at[u] : starts[u]);
        const uint32_t front = (uint32_t)((4u - (reinterpret_cast<uintptr_t>(dst) & 3u)) & 3u); // bytes in front of the first aligned dword
        const uint32_t head = min(front, size), body = (size - head) / 4;
        if (threadIdx.x < head) dst[threadIdx.x] = src[threadIdx.x];
        uint32_t *dst32 = reinterpret_cast<uint32_t *>(dst + head);
        const uint8_t *s = src + head;
        for (uint32_t j = threadIdx.x; j < body; j += WG)
            dst32[j] = (uint32_t)s[4 * j] | (uint32_t)s[4 * j + 1] << 8 | (uint32_t)s[4 * j + 2] << 16 | (uint32_t)s[4 * j + 3] << 24;
        const uint32_t done = head + 4 * body;
        if (threadIdx.x < size - done) dst[done + threadIdx.x] = src[done + threadIdx.x];
    }
}

thread_local uint64_t t_stats[4] = {0, 0, 0, 0}; // of the thread's last encode: strips, LZW codes, Clear codes, PackBits packets
thread_local uint64_t t_phases[3] = {0, 0, 0};   // and the LZW waves' ticks, summed over the strips: loading, walking, packing

} // namespace
} // namespace cvhip

using namespace cvhip;

extern "C" int cvhip_tiff_encode_last_stats(uint64_t *out_stats)
{
    if (!out_stats) return fail(CVHIP_ERR_INVALID, "tiff_encode_last_stats: null argument");
    for (int k = 0; k < 4; k++) out_stats[k] = t_stats[k];
    return CVHIP_OK;
}

extern "C" int cvhip_tiff_encode_last_phases(uint64_t *out_ticks)
{
    if (!out_ticks) return fail(CVHIP_ERR_INVALID, "tiff_encode_last_phases: null argument");
    for (int k = 0; k < 3; k++) out_ticks[k] = t_phases[k];
    return CVHIP_OK;
}

extern "C" int cvhip_tiff_encode(cvhip_device *dev, const uint8_t *pixels, uint32_t width, uint32_t height, uint32_t channels, uint32_t compression,
                                 uint32_t predictor, uint32_t rows_per_strip, uint8_t *out, uint64_t cap, uint64_t *out_size, uint64_t *out_sections)
{
    if (!dev || !pixels || !out_size || (cap && !out)) return fail(CVHIP_ERR_INVALID, "tiff_encode: null argument");
    te::Layout l;
    const te::Refusal refusal = te::plan(width, height, channels, compression, predictor, rows_per_strip, l);
    if (refusal != te::ACCEPTED)
        return fail(refusal == te::REFUSED_INVALID ? CVHIP_ERR_INVALID : CVHIP_ERR_UNSUPPORTED, std::string("tiff_encode: ") + l.why);
    const Shape g = {l.row_bytes, channels, predictor, l.rows_per_strip, height, l.strips, compression};
    const bool lzw = compression == te::COMPRESSION_LZW, packbits = compression == te::COMPRESSION_PACKBITS;
    CVHIP_TRY_HIP(hipSetDevice(dev->d.ordinal));
    hipStream_t s = dev->d.stream;
    CallScratch sc;
    const uint8_t *d_pixels = nullptr;
    // the compressed units at a worst-case stride, so that sizing and writing compress once: strips (LZW) or rows (PackBits)
    const unsigned long long units = lzw ? l.strips : packbits ? height : 0;
    const unsigned long long stride =
        lzw ? ((te::worst_strip(compression, l.rows_per_strip, l.row_bytes) + 3) / 4 + 1) * 4 : packbits ? te::worst_strip(compression, 1, l.row_bytes) : 0;
    uint8_t *scratch = nullptr;
    uint32_t *unit_sizes = nullptr, *row_at = nullptr, *strip_sizes = nullptr;
    unsigned long long *starts = nullptr, *counters = nullptr;
    hipError_t e = sc.input(pixels, (size_t)height * l.row_bytes, &d_pixels, s);
    if (e == hipSuccess) e = sc.alloc(&scratch, (size_t)(units * stride));
    if (e == hipSuccess) e = sc.alloc(&unit_sizes, (size_t)units);
    if (e == hipSuccess) e = sc.alloc(&row_at, packbits ? (size_t)height : 0);
    if (e == hipSuccess) e = sc.alloc(&strip_sizes, (size_t)l.strips);
    if (e == hipSuccess) e = sc.alloc(&starts, (size_t)l.strips + 1);
    if (e == hipSuccess) e = sc.alloc(&counters, 6);
    if (e == hipSuccess) e = hipMemsetAsync(counters, 0, 6 * sizeof(unsigned long long), s);
    if (e != hipSuccess) return device_error("tiff_encode", e);
    const dim3 wg(WG), strips_grid(grid_for(l.strips));
    if (lzw)
        hipLaunchKernelGGL(tiff_lzw_kernel, dim3(std::min<uint32_t>(l.strips, CVHIP_MESH_GRID_LANES / WAVE)), dim3(WAVE), 0, s, d_pixels, g, scratch, stride,
                           unit_sizes, counters);
    if (packbits) hipLaunchKernelGGL(tiff_packbits_kernel, dim3(grid_for(height)), wg, 0, s, d_pixels, g, scratch, stride, unit_sizes, counters);
    hipLaunchKernelGGL(tiff_sizes_kernel, strips_grid, wg, 0, s, g, unit_sizes, row_at, strip_sizes, starts);
    launch_scan_u64(starts, l.strips, starts + l.strips, s);
    unsigned long long h_counters[6] = {0, 0, 0, 0, 0, 0}, data_bytes = 0;
    uint32_t first_count = 0;
    e = hipGetLastError();
    if (e == hipSuccess) e = hipMemcpyAsync(&data_bytes, starts + l.strips, sizeof(data_bytes), hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipMemcpyAsync(&first_count, strip_sizes, sizeof(first_count), hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipMemcpyAsync(h_counters, counters, sizeof(h_counters), hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) return device_error("tiff_encode", e);
    const uint64_t size = (uint64_t)l.data_at + data_bytes;
    if (size >= (1ull << 32)) return fail(CVHIP_ERR_UNSUPPORTED, "tiff_encode: a file of 2^32 bytes or more");
    t_stats[0] = l.strips, t_stats[1] = h_counters[0], t_stats[2] = h_counters[1], t_stats[3] = h_counters[2];
    t_phases[0] = h_counters[3], t_phases[1] = h_counters[4], t_phases[2] = h_counters[5];
    *out_size = size;
    if (out_sections) out_sections[0] = l.data_at, out_sections[1] = data_bytes, out_sections[2] = 0;
    if (!cap) return CVHIP_OK;
    if (cap < size) return fail(CVHIP_ERR_INVALID, "tiff_encode: the buffer is smaller than the file image");
    // ---- the file image: the header and the IFD composed here, the two arrays and the strips by the kernels
    uint8_t *d_out = nullptr;
    e = sc.output(out, (size_t)size, &d_out);
    if (e != hipSuccess) return device_error("tiff_encode", e);
    const std::vector<uint8_t> header = te::header(l, first_count);
    e = hipMemcpyAsync(d_out, header.data(), header.size(), hipMemcpyHostToDevice, s);
    if (e != hipSuccess) return device_error("tiff_encode", e);
    hipLaunchKernelGGL(tiff_table_kernel, strips_grid, wg, 0, s, g, strip_sizes, starts, l.data_at, l.offsets_at, l.counts_at, d_out);
    const uint32_t copy_units = packbits ? height : l.strips;
    hipLaunchKernelGGL(tiff_copy_kernel, dim3(std::min<uint32_t>(copy_units, CVHIP_MESH_GRID_LANES / WG)), wg, 0, s, g, lzw || packbits ? scratch : d_pixels,
                       lzw || packbits ? stride : (unsigned long long)l.rows_per_strip * l.row_bytes, unit_sizes, row_at, strip_sizes, starts,
                       d_out + l.data_at);
    e = hipGetLastError();
    if (e == hipSuccess) e = sc.copy_out(out, d_out, (size_t)size, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) return device_error("tiff_encode", e);
    return CVHIP_OK;
}
