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

constexpr int WAVE = 64;
constexpr uint32_t BLOCK = 256;
constexpr uint32_t FLAG_ERR = 0, FLAG_CODES = 1, FLAG_CLEARS = 2, FLAG_LONGEST = 3, FLAGS = 4;
constexpr uint32_t LZW_ENTRIES = 4096;
// libtiff's table has 5119 slots and it goes on filling them when entry 4095 is taken (no code can name those); the code
// that finds no slot left - 4862 codes after the Clear - is an error there, and so here (tests/ref_tiff.py: MAX_CODES)
constexpr uint32_t LZW_MAX_CODES = 5119 - 257;

struct TiffParams {
    uint32_t width, height, rows_out, spp, sample_bytes, little, invert, predictor, rps, compressed;
    uint32_t row_bytes; // of a row in the file (below 2^31)
};

__device__ __forceinline__ uint32_t strip_rows(const TiffParams &P, uint32_t s) { return min(P.rps, P.height - s * P.rps); }

__global__ __launch_bounds__(WAVE) void tiff_packbits_kernel(const uint8_t *__restrict__ file, const uint32_t *__restrict__ offsets,
                                                             const uint32_t *__restrict__ counts, TiffParams P, uint8_t *__restrict__ raw,
                                                             uint32_t *__restrict__ flags)
{
    const uint32_t s = blockIdx.x, lane = threadIdx.x;
    const uint8_t *in = file + offsets[s];
    const uint32_t n = counts[s], need = strip_rows(P, s) * P.row_bytes;
    uint8_t *dst = raw + (unsigned long long)s * P.rps * P.row_bytes;
    uint32_t ipos = 0, opos = 0;
    while (opos < need) {
        uint32_t my_src = 0, my_out = 0, my_len = 0, my_run = 0, packets = 0;
        bool err = false;
        for (; packets < (uint32_t)WAVE && opos < need; packets++) {
            if (ipos >= n) {
                err = true;
                break;
            }
            const uint32_t header = in[ipos++];
            uint32_t len = 0, run = 0;
            if (header < 128u) {
                len = header + 1u;
                if (ipos + len > n) {
                    err = true;
                    break;
                }
            } else if (header > 128u) {
                len = 257u - header, run = 1u;
                if (ipos >= n) {
                    err = true;
                    break;
                }
            }
            if (lane == packets) my_src = ipos, my_out = opos, my_len = len, my_run = run;
            ipos += run ? (len ? 1u : 0u) : len;
            opos += len;
        }
        for (uint32_t p = 0; p < packets; p++) {
            const uint32_t src = __shfl(my_src, (int)p), out = __shfl(my_out, (int)p), len = __shfl(my_len, (int)p), run = __shfl(my_run, (int)p);
            for (uint32_t b = lane; b < len && out + b < need; b += WAVE) dst[out + b] = in[run ? src : src + b];
        }
        if (err) {
            if (lane == 0) atomicOr(&flags[FLAG_ERR], 1u);
            return;
        }
    }
}

// the bits of the codes 0 .. c - 1 after a Clear: code c is read while the next free entry is 257 + c, 9 bits wide while
// that is below 511, 10 below 1023, 11 below 2047, then 12
__device__ __forceinline__ unsigned long long lzw_bits_before(uint32_t c)
{
    return 9ull * min(c, 254u) + 10ull * min(c > 254u ? c - 254u : 0u, 512u) + 11ull * min(c > 766u ? c - 766u : 0u, 1024u) +
           12ull * (c > 1790u ? c - 1790u : 0u);
}
__device__ __forceinline__ uint32_t lzw_width(uint32_t c) { return c < 254u ? 9u : c < 766u ? 10u : c < 1790u ? 11u : 12u; }

__global__ __launch_bounds__(WAVE) void tiff_lzw_kernel(const uint8_t *__restrict__ file, const uint32_t *__restrict__ offsets,
                                                        const uint32_t *__restrict__ counts, TiffParams P, uint8_t *raw, uint32_t *__restrict__ flags)
{
    __shared__ uint32_t t_pos[LZW_ENTRIES]; // of the c-th code since the Clear: where its string begins in the strip's output
    __shared__ uint16_t t_len[LZW_ENTRIES]; // and its length (at most 3839)
    __shared__ uint32_t b_pos[WAVE + 1], b_dist[WAVE]; // of the batch: where a code's output begins; how far back its source lies (0: a literal)
    __shared__ uint8_t b_val[WAVE];
    const uint32_t s = blockIdx.x, lane = threadIdx.x;
    const uint8_t *in = file + offsets[s];
    const uint32_t n = counts[s], need = strip_rows(P, s) * P.row_bytes;
    const unsigned long long total_bits = 8ull * n;
    uint8_t *dst = raw + (unsigned long long)s * P.rps * P.row_bytes;
    unsigned long long bit = 0;
    uint32_t c0 = 0, outpos = 0, codes = 0, clears = 0, longest = 0;
    bool bad = false;
    while (outpos < need) {
        const uint32_t c = c0 + lane, w = lzw_width(c);
        const unsigned long long b = bit + (lzw_bits_before(c) - lzw_bits_before(c0));
        const bool past = b + w > total_bits;
        uint32_t code = 0;
        if (!past) {
            const unsigned long long i = b >> 3;
            const uint32_t word = (uint32_t)in[i] << 16 | (i + 1 < n ? (uint32_t)in[i + 1] : 0u) << 8 | (i + 2 < n ? (uint32_t)in[i + 2] : 0u);
            code = (word >> (24u - w - (uint32_t)(b & 7u))) & ((1u << w) - 1u);
        }
        const bool special = past || code == 256u || code == 257u;
        const uint32_t j = code - 258u;
        // above the next entry (behind a Clear only a literal), or libtiff's table overflow
        const bool invalid = !special && ((code >= 258u && j >= c) || c >= LZW_MAX_CODES);
        const unsigned long long stop = __ballot(special || invalid);
        const uint32_t f = stop ? (uint32_t)__ffsll((long long)stop) - 1u : (uint32_t)WAVE;
        const bool active = lane < f;
        int r = -1;
        uint32_t a = 0, src = 0;
        if (active) {
            if (code < 256u) a = 1;
            else if (j < c0) a = (uint32_t)t_len[j] + 1u, src = t_pos[j];
            else r = (int)(j - c0), a = 1;
        }
        const int named = r;
#pragma unroll
        for (int round = 0; round < 6; round++) { // len = len(the lane named) + 1, the chains halved per round
            const uint32_t ra = __shfl(a, r < 0 ? (int)lane : r);
            const int rr = __shfl(r, r < 0 ? (int)lane : r);
            if (r >= 0) a += ra, r = rr;
        }
        uint32_t incl = a;
#pragma unroll
        for (int d = 1; d < WAVE; d <<= 1) {
            const uint32_t t = __shfl_up(incl, d);
            if ((int)lane >= d) incl += t;
        }
        const uint32_t pos = outpos + incl - a, end = outpos + __shfl(incl, WAVE - 1);
        const uint32_t named_pos = __shfl(pos, named < 0 ? (int)lane : named);
        if (named >= 0) src = named_pos;
        if (active && c < LZW_ENTRIES) t_pos[c] = pos, t_len[c] = (uint16_t)a;
        b_pos[lane] = active ? pos : end;
        if (lane == 0) b_pos[WAVE] = end;
        b_dist[lane] = (active && code >= 258u) ? pos - src : 0u;
        b_val[lane] = (uint8_t)code;
        const bool counted = active && pos < need;
        codes += (uint32_t)__popcll(__ballot(counted));
        if (counted) longest = max(longest, a);
        __syncthreads();
        const uint32_t limit = min(end, need);
        for (uint32_t o = outpos + lane; o < limit; o += WAVE) {
            uint32_t p = o, byte;
            for (;;) {
                if (p < outpos) {
                    byte = dst[p];
                    break;
                }
                uint32_t k = 0;
#pragma unroll
                for (uint32_t step = 32; step; step >>= 1)
                    if (b_pos[k + step] <= p) k += step;
                const uint32_t dist = b_dist[k];
                if (!dist) {
                    byte = b_val[k];
                    break;
                }
                p -= dist;
            }
            dst[o] = (uint8_t)byte;
        }
        __syncthreads(); // the batch's bytes are the next batch's sources; its table entries and b_* are free again
        if (end >= need) break;
        outpos = end;
        if (f == (uint32_t)WAVE) {
            bit += lzw_bits_before(c0 + WAVE) - lzw_bits_before(c0);
            c0 += WAVE;
            continue;
        }
        const bool f_past = __shfl((int)past, (int)f) != 0;
        const uint32_t f_code = __shfl(code, (int)f), f_lo = __shfl((uint32_t)(b + w), (int)f), f_hi = __shfl((uint32_t)((b + w) >> 32), (int)f);
        if (!f_past && f_code == 256u) {
            clears++, codes++;
            bit = (unsigned long long)f_hi << 32 | f_lo;
            c0 = 0;
            continue;
        }
        bad = true; // EOI, the end of the input or a code above the next entry before the rows are full
        break;
    }
    if (bad && lane == 0) atomicOr(&flags[FLAG_ERR], 1u);
    if (lane == 0) {
        atomicAdd(&flags[FLAG_CODES], codes);
        atomicAdd(&flags[FLAG_CLEARS], clears);
    }
    if (longest) atomicMax(&flags[FLAG_LONGEST], longest);
}

// where row y of the file's rows lies: in the decompressed rows, or in its strip of the file
__device__ __forceinline__ const uint8_t *source_row(const TiffParams &P, const uint8_t *__restrict__ file, const uint32_t *__restrict__ offsets,
                                                     const uint8_t *raw, uint32_t y)
{
    if (P.compressed) return raw + (unsigned long long)y * P.row_bytes;
    return file + offsets[y / P.rps] + (unsigned long long)(y % P.rps) * P.row_bytes;
}

// sample e of a row, an integer in the file's byte order
__device__ __forceinline__ uint32_t sample_at(const TiffParams &P, const uint8_t *row, uint32_t e)
{
    if (P.sample_bytes == 1) return row[e];
    const uint32_t first = row[2u * e], second = row[2u * e + 1u];
    return P.little ? first | second << 8 : first << 8 | second;
}

// result byte `at` of a row (channels: 1 = Luma8, 3 = RGB8)
__device__ __forceinline__ uint32_t row_byte(const TiffParams &P, const uint8_t *row, uint32_t channels, uint32_t at)
{
    const uint32_t top = P.sample_bytes == 1 ? 255u : 65535u;
    const uint32_t x = channels == 3 ? at / 3u : at, ch = channels == 3 ? at % 3u : 0u;
    uint32_t v;
    if (P.spp == 1) {
        v = sample_at(P, row, x);
        if (P.invert) v = top - v;
    } else if (channels == 3) {
        v = sample_at(P, row, x * P.spp + ch);
    } else { // into_luma8, as remembered: in the samples' own depth, then 16 -> 8 bits
        const uint32_t r = sample_at(P, row, x * P.spp), g = sample_at(P, row, x * P.spp + 1u), b = sample_at(P, row, x * P.spp + 2u);
        v = (2126u * r + 7152u * g + 722u * b) / 10000u;
    }
    return P.sample_bytes == 1 ? v : (v + 128u) / 257u;
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
