// tiff_ext_kernels.hip — cvhip_tiff_ext_info / cvhip_tiff_ext_decode: what cvhip_tiff_decode takes, and Deflate (compression 8 and
// 32946) and tiled files (tags 322 to 325) as well, to Luma8 or RGB8 pixels.  The reference opens its inputs
// with image::open(path)?.into_luma8() / into_rgb8() (src/reconstruction.rs:40-60), and its `image` crate reads these files;
// tests/ref_tiff_ext.py is the definition.  The host walk is tiff_common::parse(.., extended = true).
//
// A file is a table of streams: strips of rows_per_strip rows of the image's width, or tiles, which are strips of TileLength
// rows of TileWidth pixels, the edge tiles whole.  Stream s decompresses to raw[s x stream_bytes ..): every stream but a strip
// file's last has stream_bytes bytes, so a byte's stream is a division.
//
//   tiff_packbits_kernel, tiff_lzw_kernel   tiff_decompress.inc, a wave per stream: a tile is a strip to them
//   inflate_streams       inflate_stage.inc, the stage the PNG reader runs on its one stream: a workgroup per zlib stream walks its
//                         chain of deflate blocks, a workgroup per settled window writes literals and source indices, the copies
//                         resolve inside each stream, and every stream's Adler-32 is checked.  The window and record arrays are
//                         shared by all streams; their sizes are the sums of the PNG path's bounds for each stream
//   tiffx_convert_kernel  a workgroup per result row, which gathers its bytes from tiles_across streams: Predictor 2 undone by
//                         a scan per sample channel that restarts at every tile's left edge and carries across the 256-lane
//                         chunks inside a tile, then the row's bytes as aligned dwords with single bytes at its ends
// An uncompressed file has no first pass: the convert kernel reads the strips or tiles where they lie.  A distance that reaches
// in front of its stream's first byte is the file's error; no index leaves its stream.  Once an error flag is set no kernel
// writes to `out`.
#include <algorithm>
#include <cstring>
#include <vector>

#include "cvhip_internal.hpp"

#include "png_decode_common.hpp"
#include "tiff_common.hpp"

namespace cvhip {
namespace {

namespace tc = tiff_common;
namespace pd = png_decode_common;
namespace pc = png_common;

namespace strips {
#include "tiff_decompress.inc"
}
namespace inflate {
#include "inflate_device.inc"
#include "inflate_stage.inc"
}
using namespace inflate;

struct ExtParams {
    uint32_t width, height, spp, sample_bytes, predictor, from_file;
    uint32_t tile_w, tile_l, across;         // a strip file: tile_w = width, tile_l = rows per strip, across = 1
    uint32_t stream_row_bytes, stream_bytes; // of a stream's row; of a stream: tile_l rows (below 2^31)
    unsigned long long total;                // the decompressed bytes of all streams (a strip file's last strip may be short)
};

struct Status { // read back in one copy
    uint32_t flags[FLAGS];
    uint32_t strip_flags[strips::FLAGS];
};

// ---- the pixels -----------------------------------------------------------------------------------------------------------------
// where pixel x of image row y lies: in its stream's decompressed bytes (or, stored, in the rows with Predictor 2 undone), or in
// the uploaded file
__device__ __forceinline__ unsigned long long pixel_offset(const ExtParams &X, uint32_t x, uint32_t y, uint32_t &stream)
{
    stream = y / X.tile_l * X.across + x / X.tile_w;
    return (unsigned long long)(y % X.tile_l) * X.stream_row_bytes + (unsigned long long)(x % X.tile_w) * X.spp * X.sample_bytes;
}

__global__ __launch_bounds__(BLOCK) void tiffx_convert_kernel(const uint8_t *__restrict__ file, const uint32_t *__restrict__ offsets, ExtParams X,
                                                              strips::TiffParams P, uint8_t *raw, uint32_t channels, uint8_t *__restrict__ out,
                                                              const uint32_t *__restrict__ flags, const uint32_t *__restrict__ strip_flags)
{
    __shared__ uint32_t wave_sum[BLOCK / WAVE][4], s_carry[4];
    if (flags[F_ERR] || strip_flags[strips::FLAG_ERR]) return;
    const uint32_t y = blockIdx.x, tid = threadIdx.x, lane = tid % WAVE, wave = tid / WAVE;
    bool from_file = X.from_file != 0;
    if (X.predictor == 2) {
        // horizontal differencing undone: per sample channel the running sum along the row, modulo 2^8 or 2^16, from every
        // tile's left edge on.  A lane adds what lies d to its left while that is inside its tile; a wave's last lane holds the
        // sum of its tile's part of the wave, which the lanes of that tile in later waves add; s_carry is the chunk's last lane
        for (uint32_t base = 0; base < X.width; base += BLOCK) {
            const uint32_t x = base + tid, edge = x / X.tile_w * X.tile_w; // the tile's first pixel
            uint32_t stream = 0;
            const unsigned long long at = pixel_offset(X, min(x, X.width - 1u), y, stream);
            const uint8_t *px = (from_file ? file + offsets[stream] : raw + (unsigned long long)stream * X.stream_bytes) + at;
            uint32_t v[4] = {0, 0, 0, 0}, carry[4];
#pragma unroll
            for (uint32_t ch = 0; ch < 4; ch++) {
                carry[ch] = base ? s_carry[ch] : 0u;
                if (x < X.width && ch < X.spp) v[ch] = strips::sample_at(P, px, ch);
            }
#pragma unroll
            for (uint32_t d = 1; d < WAVE; d <<= 1) {
#pragma unroll
                for (uint32_t ch = 0; ch < 4; ch++) {
                    const uint32_t t = __shfl_up(v[ch], d);
                    if (lane >= d && x - d >= edge) v[ch] += t;
                }
            }
            if (lane == WAVE - 1) {
#pragma unroll
                for (uint32_t ch = 0; ch < 4; ch++) wave_sum[wave][ch] = v[ch];
            }
            __syncthreads();
#pragma unroll
            for (uint32_t ch = 0; ch < 4; ch++) {
                uint32_t before = edge < base ? carry[ch] : 0u;
#pragma unroll
                for (uint32_t k = 0; k < BLOCK / WAVE; k++)
                    if (k < wave && base + k * WAVE + (WAVE - 1) >= edge) before += wave_sum[k][ch];
                v[ch] += before;
            }
            if (tid == BLOCK - 1) {
#pragma unroll
                for (uint32_t ch = 0; ch < 4; ch++) s_carry[ch] = v[ch];
            }
            if (x < X.width) {
                uint8_t *to = raw + (unsigned long long)stream * X.stream_bytes + at;
#pragma unroll
                for (uint32_t ch = 0; ch < 4; ch++) {
                    if (ch >= X.spp) continue;
                    if (X.sample_bytes == 1) to[ch] = (uint8_t)v[ch];
                    else to[2u * ch] = (uint8_t)(P.little ? v[ch] : v[ch] >> 8), to[2u * ch + 1u] = (uint8_t)(P.little ? v[ch] >> 8 : v[ch]);
                }
            }
            __syncthreads();
        }
        from_file = false;
    }
    // the row's bytes: single bytes up to the first 4-byte aligned address, whole dwords, single bytes behind the last
    auto result_byte = [&](uint32_t at) -> uint32_t {
        const uint32_t x = channels == 3 ? at / 3u : at, ch = channels == 3 ? at % 3u : 0u;
        uint32_t stream = 0;
        const unsigned long long where = pixel_offset(X, x, y, stream);
        return strips::row_byte(P, (from_file ? file + offsets[stream] : raw + (unsigned long long)stream * X.stream_bytes) + where, channels, ch);
    };
    const uint32_t bytes = X.width * channels;
    uint8_t *dst = out + (unsigned long long)y * bytes;
    const uint32_t lead = min(bytes, (uint32_t)((4u - (uint32_t)(reinterpret_cast<uintptr_t>(dst) & 3u)) & 3u));
    const uint32_t dwords = (bytes - lead) / 4u, tail = bytes - lead - 4u * dwords;
    for (uint32_t t = tid; t < dwords; t += BLOCK) {
        const uint32_t at = lead + 4u * t;
        uint32_t word = 0;
#pragma unroll
        for (uint32_t k = 0; k < 4; k++) word |= result_byte(at + k) << (8u * k);
        *reinterpret_cast<uint32_t *>(dst + at) = word;
    }
    if (tid < lead + tail) {
        const uint32_t at = tid < lead ? tid : lead + 4u * dwords + (tid - lead);
        dst[at] = (uint8_t)result_byte(at);
    }
}

// of the thread's last decode: streams; LZW codes, Clears, the longest string; stored, fixed, dynamic blocks; subsequences; the most
// settle rounds of a window; settle windows; rounds of the copy resolution
thread_local uint64_t t_stats[12] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};

int file_error(uint32_t err)
{
    const char *why = err & ERR_ZLIB      ? "a stream's zlib header"
                      : err & ERR_BLOCK   ? "block type 3, or a stored block whose NLEN is not ~LEN"
                      : err & ERR_LENGTHS ? "a block's code lengths"
                      : err & ERR_END     ? "a stream ends before its final block's end-of-block or inside the Adler-32"
                      : err & ERR_TOKEN   ? "a code that is not in its table, an unused symbol, or a distance before the stream's first byte"
                      : err & ERR_SIZE    ? "a stream does not inflate to the bytes of its strip or tile"
                      : err & ERR_ADLER   ? "a stream's Adler-32"
                                          : "more blocks than a stream has room for";
    return fail(CVHIP_ERR_INVALID, std::string("tiff_ext_decode: Deflate: ") + why);
}

} // namespace
} // namespace cvhip

using namespace cvhip;

extern "C" int cvhip_tiff_ext_info(const uint8_t *file, uint64_t size, uint32_t *out_info, float *out_scale)
{
    if (!file || !out_info || !out_scale) return fail(CVHIP_ERR_INVALID, "tiff_ext_info: null argument");
    tc::Header h;
    const int rc = tc::parse(file, (size_t)size, h, true);
    if (rc != tc::OK) return refused("tiff_ext_info", rc == tc::UNSUPPORTED, h.error);
    out_info[0] = h.width, out_info[1] = h.height, out_info[2] = h.samples, out_info[3] = h.bits, out_info[4] = h.compression;
    out_info[5] = h.photometric, out_info[6] = h.predictor, out_info[7] = (uint32_t)h.strips.size(), out_info[8] = h.rows_per_strip;
    out_info[9] = h.focal_length_35mm, out_info[10] = h.databar_height, out_info[11] = (h.sem ? 1u : 0u) | (h.have_tilt ? 2u : 0u);
    out_info[12] = h.tile_width, out_info[13] = h.tile_length, out_info[14] = h.tiles_across, out_info[15] = 0;
    out_scale[0] = h.scale[0], out_scale[1] = h.scale[1], out_scale[2] = h.tilt_angle;
    return CVHIP_OK;
}

extern "C" int cvhip_tiff_ext_last_stats(uint64_t *out_stats)
{
    if (!out_stats) return fail(CVHIP_ERR_INVALID, "tiff_ext_last_stats: null argument");
    for (int k = 0; k < 12; k++) out_stats[k] = t_stats[k];
    return CVHIP_OK;
}

extern "C" int cvhip_tiff_ext_decode(cvhip_device *dev, const uint8_t *file, uint64_t size, uint32_t format, uint32_t drop_rows, uint8_t *out,
                                     uint64_t cap, uint64_t *out_size)
{
    if (!dev || !file || !out_size || (cap && !out)) return fail(CVHIP_ERR_INVALID, "tiff_ext_decode: null argument");
    if (format != CVHIP_IMAGE_LUMA8 && format != CVHIP_IMAGE_RGB8)
        return fail(CVHIP_ERR_INVALID, "tiff_ext_decode: format is not CVHIP_IMAGE_LUMA8 or CVHIP_IMAGE_RGB8");
    tc::Header h;
    const int rc = tc::parse(file, (size_t)size, h, true);
    if (rc != tc::OK) return refused("tiff_ext_decode", rc == tc::UNSUPPORTED, h.error);
    if (drop_rows == CVHIP_TIFF_DROP_DATABAR) drop_rows = h.databar_height;
    if (drop_rows >= h.height) return fail(CVHIP_ERR_INVALID, "tiff_ext_decode: drop_rows leaves no row");
    const uint32_t channels = format == CVHIP_IMAGE_RGB8 ? 3u : 1u, rows_out = h.height - drop_rows;
    const unsigned long long bytes = (unsigned long long)h.width * rows_out * channels;
    *out_size = bytes;
    if (!cap) return CVHIP_OK;
    if (cap < bytes) return fail(CVHIP_ERR_INVALID, "tiff_ext_decode: the buffer is smaller than the image");

    const uint32_t streams = (uint32_t)h.strips.size();
    const bool tiled = h.tile_width != 0, deflate = h.compression == tc::COMPRESSION_DEFLATE || h.compression == tc::COMPRESSION_DEFLATE_OLD;
    ExtParams X{};
    X.width = h.width, X.height = h.height, X.spp = h.samples, X.sample_bytes = h.bits / 8, X.predictor = h.predictor;
    X.from_file = h.compression == tc::COMPRESSION_NONE ? 1u : 0u;
    X.tile_w = tiled ? h.tile_width : h.width, X.tile_l = h.rows_per_strip, X.across = tiled ? h.tiles_across : 1u;
    X.stream_row_bytes = h.strips[0].row_bytes, X.stream_bytes = X.tile_l * X.stream_row_bytes;
    X.total = tiled ? (unsigned long long)streams * X.stream_bytes : (unsigned long long)h.height * X.stream_row_bytes;
    // the decompressors' view: a tile is a strip of tile_l rows; every tile is whole, so the "image" is streams x tile_l rows high
    strips::TiffParams P{};
    P.width = X.tile_w, P.height = tiled ? streams * X.tile_l : h.height, P.rows_out = rows_out, P.spp = h.samples, P.sample_bytes = h.bits / 8;
    P.little = h.little ? 1u : 0u, P.invert = h.photometric == 0 ? 1u : 0u, P.predictor = h.predictor, P.rps = X.tile_l;
    P.compressed = X.from_file ? 0u : 1u, P.row_bytes = X.stream_row_bytes;
    // ---- the one upload: the stream table, then the file's bytes up to the last stream's end - or, for Deflate, every stream
    // at a multiple of four bytes with 32 zero bytes behind it, which is what the bit readers may reach into
    const size_t table_bytes = ((size_t)streams * 2 * sizeof(uint32_t) + 15) / 16 * 16;
    unsigned long long file_bytes = 0, max_windows = 0, max_records = 0;
    std::vector<uint32_t> placed(streams);
    for (uint32_t s = 0; s < streams; s++) {
        const tc::Strip &strip = h.strips[s];
        if (!deflate) {
            placed[s] = strip.offset;
            file_bytes = std::max<unsigned long long>(file_bytes, (unsigned long long)strip.offset + strip.count);
            continue;
        }
        placed[s] = (uint32_t)file_bytes;
        file_bytes += ((unsigned long long)strip.count + 32 + 3) / 4 * 4;
        // png_decode's bounds, stream by stream: a window or a record takes a block with output (18 bits), or a full window /
        // subsequence of the stream
        const unsigned long long bits = 8ull * strip.count, blocks = bits / 18 + 2;
        max_windows += blocks + bits / ((unsigned long long)BLOCK * pd::SUBSEQ_BITS) + 2;
        max_records += blocks + bits / pd::SUBSEQ_BITS + 2;
    }
    if (file_bytes >= (1ull << 32) || max_records >= (1ull << 32)) return fail(CVHIP_ERR_UNSUPPORTED, "tiff_ext_decode: Deflate streams of 2^32 bytes or more");
    std::vector<uint8_t> blob(table_bytes + (size_t)file_bytes);
    uint32_t *table = reinterpret_cast<uint32_t *>(blob.data());
    for (uint32_t s = 0; s < streams; s++) {
        table[s] = placed[s], table[streams + s] = h.strips[s].count;
        if (deflate) std::memcpy(blob.data() + table_bytes + placed[s], file + h.strips[s].offset, h.strips[s].count);
    }
    if (!deflate) std::memcpy(blob.data() + table_bytes, file, (size_t)file_bytes);

    CVHIP_TRY_HIP(hipSetDevice(dev->d.ordinal));
    hipStream_t s = dev->d.stream;
    CallScratch sc;
    const size_t raw_bytes = (size_t)streams * X.stream_bytes; // the decompressed streams, or the stored ones with Predictor 2 undone
    const bool need_raw = !X.from_file || X.predictor == 2;
    Carver carve;
    const size_t at_blob = carve.reserve(blob.size()), at_status = carve.reserve(sizeof(Status)), at_raw = carve.reserve(need_raw ? raw_bytes : 0);
    const size_t at_src = carve.reserve(deflate ? (size_t)X.total * 4 * 2 : 0), at_win = carve.reserve((size_t)max_windows * WIN_SLOTS * 8);
    const size_t at_entry = carve.reserve((size_t)max_records * 8), at_out = carve.reserve((size_t)max_records * 8), at_count = carve.reserve((size_t)max_records * 4);
    const size_t at_streams = carve.reserve(deflate ? (size_t)streams * 3 * 8 : 0); // per stream: the end bit; the two Adler-32 sums
    uint8_t *arena = nullptr, *d_out = nullptr;
    hipError_t e = sc.alloc(&arena, carve.total);
    if (e == hipSuccess) e = sc.output(out, (size_t)bytes, &d_out);
    if (e != hipSuccess) return device_error("tiff_ext_decode", e);
    Status *status = reinterpret_cast<Status *>(arena + at_status), h_status{};
    uint32_t *flags = status->flags, *strip_flags = status->strip_flags;
    const uint32_t *d_offsets = reinterpret_cast<const uint32_t *>(arena + at_blob), *d_counts = d_offsets + streams;
    const uint8_t *d_file = arena + at_blob + table_bytes;
    uint8_t *raw = arena + at_raw;
    e = hipMemcpyAsync(arena + at_blob, blob.data(), blob.size(), hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipMemsetAsync(status, 0, sizeof(Status), s);
    if (e == hipSuccess && deflate) e = hipMemsetAsync(arena + at_streams, 0, (size_t)streams * 3 * 8, s);
    if (e != hipSuccess) return device_error("tiff_ext_decode", e);
    auto read_status = [&]() {
        hipError_t r = hipGetLastError();
        if (r == hipSuccess) r = hipMemcpyAsync(&h_status, status, sizeof(Status), hipMemcpyDeviceToHost, s);
        if (r == hipSuccess) r = hipStreamSynchronize(s);
        return r;
    };
    auto keep_stats = [&](uint64_t copy_rounds) {
        const uint32_t *f = h_status.flags, *g = h_status.strip_flags;
        t_stats[0] = streams, t_stats[1] = g[strips::FLAG_CODES], t_stats[2] = g[strips::FLAG_CLEARS], t_stats[3] = g[strips::FLAG_LONGEST];
        t_stats[4] = f[F_STORED], t_stats[5] = f[F_FIXED], t_stats[6] = f[F_DYNAMIC], t_stats[7] = f[F_SUBSEQUENCES], t_stats[8] = f[F_ROUNDS];
        t_stats[9] = f[F_WINDOWS], t_stats[10] = copy_rounds, t_stats[11] = 0;
    };
    const dim3 block(BLOCK);
    uint32_t rounds = 0;
    if (deflate) {
        InflateArgs A{};
        A.file = d_file, A.offsets = d_offsets, A.counts = d_counts, A.streams = streams, A.layout = {X.stream_bytes, X.total};
        A.win = reinterpret_cast<unsigned long long *>(arena + at_win), A.max_windows = max_windows;
        A.rec_entry = reinterpret_cast<unsigned long long *>(arena + at_entry), A.rec_out = reinterpret_cast<unsigned long long *>(arena + at_out);
        A.rec_count = reinterpret_cast<uint32_t *>(arena + at_count), A.max_records = max_records, A.raw = raw;
        A.srcs[0] = reinterpret_cast<uint32_t *>(arena + at_src), A.srcs[1] = A.srcs[0] + X.total;
        A.end_bit = reinterpret_cast<unsigned long long *>(arena + at_streams), A.sums = A.end_bit + streams, A.flags = flags;
        uint32_t err = 0;
        const int stage = inflate_streams("tiff_ext_decode", s, A, false, h_status.flags, err, rounds);
        if (stage != CVHIP_OK) return stage;
        keep_stats(rounds);
        if (err) return file_error(err);
    } else if (h.compression == tc::COMPRESSION_LZW) {
        hipLaunchKernelGGL(strips::tiff_lzw_kernel, dim3(streams), dim3(strips::WAVE), 0, s, d_file, d_offsets, d_counts, P, raw, strip_flags);
    } else if (h.compression == tc::COMPRESSION_PACKBITS) {
        hipLaunchKernelGGL(strips::tiff_packbits_kernel, dim3(streams), dim3(strips::WAVE), 0, s, d_file, d_offsets, d_counts, P, raw, strip_flags);
    }
    hipLaunchKernelGGL(tiffx_convert_kernel, dim3(rows_out), block, 0, s, d_file, d_offsets, X, P, raw, channels, d_out, flags, strip_flags);
    if ((e = read_status()) != hipSuccess) return device_error("tiff_ext_decode", e);
    keep_stats(rounds);
    if (h_status.flags[F_ERR]) return file_error(h_status.flags[F_ERR]);
    if (h_status.strip_flags[strips::FLAG_ERR])
        return fail(CVHIP_ERR_INVALID, h.compression == tc::COMPRESSION_LZW
                                           ? "tiff_ext_decode: LZW: a code above the next entry, or EOI or the end of the input before the rows are full"
                                           : "tiff_ext_decode: PackBits: the input ends before the rows are full");
    e = sc.copy_out(out, d_out, (size_t)bytes, s);
    if (e == hipSuccess) e = sc.drain(s);
    if (e != hipSuccess) return device_error("tiff_ext_decode", e);
    return CVHIP_OK;
}
