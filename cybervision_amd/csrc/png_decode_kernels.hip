// png_decode_kernels.hip — cvhip_png_decode: a PNG file to Luma8 or RGB8 pixels, everything behind the chunk walk on the device
// (DESIGN.md 4.18).  The reference opens its inputs with image::open(path)?.into_luma8() / into_rgb8()
// (src/reconstruction.rs:40-60); tests/ref_png_in.py is the definition of the pixels.  The host (png_decode_common.hpp) walks
// the chunks, checks the CRC of the small ones and reads IHDR, PLTE and eXIf; the palette, the IDAT table and the IDAT
// payloads, end to end, go up in one copy.
//
//   png_crc_kernel       a workgroup per IDAT chunk: the CRC-32 of 256 pieces, combined with png_common.hpp's arithmetic
//   inflate_streams      inflate_stage.inc, the stage the TIFF reader runs on its Deflate strips and tiles, on a table of one
//                        stream: one workgroup walks the chain of deflate blocks and settles it window by window, a workgroup
//                        per window writes literals and source indices to the filtered image, the copies resolve by pointer
//                        doubling, and the Adler-32 is checked.  The stage's head comment says how and why
//   png_unfilter_kernel  a workgroup per row segment - None and Sub rows start one -: tiles of 64 rows through LDS, a lane of
//                        the first wave per row, skewed by one pixel per lane, `up` and `up-left` by a shuffle from the lane above
//   png_index_kernel     colour type 3: no index beyond the PLTE
//   png_convert_kernel   a lane per aligned dword of `out`: samples to 8 bits, palette, luma, drop_rows
// cvhip_png_ext_decode (tests/ref_png_adam7.py) is the same body for a superset of the files: Adam7
// interlaced ones too.  Their stream is the seven reduced images one behind the other; the last three kernels are templates
// on ADAM7 - the unfilter launch covers the rows of all passes and a workgroup finds its pass in a table passed by value,
// the index and convert kernels map a pixel to its pass, row and sample - and a file that is not interlaced runs the
// <false> instantiations, which are what these kernels were before.
// Once flags[F_ERR] is set no kernel writes to `out`.
#include <cstring>
#include <vector>

#include "cvhip_internal.hpp"

#include "png_decode_common.hpp"

namespace cvhip {
namespace {

namespace pd = png_decode_common;
namespace pc = png_common;

#include "inflate_device.inc"
#include "inflate_stage.inc"

struct IdatEntry {
    unsigned long long offset; // in the stream
    uint32_t length, crc;
};

struct PngParams {
    uint32_t width, height, colour, depth, channels, bpp, palette_entries;
    unsigned long long row_bytes, filtered; // filtered = height x (1 + row_bytes), or the sum of that over the passes
};

// The reduced images of an Adam7 file (png_decode_common.hpp's Pass), by value in the kernel arguments: the
// kernels of cvhip_png_ext_decode read it where the file is interlaced.  An empty pass has no rows.
struct PassEntry {
    uint32_t height, row_bytes, first_row, offset; // rows; bytes of one without its filter byte; first row among all passes' rows; first byte in `raw`
};
struct PassTable {
    PassEntry pass[pd::ADAM7_PASSES];
};
// x0, y0, log2 dx and log2 dy of pass p, a nibble each (png_decode_common.hpp's ADAM7_* tables)
constexpr uint32_t ADAM7_X0 = 0x0102040u, ADAM7_Y0 = 0x1020400u, ADAM7_LOG_DX = 0x0112233u, ADAM7_LOG_DY = 0x1122333u;
__host__ __device__ constexpr uint32_t nibble(uint32_t table, uint32_t p) { return (table >> (4u * p)) & 15u; }
constexpr bool nibbles_match(uint32_t table, const uint32_t (&values)[7])
{
    for (uint32_t p = 0; p < 7; p++)
        if (nibble(table, p) != values[p]) return false;
    return true;
}
static_assert(nibbles_match(ADAM7_X0, pd::ADAM7_X0) && nibbles_match(ADAM7_Y0, pd::ADAM7_Y0) && nibbles_match(ADAM7_LOG_DX, pd::ADAM7_LOG_DX) &&
                  nibbles_match(ADAM7_LOG_DY, pd::ADAM7_LOG_DY),
              "the packed Adam7 tables are png_decode_common.hpp's");

// ---- the IDAT chunks' CRCs -----------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(BLOCK) void png_crc_kernel(const uint8_t *__restrict__ stream, const IdatEntry *__restrict__ table, uint32_t type_crc,
                                                        uint32_t *__restrict__ flags)
{
    __shared__ uint32_t s_table[256], s_crc[BLOCK];
    s_table[threadIdx.x] = pc::crc_table_entry(threadIdx.x);
    __syncthreads();
    const IdatEntry chunk = table[blockIdx.x];
    const uint32_t piece = (chunk.length + BLOCK - 1) / BLOCK;
    const unsigned long long begin = min((unsigned long long)threadIdx.x * piece, (unsigned long long)chunk.length);
    const unsigned long long end = min(begin + piece, (unsigned long long)chunk.length);
    uint32_t crc = 0xFFFFFFFFu;
    for (unsigned long long i = begin; i < end; i++) crc = s_table[(crc ^ stream[chunk.offset + i]) & 255u] ^ (crc >> 8);
    s_crc[threadIdx.x] = crc ^ 0xFFFFFFFFu;
    __syncthreads();
    if (threadIdx.x) return;
    uint32_t total = type_crc; // of the chunk's type, which the CRC covers
    const uint32_t shift = pc::crc_shift(piece);
    for (uint32_t t = 0; t < BLOCK; t++) {
        const unsigned long long b = min((unsigned long long)t * piece, (unsigned long long)chunk.length);
        const unsigned long long n = min(b + piece, (unsigned long long)chunk.length) - b;
        if (n == piece && n) total = pc::crc_multiply(shift, total) ^ s_crc[t];
        else if (n) total = pc::crc_combine(total, s_crc[t], n);
    }
    if (total != chunk.crc) atomicOr(&flags[F_ERR], ERR_CRC);
}

// ---- the filters --------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ uint32_t paeth(uint32_t a, uint32_t b, uint32_t c)
{
    const int p = (int)a + (int)b - (int)c;
    const int pa = abs(p - (int)a), pb = abs(p - (int)b), pc_ = abs(p - (int)c);
    return pa <= pb && pa <= pc_ ? a : pb <= pc_ ? b : c;
}

// A workgroup per row; the one of a segment's first row (row 0, or a None or Sub row) unfilters the segment in place, 64 rows
// at a time and TILE_BYTES of them at a time: all four waves copy the tile and the row above it into LDS (a wave alone has
// too few loads in flight), the first wave filters it there - lane l has row batch + l and at step t the tile's pixel t - l,
// so the lane above has finished that pixel one step and the one to its left two steps earlier, and both come by a shuffle;
// lane 0 reads the row above the batch - and all four copy it back.  The two pixels a lane keeps carry over from tile to tile.
constexpr uint32_t TILE_BYTES = 384, UNFILTER_LANES = 256; // (a multiple of every bpp: 1, 2, 3, 4, 6, 8)

// The first wave on a tile in LDS (row 0: the row above the batch): a step's reads - the lane's own pixel and, for lane 0, the
// one above - are issued together in front of the shuffles, the loops over a pixel's BPP bytes unrolled.
template <uint32_t BPP>
__device__ __forceinline__ void unfilter_tile(uint8_t *s_tile, uint32_t lane, bool active, uint32_t type, uint32_t tp, unsigned long long &last,
                                              unsigned long long &prev, unsigned long long &above_prev)
{
    for (uint32_t t = 0; t < tp + WAVE - 1; t++) {
        const bool on = active && t >= lane && t - lane < tp;
        const uint32_t x = on ? t - lane : 0u;
        uint8_t *px = s_tile + (lane + 1) * TILE_BYTES + x * BPP;
        const uint8_t *above = s_tile + x * BPP;
        unsigned long long in = 0, up0 = 0;
#pragma unroll
        for (uint32_t k = 0; k < BPP; k++) in |= (unsigned long long)px[k] << (8 * k), up0 |= (unsigned long long)above[k] << (8 * k);
        unsigned long long b = __shfl_up(last, 1), c = __shfl_up(prev, 1);
        if (!on) continue;
        if (lane == 0) c = above_prev, b = up0, above_prev = up0;
        unsigned long long v = 0;
#pragma unroll
        for (uint32_t k = 0; k < BPP; k++) {
            const uint32_t left = (uint32_t)(last >> (8 * k)) & 255u, up = (uint32_t)(b >> (8 * k)) & 255u, up_left = (uint32_t)(c >> (8 * k)) & 255u;
            const uint32_t predicted = type == 0 ? 0u : type == 1 ? left : type == 2 ? up : type == 3 ? (left + up) >> 1 : paeth(left, up, up_left);
            const uint32_t value = (((uint32_t)(in >> (8 * k)) & 255u) + predicted) & 255u;
            px[k] = (uint8_t)value;
            v |= (unsigned long long)value << (8 * k);
        }
        prev = last, last = v;
    }
}

// ADAM7: the grid is the rows of all passes; a workgroup finds its pass in the table (uniform: scalar compares and selects)
// and from there on `raw`, `height` and `row_bytes` are its pass's, `first_row` counts from its pass's first row - which
// starts a segment whatever its type, as the last row ends one: the passes' segments run side by side in the one launch.
template <bool ADAM7>
__global__ __launch_bounds__(UNFILTER_LANES) void png_unfilter_kernel(uint8_t *__restrict__ raw, uint32_t height, unsigned long long row_bytes, uint32_t bpp,
                                                                      PassTable T, uint32_t *__restrict__ flags)
{
    __shared__ uint8_t s_tile[(WAVE + 1) * TILE_BYTES]; // row 0: the row above the batch
    uint32_t first_row = blockIdx.x;
    if constexpr (ADAM7) {
        PassEntry e = T.pass[0]; // (never empty)
#pragma unroll
        for (uint32_t p = 1; p < pd::ADAM7_PASSES; p++)
            if (T.pass[p].height && blockIdx.x >= T.pass[p].first_row) e = T.pass[p];
        raw += e.offset, height = e.height, row_bytes = e.row_bytes, first_row -= e.first_row;
    }
    const uint32_t tid = threadIdx.x, lane = tid & (WAVE - 1u);
    const bool worker = tid < WAVE;
    const unsigned long long stride = row_bytes + 1;
    if (flags[F_ERR] & ~ERR_FILTER) return; // (set by the kernels before this one only: the same for every lane)
    const uint32_t first_type = raw[first_row * stride];
    if (first_type > 4) {
        if (tid == 0) atomicOr(&flags[F_ERR], ERR_FILTER);
        return;
    }
    if (first_row != 0 && first_type >= 2) return; // the segment of a row above
    if (tid == 0) atomicAdd(&flags[F_SEGMENTS], 1u);
    for (uint32_t batch = first_row; batch < height; batch += WAVE) {
        const uint32_t row = batch + lane;
        const bool inside = row < height;
        const uint32_t type = inside ? raw[row * stride] : 0u;
        const unsigned long long starts = __ballot(inside && row != first_row && (type < 2 || type > 4)); // the next segment's first row (the same in every wave)
        const uint32_t limit = starts ? (uint32_t)__ffsll((long long)starts) - 1u : WAVE;
        const uint32_t rows = min(limit, height - batch);
        const bool active = worker && lane < rows, above_valid = batch > first_row; // (a segment's first row has zeros above it, or does not look)
        unsigned long long last = 0, prev = 0, above_prev = 0; // the pixel finished a step ago, two steps ago; lane 0: the row above's last one
        for (unsigned long long c0 = 0; c0 < row_bytes; c0 += TILE_BYTES) {
            const uint32_t n = (uint32_t)min((unsigned long long)TILE_BYTES, row_bytes - c0), tp = n / bpp, cells = (rows + 1) * TILE_BYTES;
            uint8_t *tile = raw + (unsigned long long)batch * stride + 1 + c0; // of the batch's first row
#pragma unroll 8
            for (uint32_t idx = tid; idx < cells; idx += UNFILTER_LANES) {
                const uint32_t r = idx / TILE_BYTES, k = idx % TILE_BYTES;
                uint8_t v = 0;
                if (k < n && (r || above_valid)) v = (tile + ((long long)r - 1) * (long long)stride)[k];
                s_tile[idx] = v;
            }
            __syncthreads();
            if (worker) {
                switch (bpp) {
                case 1: unfilter_tile<1>(s_tile, lane, active, type, tp, last, prev, above_prev); break;
                case 2: unfilter_tile<2>(s_tile, lane, active, type, tp, last, prev, above_prev); break;
                case 3: unfilter_tile<3>(s_tile, lane, active, type, tp, last, prev, above_prev); break;
                case 4: unfilter_tile<4>(s_tile, lane, active, type, tp, last, prev, above_prev); break;
                case 6: unfilter_tile<6>(s_tile, lane, active, type, tp, last, prev, above_prev); break;
                default: unfilter_tile<8>(s_tile, lane, active, type, tp, last, prev, above_prev); break;
                }
            }
            __syncthreads();
#pragma unroll 8
            for (uint32_t idx = TILE_BYTES + tid; idx < cells; idx += UNFILTER_LANES) {
                const uint32_t r = idx / TILE_BYTES, k = idx % TILE_BYTES;
                if (k < n) (tile + ((long long)r - 1) * (long long)stride)[k] = s_tile[idx];
            }
            __syncthreads(); // the tile is free again; the next batch reads the last row of this one as its row above
        }
        if (starts) break;
    }
}

// ---- the pixels ---------------------------------------------------------------------------------------------------------------------
// sample i of the unfiltered row (the bytes behind its filter byte)
__device__ __forceinline__ uint32_t sample_at(const uint8_t *__restrict__ row, uint32_t depth, unsigned long long i)
{
    if (depth == 8) return row[i];
    if (depth == 16) return (uint32_t)row[2 * i] << 8 | row[2 * i + 1];
    const unsigned long long bit = i * depth;
    return (row[bit >> 3] >> (8 - depth - (uint32_t)(bit & 7u))) & ((1u << depth) - 1u);
}
__device__ __forceinline__ uint32_t reduce16(uint32_t v) { return (v + 128u) / 257u; }

// The unfiltered row (the bytes behind its filter byte) that holds pixel `pix`, and in x the pixel's place in that row.
// ADAM7: the pass of pixel (x, y) is read off the low bits of x and y; its row and place follow from the pass's origin and steps.
template <bool ADAM7>
__device__ __forceinline__ const uint8_t *row_of(const uint8_t *__restrict__ raw, const PngParams &P, const PassTable &T, unsigned long long pix,
                                                 unsigned long long &x)
{
    x = pix % P.width;
    const unsigned long long y = pix / P.width;
    if constexpr (!ADAM7) return raw + y * (P.row_bytes + 1) + 1;
    const uint32_t xl = (uint32_t)x, yl = (uint32_t)y;
    const uint32_t p = yl & 1u ? 6u : xl & 1u ? 5u : yl & 2u ? 4u : xl & 2u ? 3u : yl & 4u ? 2u : xl & 4u ? 1u : 0u;
    const PassEntry e = T.pass[p];
    x = (xl - nibble(ADAM7_X0, p)) >> nibble(ADAM7_LOG_DX, p);
    return raw + e.offset + (unsigned long long)((yl - nibble(ADAM7_Y0, p)) >> nibble(ADAM7_LOG_DY, p)) * (e.row_bytes + 1ull) + 1;
}

// every pixel's index, of every pass: the padding bits at a row's end are no pixel's
template <bool ADAM7>
__global__ __launch_bounds__(BLOCK) void png_index_kernel(const uint8_t *__restrict__ raw, PngParams P, PassTable T, uint32_t *__restrict__ flags)
{
    const unsigned long long i = (unsigned long long)blockIdx.x * BLOCK + threadIdx.x;
    if (i >= (unsigned long long)P.width * P.height) return;
    unsigned long long x;
    const uint8_t *row = row_of<ADAM7>(raw, P, T, i, x);
    if (sample_at(row, P.depth, x) >= P.palette_entries) atomicOr(&flags[F_ERR], ERR_INDEX);
}

// pixel `pix`: r | g << 8 | b << 16 | luma << 24
template <bool ADAM7>
__device__ __forceinline__ uint32_t pixel_at(const uint8_t *__restrict__ raw, const uint8_t *__restrict__ palette, const PngParams &P, const PassTable &T,
                                             unsigned long long pix)
{
    unsigned long long x;
    const uint8_t *row = row_of<ADAM7>(raw, P, T, pix, x);
    if (P.colour == 0 || P.colour == 4) {
        const uint32_t v = sample_at(row, P.depth, x * P.channels);
        const uint32_t g = P.depth == 16 ? reduce16(v) : P.depth == 8 ? v : v * (255u / ((1u << P.depth) - 1u));
        return g * 0x01010101u;
    }
    uint32_t r, g, b;
    if (P.colour == 3) {
        const uint32_t i = min(sample_at(row, P.depth, x), 255u);
        r = palette[3 * i], g = palette[3 * i + 1], b = palette[3 * i + 2];
    } else {
        r = sample_at(row, P.depth, x * P.channels), g = sample_at(row, P.depth, x * P.channels + 1), b = sample_at(row, P.depth, x * P.channels + 2);
    }
    uint32_t luma = (2126u * r + 7152u * g + 722u * b) / 10000u; // into_luma8, as remembered; 16-bit samples: in 16 bits
    if (P.depth == 16 && P.colour != 3) r = reduce16(r), g = reduce16(g), b = reduce16(b), luma = reduce16(luma);
    return r | g << 8 | b << 16 | luma << 24;
}
template <bool ADAM7>
__device__ __forceinline__ uint32_t result_byte(const uint8_t *__restrict__ raw, const uint8_t *__restrict__ palette, const PngParams &P, const PassTable &T,
                                                uint32_t channels, unsigned long long at)
{
    if (channels == 3) return (pixel_at<ADAM7>(raw, palette, P, T, at / 3) >> (8 * (uint32_t)(at % 3))) & 255u;
    return pixel_at<ADAM7>(raw, palette, P, T, at) >> 24;
}

// out[0 .. bytes): `lead` single bytes up to the first 4-byte aligned address, whole dwords, the rest single bytes - a lane
// per dword and a lane per single byte (jpeg_pixels_kernel's layout)
template <bool ADAM7>
__global__ __launch_bounds__(BLOCK) void png_convert_kernel(const uint8_t *__restrict__ raw, const uint8_t *__restrict__ palette, PngParams P, PassTable T,
                                                            uint32_t channels, uint8_t *__restrict__ out, unsigned long long bytes, uint32_t lead,
                                                            const uint32_t *__restrict__ flags)
{
    if (flags[F_ERR]) return;
    const unsigned long long t = (unsigned long long)blockIdx.x * BLOCK + threadIdx.x, dwords = (bytes - lead) / 4;
    if (t < dwords) {
        const unsigned long long at = lead + 4 * t;
        uint32_t word = 0;
#pragma unroll
        for (uint32_t k = 0; k < 4; k++) word |= result_byte<ADAM7>(raw, palette, P, T, channels, at + k) << (8 * k);
        *reinterpret_cast<uint32_t *>(out + at) = word;
        return;
    }
    const unsigned long long single = t - dwords, singles = bytes - 4 * dwords;
    if (single >= singles) return;
    const unsigned long long at = single < lead ? single : 4 * dwords + single;
    out[at] = (uint8_t)result_byte<ADAM7>(raw, palette, P, T, channels, at);
}

thread_local uint64_t t_stats[8] = {0, 0, 0, 0, 0, 0, 0, 0};      // of cvhip_png_decode
thread_local uint64_t t_ext_stats[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0}; // of cvhip_png_ext_decode: and the non-empty passes, zero

int file_error(const std::string &name, uint32_t err, bool passes = false)
{
    const char *why = err & ERR_CRC       ? "an IDAT chunk's CRC"
                      : err & ERR_ZLIB    ? "the zlib header"
                      : err & ERR_BLOCK   ? "block type 3, or a stored block whose NLEN is not ~LEN"
                      : err & ERR_LENGTHS ? "a block's code lengths"
                      : err & ERR_END     ? "the stream ends before the final block's end-of-block or inside the Adler-32"
                      : err & ERR_TOKEN   ? "a code that is not in its table, an unused symbol, or a distance before the first byte"
                      : err & ERR_SIZE    ? (passes ? "the stream does not inflate to the passes' bytes" : "the stream does not inflate to height x (1 + row bytes) bytes")
                      : err & ERR_ADLER   ? "the Adler-32"
                      : err & ERR_FILTER  ? "a filter type above 4"
                      : err & ERR_INDEX   ? "a palette index beyond the PLTE"
                                          : "more blocks than the stream has room for";
    return fail(CVHIP_ERR_INVALID, name + ": " + why);
}

int info(const char *name, bool adam7, const uint8_t *file, uint64_t size, uint32_t *out_info)
{
    if (!file || !out_info) return fail(CVHIP_ERR_INVALID, std::string(name) + ": null argument");
    pd::Header h;
    const int rc = pd::parse(file, (size_t)size, h, adam7);
    if (rc != pd::OK) return refused(name, rc == pd::UNSUPPORTED, h.error);
    out_info[0] = h.width, out_info[1] = h.height, out_info[2] = h.colour, out_info[3] = h.depth, out_info[4] = h.interlace;
    out_info[5] = (uint32_t)h.idat.size(), out_info[6] = h.focal_length_35mm, out_info[7] = h.flags;
    return CVHIP_OK;
}

// The body of cvhip_png_decode (adam7 = false, stats = t_stats) and of cvhip_png_ext_decode (adam7 = true, stats = t_ext_stats, whose slot
// 8 is the non-empty passes).  A file that is not interlaced runs the same instantiations of the kernels through either.
int decode(const char *name_, bool adam7, uint64_t *stats, cvhip_device *dev, const uint8_t *file, uint64_t size, uint32_t format, uint32_t drop_rows,
           uint8_t *out, uint64_t cap, uint64_t *out_size)
{
    const std::string name = name_;
    if (!dev || !file || !out_size || (cap && !out)) return fail(CVHIP_ERR_INVALID, name + ": null argument");
    if (format != CVHIP_IMAGE_LUMA8 && format != CVHIP_IMAGE_RGB8) return fail(CVHIP_ERR_INVALID, name + ": format is not CVHIP_IMAGE_LUMA8 or CVHIP_IMAGE_RGB8");
    pd::Header h;
    const int rc = pd::parse(file, (size_t)size, h, adam7);
    if (rc != pd::OK) return refused(name_, rc == pd::UNSUPPORTED, h.error);
    if (drop_rows >= h.height) return fail(CVHIP_ERR_INVALID, name + ": drop_rows leaves no row");
    const uint32_t channels = format == CVHIP_IMAGE_RGB8 ? 3u : 1u;
    const unsigned long long bytes = (unsigned long long)h.width * (h.height - drop_rows) * channels;
    *out_size = bytes;
    if (!cap) return CVHIP_OK;
    if (cap < bytes) return fail(CVHIP_ERR_INVALID, name + ": the buffer is smaller than the image");
    const unsigned long long n = h.idat_bytes, total_bits = n * 8, n_idat = h.idat.size();
    if (n >= (1ull << 31)) return fail(CVHIP_ERR_UNSUPPORTED, name + ": IDAT data of 2^31 or more bytes");
    PngParams P{};
    P.width = h.width, P.height = h.height, P.colour = h.colour, P.depth = h.depth, P.channels = h.channels, P.bpp = h.bpp;
    P.palette_entries = h.palette_entries, P.row_bytes = h.row_bytes, P.filtered = h.filtered;
    const bool laced = h.interlace != 0;
    PassTable T{}; // (all below 2^31: parse has checked the sum)
    for (uint32_t p = 0; p < h.pass_entries; p++)
        T.pass[p] = {h.pass[p].height, (uint32_t)h.pass[p].row_bytes, h.pass[p].first_row, (uint32_t)h.pass[p].offset};
    // ---- the one upload: the palette, the IDAT table, the stage's table of the one stream (its offset and its byte count, in
    // sixteen bytes: the stream stays at a multiple of 16), the IDAT payloads end to end
    const size_t table_at = sizeof(h.palette), streams_at = table_at + (size_t)n_idat * sizeof(IdatEntry), stream_at = streams_at + 16;
    std::vector<uint8_t> blob(stream_at + (size_t)n);
    std::memcpy(blob.data(), h.palette, sizeof(h.palette));
    const uint32_t stream_table[2] = {0u, (uint32_t)n};
    std::memcpy(blob.data() + streams_at, stream_table, sizeof(stream_table));
    unsigned long long placed = 0;
    for (size_t k = 0; k < n_idat; k++) {
        const IdatEntry entry = {placed, h.idat[k].length, h.idat[k].crc};
        std::memcpy(blob.data() + table_at + k * sizeof(IdatEntry), &entry, sizeof(entry));
        std::memcpy(blob.data() + stream_at + placed, file + h.idat[k].offset, h.idat[k].length);
        placed += h.idat[k].length;
    }
    // A window or a record takes a block with output, which takes 18 bits (a fixed block of one literal), or a full
    // window / subsequence of the stream: the bounds hold for every stream, the chain kernel checks them all the same.
    const unsigned long long max_blocks = total_bits / 18 + 2;
    const unsigned long long max_windows = max_blocks + total_bits / ((unsigned long long)BLOCK * pd::SUBSEQ_BITS) + 2;
    const unsigned long long max_records = max_blocks + total_bits / pd::SUBSEQ_BITS + 2;

    CVHIP_TRY_HIP(hipSetDevice(dev->d.ordinal));
    hipStream_t s = dev->d.stream;
    CallScratch sc;
    Carver carve; // one allocation, carved
    const size_t pad = 32;
    const size_t at_blob = carve.reserve(blob.size() + pad), at_flags = carve.reserve(FLAGS * 4), at_win = carve.reserve((size_t)max_windows * WIN_SLOTS * 8);
    const size_t at_entry = carve.reserve((size_t)max_records * 8), at_out = carve.reserve((size_t)max_records * 8), at_count = carve.reserve((size_t)max_records * 4);
    const size_t at_raw = carve.reserve((size_t)P.filtered), at_src = carve.reserve((size_t)P.filtered * 4 * 2);
    const size_t at_streams = carve.reserve(3 * 8); // of the one stream: the end bit; the two Adler-32 sums
    uint8_t *arena = nullptr, *d_out = nullptr;
    hipError_t e = sc.alloc(&arena, carve.total);
    if (e == hipSuccess) e = sc.output(out, (size_t)bytes, &d_out);
    if (e != hipSuccess) return device_error(name_, e);
    uint8_t *d_blob = arena + at_blob, *raw = arena + at_raw;
    uint32_t *flags = reinterpret_cast<uint32_t *>(arena + at_flags), h_flags[FLAGS] = {}; // read back in one copy
    const uint8_t *d_palette = d_blob, *d_stream = d_blob + stream_at; // (stream_at is a multiple of 16)
    const IdatEntry *d_table = reinterpret_cast<const IdatEntry *>(d_blob + table_at);
    e = hipMemcpyAsync(d_blob, blob.data(), blob.size(), hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipMemsetAsync(d_blob + blob.size(), 0, pad, s);
    if (e == hipSuccess) e = hipMemsetAsync(flags, 0, FLAGS * 4, s);
    if (e == hipSuccess) e = hipMemsetAsync(arena + at_streams, 0, 3 * 8, s);
    if (e != hipSuccess) return device_error(name_, e);
    const dim3 block(BLOCK);
    const uint8_t idat_name[4] = {'I', 'D', 'A', 'T'};
    hipLaunchKernelGGL(png_crc_kernel, dim3((uint32_t)n_idat), block, 0, s, d_stream, d_table, pc::crc32(idat_name, 4), flags);
    auto keep_stats = [&](uint64_t copy_rounds) {
        const uint32_t *f = h_flags;
        stats[0] = f[F_STORED], stats[1] = f[F_FIXED], stats[2] = f[F_DYNAMIC], stats[3] = f[F_SUBSEQUENCES], stats[4] = f[F_ROUNDS];
        stats[5] = f[F_WINDOWS], stats[6] = copy_rounds, stats[7] = f[F_SEGMENTS];
        if (adam7) stats[8] = h.passes, stats[9] = 0;
    };
    InflateArgs A{};
    A.file = d_stream, A.offsets = reinterpret_cast<const uint32_t *>(d_blob + streams_at), A.counts = A.offsets + 1, A.streams = 1;
    A.layout = {(uint32_t)P.filtered, P.filtered}; // (below 2^31: parse has checked it)
    A.win = reinterpret_cast<unsigned long long *>(arena + at_win), A.max_windows = max_windows;
    A.rec_entry = reinterpret_cast<unsigned long long *>(arena + at_entry), A.rec_out = reinterpret_cast<unsigned long long *>(arena + at_out);
    A.rec_count = reinterpret_cast<uint32_t *>(arena + at_count), A.max_records = max_records, A.raw = raw;
    A.srcs[0] = reinterpret_cast<uint32_t *>(arena + at_src), A.srcs[1] = A.srcs[0] + P.filtered;
    A.end_bit = reinterpret_cast<unsigned long long *>(arena + at_streams), A.sums = A.end_bit + 1, A.flags = flags;
    uint32_t err = 0, rounds = 0;
    const int stage = inflate_streams(name_, s, A, true, h_flags, err, rounds);
    if (stage != CVHIP_OK) return stage;
    keep_stats(rounds);
    if (err) return file_error(name, err, laced);
    // the grid: a workgroup per row, of every pass
    if (laced) hipLaunchKernelGGL(png_unfilter_kernel<true>, dim3(h.pass_rows), dim3(UNFILTER_LANES), 0, s, raw, P.height, P.row_bytes, P.bpp, T, flags);
    else hipLaunchKernelGGL(png_unfilter_kernel<false>, dim3(P.height), dim3(UNFILTER_LANES), 0, s, raw, P.height, P.row_bytes, P.bpp, T, flags);
    const dim3 pixel_grid((uint32_t)(((unsigned long long)P.width * P.height + BLOCK - 1) / BLOCK));
    if (P.colour == 3 && laced) hipLaunchKernelGGL(png_index_kernel<true>, pixel_grid, block, 0, s, raw, P, T, flags);
    else if (P.colour == 3) hipLaunchKernelGGL(png_index_kernel<false>, pixel_grid, block, 0, s, raw, P, T, flags);
    const uint32_t lead = (uint32_t)std::min<unsigned long long>(bytes, (4 - (reinterpret_cast<uintptr_t>(d_out) & 3u)) & 3u);
    const unsigned long long lanes = (bytes - lead) / 4 + lead + (bytes - lead) % 4;
    const dim3 out_grid((uint32_t)((lanes + BLOCK - 1) / BLOCK));
    if (laced) hipLaunchKernelGGL(png_convert_kernel<true>, out_grid, block, 0, s, raw, d_palette, P, T, channels, d_out, bytes, lead, flags);
    else hipLaunchKernelGGL(png_convert_kernel<false>, out_grid, block, 0, s, raw, d_palette, P, T, channels, d_out, bytes, lead, flags);
    e = hipGetLastError();
    if (e == hipSuccess) e = hipMemcpyAsync(h_flags, flags, sizeof(h_flags), hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) return device_error(name_, e);
    keep_stats(rounds);
    if (h_flags[F_ERR]) return file_error(name, h_flags[F_ERR], laced);
    e = sc.copy_out(out, d_out, (size_t)bytes, s);
    if (e == hipSuccess) e = sc.drain(s);
    if (e != hipSuccess) return device_error(name_, e);
    return CVHIP_OK;
}

} // namespace
} // namespace cvhip

using namespace cvhip;

extern "C" int cvhip_png_info(const uint8_t *file, uint64_t size, uint32_t *out_info) { return info("png_info", false, file, size, out_info); }

extern "C" int cvhip_png_last_stats(uint64_t *out_stats)
{
    if (!out_stats) return fail(CVHIP_ERR_INVALID, "png_last_stats: null argument");
    for (int k = 0; k < 8; k++) out_stats[k] = t_stats[k];
    return CVHIP_OK;
}

extern "C" int cvhip_png_decode(cvhip_device *dev, const uint8_t *file, uint64_t size, uint32_t format, uint32_t drop_rows, uint8_t *out,
                                uint64_t cap, uint64_t *out_size)
{
    return decode("png_decode", false, t_stats, dev, file, size, format, drop_rows, out, cap, out_size);
}

// ---- the superset: Adam7 files too ------------------------------------------------------------------------------------
extern "C" int cvhip_png_ext_info(const uint8_t *file, uint64_t size, uint32_t *out_info) { return info("png_ext_info", true, file, size, out_info); }

extern "C" int cvhip_png_ext_last_stats(uint64_t *out_stats)
{
    if (!out_stats) return fail(CVHIP_ERR_INVALID, "png_ext_last_stats: null argument");
    for (int k = 0; k < 10; k++) out_stats[k] = t_ext_stats[k];
    return CVHIP_OK;
}

extern "C" int cvhip_png_ext_decode(cvhip_device *dev, const uint8_t *file, uint64_t size, uint32_t format, uint32_t drop_rows, uint8_t *out,
                                    uint64_t cap, uint64_t *out_size)
{
    return decode("png_ext_decode", true, t_ext_stats, dev, file, size, format, drop_rows, out, cap, out_size);
}
