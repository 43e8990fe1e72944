// jpeg_encode_kernels.hip — cvhip_jpeg_encode: the baseline JPEG file of an 8-bit image with 1 to 4 channels, made on the
// device.  The reference saves its depth map with img.save (src/output.rs:1141), and a path that ends in .jpg
// makes that a JPEG file.  The file is libjpeg's (tests/ref_jpeg_out.py restates it, tests/test_jpeg_out_ref.py pins the
// restatement to Pillow byte for byte): JFIF header, the Annex K tables scaled by the quality, jccolor's YCbCr, jcsample's
// h2v1 / h2v2 downsampling with its edge rules, jfdctint, one interleaved scan, the Annex K Huffman tables or libjpeg's
// optimal ones.  The host writes the segments in front of the scan (jpeg_encode_common.hpp).
//
//   jpeg_transform_kernel   eight lanes a block, a row each: colour conversion, edge replication and downsampling while the
//                           row is loaded, the row pass in registers, the transpose through LDS, the column pass, the
//                           quantisation -> int16 coefficients in zigzag order, the blocks in scan (MCU) order, dummy blocks
//                           (the luma blocks of an edge MCU that lie beyond the component) zero
//   jpeg_dummy_dc_kernel    a dummy block's DC = the DC of the block before it in its MCU (only when there are dummies)
//   jpeg_entropy_kernel     a lane a block, its symbols walked once: <HIST> the counts of the four tables, gathered per
//                           workgroup in LDS and added by vector atomics, to the HOST - the optimal tables come back, the
//                           one round trip besides the sizes; <!HIST> the block's bits under the code table, summed within
//                           its chunk of 256 blocks by the workgroup
//   (launch_scan_u64)       places the chunks
//   jpeg_write_kernel       a lane a block, its codes shifted into 32-bit words: the words a block owns alone leave by plain
//                           stores, the word it shares with a neighbour at either end by atomicOr into the zeroed,
//                           unstuffed stream - about 20 flat blocks share one; one-bits pad the last byte
//   jpeg_stuff_count_kernel the FF bytes of every 1024-byte tile of that stream; a second scan places the tiles
//   jpeg_stuff_copy_kernel  a tile's bytes with a zero behind every FF, assembled in LDS, to `out` behind the header: aligned
//                           dwords where a dword lies wholly in the tile's range, bytes at its two ends
#include <cstring>

#include "cvhip_internal.hpp"

#include "jpeg_encode_common.hpp"

namespace cvhip {
namespace {

namespace je = jpeg_encode_common;

constexpr int WG = 256;
constexpr uint32_t WG_BLOCKS = WG / 8;          // blocks a workgroup of the transform takes in one step
constexpr uint32_t TILE_WORDS = je::STUFF_TILE / 4;
constexpr uint32_t STAGE_WORDS = 2 * TILE_WORDS + 2; // a tile of FF bytes doubles; 3 bytes of misalignment in front
static_assert(TILE_WORDS == WG, "a lane of the stuffing pass takes one dword of its tile");

// natural index -> position in zigzag order
struct ZigzagPositions {
    uint8_t at[64];
    constexpr ZigzagPositions() : at()
    {
        for (int i = 0; i < 64; i++) at[je::ZIGZAG[i]] = (uint8_t)i;
    }
};
constexpr ZigzagPositions ZZ_POS{};

// where block b of the scan lies: its component, its place in the component's block grid, whether it is computed from pixels
struct BlockPlace {
    uint32_t comp, bx, by;
    bool real;
};
__device__ __forceinline__ BlockPlace place_of(const je::Geometry &g, unsigned long long b)
{
    const unsigned long long mcu = b / g.bpm;
    const uint32_t k = (uint32_t)(b % g.bpm), mx = (uint32_t)(mcu % g.mcus_x), my = (uint32_t)(mcu / g.mcus_x), ny = g.hs * g.vs;
    BlockPlace p;
    if (k < ny) {
        p.comp = 0, p.bx = mx * g.hs + k % g.hs, p.by = my * g.vs + k / g.hs;
        p.real = p.bx < g.blocks_x && p.by < g.blocks_y;
    } else
        p.comp = k - ny + 1, p.bx = mx, p.by = my, p.real = true;
    return p;
}
// the block whose DC predicts block b's: the one before it of the same component in scan order, -1 = none (prediction 0)
__device__ __forceinline__ long long predictor_of(const je::Geometry &g, unsigned long long b)
{
    const uint32_t k = (uint32_t)(b % g.bpm), ny = g.hs * g.vs;
    if (k > 0 && k < ny) return (long long)b - 1;
    if (b < g.bpm) return -1;
    return k == 0 ? (long long)(b - g.bpm + ny - 1) : (long long)(b - g.bpm);
}

// jccolor's rgb_ycc_convert for one component
__device__ __forceinline__ int ycc(uint32_t comp, int r, int g, int b)
{
    if (comp == 0) return (19595 * r + 38470 * g + 7471 * b + 32768) >> 16;
    if (comp == 1) return (-11059 * r - 21709 * g + 32768 * b + (128 << 16) + 32767) >> 16;
    return (32768 * r - 27439 * g - 5329 * b + (128 << 16) + 32767) >> 16;
}
// component comp of the pixel (x, y), both inside the image
__device__ __forceinline__ int pixel_value(const uint8_t *__restrict__ pixels, const je::Geometry &g, uint32_t comp, uint32_t x, uint32_t y)
{
    const uint8_t *p = pixels + ((unsigned long long)y * g.width + x) * g.channels;
    return g.components == 1 ? (int)p[0] : ycc(comp, p[0], p[1], p[2]);
}
// Sample (x, y) of component comp's plane as the DCT reads it.  The source row is replicated to the right before the
// downsampling; at the bottom the source is padded to a multiple of the vertical factor only, and it is the downsampled
// rows that are replicated below that (jcprepct's two expand_bottom_edge calls).
__device__ __forceinline__ int sample(const uint8_t *__restrict__ pixels, const je::Geometry &g, uint32_t comp, uint32_t x, uint32_t y)
{
    const uint32_t xl = g.width - 1, yl = g.height - 1;
    if (comp == 0 || g.hs == 1) return pixel_value(pixels, g, comp, min(x, xl), min(y, yl));
    const uint32_t x0 = min(2 * x, xl), x1 = min(2 * x + 1, xl);
    if (g.vs == 1) {
        const uint32_t sy = min(y, yl);
        return (pixel_value(pixels, g, comp, x0, sy) + pixel_value(pixels, g, comp, x1, sy) + (int)(x & 1u)) >> 1; // bias 0, 1, 0, 1, ...
    }
    const uint32_t yd = min(y, (g.height + 1) / 2 - 1), y0 = 2 * yd, y1 = min(2 * yd + 1, yl);
    return (pixel_value(pixels, g, comp, x0, y0) + pixel_value(pixels, g, comp, x1, y0) + pixel_value(pixels, g, comp, x0, y1) +
            pixel_value(pixels, g, comp, x1, y1) + 1 + (int)(x & 1u)) >> 2; // bias 1, 2, 1, 2, ...
}

// one pass of jfdctint (CONST_BITS 13, PASS1_BITS 2) over d[0 .. 8)
template <bool FIRST> __device__ __forceinline__ void fdct_pass(int (&d)[8])
{
    constexpr int CONST_BITS = 13, PASS1_BITS = 2, N = FIRST ? CONST_BITS - PASS1_BITS : CONST_BITS + PASS1_BITS;
    auto descale = [](int x, int n) { return (x + (1 << (n - 1))) >> n; };
    const int t0 = d[0] + d[7], t7 = d[0] - d[7], t1 = d[1] + d[6], t6 = d[1] - d[6];
    const int t2 = d[2] + d[5], t5 = d[2] - d[5], t3 = d[3] + d[4], t4 = d[3] - d[4];
    const int t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
    d[0] = FIRST ? (t10 + t11) * (1 << PASS1_BITS) : descale(t10 + t11, PASS1_BITS);
    d[4] = FIRST ? (t10 - t11) * (1 << PASS1_BITS) : descale(t10 - t11, PASS1_BITS);
    const int e1 = (t12 + t13) * 4433;
    d[2] = descale(e1 + t13 * 6270, N);
    d[6] = descale(e1 - t12 * 15137, N);
    const int z5 = (t4 + t6 + t5 + t7) * 9633;
    const int z1 = -(t4 + t7) * 7373, z2 = -(t5 + t6) * 20995, z3 = -(t4 + t6) * 16069 + z5, z4 = -(t5 + t7) * 3196 + z5;
    d[7] = descale(t4 * 2446 + z1 + z3, N);
    d[5] = descale(t5 * 16819 + z2 + z4, N);
    d[3] = descale(t6 * 25172 + z2 + z3, N);
    d[1] = descale(t7 * 12299 + z1 + z4, N);
}

// quant8[2][64]: the luma and the chroma table times 8, natural order.  coefs: 64 int16 a block, zigzag order, scan order.
__global__ __launch_bounds__(WG) void jpeg_transform_kernel(const uint8_t *__restrict__ pixels, je::Geometry g, const uint16_t *__restrict__ quant8,
                                                            unsigned long long n_blocks, int16_t *__restrict__ coefs)
{
    __shared__ int s_rows[WG_BLOCKS][8][9]; // the row pass's results; a row of 9 so that the column read spreads over the banks
    __shared__ uint32_t s_out[WG_BLOCKS * 32];
    __shared__ uint16_t s_quant[128];
    __shared__ uint8_t s_zz[64];
    const uint32_t tid = threadIdx.x, blk = tid >> 3, r = tid & 7u;
    if (tid < 128) s_quant[tid] = quant8[tid];
    if (tid < 64) s_zz[tid] = ZZ_POS.at[tid];
    __syncthreads();
    int16_t *out16 = reinterpret_cast<int16_t *>(s_out);
    for (unsigned long long base = (unsigned long long)blockIdx.x * WG_BLOCKS; base < n_blocks; base += (unsigned long long)gridDim.x * WG_BLOCKS) {
        const unsigned long long b = base + blk;
        const bool valid = b < n_blocks;
        BlockPlace p = {0, 0, 0, false};
        if (valid) p = place_of(g, b);
        int d[8];
        if (p.real) {
#pragma unroll
            for (uint32_t j = 0; j < 8; j++) d[j] = sample(pixels, g, p.comp, p.bx * 8 + j, p.by * 8 + r) - 128;
            fdct_pass<true>(d);
#pragma unroll
            for (uint32_t j = 0; j < 8; j++) s_rows[blk][r][j] = d[j];
        }
        __syncthreads();
        if (p.real) { // now the column r
#pragma unroll
            for (uint32_t i = 0; i < 8; i++) d[i] = s_rows[blk][i][r];
            fdct_pass<false>(d);
            const uint16_t *q = s_quant + (p.comp ? 64 : 0);
#pragma unroll
            for (uint32_t i = 0; i < 8; i++) {
                const uint32_t q8 = q[i * 8 + r], mag = ((uint32_t)abs(d[i]) + (q8 >> 1)) / q8;
                out16[blk * 64 + s_zz[i * 8 + r]] = (int16_t)(d[i] < 0 ? -(int)mag : (int)mag);
            }
        } else {
#pragma unroll
            for (uint32_t j = 0; j < 4; j++) s_out[blk * 32 + r * 4 + j] = 0;
        }
        __syncthreads();
        uint32_t *dst = reinterpret_cast<uint32_t *>(coefs) + base * 32;
        const unsigned long long words = min((unsigned long long)WG_BLOCKS, n_blocks - base) * 32;
#pragma unroll
        for (uint32_t t = 0; t < 4; t++)
            if (tid + t * WG < words) dst[tid + t * WG] = s_out[tid + t * WG];
        __syncthreads();
    }
}

// A dummy block takes the DC of the block before it in its MCU; that block may be a dummy too, the first of an MCU never is.
__global__ __launch_bounds__(WG) void jpeg_dummy_dc_kernel(je::Geometry g, unsigned long long n_blocks, int16_t *__restrict__ coefs)
{
    for (unsigned long long b = (unsigned long long)blockIdx.x * WG + threadIdx.x; b < n_blocks; b += (unsigned long long)gridDim.x * WG) {
        if (place_of(g, b).real) continue;
        unsigned long long src = b - 1;
        while (!place_of(g, src).real) src--;
        coefs[b * 64] = coefs[src * 64];
    }
}

__device__ __forceinline__ uint32_t category(int v)
{
    const uint32_t a = (uint32_t)abs(v);
    return a ? 32u - (uint32_t)__clz(a) : 0u;
}
// The symbols of a block (64 coefficients in zigzag order, the DC predicted by pred): emit(index, value, n) once per symbol -
// index into a table pair (jpeg_encode_common.hpp's kernel_table: the DC category, or 16 + the AC symbol), the n value bits.
template <typename Emit> __device__ __forceinline__ void block_symbols(const int16_t *__restrict__ c, int pred, Emit &&emit)
{
    const uint32_t *words = reinterpret_cast<const uint32_t *>(c);
    uint32_t run = 0;
    auto one = [&](int v) {
        if (v == 0) {
            run++;
            return;
        }
        for (; run > 15; run -= 16) emit(16u + 0xF0u, 0u, 0u);
        const uint32_t n = category(v);
        emit(16u + (run << 4 | n), (uint32_t)(v < 0 ? v - 1 : v) & ((1u << n) - 1u), n);
        run = 0;
    };
    for (uint32_t i = 0; i < 32; i++) {
        const uint32_t w = words[i];
        const int lo = (int16_t)(w & 0xFFFFu), hi = (int16_t)(w >> 16);
        if (i == 0) {
            const int diff = lo - pred;
            const uint32_t n = category(diff);
            emit(n, (uint32_t)(diff < 0 ? diff - 1 : diff) & ((1u << n) - 1u), n);
        } else
            one(lo);
        one(hi);
    }
    if (run) emit(16u, 0u, 0u); // EOB
}

// the exclusive sum of v over the workgroup's lanes; total = the sum over all of them
__device__ __forceinline__ uint32_t workgroup_scan(uint32_t v, uint32_t *s_waves, uint32_t &total)
{
    uint32_t incl = v;
#pragma unroll
    for (int s = 1; s < 64; s <<= 1) {
        const uint32_t t = __shfl_up(incl, s, 64);
        if ((int)(threadIdx.x & 63) >= s) incl += t;
    }
    __syncthreads(); // (s_waves is free again)
    if ((threadIdx.x & 63) == 63) s_waves[threadIdx.x >> 6] = incl;
    __syncthreads();
    uint32_t before = 0;
    total = 0;
#pragma unroll
    for (uint32_t w = 0; w < WG / 64; w++) {
        if (w < (threadIdx.x >> 6)) before += s_waves[w];
        total += s_waves[w];
    }
    return before + incl - v;
}

// HIST: out32[TABLE_ENTRIES] += the counts of the symbols, per table pair.  !HIST, a chunk of WG blocks a workgroup: out32[b] =
// the bits, under `table`, of the blocks before b in its chunk, out64[chunk] = the chunk's bits (at most 256 * 1665 a chunk).
template <bool HIST>
__global__ __launch_bounds__(WG) void jpeg_entropy_kernel(const int16_t *__restrict__ coefs, je::Geometry g, unsigned long long n_blocks,
                                                          const uint32_t *__restrict__ table, uint32_t *__restrict__ out32,
                                                          unsigned long long *__restrict__ out64)
{
    __shared__ uint32_t s_table[je::TABLE_ENTRIES]; // HIST: the counters
    __shared__ uint32_t s_waves[WG / 64];
    for (uint32_t k = threadIdx.x; k < je::TABLE_ENTRIES; k += WG) s_table[k] = HIST ? 0u : table[k];
    __syncthreads();
    const unsigned long long chunks = (n_blocks + WG - 1) / WG;
    for (unsigned long long chunk = blockIdx.x; chunk < chunks; chunk += gridDim.x) {
        const unsigned long long b = chunk * WG + threadIdx.x;
        uint32_t bits = 0;
        if (b < n_blocks) {
            const long long before = predictor_of(g, b);
            const int pred = before < 0 ? 0 : (int)coefs[before * 64];
            uint32_t *pair = s_table + ((b % g.bpm) >= g.hs * g.vs ? je::TABLE_SYMBOLS : 0);
            block_symbols(coefs + b * 64, pred, [&](uint32_t index, uint32_t, uint32_t n) {
                if (HIST) atomicAdd(&pair[index], 1u);
                else bits += (pair[index] >> 16) + n;
            });
        }
        if (!HIST) {
            uint32_t total;
            const uint32_t in_front = workgroup_scan(bits, s_waves, total);
            if (b < n_blocks) out32[b] = in_front;
            if (threadIdx.x == 0) out64[chunk] = total;
        }
    }
    if (HIST) {
        __syncthreads();
        for (uint32_t k = threadIdx.x; k < je::TABLE_ENTRIES; k += WG)
            if (s_table[k]) atomicAdd(&out32[k], s_table[k]);
    }
}

// Bit k of the scan's data, before the stuffing, is bit 7 - k % 8 of byte k / 8 of `stream` (zeroed, 4-byte aligned, whole
// dwords); chunk_start[b / WG] + offsets[b] = the bits of the blocks before b (jpeg_entropy_kernel and a scan of its chunk
// sums).  pad_bits one-bits follow the last block.
__global__ __launch_bounds__(WG) void jpeg_write_kernel(const int16_t *__restrict__ coefs, je::Geometry g, unsigned long long n_blocks,
                                                        const uint32_t *__restrict__ table, const unsigned long long *__restrict__ chunk_start,
                                                        const uint32_t *__restrict__ offsets, uint32_t pad_bits, uint32_t *__restrict__ stream)
{
    __shared__ uint32_t s_table[je::TABLE_ENTRIES];
    for (uint32_t k = threadIdx.x; k < je::TABLE_ENTRIES; k += WG) s_table[k] = table[k];
    __syncthreads();
    for (unsigned long long b = (unsigned long long)blockIdx.x * WG + threadIdx.x; b < n_blocks; b += (unsigned long long)gridDim.x * WG) {
        const long long before = predictor_of(g, b);
        const int pred = before < 0 ? 0 : (int)coefs[before * 64];
        const uint32_t *pair = s_table + ((b % g.bpm) >= g.hs * g.vs ? je::TABLE_SYMBOLS : 0);
        const unsigned long long at = chunk_start[b / WG] + offsets[b];
        unsigned long long word = at >> 5, acc = 0; // acc: the `fill` bits of dword `word` so far, the first one highest
        uint32_t fill = (uint32_t)(at & 31u);
        bool shared = fill != 0; // dword `word` holds bits of the block in front
        auto put = [&](uint32_t value, uint32_t n) {
            acc = acc << n | value;
            fill += n;
            if (fill >= 32) {
                fill -= 32;
                const uint32_t w = __builtin_bswap32((uint32_t)(acc >> fill));
                if (shared) atomicOr(&stream[word], w);
                else stream[word] = w;
                shared = false, word++;
                acc &= (1ull << fill) - 1ull;
            }
        };
        block_symbols(coefs + b * 64, pred, [&](uint32_t index, uint32_t value, uint32_t n) {
            const uint32_t entry = pair[index];
            put((entry & 0xFFFFu) << n | value, (entry >> 16) + n); // (at most 16 + 11 bits)
        });
        if (b == n_blocks - 1 && pad_bits) put((1u << pad_bits) - 1u, pad_bits);
        if (fill) atomicOr(&stream[word], __builtin_bswap32((uint32_t)(acc << (32 - fill)))); // shared with what follows
    }
}

__device__ __forceinline__ uint32_t ff_bytes(uint32_t w, uint32_t valid)
{
    uint32_t n = 0;
#pragma unroll
    for (uint32_t k = 0; k < 4; k++) n += (k < valid && ((w >> (8 * k)) & 0xFFu) == 0xFFu) ? 1u : 0u;
    return n;
}
// the lane's dword of tile `tile` and how many of its bytes lie in the stream of n bytes
__device__ __forceinline__ uint32_t tile_word(const uint32_t *__restrict__ stream, unsigned long long n, unsigned long long tile, uint32_t &valid)
{
    const unsigned long long at = tile * je::STUFF_TILE + 4ull * threadIdx.x;
    valid = at >= n ? 0u : (uint32_t)min(4ull, n - at);
    return valid ? stream[at >> 2] : 0u;
}
// counts[tile] = the FF bytes of the tile
__global__ __launch_bounds__(WG) void jpeg_stuff_count_kernel(const uint32_t *__restrict__ stream, unsigned long long n, unsigned long long tiles,
                                                              unsigned long long *__restrict__ counts)
{
    __shared__ uint32_t s_waves[WG / 64];
    for (unsigned long long tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        uint32_t valid, total;
        const uint32_t w = tile_word(stream, n, tile, valid);
        workgroup_scan(ff_bytes(w, valid), s_waves, total);
        if (threadIdx.x == 0) counts[tile] = total;
    }
}

// before[tile] = the FF bytes of the tiles in front.  data: where the scan's data begins in the file image, at any alignment.
__global__ __launch_bounds__(WG) void jpeg_stuff_copy_kernel(const uint32_t *__restrict__ stream, unsigned long long n, unsigned long long tiles,
                                                             const unsigned long long *__restrict__ before, uint8_t *__restrict__ data)
{
    __shared__ uint32_t s_waves[WG / 64];
    __shared__ uint32_t s_stage[STAGE_WORDS];
    uint8_t *stage = reinterpret_cast<uint8_t *>(s_stage);
    for (unsigned long long tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        uint8_t *dst = data + tile * je::STUFF_TILE + before[tile];
        const uint32_t front = (uint32_t)(reinterpret_cast<uintptr_t>(dst) & 3u);
        uint32_t valid, length;
        const uint32_t w = tile_word(stream, n, tile, valid);
        uint32_t at = front + workgroup_scan(valid + ff_bytes(w, valid), s_waves, length);
        for (uint32_t k = 0; k < valid; k++) {
            const uint8_t byte = (uint8_t)(w >> (8 * k));
            stage[at++] = byte;
            if (byte == 0xFFu) stage[at++] = 0;
        }
        __syncthreads();
        uint8_t *aligned = dst - front; // stage[k] belongs at aligned[k] for front <= k < front + length
        const uint32_t end = front + length;
        for (uint32_t j = threadIdx.x; 4 * j < end; j += WG) {
            if (4 * j >= front && 4 * j + 4 <= end)
                reinterpret_cast<uint32_t *>(aligned)[j] = s_stage[j];
            else
                for (uint32_t k = max(4 * j, front); k < min(4 * j + 4, end); k++) aligned[k] = stage[k];
        }
        __syncthreads();
    }
}

thread_local uint64_t t_stats[4] = {0, 0, 0, 0}; // of the thread's last encode: blocks, dummy blocks, bits before the stuffing, stuffed bytes

} // namespace
} // namespace cvhip

using namespace cvhip;

extern "C" int cvhip_jpeg_encode_last_stats(uint64_t *out_stats)
{
    if (!out_stats) return fail(CVHIP_ERR_INVALID, "jpeg_encode_last_stats: null argument");
    for (int k = 0; k < 4; k++) out_stats[k] = t_stats[k];
    return CVHIP_OK;
}

extern "C" int cvhip_jpeg_encode(cvhip_device *dev, const uint8_t *pixels, uint32_t width, uint32_t height, uint32_t channels, uint32_t quality,
                                 uint32_t sampling, uint32_t optimize, uint8_t *out, uint64_t cap, uint64_t *out_size, uint64_t *out_sections)
{
    if (!dev || !pixels || !out_size || (cap && !out)) return fail(CVHIP_ERR_INVALID, "jpeg_encode: null argument");
    if (!width || !height || width > 65535 || height > 65535) return fail(CVHIP_ERR_INVALID, "jpeg_encode: width or height is not 1 to 65535");
    if (channels < 1 || channels > 4) return fail(CVHIP_ERR_INVALID, "jpeg_encode: channels is not 1, 2, 3 or 4");
    if (quality < 1 || quality > 100) return fail(CVHIP_ERR_INVALID, "jpeg_encode: quality is not 1 to 100");
    if (sampling > CVHIP_JPEG_SAMPLING_420) return fail(CVHIP_ERR_INVALID, "jpeg_encode: sampling is not 0 (4:4:4), 1 (4:2:2) or 2 (4:2:0)");
    if (optimize > 1) return fail(CVHIP_ERR_INVALID, "jpeg_encode: optimize is not 0 or 1");
    const je::Geometry g = je::geometry(width, height, channels, sampling);
    const unsigned long long n_blocks = je::total_blocks(g), dummies = je::dummy_blocks(g);
    if (n_blocks > je::MAX_BLOCKS) return fail(CVHIP_ERR_UNSUPPORTED, "jpeg_encode: more than 2^25 blocks");
    const uint32_t pairs = g.components == 3 ? 2 : 1;
    uint16_t quants[2][64], quant8[128] = {0};
    je::quant_table(je::QUANT_LUMA, quality, quants[0]);
    je::quant_table(je::QUANT_CHROMA, quality, quants[1]);
    for (int k = 0; k < 128; k++) quant8[k] = (uint16_t)(quants[k >> 6][k & 63] * 8);
    CVHIP_TRY_HIP(hipSetDevice(dev->d.ordinal));
    hipStream_t s = dev->d.stream;
    CallScratch sc;
    const uint8_t *d_pixels = nullptr;
    int16_t *coefs = nullptr;
    uint16_t *d_quant8 = nullptr;
    uint32_t *words32 = nullptr, *block_offsets = nullptr; // the code table, the histogram; a block's bits offset in its chunk
    unsigned long long *chunk_bits = nullptr, total_bits = 0, stuffed = 0;
    const unsigned long long chunks = (n_blocks + WG - 1) / WG;
    hipError_t e = sc.input(pixels, (size_t)width * height * channels, &d_pixels, s);
    if (e == hipSuccess) e = sc.alloc(&coefs, (size_t)n_blocks * 64);
    if (e == hipSuccess) e = sc.alloc(&d_quant8, 128);
    if (e == hipSuccess) e = sc.alloc(&words32, 2 * je::TABLE_ENTRIES);
    if (e == hipSuccess) e = sc.alloc(&block_offsets, (size_t)n_blocks);
    if (e == hipSuccess) e = sc.alloc(&chunk_bits, (size_t)chunks + 1);
    if (e == hipSuccess) e = hipMemcpyAsync(d_quant8, quant8, sizeof(quant8), hipMemcpyHostToDevice, s);
    if (e != hipSuccess) return device_error("jpeg_encode", e);
    uint32_t *table = words32, *histogram = words32 + je::TABLE_ENTRIES;
    const dim3 wg(WG), lanes_grid(grid_for(n_blocks));
    const dim3 transform_grid((uint32_t)std::min<unsigned long long>(CVHIP_MESH_GRID_LANES / WG, (n_blocks + WG_BLOCKS - 1) / WG_BLOCKS));
    hipLaunchKernelGGL(jpeg_transform_kernel, transform_grid, wg, 0, s, d_pixels, g, d_quant8, n_blocks, coefs);
    if (dummies) hipLaunchKernelGGL(jpeg_dummy_dc_kernel, lanes_grid, wg, 0, s, g, n_blocks, coefs);
    je::HuffSpec specs[4];
    for (uint32_t k = 0; k < 2 * pairs; k++) specs[k] = je::standard_table(k);
    if (optimize) { // ---- the round trip: the histograms out, the tables back
        uint32_t h_histogram[je::TABLE_ENTRIES];
        e = hipMemsetAsync(histogram, 0, sizeof(h_histogram), s);
        if (e != hipSuccess) return device_error("jpeg_encode", e);
        hipLaunchKernelGGL(jpeg_entropy_kernel<true>, lanes_grid, wg, 0, s, coefs, g, n_blocks, nullptr, histogram, nullptr);
        e = hipGetLastError();
        if (e == hipSuccess) e = hipMemcpyAsync(h_histogram, histogram, sizeof(h_histogram), hipMemcpyDeviceToHost, s);
        if (e == hipSuccess) e = hipStreamSynchronize(s);
        if (e != hipSuccess) return device_error("jpeg_encode", e);
        for (uint32_t k = 0; k < 2 * pairs; k++) {
            uint64_t freq[256] = {0};
            const uint32_t *h = h_histogram + (k >> 1) * je::TABLE_SYMBOLS + (k & 1u) * 16;
            for (uint32_t i = 0; i < ((k & 1u) ? 256u : 16u); i++) freq[i] = h[i];
            specs[k] = je::optimal_table(freq);
        }
    }
    uint32_t h_table[je::TABLE_ENTRIES];
    je::kernel_table(specs, 2 * pairs, h_table);
    e = hipMemcpyAsync(table, h_table, sizeof(h_table), hipMemcpyHostToDevice, s);
    if (e != hipSuccess) return device_error("jpeg_encode", e);
    hipLaunchKernelGGL(jpeg_entropy_kernel<false>, lanes_grid, wg, 0, s, coefs, g, n_blocks, table, block_offsets, chunk_bits);
    launch_scan_u64(chunk_bits, chunks, chunk_bits + chunks, s);
    e = hipGetLastError();
    if (e == hipSuccess) e = hipMemcpyAsync(&total_bits, chunk_bits + chunks, sizeof(total_bits), hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) return device_error("jpeg_encode", e);
    // ---- the unstuffed stream, and its FF bytes: the file's size is known only behind them
    const unsigned long long stream_bytes = (total_bits + 7) / 8, stream_words = (stream_bytes + 3) / 4;
    const unsigned long long tiles = (stream_bytes + je::STUFF_TILE - 1) / je::STUFF_TILE;
    const uint32_t pad_bits = (uint32_t)(stream_bytes * 8 - total_bits);
    uint32_t *stream = nullptr;
    unsigned long long *tile_ff = nullptr;
    e = sc.alloc(&stream, (size_t)stream_words);
    if (e == hipSuccess) e = sc.alloc(&tile_ff, (size_t)tiles + 1);
    if (e == hipSuccess) e = hipMemsetAsync(stream, 0, (size_t)stream_words * 4, s);
    if (e != hipSuccess) return device_error("jpeg_encode", e);
    const dim3 tile_grid((uint32_t)std::min<unsigned long long>(CVHIP_MESH_GRID_LANES / WG, tiles));
    hipLaunchKernelGGL(jpeg_write_kernel, lanes_grid, wg, 0, s, coefs, g, n_blocks, table, chunk_bits, block_offsets, pad_bits, stream);
    hipLaunchKernelGGL(jpeg_stuff_count_kernel, tile_grid, wg, 0, s, stream, stream_bytes, tiles, tile_ff);
    launch_scan_u64(tile_ff, tiles, tile_ff + tiles, s);
    e = hipGetLastError();
    if (e == hipSuccess) e = hipMemcpyAsync(&stuffed, tile_ff + tiles, sizeof(stuffed), hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) return device_error("jpeg_encode", e);
    const std::vector<uint8_t> header = je::header(g, quants, specs);
    const uint64_t data_bytes = stream_bytes + stuffed, size = header.size() + data_bytes + 2;
    t_stats[0] = n_blocks, t_stats[1] = dummies, t_stats[2] = total_bits, t_stats[3] = stuffed;
    *out_size = size;
    if (out_sections) out_sections[0] = header.size(), out_sections[1] = data_bytes, out_sections[2] = 2;
    if (!cap) return CVHIP_OK;
    if (cap < size) return fail(CVHIP_ERR_INVALID, "jpeg_encode: the buffer is smaller than the file image");
    // ---- the file image: the segments composed here, the data with its zero bytes, EOI
    uint8_t *d_out = nullptr;
    e = sc.output(out, (size_t)size, &d_out);
    if (e != hipSuccess) return device_error("jpeg_encode", e);
    static const uint8_t eoi[2] = {0xFF, 0xD9};
    e = hipMemcpyAsync(d_out, header.data(), header.size(), hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipMemcpyAsync(d_out + header.size() + data_bytes, eoi, 2, hipMemcpyHostToDevice, s);
    if (e != hipSuccess) return device_error("jpeg_encode", e);
    hipLaunchKernelGGL(jpeg_stuff_copy_kernel, tile_grid, wg, 0, s, stream, stream_bytes, tiles, tile_ff, d_out + header.size());
    e = hipGetLastError();
    if (e == hipSuccess) e = sc.copy_out(out, d_out, (size_t)size, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) return device_error("jpeg_encode", e);
    return CVHIP_OK;
}
