// png_decode_kernels.hip — cvhip_png_decode: a PNG file to Luma8 or RGB8 pixels, everything behind the chunk walk on the device
// (DESIGN.md 4.18).  The reference opens its inputs with image::open(path)?.into_luma8() / into_rgb8()
// (src/reconstruction.rs:40-60); tests/ref_png_in.py is the definition of the pixels.  The host (png_decode_common.hpp) walks
// the chunks, checks the CRC of the small ones and reads IHDR, PLTE and eXIf; the palette, the IDAT table and the IDAT
// payloads, end to end, go up in one copy.
//
//   png_crc_kernel       a workgroup per IDAT chunk: the CRC-32 of 256 pieces, combined with png_common.hpp's arithmetic
//   png_chain_kernel     one workgroup walks the chain of deflate blocks, whose headers can only be found in order.  A
//                        dynamic block's code lengths are read by one lane, the tables are built in LDS; inside the block
//                        the decode is the self-synchronising one of jpeg_sync_kernel: a lane per subsequence of
//                        SUBSEQ_BITS bits, the state is the bit offset of a whole token, lanes decode again from their left
//                        neighbour's exit until nothing changes.  A window of 256 subsequences, its part of the stream in
//                        LDS, settles completely before the next one starts from its last exit, so nothing waits for
//                        another workgroup.  A lane does not take over "ended" from its left (a false end-of-block would
//                        be handed down the window a lane a round); only the first end-of-block of the settled chain, in
//                        front of which every lane holds its true state, ends the block.  Out come records (entry state, output bytes) per
//                        subsequence, and per 1024 bytes of a stored block a (source, length) record
//   launch_scan_u64      the output position of every record
//   png_write_kernel     a workgroup per window: the block's tables again (from its header), one more decode from the
//                        settled states: literals to the filtered image, and per output byte its source index (itself
//                        for a literal, o - distance for a copy)
//   png_resolve_kernel   pointer doubling over the source indices, two buffers, until a launch changes nothing
//   png_gather_kernel    every byte from its literal; the Adler-32 sums of the whole
//   png_finish_kernel    the Adler-32 behind the last block against those sums
//   png_unfilter_kernel  a workgroup per row segment - None and Sub rows start one -: tiles of 64 rows through LDS, a lane of
//                        the first wave per row, skewed by one pixel per lane, `up` and `up-left` by a shuffle from the lane above
//   png_index_kernel     colour type 3: no index beyond the PLTE
//   png_convert_kernel   a lane per aligned dword of `out`: samples to 8 bits, palette, luma, drop_rows
// cvhip_png_ext_decode (tests/ref_png_adam7.py) is the same body for a superset of the files: Adam7
// interlaced ones too.  Their stream is the seven reduced images one behind the other; the last three kernels are templates
// on ADAM7 - the unfilter launch covers the rows of all passes and a workgroup finds its pass in a table passed by value,
// the index and convert kernels map a pixel to its pass, row and sample - and a file that is not interlaced runs the
// <false> instantiations, which are what these kernels were before.
// A decode from a wrong state is harmless: every read is bounded by the stream's end (32 zero bytes follow it), every step
// consumes at least one bit, and a code that does not exist consumes one.  In the write pass, whose states are the true
// ones, the same events are the file's errors.  Once flags[F_ERR] is set no kernel writes to `out`.
#include <cstring>
#include <vector>

#include "cvhip_internal.hpp"

#include "png_decode_common.hpp"

namespace cvhip {
namespace {

namespace pd = png_decode_common;
namespace pc = png_common;

#include "inflate_device.inc"

struct Status { // read back in one copy
    unsigned long long values[VALUES];
    uint32_t flags[FLAGS];
};

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

// ---- the chain of blocks ---------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(BLOCK) void png_chain_kernel(const uint32_t *__restrict__ words, unsigned long long n_bytes, unsigned long long *__restrict__ win,
                                                          unsigned long long max_windows, unsigned long long *__restrict__ rec_entry,
                                                          unsigned long long *__restrict__ rec_count, unsigned long long max_records,
                                                          uint32_t *__restrict__ flags, unsigned long long *__restrict__ values)
{
    __shared__ Tables T;
    __shared__ uint32_t s_stream[WINDOW_WORDS];
    __shared__ unsigned long long s_exit[BLOCK], s_p, s_eob;
    __shared__ uint32_t s_err, s_btype, s_final, s_first, s_len;
    const uint32_t tid = threadIdx.x;
    const unsigned long long total_bits = n_bytes * 8;
    if (tid == 0) { // the zlib header
        uint32_t err = 0;
        if (n_bytes < 2) err = ERR_END;
        else {
            const uint32_t cmf = words[0] & 255u, flg = (words[0] >> 8) & 255u;
            if ((cmf & 15u) != 8 || (cmf >> 4) > 7 || (flg & 32u) || ((cmf << 8 | flg) % 31u)) err = ERR_ZLIB;
        }
        s_err = err;
    }
    __syncthreads();
    uint32_t err = s_err, stored = 0, fixed = 0, dynamic = 0, most_rounds = 0, subsequences = 0;
    unsigned long long p = 16, n_win = 0, n_rec = 0, windows = 0;
    bool final_seen = false;
    // (every block takes at least three bits: the bound holds whatever the file says)
    for (unsigned long long blocks = 0; !err && !final_seen && blocks <= total_bits; blocks++) {
        const unsigned long long header = p;
        __syncthreads(); // (the shared words of the block before are read)
        if (tid == 0) {
            uint32_t e = 0;
            unsigned long long q = p + 3;
            if (q > total_bits) e = ERR_END;
            else {
                const uint32_t b = peek(words, p);
                s_final = b & 1u, s_btype = (b >> 1) & 3u;
                if (s_btype == 3) e = ERR_BLOCK;
                else if (s_btype == 0) {
                    q = (q + 7) & ~7ull;
                    if (q + 32 > total_bits) e = ERR_END;
                    else {
                        const uint32_t v = peek(words, q);
                        s_len = v & 0xFFFFu;
                        if ((s_len ^ 0xFFFFu) != (v >> 16)) e = ERR_BLOCK;
                        q += 32;
                        if (!e && q + 8ull * s_len > total_bits) e = ERR_END;
                    }
                }
            }
            s_err = e, s_p = q;
        }
        __syncthreads();
        err = s_err;
        if (err) break;
        const uint32_t btype = s_btype;
        final_seen = s_final != 0;
        if (btype == 0) { // a stored block: a record per PIECE bytes
            stored++;
            const unsigned long long first_byte = s_p >> 3, length = s_len;
            for (unsigned long long done = 0; done < length; done += (unsigned long long)BLOCK * PIECE) {
                const unsigned long long pieces = min((unsigned long long)BLOCK, (length - done + PIECE - 1) / PIECE);
                if (n_win + 1 > max_windows || n_rec + pieces > max_records) {
                    err = ERR_ROOM;
                    break;
                }
                if (tid < pieces) {
                    const unsigned long long at = done + (unsigned long long)tid * PIECE;
                    rec_entry[n_rec + tid] = first_byte + at, rec_count[n_rec + tid] = min((unsigned long long)PIECE, length - at);
                }
                if (tid == 0) win[WIN_WORDS * n_win] = header | pieces << 44, win[WIN_WORDS * n_win + 1] = 0, win[WIN_WORDS * n_win + 2] = n_rec;
                n_win++, n_rec += pieces, windows++;
            }
            p = s_p + 8 * length;
            continue;
        }
        if (btype == 1) fixed++;
        else dynamic++;
        // the header's words to LDS first (HEADER_WORDS hold the longest one): one lane reads them, a load from memory each time otherwise
        const unsigned long long header_word = p >> 5;
        for (uint32_t k = tid; k < HEADER_WORDS; k += BLOCK) s_stream[k] = header_word + k < (n_bytes + 32) / 4 ? words[header_word + k] : 0u;
        __syncthreads();
        err = load_tables(s_stream, header_word, p + 3, total_bits, btype, T, &s_err, &s_p);
        if (err) break;
        unsigned long long base = s_p, entry0 = s_p;
        bool block_done = false;
        while (!err && !block_done) { // a window of BLOCK subsequences; each takes BLOCK x SUBSEQ_BITS bits of the stream
            if (base >= total_bits) {
                err = ERR_END; // the stream ends before the block's end-of-block
                break;
            }
            windows++;
            const unsigned long long first_bit = base + (unsigned long long)tid * pd::SUBSEQ_BITS;
            const bool active = first_bit < total_bits;
            const unsigned long long end_bit = min(first_bit + pd::SUBSEQ_BITS, total_bits);
            const unsigned long long n_active = min((unsigned long long)BLOCK, (total_bits - base + pd::SUBSEQ_BITS - 1) / pd::SUBSEQ_BITS);
            // the window's part of the stream to LDS: in this one workgroup every load from memory would be waited for
            const unsigned long long word_base = base >> 5, stream_words = (n_bytes + 32) / 4;
#pragma unroll 8
            for (uint32_t k = tid; k < WINDOW_WORDS; k += BLOCK) s_stream[k] = word_base + k < stream_words ? words[word_base + k] : 0u;
            __syncthreads();
            unsigned long long cur_entry = tid == 0 ? entry0 : first_bit, cur_exit = ENDED, count = 0, eob_after = 0;
            if (active) cur_exit = cur_entry >= end_bit ? cur_entry : decode_subsequence<false>(s_stream, word_base, T, cur_entry, end_bit, count, eob_after, nullptr, nullptr, 0, 0, nullptr);
            s_exit[tid] = cur_exit;
            if (tid == 0) s_first = BLOCK;
            uint32_t rounds = 0;
            for (uint32_t r = 0; r <= BLOCK; r++) { // lane k holds its true state after k rounds
                __syncthreads();
                // (a left neighbour that met an end-of-block says nothing about this lane: were it the block's end, this lane
                // would not count; were it a false one, adopting it would hand "ended" down the window a lane a round)
                unsigned long long want = (tid && active) ? s_exit[tid - 1] : cur_entry;
                if (want == ENDED) want = cur_entry;
                const bool change = want != cur_entry;
                if (!__syncthreads_or(change)) break; // (and every lane has read before any lane writes)
                if (change) {
                    cur_entry = want, count = 0, eob_after = 0;
                    cur_exit = cur_entry >= end_bit ? cur_entry
                                                                             : decode_subsequence<false>(s_stream, word_base, T, cur_entry, end_bit, count, eob_after, nullptr, nullptr, 0, 0, nullptr);
                    s_exit[tid] = cur_exit;
                }
                rounds++;
            }
            most_rounds = max(most_rounds, rounds);
            const bool ends_here = active && cur_exit == ENDED; // the first such lane: every lane before it holds its true state
            if (ends_here) atomicMin(&s_first, tid);
            __syncthreads();
            const uint32_t jend = s_first;
            const unsigned long long emit = jend < BLOCK ? jend + 1 : n_active;
            subsequences += (uint32_t)emit;
            if (__syncthreads_or(tid < emit && count != 0)) { // (a window without output needs no write pass)
                if (n_win + 1 > max_windows || n_rec + emit > max_records) {
                    err = ERR_ROOM;
                    break;
                }
                if (tid < emit) rec_entry[n_rec + tid] = cur_entry, rec_count[n_rec + tid] = count;
                if (tid == 0)
                    win[WIN_WORDS * n_win] = header | (unsigned long long)btype << 40 | emit << 44, win[WIN_WORDS * n_win + 1] = base,
                                        win[WIN_WORDS * n_win + 2] = n_rec;
                n_win++, n_rec += emit;
            }
            if (jend < BLOCK) {
                if (tid == jend) s_eob = eob_after;
                __syncthreads();
                p = s_eob;
                if (p > total_bits) err = ERR_END;
                block_done = true;
            } else if (n_active < BLOCK) {
                err = ERR_END;
            } else {
                entry0 = s_exit[BLOCK - 1];
                base += (unsigned long long)BLOCK * pd::SUBSEQ_BITS;
                __syncthreads();
            }
        }
    }
    if (!err && !final_seen) err = ERR_END;
    if (!err && (p + 7) / 8 + 4 > n_bytes) err = ERR_END; // the stream ends inside the Adler-32
    if (tid == 0) {
        if (err) atomicOr(&flags[F_ERR], err);
        flags[F_STORED] = stored, flags[F_FIXED] = fixed, flags[F_DYNAMIC] = dynamic, flags[F_SUBSEQUENCES] = subsequences;
        flags[F_ROUNDS] = most_rounds, flags[F_WINDOWS] = (uint32_t)windows, flags[F_EMITTED] = (uint32_t)n_win, flags[F_RECORDS] = (uint32_t)n_rec;
        values[V_END_BIT] = p;
    }
}

// rec_out: the records' counts, scanned; rec_out[n_rec] = their total
__global__ __launch_bounds__(BLOCK) void png_write_kernel(const uint32_t *__restrict__ words, unsigned long long n_bytes, const unsigned long long *__restrict__ win,
                                                          const unsigned long long *__restrict__ rec_entry, const unsigned long long *__restrict__ rec_out,
                                                          unsigned long long n_rec, uint8_t *__restrict__ raw, uint32_t *__restrict__ src,
                                                          unsigned long long filtered, uint32_t *__restrict__ flags)
{
    __shared__ Tables T;
    __shared__ unsigned long long s_p;
    __shared__ uint32_t s_err;
    const uint32_t tid = threadIdx.x;
    const unsigned long long total_bits = n_bytes * 8;
    const unsigned long long w0 = win[WIN_WORDS * (unsigned long long)blockIdx.x], base = win[WIN_WORDS * (unsigned long long)blockIdx.x + 1];
    const unsigned long long first = win[WIN_WORDS * (unsigned long long)blockIdx.x + 2];
    const unsigned long long header = w0 & ((1ull << 40) - 1ull), emit = w0 >> 44;
    const uint32_t btype = (uint32_t)(w0 >> 40) & 3u;
    if (blockIdx.x == 0 && tid == 0 && rec_out[n_rec] != filtered) atomicOr(&flags[F_ERR], ERR_SIZE); // not height x (1 + row bytes)
    if (btype == 0) {
        if (tid >= emit) return;
        const uint8_t *from = reinterpret_cast<const uint8_t *>(words) + rec_entry[first + tid];
        const unsigned long long o = rec_out[first + tid], n = rec_out[first + tid + 1] - o;
        for (unsigned long long k = 0; k < n && k < PIECE && o + k < filtered; k++) raw[o + k] = from[k], src[o + k] = (uint32_t)(o + k);
        return;
    }
    if (load_tables(words, 0, header + 3, total_bits, btype, T, &s_err, &s_p)) return; // (the chain kernel has accepted the header)
    if (tid >= emit) return;
    const unsigned long long entry = rec_entry[first + tid];
    const unsigned long long end_bit = min(base + (unsigned long long)(tid + 1) * pd::SUBSEQ_BITS, total_bits);
    if (entry == ENDED || entry >= end_bit) return;
    unsigned long long count = 0, eob_after = 0;
    decode_subsequence<true>(words, 0, T, entry, end_bit, count, eob_after, raw, src, rec_out[first + tid], filtered, flags);
}

// out[o] = in[in[o]] where that is another step back (in[o] < o for a copy, = o for a literal; anything else is left alone)
__global__ __launch_bounds__(BLOCK) void png_resolve_kernel(const uint32_t *__restrict__ in, uint32_t *__restrict__ out, unsigned long long n,
                                                            uint32_t *__restrict__ flags)
{
    const unsigned long long o = (unsigned long long)blockIdx.x * BLOCK + threadIdx.x;
    if (o >= n) return;
    uint32_t s = in[o];
    if (s < o) {
        const uint32_t t = in[s];
        if (t < s) s = t, flags[F_CHANGED] = 1u;
    }
    out[o] = s;
}

// raw[o] = its literal; values[V_ADLER_A] += sum d[o], values[V_ADLER_B] += sum ((n - o) mod 65521) d[o] (png_common.hpp: AdlerSums)
__global__ __launch_bounds__(BLOCK) void png_gather_kernel(uint8_t *__restrict__ raw, const uint32_t *__restrict__ src, unsigned long long n,
                                                           unsigned long long *__restrict__ values)
{
    const unsigned long long o = (unsigned long long)blockIdx.x * BLOCK + threadIdx.x;
    unsigned long long a = 0, b = 0;
    if (o < n) {
        const uint32_t s = src[o];
        const uint8_t d = raw[s < o ? s : o]; // (a literal's position holds its own byte: reading it while its lane rewrites it is harmless)
        if (s < o) raw[o] = d;
        a = d, b = ((n - o) % pc::ADLER_MOD) * d;
    }
    for (int step = WAVE / 2; step; step >>= 1) a += __shfl_down(a, step), b += __shfl_down(b, step);
    if ((threadIdx.x & (WAVE - 1u)) == 0 && (a | b)) atomicAdd(&values[V_ADLER_A], a), atomicAdd(&values[V_ADLER_B], b);
}

__global__ void png_finish_kernel(const uint8_t *__restrict__ stream, unsigned long long n, const unsigned long long *__restrict__ values,
                                  uint32_t *__restrict__ flags)
{
    const unsigned long long at = (values[V_END_BIT] + 7) / 8; // (the chain kernel has checked that four bytes follow)
    const uint32_t want = (uint32_t)stream[at] << 24 | (uint32_t)stream[at + 1] << 16 | (uint32_t)stream[at + 2] << 8 | stream[at + 3];
    const pc::AdlerSums sums = {(uint32_t)(values[V_ADLER_A] % pc::ADLER_MOD), (uint32_t)(values[V_ADLER_B] % pc::ADLER_MOD)};
    if (pc::adler_value(sums, n) != want) atomicOr(&flags[F_ERR], ERR_ADLER);
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
    // ---- the one upload: the palette, the IDAT table, the IDAT payloads end to end
    const size_t table_at = sizeof(h.palette), stream_at = table_at + (size_t)n_idat * sizeof(IdatEntry);
    std::vector<uint8_t> blob(stream_at + (size_t)n);
    std::memcpy(blob.data(), h.palette, sizeof(h.palette));
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
    const size_t at_blob = carve.reserve(blob.size() + pad), at_status = carve.reserve(sizeof(Status)), at_win = carve.reserve((size_t)max_windows * WIN_WORDS * 8);
    const size_t at_entry = carve.reserve((size_t)max_records * 8), at_count = carve.reserve(((size_t)max_records + 1) * 8);
    const size_t at_raw = carve.reserve((size_t)P.filtered), at_src = carve.reserve((size_t)P.filtered * 4 * 2);
    uint8_t *arena = nullptr, *d_out = nullptr;
    hipError_t e = sc.alloc(&arena, carve.total);
    if (e == hipSuccess) e = sc.output(out, (size_t)bytes, &d_out);
    if (e != hipSuccess) return device_error(name_, e);
    uint8_t *d_blob = arena + at_blob, *raw = arena + at_raw;
    Status *status = reinterpret_cast<Status *>(arena + at_status), h_status{};
    uint32_t *flags = status->flags, *srcs[2] = {reinterpret_cast<uint32_t *>(arena + at_src), reinterpret_cast<uint32_t *>(arena + at_src) + P.filtered};
    unsigned long long *values = status->values, *win = reinterpret_cast<unsigned long long *>(arena + at_win);
    unsigned long long *rec_entry = reinterpret_cast<unsigned long long *>(arena + at_entry), *rec_count = reinterpret_cast<unsigned long long *>(arena + at_count);
    const uint8_t *d_palette = d_blob, *d_stream = d_blob + stream_at;
    const IdatEntry *d_table = reinterpret_cast<const IdatEntry *>(d_blob + table_at);
    const uint32_t *words = reinterpret_cast<const uint32_t *>(d_stream); // (stream_at is a multiple of 16)
    e = hipMemcpyAsync(d_blob, blob.data(), blob.size(), hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipMemsetAsync(d_blob + blob.size(), 0, pad, s);
    if (e == hipSuccess) e = hipMemsetAsync(status, 0, sizeof(Status), s);
    if (e != hipSuccess) return device_error(name_, e);
    auto read_status = [&]() {
        hipError_t r = hipGetLastError();
        if (r == hipSuccess) r = hipMemcpyAsync(&h_status, status, sizeof(Status), hipMemcpyDeviceToHost, s);
        if (r == hipSuccess) r = hipStreamSynchronize(s);
        return r;
    };
    const dim3 block(BLOCK);
    const uint8_t idat_name[4] = {'I', 'D', 'A', 'T'};
    hipLaunchKernelGGL(png_crc_kernel, dim3((uint32_t)n_idat), block, 0, s, d_stream, d_table, pc::crc32(idat_name, 4), flags);
    hipLaunchKernelGGL(png_chain_kernel, dim3(1), block, 0, s, words, n, win, max_windows, rec_entry, rec_count, max_records, flags, values);
    if ((e = read_status()) != hipSuccess) return device_error(name_, e);
    auto keep_stats = [&](uint64_t copy_rounds) {
        const uint32_t *f = h_status.flags;
        stats[0] = f[F_STORED], stats[1] = f[F_FIXED], stats[2] = f[F_DYNAMIC], stats[3] = f[F_SUBSEQUENCES], stats[4] = f[F_ROUNDS];
        stats[5] = f[F_WINDOWS], stats[6] = copy_rounds, stats[7] = f[F_SEGMENTS];
        if (adam7) stats[8] = h.passes, stats[9] = 0;
    };
    keep_stats(0);
    if (h_status.flags[F_ERR]) return file_error(name, h_status.flags[F_ERR], laced);
    const unsigned long long n_win = h_status.flags[F_EMITTED], n_rec = h_status.flags[F_RECORDS];
    if (n_win == 0) return file_error(name, ERR_SIZE, laced); // no output at all
    launch_scan_u64(rec_count, n_rec, rec_count + n_rec, s);
    hipLaunchKernelGGL(png_write_kernel, dim3((uint32_t)n_win), block, 0, s, words, n, win, rec_entry, rec_count, n_rec, raw, srcs[0], P.filtered, flags);
    // ---- the copies: pointer doubling, a launch and one flag back per round (a chain of 2^31 copies takes 31 rounds and the one that changes nothing)
    const dim3 byte_grid((uint32_t)((P.filtered + BLOCK - 1) / BLOCK));
    uint32_t rounds = 0, from = 0;
    for (;; from ^= 1u) {
        if (rounds > 33) return fail(CVHIP_ERR_DEVICE, name + ": the copies did not resolve");
        e = hipMemsetAsync(flags + F_CHANGED, 0, sizeof(uint32_t), s);
        if (e != hipSuccess) return device_error(name_, e);
        hipLaunchKernelGGL(png_resolve_kernel, byte_grid, block, 0, s, srcs[from], srcs[from ^ 1u], P.filtered, flags);
        rounds++;
        if ((e = read_status()) != hipSuccess) return device_error(name_, e);
        if (h_status.flags[F_ERR] || !h_status.flags[F_CHANGED]) break;
    }
    keep_stats(rounds);
    if (h_status.flags[F_ERR]) return file_error(name, h_status.flags[F_ERR], laced);
    hipLaunchKernelGGL(png_gather_kernel, byte_grid, block, 0, s, raw, srcs[from ^ 1u], P.filtered, values);
    hipLaunchKernelGGL(png_finish_kernel, dim3(1), dim3(1), 0, s, d_stream, P.filtered, values, flags);
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
    if ((e = read_status()) != hipSuccess) return device_error(name_, e);
    keep_stats(rounds);
    if (h_status.flags[F_ERR]) return file_error(name, h_status.flags[F_ERR], laced);
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
