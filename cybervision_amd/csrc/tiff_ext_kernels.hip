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
//   tiffx_chain_kernel    a workgroup per zlib stream walks its chain of deflate blocks as png_chain_kernel walks the one PNG
//                         stream (inflate_device.inc): the header by one lane, the tables in LDS, the self-synchronising decode
//                         over subsequences of SUBSEQ_BITS bits in settle windows of 256.  A settled window's records get their
//                         output positions at once, by a scan over the workgroup that carries the stream's running count, so the
//                         positions restart at every stream; windows and records take the next free slots of two arrays shared
//                         by all streams, whose sizes are the sums of the PNG path's bounds for each stream
//   tiffx_write_kernel    a workgroup per window of any stream: the block's tables again, one more decode from the settled
//                         states: literals, and per output byte its source index inside the stream (itself for a literal)
//   tiffx_resolve_kernel  pointer doubling over the source indices, inside each stream, until a launch changes nothing
//   tiffx_gather_kernel   every byte from its literal; the Adler-32 sums of every stream
//   tiffx_finish_kernel   a lane per stream: the Adler-32 behind its final block against those sums
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
}
using namespace inflate;

constexpr uint32_t WIN_SLOTS = 4; // a window: png_chain_kernel's three words, and its stream

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

// stream s decompresses to this many bytes
__device__ __forceinline__ uint32_t stream_need(const ExtParams &X, uint32_t s)
{
    return (uint32_t)min((unsigned long long)X.stream_bytes, X.total - (unsigned long long)s * X.stream_bytes);
}

// ---- the chains of blocks: png_chain_kernel for stream blockIdx.x -------------------------------------------------------------------
__global__ __launch_bounds__(BLOCK) void tiffx_chain_kernel(const uint8_t *__restrict__ file, const uint32_t *__restrict__ offsets,
                                                            const uint32_t *__restrict__ counts, ExtParams X, unsigned long long *__restrict__ win,
                                                            unsigned long long max_windows, unsigned long long *__restrict__ rec_entry,
                                                            unsigned long long *__restrict__ rec_out, uint32_t *__restrict__ rec_count,
                                                            unsigned long long max_records, uint32_t *__restrict__ flags,
                                                            unsigned long long *__restrict__ end_bit)
{
    __shared__ Tables T;
    __shared__ uint32_t s_stream[WINDOW_WORDS];
    __shared__ unsigned long long s_exit[BLOCK], s_p, s_eob, s_wave[BLOCK / WAVE], s_slot[2];
    __shared__ uint32_t s_err, s_btype, s_final, s_first, s_len;
    const uint32_t tid = threadIdx.x, lane = tid % WAVE, wave = tid / WAVE, stream = blockIdx.x;
    const uint32_t *words = reinterpret_cast<const uint32_t *>(file + offsets[stream]); // (the host lays every stream at a multiple of 4, 32 zero bytes behind it)
    const unsigned long long n_bytes = counts[stream], total_bits = n_bytes * 8, need = stream_need(X, stream);
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
    uint32_t err = s_err, stored = 0, fixed = 0, dynamic = 0, most_rounds = 0, subsequences = 0, windows = 0;
    unsigned long long p = 16, out_pos = 0; // out_pos: the stream's output in front of the next record
    bool final_seen = false;
    // the next `records` records and the next window of the shared arrays -> s_slot, or ERR_ROOM
    auto take = [&](unsigned long long records) -> bool {
        __syncthreads();
        if (tid == 0) s_slot[0] = atomicAdd(&flags[F_EMITTED], 1u), s_slot[1] = atomicAdd(&flags[F_RECORDS], (uint32_t)records);
        __syncthreads();
        return s_slot[0] + 1 <= max_windows && s_slot[1] + records <= max_records;
    };
    for (unsigned long long blocks = 0; !err && !final_seen && blocks <= total_bits; blocks++) {
        const unsigned long long header = p;
        __syncthreads();
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
                if (!take(pieces)) {
                    err = ERR_ROOM;
                    break;
                }
                const unsigned long long w = s_slot[0], r = s_slot[1];
                if (tid < pieces) {
                    const unsigned long long at = done + (unsigned long long)tid * PIECE;
                    rec_entry[r + tid] = first_byte + at, rec_out[r + tid] = out_pos + at, rec_count[r + tid] = (uint32_t)min((unsigned long long)PIECE, length - at);
                }
                if (tid == 0) win[WIN_SLOTS * w] = header | pieces << 44, win[WIN_SLOTS * w + 1] = 0, win[WIN_SLOTS * w + 2] = r, win[WIN_SLOTS * w + 3] = stream;
                windows++;
            }
            out_pos += length;
            p = s_p + 8 * length;
            continue;
        }
        if (btype == 1) fixed++;
        else dynamic++;
        const unsigned long long header_word = p >> 5;
        for (uint32_t k = tid; k < HEADER_WORDS; k += BLOCK) s_stream[k] = header_word + k < (n_bytes + 32) / 4 ? words[header_word + k] : 0u;
        __syncthreads();
        err = load_tables(s_stream, header_word, p + 3, total_bits, btype, T, &s_err, &s_p);
        if (err) break;
        unsigned long long base = s_p, entry0 = s_p;
        bool block_done = false;
        while (!err && !block_done) { // a window of BLOCK subsequences
            if (base >= total_bits) {
                err = ERR_END;
                break;
            }
            windows++;
            const unsigned long long first_bit = base + (unsigned long long)tid * pd::SUBSEQ_BITS;
            const bool active = first_bit < total_bits;
            const unsigned long long end_bit_here = min(first_bit + pd::SUBSEQ_BITS, total_bits);
            const unsigned long long n_active = min((unsigned long long)BLOCK, (total_bits - base + pd::SUBSEQ_BITS - 1) / pd::SUBSEQ_BITS);
            const unsigned long long word_base = base >> 5, stream_words = (n_bytes + 32) / 4;
#pragma unroll 8
            for (uint32_t k = tid; k < WINDOW_WORDS; k += BLOCK) s_stream[k] = word_base + k < stream_words ? words[word_base + k] : 0u;
            __syncthreads();
            unsigned long long cur_entry = tid == 0 ? entry0 : first_bit, cur_exit = ENDED, count = 0, eob_after = 0;
            if (active)
                cur_exit = cur_entry >= end_bit_here
                               ? cur_entry
                               : decode_subsequence<false>(s_stream, word_base, T, cur_entry, end_bit_here, count, eob_after, nullptr, nullptr, 0, 0, nullptr);
            s_exit[tid] = cur_exit;
            if (tid == 0) s_first = BLOCK;
            uint32_t rounds = 0;
            for (uint32_t r = 0; r <= BLOCK; r++) { // lane k holds its true state after k rounds
                __syncthreads();
                unsigned long long want = (tid && active) ? s_exit[tid - 1] : cur_entry;
                if (want == ENDED) want = cur_entry; // (png_chain_kernel says why)
                const bool change = want != cur_entry;
                if (!__syncthreads_or(change)) break;
                if (change) {
                    cur_entry = want, count = 0, eob_after = 0;
                    cur_exit = cur_entry >= end_bit_here
                                   ? cur_entry
                                   : decode_subsequence<false>(s_stream, word_base, T, cur_entry, end_bit_here, count, eob_after, nullptr, nullptr, 0, 0, nullptr);
                    s_exit[tid] = cur_exit;
                }
                rounds++;
            }
            most_rounds = max(most_rounds, rounds);
            const bool ends_here = active && cur_exit == ENDED;
            if (ends_here) atomicMin(&s_first, tid);
            __syncthreads();
            const uint32_t jend = s_first;
            const unsigned long long emit = jend < BLOCK ? jend + 1 : n_active;
            subsequences += (uint32_t)emit;
            if (__syncthreads_or(tid < emit && count != 0)) { // (a window without output needs no write pass)
                // the records' output positions: the counts scanned over the workgroup, behind the stream's count so far
                const unsigned long long mine = tid < emit ? count : 0ull;
                unsigned long long incl = mine;
#pragma unroll
                for (uint32_t d = 1; d < WAVE; d <<= 1) {
                    const unsigned long long t = __shfl_up(incl, d);
                    if (lane >= d) incl += t;
                }
                if (lane == WAVE - 1) s_wave[wave] = incl;
                __syncthreads();
                unsigned long long before = 0, all = 0;
#pragma unroll
                for (uint32_t k = 0; k < BLOCK / WAVE; k++) {
                    if (k < wave) before += s_wave[k];
                    all += s_wave[k];
                }
                if (!take(emit)) {
                    err = ERR_ROOM;
                    break;
                }
                const unsigned long long w = s_slot[0], r = s_slot[1];
                if (tid < emit) rec_entry[r + tid] = cur_entry, rec_out[r + tid] = out_pos + before + incl - mine, rec_count[r + tid] = 0;
                if (tid == 0)
                    win[WIN_SLOTS * w] = header | (unsigned long long)btype << 40 | emit << 44, win[WIN_SLOTS * w + 1] = base, win[WIN_SLOTS * w + 2] = r,
                                    win[WIN_SLOTS * w + 3] = stream;
                out_pos += all;
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
    if (!err && out_pos != need) err = ERR_SIZE;          // not the strip's or tile's bytes: fewer, or more
    if (tid == 0) {
        if (err) atomicOr(&flags[F_ERR], err);
        atomicAdd(&flags[F_STORED], stored), atomicAdd(&flags[F_FIXED], fixed), atomicAdd(&flags[F_DYNAMIC], dynamic);
        atomicAdd(&flags[F_SUBSEQUENCES], subsequences), atomicAdd(&flags[F_WINDOWS], windows), atomicMax(&flags[F_ROUNDS], most_rounds);
        end_bit[stream] = p;
    }
}

// a workgroup per window: png_write_kernel on the window's stream, positions and source indices inside the stream
__global__ __launch_bounds__(BLOCK) void tiffx_write_kernel(const uint8_t *__restrict__ file, const uint32_t *__restrict__ offsets,
                                                            const uint32_t *__restrict__ counts, ExtParams X, const unsigned long long *__restrict__ win,
                                                            const unsigned long long *__restrict__ rec_entry, const unsigned long long *__restrict__ rec_out,
                                                            const uint32_t *__restrict__ rec_count, uint8_t *__restrict__ raw, uint32_t *__restrict__ src,
                                                            uint32_t *__restrict__ flags)
{
    __shared__ Tables T;
    __shared__ unsigned long long s_p;
    __shared__ uint32_t s_err;
    const uint32_t tid = threadIdx.x;
    const unsigned long long *my = win + WIN_SLOTS * (unsigned long long)blockIdx.x;
    const unsigned long long w0 = my[0], base = my[1], first = my[2];
    const uint32_t stream = (uint32_t)my[3];
    const unsigned long long header = w0 & ((1ull << 40) - 1ull), emit = w0 >> 44;
    const uint32_t btype = (uint32_t)(w0 >> 40) & 3u;
    const uint32_t *words = reinterpret_cast<const uint32_t *>(file + offsets[stream]);
    const unsigned long long total_bits = 8ull * counts[stream], need = stream_need(X, stream), at = (unsigned long long)stream * X.stream_bytes;
    raw += at, src += at;
    if (btype == 0) {
        if (tid >= emit) return;
        const uint8_t *from = reinterpret_cast<const uint8_t *>(words) + rec_entry[first + tid];
        const unsigned long long o = rec_out[first + tid], n = rec_count[first + tid];
        for (unsigned long long k = 0; k < n && k < PIECE && o + k < need; k++) raw[o + k] = from[k], src[o + k] = (uint32_t)(o + k);
        return;
    }
    if (load_tables(words, 0, header + 3, total_bits, btype, T, &s_err, &s_p)) return; // (the chain kernel has accepted the header)
    if (tid >= emit) return;
    const unsigned long long entry = rec_entry[first + tid];
    const unsigned long long end_bit_here = min(base + (unsigned long long)(tid + 1) * pd::SUBSEQ_BITS, total_bits);
    if (entry == ENDED || entry >= end_bit_here) return;
    unsigned long long count = 0, eob_after = 0;
    decode_subsequence<true>(words, 0, T, entry, end_bit_here, count, eob_after, raw, src, rec_out[first + tid], need, flags);
}

// png_resolve_kernel inside each stream: byte g of all streams is byte o = g - base of its own
__global__ __launch_bounds__(BLOCK) void tiffx_resolve_kernel(const uint32_t *__restrict__ in, uint32_t *__restrict__ out, ExtParams X, uint32_t *__restrict__ flags)
{
    const unsigned long long g = (unsigned long long)blockIdx.x * BLOCK + threadIdx.x;
    if (g >= X.total) return;
    const unsigned long long base = g / X.stream_bytes * X.stream_bytes;
    const uint32_t o = (uint32_t)(g - base);
    uint32_t s = in[g];
    if (s < o) {
        const uint32_t t = in[base + s];
        if (t < s) s = t, flags[F_CHANGED] = 1u;
    }
    out[g] = s;
}

// raw[g] = its literal; sums[2 s], sums[2 s + 1] += the Adler-32 sums of stream s (png_gather_kernel's)
__global__ __launch_bounds__(BLOCK) void tiffx_gather_kernel(uint8_t *__restrict__ raw, const uint32_t *__restrict__ src, ExtParams X,
                                                             unsigned long long *__restrict__ sums)
{
    const unsigned long long g = (unsigned long long)blockIdx.x * BLOCK + threadIdx.x;
    const bool inside = g < X.total;
    const uint32_t stream = (uint32_t)((inside ? g : X.total - 1) / X.stream_bytes);
    unsigned long long a = 0, b = 0;
    if (inside) {
        const unsigned long long base = (unsigned long long)stream * X.stream_bytes;
        const uint32_t o = (uint32_t)(g - base), s = src[g];
        const uint8_t d = raw[base + (s < o ? s : o)]; // (a literal's position holds its own byte)
        if (s < o) raw[g] = d;
        a = d, b = (unsigned long long)((stream_need(X, stream) - o) % pc::ADLER_MOD) * d;
    }
    // a wave inside one stream adds its sums up first; one that spans a stream's end adds lane by lane
    const uint32_t first = __shfl(stream, 0);
    if (__all(stream == first)) {
        for (int step = WAVE / 2; step; step >>= 1) a += __shfl_down(a, step), b += __shfl_down(b, step);
        if ((threadIdx.x & (WAVE - 1u)) != 0) return;
    }
    if (a | b) atomicAdd(&sums[2ull * stream], a), atomicAdd(&sums[2ull * stream + 1], b);
}

__global__ __launch_bounds__(BLOCK) void tiffx_finish_kernel(const uint8_t *__restrict__ file, const uint32_t *__restrict__ offsets, uint32_t streams, ExtParams X,
                                                             const unsigned long long *__restrict__ end_bit, const unsigned long long *__restrict__ sums,
                                                             uint32_t *__restrict__ flags)
{
    const uint32_t s = blockIdx.x * BLOCK + threadIdx.x;
    if (s >= streams) return;
    const uint8_t *stream = file + offsets[s];
    const unsigned long long at = (end_bit[s] + 7) / 8; // (the chain kernel has checked that four bytes follow)
    const uint32_t want = (uint32_t)stream[at] << 24 | (uint32_t)stream[at + 1] << 16 | (uint32_t)stream[at + 2] << 8 | stream[at + 3];
    const pc::AdlerSums whole = {(uint32_t)(sums[2ull * s] % pc::ADLER_MOD), (uint32_t)(sums[2ull * s + 1] % pc::ADLER_MOD)};
    if (pc::adler_value(whole, stream_need(X, s)) != want) atomicOr(&flags[F_ERR], ERR_ADLER);
}

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
        unsigned long long *win = reinterpret_cast<unsigned long long *>(arena + at_win), *rec_entry = reinterpret_cast<unsigned long long *>(arena + at_entry);
        unsigned long long *rec_out = reinterpret_cast<unsigned long long *>(arena + at_out), *end_bit = reinterpret_cast<unsigned long long *>(arena + at_streams);
        unsigned long long *sums = end_bit + streams;
        uint32_t *rec_count = reinterpret_cast<uint32_t *>(arena + at_count);
        uint32_t *srcs[2] = {reinterpret_cast<uint32_t *>(arena + at_src), reinterpret_cast<uint32_t *>(arena + at_src) + X.total};
        hipLaunchKernelGGL(tiffx_chain_kernel, dim3(streams), block, 0, s, d_file, d_offsets, d_counts, X, win, max_windows, rec_entry, rec_out, rec_count,
                           max_records, flags, end_bit);
        if ((e = read_status()) != hipSuccess) return device_error("tiff_ext_decode", e);
        keep_stats(0);
        if (h_status.flags[F_ERR]) return file_error(h_status.flags[F_ERR]);
        const uint32_t n_win = h_status.flags[F_EMITTED];
        if (n_win == 0) return file_error(ERR_SIZE); // no output at all
        hipLaunchKernelGGL(tiffx_write_kernel, dim3(n_win), block, 0, s, d_file, d_offsets, d_counts, X, win, rec_entry, rec_out, rec_count, raw, srcs[0], flags);
        // ---- the copies: pointer doubling, a launch and one flag back per round
        const dim3 byte_grid((uint32_t)((X.total + BLOCK - 1) / BLOCK));
        uint32_t from = 0;
        for (;; from ^= 1u) {
            if (rounds > 33) return fail(CVHIP_ERR_DEVICE, "tiff_ext_decode: the copies did not resolve");
            e = hipMemsetAsync(flags + F_CHANGED, 0, sizeof(uint32_t), s);
            if (e != hipSuccess) return device_error("tiff_ext_decode", e);
            hipLaunchKernelGGL(tiffx_resolve_kernel, byte_grid, block, 0, s, srcs[from], srcs[from ^ 1u], X, flags);
            rounds++;
            if ((e = read_status()) != hipSuccess) return device_error("tiff_ext_decode", e);
            if (h_status.flags[F_ERR] || !h_status.flags[F_CHANGED]) break;
        }
        keep_stats(rounds);
        if (h_status.flags[F_ERR]) return file_error(h_status.flags[F_ERR]);
        hipLaunchKernelGGL(tiffx_gather_kernel, byte_grid, block, 0, s, raw, srcs[from ^ 1u], X, sums);
        hipLaunchKernelGGL(tiffx_finish_kernel, dim3((streams + BLOCK - 1) / BLOCK), block, 0, s, d_file, d_offsets, streams, X, end_bit, sums, flags);
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
