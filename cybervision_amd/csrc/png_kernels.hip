// png_kernels.hip — cvhip_png_encode: the PNG file image of an 8-bit image with 1 to 4 channels, made on the device
// (DESIGN.md 4.15).  The reference saves its textures and its depth map with img.save (src/output.rs:845-875, 1141); byte
// parity with that encoder is not the aim - the file is defined here (tests/ref_png.py restates it): one IDAT, one dynamic
// Huffman block, tokens made per row from repeats of the previous byte only (literals and matches at distance 1), so
// that every row is independent of the others once the code is known.
//
// A wave per row, a lane per byte, 64 bytes a step:
//   png_filter_kernel     the row's filter (given, or the one of least sum of |signed byte|), the filtered bytes to scratch,
//                         the row's Adler sums
//   png_histogram_kernel  the row's tokens counted in LDS, flushed by global atomic adds -> the 286 counters, to the HOST:
//                         code lengths (package-merge), codes, the block's header bits and the token table come back
//                         (png_common.hpp) - the one round trip besides the size
//   png_length_kernel     the bits of every row under the table; a 64-bit scan (launch_scan_u64) places the rows
//   png_write_kernel      the tokens again, each lane's bits placed by a wave scan and OR-ed into a staging window in LDS; whole
//                         dwords leave by plain stores, the dword a row shares with its neighbour at either end by atomicOr
//                         into the zeroed body - the result does not depend on the order of the rows
//   png_trailer_kernel    the header's last partial byte, the end-of-block code, the Adler-32 from the rows' sums
//   png_crc_kernel        the IDAT chunk's CRC-32 from the CRCs of its pieces, each multiplied by x^(8 * bytes behind it)
//   png_finish_kernel     the CRC's bytes and IEND
#include <cstring>

#include "cvhip_internal.hpp"

#include "png_common.hpp"

namespace cvhip {
namespace {

namespace pc = png_common;

constexpr int WAVE = 64;
constexpr uint32_t TOKEN_NONE = 0xFFFFFFFFu;
constexpr uint32_t LOOK_BYTES = 5;                                         // bytes a lane compares past the window: 64 * 5 >= 257
constexpr uint32_t STAGE_WORDS = (31 + WAVE * pc::TOKEN_BITS_MAX) / 32 + 2; // a window's bits behind a partial dword, and one more
constexpr uint32_t CRC_PIECE = 256;                                        // bytes of the IDAT chunk per lane of png_crc_kernel
constexpr uint32_t PREFIX_BYTES = 8 + 25 + 8;                              // signature, IHDR chunk, IDAT length and type

__device__ __forceinline__ unsigned long long wave_sum(unsigned long long v)
{
#pragma unroll
    for (int s = 32; s; s >>= 1) v += __shfl_xor(v, s, WAVE);
    return v;
}

// the byte x under filter f with a = left, b = up, c = up-left (PNG specification 9.2)
__device__ __forceinline__ uint32_t filter_byte(uint32_t f, uint32_t x, uint32_t a, uint32_t b, uint32_t c)
{
    uint32_t pred = 0;
    if (f == 1) pred = a;
    else if (f == 2) pred = b;
    else if (f == 3) pred = (a + b) >> 1;
    else if (f == 4) {
        const int p = (int)a + (int)b - (int)c;
        const int pa = abs(p - (int)a), pb = abs(p - (int)b), pcc = abs(p - (int)c);
        pred = (pa <= pb && pa <= pcc) ? a : (pb <= pcc) ? b : c;
    }
    return (x - pred) & 0xFFu;
}

// rows: row_bytes pixels bytes each; filtered: 1 + row_bytes each, the filter's number first.  sums[row] = the Adler sums of
// the row's 1 + row_bytes bytes (png_common.hpp: a = sum d[i], b = sum (n - i) d[i], mod 65521).
__global__ __launch_bounds__(WAVE) void png_filter_kernel(const uint8_t *__restrict__ pixels, unsigned long long row_bytes, uint32_t height,
                                                          uint32_t bpp, uint32_t filter, uint8_t *__restrict__ filtered,
                                                          uint2 *__restrict__ sums)
{
    const uint32_t lane = threadIdx.x;
    const unsigned long long n = row_bytes + 1;
    for (uint32_t row = blockIdx.x; row < height; row += gridDim.x) {
        const bool top = row == 0;
        const uint8_t *cur = pixels + (unsigned long long)row * row_bytes, *up = top ? cur : cur - row_bytes;
        uint32_t f = filter;
        if (filter == CVHIP_PNG_FILTER_ADAPTIVE) {
            unsigned long long score[5] = {0, 0, 0, 0, 0};
            for (unsigned long long i = lane; i < row_bytes; i += WAVE) {
                const uint32_t x = cur[i], a = i >= bpp ? cur[i - bpp] : 0u, b = top ? 0u : up[i], c = (top || i < bpp) ? 0u : up[i - bpp];
#pragma unroll
                for (uint32_t k = 0; k < 5; k++) {
                    const uint32_t v = filter_byte(k, x, a, b, c);
                    score[k] += v < 128 ? v : 256 - v;
                }
            }
            unsigned long long best = 0;
            f = 0;
#pragma unroll
            for (uint32_t k = 0; k < 5; k++) {
                const unsigned long long total = wave_sum(score[k]);
                if (k == 0 || total < best) best = total, f = k; // (equal scores: the lowest number stays)
            }
        }
        uint8_t *dst = filtered + (unsigned long long)row * n;
        unsigned long long sa = 0, sb = 0;
        if (lane == 0) {
            dst[0] = (uint8_t)f;
            sa = f, sb = (n % pc::ADLER_MOD) * f;
        }
        for (unsigned long long i = lane; i < row_bytes; i += WAVE) {
            const uint32_t x = cur[i], a = i >= bpp ? cur[i - bpp] : 0u, b = top ? 0u : up[i], c = (top || i < bpp) ? 0u : up[i - bpp];
            const uint32_t v = filter_byte(f, x, a, b, c);
            dst[1 + i] = (uint8_t)v;
            sa += v;
            sb += ((n - 1 - i) % pc::ADLER_MOD) * v; // (< 2^24 a term, < 2^26 terms a lane)
        }
        sa = wave_sum(sa), sb = wave_sum(sb % pc::ADLER_MOD);
        if (lane == 0) sums[row] = make_uint2((uint32_t)(sa % pc::ADLER_MOD), (uint32_t)(sb % pc::ADLER_MOD));
    }
}

// The tokens of the row b[0 .. n), 64 positions a step: emit(token) is called by all lanes of the wave once per step with the
// token that BEGINS at the lane's position - a literal 0..255, TOKEN_MATCH + (length - 3), or TOKEN_NONE (a position inside
// a match, or past the row).  Position i >= 1 repeats iff b[i] == b[i - 1]; a maximal run of repeating positions is cut
// into matches of 258 from its start, the rest of 3 or more is one match, a rest of 1 or 2 is literals.  So a position
// needs its offset in its run (the last position before it that does not repeat: a ballot, and a carry between the steps)
// and at most 257 positions of the run ahead of it (the step's ballot, and LOOK_BYTES bytes a lane past the step when a
// run reaches its end).
template <typename Emit>
__device__ __forceinline__ void row_tokens(const uint8_t *__restrict__ b, unsigned long long n, uint32_t lane, Emit &&emit)
{
    unsigned long long last_plain = 0; // the last position before the step that does not repeat (position 0 is one)
    uint32_t last_byte = 0x100;        // the byte before the step
    for (unsigned long long base = 0; base < n; base += WAVE) {
        const unsigned long long i = base + lane;
        const bool valid = i < n;
        const uint32_t cur = valid ? b[i] : 0x100u; // (no byte: never equal to one)
        uint32_t prev = __shfl_up(cur, 1, WAVE);
        if (lane == 0) prev = last_byte;
        const bool rep = valid && cur == prev;
        const unsigned long long mask = __ballot(rep), plain = ~mask;
        const unsigned long long below = plain & ((1ull << lane) - 1ull);
        const unsigned long long before = below ? base + (63u - (uint32_t)__builtin_clzll(below)) : last_plain;
        const uint32_t in_chunk = (uint32_t)((i - before - 1) % 258u); // (of a repeating position)
        const unsigned long long above = (mask >> lane) >> 1;
        const uint32_t ahead_here = (uint32_t)__builtin_ctzll(~above); // repeating positions straight after this one, in the step
        const bool reaches = rep && lane + ahead_here == 63u;
        uint32_t past = 0; // positions past the step that continue the run at its end
        if (__ballot(reaches && in_chunk <= 1 && base + WAVE < n)) {
            const uint32_t run_byte = __shfl(cur, 63, WAVE);
            const unsigned long long q = base + WAVE + (unsigned long long)lane * LOOK_BYTES;
            uint32_t same = 0;
#pragma unroll
            for (uint32_t k = 0; k < LOOK_BYTES; k++)
                if (same == k && q + k < n && b[q + k] == run_byte) same++;
            const unsigned long long broken = ~__ballot(same == LOOK_BYTES);
            const uint32_t first = broken ? (uint32_t)__builtin_ctzll(broken) : 0u;
            past = broken ? first * LOOK_BYTES + (uint32_t)__shfl((int)same, (int)first, WAVE) : WAVE * LOOK_BYTES;
        }
        const uint32_t ahead = ahead_here + (reaches ? past : 0u);
        uint32_t token = TOKEN_NONE;
        if (valid) {
            if (!rep) token = cur;
            else if (in_chunk == 0) {
                const uint32_t length = ahead + 1 < 258u ? ahead + 1 : 258u;
                token = length >= 3 ? pc::TOKEN_MATCH + length - 3 : cur;
            } else if (in_chunk == 1 && ahead == 0)
                token = cur; // the second of a rest of two
        }
        emit(token);
        const unsigned long long plain_here = plain & __ballot(valid);
        if (plain_here) last_plain = base + (63u - (uint32_t)__builtin_clzll(plain_here));
        last_byte = __shfl(cur, 63, WAVE);
    }
}

__global__ __launch_bounds__(WAVE) void png_histogram_kernel(const uint8_t *__restrict__ filtered, unsigned long long n, uint32_t height,
                                                             uint32_t *__restrict__ histogram)
{
    __shared__ uint32_t s_hist[pc::LITLEN_SYMBOLS];
    const uint32_t lane = threadIdx.x;
    for (uint32_t s = lane; s < pc::LITLEN_SYMBOLS; s += WAVE) s_hist[s] = 0;
    __syncthreads();
    for (uint32_t row = blockIdx.x; row < height; row += gridDim.x)
        row_tokens(filtered + (unsigned long long)row * n, n, lane, [&](uint32_t token) {
            if (token != TOKEN_NONE) atomicAdd(&s_hist[pc::token_symbol(token)], 1u);
        });
    __syncthreads();
    for (uint32_t s = lane; s < pc::LITLEN_SYMBOLS; s += WAVE)
        if (s_hist[s]) atomicAdd(&histogram[s], s_hist[s]);
}

// table: png_common.hpp's BlockCodes::table.  row_bits[row] = the bits of the row's tokens.
__global__ __launch_bounds__(WAVE) void png_length_kernel(const uint8_t *__restrict__ filtered, unsigned long long n, uint32_t height,
                                                          const uint32_t *__restrict__ table, unsigned long long *__restrict__ row_bits)
{
    __shared__ uint32_t s_table[pc::TOKENS];
    const uint32_t lane = threadIdx.x;
    for (uint32_t t = lane; t < pc::TOKENS; t += WAVE) s_table[t] = table[t];
    __syncthreads();
    for (uint32_t row = blockIdx.x; row < height; row += gridDim.x) {
        unsigned long long bits = 0;
        row_tokens(filtered + (unsigned long long)row * n, n, lane, [&](uint32_t token) {
            if (token != TOKEN_NONE) bits += s_table[token] >> 24;
        });
        bits = wave_sum(bits);
        if (lane == 0) row_bits[row] = bits;
    }
}

// Bit k of the deflate stream is bit first_bit + k of `words` (a 4-byte aligned address at or below the stream's first
// byte); row_start[row] = the bits of the rows before it; n_words: the dwords of `words` that lie wholly in the file.  The
// body was zeroed.
__global__ __launch_bounds__(WAVE) void png_write_kernel(const uint8_t *__restrict__ filtered, unsigned long long n, uint32_t height,
                                                         const uint32_t *__restrict__ table, const unsigned long long *__restrict__ row_start,
                                                         unsigned long long first_bit, uint32_t *__restrict__ words,
                                                         unsigned long long n_words)
{
    __shared__ uint32_t s_table[pc::TOKENS];
    __shared__ uint32_t s_stage[STAGE_WORDS]; // s_stage[0] = the dword of the stream at bit `at`, so far
    const uint32_t lane = threadIdx.x;
    for (uint32_t t = lane; t < pc::TOKENS; t += WAVE) s_table[t] = table[t];
    for (uint32_t row = blockIdx.x; row < height; row += gridDim.x) {
        unsigned long long at = first_bit + row_start[row];
        const unsigned long long first_word = at >> 5;
        const bool shared_start = (at & 31u) != 0; // the row's first dword holds bits of what is in front of it
        if (lane < STAGE_WORDS) s_stage[lane] = 0;
        __syncthreads();
        row_tokens(filtered + (unsigned long long)row * n, n, lane, [&](uint32_t token) {
            const uint32_t entry = token != TOKEN_NONE ? s_table[token] : 0u, count = entry >> 24;
            uint32_t incl = count;
#pragma unroll
            for (int s = 1; s < WAVE; s <<= 1) {
                const uint32_t t = __shfl_up(incl, s, WAVE);
                if ((int)lane >= s) incl += t;
            }
            const uint32_t total = __shfl(incl, 63, WAVE), start = (uint32_t)(at & 31u);
            if (count) {
                const uint32_t bit = start + incl - count;
                const unsigned long long v = (unsigned long long)(entry & 0xFFFFFFu) << (bit & 31u);
                atomicOr(&s_stage[bit >> 5], (uint32_t)v);
                if (v >> 32) atomicOr(&s_stage[(bit >> 5) + 1], (uint32_t)(v >> 32));
            }
            __syncthreads();
            const uint32_t done = (start + total) >> 5; // whole dwords (< STAGE_WORDS - 1)
            const uint32_t mine = lane < STAGE_WORDS ? s_stage[lane] : 0u, rest = s_stage[done];
            __syncthreads();
            const unsigned long long word = (at >> 5) + lane;
            if (lane < done && word < n_words) {
                if (shared_start && word == first_word) atomicOr(&words[word], mine);
                else words[word] = mine;
            }
            if (lane < STAGE_WORDS) s_stage[lane] = lane == 0 ? rest : 0u;
            __syncthreads();
            at += total;
        });
        if (lane == 0 && (at & 31u) && (at >> 5) < n_words) atomicOr(&words[at >> 5], s_stage[0]); // shared with what follows
        __syncthreads();
    }
}

__device__ __forceinline__ void or_bits(uint32_t *__restrict__ words, unsigned long long n_words, unsigned long long bit, uint32_t bits)
{
    const unsigned long long v = (unsigned long long)bits << (bit & 31u);
    if ((uint32_t)v && (bit >> 5) < n_words) atomicOr(&words[bit >> 5], (uint32_t)v);
    if ((v >> 32) && (bit >> 5) + 1 < n_words) atomicOr(&words[(bit >> 5) + 1], (uint32_t)(v >> 32));
}

// One block.  The header's last, partial byte (its bits end at header_end_bit), the end-of-block code at eob_bit, the
// Adler-32 of the filtered bytes (sums: per row, n bytes each) big-endian at adler_out, and the seed of the CRC.
__global__ __launch_bounds__(256) void png_trailer_kernel(const uint2 *__restrict__ sums, uint32_t height, unsigned long long n,
                                                          uint32_t *__restrict__ words, unsigned long long n_words,
                                                          unsigned long long header_end_bit, uint32_t header_partial,
                                                          unsigned long long eob_bit, uint32_t eob_entry, uint8_t *__restrict__ adler_out,
                                                          uint32_t *__restrict__ crc, uint32_t crc_seed)
{
    __shared__ unsigned long long s_a[256], s_b[256];
    const unsigned long long n_mod = n % pc::ADLER_MOD;
    unsigned long long a = 0, b = 0;
    for (uint32_t row = threadIdx.x; row < height; row += 256) { // b of the whole = sum of b_row + a_row * (the bytes behind the row)
        const uint2 s = sums[row];
        const unsigned long long behind = ((unsigned long long)(height - 1 - row) % pc::ADLER_MOD) * n_mod % pc::ADLER_MOD;
        a = (a + s.x) % pc::ADLER_MOD;
        b = (b + s.y + behind * s.x) % pc::ADLER_MOD;
    }
    s_a[threadIdx.x] = a, s_b[threadIdx.x] = b;
    __syncthreads();
    if (threadIdx.x != 0) return;
    for (uint32_t k = 1; k < 256; k++) a += s_a[k], b += s_b[k];
    const uint32_t adler = pc::adler_value({(uint32_t)(a % pc::ADLER_MOD), (uint32_t)(b % pc::ADLER_MOD)}, (unsigned long long)height * n);
    for (int k = 0; k < 4; k++) adler_out[k] = (uint8_t)(adler >> (24 - 8 * k));
    if (header_end_bit & 7u) or_bits(words, n_words, header_end_bit & ~7ull, header_partial);
    or_bits(words, n_words, eob_bit, eob_entry & 0xFFFFFFu);
    *crc = crc_seed;
}

// *crc ^= the CRC-32 of every piece of data[0 .. n) times x^(8 * the bytes behind the piece)
__global__ __launch_bounds__(256) void png_crc_kernel(const uint8_t *__restrict__ data, unsigned long long n, unsigned long long pieces,
                                                      uint32_t *__restrict__ crc)
{
    __shared__ uint32_t s_table[256];
    s_table[threadIdx.x] = pc::crc_table_entry(threadIdx.x);
    __syncthreads();
    for (unsigned long long piece = (unsigned long long)blockIdx.x * 256 + threadIdx.x; piece < pieces; piece += (unsigned long long)gridDim.x * 256) {
        const unsigned long long start = piece * CRC_PIECE;
        const uint8_t *p = data + start;
        uint32_t len = (uint32_t)(n - start < CRC_PIECE ? n - start : CRC_PIECE), c = 0xFFFFFFFFu;
        const unsigned long long behind = n - start - len;
        for (; len && (reinterpret_cast<uintptr_t>(p) & 3u); len--) c = s_table[(c ^ *p++) & 0xFFu] ^ (c >> 8);
        for (; len >= 4; len -= 4, p += 4) {
            c ^= *reinterpret_cast<const uint32_t *>(p);
#pragma unroll
            for (int k = 0; k < 4; k++) c = s_table[c & 0xFFu] ^ (c >> 8);
        }
        for (; len; len--) c = s_table[(c ^ *p++) & 0xFFu] ^ (c >> 8);
        atomicXor(crc, pc::crc_multiply(pc::crc_shift(behind), c ^ 0xFFFFFFFFu));
    }
}

// the IDAT chunk's CRC and the IEND chunk, behind the IDAT data
__global__ void png_finish_kernel(const uint32_t *__restrict__ crc, uint8_t *__restrict__ out)
{
    const uint8_t iend[12] = {0, 0, 0, 0, 'I', 'E', 'N', 'D', 0xAE, 0x42, 0x60, 0x82};
    const uint32_t c = *crc;
    for (int k = 0; k < 4; k++) out[k] = (uint8_t)(c >> (24 - 8 * k));
    for (int k = 0; k < 12; k++) out[4 + k] = iend[k];
}

void put_be32(std::vector<uint8_t> &v, uint32_t x)
{
    for (int k = 0; k < 4; k++) v.push_back((uint8_t)(x >> (24 - 8 * k)));
}

} // namespace
} // namespace cvhip

using namespace cvhip;

extern "C" int cvhip_png_encode(cvhip_device *dev, const uint8_t *pixels, uint32_t width, uint32_t height, uint32_t channels, uint32_t filter,
                                uint8_t *out, uint64_t cap, uint64_t *out_size, uint64_t *out_sections)
{
    if (!dev || !pixels || !out_size || (cap && !out)) return fail(CVHIP_ERR_INVALID, "png_encode: null argument");
    if (!width || !height) return fail(CVHIP_ERR_INVALID, "png_encode: an image without pixels");
    if (channels < 1 || channels > 4) return fail(CVHIP_ERR_INVALID, "png_encode: channels is not 1, 2, 3 or 4");
    if (filter > CVHIP_PNG_FILTER_ADAPTIVE) return fail(CVHIP_ERR_INVALID, "png_encode: filter is not 0 to 4 or 5 (adaptive)");
    const unsigned long long row_bytes = (unsigned long long)width * channels, n = row_bytes + 1;
    if (n > 0xFFFFFFFEull / height) return fail(CVHIP_ERR_UNSUPPORTED, "png_encode: 2^32 - 1 or more filtered bytes");
    const unsigned long long filtered_bytes = n * height;
    CVHIP_TRY_HIP(hipSetDevice(dev->d.ordinal));
    hipStream_t s = dev->d.stream;
    CallScratch sc;
    const uint8_t *d_pixels = nullptr;
    uint8_t *filtered = nullptr;
    uint2 *sums = nullptr;
    uint32_t *words32 = nullptr; // the histogram's 286 counters, the table's 513 words, the CRC
    unsigned long long *row_bits = nullptr, body_bits = 0;
    hipError_t e = sc.input(pixels, (size_t)(row_bytes * height), &d_pixels, s);
    if (e == hipSuccess) e = sc.alloc(&filtered, (size_t)filtered_bytes);
    if (e == hipSuccess) e = sc.alloc(&sums, (size_t)height);
    if (e == hipSuccess) e = sc.alloc(&words32, pc::LITLEN_SYMBOLS + pc::TOKENS + 1);
    if (e == hipSuccess) e = sc.alloc(&row_bits, (size_t)height + 1);
    if (e != hipSuccess) return device_error("png_encode", e);
    uint32_t *histogram = words32, *table = words32 + pc::LITLEN_SYMBOLS, *crc = table + pc::TOKENS;
    const dim3 grid(std::min<uint32_t>(height, CVHIP_MESH_GRID_LANES / WAVE)), wave(WAVE);
    e = hipMemsetAsync(histogram, 0, pc::LITLEN_SYMBOLS * sizeof(uint32_t), s);
    if (e != hipSuccess) return device_error("png_encode", e);
    hipLaunchKernelGGL(png_filter_kernel, grid, wave, 0, s, d_pixels, row_bytes, height, channels, filter, filtered, sums);
    hipLaunchKernelGGL(png_histogram_kernel, grid, wave, 0, s, filtered, n, height, histogram);
    // ---- the round trip: the histogram out, the code back
    uint32_t h_histogram[pc::LITLEN_SYMBOLS];
    e = hipGetLastError();
    if (e == hipSuccess) e = hipMemcpyAsync(h_histogram, histogram, sizeof(h_histogram), hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) return device_error("png_encode", e);
    uint64_t counts[pc::LITLEN_SYMBOLS];
    for (uint32_t k = 0; k < pc::LITLEN_SYMBOLS; k++) counts[k] = h_histogram[k];
    counts[pc::EOB] += 1;
    const pc::BlockCodes codes = pc::block_codes(counts);
    e = hipMemcpyAsync(table, codes.table, sizeof(codes.table), hipMemcpyHostToDevice, s);
    if (e != hipSuccess) return device_error("png_encode", e);
    hipLaunchKernelGGL(png_length_kernel, grid, wave, 0, s, filtered, n, height, table, row_bits);
    launch_scan_u64(row_bits, height, row_bits + height, s);
    e = hipGetLastError();
    if (e == hipSuccess) e = hipMemcpyAsync(&body_bits, row_bits + height, sizeof(body_bits), hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) return device_error("png_encode", e);
    const uint32_t eob_entry = codes.table[pc::TOKEN_EOB];
    const uint64_t header_bits = codes.header.nbits, stream_bits = header_bits + body_bits + (eob_entry >> 24);
    const uint64_t stream_bytes = (stream_bits + 7) / 8, idat_bytes = 2 + stream_bytes + 4;
    if (idat_bytes >= (1ull << 31)) return fail(CVHIP_ERR_UNSUPPORTED, "png_encode: an IDAT chunk of 2^31 or more bytes");
    const uint64_t size = PREFIX_BYTES + idat_bytes + 16;
    *out_size = size;
    if (out_sections) out_sections[0] = PREFIX_BYTES, out_sections[1] = idat_bytes, out_sections[2] = 16;
    if (!cap) return CVHIP_OK;
    if (cap < size) return fail(CVHIP_ERR_INVALID, "png_encode: the buffer is smaller than the file image");
    // ---- the write pass: the bytes composed here, the zeroed body, the rows, the trailer
    uint8_t *d_out = nullptr;
    e = sc.output(out, (size_t)size, &d_out);
    if (e != hipSuccess) return device_error("png_encode", e);
    static const uint8_t colour_type[5] = {0, 0, 4, 2, 6};
    std::vector<uint8_t> prefix = {0x89, 'P', 'N', 'G', 0x0D, 0x0A, 0x1A, 0x0A};
    put_be32(prefix, 13);
    const size_t ihdr = prefix.size();
    prefix.insert(prefix.end(), {'I', 'H', 'D', 'R'});
    put_be32(prefix, width);
    put_be32(prefix, height);
    prefix.insert(prefix.end(), {8, colour_type[channels], 0, 0, 0});
    put_be32(prefix, pc::crc32(prefix.data() + ihdr, prefix.size() - ihdr));
    put_be32(prefix, (uint32_t)idat_bytes);
    prefix.insert(prefix.end(), {'I', 'D', 'A', 'T', 0x78, 0x01});
    prefix.insert(prefix.end(), codes.header.bytes.begin(), codes.header.bytes.begin() + (size_t)(header_bits / 8)); // whole bytes only
    const uint32_t header_partial = (header_bits & 7u) ? codes.header.bytes.back() : 0u;
    uint8_t *stream = d_out + PREFIX_BYTES + 2, *stream_end = stream + stream_bytes;
    const uintptr_t misaligned = reinterpret_cast<uintptr_t>(stream) & 3u;
    uint32_t *words = reinterpret_cast<uint32_t *>(stream - misaligned);
    const unsigned long long n_words = (unsigned long long)((d_out + size) - (stream - misaligned)) / 4, first_bit = 8 * misaligned + header_bits;
    const uint32_t crc_seed = pc::crc_multiply(pc::crc_shift(idat_bytes), pc::crc32(reinterpret_cast<const uint8_t *>("IDAT"), 4));
    const unsigned long long pieces = (idat_bytes + CRC_PIECE - 1) / CRC_PIECE;
    e = hipMemcpyAsync(d_out, prefix.data(), prefix.size(), hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipMemsetAsync(d_out + prefix.size(), 0, (size_t)(stream_end - (d_out + prefix.size())), s);
    if (e != hipSuccess) return device_error("png_encode", e);
    hipLaunchKernelGGL(png_write_kernel, grid, wave, 0, s, filtered, n, height, table, row_bits, first_bit, words, n_words);
    hipLaunchKernelGGL(png_trailer_kernel, dim3(1), dim3(256), 0, s, sums, height, n, words, n_words, (unsigned long long)(8 * misaligned + header_bits),
                       header_partial, (unsigned long long)(first_bit + body_bits), eob_entry, stream_end, crc, crc_seed);
    hipLaunchKernelGGL(png_crc_kernel, dim3(grid_for(pieces)), dim3(256), 0, s, d_out + PREFIX_BYTES, (unsigned long long)idat_bytes, pieces, crc);
    hipLaunchKernelGGL(png_finish_kernel, dim3(1), dim3(1), 0, s, crc, stream_end + 4);
    e = hipGetLastError();
    if (e == hipSuccess) e = sc.copy_out(out, d_out, (size_t)size, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) return device_error("png_encode", e);
    return CVHIP_OK;
}
