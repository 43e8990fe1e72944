// png_common.hpp — the host side of cvhip_png_encode (png_kernels.hip) as plain C++ that also compiles
// without HIP (tests/cpp/png_host.cpp runs it on the CPU under sanitizers): the length-limited code lengths (package-merge),
// the canonical codes, the token table the kernels index, the dynamic block's header bits, and the arithmetic that
// combines CRC-32 and Adler-32 values of pieces into the value of the whole.  tests/ref_png.py is the definition.
#pragma once

#include <algorithm>
#include <cstdint>
#include <utility>
#include <vector>

#if defined(__HIPCC__)
#define PNG_FN __host__ __device__ inline
#else
#define PNG_FN inline
#endif

namespace png_common {

constexpr uint32_t LITLEN_SYMBOLS = 286, EOB = 256;
constexpr uint32_t TOKEN_MATCH = 256;        // a token: a literal 0..255, or TOKEN_MATCH + (length - 3) for a match of 3..258 at distance 1
constexpr uint32_t TOKEN_EOB = 512, TOKENS = 513;
constexpr uint32_t TOKEN_BITS_MAX = 15 + 5 + 1; // a length code, its extra bits, the one-bit distance code
constexpr uint32_t ADLER_MOD = 65521, CRC_POLY = 0xEDB88320u;

// ---- RFC 1951 3.2.5: the symbol of a match length 3..258, its extra bits and their value ----------------------------------------
PNG_FN uint32_t length_symbol(uint32_t length, uint32_t &extra, uint32_t &value)
{
    const uint32_t x = length - 3;
    extra = 0, value = 0;
    if (x < 8) return 257 + x;
    if (x == 255) return 285;
    uint32_t top = 3; // the highest set bit of x (3..7)
    while ((x >> (top + 1)) != 0) top++;
    extra = top - 2;
    value = x & ((1u << extra) - 1u);
    return 257 + 4 * (extra + 1) + ((x >> extra) & 3u);
}
PNG_FN uint32_t token_symbol(uint32_t token)
{
    uint32_t extra, value;
    return token < TOKEN_MATCH ? token : token == TOKEN_EOB ? EOB : length_symbol(token - TOKEN_MATCH + 3, extra, value);
}

// ---- CRC-32 (reflected, as PNG and zlib use it) ------------------------------------------------------------------------------------
// a(x) * b(x) mod the polynomial; bit 31 is x^0
PNG_FN uint32_t crc_multiply(uint32_t a, uint32_t b)
{
    uint32_t p = 0;
    for (uint32_t m = 1u << 31; m; m >>= 1) {
        if (a & m) p ^= b;
        b = (b & 1u) ? (b >> 1) ^ CRC_POLY : b >> 1;
    }
    return p;
}
// x^(8 * bytes) mod the polynomial
PNG_FN uint32_t crc_shift(uint64_t bytes)
{
    uint32_t p = 1u << 31, square = 1u << 23; // x^0; x^8
    for (; bytes; bytes >>= 1) {
        if (bytes & 1u) p = crc_multiply(square, p);
        square = crc_multiply(square, square);
    }
    return p;
}
// the CRC of A followed by B from crc(A), crc(B) and B's length
PNG_FN uint32_t crc_combine(uint32_t crc_a, uint32_t crc_b, uint64_t bytes_b) { return crc_multiply(crc_shift(bytes_b), crc_a) ^ crc_b; }
PNG_FN uint32_t crc_table_entry(uint32_t n)
{
    for (int k = 0; k < 8; k++) n = (n & 1u) ? (n >> 1) ^ CRC_POLY : n >> 1;
    return n;
}
inline uint32_t crc32(const uint8_t *data, size_t n)
{
    uint32_t c = 0xFFFFFFFFu;
    for (size_t i = 0; i < n; i++) c = crc_table_entry((c ^ data[i]) & 0xFFu) ^ (c >> 8);
    return c ^ 0xFFFFFFFFu;
}

// ---- Adler-32 ---------------------------------------------------------------------------------------------------------------------
// A piece of n bytes d[0 .. n) has the sums a = sum d[i] and b = sum (n - i) d[i], both mod 65521 (the checksum of the piece
// alone is (1 + a, n + b)).  Of A followed by B: a = a_A + a_B, b = b_A + n_B a_A + b_B.
struct AdlerSums {
    uint32_t a, b;
};
PNG_FN AdlerSums adler_join(AdlerSums first, AdlerSums second, uint64_t bytes_second)
{
    const uint64_t n = bytes_second % ADLER_MOD;
    return {(uint32_t)(((uint64_t)first.a + second.a) % ADLER_MOD), (uint32_t)(((uint64_t)first.b + n * first.a + second.b) % ADLER_MOD)};
}
// the Adler-32 of the whole from its sums and its length
PNG_FN uint32_t adler_value(AdlerSums whole, uint64_t bytes)
{
    const uint32_t a = (1u + whole.a) % ADLER_MOD, b = (uint32_t)((bytes % ADLER_MOD + whole.b) % ADLER_MOD);
    return b << 16 | a;
}

// ---- code lengths: package-merge ------------------------------------------------------------------------------------------------
// Leaves sorted by (frequency, symbol); each of limit - 1 rounds pairs the current list into packages and merges the leaves
// with them by weight, stably, a leaf first on equal weight; the first 2 k - 2 items of the last list each add one to the
// length of the symbols they hold.  A lone symbol gets length 1.  k <= 2^limit.
inline std::vector<uint8_t> package_merge(const uint64_t *freqs, size_t n, int limit)
{
    std::vector<std::pair<uint64_t, uint32_t>> leaves;
    for (size_t s = 0; s < n; s++)
        if (freqs[s]) leaves.push_back({freqs[s], (uint32_t)s});
    std::sort(leaves.begin(), leaves.end());
    const size_t k = leaves.size();
    std::vector<uint8_t> lengths(n, 0);
    if (k == 0) return lengths;
    if (k == 1) {
        lengths[leaves[0].second] = 1;
        return lengths;
    }
    struct Item {
        uint64_t weight;
        std::vector<uint16_t> holds; // how often each leaf is in the item
    };
    std::vector<Item> leaf_items(k), current;
    for (size_t i = 0; i < k; i++) {
        leaf_items[i].weight = leaves[i].first;
        leaf_items[i].holds.assign(k, 0);
        leaf_items[i].holds[i] = 1;
    }
    current = leaf_items;
    for (int round = 1; round < limit; round++) {
        std::vector<Item> packages(current.size() / 2);
        for (size_t i = 0; i < packages.size(); i++) {
            packages[i].weight = current[2 * i].weight + current[2 * i + 1].weight;
            packages[i].holds = current[2 * i].holds;
            for (size_t j = 0; j < k; j++) packages[i].holds[j] = (uint16_t)(packages[i].holds[j] + current[2 * i + 1].holds[j]);
        }
        std::vector<Item> merged;
        merged.reserve(k + packages.size());
        size_t li = 0, pi = 0;
        while (li < k || pi < packages.size()) {
            if (pi >= packages.size() || (li < k && leaf_items[li].weight <= packages[pi].weight))
                merged.push_back(leaf_items[li++]);
            else
                merged.push_back(std::move(packages[pi++]));
        }
        current.swap(merged);
    }
    for (size_t i = 0; i < 2 * k - 2 && i < current.size(); i++)
        for (size_t j = 0; j < k; j++) lengths[leaves[j].second] = (uint8_t)(lengths[leaves[j].second] + current[i].holds[j]);
    return lengths;
}

// RFC 1951 3.2.2: the code of each symbol as the RFC numbers it (its first bit is the most significant)
inline std::vector<uint32_t> canonical_codes(const std::vector<uint8_t> &lengths)
{
    uint32_t count[17] = {0}, next[17] = {0};
    for (uint8_t n : lengths) count[n]++;
    count[0] = 0;
    uint32_t code = 0;
    for (int bits = 1; bits <= 16; bits++) {
        code = (code + count[bits - 1]) << 1;
        next[bits] = code;
    }
    std::vector<uint32_t> codes(lengths.size(), 0);
    for (size_t s = 0; s < lengths.size(); s++)
        if (lengths[s]) codes[s] = next[lengths[s]]++;
    return codes;
}
inline uint32_t reverse_bits(uint32_t v, uint32_t n)
{
    uint32_t r = 0;
    for (uint32_t i = 0; i < n; i++) r |= ((v >> i) & 1u) << (n - 1 - i);
    return r;
}

struct BitBuffer {
    std::vector<uint8_t> bytes;
    uint64_t nbits = 0;
    void bits(uint32_t value, uint32_t count) // least significant bit first
    {
        for (uint32_t i = 0; i < count; i++, nbits++) {
            if ((nbits & 7u) == 0) bytes.push_back(0);
            bytes.back() = (uint8_t)(bytes.back() | (((value >> i) & 1u) << (nbits & 7u)));
        }
    }
    void code(uint32_t code, uint32_t count) { bits(reverse_bits(code, count), count); } // a Huffman code: most significant bit first
};

// What the kernels need of a histogram of the 286 literal/length symbols (end-of-block counted):
struct BlockCodes {
    std::vector<uint8_t> lengths;    // 286 code lengths
    std::vector<uint8_t> cl_lengths; // the 19 lengths of the code-length code
    uint32_t hlit = 0, hclen = 0;
    BitBuffer header;                // BFINAL .. the last code length
    uint32_t table[TOKENS];          // per token: its bits, first bit lowest, in the low 24 bits; their number above
};
inline BlockCodes block_codes(const uint64_t *histogram)
{
    static const uint8_t CL_ORDER[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
    BlockCodes bc;
    bc.lengths = package_merge(histogram, LITLEN_SYMBOLS, 15);
    const std::vector<uint32_t> codes = canonical_codes(bc.lengths);
    bc.hlit = 257;
    for (uint32_t s = 257; s < LITLEN_SYMBOLS; s++)
        if (bc.lengths[s]) bc.hlit = s + 1;
    std::vector<uint8_t> sent(bc.lengths.begin(), bc.lengths.begin() + bc.hlit);
    sent.push_back(1); // HDIST = 1: distance symbol 0, one bit
    uint64_t cl_freq[19] = {0};
    for (uint8_t n : sent) cl_freq[n]++;
    bc.cl_lengths = package_merge(cl_freq, 19, 7);
    const std::vector<uint32_t> cl_codes = canonical_codes(bc.cl_lengths);
    bc.hclen = 4;
    for (uint32_t i = 4; i < 19; i++)
        if (bc.cl_lengths[CL_ORDER[i]]) bc.hclen = i + 1;
    bc.header.bits(1, 1); // BFINAL
    bc.header.bits(2, 2); // BTYPE = 10
    bc.header.bits(bc.hlit - 257, 5);
    bc.header.bits(0, 5); // HDIST - 1
    bc.header.bits(bc.hclen - 4, 4);
    for (uint32_t i = 0; i < bc.hclen; i++) bc.header.bits(bc.cl_lengths[CL_ORDER[i]], 3);
    for (uint8_t n : sent) bc.header.code(cl_codes[n], bc.cl_lengths[n]);
    for (uint32_t t = 0; t < TOKENS; t++) {
        uint32_t extra = 0, value = 0;
        const uint32_t s = t < TOKEN_MATCH ? t : t == TOKEN_EOB ? EOB : length_symbol(t - TOKEN_MATCH + 3, extra, value);
        const uint32_t n = bc.lengths[s];
        if (!n) {
            bc.table[t] = 0;
            continue;
        }
        uint32_t bits = reverse_bits(codes[s], n), count = n;
        if (t >= TOKEN_MATCH && t != TOKEN_EOB) bits |= value << n, count += extra + 1; // the distance code is one 0 bit
        bc.table[t] = bits | count << 24;
    }
    return bc;
}

} // namespace png_common
