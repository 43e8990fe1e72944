// jpeg_encode_common.hpp — the host side of cvhip_jpeg_encode (jpeg_encode_kernels.hip) as plain C++ that also
// compiles without HIP (tests/cpp/jpeg_out_host.cpp runs it on the CPU under sanitizers): the quality scaling of the Annex K
// quantisation tables, the Annex K Huffman tables, libjpeg's optimal table from a histogram, the code table the kernels
// index, the scan's geometry and the segments in front of the scan.  tests/ref_jpeg_out.py is the definition.
#pragma once

#include <cstdint>
#include <cstring>
#include <vector>

#include "jpeg_common.hpp"

namespace jpeg_encode_common {

using jpeg_common::ZIGZAG;

constexpr uint32_t TABLE_SYMBOLS = 16 + 256;          // of one table pair: the DC categories, then the AC symbols
constexpr uint32_t TABLE_ENTRIES = 2 * TABLE_SYMBOLS; // pair 0 (luma), pair 1 (chroma)
constexpr uint32_t STUFF_TILE = 1024;                 // bytes of the unstuffed stream per workgroup of the stuffing pass
constexpr uint64_t MAX_BLOCKS = 1ull << 25;           // (the decoder's limit)

// ---- ITU-T T.81 Annex K: the example tables ----------------------------------------------------------------------------------------
constexpr uint8_t QUANT_LUMA[64] = {16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57,
                                    69, 56, 14, 17, 22, 29, 51, 87, 80, 62, 18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64,
                                    81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99};
constexpr uint8_t QUANT_CHROMA[64] = {17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99,
                                      99, 99, 47, 66, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99,
                                      99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99};

struct HuffSpec {
    uint8_t bits[16] = {0};   // codes of length 1 .. 16
    uint8_t values[256] = {0};
    uint32_t total = 0;
};

inline HuffSpec make_spec(const uint8_t *bits, const uint8_t *values)
{
    HuffSpec s;
    for (int i = 0; i < 16; i++) s.bits[i] = bits[i], s.total += bits[i];
    std::memcpy(s.values, values, s.total);
    return s;
}

// table 0 .. 3: DC luma, AC luma, DC chroma, AC chroma - the order of the DHT segments
inline HuffSpec standard_table(uint32_t table)
{
    static const uint8_t dc_values[12] = {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11};
    static const uint8_t dc_luma_bits[16] = {0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0};
    static const uint8_t dc_chroma_bits[16] = {0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0};
    static const uint8_t ac_luma_bits[16] = {0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7D};
    static const uint8_t ac_luma_values[162] = {
        0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81,
        0x91, 0xA1, 0x08, 0x23, 0x42, 0xB1, 0xC1, 0x15, 0x52, 0xD1, 0xF0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0A, 0x16, 0x17, 0x18,
        0x19, 0x1A, 0x25, 0x26, 0x27, 0x28, 0x29, 0x2A, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3A, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48,
        0x49, 0x4A, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5A, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6A, 0x73, 0x74, 0x75,
        0x76, 0x77, 0x78, 0x79, 0x7A, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8A, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99,
        0x9A, 0xA2, 0xA3, 0xA4, 0xA5, 0xA6, 0xA7, 0xA8, 0xA9, 0xAA, 0xB2, 0xB3, 0xB4, 0xB5, 0xB6, 0xB7, 0xB8, 0xB9, 0xBA, 0xC2, 0xC3,
        0xC4, 0xC5, 0xC6, 0xC7, 0xC8, 0xC9, 0xCA, 0xD2, 0xD3, 0xD4, 0xD5, 0xD6, 0xD7, 0xD8, 0xD9, 0xDA, 0xE1, 0xE2, 0xE3, 0xE4, 0xE5,
        0xE6, 0xE7, 0xE8, 0xE9, 0xEA, 0xF1, 0xF2, 0xF3, 0xF4, 0xF5, 0xF6, 0xF7, 0xF8, 0xF9, 0xFA};
    static const uint8_t ac_chroma_bits[16] = {0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77};
    static const uint8_t ac_chroma_values[162] = {
        0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08,
        0x14, 0x42, 0x91, 0xA1, 0xB1, 0xC1, 0x09, 0x23, 0x33, 0x52, 0xF0, 0x15, 0x62, 0x72, 0xD1, 0x0A, 0x16, 0x24, 0x34, 0xE1, 0x25,
        0xF1, 0x17, 0x18, 0x19, 0x1A, 0x26, 0x27, 0x28, 0x29, 0x2A, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3A, 0x43, 0x44, 0x45, 0x46, 0x47,
        0x48, 0x49, 0x4A, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5A, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6A, 0x73, 0x74,
        0x75, 0x76, 0x77, 0x78, 0x79, 0x7A, 0x82, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8A, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97,
        0x98, 0x99, 0x9A, 0xA2, 0xA3, 0xA4, 0xA5, 0xA6, 0xA7, 0xA8, 0xA9, 0xAA, 0xB2, 0xB3, 0xB4, 0xB5, 0xB6, 0xB7, 0xB8, 0xB9, 0xBA,
        0xC2, 0xC3, 0xC4, 0xC5, 0xC6, 0xC7, 0xC8, 0xC9, 0xCA, 0xD2, 0xD3, 0xD4, 0xD5, 0xD6, 0xD7, 0xD8, 0xD9, 0xDA, 0xE2, 0xE3, 0xE4,
        0xE5, 0xE6, 0xE7, 0xE8, 0xE9, 0xEA, 0xF2, 0xF3, 0xF4, 0xF5, 0xF6, 0xF7, 0xF8, 0xF9, 0xFA};
    switch (table) {
    case 0: return make_spec(dc_luma_bits, dc_values);
    case 1: return make_spec(ac_luma_bits, ac_luma_values);
    case 2: return make_spec(dc_chroma_bits, dc_values);
    default: return make_spec(ac_chroma_bits, ac_chroma_values);
    }
}

// jpeg_set_quality with force_baseline: out[64] in natural order, 1 .. 255
inline void quant_table(const uint8_t *base, uint32_t quality, uint16_t *out)
{
    const uint32_t scale = quality < 50 ? 5000u / quality : 200u - 2u * quality;
    for (int i = 0; i < 64; i++) {
        const uint32_t v = (base[i] * scale + 50u) / 100u;
        out[i] = (uint16_t)(v < 1 ? 1 : v > 255 ? 255 : v);
    }
}

// libjpeg's jpeg_gen_optimal_table: freq[256] -> the table.  A 257th symbol of count 1 keeps the all-ones code free; the two
// least non-zero counts are merged (of equal counts the LARGEST symbol, the second pick excluding the first); the code sizes
// follow the `others` chain; sizes above 16 are folded down by the Annex K.3 step, from whatever depth (libjpeg stops at 32);
// counts are 64-bit and not capped (libjpeg ignores a count above 10^9).  unfolded_max: the longest size before the fold.
inline HuffSpec optimal_table(const uint64_t *freq_in, uint32_t *unfolded_max = nullptr)
{
    uint64_t freq[257];
    uint32_t codesize[257] = {0};
    int others[257];
    for (int i = 0; i < 256; i++) freq[i] = freq_in[i];
    freq[256] = 1;
    for (int i = 0; i < 257; i++) others[i] = -1;
    for (;;) {
        int c1 = -1, c2 = -1;
        for (int i = 0; i < 257; i++)
            if (freq[i] && (c1 < 0 || freq[i] <= freq[c1])) c1 = i;
        for (int i = 0; i < 257; i++)
            if (freq[i] && i != c1 && (c2 < 0 || freq[i] <= freq[c2])) c2 = i;
        if (c2 < 0) break;
        freq[c1] += freq[c2];
        freq[c2] = 0;
        codesize[c1]++;
        while (others[c1] >= 0) c1 = others[c1], codesize[c1]++;
        others[c1] = c2;
        codesize[c2]++;
        while (others[c2] >= 0) c2 = others[c2], codesize[c2]++;
    }
    uint32_t bits[258] = {0}, top = 16; // (a chain of 257 symbols is 256 deep)
    for (int i = 0; i < 257; i++)
        if (codesize[i]) bits[codesize[i]]++, top = codesize[i] > top ? codesize[i] : top;
    if (unfolded_max) *unfolded_max = top;
    for (uint32_t i = top; i > 16; i--)
        while (bits[i] > 0) {
            uint32_t j = i - 2;
            while (bits[j] == 0) j--;
            bits[i] -= 2, bits[i - 1]++, bits[j + 1] += 2, bits[j]--;
        }
    uint32_t last = 16;
    while (last && bits[last] == 0) last--;
    if (last) bits[last]--; // the 257th symbol's code (no counts at all: an empty table)
    HuffSpec s;
    for (int i = 0; i < 16; i++) s.bits[i] = (uint8_t)bits[i + 1];
    for (uint32_t n = 1; n <= top; n++)
        for (int v = 0; v < 256; v++)
            if (codesize[v] == n) s.values[s.total++] = (uint8_t)v;
    return s;
}

// entries[symbol] = code length << 16 | code (the canonical codes of Annex C), 0 for a symbol without a code
inline void code_table(const HuffSpec &spec, uint32_t *entries, uint32_t n_entries)
{
    for (uint32_t k = 0; k < n_entries; k++) entries[k] = 0;
    uint32_t code = 0, k = 0;
    for (uint32_t n = 1; n <= 16; n++) {
        for (uint32_t c = 0; c < spec.bits[n - 1]; c++, code++, k++)
            if (spec.values[k] < n_entries) entries[spec.values[k]] = n << 16 | code;
        code <<= 1;
    }
}

// what the kernels index: table[pair * TABLE_SYMBOLS + category] for DC, table[pair * TABLE_SYMBOLS + 16 + symbol] for AC;
// specs in the order DC0, AC0, DC1, AC1 (n_specs = 2 leaves pair 1 zero)
inline void kernel_table(const HuffSpec *specs, uint32_t n_specs, uint32_t *table)
{
    for (uint32_t k = 0; k < TABLE_ENTRIES; k++) table[k] = 0;
    for (uint32_t k = 0; k < n_specs; k++) code_table(specs[k], table + (k >> 1) * TABLE_SYMBOLS + (k & 1u) * 16, (k & 1u) ? 256 : 16);
}

// ---- the scan's geometry ---------------------------------------------------------------------------------------------------------------
struct Geometry {
    uint32_t width, height, channels, components;
    uint32_t hs, vs;             // luma blocks per MCU across and down
    uint32_t mcus_x, mcus_y;
    uint32_t blocks_x, blocks_y; // the luma component's width and height in blocks
    uint32_t bpm;                // blocks per MCU
};
inline Geometry geometry(uint32_t width, uint32_t height, uint32_t channels, uint32_t sampling)
{
    Geometry g{};
    g.width = width, g.height = height, g.channels = channels, g.components = channels <= 2 ? 1u : 3u;
    g.hs = g.components == 3 && sampling >= 1 ? 2u : 1u, g.vs = g.components == 3 && sampling == 2 ? 2u : 1u;
    g.mcus_x = (width + 8 * g.hs - 1) / (8 * g.hs), g.mcus_y = (height + 8 * g.vs - 1) / (8 * g.vs);
    g.blocks_x = (width + 7) / 8, g.blocks_y = (height + 7) / 8;
    g.bpm = g.components == 3 ? g.hs * g.vs + 2 : 1;
    return g;
}
inline uint64_t total_blocks(const Geometry &g) { return (uint64_t)g.mcus_x * g.mcus_y * g.bpm; }
// the luma blocks that lie beyond blocks_x or blocks_y: not computed from pixels
inline uint64_t dummy_blocks(const Geometry &g)
{
    return (uint64_t)g.mcus_x * g.hs * g.mcus_y * g.vs - (uint64_t)g.blocks_x * g.blocks_y;
}

// ---- SOI .. SOS --------------------------------------------------------------------------------------------------------------------------
inline void put_segment(std::vector<uint8_t> &out, uint8_t marker, const std::vector<uint8_t> &body)
{
    const size_t n = body.size() + 2;
    out.insert(out.end(), {0xFF, marker, (uint8_t)(n >> 8), (uint8_t)n});
    out.insert(out.end(), body.begin(), body.end());
}
// quants: components == 3 ? 2 : 1 tables of 64 in natural order; specs: 4 or 2 tables in the order DC0, AC0, DC1, AC1
inline std::vector<uint8_t> header(const Geometry &g, const uint16_t (*quants)[64], const HuffSpec *specs)
{
    std::vector<uint8_t> out = {0xFF, 0xD8};
    put_segment(out, 0xE0, {'J', 'F', 'I', 'F', 0, 1, 1, 0, 0, 1, 0, 1, 0, 0});
    const uint32_t pairs = g.components == 3 ? 2 : 1;
    for (uint32_t k = 0; k < pairs; k++) {
        std::vector<uint8_t> body = {(uint8_t)k};
        for (int i = 0; i < 64; i++) body.push_back((uint8_t)quants[k][ZIGZAG[i]]);
        put_segment(out, 0xDB, body);
    }
    std::vector<uint8_t> frame = {8, (uint8_t)(g.height >> 8), (uint8_t)g.height, (uint8_t)(g.width >> 8), (uint8_t)g.width, (uint8_t)g.components};
    for (uint32_t c = 0; c < g.components; c++)
        frame.insert(frame.end(), {(uint8_t)(c + 1), (uint8_t)(c == 0 ? g.hs << 4 | g.vs : 0x11), (uint8_t)(c ? 1 : 0)});
    put_segment(out, 0xC0, frame);
    for (uint32_t k = 0; k < 2 * pairs; k++) {
        std::vector<uint8_t> body = {(uint8_t)((k & 1u) << 4 | k >> 1)};
        body.insert(body.end(), specs[k].bits, specs[k].bits + 16);
        body.insert(body.end(), specs[k].values, specs[k].values + specs[k].total);
        put_segment(out, 0xC4, body);
    }
    std::vector<uint8_t> scan = {(uint8_t)g.components};
    for (uint32_t c = 0; c < g.components; c++) scan.insert(scan.end(), {(uint8_t)(c + 1), (uint8_t)(c ? 0x11 : 0x00)});
    scan.insert(scan.end(), {0, 63, 0});
    put_segment(out, 0xDA, scan);
    return out;
}

} // namespace jpeg_encode_common
