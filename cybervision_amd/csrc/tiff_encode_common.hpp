// tiff_encode_common.hpp — what the host and the kernels of cvhip_tiff_encode share (tiff_encode_kernels.hip), as
// plain C++ that also compiles without HIP (tests/cpp/tiff_out_host.cpp runs it on the CPU under sanitizers): the refusals and the
// strip layout, the bytes in front of the strips, the width of an LZW code, the step of the LZW walk over a byte against the
// (prefix, byte) -> code table, and the PackBits walk of one row.  tests/ref_tiff_out.py is the definition.
#pragma once

#include <cstdint>
#include <vector>

#if defined(__HIPCC__)
#define TIFF_ENCODE_HD __host__ __device__ __forceinline__
#else
#define TIFF_ENCODE_HD inline
#endif

namespace tiff_encode_common {

constexpr uint32_t COMPRESSION_NONE = 1, COMPRESSION_LZW = 5, COMPRESSION_PACKBITS = 32773;
constexpr uint32_t LZW_CLEAR = 256, LZW_EOI = 257;
constexpr uint32_t LZW_CLEAR_AFTER = 3836;  // codes since a Clear: entry 4093 was the last one added, as libtiff has it
constexpr uint32_t LZW_SLOTS = 8192;        // of the hash table: at most 3836 are live
constexpr uint32_t LZW_EMPTY = 0xFFFFFFFFu; // no key has the prefix 4095
constexpr uint32_t LZW_NO_PREFIX = 0xFFFFu;
constexpr uint32_t LZW_CHUNK = 1024;        // bytes of a strip the kernel stages at a time: 37 KB of LDS a wave, four waves a CU
constexpr uint32_t LZW_CHUNK_CODES = LZW_CHUNK + 8; // a code a byte, the first Clear, two Clears inside, the last code + Clear + EOI

// the width of the c-th code since a Clear (c = 0 is the first): the next free entry is 257 + c, libtiff's early change
TIFF_ENCODE_HD uint32_t lzw_code_width(uint32_t c) { return c < 254 ? 9u : c < 766 ? 10u : c < 1790 ? 11u : 12u; }

struct LzwState {
    uint32_t prefix = LZW_NO_PREFIX; // the code of the pending string
    uint32_t c = 0;                  // codes since the last Clear
};

// table[slot] = key << 12 | code, key = prefix << 8 | byte.  The probe is bounded by the slots.
// One byte of the strip.  put(code, width) once per code that leaves.  true: a Clear left, the table is to be emptied
// (all slots LZW_EMPTY) before the next byte.
template <typename Put> TIFF_ENCODE_HD bool lzw_byte(uint32_t *table, LzwState &st, uint32_t byte, Put &&put)
{
    if (st.prefix == LZW_NO_PREFIX) {
        st.prefix = byte;
        return false;
    }
    const uint32_t key = st.prefix << 8 | byte;
    uint32_t slot = (key * 2654435761u) >> 19, probe = 0;
    for (; probe < LZW_SLOTS; probe++, slot = (slot + 1u) & (LZW_SLOTS - 1u)) {
        const uint32_t e = table[slot];
        if (e == LZW_EMPTY) break;
        if ((e >> 12) == key) {
            st.prefix = e & 0xFFFu;
            return false;
        }
    }
    put(st.prefix, lzw_code_width(st.c));
    if (probe < LZW_SLOTS) table[slot] = key << 12 | (258u + st.c);
    st.c++;
    st.prefix = byte;
    if (st.c < LZW_CLEAR_AFTER) return false;
    put(LZW_CLEAR, lzw_code_width(st.c));
    st.c = 0;
    return true;
}
// The strip's end: the pending string, a Clear when that was the 3836th code (libtiff's LZWPostEncode), EOI.
template <typename Put> TIFF_ENCODE_HD void lzw_finish(LzwState &st, Put &&put)
{
    if (st.prefix != LZW_NO_PREFIX) {
        put(st.prefix, lzw_code_width(st.c));
        st.c++;
        if (st.c == LZW_CLEAR_AFTER) {
            put(LZW_CLEAR, lzw_code_width(st.c));
            st.c = 0;
        }
    }
    put(LZW_EOI, lzw_code_width(st.c));
}

// PackBits of one row of n bytes, the greedy rule: from the position the maximal run of equal bytes, at most 128; 3 or more
// are a run packet; otherwise a literal packet to where three equal bytes begin, to 128 bytes or to the row's end.  out holds
// n + (n + 127) / 128 bytes.  -> the bytes written; packets += the packets.
TIFF_ENCODE_HD uint32_t packbits_row(const uint8_t *row, uint32_t n, uint8_t *out, uint32_t &packets)
{
    uint32_t at = 0, o = 0;
    while (at < n) {
        uint32_t run = 1;
        while (at + run < n && run < 128 && row[at + run] == row[at]) run++;
        packets++;
        if (run >= 3) {
            out[o++] = (uint8_t)(257u - run);
            out[o++] = row[at];
            at += run;
            continue;
        }
        uint32_t end = at;
        while (end < n && end - at < 128 && !(end + 2 < n && row[end] == row[end + 1] && row[end] == row[end + 2])) end++;
        out[o++] = (uint8_t)(end - at - 1u);
        for (uint32_t k = at; k < end; k++) out[o++] = row[k];
        at = end;
    }
    return o;
}

// ---- the file's layout --------------------------------------------------------------------------------------------------------
enum Refusal { ACCEPTED = 0, REFUSED_INVALID = 1, REFUSED_UNSUPPORTED = 2 };

struct Layout {
    uint32_t width = 0, height = 0, channels = 0, compression = 0, predictor = 0;
    uint32_t row_bytes = 0, rows_per_strip = 0, strips = 0, entries = 0;
    uint32_t offsets_at = 0, counts_at = 0; // of the two arrays (strips > 1), else 0
    uint32_t data_at = 0;                   // of the first strip
    const char *why = "";
};

inline uint32_t default_rows_per_strip(uint32_t row_bytes) { return row_bytes >= 8192 ? 1u : 8192u / row_bytes; } // TIFF 6.0: about 8 KB

// the bound on a strip's bytes: the stride of the kernels' scratch
inline uint64_t worst_strip(uint32_t compression, uint64_t rows, uint64_t row_bytes)
{
    const uint64_t n = rows * row_bytes;
    if (compression == COMPRESSION_NONE) return n;
    if (compression == COMPRESSION_PACKBITS) return rows * (row_bytes + (row_bytes + 127) / 128);
    const uint64_t codes = n + 2 + n / LZW_CLEAR_AFTER + 1;
    return (12 * codes + 7) / 8;
}

// the size of an uncompressed file: known without the pixels
inline uint64_t raw_file_size(const Layout &l)
{
    const uint64_t full = (uint64_t)l.rows_per_strip * l.row_bytes, last = (uint64_t)(l.height - (l.strips - 1) * l.rows_per_strip) * l.row_bytes;
    return l.data_at + (uint64_t)(l.strips - 1) * (full + (full & 1u)) + last;
}

inline Refusal plan(uint32_t width, uint32_t height, uint32_t channels, uint32_t compression, uint32_t predictor, uint32_t rows_per_strip, Layout &l)
{
    auto refuse = [&](Refusal r, const char *why) {
        l.why = why;
        return r;
    };
    if (!width || !height) return refuse(REFUSED_INVALID, "width or height is 0");
    if (channels < 1 || channels > 4) return refuse(REFUSED_INVALID, "channels is not 1, 2, 3 or 4");
    if (compression != COMPRESSION_NONE && compression != COMPRESSION_LZW && compression != COMPRESSION_PACKBITS)
        return refuse(REFUSED_INVALID, "compression is not 1 (none), 5 (LZW) or 32773 (PackBits)");
    if (predictor != 1 && predictor != 2) return refuse(REFUSED_INVALID, "predictor is not 1 or 2");
    if (predictor == 2 && compression != COMPRESSION_LZW) return refuse(REFUSED_INVALID, "Predictor 2 without LZW");
    if (width >= 65536 || height >= 65536) return refuse(REFUSED_UNSUPPORTED, "a dimension of 65536 or more");
    l.width = width, l.height = height, l.channels = channels, l.compression = compression, l.predictor = predictor;
    l.row_bytes = width * channels;
    const uint32_t rps = rows_per_strip ? rows_per_strip : default_rows_per_strip(l.row_bytes);
    l.rows_per_strip = rps < height ? rps : height;
    if ((uint64_t)l.rows_per_strip * l.row_bytes >= (1ull << 31)) return refuse(REFUSED_UNSUPPORTED, "a strip of 2^31 bytes or more");
    l.strips = (height + l.rows_per_strip - 1) / l.rows_per_strip;
    l.entries = 10 + (predictor == 2 ? 1 : 0) + (channels == 2 || channels == 4 ? 1 : 0);
    uint32_t at = 8 + 2 + 12 * l.entries + 4;
    if (channels > 2) at += 2 * channels;
    l.offsets_at = l.counts_at = 0;
    if (l.strips > 1) l.offsets_at = at, l.counts_at = at + 4 * l.strips, at += 8 * l.strips;
    l.data_at = at;
    if (compression == COMPRESSION_NONE && raw_file_size(l) >= (1ull << 32)) return refuse(REFUSED_UNSUPPORTED, "a file of 2^32 bytes or more");
    return ACCEPTED;
}

// The bytes in front of the StripOffsets array - or, of a one-strip file, in front of the strip: its offset and its
// count (first_count) stand inline.
inline std::vector<uint8_t> header(const Layout &l, uint32_t first_count)
{
    std::vector<uint8_t> out, tail;
    auto u16 = [](std::vector<uint8_t> &v, uint32_t x) { v.push_back((uint8_t)x), v.push_back((uint8_t)(x >> 8)); };
    auto u32 = [&](std::vector<uint8_t> &v, uint32_t x) { u16(v, x & 0xFFFFu), u16(v, x >> 16); };
    uint32_t at = 8 + 2 + 12 * l.entries + 4;
    auto entry = [&](uint32_t tag, uint32_t type, uint32_t count, uint32_t value) { u16(out, tag), u16(out, type), u32(out, count), u32(out, value); };
    auto one_short = [&](uint32_t tag, uint32_t value) { entry(tag, 3, 1, value); };
    out = {'I', 'I', 42, 0, 8, 0, 0, 0};
    u16(out, l.entries);
    entry(256, 4, 1, l.width);
    entry(257, 4, 1, l.height);
    if (l.channels <= 2)
        entry(258, 3, l.channels, l.channels == 1 ? 8u : 8u | 8u << 16);
    else {
        entry(258, 3, l.channels, at);
        for (uint32_t k = 0; k < l.channels; k++) u16(tail, 8);
        at += 2 * l.channels;
    }
    one_short(259, l.compression);
    one_short(262, l.channels <= 2 ? 1 : 2);
    entry(273, 4, l.strips, l.strips > 1 ? l.offsets_at : l.data_at);
    one_short(277, l.channels);
    entry(278, 4, 1, l.rows_per_strip);
    entry(279, 4, l.strips, l.strips > 1 ? l.counts_at : first_count);
    one_short(284, 1);
    if (l.predictor == 2) one_short(317, 2);
    if (l.channels == 2 || l.channels == 4) one_short(338, 2);
    u32(out, 0);
    out.insert(out.end(), tail.begin(), tail.end());
    return out;
}

} // namespace tiff_encode_common
