// tiff_common.hpp — the host side of cvhip_tiff_info / cvhip_tiff_decode (tiff_kernels.hip) as plain C++ that
// also compiles without HIP (tests/cpp/tiff_host.cpp runs it on the CPU under sanitizers): the walk of a classic TIFF file's
// first IFD, the strip table, EXIF's FocalLengthIn35mmFilm and the SEM text block of tag 34683 / 34682
// (src/reconstruction.rs:80-144).  tests/ref_tiff.py is the definition, check for check in the same order; every read is
// bounded by the file's size.  parse(.., extended = true) is the walk of cvhip_tiff_ext_info / cvhip_tiff_ext_decode (tiff_ext_kernels.hip,
// DESIGN.md 4.23; tests/ref_tiff_ext.py is its definition): Deflate (8 and 32946) and tiles (tags 322 to 325) are taken too, a
// tile being a stream of TileLength rows of TileWidth pixels; without the flag every file gets the answer it always got.
#pragma once

#include <cstddef>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

namespace tiff_common {

constexpr int OK = 0, INVALID = -1, UNSUPPORTED = -3; // (CVHIP_OK, CVHIP_ERR_INVALID, CVHIP_ERR_UNSUPPORTED)
constexpr uint32_t COMPRESSION_NONE = 1, COMPRESSION_LZW = 5, COMPRESSION_PACKBITS = 32773, COMPRESSION_DEFLATE = 8, COMPRESSION_DEFLATE_OLD = 32946;

struct Strip {
    uint32_t offset = 0, count = 0, rows = 0; // the bytes file[offset .. offset + count) hold `rows` rows
    uint32_t row_bytes = 0, x = 0, y = 0;     // of `row_bytes` bytes each (a tile's rows are whole); its top-left sample is pixel (x, y)
};
struct Header {
    uint32_t width = 0, height = 0, samples = 0, bits = 0, compression = 1, photometric = 0, predictor = 1, rows_per_strip = 0;
    uint32_t focal_length_35mm = 0; // 0 = none
    uint32_t databar_height = 0;
    uint64_t row_bytes = 0;
    uint32_t tile_width = 0, tile_length = 0, tiles_across = 0, tiles_down = 0; // all 0: strips
    bool little = true, sem = false, have_tilt = false;
    float scale[2] = {1.0f, 1.0f}, tilt_angle = 0.0f;
    std::vector<Strip> strips;
    const char *error = "";
};

// ---- Rust's str::parse::<f32> and ::<u32> of s[0 .. n) -----------------------------------------------------------------------
inline size_t digits(const char *s, size_t n, size_t at)
{
    while (at < n && s[at] >= '0' && s[at] <= '9') at++;
    return at;
}
inline bool equals_nocase(const char *s, size_t n, const char *word)
{
    if (std::strlen(word) != n) return false;
    for (size_t k = 0; k < n; k++)
        if ((s[k] | 0x20) != word[k]) return false;
    return true;
}
// an optional sign, then inf / infinity / nan in any case or digits [. digits] [e [sign] digits] with a digit before the
// exponent; the grammar first, then strtof, which rounds the decimal text once
inline bool parse_f32(const char *s, size_t n, float &out)
{
    size_t at = (n && (s[0] == '+' || s[0] == '-')) ? 1 : 0;
    const bool word = equals_nocase(s + at, n - at, "inf") || equals_nocase(s + at, n - at, "infinity") || equals_nocase(s + at, n - at, "nan");
    if (!word) {
        size_t i = digits(s, n, at), mantissa = i - at;
        if (i < n && s[i] == '.') {
            const size_t j = digits(s, n, i + 1);
            mantissa += j - (i + 1);
            i = j;
        }
        if (!mantissa) return false;
        if (i < n && (s[i] == 'e' || s[i] == 'E')) {
            size_t k = i + 1;
            if (k < n && (s[k] == '+' || s[k] == '-')) k++;
            const size_t j = digits(s, n, k);
            if (j == k) return false;
            i = j;
        }
        if (i != n) return false;
    }
    const std::string text(s, n);
    out = std::strtof(text.c_str(), nullptr);
    return true;
}
inline bool parse_u32(const char *s, size_t n, uint32_t &out)
{
    size_t at = (n && s[0] == '+') ? 1 : 0;
    if (at == n || digits(s, n, at) != n) return false;
    uint64_t v = 0;
    for (; at < n; at++) {
        v = v * 10 + (uint64_t)(s[at] - '0');
        if (v > 0xFFFFFFFFull) return false;
    }
    out = (uint32_t)v;
    return true;
}

// str::from_utf8 accepts s[0 .. n)
inline bool valid_utf8(const uint8_t *s, size_t n)
{
    for (size_t i = 0; i < n;) {
        const uint32_t b = s[i];
        uint32_t more = 0, low = 0x80, high = 0xBF;
        if (b < 0x80) {
            i++;
            continue;
        } else if (b >= 0xC2 && b <= 0xDF) more = 1;
        else if (b >= 0xE0 && b <= 0xEF) more = 2, low = b == 0xE0 ? 0xA0 : 0x80, high = b == 0xED ? 0x9F : 0xBF;
        else if (b >= 0xF0 && b <= 0xF4) more = 3, low = b == 0xF0 ? 0x90 : 0x80, high = b == 0xF4 ? 0x8F : 0xBF;
        else return false;
        if (i + more >= n) return false;
        if (s[i + 1] < low || s[i + 1] > high) return false;
        for (uint32_t k = 2; k <= more; k++)
            if (s[i + k] < 0x80 || s[i + k] > 0xBF) return false;
        i += more + 1;
    }
    return true;
}

inline bool starts_with(const std::string &line, const char *prefix) { return line.compare(0, std::strlen(prefix), prefix) == 0; }
// what follows the first '=' of the line
inline bool tag_value(const std::string &line, const char *&value, size_t &n)
{
    const size_t eq = line.find('=');
    if (eq == std::string::npos) return false;
    value = line.data() + eq + 1, n = line.size() - eq - 1;
    return true;
}

// The block's bytes: split at NUL, the pieces that are UTF-8 joined (the others are empty), then the loop of
// reconstruction.rs:107-136 into h.scale, h.tilt_angle / h.have_tilt and h.databar_height.
inline void sem_block(const uint8_t *raw, size_t n, Header &h)
{
    std::string text;
    for (size_t at = 0; at <= n;) {
        const void *nul = at < n ? std::memchr(raw + at, 0, n - at) : nullptr;
        const size_t end = nul ? (size_t)((const uint8_t *)nul - raw) : n;
        if (valid_utf8(raw + at, end - at)) text.append(reinterpret_cast<const char *>(raw + at), end - at);
        at = end + 1;
    }
    std::string section;
    bool have_w = false, have_h = false;
    float w = 1.0f, hh = 1.0f;
    h.have_tilt = false, h.databar_height = 0;
    for (size_t at = 0; at < text.size();) { // (split_terminator: no empty line behind a final separator)
        size_t end = text.find_first_of("\r\n", at);
        if (end == std::string::npos) end = text.size();
        const std::string line = text.substr(at, end - at);
        at = end + 1;
        if (!line.empty() && line.front() == '[' && line.back() == ']') {
            section = line;
            continue;
        }
        const char *value = nullptr;
        size_t len = 0;
        float f = 0.0f;
        uint32_t u = 0;
        if (section == "[Scan]") {
            if (starts_with(line, "PixelWidth")) {
                if (!have_w && tag_value(line, value, len) && parse_f32(value, len, f)) have_w = true, w = f;
            } else if (starts_with(line, "PixelHeight")) {
                if (!have_h && tag_value(line, value, len) && parse_f32(value, len, f)) have_h = true, hh = f;
            }
        } else if (section == "[Stage]") {
            if (starts_with(line, "StageT=")) {
                h.have_tilt = tag_value(line, value, len) && parse_f32(value, len, f);
                h.tilt_angle = h.have_tilt ? f : 0.0f;
            }
        } else if (section == "[PrivateFei]" && starts_with(line, "DatabarHeight=")) {
            if (tag_value(line, value, len) && parse_u32(value, len, u)) h.databar_height = u;
        }
    }
    h.scale[0] = w, h.scale[1] = hh;
}

inline int refuse(Header &h, int code, const char *why)
{
    h.error = why;
    return code;
}

// The first IFD of data[0 .. n) -> OK, INVALID or UNSUPPORTED (h.error says why).
inline int parse(const uint8_t *data, size_t n, Header &h, bool extended = false)
{
    if (n < 8) return refuse(h, INVALID, "truncated header");
    const bool little = data[0] == 'I' && data[1] == 'I', big = data[0] == 'M' && data[1] == 'M';
    if (!little && !big) return refuse(h, INVALID, "no TIFF byte order");
    h.little = little;
    auto u16 = [&](size_t at) -> uint32_t { return little ? (uint32_t)data[at] | (uint32_t)data[at + 1] << 8 : (uint32_t)data[at] << 8 | (uint32_t)data[at + 1]; };
    auto u32 = [&](size_t at) -> uint32_t { return little ? u16(at) | u16(at + 2) << 16 : u16(at) << 16 | u16(at + 2); };
    const uint32_t magic = u16(2);
    if (magic == 43) return refuse(h, UNSUPPORTED, "BigTIFF");
    if (magic != 42) return refuse(h, INVALID, "no TIFF magic");
    const uint64_t ifd = u32(4);
    if (ifd + 2 > n) return refuse(h, INVALID, "truncated IFD");
    const uint32_t entries = u16((size_t)ifd);
    if (ifd + 2 + 12ull * entries > n) return refuse(h, INVALID, "truncated IFD");

    constexpr uint32_t SCALARS[9] = {256, 257, 259, 262, 266, 277, 278, 284, 317}, ARRAYS[5] = {258, 273, 279, 338, 339};
    struct Value {
        bool present = false;
        uint32_t kind = 0, count = 0;
        size_t where = 0;
    };
    Value scalars[9], arrays[5], sem[2], tile[4]; // sem: 34682, 34683; tile: 322 .. 325, read by the extended walk only
    bool tiles = false;
    for (uint32_t k = 0; k < entries; k++) {
        const size_t at = (size_t)ifd + 2 + 12 * (size_t)k;
        const uint32_t tag = u16(at), kind = u16(at + 2), count = u32(at + 4);
        if (tag >= 322 && tag <= 325) tiles = true;
        if ((tag == 34682 || tag == 34683) && !sem[tag - 34682].present) {
            Value &v = sem[tag - 34682];
            v.present = true, v.kind = kind, v.count = count, v.where = at + 8;
        }
        Value *slot = nullptr;
        bool scalar = false;
        for (int i = 0; i < 9; i++)
            if (SCALARS[i] == tag) slot = &scalars[i], scalar = true;
        for (int i = 0; i < 5; i++)
            if (ARRAYS[i] == tag) slot = &arrays[i];
        if (extended && tag >= 322 && tag <= 325) slot = &tile[tag - 322], scalar = tag <= 323;
        if (!slot || slot->present) continue;
        if ((kind != 3 && kind != 4) || count == 0 || (scalar && count != 1)) return refuse(h, INVALID, "a tag's type or count");
        const uint64_t total = (uint64_t)(kind == 3 ? 2 : 4) * count;
        const uint64_t where = total > 4 ? u32(at + 8) : at + 8;
        if (where + total > n) return refuse(h, INVALID, "a tag reaches past the file");
        slot->present = true, slot->kind = kind, slot->count = count, slot->where = (size_t)where;
    }
    auto item = [&](const Value &v, uint32_t k) -> uint32_t { return v.kind == 3 ? u16(v.where + 2 * (size_t)k) : u32(v.where + 4 * (size_t)k); };
    auto scalar_of = [&](uint32_t tag, uint32_t otherwise) -> uint32_t {
        for (int i = 0; i < 9; i++)
            if (SCALARS[i] == tag && scalars[i].present) return item(scalars[i], 0);
        return otherwise;
    };
    auto has = [&](uint32_t tag) -> bool {
        for (int i = 0; i < 9; i++)
            if (SCALARS[i] == tag) return scalars[i].present;
        return false;
    };
    const Value &bits = arrays[0], &offsets = arrays[1], &counts = arrays[2], &formats = arrays[4];
    if (tiles && !extended) return refuse(h, UNSUPPORTED, "tiles");
    if (tiles && (offsets.present || counts.present)) return refuse(h, INVALID, "strip tags and tile tags");
    if (!has(256) || !has(257) || !has(262) || !(tiles ? tile[0].present && tile[1].present && tile[2].present : offsets.present))
        return refuse(h, INVALID, "a required tag is missing");
    const uint32_t width = scalar_of(256, 0), height = scalar_of(257, 0);
    if (width == 0 || height == 0) return refuse(h, INVALID, "width or height 0");
    if (width >= 65536 || height >= 65536) return refuse(h, UNSUPPORTED, "a dimension of 65536 or more");
    const uint32_t spp = scalar_of(277, 1);
    if (spp == 0) return refuse(h, INVALID, "no samples");
    if (spp == 2 || spp > 4) return refuse(h, UNSUPPORTED, "2 samples or more than 4");
    uint32_t bps = 1;
    if (bits.present) {
        if (bits.count != 1 && bits.count != spp) return refuse(h, INVALID, "BitsPerSample count");
        bps = item(bits, 0);
        for (uint32_t k = 1; k < bits.count; k++)
            if (item(bits, k) != bps) return refuse(h, UNSUPPORTED, "bits per sample");
    }
    if (bps != 8 && bps != 16) return refuse(h, UNSUPPORTED, "bits per sample");
    if (formats.present)
        for (uint32_t k = 0; k < formats.count; k++)
            if (item(formats, k) != 1) return refuse(h, UNSUPPORTED, "sample format");
    const uint32_t fill = scalar_of(266, 1);
    if (fill == 2) return refuse(h, UNSUPPORTED, "FillOrder 2");
    if (fill != 1) return refuse(h, INVALID, "FillOrder");
    const uint32_t planar = scalar_of(284, 1);
    if (planar == 2) return refuse(h, UNSUPPORTED, "PlanarConfiguration 2");
    if (planar != 1) return refuse(h, INVALID, "PlanarConfiguration");
    const uint32_t compression = scalar_of(259, 1);
    const bool deflate = extended && (compression == COMPRESSION_DEFLATE || compression == COMPRESSION_DEFLATE_OLD);
    if (compression != COMPRESSION_NONE && compression != COMPRESSION_LZW && compression != COMPRESSION_PACKBITS && !deflate)
        return refuse(h, UNSUPPORTED, "compression");
    const uint32_t predictor = scalar_of(317, 1);
    if (predictor == 3) return refuse(h, UNSUPPORTED, "Predictor 3");
    if (predictor != 1 && predictor != 2) return refuse(h, INVALID, "Predictor");
    const uint32_t photometric = scalar_of(262, 0);
    if (!((spp == 1 && photometric <= 1) || (spp >= 3 && photometric == 2))) return refuse(h, UNSUPPORTED, "photometric interpretation and samples");
    const uint64_t row_bytes = (uint64_t)width * spp * (bps / 8);
    // the streams: strips of rps rows of the image's width, or tiles - strips of TileLength rows of TileWidth pixels, the edge
    // tiles whole - in rows of tiles_across
    uint32_t rps, nstrips, tile_w = 0, tile_l = 0, across = 0, down = 0;
    uint64_t stream_row_bytes = row_bytes;
    const Value &stream_offsets = tiles ? tile[2] : offsets, &stream_counts = tiles ? tile[3] : counts;
    if (tiles) {
        tile_w = item(tile[0], 0), tile_l = item(tile[1], 0);
        if (tile_w == 0 || tile_l == 0 || tile_w % 16 || tile_l % 16) return refuse(h, UNSUPPORTED, "a tile width or length that is no multiple of 16");
        // (the tags are LONGs: a row and a length are bounded before anything is multiplied, so that no product below wraps)
        stream_row_bytes = (uint64_t)tile_w * spp * (bps / 8);
        if (stream_row_bytes >= (1ull << 31) || tile_l >= (1u << 31)) return refuse(h, UNSUPPORTED, "a strip of 2^31 bytes or more");
        across = (width + tile_w - 1) / tile_w, down = (height + tile_l - 1) / tile_l;
        rps = tile_l, nstrips = across * down;
    } else {
        rps = scalar_of(278, 0xFFFFFFFFu);
        if (rps == 0) return refuse(h, INVALID, "RowsPerStrip 0");
        if (rps > height) rps = height;
        nstrips = (height + rps - 1) / rps;
    }
    if ((uint64_t)rps * stream_row_bytes >= (1ull << 31)) return refuse(h, UNSUPPORTED, "a strip of 2^31 bytes or more");
    if (stream_offsets.count != nstrips) return refuse(h, INVALID, "StripOffsets count");
    if (!stream_counts.present && compression != COMPRESSION_NONE) return refuse(h, INVALID, "StripByteCounts is missing");
    if (stream_counts.present && stream_counts.count != nstrips) return refuse(h, INVALID, "StripByteCounts count");
    h.strips.resize(nstrips);
    uint64_t compressed = 0;
    for (uint32_t s = 0; s < nstrips; s++) {
        Strip &strip = h.strips[s];
        if (tiles) strip.rows = rps, strip.x = s % across * tile_w, strip.y = s / across * tile_l;
        else strip.rows = rps < height - s * rps ? rps : height - s * rps, strip.y = s * rps;
        strip.row_bytes = (uint32_t)stream_row_bytes;
        strip.offset = item(stream_offsets, s);
        const uint64_t need = strip.rows * stream_row_bytes, count = stream_counts.present ? item(stream_counts, s) : need;
        if (count >= (1ull << 31)) return refuse(h, UNSUPPORTED, "a strip of 2^31 bytes or more");
        if ((uint64_t)strip.offset + count > n) return refuse(h, INVALID, "a strip reaches past the file");
        if (compression == COMPRESSION_NONE && count < need) return refuse(h, INVALID, "a strip shorter than its rows");
        if (compression == COMPRESSION_LZW && count >= 2 && data[strip.offset] == 0 && (data[strip.offset + 1] & 1u))
            return refuse(h, UNSUPPORTED, "old-style LZW");
        strip.count = (uint32_t)count;
        compressed += count;
    }
    // every Deflate stream is copied to an aligned place of its own: streams that share bytes could ask for any multiple of the file
    if (deflate && compressed > n) return refuse(h, UNSUPPORTED, "Deflate: streams that overlap");
    // inflate's source indices are 32-bit, as the PNG path's
    if (deflate && (uint64_t)nstrips * rps * stream_row_bytes >= (1ull << 31)) return refuse(h, UNSUPPORTED, "Deflate: 2^31 decompressed bytes or more");
    h.tile_width = tile_w, h.tile_length = tile_l, h.tiles_across = across, h.tiles_down = down;
    h.width = width, h.height = height, h.samples = spp, h.bits = bps, h.compression = compression, h.photometric = photometric;
    h.predictor = predictor, h.rows_per_strip = rps, h.row_bytes = row_bytes;

    // the SEM block: 34683 before 34682; a type that is not ASCII, or a value past the file, is no block
    const Value &block = sem[1].present ? sem[1] : sem[0];
    if (block.present && block.kind == 2) {
        const uint64_t where = block.count > 4 ? u32(block.where) : block.where;
        if (where + block.count <= n) {
            h.sem = true;
            sem_block(data + where, block.count, h);
        }
    }
    // FocalLengthIn35mmFilm: IFD0 -> 34665 (LONG) -> 0xA405 (SHORT or LONG), count 1; anything else is none
    auto find = [&](uint64_t dir, uint32_t tag, bool short_too, uint32_t &value) -> bool {
        if (dir + 2 > n) return false;
        const uint32_t count = u16((size_t)dir);
        if (dir + 2 + 12ull * count > n) return false;
        for (uint32_t k = 0; k < count; k++) {
            const size_t at = (size_t)dir + 2 + 12 * (size_t)k;
            if (u16(at) != tag) continue;
            const uint32_t kind = u16(at + 2);
            if (u32(at + 4) != 1 || !(kind == 4 || (short_too && kind == 3))) return false;
            value = kind == 3 ? u16(at + 8) : u32(at + 8);
            return true;
        }
        return false;
    };
    uint32_t sub = 0, focal = 0;
    if (find(ifd, 34665, false, sub) && find(sub, 0xA405, true, focal)) h.focal_length_35mm = focal;
    return OK;
}

} // namespace tiff_common
