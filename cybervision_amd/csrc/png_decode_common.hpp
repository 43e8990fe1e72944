// png_decode_common.hpp — the host side of cvhip_png_decode (png_decode_kernels.hip) as plain C++ that also
// compiles without HIP (tests/cpp/png_in_host.cpp runs it on the CPU under sanitizers): the chunk walk with the CRC of every
// chunk that is not an IDAT (those are checked on the device, where their bytes go anyway), IHDR, PLTE, tRNS, the eXIf
// chunk's FocalLengthIn35mmFilm (the EXIF walk of jpeg_common.hpp over the chunk, a bare TIFF structure) and the table of
// the IDAT payloads.  The SEM text tags are not read from a PNG file: no microscope writes one.  tests/ref_png_in.py is the
// definition; every read is bounded by the file's size.  parse(.., adam7 = true) is the superset behind cvhip_png_ext_decode
// (tests/ref_png_adam7.py, tests/cpp/png_adam7_host.cpp): interlace method 1 is accepted, and the header
// holds the table of the seven reduced images the stream carries one behind the other.
#pragma once

#include <cstddef>
#include <cstdint>
#include <cstring>
#include <vector>

#include "jpeg_common.hpp"
#include "png_common.hpp"

namespace png_decode_common {

constexpr int OK = 0, INVALID = -1, UNSUPPORTED = -3; // (CVHIP_OK, CVHIP_ERR_INVALID, CVHIP_ERR_UNSUPPORTED)
constexpr uint32_t FLAG_PLTE = 1, FLAG_TRNS = 2;
constexpr uint32_t MAX_DIMENSION = 65536;        // a width or height from here on is not built
constexpr uint64_t MAX_FILTERED = 1ull << 31;    // nor a filtered image (height x (1 + row bytes), or the passes' sum) from here on
constexpr uint32_t ADAM7_PASSES = 7;
constexpr uint32_t ADAM7_X0[7] = {0, 4, 0, 2, 0, 1, 0}, ADAM7_Y0[7] = {0, 0, 4, 0, 2, 0, 1};
constexpr uint32_t ADAM7_LOG_DX[7] = {3, 3, 2, 2, 1, 1, 0}, ADAM7_LOG_DY[7] = {3, 3, 3, 2, 2, 1, 1};
// The bits of a subsequence of the self-synchronising inflate, as jpeg_common::SUBSEQ_BITS: above the 48 bits of the longest
// token (15 + 5 + 15 + 13), so an exit state lies in the next subsequence, and a multiple of the 32-bit words the readers load.
constexpr uint32_t SUBSEQ_BITS = 1024;

struct Idat {
    uint64_t offset; // of the payload in the file
    uint32_t length, crc;
};
// A reduced image of an Adam7 file (or the whole image of any other, at (0, 0) with steps of one): `height` rows of a filter
// byte and `row_bytes` bytes; sample (px, py) is pixel (x0 + (px << log_dx), y0 + (py << log_dy)).  An empty pass has
// width = height = row_bytes = 0 and no bytes at all; first_row and offset are then those of the next pass.
struct Pass {
    uint32_t width = 0, height = 0;
    uint64_t row_bytes = 0;
    uint32_t first_row = 0; // in the concatenation of all passes' rows
    uint64_t offset = 0;    // of its first filter byte in the filtered image
    uint32_t x0 = 0, y0 = 0, log_dx = 0, log_dy = 0;
};
struct Header {
    uint32_t width = 0, height = 0, colour = 0, depth = 0, interlace = 0;
    Pass pass[ADAM7_PASSES];      // interlace 0: entry 0 alone
    uint32_t pass_entries = 0;    // 1 or 7
    uint32_t passes = 0;          // the non-empty ones
    uint32_t pass_rows = 0;       // of all passes
    uint64_t filtered = 0;        // the bytes the stream must inflate to: the passes' rows with their filter bytes
    uint32_t channels = 0, bpp = 0; // samples of a pixel; the filters' byte distance max(1, channels * depth / 8)
    uint64_t row_bytes = 0;         // of a row without its filter byte
    uint32_t focal_length_35mm = 0; // 0 = none
    uint32_t flags = 0;
    uint32_t palette_entries = 0;
    uint8_t palette[768] = {0};
    std::vector<Idat> idat;
    uint64_t idat_bytes = 0;
    const char *error = "";
};

inline int refuse(Header &h, int code, const char *why)
{
    h.error = why;
    return code;
}
inline uint32_t be32(const uint8_t *p) { return (uint32_t)p[0] << 24 | (uint32_t)p[1] << 16 | (uint32_t)p[2] << 8 | p[3]; }

// The chunk walk of data[0 .. n) up to IEND -> OK, INVALID or UNSUPPORTED (h.error says why).  adam7: interlace method 1 is
// accepted too.
inline int parse(const uint8_t *data, size_t n, Header &h, bool adam7 = false)
{
    static const uint8_t SIGNATURE[8] = {0x89, 'P', 'N', 'G', 0x0D, 0x0A, 0x1A, 0x0A};
    if (n < 8 || std::memcmp(data, SIGNATURE, 8) != 0) return refuse(h, INVALID, "no PNG signature");
    size_t at = 8;
    bool first = true, have_plte = false, in_idat = false;
    for (;;) {
        if (n - at < 12) return refuse(h, INVALID, at == n ? "no IEND" : "a chunk runs past the file");
        const uint32_t length = be32(data + at);
        if (length > n - at - 12) return refuse(h, INVALID, "a chunk runs past the file");
        const uint8_t *type = data + at + 4, *body = data + at + 8;
        const auto is = [&](const char *name) { return std::memcmp(type, name, 4) == 0; };
        if (first && (!is("IHDR") || length != 13)) return refuse(h, INVALID, "the first chunk is not a 13-byte IHDR");
        if (!is("IDAT") && png_common::crc32(type, (size_t)length + 4) != be32(body + length)) return refuse(h, INVALID, "a chunk's CRC");
        if (is("IHDR")) {
            if (!first) return refuse(h, INVALID, "a second IHDR");
            h.width = be32(body), h.height = be32(body + 4), h.depth = body[8], h.colour = body[9], h.interlace = body[12];
            if (h.width == 0 || h.height == 0) return refuse(h, INVALID, "a zero dimension");
            const uint32_t d = h.depth;
            const bool low = d == 1 || d == 2 || d == 4, deep = d == 8 || d == 16;
            const bool legal = h.colour == 0 ? low || deep : h.colour == 3 ? low || d == 8 : (h.colour == 2 || h.colour == 4 || h.colour == 6) && deep;
            if (!legal) return refuse(h, INVALID, "an illegal colour type / bit depth pair");
            if (body[10] != 0 || body[11] != 0) return refuse(h, INVALID, "a compression or filter method other than 0");
            if (h.interlace > 1) return refuse(h, INVALID, "an interlace method above 1");
            if (h.interlace == 1 && !adam7) return refuse(h, UNSUPPORTED, "Adam7 interlacing");
            if (h.width >= MAX_DIMENSION || h.height >= MAX_DIMENSION) return refuse(h, UNSUPPORTED, "a dimension of 65 536 or more");
            h.channels = h.colour == 2 ? 3 : h.colour == 4 ? 2 : h.colour == 6 ? 4 : 1;
            const uint32_t pixel_bits = h.channels * h.depth;
            h.bpp = pixel_bits < 8 ? 1 : pixel_bits / 8;
            h.row_bytes = ((uint64_t)h.width * pixel_bits + 7) / 8;
            if ((h.row_bytes + 1) * h.height >= MAX_FILTERED) return refuse(h, UNSUPPORTED, "a filtered image of 2^31 bytes or more");
            // the pass table: both dimensions are below 2^16 and a pixel has 64 bits at most, so a row stays below 2^20 bytes,
            // a pass below 2^36 and the sum of seven below 2^39
            h.pass_entries = h.interlace ? ADAM7_PASSES : 1u;
            for (uint32_t p = 0; p < h.pass_entries; p++) {
                Pass &e = h.pass[p];
                if (h.interlace) e.x0 = ADAM7_X0[p], e.y0 = ADAM7_Y0[p], e.log_dx = ADAM7_LOG_DX[p], e.log_dy = ADAM7_LOG_DY[p];
                const uint32_t pw = h.width > e.x0 ? (h.width - e.x0 + (1u << e.log_dx) - 1u) >> e.log_dx : 0u;
                const uint32_t ph = h.height > e.y0 ? (h.height - e.y0 + (1u << e.log_dy) - 1u) >> e.log_dy : 0u;
                e.first_row = h.pass_rows, e.offset = h.filtered;
                if (pw == 0 || ph == 0) continue; // no bytes at all, not even filter bytes
                e.width = pw, e.height = ph, e.row_bytes = ((uint64_t)pw * pixel_bits + 7) / 8;
                h.passes++, h.pass_rows += ph, h.filtered += (e.row_bytes + 1) * ph;
            }
            if (h.filtered >= MAX_FILTERED) return refuse(h, UNSUPPORTED, "passes of 2^31 bytes or more");
        } else if (is("PLTE")) {
            if (have_plte || !h.idat.empty()) return refuse(h, INVALID, "a PLTE out of place");
            if (length == 0 || length % 3 != 0 || length > 768) return refuse(h, INVALID, "a PLTE whose length is not 3 .. 768 in threes");
            std::memcpy(h.palette, body, length);
            h.palette_entries = length / 3, h.flags |= FLAG_PLTE, have_plte = true;
        } else if (is("IDAT")) {
            if (!h.idat.empty() && !in_idat) return refuse(h, INVALID, "IDAT chunks that are not consecutive");
            h.idat.push_back({(uint64_t)(body - data), length, be32(body + length)});
            h.idat_bytes += length;
        } else if (is("IEND")) {
            if (h.idat.empty()) return refuse(h, INVALID, "no IDAT");
            if (h.colour == 3 && !have_plte) return refuse(h, INVALID, "colour type 3 without PLTE");
            return OK;
        } else if (is("tRNS")) {
            h.flags |= FLAG_TRNS;
        } else if (is("eXIf")) {
            if (h.focal_length_35mm == 0) h.focal_length_35mm = jpeg_common::exif_focal_length_35mm(body, length);
        } else if ((type[0] & 0x20u) == 0) {
            return refuse(h, INVALID, "an unknown critical chunk");
        }
        in_idat = is("IDAT");
        first = false;
        at += (size_t)length + 12;
    }
}

} // namespace png_decode_common
