// jpeg_common.hpp — the host side of cvhip_jpeg_decode (jpeg_kernels.hip) as plain C++ that also compiles
// without HIP (tests/cpp/jpeg_host.cpp runs it on the CPU under sanitizers): the marker walk up to the scan, the quantisation
// and Huffman tables (a 16-bit-prefix lookup per table), the scan's byte range, and EXIF's FocalLengthIn35mmFilm.
// tests/ref_jpeg.py is the definition; every read is bounded by the file's size.
#pragma once

#include <cstddef>
#include <cstdint>
#include <cstring>

namespace jpeg_common {

constexpr int OK = 0, INVALID = -1, UNSUPPORTED = -3; // (CVHIP_OK, CVHIP_ERR_INVALID, CVHIP_ERR_UNSUPPORTED)
// The bits of a subsequence of the self-synchronising entropy decode.  A lane decodes one: at ~5 bits a symbol that is ~200
// symbols of serial work, and a 2048 x 2048 photograph of ~1 MB still gives ~8000 lanes.  Shorter subsequences give more
// lanes but more boundary symbols decoded twice and more states to settle; 1024 is also a multiple of the 32-bit words the
// readers load, and above the 31 bits of the longest symbol, so an exit state lies in the next subsequence.
constexpr uint32_t SUBSEQ_BITS = 1024;
constexpr uint32_t LUT_ENTRIES = 65536; // per Huffman table: entry[the next 16 bits] = code length << 8 | symbol, 0 = no such code

struct Component {
    uint8_t id = 0, h = 0, v = 0, tq = 0, td = 0, ta = 0;
};
struct HuffmanTable {
    bool present = false;
    uint8_t counts[16] = {0};
    uint8_t symbols[256] = {0};
    uint32_t total = 0;
};
struct Header {
    uint32_t width = 0, height = 0, components = 0, hmax = 0, vmax = 0, mcus_x = 0, mcus_y = 0;
    uint32_t restart = 0;           // MCUs per restart interval, 0 = none
    uint32_t focal_length_35mm = 0; // 0 = none
    uint64_t scan_begin = 0, scan_end = 0;
    Component comp[3];
    bool have_quant[4] = {false, false, false, false};
    uint16_t quant[4][64]; // natural order
    HuffmanTable huff[2][4];
    const char *error = "";
};

constexpr uint8_t ZIGZAG[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                                41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                                30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

// FocalLengthIn35mmFilm of the TIFF block behind "Exif\0\0": IFD0 -> 0x8769 -> 0xA405 (SHORT or LONG); 0 = none
inline uint32_t exif_focal_length_35mm(const uint8_t *tiff, size_t n)
{
    if (n < 8) return 0;
    const bool little = tiff[0] == 'I' && tiff[1] == 'I', big = tiff[0] == 'M' && tiff[1] == 'M';
    if (!little && !big) return 0;
    auto u16 = [&](size_t at) -> uint32_t { return little ? tiff[at] | tiff[at + 1] << 8 : tiff[at] << 8 | tiff[at + 1]; };
    auto u32 = [&](size_t at) -> uint32_t { return little ? u16(at) | u16(at + 2) << 16 : u16(at) << 16 | u16(at + 2); };
    if (u16(2) != 42) return 0;
    // the value of `tag` in the IFD at `ifd` when its type is LONG, or SHORT where allowed, and its count 1
    auto find = [&](uint64_t ifd, uint32_t tag, bool short_too, uint32_t &value) -> bool {
        if (ifd + 2 > n) return false;
        const uint32_t count = u16((size_t)ifd);
        for (uint32_t k = 0; k < count; k++) {
            const uint64_t at = ifd + 2 + 12ull * k;
            if (at + 12 > n) return false;
            if (u16((size_t)at) != tag) continue;
            const uint32_t kind = u16((size_t)at + 2);
            if (u32((size_t)at + 4) != 1 || !(kind == 4 || (short_too && kind == 3))) return false;
            value = kind == 3 ? u16((size_t)at + 8) : u32((size_t)at + 8);
            return true;
        }
        return false;
    };
    uint32_t sub = 0, focal = 0;
    if (!find(u32(4), 0x8769, false, sub)) return 0;
    return find(sub, 0xA405, true, focal) ? focal : 0;
}

inline int refuse(Header &h, int code, const char *why)
{
    h.error = why;
    return code;
}

// The marker walk of data[0 .. n) up to and including the one scan -> OK, INVALID or UNSUPPORTED (h.error says why).
inline int parse(const uint8_t *data, size_t n, Header &h)
{
    if (n < 4 || data[0] != 0xFF || data[1] != 0xD8) return refuse(h, INVALID, "no SOI");
    size_t at = 2;
    bool have_frame = false;
    int adobe = -1;
    for (;;) {
        if (at >= n || data[at] != 0xFF) return refuse(h, INVALID, "no marker");
        while (at < n && data[at] == 0xFF) at++;
        if (at >= n) return refuse(h, INVALID, "the file ends in a marker");
        const uint32_t m = data[at++];
        if (m == 0xD9 || m == 0xD8 || (m >= 0xD0 && m <= 0xD7) || m == 0x00) return refuse(h, INVALID, "a marker that cannot stand before the scan");
        if (m == 0x01) continue;
        if (at + 2 > n) return refuse(h, INVALID, "truncated segment");
        const size_t length = (size_t)data[at] << 8 | data[at + 1];
        if (length < 2 || at + length > n) return refuse(h, INVALID, "truncated segment");
        const uint8_t *seg = data + at + 2;
        const size_t len = length - 2;
        if (m == 0xDB) {
            for (size_t k = 0; k < len;) {
                const uint32_t pq = seg[k] >> 4, tq = seg[k] & 15u;
                if (pq > 1 || tq > 3 || k + 1 + 64 * (pq + 1) > len) return refuse(h, INVALID, "DQT");
                for (int i = 0; i < 64; i++)
                    h.quant[tq][ZIGZAG[i]] = pq ? (uint16_t)(seg[k + 1 + 2 * i] << 8 | seg[k + 2 + 2 * i]) : seg[k + 1 + i];
                h.have_quant[tq] = true;
                k += 1 + 64 * (pq + 1);
            }
        } else if (m == 0xC4) {
            for (size_t k = 0; k < len;) {
                if (k + 17 > len) return refuse(h, INVALID, "DHT");
                const uint32_t tc = seg[k] >> 4, th = seg[k] & 15u;
                uint32_t total = 0;
                for (int i = 0; i < 16; i++) total += seg[k + 1 + i];
                if (tc > 1 || th > 3 || total > 256 || k + 17 + total > len) return refuse(h, INVALID, "DHT");
                HuffmanTable &t = h.huff[tc][th];
                uint32_t code = 0, s = 0;
                for (int bits = 1; bits <= 16; bits++) {
                    for (uint32_t c = 0; c < seg[k + bits]; c++, code++, s++) {
                        if (code >= (1u << bits)) return refuse(h, INVALID, "DHT: the code space is overfull");
                        if (tc == 0 && seg[k + 17 + s] > 15) return refuse(h, INVALID, "DHT: a DC category above 15");
                    }
                    code <<= 1;
                }
                t.present = true, t.total = total;
                std::memcpy(t.counts, seg + k + 1, 16);
                std::memcpy(t.symbols, seg + k + 17, total);
                k += 17 + total;
            }
        } else if (m == 0xDD) {
            if (len != 2) return refuse(h, INVALID, "DRI");
            h.restart = (uint32_t)seg[0] << 8 | seg[1];
        } else if (m == 0xC0) {
            if (have_frame) return refuse(h, INVALID, "two frames");
            if (len < 6) return refuse(h, INVALID, "SOF");
            const uint32_t p = seg[0], hh = (uint32_t)seg[1] << 8 | seg[2], w = (uint32_t)seg[3] << 8 | seg[4], nf = seg[5];
            if (len != 6 + 3 * (size_t)nf) return refuse(h, INVALID, "SOF");
            if (p == 12) return refuse(h, UNSUPPORTED, "12-bit samples");
            if (p != 8) return refuse(h, INVALID, "precision");
            if (hh == 0) return refuse(h, UNSUPPORTED, "DNL");
            if (w == 0) return refuse(h, INVALID, "width 0");
            if (nf == 2 || nf == 4) return refuse(h, UNSUPPORTED, "2 or 4 components");
            if (nf != 1 && nf != 3) return refuse(h, INVALID, "components");
            for (uint32_t c = 0; c < nf; c++) {
                Component &comp = h.comp[c];
                comp.id = seg[6 + 3 * c], comp.h = seg[7 + 3 * c] >> 4, comp.v = seg[7 + 3 * c] & 15u, comp.tq = seg[8 + 3 * c];
                if (comp.h < 1 || comp.h > 4 || comp.v < 1 || comp.v > 4 || comp.tq > 3) return refuse(h, INVALID, "SOF");
            }
            if (nf == 1)
                h.comp[0].h = h.comp[0].v = 1; // (a single component is never interleaved: its factors do not count)
            else {
                const Component &y = h.comp[0];
                const bool luma_ok = (y.h == 1 && y.v == 1) || (y.h == 2 && y.v == 1) || (y.h == 2 && y.v == 2);
                if (!luma_ok || h.comp[1].h != 1 || h.comp[1].v != 1 || h.comp[2].h != 1 || h.comp[2].v != 1)
                    return refuse(h, UNSUPPORTED, "sampling factors other than 1x1, 2x1 or 2x2 luma over 1x1 chroma");
            }
            h.width = w, h.height = hh, h.components = nf;
            have_frame = true;
        } else if (m >= 0xC1 && m <= 0xCF && m != 0xC4 && m != 0xC8 && m != 0xCC) {
            return refuse(h, UNSUPPORTED, "a frame that is not baseline (SOF0)");
        } else if (m == 0xCC) {
            return refuse(h, UNSUPPORTED, "arithmetic conditioning");
        } else if (m == 0xDC) {
            return refuse(h, UNSUPPORTED, "DNL");
        } else if (m == 0xE1 && len >= 6 && std::memcmp(seg, "Exif\0\0", 6) == 0 && h.focal_length_35mm == 0) {
            h.focal_length_35mm = exif_focal_length_35mm(seg + 6, len - 6);
        } else if (m == 0xEE && len >= 12 && std::memcmp(seg, "Adobe", 5) == 0) {
            adobe = seg[11];
        } else if (m == 0xDA) {
            if (!have_frame) return refuse(h, INVALID, "a scan before the frame");
            if (len < 1 || len != 4 + 2 * (size_t)seg[0]) return refuse(h, INVALID, "SOS");
            const uint32_t ns = seg[0];
            if (ns < 1 || ns > 4) return refuse(h, INVALID, "SOS");
            if (ns != h.components) return refuse(h, UNSUPPORTED, "more than one scan");
            for (uint32_t c = 0; c < ns; c++) {
                Component &comp = h.comp[c];
                if (seg[1 + 2 * c] != comp.id) return refuse(h, UNSUPPORTED, "the scan's components are not the frame's in order");
                comp.td = seg[2 + 2 * c] >> 4, comp.ta = seg[2 + 2 * c] & 15u;
                if (comp.td > 3 || comp.ta > 3) return refuse(h, INVALID, "SOS");
                if (!h.huff[0][comp.td].present || !h.huff[1][comp.ta].present || !h.have_quant[comp.tq]) return refuse(h, INVALID, "a missing table");
            }
            if (h.components == 3 && adobe >= 0 && adobe != 1) return refuse(h, UNSUPPORTED, "an Adobe transform that is not YCbCr");
            // the scan ends at the first FF that is followed by neither 00, FF nor RSTn (or at the file's end)
            size_t end = at + length;
            h.scan_begin = end;
            while (end < n) {
                const void *ff = std::memchr(data + end, 0xFF, n - end);
                if (!ff || (size_t)((const uint8_t *)ff - data) + 1 >= n) {
                    end = n;
                    break;
                }
                end = (size_t)((const uint8_t *)ff - data);
                const uint32_t nx = data[end + 1];
                if (nx == 0 || nx == 0xFF || (nx >= 0xD0 && nx <= 0xD7)) {
                    end += nx == 0xFF ? 1 : 2;
                    continue;
                }
                break;
            }
            h.scan_end = end;
            for (size_t k = end; k + 1 < n;) { // what follows the scan: a second scan or DNL is not built
                if (data[k] != 0xFF) break;
                while (k < n && data[k] == 0xFF) k++;
                if (k >= n || data[k] == 0xD9) break;
                if (data[k] == 0xDC) return refuse(h, UNSUPPORTED, "DNL");
                if (data[k] == 0xDA) return refuse(h, UNSUPPORTED, "more than one scan");
                if (k + 2 >= n) break;
                k += 1 + ((size_t)data[k + 1] << 8 | data[k + 2]);
            }
            h.hmax = h.comp[0].h, h.vmax = h.comp[0].v;
            h.mcus_x = (h.width + 8 * h.hmax - 1) / (8 * h.hmax), h.mcus_y = (h.height + 8 * h.vmax - 1) / (8 * h.vmax);
            return OK;
        }
        at += length;
    }
}

// lut[the next 16 bits of the stream] = code length << 8 | symbol, 0 where no code begins so (parse has checked the table)
inline void build_lut(const HuffmanTable &t, uint16_t *lut)
{
    std::memset(lut, 0, LUT_ENTRIES * sizeof(uint16_t));
    uint32_t code = 0, s = 0;
    for (uint32_t bits = 1; bits <= 16; bits++) {
        for (uint32_t c = 0; c < t.counts[bits - 1]; c++, code++, s++) {
            const uint16_t entry = (uint16_t)(bits << 8 | t.symbols[s]);
            uint16_t *p = lut + ((size_t)code << (16 - bits));
            for (uint32_t k = 0; k < (1u << (16 - bits)); k++) p[k] = entry;
        }
        code <<= 1;
    }
}

inline uint32_t blocks_per_mcu(const Header &h) { return h.components == 1 ? 1u : h.hmax * h.vmax + 2u; }
// restart intervals of the scan
inline uint64_t segments(const Header &h)
{
    const uint64_t mcus = (uint64_t)h.mcus_x * h.mcus_y;
    return h.restart ? (mcus + h.restart - 1) / h.restart : 1;
}

} // namespace jpeg_common
