// jpeg_common.hpp — the host side of cvhip_jpeg_decode (jpeg_kernels.hip) as plain C++ that also compiles
// without HIP (tests/cpp/jpeg_host.cpp runs it on the CPU under sanitizers): the marker walk up to the scan, the quantisation
// and Huffman tables (a 16-bit-prefix lookup per table), the scan's byte range, and EXIF's FocalLengthIn35mmFilm.
// The walk itself - the marker loop, the table and frame segments, the search for a scan's end - is walk() below, which
// jpeg_prog_common.hpp drives over a whole progressive file; a parser adds what it does with a scan.
// tests/ref_jpeg.py is the definition; every read is bounded by the file's size.
#pragma once

#include <cstddef>
#include <cstdint>
#include <cstring>

namespace jpeg_common {

constexpr int OK = 0, INVALID = -1, UNSUPPORTED = -3; // (CVHIP_OK, CVHIP_ERR_INVALID, CVHIP_ERR_UNSUPPORTED)
constexpr int STOP = 1;                               // of a scan handler: the walk ends here, accepted
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
// what the walk has gathered when it meets a scan: the frame and the tables in force
struct Walk {
    bool have_frame = false;
    uint32_t width = 0, height = 0, components = 0, hmax = 0, vmax = 0, mcus_x = 0, mcus_y = 0;
    uint32_t restart = 0;           // MCUs per restart interval, 0 = none
    uint32_t focal_length_35mm = 0; // 0 = none
    int adobe = -1;                 // the transform of an APP14 "Adobe" segment, -1 = none
    bool may_end = false;           // EOI or the file's end may end the walk: a scan handler that carries on sets it
    Component comp[3];
    bool have_quant[4] = {false, false, false, false};
    uint16_t quant[4][64]; // natural order
    HuffmanTable huff[2][4];
    const char *error = "";
};
struct Header : Walk {
    uint64_t scan_begin = 0, scan_end = 0;
};
// what a parser's walk differs in, beside what it does with a scan
struct Dialect {
    uint32_t sof;             // the frame it takes
    const char *other_frame;  // why it refuses the others
    const char *stray_marker; // why it refuses EOI, SOI, RSTn or 00 where a segment should begin
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

inline int refuse(Walk &w, int code, const char *why)
{
    w.error = why;
    return code;
}

inline uint32_t blocks_per_mcu(uint32_t components, uint32_t hmax, uint32_t vmax) { return components == 1 ? 1u : hmax * vmax + 2u; }
inline uint32_t blocks_per_mcu(const Walk &w) { return blocks_per_mcu(w.components, w.hmax, w.vmax); }
// the MCUs across (or down) `extent` pixels where the largest sampling factor is `factor`
inline uint32_t mcus_over(uint32_t extent, uint32_t factor) { return (extent + 8 * factor - 1) / (8 * factor); }

// ---- the segments ------------------------------------------------------------------------------------------------------------
inline int read_dqt(Walk &w, const uint8_t *seg, size_t len)
{
    for (size_t k = 0; k < len;) {
        const uint32_t pq = seg[k] >> 4, tq = seg[k] & 15u;
        if (pq > 1 || tq > 3 || k + 1 + 64 * (pq + 1) > len) return refuse(w, INVALID, "DQT");
        for (int i = 0; i < 64; i++) w.quant[tq][ZIGZAG[i]] = pq ? (uint16_t)(seg[k + 1 + 2 * i] << 8 | seg[k + 2 + 2 * i]) : seg[k + 1 + i];
        w.have_quant[tq] = true;
        k += 1 + 64 * (pq + 1);
    }
    return OK;
}

// (a table replaces its slot whole: the symbols behind its own are none of the table before's)
inline int read_dht(Walk &w, const uint8_t *seg, size_t len)
{
    for (size_t k = 0; k < len;) {
        if (k + 17 > len) return refuse(w, INVALID, "DHT");
        const uint32_t tc = seg[k] >> 4, th = seg[k] & 15u;
        uint32_t total = 0;
        for (int i = 0; i < 16; i++) total += seg[k + 1 + i];
        if (tc > 1 || th > 3 || total > 256 || k + 17 + total > len) return refuse(w, INVALID, "DHT");
        uint32_t code = 0, s = 0;
        for (int bits = 1; bits <= 16; bits++) {
            for (uint32_t c = 0; c < seg[k + bits]; c++, code++, s++) {
                if (code >= (1u << bits)) return refuse(w, INVALID, "DHT: the code space is overfull");
                if (tc == 0 && seg[k + 17 + s] > 15) return refuse(w, INVALID, "DHT: a DC category above 15");
            }
            code <<= 1;
        }
        HuffmanTable &t = w.huff[tc][th];
        t = HuffmanTable();
        t.present = true, t.total = total;
        std::memcpy(t.counts, seg + k + 1, 16);
        std::memcpy(t.symbols, seg + k + 17, total);
        k += 17 + total;
    }
    return OK;
}

// the frame: 8 bits, one component or three with 1x1, 2x1 or 2x2 luma over 1x1 chroma; and the MCU geometry
inline int read_sof(Walk &w, const uint8_t *seg, size_t len)
{
    if (w.have_frame) return refuse(w, INVALID, "two frames");
    if (len < 6) return refuse(w, INVALID, "SOF");
    const uint32_t p = seg[0], hh = (uint32_t)seg[1] << 8 | seg[2], ww = (uint32_t)seg[3] << 8 | seg[4], nf = seg[5];
    if (len != 6 + 3 * (size_t)nf) return refuse(w, INVALID, "SOF");
    if (p == 12) return refuse(w, UNSUPPORTED, "12-bit samples");
    if (p != 8) return refuse(w, INVALID, "precision");
    if (hh == 0) return refuse(w, UNSUPPORTED, "DNL");
    if (ww == 0) return refuse(w, INVALID, "width 0");
    if (nf == 2 || nf == 4) return refuse(w, UNSUPPORTED, "2 or 4 components");
    if (nf != 1 && nf != 3) return refuse(w, INVALID, "components");
    for (uint32_t c = 0; c < nf; c++) {
        Component &comp = w.comp[c];
        comp.id = seg[6 + 3 * c], comp.h = seg[7 + 3 * c] >> 4, comp.v = seg[7 + 3 * c] & 15u, comp.tq = seg[8 + 3 * c];
        if (comp.h < 1 || comp.h > 4 || comp.v < 1 || comp.v > 4 || comp.tq > 3) return refuse(w, INVALID, "SOF");
    }
    if (nf == 1)
        w.comp[0].h = w.comp[0].v = 1; // (a single component is never interleaved: its factors do not count)
    else {
        const Component &y = w.comp[0];
        const bool luma_ok = (y.h == 1 && y.v == 1) || (y.h == 2 && y.v == 1) || (y.h == 2 && y.v == 2);
        if (!luma_ok || w.comp[1].h != 1 || w.comp[1].v != 1 || w.comp[2].h != 1 || w.comp[2].v != 1)
            return refuse(w, UNSUPPORTED, "sampling factors other than 1x1, 2x1 or 2x2 luma over 1x1 chroma");
    }
    w.width = ww, w.height = hh, w.components = nf, w.hmax = w.comp[0].h, w.vmax = w.comp[0].v;
    w.mcus_x = mcus_over(ww, w.hmax), w.mcus_y = mcus_over(hh, w.vmax);
    w.have_frame = true;
    return OK;
}

// the first FF at or behind `start` that is followed by neither 00, FF nor RSTn, or the file's end: where a scan's bytes end
inline size_t scan_end(const uint8_t *data, size_t n, size_t start)
{
    size_t end = start;
    while (end < n) {
        const void *ff = std::memchr(data + end, 0xFF, n - end);
        if (!ff || (size_t)((const uint8_t *)ff - data) + 1 >= n) return n;
        end = (size_t)((const uint8_t *)ff - data);
        const uint32_t nx = data[end + 1];
        if (nx == 0 || nx == 0xFF || (nx >= 0xD0 && nx <= 0xD7)) {
            end += nx == 0xFF ? 1 : 2;
            continue;
        }
        break;
    }
    return end;
}

// The marker walk of data[0 .. n): the next marker, its segment's length, the segment -> OK, INVALID or UNSUPPORTED (w.error
// says why).  on_sos(seg, len, at) takes a scan's header, `at` at the first byte behind it: it returns STOP (the walk ends,
// accepted), a refusal, or OK with `at` where the walk carries on.
template <typename Sos> inline int walk(const uint8_t *data, size_t n, Walk &w, const Dialect &d, Sos &&on_sos)
{
    if (n < 4 || data[0] != 0xFF || data[1] != 0xD8) return refuse(w, INVALID, "no SOI");
    size_t at = 2;
    for (;;) {
        if (at >= n && w.may_end) return OK; // (no EOI: the file's end is the end)
        if (at >= n || data[at] != 0xFF) return refuse(w, INVALID, "no marker");
        while (at < n && data[at] == 0xFF) at++;
        if (at >= n) return w.may_end ? OK : refuse(w, INVALID, "the file ends in a marker");
        const uint32_t m = data[at++];
        if (m == 0xD9 && w.may_end) return OK;
        if (m == 0xD9 || m == 0xD8 || (m >= 0xD0 && m <= 0xD7) || m == 0x00) return refuse(w, INVALID, d.stray_marker);
        if (m == 0x01) continue;
        if (at + 2 > n) return refuse(w, INVALID, "truncated segment");
        const size_t length = (size_t)data[at] << 8 | data[at + 1];
        if (length < 2 || at + length > n) return refuse(w, INVALID, "truncated segment");
        const uint8_t *seg = data + at + 2;
        const size_t len = length - 2;
        at += length;
        int rc = OK;
        if (m == 0xDB) rc = read_dqt(w, seg, len);
        else if (m == 0xC4) rc = read_dht(w, seg, len);
        else if (m == 0xDD) {
            if (len != 2) return refuse(w, INVALID, "DRI");
            w.restart = (uint32_t)seg[0] << 8 | seg[1];
        } else if (m == d.sof) rc = read_sof(w, seg, len);
        else if (m >= 0xC0 && m <= 0xCF && m != 0xC8 && m != 0xCC) return refuse(w, UNSUPPORTED, d.other_frame);
        else if (m == 0xCC) return refuse(w, UNSUPPORTED, "arithmetic conditioning");
        else if (m == 0xDC) return refuse(w, UNSUPPORTED, "DNL");
        else if (m == 0xE1 && len >= 6 && std::memcmp(seg, "Exif\0\0", 6) == 0 && w.focal_length_35mm == 0)
            w.focal_length_35mm = exif_focal_length_35mm(seg + 6, len - 6);
        else if (m == 0xEE && len >= 12 && std::memcmp(seg, "Adobe", 5) == 0) w.adobe = seg[11];
        else if (m == 0xDA) rc = on_sos(seg, len, at);
        if (rc == STOP) return OK;
        if (rc != OK) return rc;
    }
}

// The marker walk of data[0 .. n) up to and including the one scan -> OK, INVALID or UNSUPPORTED (h.error says why).
inline int parse(const uint8_t *data, size_t n, Header &h)
{
    const Dialect baseline{0xC0, "a frame that is not baseline (SOF0)", "a marker that cannot stand before the scan"};
    return walk(data, n, h, baseline, [&](const uint8_t *seg, size_t len, size_t &at) {
        if (!h.have_frame) return refuse(h, INVALID, "a scan before the frame");
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
        if (h.components == 3 && h.adobe >= 0 && h.adobe != 1) return refuse(h, UNSUPPORTED, "an Adobe transform that is not YCbCr");
        h.scan_begin = at, h.scan_end = scan_end(data, n, at);
        for (size_t k = h.scan_end; k + 1 < n;) { // what follows the scan: a second scan or DNL is not built
            if (data[k] != 0xFF) break;
            while (k < n && data[k] == 0xFF) k++;
            if (k >= n || data[k] == 0xD9) break;
            if (data[k] == 0xDC) return refuse(h, UNSUPPORTED, "DNL");
            if (data[k] == 0xDA) return refuse(h, UNSUPPORTED, "more than one scan");
            if (k + 2 >= n) break;
            k += 1 + ((size_t)data[k + 1] << 8 | data[k + 2]);
        }
        return STOP;
    });
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

// restart intervals of the scan
inline uint64_t segments(const Header &h)
{
    const uint64_t mcus = (uint64_t)h.mcus_x * h.mcus_y;
    return h.restart ? (mcus + h.restart - 1) / h.restart : 1;
}

} // namespace jpeg_common
