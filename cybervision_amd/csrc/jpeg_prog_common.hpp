// jpeg_prog_common.hpp — the host side of cvhip_jpeg_progressive_decode (jpeg_prog_kernels.hip) as plain C++
// that also compiles without HIP (tests/cpp/jpeg_prog_host.cpp runs it on the CPU under sanitizers): the marker walk over the
// whole file (jpeg_common.hpp's walk(), with this file's handling of a scan), the scan list (components, Ss, Se, Ah, Al, byte range, restart interval, the Huffman tables in force), the
// progression checks with a ledger of the Al every coefficient was last sent with, one 16-bit-prefix lookup per distinct table
// a scan uses, and the launch order of the scans.  The device cuts the scans at their RSTn markers and decodes them; for the
// CPU program that checks the walk, parse(.., cut = true) cuts them on the host too and decode_interval is the sequential
// entropy decode of one restart interval of one scan of any kind (its bit reader is also the device's in the AC refinement).
// tests/ref_jpeg_prog.py is the definition; every read is bounded by the file's size.
#pragma once

#include <vector>

#include "jpeg_common.hpp"

#if defined(__HIPCC__)
#define JPEG_PROG_HD __host__ __device__
#else
#define JPEG_PROG_HD
#endif

namespace jpeg_prog {

namespace jc = jpeg_common;
using jc::INVALID;
using jc::OK;
using jc::UNSUPPORTED;

constexpr uint32_t MAX_SCANS = 256;
constexpr uint32_t NO_LUT = 0xFFFFFFFFu;
constexpr uint32_t ERR_RST = 1, ERR_CODE = 2, ERR_RUN = 4, ERR_DATA = 8, ERR_REFINE = 16;
// what a decode met, beside the error bits
constexpr uint32_t MET_EOB_RUN = 0, MET_ZRL_IN_REFINEMENT = 1, MET_NEW_AT_SE = 2, MET_CORRECTIONS_IN_RUN = 3, METS = 4;

// the frame as the kernels take it (DESIGN.md 4.16's block store: MCU by MCU, the luma blocks first)
struct Frame {
    uint32_t width, height, ncomp, hmax, vmax, mcus_x, mcus_y, bpm;
};

// a scan as the kernels take it
struct Scan {
    uint32_t ncomp, comp[3]; // indices into the frame's components, ascending
    uint32_t ss, se, ah, al;
    uint32_t restart;      // the scan's MCUs in a restart interval (all of them without DRI)
    uint32_t mcus, across; // the scan's MCUs; the blocks across of a single-component scan
    uint32_t dc_lut[3], ac_lut;
    uint32_t first_interval, intervals, level; // level: the launch it goes in
    uint32_t begin, end;                       // the scan's entropy bytes in the file: stuffed, with its RSTn markers
    uint32_t vfirst;  // where they begin among all scans' bytes laid end to end, every scan from a multiple of 64 (the byte kernels)
    uint32_t ifirst;  // the scan's first restart interval among all intervals in file order (seg_start's index)
};

struct Interval {
    uint32_t scan, index; // the scan, and the interval's number within it
    uint32_t begin, end;  // its bytes in the file: stuffed, up to the first FF of the marker behind it (parse with cut alone)
};

struct File {
    Frame frame{};
    uint32_t focal_length_35mm = 0;
    uint16_t quant[3][64]; // per component, natural order, as in force at the component's first scan
    std::vector<Scan> scans;
    std::vector<Interval> intervals;        // sorted by the scan's level, then AC refinement or not, then by scan
    std::vector<uint32_t> level_first;      // intervals[level_first[l] .. level_first[l + 1]) go in the launches of level l,
    std::vector<uint32_t> level_dc, level_split; // from level_dc[l] on the level's DC-refinement scans' (decoded a lane per block:
                                                 // dc_refinements), from level_split[l] on its AC-refinement scans' (a wave each)
    std::vector<uint32_t> dc_refinements, dc_first; // the DC-refinement scans by level: dc_refinements[dc_first[l] .. dc_first[l + 1])
    uint32_t virtual_bytes = 0;                     // all scans' bytes laid end to end, each scan from a multiple of 64
    std::vector<jc::HuffmanTable> tables;   // the distinct tables the scans use: lookup t is build_lut(tables[t])
    uint64_t subsequences = 0, scan_bytes = 0;
    uint32_t ac_refinement_scans = 0, ac_refinement_launches = 0;
    const char *error = "";
};

inline int refuse(File &f, int code, const char *why)
{
    f.error = why;
    return code;
}

JPEG_PROG_HD inline uint32_t first_slot(const Frame &F, uint32_t c) { return c == 0 ? 0u : F.hmax * F.vmax + c - 1u; }

// block q of scan MCU m of component c -> its index in the block store
JPEG_PROG_HD inline uint32_t block_index(const Frame &F, const Scan &S, uint32_t c, uint32_t m, uint32_t q)
{
    if (S.ncomp > 1) return m * F.bpm + first_slot(F, c) + q;
    const uint32_t ch = c == 0 ? F.hmax : 1u, cv = c == 0 ? F.vmax : 1u, bx = m % S.across, by = m / S.across;
    return ((by / cv) * F.mcus_x + bx / ch) * F.bpm + first_slot(F, c) + (by % cv) * ch + bx % ch;
}

// ---- the marker walk ---------------------------------------------------------------------------------------------------------------
namespace detail {

inline uint32_t table_id(File &f, const jc::HuffmanTable &t)
{
    for (size_t k = 0; k < f.tables.size(); k++)
        if (f.tables[k].total == t.total && !std::memcmp(f.tables[k].counts, t.counts, 16) && !std::memcmp(f.tables[k].symbols, t.symbols, t.total))
            return (uint32_t)k;
    f.tables.push_back(t);
    return (uint32_t)f.tables.size() - 1;
}

// The scan's bytes [s0, s1) cut at its RSTn markers (tests/ref_jpeg_prog.py: intervals).  A run of FF bytes is a data byte
// when 00 follows it, a marker when RSTn does, and the end of the data where the range ends.
inline int cut_intervals(File &f, const uint8_t *data, size_t s0, size_t s1, uint32_t scan, uint32_t want)
{
    uint32_t found = 0;
    size_t begin = s0, i = s0, dropped = 0;
    const size_t first = f.intervals.size();
    auto close = [&](size_t end) {
        const uint64_t bits = (uint64_t)(end - begin - dropped) * 8;
        f.subsequences += bits ? (bits + jc::SUBSEQ_BITS - 1) / jc::SUBSEQ_BITS : 1;
        f.intervals.push_back(Interval{scan, found, (uint32_t)begin, (uint32_t)end});
    };
    while (i < s1) {
        const void *ff = std::memchr(data + i, 0xFF, s1 - i);
        if (!ff) break;
        i = (size_t)((const uint8_t *)ff - data);
        size_t q = i + 1;
        while (q < s1 && data[q] == 0xFF) q++;
        if (q >= s1) {
            s1 = i; // (the data ends at this FF)
            break;
        }
        if (data[q] == 0) {
            dropped += q - i; // the fill bytes and the 00
            i = q + 1;
            continue;
        }
        if (data[q] != 0xD0u + (found & 7u) || found + 1 >= want) return refuse(f, INVALID, "a misnumbered or surplus RSTn");
        close(i);
        found++, begin = i = q + 1, dropped = 0;
    }
    close(s1);
    if (found + 1 != want) {
        f.intervals.resize(first);
        return refuse(f, INVALID, "a missing RSTn");
    }
    return OK;
}

} // namespace detail

// The marker walk of data[0 .. n) over every scan -> OK, INVALID or UNSUPPORTED (f.error says why): jpeg_common.hpp's walk(),
// carried on behind every scan up to EOI or the file's end.  cut: also walk every scan's bytes for its RSTn markers (the
// restart intervals' byte ranges, their numbering and count, the subsequences) - what the device does for the library
// (jpeg_prog_kernels.hip), restated on the host for the CPU program that checks it.
inline int parse(const uint8_t *data, size_t n, File &f, bool cut = false)
{
    // (a file without SOI is refused for that, whatever its size)
    if (n >= (1ull << 31) && data[0] == 0xFF && data[1] == 0xD8) return refuse(f, UNSUPPORTED, "a file of 2^31 or more bytes");
    const jc::Dialect progressive{0xC2, "a frame that is not progressive (SOF2)", "a marker that cannot stand outside a scan"}; // (a baseline file too: cvhip_jpeg_decode's)
    jc::Walk w;
    bool latched[3] = {false, false, false};
    int ledger[3][64];
    for (auto &row : ledger)
        for (int &v : row) v = -1;
    Frame &F = f.frame;
    const int walked = jc::walk(data, n, w, progressive, [&](const uint8_t *seg, size_t len, size_t &at) {
        if (!w.have_frame) return jc::refuse(w, INVALID, "a scan before the frame");
        F = Frame{w.width, w.height, w.components, w.hmax, w.vmax, w.mcus_x, w.mcus_y, jc::blocks_per_mcu(w)};
        if (f.scans.size() >= MAX_SCANS) return jc::refuse(w, UNSUPPORTED, "more than 256 scans");
        if (len < 1 || len != 4 + 2 * (size_t)seg[0]) return jc::refuse(w, INVALID, "SOS");
        const uint32_t ns = seg[0];
        if (ns < 1 || ns > F.ncomp) return jc::refuse(w, INVALID, "SOS");
        Scan S{};
        S.ncomp = ns, S.ss = seg[1 + 2 * ns], S.se = seg[2 + 2 * ns], S.ah = seg[3 + 2 * ns] >> 4, S.al = seg[3 + 2 * ns] & 15u;
        S.ac_lut = NO_LUT;
        if (S.ss > S.se || S.se > 63 || (S.ss == 0 && S.se != 0) || (S.ss > 0 && ns != 1) || S.al > 13 || S.ah > 13)
            return jc::refuse(w, INVALID, "SOS: the band or the bit position");
        if (S.ah && S.al != S.ah - 1) return jc::refuse(w, INVALID, "SOS: a refinement of more than one bit");
        if (F.ncomp == 3 && w.adobe >= 0 && w.adobe != 1) return jc::refuse(w, UNSUPPORTED, "an Adobe transform that is not YCbCr");
        for (uint32_t k = 0; k < ns; k++) {
            uint32_t c = 0;
            while (c < F.ncomp && w.comp[c].id != seg[1 + 2 * k]) c++;
            if (c == F.ncomp) return jc::refuse(w, INVALID, "SOS: no such component");
            if (k && c <= S.comp[k - 1]) return jc::refuse(w, INVALID, "SOS: the components are not in the frame's order");
            const uint32_t td = seg[2 + 2 * k] >> 4, ta = seg[2 + 2 * k] & 15u;
            if (td > 3 || ta > 3) return jc::refuse(w, INVALID, "SOS");
            if (!latched[c]) { // (libjpeg latches a component's table at its first scan)
                if (!w.have_quant[w.comp[c].tq]) return jc::refuse(w, INVALID, "a missing table");
                std::memcpy(f.quant[c], w.quant[w.comp[c].tq], sizeof(f.quant[c]));
                latched[c] = true;
            }
            S.comp[k] = c, S.dc_lut[k] = NO_LUT;
            if (S.ss == 0 && S.ah == 0) {
                if (!w.huff[0][td].present) return jc::refuse(w, INVALID, "a missing table");
                S.dc_lut[k] = detail::table_id(f, w.huff[0][td]);
            }
            if (S.ss > 0) {
                if (!w.huff[1][ta].present) return jc::refuse(w, INVALID, "a missing table");
                S.ac_lut = detail::table_id(f, w.huff[1][ta]);
                if (ledger[c][0] < 0) return jc::refuse(w, INVALID, "an AC scan before the component's DC scan");
            }
            for (uint32_t z = S.ss; z <= S.se; z++) {
                if (S.ah == 0 && ledger[c][z] >= 0) return jc::refuse(w, INVALID, "a first scan of coefficients that were sent");
                if (S.ah && ledger[c][z] != (int)S.ah) return jc::refuse(w, INVALID, "Ah is not the Al the coefficients were last sent with");
                ledger[c][z] = (int)S.al;
            }
        }
        if (ns > 1)
            S.mcus = F.mcus_x * F.mcus_y, S.across = 0;
        else {
            const uint32_t c = S.comp[0], ch = c == 0 ? F.hmax : 1u, cv = c == 0 ? F.vmax : 1u;
            const uint32_t dw = (F.width * ch + F.hmax - 1) / F.hmax, dh = (F.height * cv + F.vmax - 1) / F.vmax;
            S.across = (dw + 7) / 8, S.mcus = S.across * ((dh + 7) / 8);
        }
        S.intervals = w.restart ? (S.mcus + w.restart - 1) / w.restart : 1u;
        S.restart = w.restart ? w.restart : S.mcus;
        // the launch it goes in: behind every earlier scan of one of its components whose band overlaps its own, where it
        // reads what that scan wrote (a refinement); first scans write where nothing was sent
        S.level = 0;
        if (S.ah)
            for (const Scan &before : f.scans) {
                bool shares = false;
                for (uint32_t a = 0; a < before.ncomp; a++)
                    for (uint32_t b = 0; b < ns; b++) shares |= before.comp[a] == S.comp[b];
                if (shares && before.ss <= S.se && S.ss <= before.se && before.level + 1 > S.level) S.level = before.level + 1;
            }
        const size_t start = at, end = jc::scan_end(data, n, start);
        S.first_interval = S.ifirst = (uint32_t)f.intervals.size();
        S.begin = (uint32_t)start, S.end = (uint32_t)end, S.vfirst = f.virtual_bytes;
        f.virtual_bytes += end > start ? (uint32_t)((end - start + 63) / 64 * 64) : 64u;
        if (cut) {
            const int rc = detail::cut_intervals(f, data, start, end, (uint32_t)f.scans.size(), S.intervals);
            if (rc != OK) return jc::refuse(w, rc, f.error);
        } else
            for (uint32_t k = 0; k < S.intervals; k++) f.intervals.push_back(Interval{(uint32_t)f.scans.size(), k, 0u, 0u});
        f.scan_bytes += end - start;
        f.scans.push_back(S);
        at = end;
        w.may_end = true; // behind a scan EOI, or the file's end without one, ends the walk
        return OK;
    });
    f.focal_length_35mm = w.focal_length_35mm;
    if (walked != OK) return refuse(f, walked, w.error);
    for (uint32_t c = 0; c < F.ncomp; c++)
        for (int z = 0; z < 10; z++)
            if (ledger[c][z] != 0) return refuse(f, UNSUPPORTED, "an incomplete progression: a coefficient 0 .. 9 is unsent or unrefined");
    // the launches: the intervals sorted by their scan's level (stable: a level's intervals stay in file order)
    uint32_t levels = 0;
    for (const Scan &S : f.scans) levels = S.level + 1 > levels ? S.level + 1 : levels;
    std::vector<Interval> sorted;
    sorted.reserve(f.intervals.size());
    f.level_first.assign(1, 0u);
    f.dc_first.assign(1, 0u);
    for (uint32_t l = 0; l < levels; l++) {
        bool ac_refinement = false;
        for (int pass = 0; pass < 3; pass++) { // the level's first scans, its DC refinements, its AC refinements
            for (uint32_t s = 0; s < f.scans.size(); s++) {
                Scan &S = f.scans[s];
                const int kind = S.ah == 0 ? 0 : S.ss == 0 ? 1 : 2;
                if (S.level != l || kind != pass) continue;
                const uint32_t from = S.first_interval;
                S.first_interval = (uint32_t)sorted.size();
                for (uint32_t k = 0; k < S.intervals; k++) sorted.push_back(f.intervals[from + k]);
                if (pass == 1) f.dc_refinements.push_back(s);
                if (pass == 2) ac_refinement = true, f.ac_refinement_scans++;
            }
            if (pass == 0) f.level_dc.push_back((uint32_t)sorted.size());
            if (pass == 1) f.level_split.push_back((uint32_t)sorted.size());
        }
        f.level_first.push_back((uint32_t)sorted.size());
        f.dc_first.push_back((uint32_t)f.dc_refinements.size());
        f.ac_refinement_launches += ac_refinement ? 1u : 0u;
    }
    f.intervals.swap(sorted);
    return OK;
}

// ---- the entropy decode of one restart interval ----------------------------------------------------------------------------------------
// The bits of file[pos .. end): stuffed bytes, read through a 64-bit window.  Behind the data the bits are ones; `pad` counts
// those in the window, and cnt < pad says that one of them was consumed (it stays so: both grow together).
struct BitReader {
    const uint8_t *data;
    uint32_t pos, end;
    uint64_t buf;
    int cnt, pad;
    bool stuffed; // the file's bytes (FF 00, FF fill); or the device's clean buffer: data bytes alone
};

// After fill the window holds at least 32 bits (a reader takes at most 16 between two fills).  It is refilled only below that,
// so that a refill takes four to eight bytes in one load where no FF is among them; an FF, and the interval's last bytes, go
// byte by byte.
JPEG_PROG_HD inline void fill(BitReader &r)
{
    if (r.cnt >= 32) return;
    if (r.end - r.pos >= 8) {
        uint64_t w;
        __builtin_memcpy(&w, r.data + r.pos, 8);
        w = __builtin_bswap64(w); // the byte at pos is the highest
        const uint32_t k = (uint32_t)(64 - r.cnt) / 8; // 4 .. 8 bytes fit
        const uint64_t chunk = k == 8 ? w : w & ~(~0ull >> (8 * k));
        const uint64_t x = ~chunk; // a byte FF of the chunk is a byte 00 here (the bytes behind the chunk are FF here)
        if (!r.stuffed || ((x - 0x0101010101010101ull) & ~x & 0x8080808080808080ull) == 0) {
            r.buf |= chunk >> r.cnt;
            r.cnt += (int)(8 * k), r.pos += k;
            return;
        }
    }
    while (r.cnt <= 56) {
        uint32_t b = 0xFF;
        if (r.pos < r.end) {
            b = r.data[r.pos++];
            if (b == 0xFF && r.stuffed) {
                uint32_t q = r.pos;
                while (q < r.end && r.data[q] == 0xFF) q++;
                if (q < r.end && r.data[q] == 0) r.pos = q + 1;
                else r.pos = r.end, r.pad += 8; // the data ends at this FF
            }
        } else
            r.pad += 8;
        r.buf |= (uint64_t)b << (56 - r.cnt);
        r.cnt += 8;
    }
}

// n <= 16 bits
JPEG_PROG_HD inline uint32_t get_bits(BitReader &r, uint32_t n)
{
    if (n == 0) return 0;
    fill(r);
    const uint32_t v = (uint32_t)(r.buf >> (64 - n));
    r.buf <<= n, r.cnt -= (int)n;
    return v;
}

// the next symbol of lookup `lut` -> the symbol, or -1 where no code begins so
JPEG_PROG_HD inline int get_symbol(BitReader &r, const uint16_t *lut)
{
    fill(r);
    const uint32_t entry = lut[r.buf >> 48];
    if (entry == 0) return -1;
    r.buf <<= (entry >> 8), r.cnt -= (int)(entry >> 8);
    return (int)(entry & 255u);
}

JPEG_PROG_HD inline int extend(uint32_t v, uint32_t s) { return s && v < (1u << (s - 1)) ? (int)v - (1 << s) + 1 : (int)v; }

// one correction bit for the non-zero coefficient *v: adds +-(1 << al) where that bit is still clear
JPEG_PROG_HD inline void correct(BitReader &r, int16_t *v, uint32_t al)
{
    if (get_bits(r, 1) && ((int)*v & (1 << al)) == 0) *v = (int16_t)(*v >= 0 ? *v + (1 << al) : *v - (1 << al));
}

// Interval `index` of scan S: file[begin .. end) (stuffed bytes, or with stuffed = false a clean buffer's) into coef (the block store; a refinement reads what is there).  luts: the
// lookups, LUT_ENTRIES each.  -> the error bits; met[METS] takes what the decode met.  Every loop is bounded by the
// interval's blocks and by Se, whatever the bytes are, and every block index lies in the store (block_index).
JPEG_PROG_HD inline uint32_t decode_interval(const uint8_t *file, const Frame &F, const Scan &S, uint32_t index, uint32_t begin, uint32_t end,
                                             const uint16_t *luts, const uint8_t *zigzag, int16_t *coef, uint32_t *met, bool stuffed = true)
{
    BitReader r{file, begin, end, 0, 0, 0, stuffed};
    int pred[3] = {0, 0, 0};
    uint32_t eobrun = 0;
    const uint32_t first = index * S.restart, last = S.mcus - first < S.restart ? S.mcus : first + S.restart;
    const uint16_t *ac = S.ac_lut == NO_LUT ? nullptr : luts + (size_t)S.ac_lut * jc::LUT_ENTRIES;
    for (uint32_t m = first; m < last; m++) {
        for (uint32_t k = 0; k < S.ncomp; k++) {
            const uint32_t c = S.comp[k], nq = S.ncomp > 1 && c == 0 ? F.hmax * F.vmax : 1u;
            for (uint32_t q = 0; q < nq; q++) {
                int16_t *block = coef + (size_t)block_index(F, S, c, m, q) * 64;
                if (S.ss == 0 && S.ah == 0) { // DC first: the running sum, shifted
                    const int s = get_symbol(r, luts + (size_t)S.dc_lut[k] * jc::LUT_ENTRIES);
                    if (s < 0) return ERR_CODE;
                    pred[k] += extend(get_bits(r, (uint32_t)s), (uint32_t)s);
                    block[0] = (int16_t)((uint32_t)pred[k] << S.al);
                } else if (S.ss == 0) { // DC refinement: one bit
                    if (get_bits(r, 1)) block[0] = (int16_t)(block[0] | (1 << S.al));
                } else if (S.ah == 0) { // AC first
                    if (eobrun) {
                        eobrun--;
                        continue;
                    }
                    for (uint32_t z = S.ss; z <= S.se;) {
                        const int sym = get_symbol(r, ac);
                        if (sym < 0) return ERR_CODE;
                        const uint32_t run = (uint32_t)sym >> 4, s = (uint32_t)sym & 15u;
                        if (s) {
                            z += run;
                            if (z > S.se) return ERR_RUN;
                            block[zigzag[z]] = (int16_t)((uint32_t)extend(get_bits(r, s), s) << S.al);
                            z++;
                        } else if (run == 15) {
                            if (z + 16 > S.se + 1) return ERR_RUN;
                            z += 16;
                        } else {
                            eobrun = (1u << run) + get_bits(r, run);
                            if (eobrun > met[MET_EOB_RUN]) met[MET_EOB_RUN] = eobrun;
                            eobrun--;
                            break;
                        }
                    }
                } else { // AC refinement (jdphuff.c: decode_mcu_AC_refine)
                    uint32_t z = S.ss;
                    const bool in_run = eobrun > 0;
                    if (!in_run) {
                        while (z <= S.se) {
                            const int sym = get_symbol(r, ac);
                            if (sym < 0) return ERR_CODE;
                            int run = sym >> 4;
                            const uint32_t s = (uint32_t)sym & 15u;
                            int value = 0;
                            if (s) {
                                if (s != 1) return ERR_REFINE;
                                value = get_bits(r, 1) ? (1 << S.al) : -(1 << S.al); // (the sign comes before the position is walked)
                            } else if (run != 15) {
                                eobrun = (1u << run) + get_bits(r, (uint32_t)run);
                                if (eobrun > met[MET_EOB_RUN]) met[MET_EOB_RUN] = eobrun;
                                break;
                            } else
                                met[MET_ZRL_IN_REFINEMENT] = 1;
                            // `run` zero-history coefficients are skipped, a correction bit for every non-zero one on the way
                            for (;; z++) {
                                if (z > S.se) return ERR_RUN;
                                int16_t *v = block + zigzag[z];
                                if (*v) correct(r, v, S.al);
                                else if (--run < 0) break;
                            }
                            if (s) {
                                block[zigzag[z]] = (int16_t)value;
                                if (z == S.se) met[MET_NEW_AT_SE] = 1;
                            }
                            z++;
                        }
                    }
                    if (eobrun) {
                        bool any = false;
                        for (; z <= S.se; z++)
                            if (block[zigzag[z]]) correct(r, block + zigzag[z], S.al), any = true;
                        if (in_run && any) met[MET_CORRECTIONS_IN_RUN] = 1; // (a block inside the run still reads its correction bits)
                        eobrun--;
                    }
                }
                if (r.cnt < r.pad) return ERR_DATA; // the data ends before the scan's last block
            }
        }
    }
    return 0;
}

} // namespace jpeg_prog
