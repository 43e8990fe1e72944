// jpeg_prog_kernels.hip — cvhip_jpeg_progressive_decode: a progressive (SOF2) JPEG file to Luma8 or RGB8 pixels.
// The pixels are DEFINED as libjpeg's default decode of the whole file (tests/ref_jpeg_prog.py restates it and is pinned to
// Pillow): the coefficients accumulate over all scans as jdphuff.c does and then go through DESIGN.md 4.16's tail unchanged.
// The host (jpeg_prog_common.hpp) walks the markers of the whole file, checks the progression, finds every scan's byte range,
// builds one 16-bit-prefix lookup per distinct Huffman table and orders the scans into launches; the file, the lookups, the scan
// list and the interval list go up in one copy.
//
//   jpeg_prog_mark_kernel     a lane per byte of ALL scans' entropy bytes (laid end to end, every scan from a multiple of 64): data
//                             byte, dropped byte or RSTn, section 4.16's rule; a ballot per wave, launch_scan_u64
//   jpeg_prog_compact_kernel  the data bytes of all scans to one clean buffer; marker k of a scan must be RST(k mod 8) and gives
//                             the scan's restart interval k + 1 its first byte (seg_start, indexed by interval in file order)
//   jpeg_prog_segments_kernel a lane per restart interval: the scan's marker count, the interval's bytes, its 1024-bit subsequences
//   jpeg_prog_subseq_kernel, jpeg_prog_sync_kernel, jpeg_prog_write_kernel   the DC-first and AC-first scans do not depend on
//                             earlier coefficients: ALL of them settle together in one chain of self-synchronising launches, as
//                             section 4.16's one scan does - a lane per subsequence with its own scan's tables, band and MCU, exit
//                             state (bit, block of the scan MCU, zig-zag index), the blocks completed jumping by an EOB run, which
//                             is applied when its symbol is read; launch_scan_u64 over the block counts; a write pass from the
//                             settled states stores the shifted AC values and the DC differences.  A single-component scan maps
//                             its raster block to the store's MCU-padded index by arithmetic (block_index)
//   jpeg_prog_dc_sums_kernel, jpeg_prog_dc_values_kernel   per DC-first scan and component the sums of the differences per scan
//                             MCU, launch_scan_u64, and the DC values: the sum from the restart interval's first MCU on in 16
//                             bits, shifted by Al
//   then per level of the scans' dependency order (a refinement lies behind every earlier scan of its component whose band
//   overlaps its own, so Cb and Cr, or two bands of a component, share a level; a level's scans write disjoint coefficients):
//   jpeg_prog_dc_refine_kernel  a lane per block of all the level's DC-refinement scans: the bit of block b of a restart
//                             interval is bit b of the interval's data
//   jpeg_prog_refine_kernel   the level's AC-refinement scans, a wave per restart interval (jdphuff.c's decode_mcu_AC_refine:
//                             the parse depends on which coefficients are non-zero already, so a guessed block start never
//                             synchronises and a scan is serial within a restart interval): a step per symbol over a ballot of
//                             the block's non-zero history
//   jpeg_prog_dc_kernel       the luma DC values of an MCU to their differences within the MCU: the form jpeg_idct_kernel sums
//   jpeg_idct_kernel, jpeg_pixels_kernel   the baseline path's tail (jpeg_tail.inc), as it is
// A decode from a wrong state is harmless (decode_first), and a refinement wave starts from its interval's true state; whatever
// the bytes are the work is bounded: every read lies inside the interval, every step consumes a bit or moves past a coefficient,
// and every block index lies in the store.  Nothing is written to `out` once an error is flagged.
#include <cstring>
#include <vector>

#include "cvhip_internal.hpp"

#include "jpeg_prog_common.hpp"

namespace cvhip {
namespace {

namespace jc = jpeg_common;
namespace jp = jpeg_prog;

#include "jpeg_tail.inc"

#include "jpeg_entropy.inc"

constexpr uint64_t MAX_BLOCKS = 1ull << 25;
constexpr uint32_t PROG_FLAGS = FLAGS + jp::METS; // flags[FLAG_ERR], and behind the baseline path's words what the decode met

// the scan that virtual byte v lies in: the last with vfirst <= v
__device__ __forceinline__ uint32_t scan_of_byte(const jp::Scan *__restrict__ scans, uint32_t n_scans, uint32_t v)
{
    return last_not_above(n_scans, v, [&](uint32_t s) { return scans[s].vfirst; });
}

// the scan that restart interval g (file order) lies in: the last with ifirst <= g
__device__ __forceinline__ uint32_t scan_of_interval(const jp::Scan *__restrict__ scans, uint32_t n_scans, uint32_t g)
{
    return last_not_above(n_scans, g, [&](uint32_t s) { return scans[s].ifirst; });
}

// The bytes of ALL scans, laid end to end with every scan begun at a multiple of 64 (virtual bytes 0 .. n_virtual; those behind
// a scan's last byte are dropped): a lane per byte.  counts[v / 64] = data bytes | markers << 32 of virtual bytes 64 (v / 64) .. + 63
__device__ __forceinline__ uint32_t kind_of(const uint8_t *__restrict__ file, const jp::Scan *__restrict__ scans, uint32_t n_scans, uint32_t n_virtual,
                                            uint32_t v, uint32_t &s, uint32_t &i)
{
    if (v >= n_virtual) return KIND_DROP;
    s = scan_of_byte(scans, n_scans, v);
    i = scans[s].begin + (v - scans[s].vfirst);
    return i < scans[s].end ? classify<false>(file, scans[s].begin, scans[s].end, i) : KIND_DROP;
}

__global__ __launch_bounds__(BLOCK) void jpeg_prog_mark_kernel(const uint8_t *__restrict__ file, const jp::Scan *__restrict__ scans, uint32_t n_scans,
                                                               uint32_t n_virtual, unsigned long long *__restrict__ counts)
{
    const uint32_t v = blockIdx.x * BLOCK + threadIdx.x;
    uint32_t s = 0, i = 0;
    const uint32_t kind = kind_of(file, scans, n_scans, n_virtual, v, s, i);
    const unsigned long long data = __ballot(kind == KIND_DATA), rst = __ballot(kind == KIND_RST);
    if ((threadIdx.x & 63u) == 0 && v < n_virtual) counts[v >> 6] = (unsigned long long)__popcll(data) | (unsigned long long)__popcll(rst) << 32;
}

// counts: scanned.  clean: the data bytes of all scans in order.  seg_start[g] = the data bytes in front of restart interval g
// (file order; zeroed before): a scan's first byte gives its first interval's, marker k of a scan - which must be RST(k mod 8)
// and not one too many - interval k + 1's.
__global__ __launch_bounds__(BLOCK) void jpeg_prog_compact_kernel(const uint8_t *__restrict__ file, const jp::Scan *__restrict__ scans, uint32_t n_scans,
                                                                  uint32_t n_virtual, const unsigned long long *__restrict__ counts,
                                                                  uint8_t *__restrict__ clean, unsigned long long *__restrict__ seg_start,
                                                                  uint32_t *__restrict__ flags)
{
    const uint32_t v = blockIdx.x * BLOCK + threadIdx.x, lane = threadIdx.x & 63u;
    uint32_t s = 0, i = 0;
    const uint32_t kind = kind_of(file, scans, n_scans, n_virtual, v, s, i);
    const unsigned long long data = __ballot(kind == KIND_DATA), rst = __ballot(kind == KIND_RST), below = (1ull << lane) - 1ull;
    if (v >= n_virtual) return;
    const unsigned long long off = counts[v >> 6];
    const unsigned long long at = (off & 0xFFFFFFFFull) + (unsigned long long)__popcll(data & below);
    if (v == scans[s].vfirst) seg_start[scans[s].ifirst] = at; // (lane 0 of its chunk: at is the chunk's)
    if (kind == KIND_DATA) clean[at] = file[i]; // (at < the data bytes of all scans <= n_virtual)
    if (kind == KIND_RST) {
        const unsigned long long k = (off >> 32) + (unsigned long long)__popcll(rst & below) - (counts[scans[s].vfirst >> 6] >> 32);
        if (k + 1 >= scans[s].intervals || file[i] != 0xD0u + (uint32_t)(k & 7u)) atomicOr(&flags[FLAG_ERR], jp::ERR_RST); // surplus or misnumbered
        else seg_start[scans[s].ifirst + k + 1] = at;
    }
}

// A lane per restart interval g of the n_intervals of all scans: its scan's marker count (a missing RSTn), its bytes, and the
// 1024-bit subsequences they would make (summed into flags[FLAG_SUBSEQUENCES]).  *totals = all data bytes | all markers << 32
__global__ __launch_bounds__(BLOCK) void jpeg_prog_segments_kernel(const jp::Scan *__restrict__ scans, uint32_t n_scans, uint32_t n_intervals,
                                                                   const unsigned long long *__restrict__ counts,
                                                                   const unsigned long long *__restrict__ totals,
                                                                   unsigned long long *__restrict__ seg_start, uint32_t *__restrict__ flags)
{
    const uint32_t g = blockIdx.x * BLOCK + threadIdx.x;
    if (g >= n_intervals) return;
    const uint32_t s = scan_of_interval(scans, n_scans, g);
    const unsigned long long bytes = *totals & 0xFFFFFFFFull;
    if (g == scans[s].ifirst) {
        const unsigned long long behind = s + 1 < n_scans ? counts[scans[s + 1].vfirst >> 6] : *totals;
        if ((behind >> 32) - (counts[scans[s].vfirst >> 6] >> 32) + 1 != scans[s].intervals) atomicOr(&flags[FLAG_ERR], jp::ERR_RST); // a missing RSTn
    }
    const unsigned long long a = seg_start[g], b = g + 1 < n_intervals ? seg_start[g + 1] : bytes;
    if (b < a || b > bytes) { // (only with a marker missing: the entry was never written)
        atomicOr(&flags[FLAG_ERR], jp::ERR_RST);
        return;
    }
    if (g + 1 == n_intervals) seg_start[n_intervals] = bytes;
    const unsigned long long subs = ((b - a) * 8 + jc::SUBSEQ_BITS - 1) / jc::SUBSEQ_BITS;
    atomicAdd(&flags[FLAG_SUBSEQUENCES], (uint32_t)(subs ? subs : 1));
}

// DC refinement: a lane per block of every DC-refinement scan of one level (list[first .. first + count): the scans;
// block_first[k]: the blocks of the scans in front of list[first + k], block_first[count] = all).  The bit of block b of a restart
// interval is bit b of the interval's data.
__global__ __launch_bounds__(BLOCK) void jpeg_prog_dc_refine_kernel(const uint8_t *__restrict__ clean, jp::Frame F, const jp::Scan *__restrict__ scans,
                                                                    const uint32_t *__restrict__ list, const uint32_t *__restrict__ block_first,
                                                                    uint32_t count, const unsigned long long *__restrict__ seg_start,
                                                                    uint32_t n_intervals, const unsigned long long *__restrict__ totals,
                                                                    short *__restrict__ coef, uint32_t *__restrict__ flags)
{
    if (flags[FLAG_ERR]) return; // (set by the launches before this one only: the same for every lane)
    const uint32_t t = blockIdx.x * BLOCK + threadIdx.x;
    if (t >= block_first[count]) return;
    uint32_t k = 0;
    while (k + 1 < count && block_first[k + 1] <= t) k++; // (a level has a few such scans at most)
    const jp::Scan &S = scans[list[k]];
    uint32_t per_mcu = 0;
    for (uint32_t q = 0; q < S.ncomp; q++) per_mcu += S.ncomp > 1 && S.comp[q] == 0 ? F.hmax * F.vmax : 1u;
    const uint32_t n = t - block_first[k], m = n / per_mcu;
    uint32_t within = n % per_mcu, c = S.comp[0];
    for (uint32_t q = 0; q < S.ncomp; q++) { // the block's component and its number among the component's blocks of the MCU
        const uint32_t nq = S.ncomp > 1 && S.comp[q] == 0 ? F.hmax * F.vmax : 1u;
        c = S.comp[q];
        if (within < nq) break;
        within -= nq;
    }
    const uint32_t j = m / S.restart, g = S.ifirst + j;
    const unsigned long long end = (g + 1 < n_intervals ? seg_start[g + 1] : *totals & 0xFFFFFFFFull) * 8;
    const unsigned long long bit = seg_start[g] * 8 + (n - j * S.restart * per_mcu);
    if (bit >= end) {
        atomicOr(&flags[FLAG_ERR], jp::ERR_DATA); // the data ends before the scan's last block
        return;
    }
    if ((clean[bit >> 3] >> (7u - (uint32_t)(bit & 7u))) & 1u) {
        short *dc = coef + (size_t)jp::block_index(F, S, c, m, within) * 64;
        *dc = (short)(*dc | (1 << S.al));
    }
}

// ---- the first scans (DC first, AC first): they do not depend on earlier coefficients, so all of them settle together in one chain
// of self-synchronising launches, as section 4.16's one scan does.  intervals[0 .. n_first) are their restart intervals.
// sub_count[t] = the subsequences (SUBSEQ_BITS bits) of interval t, at least one
__global__ __launch_bounds__(BLOCK) void jpeg_prog_subseq_kernel(const jp::Scan *__restrict__ scans, const jp::Interval *__restrict__ intervals,
                                                                 uint32_t n_first, const unsigned long long *__restrict__ seg_start,
                                                                 unsigned long long *__restrict__ sub_count, const uint32_t *__restrict__ flags)
{
    const uint32_t t = blockIdx.x * BLOCK + threadIdx.x;
    if (t >= n_first) return;
    const uint32_t g = scans[intervals[t].scan].ifirst + intervals[t].index;
    const unsigned long long bits = flags[FLAG_ERR] ? 0ull : (seg_start[g + 1] - seg_start[g]) * 8; // (a broken cut: one subsequence each, never decoded)
    const unsigned long long subs = (bits + jc::SUBSEQ_BITS - 1) / jc::SUBSEQ_BITS;
    sub_count[t] = subs ? subs : 1;
}

// the blocks of a scan MCU
__device__ __forceinline__ uint32_t blocks_per_scan_mcu(const jp::Frame &F, const jp::Scan &S)
{
    uint32_t n = 0;
    for (uint32_t q = 0; q < S.ncomp; q++) n += S.ncomp > 1 && S.comp[q] == 0 ? F.hmax * F.vmax : 1u;
    return n;
}

// block `slot` of a scan MCU -> the component's position in the scan; within = its number among that component's blocks
__device__ __forceinline__ uint32_t slot_position(const jp::Frame &F, const jp::Scan &S, uint32_t slot, uint32_t &within)
{
    uint32_t q = 0;
    within = slot;
    for (; q + 1 < S.ncomp; q++) {
        const uint32_t nq = S.comp[q] == 0 ? F.hmax * F.vmax : 1u; // (S.ncomp > 1 here)
        if (within < nq) break;
        within -= nq;
    }
    return q;
}

// Decodes scan S from `state` while the next bit is below end_bit -> the exit state; blocks += the blocks completed, which an
// EOB run makes many at once: the run is applied when its symbol is read, so none is pending at a boundary.  WRITE: the
// coefficients of the scan's blocks `block` .. below block_limit go to coef (a DC value as its difference), and what the file does
// wrong is flagged.  From a wrong state the decode is harmless: every read is bounded by the interval's end (the bits past it
// read as ones), every step consumes a bit, an unknown code consumes 16 bits and restarts the block, a run past Se ends it.
template <bool WRITE>
__device__ __forceinline__ unsigned long long decode_first(const uint32_t *__restrict__ words, const uint16_t *__restrict__ luts, const jp::Frame &F,
                                                           const jp::Scan &S, unsigned long long state, unsigned long long end_bit,
                                                           unsigned long long seg_end_bits, unsigned long long &blocks, short *__restrict__ coef,
                                                           unsigned long long block, unsigned long long block_limit, uint32_t *__restrict__ flags)
{
    unsigned long long p = state & ((1ull << 40) - 1ull);
    uint32_t slot = (uint32_t)(state >> 40) & 15u, k = (uint32_t)(state >> 44) & 127u;
    const uint32_t ss = S.ss, se = S.se, al = S.al, per_mcu = blocks_per_scan_mcu(F, S);
    const bool dc = ss == 0;
    unsigned long long held_word = ~0ull, held = 0; // the window of word `held_word`: loaded once for the symbols that begin in it
    while (p < end_bit) {
        if (WRITE && block >= block_limit) break;
        uint32_t within = 0;
        const uint32_t position = dc ? slot_position(F, S, slot, within) : 0u;
        const uint32_t table = dc ? S.dc_lut[position] : S.ac_lut;
        if ((p >> 5) != held_word) held_word = p >> 5, held = load_window(words, held_word, seg_end_bits);
        const uint32_t win = (uint32_t)((held << (p & 31u)) >> 32); // the 32 bits at p
        const uint32_t entry = luts[(size_t)table * jc::LUT_ENTRIES + (win >> 16)];
        const uint32_t len = entry >> 8, sym = entry & 255u;
        if (len == 0) { // no such code: 16 bits are consumed and the block starts again
            if (WRITE) atomicOr(&flags[FLAG_ERR], jp::ERR_CODE);
            p += 16, k = ss;
            continue;
        }
        bool done = false;
        if (dc) {
            p += len + sym; // (a DC category is at most 15: jpeg_prog_common.hpp)
            if (WRITE) {
                const int diff = jp::extend(sym ? (win << len) >> (32 - sym) : 0u, sym);
                coef[(size_t)jp::block_index(F, S, S.comp[position], (uint32_t)(block / per_mcu), within) * 64] = (short)diff;
            }
            done = true;
        } else {
            const uint32_t run = sym >> 4, size = sym & 15u;
            if (size) {
                p += len + size;
                k += run;
                if (k > se) {
                    if (WRITE) atomicOr(&flags[FLAG_ERR], jp::ERR_RUN);
                } else if (WRITE) {
                    const int v = jp::extend((win << len) >> (32 - size), size);
                    coef[(size_t)jp::block_index(F, S, S.comp[0], (uint32_t)block, 0) * 64 + d_zigzag[k]] = (short)((uint32_t)v << al);
                }
                k++;
                done = k > se;
            } else if (run == 15) {
                p += len;
                if (WRITE && k + 16 > se + 1) atomicOr(&flags[FLAG_ERR], jp::ERR_RUN);
                k += 16;
                done = k > se;
            } else { // EOBn: this block and the (1 << n) + bits - 1 behind it
                p += len + run;
                const uint32_t eobrun = (1u << run) + (run ? (win << len) >> (32 - run) : 0u);
                if (WRITE) atomicMax(&flags[FLAGS + jp::MET_EOB_RUN], eobrun);
                blocks += eobrun, block += eobrun;
                k = ss;
            }
        }
        if (WRITE && p > seg_end_bits) atomicOr(&flags[FLAG_ERR], jp::ERR_DATA); // the data ends inside a symbol
        if (done) {
            k = ss;
            slot = slot + 1 >= per_mcu ? 0u : slot + 1;
            blocks++, block++;
        }
    }
    return pack_state(p, slot, k);
}

// Section 4.16's jpeg_sync_kernel over the subsequences of ALL first scans, every lane with its own scan's tables, band and
// MCU: its interval, scan and bit range, then jpeg_entropy.inc's settle loop from the guess "its first bit, block 0 of the MCU,
// coefficient Ss" - the true state of an interval's first subsequence.
__global__ __launch_bounds__(BLOCK) void jpeg_prog_sync_kernel(const uint32_t *__restrict__ words, const uint16_t *__restrict__ luts, jp::Frame F,
                                                               const jp::Scan *__restrict__ scans, const jp::Interval *__restrict__ intervals,
                                                               uint32_t n_first, const unsigned long long *__restrict__ seg_start,
                                                               const unsigned long long *__restrict__ sub_first, unsigned long long *__restrict__ entry,
                                                               const unsigned long long *__restrict__ exit_in, unsigned long long *__restrict__ exit_out,
                                                               unsigned long long *__restrict__ counts, uint32_t round, uint32_t *__restrict__ flags)
{
    if (flags[FLAG_ERR]) return; // (set by the kernels before this one only: the same for every lane)
    const unsigned long long i = (unsigned long long)blockIdx.x * BLOCK + threadIdx.x, total = sub_first[n_first];
    const bool active = i < total;
    unsigned long long first_bit = 0, end_bit = 0, seg_end_bits = 0;
    bool known = false;
    uint32_t scan = 0;
    if (active) {
        const uint32_t t = interval_of(sub_first, n_first, i);
        scan = intervals[t].scan;
        const uint32_t g = scans[scan].ifirst + intervals[t].index;
        const unsigned long long j = i - sub_first[t];
        first_bit = seg_start[g] * 8 + j * jc::SUBSEQ_BITS, seg_end_bits = seg_start[g + 1] * 8;
        end_bit = first_bit + jc::SUBSEQ_BITS < seg_end_bits ? first_bit + jc::SUBSEQ_BITS : seg_end_bits;
        known = j == 0;
    }
    settle(
        active, known, i, round, entry, exit_in, exit_out, counts, flags, [&]() { return pack_state(first_bit, 0, scans[scan].ss); },
        [&](unsigned long long state, unsigned long long &blocks) {
            return decode_first<false>(words, luts, F, scans[scan], state, end_bit, seg_end_bits, blocks, nullptr, 0, 0, nullptr);
        });
}

// counts: scanned, counts[the launch's lanes] = their total.  One more decode from the settled states stores the shifted AC
// values and the DC differences into the zeroed block store.
__global__ __launch_bounds__(BLOCK) void jpeg_prog_write_kernel(const uint32_t *__restrict__ words, const uint16_t *__restrict__ luts, jp::Frame F,
                                                                const jp::Scan *__restrict__ scans, const jp::Interval *__restrict__ intervals,
                                                                uint32_t n_first, const unsigned long long *__restrict__ seg_start,
                                                                const unsigned long long *__restrict__ sub_first,
                                                                const unsigned long long *__restrict__ entry, const unsigned long long *__restrict__ counts,
                                                                short *__restrict__ coef, uint32_t *__restrict__ flags)
{
    if (flags[FLAG_ERR] & jp::ERR_RST) return; // (set by the kernels before this one only: the same for every lane)
    const unsigned long long i = (unsigned long long)blockIdx.x * BLOCK + threadIdx.x;
    if (i >= sub_first[n_first]) return;
    const uint32_t t = interval_of(sub_first, n_first, i);
    const jp::Scan &S = scans[intervals[t].scan];
    const uint32_t g = S.ifirst + intervals[t].index, per_mcu = blocks_per_scan_mcu(F, S);
    const unsigned long long j = i - sub_first[t], first_bit = seg_start[g] * 8 + j * jc::SUBSEQ_BITS, seg_end_bits = seg_start[g + 1] * 8;
    const unsigned long long end_bit = first_bit + jc::SUBSEQ_BITS < seg_end_bits ? first_bit + jc::SUBSEQ_BITS : seg_end_bits;
    // the interval's blocks: those of its MCUs, the last interval's may be fewer
    const unsigned long long first_mcu = (unsigned long long)intervals[t].index * S.restart;
    const unsigned long long mcus = S.mcus - first_mcu < S.restart ? S.mcus - first_mcu : S.restart, want = mcus * per_mcu;
    const unsigned long long before = counts[i] - counts[sub_first[t]], here = counts[i + 1] - counts[i];
    if (i + 1 == sub_first[t + 1] && before + here < want) atomicOr(&flags[FLAG_ERR], jp::ERR_DATA); // the data ends before the last block
    if (before >= want) return; // (what follows an interval's last block is not read)
    unsigned long long blocks = 0;
    decode_first<true>(words, luts, F, S, entry[i], end_bit, seg_end_bits, blocks, coef, first_mcu * per_mcu + before, first_mcu * per_mcu + want, flags);
}

// The DC-first scans, a component each (list[3 e ..] = the scan, the component's position in it, the sums in front of it;
// sum_first[n_entries] = all): a lane per scan MCU.  sums[..] = the sum of the DC differences of the component's blocks in it
__device__ __forceinline__ uint32_t dc_entry(const uint32_t *__restrict__ list, uint32_t n_entries, uint32_t t)
{
    uint32_t e = 0;
    while (e + 1 < n_entries && list[3 * (e + 1) + 2] <= t) e++;
    return e;
}

__global__ __launch_bounds__(BLOCK) void jpeg_prog_dc_sums_kernel(const short *__restrict__ coef, jp::Frame F, const jp::Scan *__restrict__ scans,
                                                                  const uint32_t *__restrict__ list, uint32_t n_entries, uint32_t total,
                                                                  unsigned long long *__restrict__ sums, const uint32_t *__restrict__ flags)
{
    const uint32_t t = blockIdx.x * BLOCK + threadIdx.x;
    if (t >= total) return;
    const uint32_t e = dc_entry(list, n_entries, t), m = t - list[3 * e + 2];
    const jp::Scan &S = scans[list[3 * e]];
    const uint32_t c = S.comp[list[3 * e + 1]], nq = S.ncomp > 1 && c == 0 ? F.hmax * F.vmax : 1u;
    long long sum = 0;
    if (!flags[FLAG_ERR])
        for (uint32_t q = 0; q < nq; q++) sum += coef[(size_t)jp::block_index(F, S, c, m, q) * 64];
    sums[t] = (unsigned long long)sum;
}

// sums: scanned.  The DC value of a block: the differences of its component from the restart interval's first MCU on, in 16
// bits, shifted by Al (jdphuff.c: decode_mcu_DC_first).
__global__ __launch_bounds__(BLOCK) void jpeg_prog_dc_values_kernel(short *__restrict__ coef, jp::Frame F, const jp::Scan *__restrict__ scans,
                                                                    const uint32_t *__restrict__ list, uint32_t n_entries, uint32_t total,
                                                                    const unsigned long long *__restrict__ sums, const uint32_t *__restrict__ flags)
{
    if (flags[FLAG_ERR]) return;
    const uint32_t t = blockIdx.x * BLOCK + threadIdx.x;
    if (t >= total) return;
    const uint32_t e = dc_entry(list, n_entries, t), base = list[3 * e + 2], m = t - base;
    const jp::Scan &S = scans[list[3 * e]];
    const uint32_t c = S.comp[list[3 * e + 1]], nq = S.ncomp > 1 && c == 0 ? F.hmax * F.vmax : 1u;
    long long value = (long long)(sums[t] - sums[base + m / S.restart * S.restart]);
    for (uint32_t q = 0; q < nq; q++) {
        short *dc = coef + (size_t)jp::block_index(F, S, c, m, q) * 64;
        value += *dc;
        *dc = (short)((uint32_t)(short)value << S.al);
    }
}

// the next n <= 63 bits as one field, the first bit the highest
__device__ __forceinline__ unsigned long long get_field(jp::BitReader &r, uint32_t n)
{
    unsigned long long field = 0;
    while (n) { // (at most four rounds)
        const uint32_t k = n < 16 ? n : 16u;
        field = field << k | jp::get_bits(r, k);
        n -= k;
    }
    return field;
}

// One correction bit for every coefficient of cmask (zig-zag positions of non-zero coefficients), lowest position first: one
// field of popcount bits, lane z takes bit number popcount(cmask below z) of it and adds +-(1 << al) where that bit of its
// coefficient is still clear.
__device__ __forceinline__ void correct_wave(jp::BitReader &r, unsigned long long cmask, uint32_t lane, uint32_t al, int &v)
{
    const uint32_t n = (uint32_t)__popcll(cmask);
    if (!n) return;
    const unsigned long long field = get_field(r, n);
    if (!((cmask >> lane) & 1ull)) return;
    const uint32_t i = (uint32_t)__popcll(cmask & ((1ull << lane) - 1ull));
    if (((field >> (n - 1 - i)) & 1ull) && (v & (1 << al)) == 0) v = (short)(v >= 0 ? v + (1 << al) : v - (1 << al));
}

// AC refinement (jdphuff.c: decode_mcu_AC_refine), a wave per restart interval: intervals[first + blockIdx.x].  The parse
// depends on which coefficients of the block are non-zero already, so the blocks of an interval go one after the other; within
// a block the wave holds the 64 coefficients a lane each in zig-zag order, and the walk costs a step per symbol, not per
// coefficient: the non-zero history is one ballot, "skip r zero-history coefficients" is the (r + 1)-th clear bit of it, and the
// correction bits of the coefficients in between are one field of popcount bits, read at once and taken by their lanes.  Every
// lane decodes the same symbols from the same bytes: the control flow is the wave's.  A step moves past at least one
// coefficient or ends the block, so a block takes at most Se - Ss + 2 symbols whatever the bytes are.
__global__ __launch_bounds__(WAVE) void jpeg_prog_refine_kernel(const uint8_t *__restrict__ clean, const unsigned long long *__restrict__ seg_start,
                                                                jp::Frame F, const jp::Scan *__restrict__ scans,
                                                                const jp::Interval *__restrict__ intervals, uint32_t first,
                                                                const uint16_t *__restrict__ luts, short *__restrict__ coef, uint32_t *__restrict__ flags)
{
    __shared__ uint16_t s_short[SHORT_ENTRIES];
    if (flags[FLAG_ERR]) return; // (set by the launches before this one only: the same for every lane)
    const uint32_t lane = threadIdx.x;
    const jp::Interval iv = intervals[first + blockIdx.x];
    const jp::Scan &S = scans[iv.scan];
    const uint32_t ss = S.ss, se = S.se, al = S.al, c = S.comp[0];
    const uint16_t *lut = luts + (size_t)S.ac_lut * jc::LUT_ENTRIES;
    for (uint32_t at = lane; at < SHORT_ENTRIES; at += WAVE) s_short[at] = short_entry(lut[at << (16 - SHORT_BITS)]); // (jpeg_entropy.inc: load_short_tables)
    __syncthreads();
    const uint32_t natural = d_zigzag[lane];
    const bool in_band = lane >= ss && lane <= se;
    const unsigned long long band = (~0ull >> (63 - se)) & (~0ull << ss);
    const uint32_t g = S.ifirst + iv.index;
    jp::BitReader r{clean, (uint32_t)seg_start[g], (uint32_t)seg_start[g + 1], 0, 0, 0, false};
    uint32_t eobrun = 0, err = 0, longest = 0, met = 0;
    const uint32_t first_mcu = iv.index * S.restart, last_mcu = S.mcus - first_mcu < S.restart ? S.mcus : first_mcu + S.restart;
    short *block = coef + (size_t)jp::block_index(F, S, c, first_mcu, 0) * 64;
    int next = in_band ? block[natural] : 0; // (the block behind is loaded while this one is decoded)
    for (uint32_t m = first_mcu; m < last_mcu && !err; m++) {
        short *mine = block + natural;
        const int old = next;
        if (m + 1 < last_mcu) {
            block = coef + (size_t)jp::block_index(F, S, c, m + 1, 0) * 64;
            next = in_band ? block[natural] : 0;
        }
        int v = old;
        const unsigned long long nz = __ballot(old != 0);
        uint32_t z = ss;
        const bool in_run = eobrun > 0;
        if (!in_run) {
            while (z <= se) {
                jp::fill(r);
                uint32_t entry = s_short[r.buf >> (64 - SHORT_BITS)];
                if (entry == 0) entry = lut[r.buf >> 48];
                if (entry == 0) {
                    err = jp::ERR_CODE;
                    break;
                }
                r.buf <<= (entry >> 8), r.cnt -= (int)(entry >> 8);
                const uint32_t run = (entry >> 4) & 15u, s = entry & 15u;
                int value = 0;
                if (s) {
                    if (s != 1) {
                        err = jp::ERR_REFINE;
                        break;
                    }
                    value = jp::get_bits(r, 1) ? (1 << al) : -(1 << al); // (the sign comes before the position is walked)
                } else if (run != 15) {
                    eobrun = (1u << run) + jp::get_bits(r, run);
                    longest = eobrun > longest ? eobrun : longest;
                    break;
                } else
                    met |= 1u << jp::MET_ZRL_IN_REFINEMENT;
                // the (run + 1)-th zero-history coefficient at or behind z
                unsigned long long zeros = ~nz & band & (~0ull << z);
                for (uint32_t k = 0; k < run; k++) zeros &= zeros - 1;
                if (!zeros) {
                    err = jp::ERR_RUN;
                    break;
                }
                const uint32_t t = (uint32_t)__builtin_ctzll(zeros);
                correct_wave(r, nz & (~0ull << z) & ((1ull << t) - 1ull), lane, al, v);
                if (s) {
                    if (lane == t) v = value;
                    if (t == se) met |= 1u << jp::MET_NEW_AT_SE;
                }
                z = t + 1;
            }
        }
        if (eobrun && !err) { // the rest of the band: correction bits alone; a block inside the run reads its own too
            const unsigned long long cmask = z <= se ? nz & band & (~0ull << z) : 0ull;
            correct_wave(r, cmask, lane, al, v);
            if (in_run && cmask) met |= 1u << jp::MET_CORRECTIONS_IN_RUN;
            eobrun--;
        }
        if (!err && r.cnt < r.pad) err = jp::ERR_DATA; // the data ends before the scan's last block
        if (v != old) *mine = (short)v;
    }
    if (lane) return;
    if (err) atomicOr(&flags[FLAG_ERR], err);
    if (longest) atomicMax(&flags[FLAGS + jp::MET_EOB_RUN], longest);
    for (uint32_t k = 1; k < jp::METS; k++)
        if (met & (1u << k)) atomicOr(&flags[FLAGS + k], 1u);
}

// The store holds DC values; jpeg_idct_kernel adds up, per block, the luma DC entries of its MCU up to its own (the baseline
// path keeps differences there).  So luma slot q > 0 of every MCU gets its value minus slot q - 1's, in 16 bits.
__global__ __launch_bounds__(BLOCK) void jpeg_prog_dc_kernel(short *__restrict__ coef, JpegParams P, const uint32_t *__restrict__ flags)
{
    if (flags[FLAG_ERR]) return;
    const uint32_t m = blockIdx.x * BLOCK + threadIdx.x;
    if (m >= P.mcus) return;
    for (uint32_t q = P.luma_blocks - 1; q > 0; q--) {
        short *at = coef + ((unsigned long long)m * P.bpm + q) * 64;
        at[0] = (short)(at[0] - at[-64]);
    }
}

thread_local uint64_t t_stats[8] = {0, 0, 0, 0, 0, 0, 0, 0};

} // namespace
} // namespace cvhip

using namespace cvhip;

extern "C" int cvhip_jpeg_progressive_info(const uint8_t *file, uint64_t size, uint32_t *out_info)
{
    if (!file || !out_info) return fail(CVHIP_ERR_INVALID, "jpeg_progressive_info: null argument");
    jp::File f;
    const int rc = jp::parse(file, (size_t)size, f);
    if (rc != jp::OK) return refused("jpeg_progressive_info", rc == jp::UNSUPPORTED, f.error);
    out_info[0] = f.frame.width, out_info[1] = f.frame.height, out_info[2] = f.frame.ncomp, out_info[3] = f.frame.hmax, out_info[4] = f.frame.vmax;
    out_info[5] = f.focal_length_35mm, out_info[6] = (uint32_t)f.scans.size();
    return CVHIP_OK;
}

extern "C" int cvhip_jpeg_progressive_last_stats(uint64_t *out_stats)
{
    if (!out_stats) return fail(CVHIP_ERR_INVALID, "jpeg_progressive_last_stats: null argument");
    for (int k = 0; k < 8; k++) out_stats[k] = t_stats[k];
    return CVHIP_OK;
}

extern "C" int cvhip_jpeg_progressive_decode(cvhip_device *dev, const uint8_t *file, uint64_t size, uint32_t format, uint32_t drop_rows, uint8_t *out,
                                             uint64_t cap, uint64_t *out_size)
{
    const char *what = "jpeg_progressive_decode";
    if (!dev || !file || !out_size || (cap && !out)) return fail(CVHIP_ERR_INVALID, "jpeg_progressive_decode: null argument");
    if (format != CVHIP_IMAGE_LUMA8 && format != CVHIP_IMAGE_RGB8)
        return fail(CVHIP_ERR_INVALID, "jpeg_progressive_decode: format is not CVHIP_IMAGE_LUMA8 or CVHIP_IMAGE_RGB8");
    jp::File f;
    const int rc = jp::parse(file, (size_t)size, f);
    if (rc != jp::OK) return refused(what, rc == jp::UNSUPPORTED, f.error);
    const jp::Frame &F = f.frame;
    if (drop_rows >= F.height) return fail(CVHIP_ERR_INVALID, "jpeg_progressive_decode: drop_rows leaves no row");
    const uint32_t channels = format == CVHIP_IMAGE_RGB8 ? 3u : 1u;
    const unsigned long long bytes = (unsigned long long)F.width * (F.height - drop_rows) * channels;
    *out_size = bytes;
    if (!cap) return CVHIP_OK;
    if (cap < bytes) return fail(CVHIP_ERR_INVALID, "jpeg_progressive_decode: the buffer is smaller than the image");
    JpegParams P{};
    P.width = F.width, P.height = F.height, P.ncomp = F.ncomp, P.hmax = F.hmax, P.vmax = F.vmax, P.mcus_x = F.mcus_x, P.mcus_y = F.mcus_y;
    P.bpm = F.bpm, P.mcus = F.mcus_x * F.mcus_y, P.interval = P.mcus, P.luma_blocks = F.hmax * F.vmax;
    const unsigned long long n_blocks = (unsigned long long)P.mcus * P.bpm;
    if (n_blocks > MAX_BLOCKS) return fail(CVHIP_ERR_UNSUPPORTED, "jpeg_progressive_decode: more than 2^25 blocks");
    // ---- the one upload: the quantisation tables, the lookups, the scan list, the interval list, the DC-refinement lists, the file
    auto round16 = [](size_t v) { return (v + 15) / 16 * 16; };
    const size_t quant_bytes = 3 * 64 * sizeof(uint16_t), lut_bytes = f.tables.size() * jc::LUT_ENTRIES * sizeof(uint16_t);
    const size_t scan_bytes = round16(f.scans.size() * sizeof(jp::Scan)), interval_bytes = round16(f.intervals.size() * sizeof(jp::Interval));
    // the DC-refinement scans by level, and per level the blocks in front of each (a lane per block)
    std::vector<uint32_t> dc_blocks;
    for (size_t l = 0; l + 1 < f.dc_first.size(); l++) {
        uint32_t blocks = 0;
        for (uint32_t k = f.dc_first[l]; k <= f.dc_first[l + 1]; k++) {
            dc_blocks.push_back(blocks);
            if (k == f.dc_first[l + 1]) break;
            const jp::Scan &S = f.scans[f.dc_refinements[k]];
            uint32_t per_mcu = 0;
            for (uint32_t q = 0; q < S.ncomp; q++) per_mcu += S.ncomp > 1 && S.comp[q] == 0 ? F.hmax * F.vmax : 1u;
            blocks += S.mcus * per_mcu; // (at most 2^25: a scan's blocks are the frame's or fewer, a level's scans disjoint)
        }
    }
    // the DC-first scans a component each: the scan, the component's position in it, the scan MCUs in front (a lane per scan MCU)
    std::vector<uint32_t> dc_first_list;
    uint32_t dc_mcus = 0;
    for (size_t k = 0; k < f.scans.size(); k++)
        if (f.scans[k].ss == 0 && f.scans[k].ah == 0)
            for (uint32_t q = 0; q < f.scans[k].ncomp; q++) {
                dc_first_list.insert(dc_first_list.end(), {(uint32_t)k, q, dc_mcus});
                dc_mcus += f.scans[k].mcus;
            }
    const uint32_t n_dc_entries = (uint32_t)dc_first_list.size() / 3;
    const size_t dc_bytes = round16((f.dc_refinements.size() + dc_blocks.size() + dc_first_list.size()) * sizeof(uint32_t));
    const size_t at_luts = quant_bytes, at_scans = at_luts + lut_bytes, at_intervals = at_scans + scan_bytes, at_dc = at_intervals + interval_bytes;
    const size_t at_file = at_dc + dc_bytes;
    std::vector<uint8_t> blob(at_file + (size_t)size);
    if (!f.dc_refinements.empty()) std::memcpy(blob.data() + at_dc, f.dc_refinements.data(), f.dc_refinements.size() * sizeof(uint32_t));
    std::memcpy(blob.data() + at_dc + f.dc_refinements.size() * sizeof(uint32_t), dc_blocks.data(), dc_blocks.size() * sizeof(uint32_t));
    if (n_dc_entries)
        std::memcpy(blob.data() + at_dc + (f.dc_refinements.size() + dc_blocks.size()) * sizeof(uint32_t), dc_first_list.data(),
                    dc_first_list.size() * sizeof(uint32_t));
    for (uint32_t c = 0; c < F.ncomp; c++) std::memcpy(blob.data() + c * 64 * sizeof(uint16_t), f.quant[c], 64 * sizeof(uint16_t));
    for (size_t t = 0; t < f.tables.size(); t++) jc::build_lut(f.tables[t], reinterpret_cast<uint16_t *>(blob.data() + at_luts) + t * jc::LUT_ENTRIES);
    std::memcpy(blob.data() + at_scans, f.scans.data(), f.scans.size() * sizeof(jp::Scan));
    std::memcpy(blob.data() + at_intervals, f.intervals.data(), f.intervals.size() * sizeof(jp::Interval));
    std::memcpy(blob.data() + at_file, file, (size_t)size);

    CVHIP_TRY_HIP(hipSetDevice(dev->d.ordinal));
    hipStream_t s = dev->d.stream;
    CallScratch sc;
    PlaneLayout layout(P);
    Carver carve; // one allocation, carved: an allocation costs more than most of these kernels
    const size_t sums_bytes = ((size_t)P.ncomp * P.mcus + 1) * 8;
    const uint32_t n_virtual = f.virtual_bytes, chunks = n_virtual / 64, n_scans = (uint32_t)f.scans.size(), n_intervals = (uint32_t)f.intervals.size();
    const size_t at_blob = carve.reserve(blob.size()), at_flags = carve.reserve(PROG_FLAGS * sizeof(uint32_t));
    const uint32_t n_first = f.level_dc[0]; // the restart intervals of the first scans: intervals[0 .. n_first)
    const unsigned long long sub_cap = n_virtual / (jc::SUBSEQ_BITS / 8) + n_first + 1;
    const uint32_t sync_blocks = (uint32_t)((sub_cap + BLOCK - 1) / BLOCK);
    const size_t at_sub = carve.reserve(((size_t)n_first + 1) * 8), at_states = carve.reserve((size_t)sub_cap * 3 * 8); // entry states, the exit states of two launches
    const size_t at_counts = carve.reserve(((size_t)sub_cap + 1) * 8), at_dc_sums = carve.reserve(((size_t)dc_mcus + 1) * 8);
    const size_t at_clean = carve.reserve((size_t)n_virtual + 16), at_chunks = carve.reserve(((size_t)chunks + 1) * 8), at_seg = carve.reserve(((size_t)n_intervals + 1) * 8);
    const size_t at_coef = carve.reserve((size_t)n_blocks * 64 * sizeof(short)), at_sums = carve.reserve(sums_bytes), at_planes = carve.reserve(layout.total);
    uint8_t *arena = nullptr, *d_out = nullptr;
    hipError_t e = sc.alloc(&arena, carve.total);
    if (e == hipSuccess) e = sc.output(out, (size_t)bytes, &d_out);
    if (e != hipSuccess) return device_error(what, e);
    uint8_t *d_blob = arena + at_blob;
    uint32_t *flags = reinterpret_cast<uint32_t *>(arena + at_flags), h_flags[PROG_FLAGS] = {0};
    short *coef = reinterpret_cast<short *>(arena + at_coef);
    unsigned long long *sums = reinterpret_cast<unsigned long long *>(arena + at_sums); // zero: the store holds DC values, not differences
    if (e == hipSuccess) e = hipMemcpyAsync(d_blob, blob.data(), blob.size(), hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipMemsetAsync(flags, 0, PROG_FLAGS * sizeof(uint32_t), s);
    if (e == hipSuccess) e = hipMemsetAsync(coef, 0, (size_t)n_blocks * 64 * sizeof(short), s);
    if (e == hipSuccess) e = hipMemsetAsync(sums, 0, sums_bytes, s);
    uint8_t *clean = arena + at_clean;
    unsigned long long *chunk_counts = reinterpret_cast<unsigned long long *>(arena + at_chunks), *seg_start = reinterpret_cast<unsigned long long *>(arena + at_seg);
    if (e == hipSuccess) e = hipMemsetAsync(seg_start, 0, ((size_t)n_intervals + 1) * 8, s);
    unsigned long long *sub_first = reinterpret_cast<unsigned long long *>(arena + at_sub), *states = reinterpret_cast<unsigned long long *>(arena + at_states);
    unsigned long long *counts = reinterpret_cast<unsigned long long *>(arena + at_counts), *dc_sums = reinterpret_cast<unsigned long long *>(arena + at_dc_sums);
    if (e == hipSuccess) e = hipMemsetAsync(counts, 0, ((size_t)sub_cap + 1) * 8, s);
    if (e != hipSuccess) return device_error(what, e);
    const Planes &planes = layout.placed(arena + at_planes, P.ncomp);
    const uint16_t *d_quant = reinterpret_cast<const uint16_t *>(d_blob), *d_luts = reinterpret_cast<const uint16_t *>(d_blob + at_luts);
    const jp::Scan *d_scans = reinterpret_cast<const jp::Scan *>(d_blob + at_scans);
    const jp::Interval *d_intervals = reinterpret_cast<const jp::Interval *>(d_blob + at_intervals);
    const uint8_t *d_file = d_blob + at_file;
    const uint32_t *d_dc_list = reinterpret_cast<const uint32_t *>(d_blob + at_dc), *d_dc_blocks = d_dc_list + f.dc_refinements.size();
    const dim3 block(BLOCK), byte_grid((n_virtual + BLOCK - 1) / BLOCK);
    // ---- the bytes of all scans: marked, compacted and cut into restart intervals, one launch each
    hipLaunchKernelGGL(jpeg_prog_mark_kernel, byte_grid, block, 0, s, d_file, d_scans, n_scans, n_virtual, chunk_counts);
    launch_scan_u64(chunk_counts, chunks, chunk_counts + chunks, s);
    hipLaunchKernelGGL(jpeg_prog_compact_kernel, byte_grid, block, 0, s, d_file, d_scans, n_scans, n_virtual, chunk_counts, clean, seg_start, flags);
    hipLaunchKernelGGL(jpeg_prog_segments_kernel, dim3((n_intervals + BLOCK - 1) / BLOCK), block, 0, s, d_scans, n_scans, n_intervals, chunk_counts,
                       chunk_counts + chunks, seg_start, flags);
    // ---- the first scans: their states settle within the workgroups, then across them, a launch and one flag back per round
    const uint32_t *words = reinterpret_cast<const uint32_t *>(clean), *d_dc_first = d_dc_blocks + dc_blocks.size();
    unsigned long long *entry = states, *exits[2] = {states + sub_cap, states + 2 * sub_cap};
    hipLaunchKernelGGL(jpeg_prog_subseq_kernel, dim3((n_first + BLOCK - 1) / BLOCK), block, 0, s, d_scans, d_intervals, n_first, seg_start, sub_first, flags);
    launch_scan_u64(sub_first, n_first, sub_first + n_first, s);
    uint32_t launches = 0;
    int status = settle_launches(what, sync_blocks, flags, h_flags, PROG_FLAGS, s, launches, [&](uint32_t round, uint32_t from, uint32_t to) {
        hipLaunchKernelGGL(jpeg_prog_sync_kernel, dim3(sync_blocks), block, 0, s, words, d_luts, F, d_scans, d_intervals, n_first, seg_start, sub_first, entry,
                           exits[from], exits[to], counts, round, flags);
    });
    if (status != CVHIP_OK) return status;
    launch_scan_u64(counts, sub_cap, counts + sub_cap, s);
    hipLaunchKernelGGL(jpeg_prog_write_kernel, dim3(sync_blocks), block, 0, s, words, d_luts, F, d_scans, d_intervals, n_first, seg_start, sub_first, entry,
                       counts, coef, flags);
    const dim3 dc_grid((dc_mcus + BLOCK - 1) / BLOCK);
    hipLaunchKernelGGL(jpeg_prog_dc_sums_kernel, dc_grid, block, 0, s, coef, F, d_scans, d_dc_first, n_dc_entries, dc_mcus, dc_sums, flags);
    launch_scan_u64(dc_sums, dc_mcus, dc_sums + dc_mcus, s);
    hipLaunchKernelGGL(jpeg_prog_dc_values_kernel, dc_grid, block, 0, s, coef, F, d_scans, d_dc_first, n_dc_entries, dc_mcus, dc_sums, flags);
    // ---- the refinements, level by level: the DC refinements a lane per block, the AC refinements a wave per restart interval
    for (size_t l = 1; l + 1 < f.level_first.size(); l++) {
        const uint32_t split = f.level_split[l], end = f.level_first[l + 1];
        const uint32_t dc_count = f.dc_first[l + 1] - f.dc_first[l], dc_at = f.dc_first[l] + (uint32_t)l; // (a level's list has one entry more)
        if (dc_count && dc_blocks[dc_at + dc_count])
            hipLaunchKernelGGL(jpeg_prog_dc_refine_kernel, dim3((dc_blocks[dc_at + dc_count] + BLOCK - 1) / BLOCK), block, 0, s, clean, F, d_scans,
                               d_dc_list + f.dc_first[l], d_dc_blocks + dc_at, dc_count, seg_start, n_intervals, chunk_counts + chunks, coef, flags);
        if (end > split)
            hipLaunchKernelGGL(jpeg_prog_refine_kernel, dim3(end - split), dim3(WAVE), 0, s, clean, seg_start, F, d_scans, d_intervals, split, d_luts, coef,
                               flags);
    }
    // ---- the tail, as the baseline path's
    if (P.luma_blocks > 1) hipLaunchKernelGGL(jpeg_prog_dc_kernel, dim3((P.mcus + BLOCK - 1) / BLOCK), block, 0, s, coef, P, flags);
    status = launch_tail(what, P, planes, coef, sums, d_quant, channels, d_out, bytes, flags, h_flags, PROG_FLAGS, s);
    if (status != CVHIP_OK) return status;
    t_stats[0] = f.scans.size(), t_stats[1] = f.intervals.size(), t_stats[2] = h_flags[FLAG_SUBSEQUENCES], t_stats[3] = launches, t_stats[4] = h_flags[FLAG_ROUNDS];
    t_stats[5] = f.ac_refinement_scans, t_stats[6] = f.ac_refinement_launches, t_stats[7] = h_flags[FLAGS + jp::MET_EOB_RUN];
    const uint32_t err = h_flags[FLAG_ERR];
    if (err & jp::ERR_RST) return fail(CVHIP_ERR_INVALID, "jpeg_progressive_decode: a missing, surplus or misnumbered RSTn");
    if (err & jp::ERR_CODE) return fail(CVHIP_ERR_INVALID, "jpeg_progressive_decode: a code that is not in its table");
    if (err & jp::ERR_RUN) return fail(CVHIP_ERR_INVALID, "jpeg_progressive_decode: a run past Se");
    if (err & jp::ERR_REFINE) return fail(CVHIP_ERR_INVALID, "jpeg_progressive_decode: a refinement symbol of more than one bit");
    if (err & jp::ERR_DATA) return fail(CVHIP_ERR_INVALID, "jpeg_progressive_decode: the data ends before the scan's last block");
    return deliver(what, sc, out, d_out, bytes, s);
}
