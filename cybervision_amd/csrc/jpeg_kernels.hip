// jpeg_kernels.hip — cvhip_jpeg_decode: a baseline JPEG file to Luma8 or RGB8 pixels, everything behind the marker walk on the
// device.  The reference opens its inputs with image::open(path)?.into_luma8() / into_rgb8()
// (src/reconstruction.rs:40-60); the pixels are DEFINED here as libjpeg's default decode (tests/ref_jpeg.py restates it and
// is pinned to Pillow on encoder-made files).  The host (jpeg_common.hpp) walks the markers, builds one 16-bit-prefix
// lookup per Huffman table and finds the scan's bytes; tables and scan go up in one copy.
//
//   jpeg_mark_kernel      a lane per byte of the scan: data byte, dropped byte (the 00 behind an FF, FF fill, a marker's
//                         bytes) or RSTn; a ballot per wave -> per 64 bytes the data bytes and the markers; launch_scan_u64
//   jpeg_compact_kernel   the data bytes to the clean buffer (no stuffing, no markers); marker k must be RST(k mod 8) and
//                         gives restart interval k + 1 its first byte
//   jpeg_segments_kernel  the subsequences (SUBSEQ_BITS bits) of every restart interval; a scan places them
//   jpeg_sync_kernel      the self-synchronising decode: a lane decodes its subsequence from a guessed state (its first bit,
//                         block slot 0, coefficient 0), records its exit state (bit, slot in the MCU, zig-zag index) and
//                         the blocks it completed, and decodes again from its left neighbour's exit state until no state in
//                         the workgroup changes.  Across workgroups the kernel is launched again, each first lane taking
//                         the last exit state of the workgroup before it from the launch before, until a launch changes
//                         no workgroup's last exit state.  The first subsequence of an interval starts from the known
//                         state, so the settled states are the sequential decoder's, whatever the number of rounds
//   jpeg_write_kernel     a scan of the block counts gives every subsequence its first block; one more decode from the
//                         settled states stores DC differences and AC coefficients as int16 blocks in natural order
//   jpeg_dc_kernel        per MCU and component the sum of its DC differences; a scan (the DC value of a block is a
//                         difference of two prefix sums plus the differences before it in its MCU, 16-bit wrap)
//   jpeg_idct_kernel      a lane per block: DC, dequantisation, jidctint in 64-bit integers, clamp, the 8 x 8 samples
//                         into the component's plane
//   jpeg_pixels_kernel    a lane per aligned dword of `out`: fancy upsampling, YCbCr -> RGB, luma, crop and drop_rows;
//                         single bytes only in front of the first and behind the last whole dword
// A decode from a wrong state is harmless: every read is bounded by the interval's end (the bits past it read as ones), an
// unknown code consumes 16 bits and restarts the block, a run past coefficient 63 ends the block.  In the write pass, whose
// states are the true ones, the same events are the file's errors.
#include <cstring>
#include <vector>

#include "cvhip_internal.hpp"

#include "jpeg_common.hpp"

namespace cvhip {
namespace {

namespace jc = jpeg_common;

#include "jpeg_tail.inc"

#include "jpeg_entropy.inc"

constexpr uint32_t ERR_RST = 1, ERR_CODE = 2, ERR_RUN = 4, ERR_DATA = 8;
constexpr uint32_t MAX_LUTS = 6; // the tables of a scan, whose short codes lie in LDS
constexpr uint64_t MAX_SCAN_BYTES = 1ull << 31, MAX_BLOCKS = 1ull << 25;

// counts[i / 64] = data bytes | markers << 32 of bytes 64 (i / 64) .. + 63
__global__ __launch_bounds__(BLOCK) void jpeg_mark_kernel(const uint8_t *__restrict__ scan, unsigned long long n, unsigned long long *__restrict__ counts)
{
    const unsigned long long i = (unsigned long long)blockIdx.x * BLOCK + threadIdx.x;
    const uint32_t kind = i < n ? classify<true>(scan, 0ull, n, i) : KIND_DROP;
    const unsigned long long data = __ballot(kind == KIND_DATA), rst = __ballot(kind == KIND_RST);
    if ((threadIdx.x & 63u) == 0 && i < n) counts[i >> 6] = (unsigned long long)__popcll(data) | (unsigned long long)__popcll(rst) << 32;
}

// counts: scanned.  clean: the data bytes in order.  seg_start[k + 1] = the data bytes in front of marker k (zeroed before).
__global__ __launch_bounds__(BLOCK) void jpeg_compact_kernel(const uint8_t *__restrict__ scan, unsigned long long n,
                                                             const unsigned long long *__restrict__ counts, uint8_t *__restrict__ clean,
                                                             unsigned long long *__restrict__ seg_start, uint32_t nseg, uint32_t *__restrict__ flags)
{
    const unsigned long long i = (unsigned long long)blockIdx.x * BLOCK + threadIdx.x;
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t kind = i < n ? classify<true>(scan, 0ull, n, i) : KIND_DROP;
    const unsigned long long data = __ballot(kind == KIND_DATA), rst = __ballot(kind == KIND_RST), below = (1ull << lane) - 1ull;
    if (i >= n) return;
    const unsigned long long off = counts[i >> 6];
    const unsigned long long at = (off & 0xFFFFFFFFull) + (unsigned long long)__popcll(data & below);
    if (kind == KIND_DATA) clean[at] = scan[i]; // (at < the data bytes of the scan <= n)
    if (kind == KIND_RST) {
        const unsigned long long k = (off >> 32) + (unsigned long long)__popcll(rst & below);
        if (k + 1 >= nseg || scan[i] != 0xD0u + (uint32_t)(k & 7u)) atomicOr(&flags[FLAG_ERR], ERR_RST); // surplus or misnumbered
        else seg_start[k + 1] = at;
    }
}

// sub_count[s] = the subsequences of interval s (at least one); *totals = the scan's data bytes | markers << 32
__global__ __launch_bounds__(BLOCK) void jpeg_segments_kernel(unsigned long long *__restrict__ seg_start, uint32_t nseg,
                                                              const unsigned long long *__restrict__ totals,
                                                              unsigned long long *__restrict__ sub_count, uint32_t *__restrict__ flags)
{
    const uint32_t s = blockIdx.x * BLOCK + threadIdx.x;
    if (s >= nseg) return;
    const unsigned long long bytes = *totals & 0xFFFFFFFFull, markers = *totals >> 32;
    if (s == 0 && markers + 1 != nseg) atomicOr(&flags[FLAG_ERR], ERR_RST); // a missing RSTn
    const unsigned long long a = seg_start[s];
    unsigned long long b = s + 1 < nseg ? seg_start[s + 1] : bytes;
    if (b < a || b > bytes) b = a, atomicOr(&flags[FLAG_ERR], ERR_RST); // (only with a marker missing: the entry was never written)
    const unsigned long long subs = ((b - a) * 8 + jc::SUBSEQ_BITS - 1) / jc::SUBSEQ_BITS;
    sub_count[s] = subs ? subs : 1;
    if (s + 1 == nseg) seg_start[nseg] = bytes;
}

// ---- the entropy decoder of one subsequence ---------------------------------------------------------------------------------------
// Decodes from `state` while the next bit is below end_bit -> the exit state; blocks += the blocks completed.  WRITE: the
// coefficients of blocks `block` .. below block_limit go to coef (the DC as its difference), and what the file does wrong is
// flagged.
template <bool WRITE>
__device__ __forceinline__ unsigned long long decode_subsequence(const uint32_t *__restrict__ words, const uint16_t *__restrict__ luts,
                                                                 const uint16_t *s_short, const JpegParams &P, unsigned long long state, unsigned long long end_bit,
                                                                 unsigned long long seg_end_bits, unsigned long long &blocks,
                                                                 short *__restrict__ coef, unsigned long long block, unsigned long long block_limit,
                                                                 uint32_t *__restrict__ flags)
{
    unsigned long long p = state & ((1ull << 40) - 1ull);
    uint32_t slot = (uint32_t)(state >> 40) & 15u, k = (uint32_t)(state >> 44) & 127u;
    unsigned long long held_word = ~0ull, held = 0; // the window of word `held_word`: loaded once for the symbols that begin in it
    while (p < end_bit) {
        if (WRITE && block >= block_limit) break;
        const uint32_t c = slot_component(P, slot);
        const uint32_t table = k == 0 ? pick(P.dc_lut, c) : pick(P.ac_lut, c);
        if ((p >> 5) != held_word) held_word = p >> 5, held = load_window(words, held_word, seg_end_bits);
        const uint32_t win = (uint32_t)((held << (p & 31u)) >> 32); // the 32 bits at p
        uint32_t entry = s_short[table * SHORT_ENTRIES + (win >> (32 - SHORT_BITS))];
        if (entry == 0) entry = luts[(size_t)table * jc::LUT_ENTRIES + (win >> 16)];
        const uint32_t len = entry >> 8, sym = entry & 255u;
        if (len == 0) { // no such code: 16 bits are consumed and the block starts again
            if (WRITE) atomicOr(&flags[FLAG_ERR], ERR_CODE);
            p += 16, k = 0;
            continue;
        }
        const uint32_t run = k == 0 ? 0u : sym >> 4, size = k == 0 ? sym : sym & 15u; // (a DC category is at most 15: jpeg_common.hpp)
        p += len + size;
        if (WRITE && p > seg_end_bits) atomicOr(&flags[FLAG_ERR], ERR_DATA); // the data ends inside a symbol
        if (k != 0 && size == 0) {
            if (run == 15 && k + 16 <= 64) k += 16;
            else {
                if (WRITE && run == 15) atomicOr(&flags[FLAG_ERR], ERR_RUN);
                k = 64; // end of block
            }
        } else {
            k += run;
            if (k > 63) {
                if (WRITE) atomicOr(&flags[FLAG_ERR], ERR_RUN);
                k = 64;
            } else {
                if (WRITE) {
                    int v = size ? (int)((win << len) >> (32 - size)) : 0;
                    if (size && v < (1 << (size - 1))) v -= (1 << size) - 1;
                    coef[block * 64 + d_zigzag[k]] = (short)v;
                }
                k++;
            }
        }
        if (k >= 64) {
            k = 0;
            slot = slot + 1 == P.bpm ? 0u : slot + 1;
            blocks++, block++;
        }
    }
    return pack_state(p, slot, k);
}

// A lane per subsequence: its interval and bit range, then jpeg_entropy.inc's settle loop from the guess "its first bit, block
// slot 0, coefficient 0" - the true state of an interval's first subsequence.
__global__ __launch_bounds__(BLOCK) void jpeg_sync_kernel(const uint32_t *__restrict__ words, const uint16_t *__restrict__ luts, JpegParams P,
                                                          const unsigned long long *__restrict__ seg_start,
                                                          const unsigned long long *__restrict__ sub_first, unsigned long long *__restrict__ entry,
                                                          const unsigned long long *__restrict__ exit_in, unsigned long long *__restrict__ exit_out,
                                                          unsigned long long *__restrict__ counts, uint32_t round, uint32_t *__restrict__ flags)
{
    __shared__ uint16_t s_short[MAX_LUTS * SHORT_ENTRIES];
    if (flags[FLAG_ERR]) return; // (set by the kernels before this one only: the same for every lane)
    load_short_tables(luts, P.n_luts, s_short);
    const unsigned long long i = (unsigned long long)blockIdx.x * BLOCK + threadIdx.x, total = sub_first[P.nseg];
    const bool active = i < total;
    unsigned long long first_bit = 0, end_bit = 0, seg_end_bits = 0;
    bool known = false;
    if (active) {
        const uint32_t s = interval_of(sub_first, P.nseg, i);
        const unsigned long long j = i - sub_first[s];
        first_bit = seg_start[s] * 8 + j * jc::SUBSEQ_BITS, seg_end_bits = seg_start[s + 1] * 8;
        end_bit = first_bit + jc::SUBSEQ_BITS < seg_end_bits ? first_bit + jc::SUBSEQ_BITS : seg_end_bits;
        known = j == 0;
    }
    settle(
        active, known, i, round, entry, exit_in, exit_out, counts, flags, [&]() { return pack_state(first_bit, 0, 0); },
        [&](unsigned long long state, unsigned long long &blocks) {
            return decode_subsequence<false>(words, luts, s_short, P, state, end_bit, seg_end_bits, blocks, nullptr, 0, 0, nullptr);
        });
}

// counts: scanned, counts[the launch's lanes] = their total.  coef was zeroed.
__global__ __launch_bounds__(BLOCK) void jpeg_write_kernel(const uint32_t *__restrict__ words, const uint16_t *__restrict__ luts, JpegParams P,
                                                           const unsigned long long *__restrict__ seg_start,
                                                           const unsigned long long *__restrict__ sub_first,
                                                           const unsigned long long *__restrict__ entry, const unsigned long long *__restrict__ counts,
                                                           short *__restrict__ coef, uint32_t *__restrict__ flags)
{
    __shared__ uint16_t s_short[MAX_LUTS * SHORT_ENTRIES];
    if (flags[FLAG_ERR] & ERR_RST) return; // (set by the kernels before this one only: the same for every lane)
    load_short_tables(luts, P.n_luts, s_short);
    const unsigned long long i = (unsigned long long)blockIdx.x * BLOCK + threadIdx.x;
    if (i == 0) flags[FLAG_SUBSEQUENCES] = (uint32_t)sub_first[P.nseg];
    if (i >= sub_first[P.nseg]) return;
    const uint32_t s = interval_of(sub_first, P.nseg, i);
    const unsigned long long j = i - sub_first[s], first_bit = seg_start[s] * 8 + j * jc::SUBSEQ_BITS, seg_end_bits = seg_start[s + 1] * 8;
    const unsigned long long end_bit = first_bit + jc::SUBSEQ_BITS < seg_end_bits ? first_bit + jc::SUBSEQ_BITS : seg_end_bits;
    // the interval's blocks: those of its MCUs, the last interval's may be fewer
    const unsigned long long first_mcu = (unsigned long long)s * P.interval;
    const unsigned long long mcus = P.mcus - first_mcu < P.interval ? P.mcus - first_mcu : P.interval, want = mcus * P.bpm;
    const unsigned long long before = counts[i] - counts[sub_first[s]], here = counts[i + 1] - counts[i];
    if (i + 1 == sub_first[s + 1] && before + here < want) atomicOr(&flags[FLAG_ERR], ERR_DATA); // the data ends before the last MCU
    if (before >= want) return; // (what follows an interval's last block is not read)
    unsigned long long blocks = 0;
    decode_subsequence<true>(words, luts, s_short, P, entry[i], end_bit, seg_end_bits, blocks, coef, first_mcu * P.bpm + before, first_mcu * P.bpm + want, flags);
}

// sums[c * mcus + m] = the sum of the DC differences of component c's blocks in MCU m
__global__ __launch_bounds__(BLOCK) void jpeg_dc_kernel(const short *__restrict__ coef, JpegParams P, unsigned long long *__restrict__ sums)
{
    const uint32_t m = blockIdx.x * BLOCK + threadIdx.x;
    if (m >= P.mcus) return;
    long long luma = 0;
    for (uint32_t slot = 0; slot < P.bpm; slot++) {
        const long long diff = coef[((unsigned long long)m * P.bpm + slot) * 64];
        if (slot < P.luma_blocks) luma += diff;
        else sums[(unsigned long long)(slot - P.luma_blocks + 1) * P.mcus + m] = (unsigned long long)diff;
    }
    sums[m] = (unsigned long long)luma;
}


thread_local uint64_t t_stats[4] = {0, 0, 0, 0}; // of the thread's last decode: intervals, subsequences, sync launches, rounds within a workgroup

} // namespace
} // namespace cvhip

using namespace cvhip;

extern "C" int cvhip_jpeg_info(const uint8_t *file, uint64_t size, uint32_t *out_info)
{
    if (!file || !out_info) return fail(CVHIP_ERR_INVALID, "jpeg_info: null argument");
    jc::Header h;
    const int rc = jc::parse(file, (size_t)size, h);
    if (rc != jc::OK) return refused("jpeg_info", rc == jc::UNSUPPORTED, h.error);
    out_info[0] = h.width, out_info[1] = h.height, out_info[2] = h.components, out_info[3] = h.hmax, out_info[4] = h.vmax;
    out_info[5] = h.focal_length_35mm;
    return CVHIP_OK;
}

extern "C" int cvhip_jpeg_last_stats(uint64_t *out_stats)
{
    if (!out_stats) return fail(CVHIP_ERR_INVALID, "jpeg_last_stats: null argument");
    for (int k = 0; k < 4; k++) out_stats[k] = t_stats[k];
    return CVHIP_OK;
}

extern "C" int cvhip_jpeg_decode(cvhip_device *dev, const uint8_t *file, uint64_t size, uint32_t format, uint32_t drop_rows, uint8_t *out,
                                 uint64_t cap, uint64_t *out_size)
{
    if (!dev || !file || !out_size || (cap && !out)) return fail(CVHIP_ERR_INVALID, "jpeg_decode: null argument");
    if (format != CVHIP_IMAGE_LUMA8 && format != CVHIP_IMAGE_RGB8) return fail(CVHIP_ERR_INVALID, "jpeg_decode: format is not CVHIP_IMAGE_LUMA8 or CVHIP_IMAGE_RGB8");
    jc::Header h;
    const int rc = jc::parse(file, (size_t)size, h);
    if (rc != jc::OK) return refused("jpeg_decode", rc == jc::UNSUPPORTED, h.error);
    if (drop_rows >= h.height) return fail(CVHIP_ERR_INVALID, "jpeg_decode: drop_rows leaves no row");
    const uint32_t channels = format == CVHIP_IMAGE_RGB8 ? 3u : 1u;
    const unsigned long long bytes = (unsigned long long)h.width * (h.height - drop_rows) * channels;
    *out_size = bytes;
    if (!cap) return CVHIP_OK;
    if (cap < bytes) return fail(CVHIP_ERR_INVALID, "jpeg_decode: the buffer is smaller than the image");
    const unsigned long long n = h.scan_end - h.scan_begin, nseg = jc::segments(h);
    JpegParams P{};
    P.width = h.width, P.height = h.height, P.ncomp = h.components, P.hmax = h.hmax, P.vmax = h.vmax, P.mcus_x = h.mcus_x, P.mcus_y = h.mcus_y;
    P.bpm = jc::blocks_per_mcu(h), P.mcus = h.mcus_x * h.mcus_y, P.interval = h.restart ? h.restart : P.mcus, P.nseg = (uint32_t)nseg;
    const unsigned long long n_blocks = (unsigned long long)P.mcus * P.bpm;
    if (n == 0) return fail(CVHIP_ERR_INVALID, "jpeg_decode: the data ends before the last MCU");
    if (n >= MAX_SCAN_BYTES) return fail(CVHIP_ERR_UNSUPPORTED, "jpeg_decode: a scan of 2^31 or more bytes");
    if (n_blocks > MAX_BLOCKS) return fail(CVHIP_ERR_UNSUPPORTED, "jpeg_decode: more than 2^25 blocks");
    if (nseg > n) return fail(CVHIP_ERR_INVALID, "jpeg_decode: a missing RSTn"); // (every marker takes two bytes)
    P.luma_blocks = h.hmax * h.vmax;
    // ---- the one upload: the components' quantisation tables, the lookups of the tables the scan uses, the scan's bytes
    int lut_of[2][4] = {{-1, -1, -1, -1}, {-1, -1, -1, -1}};
    uint32_t n_luts = 0;
    for (uint32_t c = 0; c < P.ncomp; c++) {
        if (lut_of[0][h.comp[c].td] < 0) lut_of[0][h.comp[c].td] = (int)n_luts++;
        if (lut_of[1][h.comp[c].ta] < 0) lut_of[1][h.comp[c].ta] = (int)n_luts++;
        P.dc_lut[c] = (uint32_t)lut_of[0][h.comp[c].td], P.ac_lut[c] = (uint32_t)lut_of[1][h.comp[c].ta];
    }
    P.n_luts = n_luts;
    const size_t quant_bytes = 3 * 64 * sizeof(uint16_t), lut_bytes = (size_t)n_luts * jc::LUT_ENTRIES * sizeof(uint16_t);
    std::vector<uint8_t> blob(quant_bytes + lut_bytes + (size_t)n);
    for (uint32_t c = 0; c < P.ncomp; c++) std::memcpy(blob.data() + c * 64 * sizeof(uint16_t), h.quant[h.comp[c].tq], 64 * sizeof(uint16_t));
    for (int cls = 0; cls < 2; cls++)
        for (int id = 0; id < 4; id++)
            if (lut_of[cls][id] >= 0)
                jc::build_lut(h.huff[cls][id], reinterpret_cast<uint16_t *>(blob.data() + quant_bytes) + (size_t)lut_of[cls][id] * jc::LUT_ENTRIES);
    std::memcpy(blob.data() + quant_bytes + lut_bytes, file + h.scan_begin, (size_t)n);

    CVHIP_TRY_HIP(hipSetDevice(dev->d.ordinal));
    hipStream_t s = dev->d.stream;
    CallScratch sc;
    const unsigned long long chunks = (n + 63) / 64, sub_cap = n / (jc::SUBSEQ_BITS / 8) + nseg + 1;
    const uint32_t sync_blocks = (uint32_t)((sub_cap + BLOCK - 1) / BLOCK);
    uint8_t *d_blob = nullptr, *clean = nullptr, *d_out = nullptr;
    unsigned long long *chunk_counts = nullptr, *seg_start = nullptr, *sub_first = nullptr, *states = nullptr, *counts = nullptr, *sums = nullptr;
    uint32_t *flags = nullptr, h_flags[FLAGS] = {0, 0, 0, 0};
    short *coef = nullptr;
    PlaneLayout layout(P);
    Carver carve; // one allocation, carved: an allocation costs more than most of these kernels
    const size_t at_blob = carve.reserve(blob.size()), at_clean = carve.reserve((size_t)n + 16); // (window() reads the word behind a position's own)
    const size_t at_chunks = carve.reserve(((size_t)chunks + 1) * 8), at_seg = carve.reserve(((size_t)nseg + 1) * 8), at_sub = carve.reserve(((size_t)nseg + 1) * 8);
    const size_t at_states = carve.reserve((size_t)sub_cap * 3 * 8); // entry states, and the exit states of two launches
    const size_t at_counts = carve.reserve(((size_t)sub_cap + 1) * 8), at_flags = carve.reserve(FLAGS * sizeof(uint32_t));
    const size_t at_coef = carve.reserve((size_t)n_blocks * 64 * sizeof(short)), at_sums = carve.reserve(((size_t)P.ncomp * P.mcus + 1) * 8);
    const size_t at_planes = carve.reserve(layout.total);
    uint8_t *arena = nullptr;
    hipError_t e = sc.alloc(&arena, carve.total);
    if (e == hipSuccess) e = sc.output(out, (size_t)bytes, &d_out);
    if (e != hipSuccess) return device_error("jpeg_decode", e);
    d_blob = arena + at_blob, clean = arena + at_clean;
    chunk_counts = reinterpret_cast<unsigned long long *>(arena + at_chunks), seg_start = reinterpret_cast<unsigned long long *>(arena + at_seg);
    sub_first = reinterpret_cast<unsigned long long *>(arena + at_sub), states = reinterpret_cast<unsigned long long *>(arena + at_states);
    counts = reinterpret_cast<unsigned long long *>(arena + at_counts), sums = reinterpret_cast<unsigned long long *>(arena + at_sums);
    flags = reinterpret_cast<uint32_t *>(arena + at_flags), coef = reinterpret_cast<short *>(arena + at_coef);
    if (e == hipSuccess) e = hipMemcpyAsync(d_blob, blob.data(), blob.size(), hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipMemsetAsync(seg_start, 0, ((size_t)nseg + 1) * sizeof(unsigned long long), s);
    if (e == hipSuccess) e = hipMemsetAsync(counts, 0, ((size_t)sub_cap + 1) * sizeof(unsigned long long), s);
    if (e == hipSuccess) e = hipMemsetAsync(flags, 0, FLAGS * sizeof(uint32_t), s);
    if (e == hipSuccess) e = hipMemsetAsync(coef, 0, (size_t)n_blocks * 64 * sizeof(short), s);
    if (e != hipSuccess) return device_error("jpeg_decode", e);
    const Planes &planes = layout.placed(arena + at_planes, P.ncomp);
    const uint16_t *d_quant = reinterpret_cast<const uint16_t *>(d_blob), *d_luts = reinterpret_cast<const uint16_t *>(d_blob + quant_bytes);
    const uint8_t *d_scan = d_blob + quant_bytes + lut_bytes;
    const uint32_t *words = reinterpret_cast<const uint32_t *>(clean);
    unsigned long long *entry = states, *exits[2] = {states + sub_cap, states + 2 * sub_cap};
    const dim3 block(BLOCK), byte_grid((uint32_t)((n + BLOCK - 1) / BLOCK));
    hipLaunchKernelGGL(jpeg_mark_kernel, byte_grid, block, 0, s, d_scan, n, chunk_counts);
    launch_scan_u64(chunk_counts, chunks, chunk_counts + chunks, s);
    hipLaunchKernelGGL(jpeg_compact_kernel, byte_grid, block, 0, s, d_scan, n, chunk_counts, clean, seg_start, P.nseg, flags);
    hipLaunchKernelGGL(jpeg_segments_kernel, dim3((uint32_t)((nseg + BLOCK - 1) / BLOCK)), block, 0, s, seg_start, P.nseg, chunk_counts + chunks, sub_first,
                       flags);
    launch_scan_u64(sub_first, nseg, sub_first + nseg, s);
    // ---- the states settle: within the workgroups, then across them, a launch and one flag back per round
    uint32_t launches = 0;
    int status = settle_launches("jpeg_decode", sync_blocks, flags, h_flags, FLAGS, s, launches, [&](uint32_t round, uint32_t from, uint32_t to) {
        hipLaunchKernelGGL(jpeg_sync_kernel, dim3(sync_blocks), block, 0, s, words, d_luts, P, seg_start, sub_first, entry, exits[from], exits[to], counts, round,
                           flags);
    });
    if (status != CVHIP_OK) return status;
    launch_scan_u64(counts, sub_cap, counts + sub_cap, s);
    hipLaunchKernelGGL(jpeg_write_kernel, dim3(sync_blocks), block, 0, s, words, d_luts, P, seg_start, sub_first, entry, counts, coef, flags);
    hipLaunchKernelGGL(jpeg_dc_kernel, dim3((P.mcus + BLOCK - 1) / BLOCK), block, 0, s, coef, P, sums);
    launch_scan_u64(sums, (unsigned long long)P.ncomp * P.mcus, sums + (size_t)P.ncomp * P.mcus, s);
    status = launch_tail("jpeg_decode", P, planes, coef, sums, d_quant, channels, d_out, bytes, flags, h_flags, FLAGS, s);
    if (status != CVHIP_OK) return status;
    t_stats[0] = nseg, t_stats[1] = h_flags[FLAG_SUBSEQUENCES], t_stats[2] = launches, t_stats[3] = h_flags[FLAG_ROUNDS];
    const uint32_t err = h_flags[FLAG_ERR];
    if (err & ERR_RST) return fail(CVHIP_ERR_INVALID, "jpeg_decode: a missing, surplus or misnumbered RSTn");
    if (err & ERR_CODE) return fail(CVHIP_ERR_INVALID, "jpeg_decode: a code that is not in its table");
    if (err & ERR_RUN) return fail(CVHIP_ERR_INVALID, "jpeg_decode: a run past coefficient 63");
    if (err & ERR_DATA) return fail(CVHIP_ERR_INVALID, "jpeg_decode: the data ends before the last MCU");
    return deliver("jpeg_decode", sc, out, d_out, bytes, s);
}
