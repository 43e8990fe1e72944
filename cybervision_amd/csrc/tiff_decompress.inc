// tiff_decompress.inc — what cvhip_tiff_decode (tiff_kernels.hip, DESIGN.md 4.17) and cvhip_tiff_ext_decode (tiff_ext_kernels.hip,
// DESIGN.md 4.23) share on the device: the PackBits and LZW kernels, a wave per strip - or per tile, which is a strip of
// TileLength rows of TileWidth pixels -, and the sample and result-byte rules.  Included inside the including file's namespace.
constexpr int WAVE = 64;
constexpr uint32_t BLOCK = 256;
constexpr uint32_t FLAG_ERR = 0, FLAG_CODES = 1, FLAG_CLEARS = 2, FLAG_LONGEST = 3, FLAGS = 4;
constexpr uint32_t LZW_ENTRIES = 4096;
// libtiff's table has 5119 slots and it goes on filling them when entry 4095 is taken (no code can name those); the code
// that finds no slot left - 4862 codes after the Clear - is an error there, and so here (tests/ref_tiff.py: MAX_CODES)
constexpr uint32_t LZW_MAX_CODES = 5119 - 257;

struct TiffParams {
    uint32_t width, height, rows_out, spp, sample_bytes, little, invert, predictor, rps, compressed;
    uint32_t row_bytes; // of a row in the file (below 2^31)
};

__device__ __forceinline__ uint32_t strip_rows(const TiffParams &P, uint32_t s) { return min(P.rps, P.height - s * P.rps); }

__global__ __launch_bounds__(WAVE) void tiff_packbits_kernel(const uint8_t *__restrict__ file, const uint32_t *__restrict__ offsets,
                                                             const uint32_t *__restrict__ counts, TiffParams P, uint8_t *__restrict__ raw,
                                                             uint32_t *__restrict__ flags)
{
    const uint32_t s = blockIdx.x, lane = threadIdx.x;
    const uint8_t *in = file + offsets[s];
    const uint32_t n = counts[s], need = strip_rows(P, s) * P.row_bytes;
    uint8_t *dst = raw + (unsigned long long)s * P.rps * P.row_bytes;
    uint32_t ipos = 0, opos = 0;
    while (opos < need) {
        uint32_t my_src = 0, my_out = 0, my_len = 0, my_run = 0, packets = 0;
        bool err = false;
        for (; packets < (uint32_t)WAVE && opos < need; packets++) {
            if (ipos >= n) {
                err = true;
                break;
            }
            const uint32_t header = in[ipos++];
            uint32_t len = 0, run = 0;
            if (header < 128u) {
                len = header + 1u;
                if (ipos + len > n) {
                    err = true;
                    break;
                }
            } else if (header > 128u) {
                len = 257u - header, run = 1u;
                if (ipos >= n) {
                    err = true;
                    break;
                }
            }
            if (lane == packets) my_src = ipos, my_out = opos, my_len = len, my_run = run;
            ipos += run ? (len ? 1u : 0u) : len;
            opos += len;
        }
        for (uint32_t p = 0; p < packets; p++) {
            const uint32_t src = __shfl(my_src, (int)p), out = __shfl(my_out, (int)p), len = __shfl(my_len, (int)p), run = __shfl(my_run, (int)p);
            for (uint32_t b = lane; b < len && out + b < need; b += WAVE) dst[out + b] = in[run ? src : src + b];
        }
        if (err) {
            if (lane == 0) atomicOr(&flags[FLAG_ERR], 1u);
            return;
        }
    }
}

// the bits of the codes 0 .. c - 1 after a Clear: code c is read while the next free entry is 257 + c, 9 bits wide while
// that is below 511, 10 below 1023, 11 below 2047, then 12
__device__ __forceinline__ unsigned long long lzw_bits_before(uint32_t c)
{
    return 9ull * min(c, 254u) + 10ull * min(c > 254u ? c - 254u : 0u, 512u) + 11ull * min(c > 766u ? c - 766u : 0u, 1024u) +
           12ull * (c > 1790u ? c - 1790u : 0u);
}
__device__ __forceinline__ uint32_t lzw_width(uint32_t c) { return c < 254u ? 9u : c < 766u ? 10u : c < 1790u ? 11u : 12u; }

__global__ __launch_bounds__(WAVE) void tiff_lzw_kernel(const uint8_t *__restrict__ file, const uint32_t *__restrict__ offsets,
                                                        const uint32_t *__restrict__ counts, TiffParams P, uint8_t *raw, uint32_t *__restrict__ flags)
{
    __shared__ uint32_t t_pos[LZW_ENTRIES]; // of the c-th code since the Clear: where its string begins in the strip's output
    __shared__ uint16_t t_len[LZW_ENTRIES]; // and its length (at most 3839)
    __shared__ uint32_t b_pos[WAVE + 1], b_dist[WAVE]; // of the batch: where a code's output begins; how far back its source lies (0: a literal)
    __shared__ uint8_t b_val[WAVE];
    const uint32_t s = blockIdx.x, lane = threadIdx.x;
    const uint8_t *in = file + offsets[s];
    const uint32_t n = counts[s], need = strip_rows(P, s) * P.row_bytes;
    const unsigned long long total_bits = 8ull * n;
    uint8_t *dst = raw + (unsigned long long)s * P.rps * P.row_bytes;
    unsigned long long bit = 0;
    uint32_t c0 = 0, outpos = 0, codes = 0, clears = 0, longest = 0;
    bool bad = false;
    while (outpos < need) {
        const uint32_t c = c0 + lane, w = lzw_width(c);
        const unsigned long long b = bit + (lzw_bits_before(c) - lzw_bits_before(c0));
        const bool past = b + w > total_bits;
        uint32_t code = 0;
        if (!past) {
            const unsigned long long i = b >> 3;
            const uint32_t word = (uint32_t)in[i] << 16 | (i + 1 < n ? (uint32_t)in[i + 1] : 0u) << 8 | (i + 2 < n ? (uint32_t)in[i + 2] : 0u);
            code = (word >> (24u - w - (uint32_t)(b & 7u))) & ((1u << w) - 1u);
        }
        const bool special = past || code == 256u || code == 257u;
        const uint32_t j = code - 258u;
        // above the next entry (behind a Clear only a literal), or libtiff's table overflow
        const bool invalid = !special && ((code >= 258u && j >= c) || c >= LZW_MAX_CODES);
        const unsigned long long stop = __ballot(special || invalid);
        const uint32_t f = stop ? (uint32_t)__ffsll((long long)stop) - 1u : (uint32_t)WAVE;
        const bool active = lane < f;
        int r = -1;
        uint32_t a = 0, src = 0;
        if (active) {
            if (code < 256u) a = 1;
            else if (j < c0) a = (uint32_t)t_len[j] + 1u, src = t_pos[j];
            else r = (int)(j - c0), a = 1;
        }
        const int named = r;
#pragma unroll
        for (int round = 0; round < 6; round++) { // len = len(the lane named) + 1, the chains halved per round
            const uint32_t ra = __shfl(a, r < 0 ? (int)lane : r);
            const int rr = __shfl(r, r < 0 ? (int)lane : r);
            if (r >= 0) a += ra, r = rr;
        }
        uint32_t incl = a;
#pragma unroll
        for (int d = 1; d < WAVE; d <<= 1) {
            const uint32_t t = __shfl_up(incl, d);
            if ((int)lane >= d) incl += t;
        }
        const uint32_t pos = outpos + incl - a, end = outpos + __shfl(incl, WAVE - 1);
        const uint32_t named_pos = __shfl(pos, named < 0 ? (int)lane : named);
        if (named >= 0) src = named_pos;
        if (active && c < LZW_ENTRIES) t_pos[c] = pos, t_len[c] = (uint16_t)a;
        b_pos[lane] = active ? pos : end;
        if (lane == 0) b_pos[WAVE] = end;
        b_dist[lane] = (active && code >= 258u) ? pos - src : 0u;
        b_val[lane] = (uint8_t)code;
        const bool counted = active && pos < need;
        codes += (uint32_t)__popcll(__ballot(counted));
        if (counted) longest = max(longest, a);
        __syncthreads();
        const uint32_t limit = min(end, need);
        for (uint32_t o = outpos + lane; o < limit; o += WAVE) {
            uint32_t p = o, byte;
            for (;;) {
                if (p < outpos) {
                    byte = dst[p];
                    break;
                }
                uint32_t k = 0;
#pragma unroll
                for (uint32_t step = 32; step; step >>= 1)
                    if (b_pos[k + step] <= p) k += step;
                const uint32_t dist = b_dist[k];
                if (!dist) {
                    byte = b_val[k];
                    break;
                }
                p -= dist;
            }
            dst[o] = (uint8_t)byte;
        }
        __syncthreads(); // the batch's bytes are the next batch's sources; its table entries and b_* are free again
        if (end >= need) break;
        outpos = end;
        if (f == (uint32_t)WAVE) {
            bit += lzw_bits_before(c0 + WAVE) - lzw_bits_before(c0);
            c0 += WAVE;
            continue;
        }
        const bool f_past = __shfl((int)past, (int)f) != 0;
        const uint32_t f_code = __shfl(code, (int)f), f_lo = __shfl((uint32_t)(b + w), (int)f), f_hi = __shfl((uint32_t)((b + w) >> 32), (int)f);
        if (!f_past && f_code == 256u) {
            clears++, codes++;
            bit = (unsigned long long)f_hi << 32 | f_lo;
            c0 = 0;
            continue;
        }
        bad = true; // EOI, the end of the input or a code above the next entry before the rows are full
        break;
    }
    if (bad && lane == 0) atomicOr(&flags[FLAG_ERR], 1u);
    if (lane == 0) {
        atomicAdd(&flags[FLAG_CODES], codes);
        atomicAdd(&flags[FLAG_CLEARS], clears);
    }
    if (longest) atomicMax(&flags[FLAG_LONGEST], longest);
}

// sample e of a row, an integer in the file's byte order
__device__ __forceinline__ uint32_t sample_at(const TiffParams &P, const uint8_t *row, uint32_t e)
{
    if (P.sample_bytes == 1) return row[e];
    const uint32_t first = row[2u * e], second = row[2u * e + 1u];
    return P.little ? first | second << 8 : first << 8 | second;
}

// result byte `at` of a row (channels: 1 = Luma8, 3 = RGB8)
__device__ __forceinline__ uint32_t row_byte(const TiffParams &P, const uint8_t *row, uint32_t channels, uint32_t at)
{
    const uint32_t top = P.sample_bytes == 1 ? 255u : 65535u;
    const uint32_t x = channels == 3 ? at / 3u : at, ch = channels == 3 ? at % 3u : 0u;
    uint32_t v;
    if (P.spp == 1) {
        v = sample_at(P, row, x);
        if (P.invert) v = top - v;
    } else if (channels == 3) {
        v = sample_at(P, row, x * P.spp + ch);
    } else { // into_luma8, as remembered (DESIGN.md 4.17): in the samples' own depth, then 16 -> 8 bits
        const uint32_t r = sample_at(P, row, x * P.spp), g = sample_at(P, row, x * P.spp + 1u), b = sample_at(P, row, x * P.spp + 2u);
        v = (2126u * r + 7152u * g + 722u * b) / 10000u;
    }
    return P.sample_bytes == 1 ? v : (v + 128u) / 257u;
}
