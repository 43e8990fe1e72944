// inflate_device.inc — the device functions of inflate under the stage that the PNG reader (png_decode_kernels.hip, DESIGN.md
// 4.18) and the TIFF reader's Deflate strips and tiles (tiff_ext_kernels.hip, DESIGN.md 4.23) share (inflate_stage.inc, which
// is included behind this file): the constants, the tables in LDS, peek, the symbol decode, the code build, a dynamic block's
// header and the decode of one subsequence.  Included inside the including file's namespace, behind png_decode_common.hpp and
// `namespace pd = png_decode_common`.
constexpr uint32_t WAVE = 64, BLOCK = 256; // BLOCK: lanes of a workgroup; of the chain kernel: the subsequences of a settle window
constexpr uint32_t SHORT_BITS = 10, SHORT_ENTRIES = 1u << SHORT_BITS; // codes of up to 10 bits: one LDS lookup; longer ones: the canonical walk
constexpr unsigned long long ENDED = ~0ull;                           // the state behind an end-of-block
constexpr uint32_t LIT_SYMBOLS = 288, DIST_SYMBOLS = 32, PIECE = 1024; // PIECE: bytes of a stored block's record
constexpr uint32_t F_ERR = 0, F_CHANGED = 1, F_STORED = 2, F_FIXED = 3, F_DYNAMIC = 4, F_SUBSEQUENCES = 5, F_ROUNDS = 6, F_WINDOWS = 7,
                   F_RECORDS = 8, F_SEGMENTS = 9, F_EMITTED = 10, FLAGS = 12;
constexpr uint32_t ERR_CRC = 1, ERR_ZLIB = 2, ERR_BLOCK = 4, ERR_LENGTHS = 8, ERR_TOKEN = 16, ERR_END = 32, ERR_SIZE = 64, ERR_ADLER = 128,
                   ERR_FILTER = 256, ERR_INDEX = 512, ERR_ROOM = 1024;
constexpr uint32_t WINDOW_WORDS = BLOCK * pd::SUBSEQ_BITS / 32 + 8; // a settle window's words of the stream, and those its last token may reach into
constexpr uint32_t HEADER_WORDS = 168; // 3 + 14 + 57 bits and 316 code lengths of at most 14 bits: 4 498 bits, and what a read reaches beyond

__device__ const uint8_t d_cl_order[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};

// What a block's decode needs, in LDS.  lengths: the literal/length code's at 0, the distance code's at LIT_SYMBOLS.
struct Tables {
    uint16_t lit_short[SHORT_ENTRIES], dist_short[SHORT_ENTRIES]; // [the next SHORT_BITS bits] = code length << 9 | symbol, 0: walk
    uint16_t lit_sym[LIT_SYMBOLS], dist_sym[DIST_SYMBOLS];        // the symbols by (length, symbol)
    uint16_t lit_count[16], dist_count[16];                       // codes per length
    uint16_t codes[LIT_SYMBOLS + DIST_SYMBOLS];
    uint16_t work[32];
    uint8_t lengths[LIT_SYMBOLS + DIST_SYMBOLS];
    uint8_t cl_lengths[19];
};

// the 32 bits of the stream from bit p on, first bit lowest (the stream is followed by 32 zero bytes; p <= its bits + 64)
__device__ __forceinline__ uint32_t peek(const uint32_t *words, unsigned long long p, unsigned long long word_base = 0)
{
    const unsigned long long w = (p >> 5) - word_base; // (words: the stream from its word `word_base` on)
    const unsigned long long v = (unsigned long long)words[w] | (unsigned long long)words[w + 1] << 32;
    return (uint32_t)(v >> (p & 31u));
}

// the canonical walk (a bit at a time, the code's first bit first) -> code length << 9 | symbol, 0: no such code
__device__ __forceinline__ uint32_t walk_symbol(const uint16_t *count, const uint16_t *syms, uint32_t bits)
{
    int code = 0, first = 0, index = 0;
    for (int len = 1; len <= 15; len++) {
        code |= (int)(bits & 1u);
        bits >>= 1;
        const int n = count[len];
        if (code - n < first) return (uint32_t)len << 9 | syms[index + (code - first)];
        index += n, first += n;
        first <<= 1, code <<= 1;
    }
    return 0;
}
__device__ __forceinline__ uint32_t decode_symbol(const uint16_t *short_table, const uint16_t *count, const uint16_t *syms, uint32_t bits)
{
    const uint32_t entry = short_table[bits & (SHORT_ENTRIES - 1u)];
    return entry ? entry : walk_symbol(count, syms, bits);
}

// One lane: count[], syms[] and the canonical codes of n code lengths -> 0 or ERR_LENGTHS.  Over-subscribed lengths are
// refused, incomplete ones too unless no code is longer than one bit (zlib's rule: the single-code table of RFC 1951, and
// the table without codes, whose use is the error).
__device__ __forceinline__ uint32_t build_code(const uint8_t *len, uint32_t n, uint16_t *count, uint16_t *syms, uint16_t *codes, uint16_t *work)
{
    uint16_t *offs = work, *next = work + 16;
    for (uint32_t l = 0; l < 16; l++) count[l] = 0;
    for (uint32_t s = 0; s < n; s++) count[len[s]]++;
    count[0] = 0;
    int left = 1;
    uint32_t longest = 0, code = 0;
    offs[0] = 0, offs[1] = 0, next[0] = 0;
    for (uint32_t l = 1; l <= 15; l++) {
        left = left * 2 - (int)count[l];
        if (left < 0) return ERR_LENGTHS;
        if (count[l]) longest = l;
        code = (code + count[l - 1]) << 1;
        next[l] = (uint16_t)code;
        if (l < 15) offs[l + 1] = (uint16_t)(offs[l] + count[l]);
    }
    for (uint32_t s = 0; s < n; s++) {
        const uint32_t l = len[s];
        if (!l) continue;
        syms[offs[l]++] = (uint16_t)s;
        codes[s] = next[l]++;
    }
    return left > 0 && longest > 1 ? ERR_LENGTHS : 0u;
}

// One lane: HLIT, HDIST, HCLEN and the code lengths of the dynamic block whose header's first three bits end at p ->
// T.lengths, *p_out (an LDS word: a reference to a register would put it into scratch memory) the bit behind them; 0,
// ERR_LENGTHS or ERR_END.
__device__ __forceinline__ uint32_t read_dynamic_lengths(const uint32_t *words, unsigned long long word_base, unsigned long long p,
                                                         unsigned long long total_bits, Tables &T, unsigned long long *p_out)
{
    if (p + 14 > total_bits) return ERR_END;
    uint32_t bits = peek(words, p, word_base);
    const uint32_t hlit = (bits & 31u) + 257u, hdist = ((bits >> 5) & 31u) + 1u, hclen = ((bits >> 10) & 15u) + 4u;
    p += 14;
    if (hlit > 286 || hdist > 30) return ERR_LENGTHS;
    if (p + 3ull * hclen > total_bits) return ERR_END;
    for (uint32_t i = 0; i < 19; i++) {
        T.cl_lengths[d_cl_order[i]] = i < hclen ? (uint8_t)(peek(words, p, word_base) & 7u) : (uint8_t)0;
        if (i < hclen) p += 3;
    }
    if (build_code(T.cl_lengths, 19, T.dist_count, T.dist_sym, T.codes, T.work)) return ERR_LENGTHS;
    // the code-length code has at most 7 bits: one lookup in the (still empty) distance lookup's first 128 entries
    for (uint32_t s = 0; s < 19; s++) {
        const uint32_t l = T.cl_lengths[s];
        if (l)
            for (uint32_t k = __brev((uint32_t)T.codes[s]) >> (32 - l); k < 128; k += 1u << l) T.dist_short[k] = (uint16_t)(l << 9 | s);
    }
    const uint32_t want = hlit + hdist;
    uint32_t n = 0;
    while (n < want) {
        if (p >= total_bits) return ERR_END;
        const uint32_t entry = T.dist_short[peek(words, p, word_base) & 127u];
        if (!entry) return ERR_LENGTHS;
        p += entry >> 9;
        const uint32_t sym = entry & 511u;
        if (sym < 16) {
            T.lengths[n++] = (uint8_t)sym;
            continue;
        }
        bits = peek(words, p, word_base);
        uint32_t value = 0, repeat;
        if (sym == 16) {
            if (n == 0) return ERR_LENGTHS; // nothing to repeat
            value = T.lengths[n - 1], repeat = 3 + (bits & 3u), p += 2;
        } else if (sym == 17) repeat = 3 + (bits & 7u), p += 3;
        else repeat = 11 + (bits & 127u), p += 7;
        if (n + repeat > want) return ERR_LENGTHS; // past HLIT + HDIST
        for (uint32_t k = 0; k < repeat; k++) T.lengths[n++] = (uint8_t)value;
    }
    if (p > total_bits) return ERR_END;
    *p_out = p;
    for (uint32_t k = 0; k < 128; k++) T.dist_short[k] = 0;
    // the distance lengths to their place (upwards: from the last one), zeros behind both
    for (uint32_t k = hdist; k-- > 0;) T.lengths[LIT_SYMBOLS + k] = T.lengths[hlit + k];
    for (uint32_t s = hlit; s < LIT_SYMBOLS; s++) T.lengths[s] = 0;
    for (uint32_t s = LIT_SYMBOLS + hdist; s < LIT_SYMBOLS + DIST_SYMBOLS; s++) T.lengths[s] = 0;
    return 0;
}

// The whole workgroup: the tables of the fixed (btype 1) or dynamic (btype 2) block whose three header bits end at p ->
// 0 or the error; *s_p = the block's first token bit.  s_err, s_p: LDS words of the caller.
__device__ __forceinline__ uint32_t load_tables(const uint32_t *words, unsigned long long word_base, unsigned long long p, unsigned long long total_bits,
                                                uint32_t btype, Tables &T, uint32_t *s_err, unsigned long long *s_p)
{
    if (btype == 1)
        for (uint32_t s = threadIdx.x; s < LIT_SYMBOLS + DIST_SYMBOLS; s += BLOCK)
            T.lengths[s] = (uint8_t)(s < 144 ? 8 : s < 256 ? 9 : s < 280 ? 7 : s < LIT_SYMBOLS ? 8 : 5);
    for (uint32_t k = threadIdx.x; k < SHORT_ENTRIES; k += BLOCK) T.lit_short[k] = 0, T.dist_short[k] = 0;
    __syncthreads();
    if (threadIdx.x == 0) {
        *s_p = p;
        uint32_t err = btype == 2 ? read_dynamic_lengths(words, word_base, p, total_bits, T, s_p) : 0u;
        if (!err && T.lengths[256] == 0) err = ERR_LENGTHS; // no end-of-block
        if (!err) err = build_code(T.lengths, LIT_SYMBOLS, T.lit_count, T.lit_sym, T.codes, T.work);
        if (!err) err = build_code(T.lengths + LIT_SYMBOLS, DIST_SYMBOLS, T.dist_count, T.dist_sym, T.codes + LIT_SYMBOLS, T.work);
        *s_err = err;
    }
    __syncthreads();
    if (*s_err) return *s_err;
    for (uint32_t s = threadIdx.x; s < LIT_SYMBOLS + DIST_SYMBOLS; s += BLOCK) {
        const uint32_t l = T.lengths[s];
        if (!l || l > SHORT_BITS) continue;
        const bool lit = s < LIT_SYMBOLS;
        uint16_t *table = lit ? T.lit_short : T.dist_short;
        const uint16_t entry = (uint16_t)(l << 9 | (lit ? s : s - LIT_SYMBOLS));
        for (uint32_t k = __brev((uint32_t)T.codes[s]) >> (32 - l); k < SHORT_ENTRIES; k += 1u << l) table[k] = entry;
    }
    __syncthreads();
    return 0;
}

// Decodes whole tokens from bit p while p < end_bit -> the exit state: the next token's bit, or ENDED behind an
// end-of-block (eob_after = the bit behind it).  count += the output bytes.  WRITE: output byte o on gets its literal
// (raw) and its source index (src), below `filtered`; what the file does wrong is flagged.
template <bool WRITE>
__device__ __forceinline__ unsigned long long decode_subsequence(const uint32_t *words, unsigned long long word_base, const Tables &T, unsigned long long p,
                                                                 unsigned long long end_bit, unsigned long long &count,
                                                                 unsigned long long &eob_after, uint8_t *__restrict__ raw, uint32_t *__restrict__ src,
                                                                 unsigned long long o, unsigned long long filtered, uint32_t *__restrict__ flags)
{
    while (p < end_bit) {
        uint32_t bits = peek(words, p, word_base);
        uint32_t entry = decode_symbol(T.lit_short, T.lit_count, T.lit_sym, bits);
        if (!entry) { // no such code
            if (WRITE) atomicOr(&flags[F_ERR], ERR_TOKEN);
            p += 1;
            continue;
        }
        const uint32_t sym = entry & 511u;
        p += entry >> 9;
        if (sym < 256) {
            if (WRITE && o < filtered) raw[o] = (uint8_t)sym, src[o] = (uint32_t)o;
            o++, count++;
            continue;
        }
        if (sym == 256) {
            eob_after = p;
            return ENDED;
        }
        if (sym >= 286) {
            if (WRITE) atomicOr(&flags[F_ERR], ERR_TOKEN);
            continue;
        }
        bits >>= entry >> 9;
        uint32_t length = 258;
        if (sym < 265) length = sym - 254;
        else if (sym < 285) {
            const uint32_t e = (sym - 261) >> 2;
            length = 3 + ((4 + ((sym - 261) & 3u)) << e) + (bits & ((1u << e) - 1u));
            p += e;
        }
        bits = peek(words, p, word_base);
        entry = decode_symbol(T.dist_short, T.dist_count, T.dist_sym, bits);
        if (!entry) {
            if (WRITE) atomicOr(&flags[F_ERR], ERR_TOKEN);
            p += 1;
            continue;
        }
        const uint32_t dsym = entry & 511u;
        p += entry >> 9;
        if (dsym >= 30) {
            if (WRITE) atomicOr(&flags[F_ERR], ERR_TOKEN);
            continue;
        }
        bits >>= entry >> 9;
        uint32_t distance = dsym + 1;
        if (dsym >= 4) {
            const uint32_t e = (dsym >> 1) - 1;
            distance = 1 + ((2 + (dsym & 1u)) << e) + (bits & ((1u << e) - 1u));
            p += e;
        }
        if (WRITE) {
            const bool far = distance > o; // before the first output byte
            if (far) atomicOr(&flags[F_ERR], ERR_TOKEN);
            for (uint32_t k = 0; k < length && o + k < filtered; k++) src[o + k] = (uint32_t)(far ? o + k : o + k - distance);
        }
        o += length, count += length;
    }
    return p;
}
