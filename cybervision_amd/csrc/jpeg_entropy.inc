// jpeg_entropy.inc — what cvhip_jpeg_decode (jpeg_kernels.hip, DESIGN.md 4.16) and cvhip_jpeg_progressive_decode (jpeg_prog_kernels.hip,
// DESIGN.md 4.22) share in front of their block stores: what a byte of a scan is, the window of the clean buffer a symbol is read
// from, the short-code tables in LDS, the search for an interval or a scan, and the self-synchronising settle loop with the chain
// of launches that drives it across workgroups.  Included behind jpeg_tail.inc inside namespace cvhip { namespace { of each of the
// two sources: everything here is compiled into both, nothing is called across them.

constexpr uint32_t KIND_DROP = 0, KIND_DATA = 1, KIND_RST = 2;
constexpr uint32_t SHORT_BITS = 10, SHORT_ENTRIES = 1u << SHORT_BITS; // the codes of up to 10 bits of a table, in LDS

__device__ const uint8_t d_zigzag[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                                         41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                                         30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

// What byte i of a scan's bytes[begin .. end) is.  One byte back and one ahead decide it (tests/ref_jpeg.py: segments).  An FF
// that the range ends behind is a data byte with LAST_FF_IS_DATA (the baseline scan) and dropped without (a progressive scan:
// tests/ref_jpeg_prog.py: intervals - the data ends there).
template <bool LAST_FF_IS_DATA, typename Index>
__device__ __forceinline__ uint32_t classify(const uint8_t *__restrict__ bytes, Index begin, Index end, Index i)
{
    const uint32_t b = bytes[i], prev = i > begin ? bytes[i - 1] : 0u, next = i + 1 < end ? bytes[i + 1] : 0x100u;
    if (b == 0xFF) return (next == 0x00 || (LAST_FF_IS_DATA && next == 0x100)) ? KIND_DATA : KIND_DROP; // stuffed; fill, or a marker's first byte
    if (prev == 0xFF) {
        if (b == 0x00) return KIND_DROP;
        if (b >= 0xD0 && b <= 0xD7) return KIND_RST;
    }
    return KIND_DATA;
}

// the last k of 0 .. n - 1 with key(k) <= x, for keys that ascend from key(0) <= x
template <typename Key, typename X> __device__ __forceinline__ uint32_t last_not_above(uint32_t n, X x, Key &&key)
{
    uint32_t lo = 0, hi = n;
    while (hi - lo > 1) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (key(mid) <= x) lo = mid;
        else hi = mid;
    }
    return lo;
}

// the interval of subsequence i: the last s with sub_first[s] <= i (sub_first[n] = all subsequences > i)
__device__ __forceinline__ uint32_t interval_of(const unsigned long long *__restrict__ sub_first, uint32_t n, unsigned long long i)
{
    return last_not_above(n, i, [&](uint32_t s) { return sub_first[s]; });
}

// A state: the next bit (of the clean buffer) | the block's number in its MCU << 40 | the zig-zag index << 44
__device__ __forceinline__ unsigned long long pack_state(unsigned long long p, uint32_t slot, uint32_t k)
{
    return p | (unsigned long long)slot << 40 | (unsigned long long)k << 44;
}

// the 64 bits of the clean buffer (big-endian) from word wi on, those at and past seg_end_bits read as ones; 32 wi < seg_end_bits
__device__ __forceinline__ unsigned long long load_window(const uint32_t *__restrict__ words, unsigned long long wi, unsigned long long seg_end_bits)
{
    const unsigned long long base = wi << 5;
    unsigned long long v = (unsigned long long)__builtin_bswap32(words[wi]) << 32 | __builtin_bswap32(words[wi + 1]);
    if (seg_end_bits < base + 64) v |= ~0ull >> (seg_end_bits - base); // (1 .. 63 valid bits)
    return v;
}

// a table's entry as its short table's: itself where the code has at most SHORT_BITS bits, else 0 (look in the whole table)
__device__ __forceinline__ uint16_t short_entry(uint16_t entry) { return (entry >> 8) <= SHORT_BITS ? entry : (uint16_t)0; }

// s_short[t][the next SHORT_BITS bits] = short_entry of table t's entry there, by the BLOCK lanes of a workgroup.  Nearly every
// symbol of a photograph is decoded from LDS; the whole tables stay in global memory.  (jpeg_prog_refine_kernel fills its one
// table, a wave wide, in its own text: through a function its registers come out renamed, DESIGN.md 4.22.)
__device__ __forceinline__ void load_short_tables(const uint16_t *__restrict__ luts, uint32_t n_luts, uint16_t *s_short)
{
    for (uint32_t at = threadIdx.x; at < n_luts * SHORT_ENTRIES; at += BLOCK)
        s_short[at] = short_entry(luts[(size_t)(at >> SHORT_BITS) * jc::LUT_ENTRIES + ((at & (SHORT_ENTRIES - 1u)) << (16 - SHORT_BITS))]);
    __syncthreads();
}

// The body of a sync kernel behind its prologue, for subsequence i of the launch (active: there is one; known: it is an
// interval's first, whose guess is its true state).  round 0: every subsequence from guess(), settled within the workgroup: a lane
// decodes again from its left neighbour's exit state until no state in the workgroup changes.  round > 0: the first lane of a
// workgroup takes exit_in[i - 1], the launch before's; flags[FLAG_CHANGED] is set when a workgroup's last exit state differs
// from exit_in's.  decode(state, blocks) decodes the lane's subsequence from `state` -> the exit state, blocks += the blocks
// completed.
template <typename Guess, typename Decode>
__device__ __forceinline__ void settle(bool active, bool known, unsigned long long i, uint32_t round, unsigned long long *__restrict__ entry,
                                       const unsigned long long *__restrict__ exit_in, unsigned long long *__restrict__ exit_out,
                                       unsigned long long *__restrict__ counts, uint32_t *__restrict__ flags, Guess &&guess, Decode &&decode)
{
    __shared__ unsigned long long s_exit[BLOCK];
    unsigned long long cur_entry = 0, cur_exit = 0, blocks = 0, old_exit = 0;
    if (active) {
        if (round == 0) {
            cur_entry = guess();
            cur_exit = decode(cur_entry, blocks);
        } else {
            cur_entry = entry[i], cur_exit = old_exit = exit_in[i], blocks = counts[i];
        }
    }
    s_exit[threadIdx.x] = cur_exit;
    uint32_t rounds = 0;
    for (;;) {
        __syncthreads();
        unsigned long long want = cur_entry;
        if (active && !known) {
            if (threadIdx.x) want = s_exit[threadIdx.x - 1];
            else if (round) want = exit_in[i - 1];
        }
        const bool change = want != cur_entry;
        if (!__syncthreads_or(change)) break; // (and every lane has read before any lane writes)
        if (change) {
            cur_entry = want, blocks = 0;
            cur_exit = decode(cur_entry, blocks);
            s_exit[threadIdx.x] = cur_exit;
        }
        rounds++;
    }
    if (active) {
        entry[i] = cur_entry, exit_out[i] = cur_exit, counts[i] = blocks;
        if (threadIdx.x == BLOCK - 1 && (round == 0 || cur_exit != old_exit)) atomicOr(&flags[FLAG_CHANGED], 1u);
    }
    if (threadIdx.x == 0 && rounds) atomicMax(&flags[FLAG_ROUNDS], rounds);
}

// The states settle within the workgroups, then across them, a launch and one flag back per round: launch(round, from, to)
// enqueues the sync kernel's launch `round` over sync_blocks workgroups, which reads the exit states of buffer `from` and writes
// those of buffer `to`.  h_flags takes flags[0 .. n_flags) of the last launch that was waited for.  -> launches
template <typename Launch>
int settle_launches(const char *what, uint32_t sync_blocks, uint32_t *flags, uint32_t *h_flags, size_t n_flags, hipStream_t s, uint32_t &launches,
                    Launch &&launch)
{
    launch(0u, 0u, 0u);
    launches = 1;
    for (uint32_t from = 0; sync_blocks > 1; from ^= 1u, launches++) {
        if (launches > sync_blocks + 1) return fail(CVHIP_ERR_DEVICE, std::string(what) + ": the decoder's states did not settle");
        hipError_t e = hipGetLastError();
        if (e == hipSuccess) e = hipMemsetAsync(flags + FLAG_CHANGED, 0, sizeof(uint32_t), s);
        if (e != hipSuccess) return device_error(what, e);
        launch(launches, from, from ^ 1u);
        e = hipGetLastError();
        if (e == hipSuccess) e = hipMemcpyAsync(h_flags, flags, n_flags * sizeof(uint32_t), hipMemcpyDeviceToHost, s);
        if (e == hipSuccess) e = hipStreamSynchronize(s);
        if (e != hipSuccess) return device_error(what, e);
        if (h_flags[FLAG_ERR] || !h_flags[FLAG_CHANGED]) {
            launches++;
            break;
        }
    }
    return CVHIP_OK;
}
