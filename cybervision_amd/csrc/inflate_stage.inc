// inflate_stage.inc — the inflate stage of the PNG reader (png_decode_kernels.hip, DESIGN.md 4.18) and of the TIFF reader's
// Deflate strips and tiles (tiff_ext_kernels.hip, DESIGN.md 4.23), once: the five kernels that turn a table of zlib streams
// into their bytes, and the host sequence that drives them.  Included behind inflate_device.inc inside the including file's
// namespace, behind `namespace pc = png_common`: everything here is compiled into both, nothing is called across them.
//
// A file is a table of streams: stream s is counts[s] bytes at file + offsets[s], a multiple of four, with 32 zero bytes behind
// it, and inflates to raw[s x stream_bytes ..).  A PNG file's IDAT data is a table of one stream.
//
//   inflate_chain_kernel    a workgroup per stream walks its chain of deflate blocks, whose headers can only be found in order.  A
//                           dynamic block's code lengths are read by one lane, the tables are built in LDS; inside the block
//                           the decode is the self-synchronising one of jpeg_sync_kernel: a lane per subsequence of
//                           SUBSEQ_BITS bits, the state is the bit offset of a whole token, lanes decode again from their left
//                           neighbour's exit until nothing changes.  A window of 256 subsequences, its part of the stream in
//                           LDS, settles completely before the next one starts from its last exit, so nothing waits for
//                           another workgroup.  A lane does not take over "ended" from its left (a false end-of-block would
//                           be handed down the window a lane a round); only the first end-of-block of the settled chain, in
//                           front of which every lane holds its true state, ends the block.  Out come records (entry state,
//                           output position) per subsequence, and per 1024 bytes of a stored block a (source, position, length)
//                           record.  A settled window's records get their output positions at once, by a scan over the
//                           workgroup that carries the stream's running count, so the positions restart at every stream; windows
//                           and records take the next free slots of two arrays shared by all streams - one workgroup is handed
//                           0, 1, 2, ... in its own order
//   inflate_write_kernel    a workgroup per window of any stream: the block's tables again (from its header), one more decode
//                           from the settled states: literals to the stream's bytes, and per output byte its source index inside
//                           the stream (itself for a literal, o - distance for a copy)
//   inflate_resolve_kernel  pointer doubling over the source indices, inside each stream, two buffers, until a launch changes nothing
//   inflate_gather_kernel   every byte from its literal; the Adler-32 sums of every stream
//   inflate_finish_kernel   a lane per stream: the Adler-32 behind its final block against those sums
// A decode from a wrong state is harmless: every read is bounded by the stream's end (32 zero bytes follow it), every step
// consumes at least one bit, and a code that does not exist consumes one.  In the write pass, whose states are the true
// ones, the same events are the file's errors.  A distance that reaches in front of its stream's first byte is the file's
// error; no index leaves its stream.
constexpr uint32_t WIN_SLOTS = 4; // a window: header bit | BTYPE << 40 | records << 44; the first subsequence's first bit; the first record; the stream

// Every stream but the last inflates to stream_bytes bytes (below 2^31), the last to what is left of `total`.
struct InflateLayout {
    uint32_t stream_bytes;
    unsigned long long total; // the inflated bytes of all streams
};

// stream s inflates to this many bytes
__device__ __forceinline__ uint32_t stream_need(const InflateLayout &L, uint32_t s)
{
    return (uint32_t)min((unsigned long long)L.stream_bytes, L.total - (unsigned long long)s * L.stream_bytes);
}

// ---- the chains of blocks: stream blockIdx.x ---------------------------------------------------------------------------------------
__global__ __launch_bounds__(BLOCK) void inflate_chain_kernel(const uint8_t *__restrict__ file, const uint32_t *__restrict__ offsets,
                                                              const uint32_t *__restrict__ counts, InflateLayout L, unsigned long long *__restrict__ win,
                                                              unsigned long long max_windows, unsigned long long *__restrict__ rec_entry,
                                                              unsigned long long *__restrict__ rec_out, uint32_t *__restrict__ rec_count,
                                                              unsigned long long max_records, uint32_t *__restrict__ flags,
                                                              unsigned long long *__restrict__ end_bit)
{
    __shared__ Tables T;
    __shared__ uint32_t s_stream[WINDOW_WORDS];
    __shared__ unsigned long long s_exit[BLOCK], s_p, s_eob, s_wave[BLOCK / WAVE], s_slot[2];
    __shared__ uint32_t s_err, s_btype, s_final, s_first, s_len;
    const uint32_t tid = threadIdx.x, lane = tid % WAVE, wave = tid / WAVE, stream = blockIdx.x;
    const uint32_t *words = reinterpret_cast<const uint32_t *>(file + offsets[stream]);
    const unsigned long long n_bytes = counts[stream], total_bits = n_bytes * 8, need = stream_need(L, stream);
    if (tid == 0) { // the zlib header
        uint32_t err = 0;
        if (n_bytes < 2) err = ERR_END;
        else {
            const uint32_t cmf = words[0] & 255u, flg = (words[0] >> 8) & 255u;
            if ((cmf & 15u) != 8 || (cmf >> 4) > 7 || (flg & 32u) || ((cmf << 8 | flg) % 31u)) err = ERR_ZLIB;
        }
        s_err = err;
    }
    __syncthreads();
    uint32_t err = s_err, stored = 0, fixed = 0, dynamic = 0, most_rounds = 0, subsequences = 0, windows = 0;
    unsigned long long p = 16, out_pos = 0; // out_pos: the stream's output in front of the next record
    bool final_seen = false;
    // the next `records` records and the next window of the shared arrays -> s_slot, or ERR_ROOM
    auto take = [&](unsigned long long records) -> bool {
        __syncthreads();
        if (tid == 0) s_slot[0] = atomicAdd(&flags[F_EMITTED], 1u), s_slot[1] = atomicAdd(&flags[F_RECORDS], (uint32_t)records);
        __syncthreads();
        return s_slot[0] + 1 <= max_windows && s_slot[1] + records <= max_records;
    };
    // (every block takes at least three bits: the bound holds whatever the file says)
    for (unsigned long long blocks = 0; !err && !final_seen && blocks <= total_bits; blocks++) {
        const unsigned long long header = p;
        __syncthreads(); // (the shared words of the block before are read)
        if (tid == 0) {
            uint32_t e = 0;
            unsigned long long q = p + 3;
            if (q > total_bits) e = ERR_END;
            else {
                const uint32_t b = peek(words, p);
                s_final = b & 1u, s_btype = (b >> 1) & 3u;
                if (s_btype == 3) e = ERR_BLOCK;
                else if (s_btype == 0) {
                    q = (q + 7) & ~7ull;
                    if (q + 32 > total_bits) e = ERR_END;
                    else {
                        const uint32_t v = peek(words, q);
                        s_len = v & 0xFFFFu;
                        if ((s_len ^ 0xFFFFu) != (v >> 16)) e = ERR_BLOCK;
                        q += 32;
                        if (!e && q + 8ull * s_len > total_bits) e = ERR_END;
                    }
                }
            }
            s_err = e, s_p = q;
        }
        __syncthreads();
        err = s_err;
        if (err) break;
        const uint32_t btype = s_btype;
        final_seen = s_final != 0;
        if (btype == 0) { // a stored block: a record per PIECE bytes
            stored++;
            const unsigned long long first_byte = s_p >> 3, length = s_len;
            for (unsigned long long done = 0; done < length; done += (unsigned long long)BLOCK * PIECE) {
                const unsigned long long pieces = min((unsigned long long)BLOCK, (length - done + PIECE - 1) / PIECE);
                if (!take(pieces)) {
                    err = ERR_ROOM;
                    break;
                }
                const unsigned long long w = s_slot[0], r = s_slot[1];
                if (tid < pieces) {
                    const unsigned long long at = done + (unsigned long long)tid * PIECE;
                    rec_entry[r + tid] = first_byte + at, rec_out[r + tid] = out_pos + at, rec_count[r + tid] = (uint32_t)min((unsigned long long)PIECE, length - at);
                }
                if (tid == 0) win[WIN_SLOTS * w] = header | pieces << 44, win[WIN_SLOTS * w + 1] = 0, win[WIN_SLOTS * w + 2] = r, win[WIN_SLOTS * w + 3] = stream;
                windows++;
            }
            out_pos += length;
            p = s_p + 8 * length;
            continue;
        }
        if (btype == 1) fixed++;
        else dynamic++;
        // the header's words to LDS first (HEADER_WORDS hold the longest one): one lane reads them, a load from memory each time otherwise
        const unsigned long long header_word = p >> 5;
        for (uint32_t k = tid; k < HEADER_WORDS; k += BLOCK) s_stream[k] = header_word + k < (n_bytes + 32) / 4 ? words[header_word + k] : 0u;
        __syncthreads();
        err = load_tables(s_stream, header_word, p + 3, total_bits, btype, T, &s_err, &s_p);
        if (err) break;
        unsigned long long base = s_p, entry0 = s_p;
        bool block_done = false;
        while (!err && !block_done) { // a window of BLOCK subsequences; each takes BLOCK x SUBSEQ_BITS bits of the stream
            if (base >= total_bits) {
                err = ERR_END; // the stream ends before the block's end-of-block
                break;
            }
            windows++;
            const unsigned long long first_bit = base + (unsigned long long)tid * pd::SUBSEQ_BITS;
            const bool active = first_bit < total_bits;
            const unsigned long long end_bit_here = min(first_bit + pd::SUBSEQ_BITS, total_bits);
            const unsigned long long n_active = min((unsigned long long)BLOCK, (total_bits - base + pd::SUBSEQ_BITS - 1) / pd::SUBSEQ_BITS);
            // the window's part of the stream to LDS: in this one workgroup every load from memory would be waited for
            const unsigned long long word_base = base >> 5, stream_words = (n_bytes + 32) / 4;
#pragma unroll 8
            for (uint32_t k = tid; k < WINDOW_WORDS; k += BLOCK) s_stream[k] = word_base + k < stream_words ? words[word_base + k] : 0u;
            __syncthreads();
            unsigned long long cur_entry = tid == 0 ? entry0 : first_bit, cur_exit = ENDED, count = 0, eob_after = 0;
            if (active)
                cur_exit = cur_entry >= end_bit_here
                               ? cur_entry
                               : decode_subsequence<false>(s_stream, word_base, T, cur_entry, end_bit_here, count, eob_after, nullptr, nullptr, 0, 0, nullptr);
            s_exit[tid] = cur_exit;
            if (tid == 0) s_first = BLOCK;
            uint32_t rounds = 0;
            for (uint32_t r = 0; r <= BLOCK; r++) { // lane k holds its true state after k rounds
                __syncthreads();
                // (a left neighbour that met an end-of-block says nothing about this lane: were it the block's end, this lane
                // would not count; were it a false one, adopting it would hand "ended" down the window a lane a round)
                unsigned long long want = (tid && active) ? s_exit[tid - 1] : cur_entry;
                if (want == ENDED) want = cur_entry;
                const bool change = want != cur_entry;
                if (!__syncthreads_or(change)) break; // (and every lane has read before any lane writes)
                if (change) {
                    cur_entry = want, count = 0, eob_after = 0;
                    cur_exit = cur_entry >= end_bit_here
                                   ? cur_entry
                                   : decode_subsequence<false>(s_stream, word_base, T, cur_entry, end_bit_here, count, eob_after, nullptr, nullptr, 0, 0, nullptr);
                    s_exit[tid] = cur_exit;
                }
                rounds++;
            }
            most_rounds = max(most_rounds, rounds);
            const bool ends_here = active && cur_exit == ENDED; // the first such lane: every lane before it holds its true state
            if (ends_here) atomicMin(&s_first, tid);
            __syncthreads();
            const uint32_t jend = s_first;
            const unsigned long long emit = jend < BLOCK ? jend + 1 : n_active;
            subsequences += (uint32_t)emit;
            if (__syncthreads_or(tid < emit && count != 0)) { // (a window without output needs no write pass)
                // the records' output positions: the counts scanned over the workgroup, behind the stream's count so far
                const unsigned long long mine = tid < emit ? count : 0ull;
                unsigned long long incl = mine;
#pragma unroll
                for (uint32_t d = 1; d < WAVE; d <<= 1) {
                    const unsigned long long t = __shfl_up(incl, d);
                    if (lane >= d) incl += t;
                }
                if (lane == WAVE - 1) s_wave[wave] = incl;
                __syncthreads();
                unsigned long long before = 0, all = 0;
#pragma unroll
                for (uint32_t k = 0; k < BLOCK / WAVE; k++) {
                    if (k < wave) before += s_wave[k];
                    all += s_wave[k];
                }
                if (!take(emit)) {
                    err = ERR_ROOM;
                    break;
                }
                const unsigned long long w = s_slot[0], r = s_slot[1];
                if (tid < emit) rec_entry[r + tid] = cur_entry, rec_out[r + tid] = out_pos + before + incl - mine, rec_count[r + tid] = 0;
                if (tid == 0)
                    win[WIN_SLOTS * w] = header | (unsigned long long)btype << 40 | emit << 44, win[WIN_SLOTS * w + 1] = base, win[WIN_SLOTS * w + 2] = r,
                                    win[WIN_SLOTS * w + 3] = stream;
                out_pos += all;
            }
            if (jend < BLOCK) {
                if (tid == jend) s_eob = eob_after;
                __syncthreads();
                p = s_eob;
                if (p > total_bits) err = ERR_END;
                block_done = true;
            } else if (n_active < BLOCK) {
                err = ERR_END;
            } else {
                entry0 = s_exit[BLOCK - 1];
                base += (unsigned long long)BLOCK * pd::SUBSEQ_BITS;
                __syncthreads();
            }
        }
    }
    if (!err && !final_seen) err = ERR_END;
    if (!err && (p + 7) / 8 + 4 > n_bytes) err = ERR_END; // the stream ends inside the Adler-32
    if (!err && out_pos != need) err = ERR_SIZE;          // not the stream's bytes: fewer, or more
    if (tid == 0) {
        if (err) atomicOr(&flags[F_ERR], err);
        atomicAdd(&flags[F_STORED], stored), atomicAdd(&flags[F_FIXED], fixed), atomicAdd(&flags[F_DYNAMIC], dynamic);
        atomicAdd(&flags[F_SUBSEQUENCES], subsequences), atomicAdd(&flags[F_WINDOWS], windows), atomicMax(&flags[F_ROUNDS], most_rounds);
        end_bit[stream] = p;
    }
}

// a workgroup per window, on the window's stream: positions and source indices inside the stream
__global__ __launch_bounds__(BLOCK) void inflate_write_kernel(const uint8_t *__restrict__ file, const uint32_t *__restrict__ offsets,
                                                              const uint32_t *__restrict__ counts, InflateLayout L, const unsigned long long *__restrict__ win,
                                                              const unsigned long long *__restrict__ rec_entry, const unsigned long long *__restrict__ rec_out,
                                                              const uint32_t *__restrict__ rec_count, uint8_t *__restrict__ raw, uint32_t *__restrict__ src,
                                                              uint32_t *__restrict__ flags)
{
    __shared__ Tables T;
    __shared__ unsigned long long s_p;
    __shared__ uint32_t s_err;
    const uint32_t tid = threadIdx.x;
    const unsigned long long *my = win + WIN_SLOTS * (unsigned long long)blockIdx.x;
    const unsigned long long w0 = my[0], base = my[1], first = my[2];
    const uint32_t stream = (uint32_t)my[3];
    const unsigned long long header = w0 & ((1ull << 40) - 1ull), emit = w0 >> 44;
    const uint32_t btype = (uint32_t)(w0 >> 40) & 3u;
    const uint32_t *words = reinterpret_cast<const uint32_t *>(file + offsets[stream]);
    const unsigned long long total_bits = 8ull * counts[stream], need = stream_need(L, stream), at = (unsigned long long)stream * L.stream_bytes;
    raw += at, src += at;
    if (btype == 0) {
        if (tid >= emit) return;
        const uint8_t *from = reinterpret_cast<const uint8_t *>(words) + rec_entry[first + tid];
        const unsigned long long o = rec_out[first + tid], n = rec_count[first + tid];
        for (unsigned long long k = 0; k < n && k < PIECE && o + k < need; k++) raw[o + k] = from[k], src[o + k] = (uint32_t)(o + k);
        return;
    }
    if (load_tables(words, 0, header + 3, total_bits, btype, T, &s_err, &s_p)) return; // (the chain kernel has accepted the header)
    if (tid >= emit) return;
    const unsigned long long entry = rec_entry[first + tid];
    const unsigned long long end_bit_here = min(base + (unsigned long long)(tid + 1) * pd::SUBSEQ_BITS, total_bits);
    if (entry == ENDED || entry >= end_bit_here) return;
    unsigned long long count = 0, eob_after = 0;
    decode_subsequence<true>(words, 0, T, entry, end_bit_here, count, eob_after, raw, src, rec_out[first + tid], need, flags);
}

// Byte g of all streams is byte o = g - base of its own: out[o] = in[in[o]] where that is another step back (in[o] < o for a
// copy, = o for a literal; anything else is left alone)
__global__ __launch_bounds__(BLOCK) void inflate_resolve_kernel(const uint32_t *__restrict__ in, uint32_t *__restrict__ out, InflateLayout L,
                                                                uint32_t *__restrict__ flags)
{
    const unsigned long long g = (unsigned long long)blockIdx.x * BLOCK + threadIdx.x;
    if (g >= L.total) return;
    const unsigned long long base = g / L.stream_bytes * L.stream_bytes;
    const uint32_t o = (uint32_t)(g - base);
    uint32_t s = in[g];
    if (s < o) {
        const uint32_t t = in[base + s];
        if (t < s) s = t, flags[F_CHANGED] = 1u;
    }
    out[g] = s;
}

// raw[g] = its literal; sums[2 s] += sum d[o], sums[2 s + 1] += sum ((n - o) mod 65521) d[o] over stream s's n bytes
// (png_common.hpp: AdlerSums)
__global__ __launch_bounds__(BLOCK) void inflate_gather_kernel(uint8_t *__restrict__ raw, const uint32_t *__restrict__ src, InflateLayout L,
                                                               unsigned long long *__restrict__ sums)
{
    const unsigned long long g = (unsigned long long)blockIdx.x * BLOCK + threadIdx.x;
    const bool inside = g < L.total;
    const uint32_t stream = (uint32_t)((inside ? g : L.total - 1) / L.stream_bytes);
    unsigned long long a = 0, b = 0;
    if (inside) {
        const unsigned long long base = (unsigned long long)stream * L.stream_bytes;
        const uint32_t o = (uint32_t)(g - base), s = src[g];
        const uint8_t d = raw[base + (s < o ? s : o)]; // (a literal's position holds its own byte: reading it while its lane rewrites it is harmless)
        if (s < o) raw[g] = d;
        a = d, b = (unsigned long long)((stream_need(L, stream) - o) % pc::ADLER_MOD) * d;
    }
    // a wave inside one stream adds its sums up first; one that spans a stream's end adds lane by lane
    const uint32_t first = __shfl(stream, 0);
    if (__all(stream == first)) {
        for (int step = WAVE / 2; step; step >>= 1) a += __shfl_down(a, step), b += __shfl_down(b, step);
        if ((threadIdx.x & (WAVE - 1u)) != 0) return;
    }
    if (a | b) atomicAdd(&sums[2ull * stream], a), atomicAdd(&sums[2ull * stream + 1], b);
}

__global__ __launch_bounds__(BLOCK) void inflate_finish_kernel(const uint8_t *__restrict__ file, const uint32_t *__restrict__ offsets, uint32_t streams,
                                                               InflateLayout L, const unsigned long long *__restrict__ end_bit,
                                                               const unsigned long long *__restrict__ sums, uint32_t *__restrict__ flags)
{
    const uint32_t s = blockIdx.x * BLOCK + threadIdx.x;
    if (s >= streams) return;
    const uint8_t *stream = file + offsets[s];
    const unsigned long long at = (end_bit[s] + 7) / 8; // (the chain kernel has checked that four bytes follow)
    const uint32_t want = (uint32_t)stream[at] << 24 | (uint32_t)stream[at + 1] << 16 | (uint32_t)stream[at + 2] << 8 | stream[at + 3];
    const pc::AdlerSums whole = {(uint32_t)(sums[2ull * s] % pc::ADLER_MOD), (uint32_t)(sums[2ull * s + 1] % pc::ADLER_MOD)};
    if (pc::adler_value(whole, stream_need(L, s)) != want) atomicOr(&flags[F_ERR], ERR_ADLER);
}

// ---- the host sequence ---------------------------------------------------------------------------------------------------------------
// What the stage works on, all in device memory and all the caller's: it sizes and zeroes them (flags, end_bit and sums start
// at zero) and knows the bounds max_windows and max_records, which the chain kernel checks all the same.
struct InflateArgs {
    const uint8_t *file;
    const uint32_t *offsets, *counts; // of the `streams` streams
    uint32_t streams;
    InflateLayout layout;
    unsigned long long *win, max_windows;                     // WIN_SLOTS words a window
    unsigned long long *rec_entry, *rec_out, max_records;     // a record: its entry state (a stored one: its first byte), its output position
    uint32_t *rec_count;                                      // and, of a stored one, its bytes
    uint8_t *raw;                                             // the streams' bytes
    uint32_t *srcs[2];                                        // the source indices, layout.total each
    unsigned long long *end_bit, *sums;                       // per stream: the bit behind its final block; the two Adler-32 sums
    uint32_t *flags;                                          // FLAGS words
};

// Chain, write, the copies, gather and finish on stream s -> CVHIP_OK, or the device's failure as `name`'s.  err: the error bits
// of the file, for the caller's words (0: the finish kernel's verdict comes with the caller's next read of the flags);
// h_flags: the FLAGS words as last read back; copy_rounds: the launches of the resolve kernel.
// size_after_write: a size error alone does not stop before the write pass, whose token errors the caller ranks first (PNG).
int inflate_streams(const char *name, hipStream_t s, const InflateArgs &a, bool size_after_write, uint32_t *h_flags, uint32_t &err, uint32_t &copy_rounds)
{
    auto read_flags = [&]() {
        hipError_t r = hipGetLastError();
        if (r == hipSuccess) r = hipMemcpyAsync(h_flags, a.flags, FLAGS * sizeof(uint32_t), hipMemcpyDeviceToHost, s);
        if (r == hipSuccess) r = hipStreamSynchronize(s);
        return r;
    };
    const dim3 block(BLOCK);
    hipError_t e;
    err = 0, copy_rounds = 0;
    hipLaunchKernelGGL(inflate_chain_kernel, dim3(a.streams), block, 0, s, a.file, a.offsets, a.counts, a.layout, a.win, a.max_windows, a.rec_entry, a.rec_out,
                       a.rec_count, a.max_records, a.flags, a.end_bit);
    if ((e = read_flags()) != hipSuccess) return device_error(name, e);
    if ((err = h_flags[F_ERR]) != 0 && !(size_after_write && err == ERR_SIZE)) return CVHIP_OK;
    const uint32_t n_win = h_flags[F_EMITTED];
    if (n_win == 0) { // no output at all
        err = ERR_SIZE;
        return CVHIP_OK;
    }
    hipLaunchKernelGGL(inflate_write_kernel, dim3(n_win), block, 0, s, a.file, a.offsets, a.counts, a.layout, a.win, a.rec_entry, a.rec_out, a.rec_count, a.raw,
                       a.srcs[0], a.flags);
    // ---- the copies: pointer doubling, a launch and one flag back per round (a chain of 2^31 copies takes 31 rounds and the one that changes nothing)
    const dim3 byte_grid((uint32_t)((a.layout.total + BLOCK - 1) / BLOCK));
    uint32_t from = 0;
    for (;; from ^= 1u) {
        if (copy_rounds > 33) return fail(CVHIP_ERR_DEVICE, std::string(name) + ": the copies did not resolve");
        e = hipMemsetAsync(a.flags + F_CHANGED, 0, sizeof(uint32_t), s);
        if (e != hipSuccess) return device_error(name, e);
        hipLaunchKernelGGL(inflate_resolve_kernel, byte_grid, block, 0, s, a.srcs[from], a.srcs[from ^ 1u], a.layout, a.flags);
        copy_rounds++;
        if ((e = read_flags()) != hipSuccess) return device_error(name, e);
        if (h_flags[F_ERR] || !h_flags[F_CHANGED]) break;
    }
    if ((err = h_flags[F_ERR]) != 0) return CVHIP_OK;
    hipLaunchKernelGGL(inflate_gather_kernel, byte_grid, block, 0, s, a.raw, a.srcs[from ^ 1u], a.layout, a.sums);
    hipLaunchKernelGGL(inflate_finish_kernel, dim3((a.streams + BLOCK - 1) / BLOCK), block, 0, s, a.file, a.offsets, a.streams, a.layout, a.end_bit, a.sums, a.flags);
    return CVHIP_OK;
}
