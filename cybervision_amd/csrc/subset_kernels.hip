// subset_kernels.hip — max_points on the device: a seeded random subset of a surface's rows.
//
// Replaces the tail of PerspectiveTriangulation::triangulate_all (zlogic/cybervision src/triangulation.rs:837-843):
// `tracks.shuffle(rng); tracks.truncate(max_points)` with an OS-seeded generator.  Here row i of n gets the key
// mix64(mix64(seed) + (i + 1) * 0x9E3779B97F4A7C15) (subset_common.hpp) and the max_points rows with the smallest keys are
// kept, in ascending row order - the same distribution of the kept SET, a defined order instead of a random one.
//
//   subset_histogram_kernel  x 8   radix select of the max_points-th smallest key, 8 bits per pass from the top: an LDS histogram
//                                  per workgroup of the digit of the rows under the prefix found so far, merged into the pass's
//                                  256 global counters; every workgroup derives the prefix and the remaining rank from the pass
//                                  before (descend) - no host round trip, and hashed keys are recomputed, never stored
//   subset_count_kernel            per chunk of CVHIP_SUBSET_WG_ROWS rows: the rows below the threshold T and the rows equal to it
//   launch_scan_u64                their exclusive scan over the chunks (both counts in one 64-bit word)
//   subset_write_kernel            the kept rows - key < T, and the first (max_points - rows below T) rows with key == T - to
//                                  their places, by wave ballots inside the chunk
//   subset_gather_*_kernel         points and track rows of the kept rows, one lane per output element
// Integer only: exact.  The same kernels select on keys given by the caller (cvhip_select_smallest_u64; ties: the lower row).
#include "cvhip_internal.hpp"
#include "subset_common.hpp"

#include <cstring>

namespace cvhip {
namespace {

using namespace subset;
constexpr uint32_t WG_ROWS = CVHIP_SUBSET_WG_ROWS;

struct HashedKeys {
    unsigned long long start; // mix64(seed)
    __device__ __forceinline__ unsigned long long operator()(unsigned long long row) const { return hashed_key(start, row); }
};
struct LoadedKeys {
    const unsigned long long *keys;
    __device__ __forceinline__ unsigned long long operator()(unsigned long long row) const { return keys[row]; }
};

// The descent going INTO a pass: the digits of the threshold found so far and the rank of the threshold among the rows whose
// key begins with them.  state[p] is written by workgroup 0 of pass p's kernel (p = 1 .. PASSES) and read by the next launch.
struct Descent {
    unsigned long long prefix, rank;
};

// Every lane of the workgroup calls it: the descent going into `pass`, from the one going into pass - 1 and that pass's
// histogram - the digit whose range of ranks holds the rank is appended.  (0, m - 1) goes into pass 0: the threshold is the
// key of 0-based rank m - 1, and there are always more rows under the prefix than the rank.
__device__ __forceinline__ Descent descend(uint32_t pass, unsigned long long m, const Descent *state, const uint32_t *hist,
                                           uint32_t *s_wave, Descent *s_out)
{
    Descent d{0, m - 1};
    if (pass == 0) return d;
    if (pass > 1) d = state[pass - 1];
    const uint32_t lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const uint32_t c = hist[(pass - 1) * DIGITS + threadIdx.x];
    uint32_t incl = c;
#pragma unroll
    for (int s = 1; s < 64; s <<= 1) {
        const uint32_t t = __shfl_up(incl, s, 64);
        if ((int)lane >= s) incl += t;
    }
    if (lane == 63) s_wave[wv] = incl;
    __syncthreads();
    for (uint32_t w = 0; w < wv; w++) incl += s_wave[w];
    const unsigned long long excl = incl - c;
    if (excl <= d.rank && d.rank < incl) *s_out = Descent{d.prefix << DIGIT_BITS | threadIdx.x, d.rank - excl};
    __syncthreads();
    return *s_out;
}

template <typename Keys>
__global__ __launch_bounds__(BLOCK) void subset_histogram_kernel(Keys keys, unsigned long long n, unsigned long long m, uint32_t pass,
                                                                 Descent *state, uint32_t *hist)
{
    __shared__ uint32_t s_hist[DIGITS];
    __shared__ uint32_t s_wave[BLOCK / 64];
    __shared__ Descent s_d;
    s_hist[threadIdx.x] = 0;
    const Descent d = descend(pass, m, state, hist, s_wave, &s_d);
    if (pass > 0 && blockIdx.x == 0 && threadIdx.x == 0) state[pass] = d;
    __syncthreads();
    const uint32_t shift = 64 - DIGIT_BITS * (pass + 1);
    const unsigned long long chunks = (n + WG_ROWS - 1) / WG_ROWS;
    for (unsigned long long chunk = blockIdx.x; chunk < chunks; chunk += gridDim.x) {
#pragma unroll
        for (uint32_t j = 0; j < LANE_ROWS; j++) {
            const unsigned long long row = chunk * WG_ROWS + j * BLOCK + threadIdx.x;
            if (row >= n) continue;
            const unsigned long long key = keys(row);
            if (pass == 0 || (key >> (shift + DIGIT_BITS)) == d.prefix) atomicAdd(&s_hist[(key >> shift) & (DIGITS - 1)], 1u);
        }
    }
    __syncthreads();
    const uint32_t c = s_hist[threadIdx.x];
    if (c) atomicAdd(&hist[pass * DIGITS + threadIdx.x], c);
}

// counts[chunk] = rows of the chunk below T | rows equal to T << 32; workgroup 0 leaves the final descent in state[PASSES]:
// prefix = T, rank = its rank among the rows equal to T (rank + 1 of them are kept)
template <typename Keys>
__global__ __launch_bounds__(BLOCK) void subset_count_kernel(Keys keys, unsigned long long n, unsigned long long m, Descent *state,
                                                             const uint32_t *hist, unsigned long long *__restrict__ counts)
{
    __shared__ uint32_t s_wave[BLOCK / 64];
    __shared__ unsigned long long s_cnt[BLOCK / 64];
    __shared__ Descent s_d;
    const Descent d = descend(PASSES, m, state, hist, s_wave, &s_d);
    if (blockIdx.x == 0 && threadIdx.x == 0) state[PASSES] = d;
    const unsigned long long T = d.prefix;
    const unsigned long long chunks = (n + WG_ROWS - 1) / WG_ROWS;
    for (unsigned long long chunk = blockIdx.x; chunk < chunks; chunk += gridDim.x) {
        unsigned long long cnt = 0;
#pragma unroll
        for (uint32_t j = 0; j < LANE_ROWS; j++) {
            const unsigned long long row = chunk * WG_ROWS + j * BLOCK + threadIdx.x;
            const unsigned long long key = row < n ? keys(row) : 0;
            cnt += (unsigned long long)__popcll(__ballot(row < n && key < T));
            cnt += (unsigned long long)__popcll(__ballot(row < n && key == T)) << 32;
        }
        if ((threadIdx.x & 63) == 0) s_cnt[threadIdx.x >> 6] = cnt;
        __syncthreads();
        if (threadIdx.x == 0) counts[chunk] = s_cnt[0] + s_cnt[1] + s_cnt[2] + s_cnt[3];
        __syncthreads();
    }
}

// offsets = the exclusive scan of counts.  A row is kept iff key < T, or key == T and fewer than need_eq equal rows come before
// it; its place is the number of kept rows before it.  sel (u32, for the gathers) and out_rows (u64) may each be null.
template <typename Keys>
__global__ __launch_bounds__(BLOCK) void subset_write_kernel(Keys keys, unsigned long long n, const Descent *__restrict__ state,
                                                             const unsigned long long *__restrict__ offsets, unsigned long long out_n,
                                                             uint32_t *__restrict__ sel, unsigned long long *__restrict__ out_rows)
{
    __shared__ uint32_t s_less[LANE_ROWS][BLOCK / 64], s_eq[LANE_ROWS][BLOCK / 64];
    const unsigned long long T = state[PASSES].prefix, need_eq = state[PASSES].rank + 1;
    const uint32_t lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const unsigned long long below = (1ull << lane) - 1ull;
    const unsigned long long chunks = (n + WG_ROWS - 1) / WG_ROWS;
    for (unsigned long long chunk = blockIdx.x; chunk < chunks; chunk += gridDim.x) {
        bool less[LANE_ROWS], eq[LANE_ROWS];
        uint32_t less_before[LANE_ROWS], eq_before[LANE_ROWS]; // among the wave's own 64 rows of step j
#pragma unroll
        for (uint32_t j = 0; j < LANE_ROWS; j++) {
            const unsigned long long row = chunk * WG_ROWS + j * BLOCK + threadIdx.x;
            const unsigned long long key = row < n ? keys(row) : 0;
            less[j] = row < n && key < T;
            eq[j] = row < n && key == T;
            const unsigned long long bl = __ballot(less[j]), be = __ballot(eq[j]);
            less_before[j] = (uint32_t)__popcll(bl & below);
            eq_before[j] = (uint32_t)__popcll(be & below);
            if (lane == 0) {
                s_less[j][wv] = (uint32_t)__popcll(bl);
                s_eq[j][wv] = (uint32_t)__popcll(be);
            }
        }
        __syncthreads();
        const unsigned long long off = offsets[chunk];
        unsigned long long nl = off & 0xFFFFFFFFull, ne = off >> 32; // rows below / equal before wave (j, w), in row order
#pragma unroll
        for (uint32_t j = 0; j < LANE_ROWS; j++)
            for (uint32_t w = 0; w < BLOCK / 64; w++) {
                if (w == wv && (less[j] || eq[j])) {
                    const unsigned long long e = ne + eq_before[j];
                    const unsigned long long pos = nl + less_before[j] + (e < need_eq ? e : need_eq);
                    if ((less[j] || e < need_eq) && pos < out_n) {
                        const unsigned long long row = chunk * WG_ROWS + j * BLOCK + threadIdx.x;
                        if (sel) sel[pos] = (uint32_t)row;
                        if (out_rows) out_rows[pos] = row;
                    }
                }
                nl += s_less[j][w];
                ne += s_eq[j][w];
            }
        __syncthreads();
    }
}

// out_points[k] = points[sel[k]]: one lane per output f64
__global__ __launch_bounds__(256) void subset_gather_points_kernel(const uint32_t *__restrict__ sel, const double *__restrict__ points,
                                                                   unsigned long long out_n, double *__restrict__ out)
{
    const unsigned long long total = out_n * 3, step = (unsigned long long)gridDim.x * 256;
    for (unsigned long long g = (unsigned long long)blockIdx.x * 256 + threadIdx.x; g < total; g += step) {
        const unsigned long long k = g / 3;
        out[g] = points[(unsigned long long)sel[k] * 3 + (g - k * 3)];
    }
}

// out_tracks[k] = tracks[sel[k]], rows of `width` = 2 * m_cams int32: one lane per output dword
__global__ __launch_bounds__(256) void subset_gather_tracks_kernel(const uint32_t *__restrict__ sel, const int32_t *__restrict__ tracks,
                                                                   uint32_t width, unsigned long long out_n, int32_t *__restrict__ out)
{
    const unsigned long long total = out_n * width, step = (unsigned long long)gridDim.x * 256;
    for (unsigned long long g = (unsigned long long)blockIdx.x * 256 + threadIdx.x; g < total; g += step) {
        const unsigned long long k = g / width;
        out[g] = tracks[(unsigned long long)sel[k] * width + (g - k * width)];
    }
}

// max_points >= n: every row, in order
__global__ __launch_bounds__(256) void subset_iota_kernel(unsigned long long n, unsigned long long *__restrict__ out_rows)
{
    const unsigned long long step = (unsigned long long)gridDim.x * 256;
    for (unsigned long long i = (unsigned long long)blockIdx.x * 256 + threadIdx.x; i < n; i += step) out_rows[i] = i;
}

// the m (1 <= m < n) rows with the smallest (key, row), ascending, into d_sel and d_rows (device, each may be null)
template <typename Keys>
hipError_t select_rows(CallScratch &sc, Keys keys, unsigned long long n, unsigned long long m, uint32_t *d_sel,
                       unsigned long long *d_rows, hipStream_t s)
{
    const unsigned long long chunks = (n + WG_ROWS - 1) / WG_ROWS;
    const uint32_t grid = (uint32_t)std::min<unsigned long long>(chunks, GRID_BLOCKS);
    // one allocation: the descents, then the histograms
    constexpr size_t STATE_WORDS = 2 * (PASSES + 1), HIST_WORDS = PASSES * DIGITS / 2;
    unsigned long long *d_work = nullptr, *d_counts = nullptr;
    hipError_t e = sc.alloc(&d_work, STATE_WORDS + HIST_WORDS);
    if (e == hipSuccess) e = sc.alloc(&d_counts, (size_t)chunks + 1);
    if (e == hipSuccess) e = hipMemsetAsync(d_work, 0, (STATE_WORDS + HIST_WORDS) * sizeof(unsigned long long), s);
    if (e != hipSuccess) return e;
    Descent *state = reinterpret_cast<Descent *>(d_work);
    uint32_t *hist = reinterpret_cast<uint32_t *>(d_work + STATE_WORDS);
    for (uint32_t pass = 0; pass < PASSES; pass++)
        hipLaunchKernelGGL(subset_histogram_kernel<Keys>, dim3(grid), dim3(BLOCK), 0, s, keys, n, m, pass, state, hist);
    hipLaunchKernelGGL(subset_count_kernel<Keys>, dim3(grid), dim3(BLOCK), 0, s, keys, n, m, state, hist, d_counts);
    launch_scan_u64(d_counts, chunks, d_counts + chunks, s);
    hipLaunchKernelGGL(subset_write_kernel<Keys>, dim3(grid), dim3(BLOCK), 0, s, keys, n, state, d_counts, m, d_sel, d_rows);
    return hipGetLastError();
}

// host or device array to host or device array, enqueued
hipError_t copy_any(void *dst, const void *src, size_t bytes, hipStream_t s)
{
    if (!bytes) return hipSuccess;
    const bool dd = on_device(dst), sd = on_device(src);
    if (!dd && !sd) {
        std::memcpy(dst, src, bytes);
        return hipSuccess;
    }
    return hipMemcpyAsync(dst, src, bytes, dd ? (sd ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice) : hipMemcpyDeviceToHost, s);
}

// both entry points behind their argument checks: keys == nullptr takes the hashed keys of `seed`
int subset_run(const char *what, Device &d, const unsigned long long *keys, uint64_t seed, uint64_t n, uint64_t max_points, const double *points,
               const int32_t *tracks, uint32_t m_cams, uint64_t *out_rows, double *out_points, int32_t *out_tracks, uint64_t *out_n)
{
    const uint64_t out = std::min(n, max_points);
    if (!out) {
        *out_n = 0;
        return CVHIP_OK;
    }
    CVHIP_TRY_HIP(hipSetDevice(d.ordinal));
    hipStream_t s = d.stream;
    const size_t width = 2 * (size_t)m_cams;
    unsigned long long *const rows = reinterpret_cast<unsigned long long *>(out_rows), *d_rows = nullptr;
    CallScratch sc;
    hipError_t e = sc.output(rows, (size_t)out, &d_rows);
    if (out == n) { // the reference only acts when len > max_points: copies, no selection
        if (e == hipSuccess && d_rows) {
            hipLaunchKernelGGL(subset_iota_kernel, dim3(grid_for(n)), dim3(256), 0, s, n, d_rows);
            e = hipGetLastError();
        }
        if (e == hipSuccess) e = sc.copy_out(rows, d_rows, (size_t)out, s);
        if (e == hipSuccess && out_points) e = copy_any(out_points, points, (size_t)n * 3 * sizeof(double), s);
        if (e == hipSuccess && out_tracks) e = copy_any(out_tracks, tracks, (size_t)n * width * sizeof(int32_t), s);
        if (e == hipSuccess) e = hipStreamSynchronize(s);
        if (e != hipSuccess) return device_error(what, e);
        *out_n = out;
        return CVHIP_OK;
    }
    const unsigned long long *d_keys = nullptr;
    const double *d_points = nullptr;
    const int32_t *d_tracks = nullptr;
    double *d_opoints = nullptr;
    int32_t *d_otracks = nullptr;
    uint32_t *d_sel = nullptr;
    if (e == hipSuccess && keys) e = sc.input(keys, (size_t)n, &d_keys, s);
    if (e == hipSuccess && out_points) e = sc.input(points, (size_t)n * 3, &d_points, s);
    if (e == hipSuccess && out_tracks) e = sc.input(tracks, (size_t)n * width, &d_tracks, s);
    if (e == hipSuccess) e = sc.output(out_points, (size_t)out * 3, &d_opoints);
    if (e == hipSuccess) e = sc.output(out_tracks, (size_t)out * width, &d_otracks);
    if (e == hipSuccess && (out_points || out_tracks)) e = sc.alloc(&d_sel, (size_t)out);
    if (e == hipSuccess && (d_sel || d_rows))
        e = keys ? select_rows(sc, LoadedKeys{d_keys}, n, out, d_sel, d_rows, s)
                 : select_rows(sc, HashedKeys{mix64(seed)}, n, out, d_sel, d_rows, s);
    if (e == hipSuccess && out_points)
        hipLaunchKernelGGL(subset_gather_points_kernel, dim3(grid_for(out * 3)), dim3(256), 0, s, d_sel, d_points, out, d_opoints);
    if (e == hipSuccess && out_tracks)
        hipLaunchKernelGGL(subset_gather_tracks_kernel, dim3(grid_for(out * width)), dim3(256), 0, s, d_sel, d_tracks, (uint32_t)width, out,
                           d_otracks);
    if (e == hipSuccess) e = hipGetLastError();
    if (e == hipSuccess) e = sc.copy_out(rows, d_rows, (size_t)out, s);
    if (e == hipSuccess) e = sc.copy_out(out_points, d_opoints, (size_t)out * 3, s);
    if (e == hipSuccess) e = sc.copy_out(out_tracks, d_otracks, (size_t)out * width, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) return device_error(what, e);
    *out_n = out;
    return CVHIP_OK;
}

} // namespace
} // namespace cvhip

using namespace cvhip;

extern "C" int cvhip_surface_subset(cvhip_device *dev, uint64_t n, uint64_t max_points, uint64_t seed, const double *points,
                                    const int32_t *tracks, uint32_t m_cams, uint64_t *out_rows, double *out_points, int32_t *out_tracks,
                                    uint64_t *out_n)
{
    if (!dev || !out_n) return fail(CVHIP_ERR_INVALID, "null argument");
    if ((out_points && !points) || (out_tracks && !tracks)) return fail(CVHIP_ERR_INVALID, "surface_subset: an output without its input");
    if (tracks && m_cams == 0) return fail(CVHIP_ERR_INVALID, "surface_subset: tracks of no camera");
    if (m_cams > CVHIP_TRIANGULATE_MAX_CAMERAS) return fail(CVHIP_ERR_UNSUPPORTED, "surface_subset: more than CVHIP_TRIANGULATE_MAX_CAMERAS cameras");
    if (n >= 0xFFFFFFFFull) return fail(CVHIP_ERR_UNSUPPORTED, "surface_subset: more than 2^32 - 2 rows"); // the kept rows are 32-bit
    return subset_run("surface_subset", dev->d, nullptr, seed, n, max_points, points, tracks, m_cams, out_rows, out_points, out_tracks, out_n);
}

extern "C" int cvhip_select_smallest_u64(cvhip_device *dev, const uint64_t *keys, uint64_t n, uint64_t m, uint64_t *out_rows,
                                         uint64_t *out_n)
{
    if (!dev || !out_n || (n && !keys)) return fail(CVHIP_ERR_INVALID, "null argument");
    if (n >= 0xFFFFFFFFull) return fail(CVHIP_ERR_UNSUPPORTED, "select_smallest_u64: more than 2^32 - 2 rows");
    return subset_run("select_smallest_u64", dev->d, reinterpret_cast<const unsigned long long *>(keys), 0, n, m, nullptr, nullptr, 0, out_rows,
                      nullptr, nullptr, out_n);
}
