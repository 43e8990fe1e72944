// jpeg_tail.inc — what cvhip_jpeg_decode (jpeg_kernels.hip, DESIGN.md 4.16) and cvhip_jpeg_progressive_decode (jpeg_prog_kernels.hip,
// DESIGN.md 4.22) share behind their entropy decodes: the frame as the kernels take it, and the tail from the block store to the
// pixels - jpeg_idct_kernel and jpeg_pixels_kernel - with its host side: the planes' layout, the two launches with the flags' way
// back, the copy into the caller's array.  Included inside namespace cvhip { namespace { of each of the two sources, in front of
// jpeg_entropy.inc (what they share in front of the block store): every kernel here is compiled into both, none is called across them.

constexpr int WAVE = 64;
constexpr uint32_t BLOCK = 256;      // lanes of a workgroup; of jpeg_sync_kernel: the subsequences that settle within one launch
constexpr uint32_t FLAG_ERR = 0, FLAG_CHANGED = 1, FLAG_ROUNDS = 2, FLAG_SUBSEQUENCES = 3, FLAGS = 4;

struct JpegParams {
    uint32_t width, height, ncomp, hmax, vmax, mcus_x, mcus_y, bpm;
    uint32_t interval; // MCUs of a restart interval (all of them without DRI)
    uint32_t nseg, mcus;
    uint32_t luma_blocks;          // the first component's blocks in an MCU; the others have one each
    uint32_t dc_lut[3], ac_lut[3]; // the component's tables among the uploaded ones
    uint32_t n_luts;
};

// (selects, not indexed loads: a lane-dependent index into the kernel's arguments would put them into scratch memory)
__device__ __forceinline__ uint32_t slot_component(const JpegParams &P, uint32_t slot) { return slot < P.luma_blocks ? 0u : slot - P.luma_blocks + 1u; }
__device__ __forceinline__ uint32_t pick(const uint32_t (&v)[3], uint32_t c) { return c == 0 ? v[0] : c == 1 ? v[1] : v[2]; }

// jidctint's one-dimensional pass (CONST_BITS 13) over v[0 .. 8), descaled by SHIFT
template <int SHIFT> __device__ __forceinline__ void idct_pass(long long (&v)[8])
{
    long long z2 = v[2], z3 = v[6];
    long long z1 = (z2 + z3) * 4433;
    long long tmp2 = z1 - z3 * 15137, tmp3 = z1 + z2 * 6270;
    long long tmp0 = (v[0] + v[4]) * 8192, tmp1 = (v[0] - v[4]) * 8192;
    const long long tmp10 = tmp0 + tmp3, tmp13 = tmp0 - tmp3, tmp11 = tmp1 + tmp2, tmp12 = tmp1 - tmp2;
    tmp0 = v[7], tmp1 = v[5], tmp2 = v[3], tmp3 = v[1];
    z1 = tmp0 + tmp3, z2 = tmp1 + tmp2, z3 = tmp0 + tmp2;
    long long z4 = tmp1 + tmp3;
    const long long z5 = (z3 + z4) * 9633;
    tmp0 *= 2446, tmp1 *= 16819, tmp2 *= 25172, tmp3 *= 12299;
    z1 *= -7373, z2 *= -20995, z3 = z3 * -16069 + z5, z4 = z4 * -3196 + z5;
    tmp0 += z1 + z3, tmp1 += z2 + z4, tmp2 += z2 + z3, tmp3 += z1 + z4;
    const long long half = 1ll << (SHIFT - 1);
    v[0] = (tmp10 + tmp3 + half) >> SHIFT, v[7] = (tmp10 - tmp3 + half) >> SHIFT;
    v[1] = (tmp11 + tmp2 + half) >> SHIFT, v[6] = (tmp11 - tmp2 + half) >> SHIFT;
    v[2] = (tmp12 + tmp1 + half) >> SHIFT, v[5] = (tmp12 - tmp1 + half) >> SHIFT;
    v[3] = (tmp13 + tmp0 + half) >> SHIFT, v[4] = (tmp13 - tmp0 + half) >> SHIFT;
}

struct Planes {
    uint8_t *base[3];
    uint32_t stride[3]; // bytes of a row: the component's blocks across, times 8
};

// sums: scanned.  quant: [component][64], natural order.  64-bit integers throughout: |coefficient| <= 2^15 times a table entry
// < 2^16 is < 2^31, a pass multiplies by < 2^15 and adds 8 terms, so the columns stay below 2^50 (2^39 descaled) and the rows
// below 2^58 - what an encoder emits would fit 32 bits, what a file may hold does not, and the definition clamps.
__global__ __launch_bounds__(WAVE) void jpeg_idct_kernel(const short *__restrict__ coef, JpegParams P, const unsigned long long *__restrict__ sums,
                                                         const uint16_t *__restrict__ quant, Planes planes, unsigned long long n_blocks,
                                                         const uint32_t *__restrict__ flags)
{
    __shared__ uint32_t s_quant[3 * 64];
    if (flags[FLAG_ERR]) return;
    for (uint32_t k = threadIdx.x; k < P.ncomp * 64; k += WAVE) s_quant[k] = quant[k];
    __syncthreads();
    const unsigned long long b = (unsigned long long)blockIdx.x * WAVE + threadIdx.x;
    if (b >= n_blocks) return;
    const uint32_t m = (uint32_t)(b / P.bpm), slot = (uint32_t)(b % P.bpm), c = slot_component(P, slot);
    const short *in = coef + b * 64;
    // the DC value: the differences of the component from the interval's first MCU on, in 16 bits
    const unsigned long long *comp_sums = sums + (unsigned long long)c * P.mcus;
    long long dc = (long long)(comp_sums[m] - comp_sums[m / P.interval * P.interval]);
    const uint32_t first_slot = c == 0 ? 0u : slot; // the component's first slot in the MCU
    for (uint32_t q = first_slot; q <= slot; q++) dc += coef[((unsigned long long)m * P.bpm + q) * 64];
    long long ws[64];
#pragma unroll
    for (int col = 0; col < 8; col++) {
        long long v[8];
#pragma unroll
        for (int r = 0; r < 8; r++) v[r] = (long long)in[r * 8 + col] * (long long)s_quant[c * 64 + r * 8 + col];
        if (col == 0) v[0] = (long long)(short)dc * (long long)s_quant[c * 64];
        idct_pass<11>(v);
#pragma unroll
        for (int r = 0; r < 8; r++) ws[r * 8 + col] = v[r];
    }
    const uint32_t q = slot - first_slot, across = c == 0 ? P.hmax : 1u, down = c == 0 ? P.vmax : 1u;
    const uint32_t bx = (m % P.mcus_x) * across + q % across, by = (m / P.mcus_x) * down + q / across;
    uint8_t *dst = planes.base[c] + ((unsigned long long)by * 8) * planes.stride[c] + (unsigned long long)bx * 8;
#pragma unroll
    for (int r = 0; r < 8; r++) {
        long long v[8];
#pragma unroll
        for (int col = 0; col < 8; col++) v[col] = ws[r * 8 + col];
        idct_pass<18>(v);
        uint32_t lo = 0, hi = 0;
#pragma unroll
        for (int col = 0; col < 8; col++) {
            const long long x = v[col] + 128;
            const uint32_t px = x < 0 ? 0u : x > 255 ? 255u : (uint32_t)x;
            if (col < 4) lo |= px << (8 * col);
            else hi |= px << (8 * (col - 4));
        }
        *reinterpret_cast<uint2 *>(dst + (unsigned long long)r * planes.stride[c]) = make_uint2(lo, hi); // (8-byte aligned: strides and bx * 8 are)
    }
}

// libjpeg's fancy upsampling of a chroma plane of dw x dh samples that count, at pixel (x, y) (tests/ref_jpeg.py: upsample)
__device__ __forceinline__ int chroma_at(const uint8_t *__restrict__ plane, uint32_t stride, uint32_t dw, uint32_t dh, uint32_t hs, uint32_t vs,
                                         uint32_t x, uint32_t y)
{
    if (hs == 1) return plane[(unsigned long long)y * stride + x];
    const uint32_t i = x >> 1;
    if (vs == 1) {
        const uint8_t *row = plane + (unsigned long long)y * stride;
        if (dw <= 2 || x == 0 || x == 2 * dw - 1) return row[i];
        return (x & 1u) ? (3 * row[i] + row[i + 1] + 2) >> 2 : (3 * row[i] + row[i - 1] + 1) >> 2;
    }
    const uint32_t r = y >> 1;
    if (dw <= 2) return plane[(unsigned long long)r * stride + i];
    const uint32_t other = (y & 1u) ? (r + 1 < dh ? r + 1 : dh - 1) : (r ? r - 1 : 0u);
    const uint8_t *near = plane + (unsigned long long)r * stride, *far = plane + (unsigned long long)other * stride;
    const int t = 3 * near[i] + far[i];
    if (x == 0) return (4 * t + 8) >> 4;
    if (x == 2 * dw - 1) return (4 * t + 7) >> 4;
    return (x & 1u) ? (3 * t + 3 * near[i + 1] + far[i + 1] + 7) >> 4 : (3 * t + 3 * near[i - 1] + far[i - 1] + 8) >> 4;
}

__device__ __forceinline__ uint32_t clamp_byte(int v) { return v < 0 ? 0u : v > 255 ? 255u : (uint32_t)v; }

// pixel `pix` of the width x rows result: r | g << 8 | b << 16 (a grey file: its sample three times)
__device__ __forceinline__ uint32_t pixel_rgb(const JpegParams &P, const Planes &planes, uint32_t dw, uint32_t dh, uint32_t pix)
{
    const uint32_t x = pix % P.width, y = pix / P.width;
    const int luma = planes.base[0][(unsigned long long)y * planes.stride[0] + x];
    if (P.ncomp == 1) return (uint32_t)luma * 0x010101u;
    const int cb = chroma_at(planes.base[1], planes.stride[1], dw, dh, P.hmax, P.vmax, x, y) - 128;
    const int cr = chroma_at(planes.base[2], planes.stride[2], dw, dh, P.hmax, P.vmax, x, y) - 128;
    const uint32_t r = clamp_byte(luma + ((91881 * cr + 32768) >> 16)), b = clamp_byte(luma + ((116130 * cb + 32768) >> 16));
    const uint32_t g = clamp_byte(luma + ((-22554 * cb - 46802 * cr + 32768) >> 16));
    return r | g << 8 | b << 16;
}

// byte `at` of the result (channels: 1 = Luma8, 3 = RGB8)
__device__ __forceinline__ uint32_t result_byte(const JpegParams &P, const Planes &planes, uint32_t dw, uint32_t dh, uint32_t channels,
                                                unsigned long long at)
{
    if (channels == 3) return (pixel_rgb(P, planes, dw, dh, (uint32_t)(at / 3)) >> (8 * (uint32_t)(at % 3))) & 255u;
    if (P.ncomp == 1) return pixel_rgb(P, planes, dw, dh, (uint32_t)at) & 255u;
    const uint32_t rgb = pixel_rgb(P, planes, dw, dh, (uint32_t)at);
    return (2126u * (rgb & 255u) + 7152u * ((rgb >> 8) & 255u) + 722u * (rgb >> 16)) / 10000u; // into_luma8, as remembered (DESIGN.md 4.16)
}

// out[0 .. bytes): `lead` single bytes up to the first 4-byte aligned address, whole dwords, the rest single bytes - a lane
// per dword and a lane per single byte
__global__ __launch_bounds__(BLOCK) void jpeg_pixels_kernel(JpegParams P, Planes planes, uint32_t channels, uint8_t *__restrict__ out,
                                                            unsigned long long bytes, uint32_t lead, const uint32_t *__restrict__ flags)
{
    if (flags[FLAG_ERR]) return;
    const uint32_t dw = (P.width + P.hmax - 1) / P.hmax, dh = (P.height + P.vmax - 1) / P.vmax;
    const unsigned long long t = (unsigned long long)blockIdx.x * BLOCK + threadIdx.x, dwords = (bytes - lead) / 4;
    if (t < dwords) {
        const unsigned long long at = lead + 4 * t;
        uint32_t word = 0;
        if (channels == 3) {
            const uint32_t pix = (uint32_t)(at / 3), c = (uint32_t)(at % 3);
            const unsigned long long both = (unsigned long long)pixel_rgb(P, planes, dw, dh, pix) |
                                            (unsigned long long)(at + 3 - c < bytes ? pixel_rgb(P, planes, dw, dh, pix + 1) : 0u) << 24;
            word = (uint32_t)(both >> (8 * c));
        } else {
#pragma unroll
            for (uint32_t k = 0; k < 4; k++) word |= result_byte(P, planes, dw, dh, 1, at + k) << (8 * k);
        }
        *reinterpret_cast<uint32_t *>(out + at) = word;
        return;
    }
    const unsigned long long single = t - dwords, singles = bytes - 4 * dwords;
    if (single >= singles) return;
    const unsigned long long at = single < lead ? single : 4 * dwords + single;
    out[at] = (uint8_t)result_byte(P, planes, dw, dh, channels, at);
}

// ---- the host side of the tail ---------------------------------------------------------------------------------------------------
// the components' planes one behind the other: their strides, where each begins and the bytes of all
struct PlaneLayout {
    Planes planes{};
    size_t at[3] = {0, 0, 0}, total = 0;
    explicit PlaneLayout(const JpegParams &P)
    {
        for (uint32_t c = 0; c < P.ncomp; c++) {
            planes.stride[c] = P.mcus_x * (c == 0 ? P.hmax : 1u) * 8u;
            at[c] = total;
            total += (size_t)planes.stride[c] * P.mcus_y * (c == 0 ? P.vmax : 1u) * 8u; // (a multiple of 64 bytes)
        }
    }
    const Planes &placed(uint8_t *base, uint32_t ncomp)
    {
        for (uint32_t c = 0; c < ncomp; c++) planes.base[c] = base + at[c];
        return planes;
    }
};

// The block store to the pixels in d_out[0 .. bytes), and flags[0 .. n_flags) back into h_flags: waits for the stream.
inline int launch_tail(const char *what, const JpegParams &P, const Planes &planes, const short *coef, const unsigned long long *sums,
                       const uint16_t *d_quant, uint32_t channels, uint8_t *d_out, unsigned long long bytes, uint32_t *flags, uint32_t *h_flags,
                       size_t n_flags, hipStream_t s)
{
    const unsigned long long n_blocks = (unsigned long long)P.mcus * P.bpm;
    hipLaunchKernelGGL(jpeg_idct_kernel, dim3((uint32_t)((n_blocks + WAVE - 1) / WAVE)), dim3(WAVE), 0, s, coef, P, sums, d_quant, planes, n_blocks, flags);
    const uint32_t lead = (uint32_t)std::min<unsigned long long>(bytes, (4 - (reinterpret_cast<uintptr_t>(d_out) & 3u)) & 3u);
    const unsigned long long lanes = (bytes - lead) / 4 + lead + (bytes - lead) % 4;
    hipLaunchKernelGGL(jpeg_pixels_kernel, dim3((uint32_t)((lanes + BLOCK - 1) / BLOCK)), dim3(BLOCK), 0, s, P, planes, channels, d_out, bytes, lead, flags);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipMemcpyAsync(h_flags, flags, n_flags * sizeof(uint32_t), hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    return e == hipSuccess ? CVHIP_OK : device_error(what, e);
}

// the pixels into the caller's array, once the flags say that they are good
inline int deliver(const char *what, CallScratch &sc, uint8_t *out, const uint8_t *d_out, unsigned long long bytes, hipStream_t s)
{
    hipError_t e = sc.copy_out(out, d_out, (size_t)bytes, s);
    if (e == hipSuccess) e = sc.drain(s);
    return e == hipSuccess ? CVHIP_OK : device_error(what, e);
}
