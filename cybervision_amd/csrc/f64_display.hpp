// f64_display.hpp — what Rust's `{}` writes for an f64 and for an unsigned integer, as __host__ __device__ code that is also
// plain C++ (tests/cpp/f64_display_host.cpp builds it with g++ alone).  DESIGN.md 4.14.
//
// `{}` on an f64: "NaN" for every NaN, "inf" / "-inf", otherwise an optional '-' and the SHORTEST decimal digit string d1..dk
// with exponent e that reads back as the same double - the closest such string to the exact value - laid out positionally: no
// exponent notation, no trailing ".0", a leading "0." below one ("0" and "-0" for the zeros).
//
// The digits are Schubfach's (R. Giulietti, "The Schubfach way to render doubles"): with the double c * 2^q, k =
// floor(log10(2^q)) (of 3/4 * 2^q at a power of two, whose lower neighbour is half as far) and g = the 128 leading bits of
// 10^-k, rounded up, the three products of g with 4c and the interval's ends 4c -+ 2 - kept to 2 bits below the decimal
// point, with every lower bit folded into the last one - decide exactly which multiples of 10^(k + 1) and of 10^k lie in the
// rounding interval (ends included iff c is even) and which of two is closer.  No value is sent anywhere else: every f64 bit
// pattern is finished here, in 64-bit integer arithmetic (three 128 x 64-bit products from 64-bit halves).
// The power table is f64_pow10.inc, written by scripts/gen_f64_pow10.py with exact integers; that script also checks the three
// fixed-point logarithms below over the ranges they are used on.
//
// Characters go straight to `dst` (LDS or global memory on the device) from digits % 10: there is no private character array.
#pragma once

#include <cstdint>

#if defined(__HIPCC__)
#define F64D_FN __host__ __device__ inline
#else
#define F64D_FN inline
#endif

namespace f64_display {

constexpr int POW10_MIN = -292, POW10_MAX = 324;
static const uint64_t POW10_HOST[POW10_MAX - POW10_MIN + 1][2] = {
#include "f64_pow10.inc"
};
#if defined(__HIPCC__)
static __device__ const uint64_t POW10_DEVICE[POW10_MAX - POW10_MIN + 1][2] = {
#include "f64_pow10.inc"
};
#endif

enum : uint32_t { FINITE = 0, INF = 1, NOT_A_NUMBER = 2 };

// value = (-1)^negative * digits * 10^exp10, digits without trailing zeros (0 for the zeros)
struct Decimal {
    uint64_t digits;
    int32_t exp10;
    uint32_t kind;
    bool negative;
};

F64D_FN uint64_t mul_high(uint64_t a, uint64_t b)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __umul64hi(a, b);
#else
    return (uint64_t)(((unsigned __int128)a * b) >> 64);
#endif
}

// bits 64 .. 127 of the 192-bit product g * cp (those above bit 127 are 0 here), with bit 0 set when any lower bit but the
// lowest two of the middle word is: "round to odd"
F64D_FN uint64_t round_to_odd(uint64_t g_hi, uint64_t g_lo, uint64_t cp)
{
    const uint64_t x_hi = mul_high(g_lo, cp);
    const uint64_t y_lo = g_hi * cp, y_hi = mul_high(g_hi, cp);
    const uint64_t mid = y_lo + x_hi;
    const uint64_t top = y_hi + (mid < y_lo ? 1u : 0u);
    return top | (mid > 1 ? 1u : 0u);
}

F64D_FN uint32_t digits10(uint64_t v)
{
    uint32_t n = 1;
    if (v >= 10000000000000000ull) v /= 10000000000000000ull, n += 16;
    if (v >= 100000000ull) v /= 100000000ull, n += 8;
    uint32_t w = (uint32_t)v;
    if (w >= 10000u) w /= 10000u, n += 4;
    if (w >= 100u) w /= 100u, n += 2;
    if (w >= 10u) n += 1;
    return n;
}

F64D_FN Decimal shortest(double value)
{
    uint64_t bits;
    __builtin_memcpy(&bits, &value, sizeof(bits));
    const uint64_t fraction = bits & ((1ull << 52) - 1);
    const uint32_t exponent = (uint32_t)(bits >> 52) & 0x7FFu;
    Decimal d{0, 0, FINITE, (bits >> 63) != 0};
    if (exponent == 0x7FFu) {
        d.kind = fraction ? NOT_A_NUMBER : INF;
        return d;
    }
    if (exponent == 0 && fraction == 0) return d;
    const uint64_t c = exponent ? (fraction | (1ull << 52)) : fraction;
    const int32_t q = exponent ? (int32_t)exponent - 1075 : -1074;
    const bool even = (c & 1) == 0;
    const bool lower_closer = fraction == 0 && exponent > 1;
    const int32_t k = lower_closer ? (q * 1262611 - 524031) >> 22 : (q * 1262611) >> 22; // floor(log10((3/4) 2^q))
    const int32_t h = q + ((-k * 1741647) >> 19) + 1;                                    // q + floor(log2(10^-k)) + 1: 1 .. 4
#if defined(__HIP_DEVICE_COMPILE__)
    const uint64_t g_hi = POW10_DEVICE[-k - POW10_MIN][0], g_lo = POW10_DEVICE[-k - POW10_MIN][1];
#else
    const uint64_t g_hi = POW10_HOST[-k - POW10_MIN][0], g_lo = POW10_HOST[-k - POW10_MIN][1];
#endif
    const uint64_t cb = 4 * c;
    const uint64_t vbl = round_to_odd(g_hi, g_lo, (cb - 2 + (lower_closer ? 1 : 0)) << h);
    const uint64_t vb = round_to_odd(g_hi, g_lo, cb << h);
    const uint64_t vbr = round_to_odd(g_hi, g_lo, (cb + 2) << h);
    const uint64_t lower = vbl + (even ? 0 : 1), upper = vbr - (even ? 0 : 1);
    const uint64_t s = vb >> 2;
    uint64_t digits;
    int32_t exp10 = k;
    bool done = false;
    if (s >= 10) { // a multiple of 10^(k + 1) in the interval is shorter than any of 10^k
        const uint64_t sp = s / 10;
        const bool lo_in = lower <= 40 * sp, hi_in = 40 * sp + 40 <= upper;
        if (lo_in != hi_in) {
            digits = sp + (hi_in ? 1 : 0), exp10 = k + 1;
            done = true;
        }
    }
    if (!done) {
        const bool lo_in = lower <= 4 * s, hi_in = 4 * s + 4 <= upper;
        if (lo_in != hi_in)
            digits = s + (hi_in ? 1 : 0);
        else { // both or neither: the closer one, ties to even
            const uint64_t mid = 4 * s + 2;
            digits = s + ((vb > mid || (vb == mid && (s & 1))) ? 1 : 0);
        }
    }
    // strip trailing zeros (at most 16: digits < 10^17)
    if (digits % 100000000ull == 0) digits /= 100000000ull, exp10 += 8;
    if (digits % 10000u == 0) digits /= 10000u, exp10 += 4;
    if (digits % 100u == 0) digits /= 100u, exp10 += 2;
    if (digits % 10u == 0) digits /= 10u, exp10 += 1;
    if (digits % 10u == 0) digits /= 10u, exp10 += 1;
    d.digits = digits, d.exp10 = exp10;
    return d;
}

// ---- the positional layout ------------------------------------------------------------------------------------------------------
F64D_FN uint32_t display_len(const Decimal &d)
{
    if (d.kind == NOT_A_NUMBER) return 3;
    const uint32_t sign = d.negative ? 1 : 0;
    if (d.kind == INF) return 3 + sign;
    const int32_t nd = (int32_t)digits10(d.digits), point = nd + d.exp10; // digits in front of the decimal point
    if (d.exp10 >= 0) return sign + (uint32_t)point;
    if (point > 0) return sign + (uint32_t)nd + 1;
    return sign + 2 + (uint32_t)(-point) + (uint32_t)nd;
}

// the `count` low decimal digits of v at dst[0 .. count), most significant first -> v without them
template <typename Byte> F64D_FN uint64_t put_digits(Byte *dst, uint32_t count, uint64_t v)
{
    while (count > 0 && (v >> 32)) dst[--count] = (Byte)('0' + (uint32_t)(v % 10)), v /= 10;
    uint32_t w = (uint32_t)v; // (the rest in 32-bit arithmetic: a 64-bit division by 10 is ~4 times the work on the device)
    if (v >> 32) return v;
    while (count > 0) dst[--count] = (Byte)('0' + w % 10), w /= 10;
    return w;
}

template <typename Byte> F64D_FN uint32_t display_write(Byte *dst, const Decimal &d)
{
    if (d.kind == NOT_A_NUMBER) {
        dst[0] = 'N', dst[1] = 'a', dst[2] = 'N';
        return 3;
    }
    uint32_t p = 0;
    if (d.negative) dst[p++] = '-';
    if (d.kind == INF) {
        dst[p] = 'i', dst[p + 1] = 'n', dst[p + 2] = 'f';
        return p + 3;
    }
    const int32_t nd = (int32_t)digits10(d.digits), point = nd + d.exp10;
    if (d.exp10 >= 0) {
        put_digits(dst + p, (uint32_t)nd, d.digits);
        for (int32_t j = nd; j < point; j++) dst[p + j] = '0';
        return p + (uint32_t)point;
    }
    if (point > 0) {
        const uint64_t whole = put_digits(dst + p + point + 1, (uint32_t)-d.exp10, d.digits);
        dst[p + point] = '.';
        put_digits(dst + p, (uint32_t)point, whole);
        return p + (uint32_t)nd + 1;
    }
    dst[p] = '0', dst[p + 1] = '.';
    for (int32_t j = 0; j < -point; j++) dst[p + 2 + j] = '0';
    put_digits(dst + p + 2 - point, (uint32_t)nd, d.digits);
    return p + 2 + (uint32_t)(-point) + (uint32_t)nd;
}

// `{}` of an f64: its length, and its characters at dst -> the length
F64D_FN uint32_t f64_len(double v) { return display_len(shortest(v)); }
template <typename Byte> F64D_FN uint32_t f64_write(Byte *dst, double v) { return display_write(dst, shortest(v)); }

// `{}` of an unsigned integer
F64D_FN uint32_t u64_len(uint64_t v) { return digits10(v); }
template <typename Byte> F64D_FN uint32_t u64_write(Byte *dst, uint64_t v)
{
    const uint32_t n = digits10(v);
    put_digits(dst, n, v);
    return n;
}

} // namespace f64_display
