// oem_text_format.h -- the numbers of a `.prob` line as decimal text, exactly and without floating point.
//
// Reference (COMBINE-lab/oarfish v0.10.3, src/util/write_function.rs:320-331): transcript ids with `{}`, probabilities
// with `{:.d}` (d = prob_display_decimals, :218-224).  Rust's `{:.d}` of an f64 is the exact binary value rounded
// correctly to d decimals, ties to even; glibc's `%.*f` and Python's `f"{x:.{d}f}"` print the same.  The functions
// here are pure (host and device; nothing from HIP, so a host compiler builds them and tests/test_text_format.py holds
// them to Python's formatting at the ties): every printer comes as a pair, `*_len` (the bytes it will write) and
// `emit_*` (writes them, returns the byte after the last), so the kernel that measures a line and the kernel that
// writes it cannot disagree.
#pragma once

#include <stdint.h>
#include <string.h>

#ifndef OEM_HD
#ifdef __HIPCC__
#include <hip/hip_runtime.h>
#define OEM_HD __host__ __device__
#else
#define OEM_HD
#endif
#endif

namespace oem {

// -- unsigned decimals -------------------------------------------------------------------------------------------------
OEM_HD inline uint32_t u32_dec_len(uint32_t v)
{
    uint32_t n = 1;
    while (v >= 10u) {
        v /= 10u;
        ++n;
    }
    return n;
}

OEM_HD inline uint32_t u64_dec_len(uint64_t v)
{
    uint32_t n = 1;
    while (v >> 32) { // the high digits with 64-bit division, the rest (the common case: all of it) with 32-bit
        v /= 10u;
        ++n;
    }
    return n - 1 + u32_dec_len((uint32_t)v);
}

// the low `n` digits of v at p[0 .. n), most significant first (zero-padded on the left)
OEM_HD inline void put_digits_u32(uint8_t *p, uint32_t v, uint32_t n)
{
    while (n) {
        p[--n] = (uint8_t)('0' + v % 10u);
        v /= 10u;
    }
}

OEM_HD inline uint8_t *emit_u32(uint8_t *p, uint32_t v)
{
    const uint32_t n = u32_dec_len(v);
    put_digits_u32(p, v, n);
    return p + n;
}

OEM_HD inline uint8_t *emit_u64(uint8_t *p, uint64_t v)
{
    uint32_t n = u64_dec_len(v);
    uint8_t *const end = p + n;
    while (v >> 32) {
        p[--n] = (uint8_t)('0' + (uint32_t)(v % 10u));
        v /= 10u;
    }
    put_digits_u32(p, (uint32_t)v, n);
    return end;
}

// -- fixed-point decimals of an f64 ------------------------------------------------------------------------------------
// 10^d for the decimals a `.prob` file uses (3 .. 9; anything up to 9 fits a u32)
OEM_HD inline uint32_t pow10_u32(uint32_t d)
{
    uint32_t p = 1;
    while (d--) p *= 10u;
    return p;
}

OEM_HD inline uint64_t f64_bits(double x)
{
    uint64_t b;
    memcpy(&b, &x, sizeof b);
    return b;
}

OEM_HD inline bool f64_is_nan(uint64_t bits) { return (bits & 0x7fffffffffffffffull) > 0x7ff0000000000000ull; }

// |x| * 10^d rounded to an integer, correctly on the exact binary value and ties to even, for finite |x| < 2^20 and
// d <= 9.  |x| = m * 2^-s with m < 2^53, so N = m * 10^d < 2^83 is exact in 128 bits; q = N >> s with the remainder
// deciding the rounding.  s >= 128 leaves q = 0 and a remainder N < 2^83 <= half: never rounded up.  (|x| < 2^20 has
// s >= 33; a value of 2^53 or more, s <= 0, would shift left -- outside what this prints, and kept only so that the
// function is total.)
OEM_HD inline uint64_t fixed_round(uint64_t bits, uint32_t d)
{
    const uint32_t e = (uint32_t)(bits >> 52) & 0x7ffu;
    const uint64_t frac = bits & 0x000fffffffffffffull;
    const uint64_t m = e ? (frac | 0x0010000000000000ull) : frac;
    const int s = 1075 - (int)(e ? e : 1u);
    const unsigned __int128 N = (unsigned __int128)m * pow10_u32(d);
    if (s <= 0) return (uint64_t)(N << (s > -44 ? -s : 44));
    if (s >= 128) return 0;
    uint64_t q = (uint64_t)(N >> s);
    const unsigned __int128 rem = N & ((((unsigned __int128)1) << s) - 1);
    const unsigned __int128 half = ((unsigned __int128)1) << (s - 1);
    if (rem > half || (rem == half && (q & 1u))) ++q;
    return q;
}

// Bytes of `{:.d}` of x: "NaN" for a NaN (Rust prints no sign for it), else [-] integer digits . d digits.
OEM_HD inline uint32_t fixed_len(double x, uint32_t d)
{
    const uint64_t bits = f64_bits(x);
    if (f64_is_nan(bits)) return 3;
    const uint32_t sign = (uint32_t)(bits >> 63);
    // below 9 the rounded value is below 10: one integer digit, whatever the rounding does (a probability always is)
    if ((bits & 0x7fffffffffffffffull) < 0x4022000000000000ull) return sign + 2 + d;
    return sign + u64_dec_len(fixed_round(bits, d) / pow10_u32(d)) + 1 + d;
}

OEM_HD inline uint8_t *emit_fixed(uint8_t *p, double x, uint32_t d)
{
    const uint64_t bits = f64_bits(x);
    if (f64_is_nan(bits)) {
        p[0] = 'N';
        p[1] = 'a';
        p[2] = 'N';
        return p + 3;
    }
    if (bits >> 63) *p++ = '-';
    const uint64_t q = fixed_round(bits, d);
    const uint32_t p10 = pow10_u32(d);
    uint32_t fr;
    if (q >> 32) {
        p = emit_u64(p, q / p10);
        fr = (uint32_t)(q % p10);
    } else { // a probability: q <= 10^9, 32-bit division
        p = emit_u32(p, (uint32_t)q / p10);
        fr = (uint32_t)q % p10;
    }
    *p++ = '.';
    put_digits_u32(p, fr, d);
    return p + d;
}

} // namespace oem
