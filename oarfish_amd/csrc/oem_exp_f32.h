// oem_exp_f32.h -- expf of a continuous f32 argument, for code that has to give the host libm's answer bit for bit.
//
// Rust's f32::exp lowers to libm's expf, and that function is this project's definition of as_prob on the projected path
// (oem_filter_projected.h).  expf is not the correctly rounded function, so no independent exponential equals it
// everywhere; but it errs by far less than half an ulp before its final rounding (glibc documents 0.502 ulp in all, i.e.
// 0.002 ulp before rounding), so it DOES return the correctly rounded f32 wherever the exact value is not close to a
// rounding tie.  exp_f32_candidate computes c = (float)exp((double)f) and says whether that is such a place:
//
//   *sure == true    c is the correctly rounded f32 of e^f, and every expf that errs by less than 1/256 ulp before
//                    rounding returns c too.  The f64 exp used here may be the host's or the device's: they differ by a
//                    few f64 ulps, 2^21 times less than the margin.
//   *sure == false   nothing is promised: the caller asks libm's expf.  That is the case when f is not finite, when
//                    f > 0 (the projected path's arguments are <= 0; the rest is left to libm), when c is below FLT_MIN
//                    (subnormal results, where an f32 ulp is no longer 2^-23 of the value) or when the f64 value lies
//                    within 1/256 of an f32 ulp of the midpoint between two f32 neighbours.
//
// The tie test reads the f64's bits: for a normal f32 result the 29 mantissa bits below f32 precision are the position
// between two f32 neighbours in units of 2^-29 ulp, the midpoint is 2^28 and the margin 2^29 / 256 = 2^21.
#pragma once

#include <math.h>
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

constexpr float kExpF32Min = 1.17549435e-38f;        // FLT_MIN
constexpr int64_t kExpTieMargin = 1ll << 21;         // 1/256 of an f32 ulp, in units of the f64's last 29 bits

OEM_HD inline float exp_f32_candidate(float f, bool *sure)
{
    const double d = exp((double)f);
    const float c = (float)d;
    *sure = false;
    if (!(f <= 0.0f) || f < -3.4028234663852886e38f) return c;      // NaN, positive, -inf
    if (!(c >= kExpF32Min) || !(d >= (double)kExpF32Min)) return c; // the result, or the value before rounding, is subnormal
    uint64_t bits;
    memcpy(&bits, &d, sizeof(bits));
    const int64_t below = (int64_t)(bits & ((1ull << 29) - 1));      // position between the two f32 neighbours
    const int64_t off = below - (1ll << 28);
    *sure = off > kExpTieMargin || off < -kExpTieMargin;
    return c;
}

} // namespace oem
