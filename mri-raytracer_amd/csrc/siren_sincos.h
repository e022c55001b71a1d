// STRICT sine and cosine of an fp32 argument for the SIREN training step: the fp32 argument widened to
// fp64, reduced by multiples of pi/2 with a three-constant Cody-Waite split, sine and cosine polynomials in fp64, picked by
// quadrant, rounded ONCE to fp32 -- the construction of exp_f64_to_f32 (mrirt_device.h).  Only correctly rounded fp64 *, +, -,
// rint and conversions, in the written order and unfused (the library is built with -ffp-contract=off and no fma is asked
// for), so tests/inr_siren_ref.py restates it in NumPy float64 operation by operation and gets the same bits.
//
// Domain: |a| <= 2^20.  There k = rint(a 2/pi) has at most 20 bits, so k P1 (P1: the leading 33 bits of pi/2) is exact, and
// the reduced r = ((a - k P1) - k P2) - k P3 is within 2^-60 of a - k pi/2 in absolute terms while |r| <= pi/4 + 2^-30.  The
// Taylor polynomials to r^17 / r^16 are then within 2^-58 of sin r / cos r (first dropped terms (pi/4)^19 / 19!,
// (pi/4)^18 / 18!), i.e. the fp64 value carries < 2^-5 fp32 ulp of error before the single rounding: measured 0 differences
// from float32(sin(float64(a))) on 2.2 M arguments, worst error 0.4999999 fp32 ulp.
// Beyond the domain: a finite a is replaced by a * 0 (sin = +0, cos = 1; +0 for a negative a too, and for a = -0, since then
// r = -0 - (-0 * P1) = +0); NaN and +-inf give NaN for both, since a * 0 is then NaN.  k is never converted to an integer: the
// quadrant is k - 4 rint(k / 4), compared as an fp64 value.
#pragma once
#include "mrirt_device.h"

namespace mrirt {

constexpr double kSinDomain = 1048576.0;                     // 2^20
constexpr double kTwoOverPi = 0x1.45f306dc9c883p-1;
constexpr double kPio2_1 = 0x1.921fb54400000p+0;             // 33 bits of pi/2
constexpr double kPio2_2 = 0x1.0b4611a600000p-34;            // the next 33
constexpr double kPio2_3 = 0x1.3198a2e037073p-69;            // the next 53

MRIRT_HD void siren_sincos(float a, float& sn, float& cs) {
    double x = (double)a;
    x = __builtin_fabs(x) <= kSinDomain ? x : x * 0.0;       // NaN and +-inf: NaN from here on
    const double k = __builtin_rint(x * kTwoOverPi);
    double r = x - k * kPio2_1;
    r = r - k * kPio2_2;
    r = r - k * kPio2_3;
    const double r2 = r * r;
    double s = 0x1.952c77030ad4ap-49 * r2;                   // 1/17!
    s = (s + -0x1.ae7f3e733b81fp-41) * r2;                   // -1/15!
    s = (s + 0x1.6124613a86d09p-33) * r2;
    s = (s + -0x1.ae64567f544e4p-26) * r2;
    s = (s + 0x1.71de3a556c734p-19) * r2;
    s = (s + -0x1.a01a01a01a01ap-13) * r2;
    s = (s + 0x1.1111111111111p-7) * r2;
    s = (s + -0x1.5555555555555p-3) * r2;                    // -1/3!
    s = r + r * s;
    double c = 0x1.ae7f3e733b81fp-45 * r2;                   // 1/16!
    c = (c + -0x1.93974a8c07c9dp-37) * r2;
    c = (c + 0x1.1eed8eff8d898p-29) * r2;
    c = (c + -0x1.27e4fb7789f5cp-22) * r2;
    c = (c + 0x1.a01a01a01a01ap-16) * r2;
    c = (c + -0x1.6c16c16c16c17p-10) * r2;
    c = (c + 0x1.5555555555555p-5) * r2;
    c = (c + -0.5) * r2;                                     // -1/2!
    c = 1.0 + c;
    const double q = k - 4.0 * __builtin_rint(k * 0.25);     // -2 .. 2 (+-2: the same quadrant); NaN for a NaN
    double so, co;
    if (q == 0.0) { so = s; co = c; }
    else if (q == 1.0) { so = c; co = -s; }
    else if (q == 2.0 || q == -2.0) { so = -s; co = -c; }
    else { so = -c; co = s; }                                // q == -1, and the NaN
    sn = (float)so;
    cs = (float)co;
}

}  // namespace mrirt
