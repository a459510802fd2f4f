// model_math.hpp -- what a user's header may call PER ELEMENT besides + - * / sqrt fma (include/muse_model.h): the exponential.
// muse::model_exp(x) returns, for every double x, the BITS of muse::muse_exp(x) (step.hpp; restated by the CPU checker's mo_exp) --
// NaN, +-inf, +-0, both cut-offs and subnormal results included -- by another instruction sequence, one the LDS-resident solve can
// afford ten times per thread and evaluation:
//   * one straight-line body.  The argument is clamped into the range the cut-offs leave (so that the conversion to an integer is
//     defined for every x) and the three special results are selected at the end: no branch, nothing live across one.
//   * the division (r c) / (2 - c) by a reciprocal: the denominator lies in [1.2, 2.8] and the numerator below 0.2 in size, so none of
//     the range scaling of a general IEEE division (div_scale / div_fmas / div_fixup) is needed.  Seed, two Newton steps, the product
//     and ONE fused residual correction -- the sequence the compiler's own division ends in -- give the correctly rounded quotient
//     wherever the quotient can change the result: where the numerator r c ~ r^2 is so small (below 2^-960) that the residual itself
//     rounds, the quotient is below 2^-400 of what it is subtracted from (lo, or r itself when k = 0) and is absorbed whatever
//     its last bit.
//   * the scaling by 2^k through ldexp (v_ldexp_f64) instead of a power of two assembled in the exponent field: y 2^k is exact where
//     the result is normal; where it is subnormal muse_exp's two-step product (y 2^(k + 1000)) 2^-1000 rounds once, in its second
//     step, and so does ldexp; for k = 1024 muse_exp's (2 y) 2^1023 and ldexp(y, 1024) both round (or overflow) y 2^1024 once.
// The polynomial, the reduction and their order are muse_exp's, statement by statement (compiled without contraction, as everything).
// The host keeps muse::muse_exp; this file compiles for the host as well -- with the seed below -- only so that the sequence can be
// checked without a device (tests/native/model_exp_driver.cpp).
#pragma once
#include <math.h>

#if defined(__HIPCC__)
#define MUSE_MM_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define MUSE_MM_HD inline
#endif

// the reciprocal's seed: the hardware's on the device (v_rcp_f64); on the host a single-precision-accurate one, so that a host
// evaluation exercises the refinement (a test may supply its own, worse, seed)
#ifndef MUSE_MM_RCP_SEED
#if defined(__HIP_DEVICE_COMPILE__)
#define MUSE_MM_RCP_SEED(d) __builtin_amdgcn_rcp(d)
#else
#define MUSE_MM_RCP_SEED(d) ((double)(float)(1.0 / (d)))
#endif
#endif

namespace muse {

// n / d for d in [1, 4] and |n| <= 1: the correctly rounded quotient (see above for |n| < 2^-960)
MUSE_MM_HD double model_div_unscaled(double n, double d) {
    double y = MUSE_MM_RCP_SEED(d);
    y = fma(y, fma(-d, y, 1.0), y);
    y = fma(y, fma(-d, y, 1.0), y);
    const double q = n * y;
    return fma(fma(-d, q, n), y, q);
}

MUSE_MM_HD double model_exp(double x) {
    const double ln2HI = 6.93147180369123816490e-01, ln2LO = 1.90821492927058770002e-10, invln2 = 1.44269504088896338700e+00,
                 P1 = 1.66666666666666019037e-01, P2 = -2.77777777770155933842e-03, P3 = 6.61375632143793436117e-05,
                 P4 = -1.65339022054652515390e-06, P5 = 4.13813679705723846039e-08;
    // inside the cut-offs xc == x; beyond them (and for NaN: fmax / fmin return the other operand) any finite stand-in
    const double xc = fmin(fmax(x, -746.0), 710.0);
    const int k = (int)(invln2 * xc + (xc < 0.0 ? -0.5 : 0.5));   // -1076 .. 1024
    const double dk = (double)k;
    const double hi = xc - dk * ln2HI, lo = dk * ln2LO;
    const double r = hi - lo;
    const double t = r * r;
    const double c = r - t * (P1 + t * (P2 + t * (P3 + t * (P4 + t * P5))));
    const double y = 1.0 - ((lo - model_div_unscaled(r * c, 2.0 - c)) - hi);
    double e = ldexp(y, k);
    e = x > 7.09782712893383973096e+02 ? (double)INFINITY : e;
    e = x < -7.45133219101941108420e+02 ? 0.0 : e;
    return x != x ? x : e;
}

}  // namespace muse
