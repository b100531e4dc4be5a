// fnn_dist_model.h -- corrected alignment distances: what one lane does with the exact integer counts
// of one (b, i, j) under FNN_DIST_JC69 and FNN_DIST_K2P.  Shared by k_dist_model (fnn_dist.hip) and the CPU driver
// (tests/emu/fnn_dist_model_emu.cpp); tests/dist_model_common.py restates every line with Python floats.
//
// Every fp64 step below is ONE written operation with one rounding (-ffp-contract=off on host and device): + - * / and
// conversions of integers below 2^53 only.  No fma, no libm, no ocml: the bits are the same in all three places.
#ifndef FNN_DIST_MODEL_H
#define FNN_DIST_MODEL_H

#include <stdint.h>

#include "fnn_core.h"  // FNN_HD

namespace fnn {

FNN_HD uint64_t dist_bits(double x) {
    uint64_t u;
    __builtin_memcpy(&u, &x, 8);
    return u;
}
FNN_HD double dist_from_bits(uint64_t u) {
    double x;
    __builtin_memcpy(&x, &u, 8);
    return x;
}

// log(1 + x) for x > -1 after the published fdlibm algorithm: 1 + x = 2^k (1 + f) with sqrt(2)/2 < 1 + f < sqrt(2) from the
// exponent bits of u = 1 + x (and the rounding error of that sum as a correction c), log(1 + f) = f - f^2/2 + s (f^2/2 + R)
// with s = f / (2 + f) and R a degree-7 polynomial in s^2, and k ln 2 added in two parts.  x <= -1 and NaN are the
// caller's to keep away (the saturation test is an integer test); they give NaN here.
FNN_HD double dist_log1p(double x) {
    const double ln2_hi = 6.93147180369123816490e-01, ln2_lo = 1.90821492927058770002e-10;
    const double Lp1 = 6.666666666666735130e-01, Lp2 = 3.999999999940941908e-01, Lp3 = 2.857142874366239149e-01,
                 Lp4 = 2.222219843214978396e-01, Lp5 = 1.818357216161805012e-01, Lp6 = 1.531383769920937332e-01,
                 Lp7 = 1.479819860511658591e-01;
    const uint64_t bx = dist_bits(x);
    const int32_t hx = (int32_t)(uint32_t)(bx >> 32);     // sign, exponent and the top 20 mantissa bits
    const int32_t ax = hx & 0x7fffffff;
    if (!(x > -1.0) || ax >= 0x7ff00000) return dist_from_bits(0x7ff8000000000000ull);
    int32_t k = 1, hu = 1;
    double f = 0.0, c = 0.0;
    if (hx < 0x3fda827a) {                                // x < sqrt(2) - 1
        if (ax < 0x3e200000) {                            // |x| < 2^-29
            if (ax < 0x3c900000) return x;                // |x| < 2^-54 (and -0.0 stays -0.0)
            return x - x * x * 0.5;
        }
        if (hx > 0 || hx <= (int32_t)0xbfd2bec3u) {       // sqrt(2)/2 - 1 < x: no reduction
            k = 0;
            f = x;
            hu = 1;
        }
    }
    if (k != 0) {
        double u;
        if (hx < 0x43400000) {                            // x < 2^53
            u = 1.0 + x;
            hu = (int32_t)(uint32_t)(dist_bits(u) >> 32);
            k = (hu >> 20) - 1023;
            c = k > 0 ? 1.0 - (u - x) : x - (u - 1.0);    // what the sum 1 + x lost
            c = c / u;
        } else {
            u = x;
            hu = (int32_t)(uint32_t)(dist_bits(u) >> 32);
            k = (hu >> 20) - 1023;
            c = 0.0;
        }
        hu &= 0x000fffff;
        const uint64_t lo = dist_bits(u) & 0xffffffffull;
        if (hu < 0x6a09e) {                               // mantissa below sqrt(2): u / 2^k
            u = dist_from_bits(((uint64_t)(uint32_t)(hu | 0x3ff00000) << 32) | lo);
        } else {                                          // u / 2^(k + 1)
            k += 1;
            u = dist_from_bits(((uint64_t)(uint32_t)(hu | 0x3fe00000) << 32) | lo);
            hu = (0x00100000 - hu) >> 2;
        }
        f = u - 1.0;
    }
    const double dk = (double)k;
    const double hfsq = 0.5 * f * f;
    if (hu == 0) {                                        // |f| < 2^-20
        if (f == 0.0) {
            if (k == 0) return 0.0;
            c = c + dk * ln2_lo;
            return dk * ln2_hi + c;
        }
        const double R = hfsq * (1.0 - 0.66666666666666666 * f);
        if (k == 0) return f - R;
        return dk * ln2_hi - ((R - (dk * ln2_lo + c)) - f);
    }
    const double s = f / (2.0 + f);
    const double z = s * s;
    const double R = z * (Lp1 + z * (Lp2 + z * (Lp3 + z * (Lp4 + z * (Lp5 + z * (Lp6 + z * Lp7))))));
    if (k == 0) return f - (hfsq - s * (hfsq + R));
    return dk * ln2_hi - ((hfsq - (s * (hfsq + R) + (dk * ln2_lo + c))) - f);
}

// ---- Jukes-Cantor with k states: m mismatches among v common sites (0 < m, 0 < v; k m and (k - 1) v stay below 2^53)
FNN_HD bool dist_jc69_saturated(int64_t k, int64_t m, int64_t v) { return k * m >= (k - 1) * v; }
FNN_HD double dist_jc69(int64_t k, int64_t m, int64_t v) {
    const double y = (double)(k * m) / (double)((k - 1) * v);
    const double e = (double)(k - 1) / (double)k;
    return -(e * dist_log1p(-y));
}

// ---- Kimura two-parameter: ts transitions and tv transversions among v common sites (0 < ts + tv, 0 < v)
FNN_HD bool dist_k2p_saturated(int64_t ts, int64_t tv, int64_t v) { return 2 * ts + tv >= v || 2 * tv >= v; }
FNN_HD double dist_k2p(int64_t ts, int64_t tv, int64_t v) {
    const double y1 = (double)(2 * ts + tv) / (double)v;
    const double y2 = (double)(2 * tv) / (double)v;
    const double a = 0.5 * (-dist_log1p(-y1));
    const double b = 0.25 * (-dist_log1p(-y2));
    return a + b;
}

}  // namespace fnn
#endif
