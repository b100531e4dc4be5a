// fnn_dist_model.h -- corrected alignment distances: what one lane does with the exact integer counts
// of one (b, i, j) under FNN_DIST_JC69 and FNN_DIST_K2P.  Shared by k_dist_model (fnn_dist.hip) and the CPU driver
// (tests/emu/fnn_dist_model_emu.cpp); tests/dist_model_common.py restates every line with Python floats.
// Below those: dist_log and FNN_DIST_F81 ... FNN_DIST_LOGDET on the exact 4 x 4 table of state pairs,
// shared by k_dist_pairs and tests/emu/fnn_dist_pairs_emu.cpp and restated in tests/dist_pairs_common.py.
// Between them: dist_expm1 and dist_rate_log, gamma-distributed rates for the five logarithmic models,
// restated in tests/dist_gamma_common.py.
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

// e^x - 1 after the published fdlibm algorithm (s_expm1.c): x = k ln 2 + r with |r| <= 0.5 ln 2 (k = +-1 taken directly for
// 0.5 ln 2 < |x| < 1.5 ln 2, else k = (int)(x / ln 2 +- 0.5)) and c the rounding error of r; expm1(r) = r - (r e - hxs) with
// hxs = r^2 / 2, R1 = 1 + hxs (Q1 + ... + hxs Q5), t = 3 - R1 r / 2 and e = hxs ((R1 - t) / (6 - r t)); then one of six
// reconstructions of 2^k (1 + expm1(r)) - 1, the scaling by 2^k an addition to the exponent bits.  NaN gives NaN, +inf and
// every x above 709.78... give +inf, -inf and every x below -56 ln 2 give -1, |x| < 2^-54 gives x.
FNN_HD double dist_expm1(double x) {
    const double ln2_hi = 6.93147180369123816490e-01, ln2_lo = 1.90821492927058770002e-10, invln2 = 1.44269504088896338700e+00;
    const double o_threshold = 7.09782712893383973096e+02;
    const double Q1 = -3.33333333333331316428e-02, Q2 = 1.58730158725481460165e-03, Q3 = -7.93650757867487942473e-05,
                 Q4 = 4.00821782732936239552e-06, Q5 = -2.01099218183624371326e-07;
    const uint64_t bx = dist_bits(x);
    const bool neg = (bx >> 63) != 0;
    const uint32_t hx = (uint32_t)(bx >> 32) & 0x7fffffffu;   // exponent and the top 20 mantissa bits of |x|
    if (hx >= 0x4043687au) {                              // |x| >= 56 ln 2
        if (hx >= 0x40862e42u) {                          // |x| >= 709.78...
            if (hx >= 0x7ff00000u) {
                if (((hx & 0x000fffffu) | (uint32_t)bx) != 0) return x + x;   // NaN
                return neg ? -1.0 : x;
            }
            if (x > o_threshold) return dist_from_bits(0x7ff0000000000000ull);
        }
        if (neg) return -1.0;
    }
    int32_t k = 0;
    double c = 0.0;
    if (hx > 0x3fd62e42u) {                               // |x| > 0.5 ln 2
        double hi, lo;
        if (hx < 0x3ff0a2b2u) {                           // |x| < 1.5 ln 2
            if (!neg) { hi = x - ln2_hi; lo = ln2_lo; k = 1; }
            else { hi = x + ln2_hi; lo = -ln2_lo; k = -1; }
        } else {
            k = (int32_t)(invln2 * x + (neg ? -0.5 : 0.5));
            const double t = (double)k;
            hi = x - t * ln2_hi;
            lo = t * ln2_lo;
        }
        x = hi - lo;
        c = (hi - x) - lo;
    } else if (hx < 0x3c900000u)                          // |x| < 2^-54 (and -0.0 stays -0.0)
        return x;
    const double hfx = 0.5 * x;
    const double hxs = x * hfx;
    const double r1 = 1.0 + hxs * (Q1 + hxs * (Q2 + hxs * (Q3 + hxs * (Q4 + hxs * Q5))));
    double t = 3.0 - r1 * hfx;
    double e = hxs * ((r1 - t) / (6.0 - x * t));
    if (k == 0) return x - (x * e - hxs);
    e = x * (e - c) - c;
    e = e - hxs;
    if (k == -1) return 0.5 * (x - e) - 0.5;
    if (k == 1) {
        if (x < -0.25) return -2.0 * (e - (x + 0.5));
        return 1.0 + 2.0 * (x - e);
    }
    const uint64_t scale = (uint64_t)(int64_t)k << 52;    // k added to the exponent bits
    double y;
    if (k <= -2 || k > 56) {                              // 2^k (1 + expm1(r)) - 1, the 1 inside below an ulp or dominant
        y = 1.0 - (e - x);
        if (k == 1024) y = (y * 2.0) * dist_from_bits(0x7fe0000000000000ull);   // (2^1023: the exponent bits would run over)
        else y = dist_from_bits(dist_bits(y) + scale);
        return y - 1.0;
    }
    if (k < 20) {
        t = dist_from_bits((uint64_t)(0x3ff00000u - (0x00200000u >> k)) << 32);   // 1 - 2^-k
        y = t - (e - x);
        return dist_from_bits(dist_bits(y) + scale);
    }
    t = dist_from_bits((uint64_t)(uint32_t)(0x3ff - k) << 52);                    // 2^-k
    y = x - (e + t);
    y = y + 1.0;
    return dist_from_bits(dist_bits(y) + scale);
}

// ---- rates across sites.  What stands where the equal-rates sequences have log1p'(-y): with shape == 0.0
// (equal rates) that logarithm; with shape = alpha > 0 (gamma-distributed rates) -g, where
//   l = log1p'(-y);  t = (-l) / alpha;  e = expm1'(t);  g = alpha * e          (g = alpha ((1 - y)^(-1/alpha) - 1))
// `over` is set when e is not finite (!(e < inf): a small alpha has pushed t over expm1's overflow threshold); the pair is
// saturated then.  shape is uniform over the wave (a kernel argument).
FNN_HD double dist_rate_log(double y, double shape, bool& over) {
    const double l = dist_log1p(-y);
    if (shape == 0.0) return l;
    const double t = (-l) / shape;
    const double e = dist_expm1(t);
    if (!(e < dist_from_bits(0x7ff0000000000000ull))) over = true;
    const double g = shape * e;
    return -g;
}

// ---- Jukes-Cantor with k states: m mismatches among v common sites (0 < m, 0 < v; k m and (k - 1) v stay below 2^53)
FNN_HD bool dist_jc69_saturated(int64_t k, int64_t m, int64_t v) { return k * m >= (k - 1) * v; }
FNN_HD double dist_jc69(int64_t k, int64_t m, int64_t v, double shape, bool& over) {
    const double y = (double)(k * m) / (double)((k - 1) * v);
    const double e = (double)(k - 1) / (double)k;
    return -(e * dist_rate_log(y, shape, over));
}
FNN_HD double dist_jc69(int64_t k, int64_t m, int64_t v) {
    bool over = false;
    return dist_jc69(k, m, v, 0.0, over);
}

// ---- Kimura two-parameter: ts transitions and tv transversions among v common sites (0 < ts + tv, 0 < v)
FNN_HD bool dist_k2p_saturated(int64_t ts, int64_t tv, int64_t v) { return 2 * ts + tv >= v || 2 * tv >= v; }
FNN_HD double dist_k2p(int64_t ts, int64_t tv, int64_t v, double shape, bool& over) {
    const double y1 = (double)(2 * ts + tv) / (double)v;
    const double y2 = (double)(2 * tv) / (double)v;
    const double a = 0.5 * (-dist_rate_log(y1, shape, over));
    const double b = 0.25 * (-dist_rate_log(y2, shape, over));
    return a + b;
}
FNN_HD double dist_k2p(int64_t ts, int64_t tv, int64_t v) {
    bool over = false;
    return dist_k2p(ts, tv, v, 0.0, over);
}

// log(x) for finite x > 0 after the published fdlibm algorithm (e_log.c): x = 2^k (1 + f) with sqrt(2)/2 < 1 + f < sqrt(2)
// from the exponent bits (a subnormal x is multiplied by 2^54 first), log(1 + f) = f - s (f - R) or f - (f^2/2 - s (f^2/2 + R))
// with s = f / (2 + f) and R the same degree-7 polynomial, here split into its even and odd halves as the source has it, and
// k ln 2 added in two parts.  x <= 0, NaN and +inf are the caller's to keep away; they give NaN here.
FNN_HD double dist_log(double x) {
    const double ln2_hi = 6.93147180369123816490e-01, ln2_lo = 1.90821492927058770002e-10, two54 = 1.80143985094819840000e+16;
    const double Lg1 = 6.666666666666735130e-01, Lg2 = 3.999999999940941908e-01, Lg3 = 2.857142874366239149e-01,
                 Lg4 = 2.222219843214978396e-01, Lg5 = 1.818357216161805012e-01, Lg6 = 1.531383769920937332e-01,
                 Lg7 = 1.479819860511658591e-01;
    if (!(x > 0.0)) return dist_from_bits(0x7ff8000000000000ull);
    int32_t hx = (int32_t)(uint32_t)(dist_bits(x) >> 32);
    if (hx >= 0x7ff00000) return dist_from_bits(0x7ff8000000000000ull);
    int32_t k = 0;
    if (hx < 0x00100000) {                                // subnormal
        k = -54;
        x = x * two54;
        hx = (int32_t)(uint32_t)(dist_bits(x) >> 32);
    }
    k += (hx >> 20) - 1023;
    hx &= 0x000fffff;
    const int32_t i = (hx + 0x95f64) & 0x100000;          // the mantissa is at or above sqrt(2): x / 2^(k + 1)
    x = dist_from_bits(((uint64_t)(uint32_t)(hx | (i ^ 0x3ff00000)) << 32) | (dist_bits(x) & 0xffffffffull));
    k += i >> 20;
    const double f = x - 1.0;
    const double dk = (double)k;
    if ((0x000fffff & (2 + hx)) < 3) {                    // |f| < 2^-20
        if (f == 0.0) {
            if (k == 0) return 0.0;
            return dk * ln2_hi + dk * ln2_lo;
        }
        const double R = f * f * (0.5 - 0.33333333333333333 * f);
        if (k == 0) return f - R;
        return dk * ln2_hi - ((R - dk * ln2_lo) - f);
    }
    const double s = f / (2.0 + f);
    const double z = s * s;
    const double w = z * z;
    const double t1 = w * (Lg2 + w * (Lg4 + w * Lg6));
    const double t2 = z * (Lg1 + w * (Lg3 + w * (Lg5 + w * Lg7)));
    const double R = t2 + t1;
    if (((hx - 0x6147a) | (0x6b851 - hx)) > 0) {
        const double hfsq = 0.5 * f * f;
        if (k == 0) return f - (hfsq - s * (hfsq + R));
        return dk * ln2_hi - ((hfsq - (s * (hfsq + R) + dk * ln2_lo)) - f);
    }
    if (k == 0) return f - s * (f - R);
    return dk * ln2_hi - ((s * (f - R) - dk * ln2_lo) - f);
}

// ---- models on the 4 x 4 table of state pairs: F[4 s + t] = the count-weighted number of sites at which
// the lower-numbered taxon shows code s and the other code t (A 0, C 1, G 2, T 3); every entry, and 2 v, stays below 2^53.
//   v = sum F;  r_s = sum_t F[s][t];  c_t = sum_s F[s][t];  n_s = r_s + c_s;  mism = v - trace F          (integers)
//   ts1 = F[A][G] + F[G][A];  ts2 = F[C][T] + F[T][C];  tv = mism - ts1 - ts2                              (integers)
//   g_s = (double)n_s / (double)(2 v)   - the pair's own base frequencies -;  gR = gA + gG;  gY = gC + gT
// The callers have seen v > 0 and mism > 0.  dist_pairs_kind says what a pair is: DEGENERATE by integer tests alone (F84,
// TN93: some n_s == 0; LogDet: some r_s == 0 or c_s == 0; F81: never, mism > 0 leaves two n_s > 0 and so E > 0), SATURATED
// when an argument y of a logarithm ln(1 - y) is not below 1.0 (`!(y < 1.0)` on the computed double) or LogDet's computed
// determinant is not above 0.0.  The value is computed by the sequences below, one rounding per written operation:
//   F81     sq = ((gA gA + gC gC) + gG gG) + gT gT;  E = 1 - sq;  p = (double)mism / (double)v;  y = p / E;
//           D = -(E * log1p'(-y))
//   F84     ct = gC gT;  ag = gA gG;  A = ct / gY + ag / gR;  B = ct + ag;  C = gR gY;  A2 = 2 A;
//           P = (double)(ts1 + ts2) / (double)v;  Q = (double)tv / (double)v;
//           y1 = P / A2 + ((A - B) Q) / (A2 C);  y2 = Q / (2 C);
//           D = -(A2 * log1p'(-y1)) + (2 ((A - B) - C)) * log1p'(-y2)
//   TN93    k1 = (2 gA gG) / gR  [(2 gA) gG];  k2 = (2 gT gC) / gY  [(2 gT) gC];
//           k3 = 2 ((gR gY - ((gA gG) gY) / gR) - ((gT gC) gR) / gY);
//           P1 = (double)ts1 / (double)v;  P2 = (double)ts2 / (double)v;  Q = (double)tv / (double)v;
//           y1 = P1 / k1 + Q / (2 gR);  y2 = P2 / k2 + Q / (2 gY);  y3 = Q / (2 (gR gY));
//           D = (-(k1 * log1p'(-y1)) - k2 * log1p'(-y2)) - k3 * log1p'(-y3)
//   LogDet  m[s][t] = (double)F[s][t] / (double)v;  det = the cofactor expansion along row 0,
//           det = ((m00 C0 - m01 C1) + m02 C2) - m03 C3,  Ck = det3 of rows 1 ... 3 without column k,
//           det3(a b c / d e f / g h i) = (a (e i - f h) - b (d i - f g)) + c (d h - e g);
//           ls = sum over s = A, C, G, T in turn, from 0.0, of (log'(r_s / v) + log'(c_s / v));
//           D = -(0.25 * (log'(det) - 0.5 * ls))
enum { DIST_KIND_OK = 0, DIST_KIND_DEGENERATE = 1, DIST_KIND_SATURATED = 2 };

struct DistTable {
    int64_t F[16];
    int64_t v, mism, ts1, ts2, tv, r[4], c[4];
};
FNN_HD void dist_table_sums(DistTable& t) {
#pragma unroll
    for (int s = 0; s < 4; s++) t.r[s] = ((t.F[4 * s] + t.F[4 * s + 1]) + t.F[4 * s + 2]) + t.F[4 * s + 3];
#pragma unroll
    for (int s = 0; s < 4; s++) t.c[s] = ((t.F[s] + t.F[4 + s]) + t.F[8 + s]) + t.F[12 + s];
    t.v = ((t.r[0] + t.r[1]) + t.r[2]) + t.r[3];
    t.mism = t.v - (((t.F[0] + t.F[5]) + t.F[10]) + t.F[15]);
    t.ts1 = t.F[2] + t.F[8];
    t.ts2 = t.F[7] + t.F[13];
    t.tv = t.mism - t.ts1 - t.ts2;
}
FNN_HD double dist_pair_freq(const DistTable& t, int s) { return (double)(t.r[s] + t.c[s]) / (double)(2 * t.v); }
FNN_HD bool dist_pair_lacks_a_base(const DistTable& t) {
    return t.r[0] + t.c[0] == 0 || t.r[1] + t.c[1] == 0 || t.r[2] + t.c[2] == 0 || t.r[3] + t.c[3] == 0;
}

FNN_HD int32_t dist_f81(const DistTable& t, double& D, double shape = 0.0) {
    const double gA = dist_pair_freq(t, 0), gC = dist_pair_freq(t, 1), gG = dist_pair_freq(t, 2), gT = dist_pair_freq(t, 3);
    const double sq = ((gA * gA + gC * gC) + gG * gG) + gT * gT;
    const double E = 1.0 - sq;
    const double p = (double)t.mism / (double)t.v;
    const double y = p / E;
    if (!(y < 1.0)) return DIST_KIND_SATURATED;
    bool over = false;
    D = -(E * dist_rate_log(y, shape, over));
    return over ? DIST_KIND_SATURATED : DIST_KIND_OK;
}
FNN_HD int32_t dist_f84(const DistTable& t, double& D, double shape = 0.0) {
    if (dist_pair_lacks_a_base(t)) return DIST_KIND_DEGENERATE;
    const double gA = dist_pair_freq(t, 0), gC = dist_pair_freq(t, 1), gG = dist_pair_freq(t, 2), gT = dist_pair_freq(t, 3);
    const double gR = gA + gG, gY = gC + gT;
    const double ct = gC * gT, ag = gA * gG;
    const double A = ct / gY + ag / gR;
    const double B = ct + ag;
    const double Cc = gR * gY;
    const double A2 = 2.0 * A;
    const double P = (double)(t.ts1 + t.ts2) / (double)t.v;
    const double Q = (double)t.tv / (double)t.v;
    const double y1 = P / A2 + ((A - B) * Q) / (A2 * Cc);
    const double y2 = Q / (2.0 * Cc);
    if (!(y1 < 1.0) || !(y2 < 1.0)) return DIST_KIND_SATURATED;
    bool over = false;
    D = -(A2 * dist_rate_log(y1, shape, over)) + (2.0 * ((A - B) - Cc)) * dist_rate_log(y2, shape, over);
    return over ? DIST_KIND_SATURATED : DIST_KIND_OK;
}
FNN_HD int32_t dist_tn93(const DistTable& t, double& D, double shape = 0.0) {
    if (dist_pair_lacks_a_base(t)) return DIST_KIND_DEGENERATE;
    const double gA = dist_pair_freq(t, 0), gC = dist_pair_freq(t, 1), gG = dist_pair_freq(t, 2), gT = dist_pair_freq(t, 3);
    const double gR = gA + gG, gY = gC + gT;
    const double k1 = ((2.0 * gA) * gG) / gR;
    const double k2 = ((2.0 * gT) * gC) / gY;
    const double k3 = 2.0 * ((gR * gY - ((gA * gG) * gY) / gR) - ((gT * gC) * gR) / gY);
    const double P1 = (double)t.ts1 / (double)t.v;
    const double P2 = (double)t.ts2 / (double)t.v;
    const double Q = (double)t.tv / (double)t.v;
    const double y1 = P1 / k1 + Q / (2.0 * gR);
    const double y2 = P2 / k2 + Q / (2.0 * gY);
    const double y3 = Q / (2.0 * (gR * gY));
    if (!(y1 < 1.0) || !(y2 < 1.0) || !(y3 < 1.0)) return DIST_KIND_SATURATED;
    bool over = false;
    D = (-(k1 * dist_rate_log(y1, shape, over)) - k2 * dist_rate_log(y2, shape, over)) - k3 * dist_rate_log(y3, shape, over);
    return over ? DIST_KIND_SATURATED : DIST_KIND_OK;
}
FNN_HD double dist_det3(double a, double b, double c, double d, double e, double f, double g, double h, double i) {
    return (a * (e * i - f * h) - b * (d * i - f * g)) + c * (d * h - e * g);
}
FNN_HD int32_t dist_logdet(const DistTable& t, double& D) {
    bool lacks = false;
#pragma unroll
    for (int s = 0; s < 4; s++) lacks = lacks || t.r[s] == 0 || t.c[s] == 0;
    if (lacks) return DIST_KIND_DEGENERATE;
    const double v = (double)t.v;
    double m[16];
#pragma unroll
    for (int k = 0; k < 16; k++) m[k] = (double)t.F[k] / v;
    const double C0 = dist_det3(m[5], m[6], m[7], m[9], m[10], m[11], m[13], m[14], m[15]);
    const double C1 = dist_det3(m[4], m[6], m[7], m[8], m[10], m[11], m[12], m[14], m[15]);
    const double C2 = dist_det3(m[4], m[5], m[7], m[8], m[9], m[11], m[12], m[13], m[15]);
    const double C3 = dist_det3(m[4], m[5], m[6], m[8], m[9], m[10], m[12], m[13], m[14]);
    const double det = ((m[0] * C0 - m[1] * C1) + m[2] * C2) - m[3] * C3;
    if (!(det > 0.0)) return DIST_KIND_SATURATED;
    double ls = 0.0;
#pragma unroll
    for (int s = 0; s < 4; s++) ls = ls + (dist_log((double)t.r[s] / v) + dist_log((double)t.c[s] / v));
    D = -(0.25 * (dist_log(det) - 0.5 * ls));
    return DIST_KIND_OK;
}

}  // namespace fnn
#endif
