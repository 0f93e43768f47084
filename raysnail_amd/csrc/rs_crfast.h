// Fast paths that return the bits of include/rs_crmath.h's sincos_cr and sin3_negative for every input, host and
// device. rs_crmath.h is the oracle's and stays as it is; the kernels' call sites (rs_device.h) call these, so the GPU
// parity tests against the oracle check this header independently. -DRS_CRFAST=0 builds the original calls.
//
// sincos_cr_fast
// --------------
// sincos_cr evaluates both Taylor series in double-double down to the coefficient of z^7 (8 steps of the 27-operation
// mul + add pair each) for about 2^-100, and keeps the leading double. Here the plain-double Horner part runs four
// steps further (down to z^4), the double-double part keeps the last four steps (z^3 .. z^0) with a cheaper add, and a
// rounding test says whether the 53 bits kept can depend on what was left out. If it says they might, sin_poly and
// cos_poly run on the same r, z: the original code.
//
// E, the relative distance between the fast double-double and the full one. Both start from the same r = reduce_pio2(x)
// and z = r r, with |k| < 2^20, so |r| <= pi/4 + 2^-32 and z <= 0.6169. Write c_j for the series' coefficient of z^j
// (|c_j| = 1/(2j)! for cos, 1/(2j+1)! for sin/r), P_j for the full path's value at level j (c_j + z P_{j+1}), and u = 2^-53.
//  (1) Level 4 in plain double, q = fl(c_4.h + fl(t_5 z.h)), against P_4. What differs: c_4.l dropped (<= u |c_4|); the
//      rounding of the sum (<= u |q| <= u |c_4|, the series alternates and decreases); the rounding of the product, of
//      t_5 itself and its dropped c_5.l, and z.h for z (each <= u |c_5| z, and |c_5| z <= 0.0069 |c_4| for cos, 0.0057
//      for sin; what t_6 .. contribute to t_5 is below u |c_5| / 100). So |q - P_4| <= 2.03 u |c_4|.
//  (2) That reaches the result multiplied by z^4: z^4 |c_4| <= 0.6169^4 / 8! = 2^-18.09 for cos, whose value is >=
//      cos(pi/4 + 2^-32) = 0.7071: relative 2.03 * 2^-53 * 2^-18.09 / 0.7071 = 2^-69.57. For sin it is 0.6169^4 / 9!
//      = 2^-21.26 against sin(r)/r >= 0.9003: 2^-73.1, and the last mul(r, p) is the same code in both.
//  (3) The four double-double steps. mul is the header's (relative error <= 2^-104 for the DD x DD form, and the first
//      step's DD x double form is the same operations without a zero term). add_ord(c, a) needs |c.h| >= |a.h|, which
//      holds at every level: |P_{j+1}| <= |c_{j+1}| <= |c_j| / 2, so |z P_{j+1}| < 0.31 |c_j|. Then s = fl(c.h + a.h) with the
//      exact error e1 (Dekker), v = fl(c.l + a.l) is off by <= u (u |c.h| + u |a.h|) <= 2^-105 |c.h|, w = fl(e1 + v) by
//      <= u |w| <= 2^-104 |c.h|, and the closing quick_two_sum is exact: <= 2^-103 |c_j| per step, z^j |c_j| <= 1, four
//      steps, value >= 0.7071: below 2^-100 in all. The full path's own arithmetic on those steps is below 2^-100 too
//      (the header's figure for all sixteen).
//  So E <= 2^-69.57 + 2^-99 < 2^-69.5 for either value.
//
// The rounding test. The fast value (h, l) is normalised (quick_two_sum), h = RN(h + l). With e = M |h|, M = 2^-67, it
// passes when fl(h + fl(l - e)) == fl(h + fl(l + e)); fl(l -+ e) is off by <= u (|l| + e) <= 2^-105 |h|. Rounding is
// monotone, so every real in [h + l - e', h + l + e'], e' = (M - 2^-105) |h|, then rounds to that one double, which is
// h because h + l is among them. M >= 4 E + 2^-100 + 2^-105 (4 * 2^-69.5 = 2^-67.5 = 0.71 M): the full double-double
// F = (H, L) has |F - (h + l)| <= E |F| <= 1.01 E |h| < e', and so has the true value, within 2^-100 |F| of F. F is
// normalised too, so sin_poly(..).h = H = RN(H + L) = h. When the test fails the original code runs. A value falls
// back when a rounding boundary of its binade lies within e of it: 2 M |h| / ulp(h) in [2^-14, 2^-13) of the values.
//
// Outside |k| < 2^20 (the reduction is no longer exact and r is not bounded) and for |x| < 2^-500 (where z and e can
// underflow) nothing above is claimed, and the original code runs.
//
// sin3_negative_fast
// ------------------
// sin_sign needs the quadrant k and the sign of r.h only. reduce_pio2's first two lines give k and t1 = x - k C1; the
// three further terms it subtracts total less than |k| 2^-33 (C2 = 1.05 * 2^-34 and the rest below 2^-68 per unit of
// k). When |k| < 2^20 and |t1| > |k| 2^-30 what remains is below |t1| / 8, the double-double sums are accurate to
// 2^-100, and so r.h has t1's sign (k = 0: r.h = x). Otherwise sin_sign itself runs.
#pragma once
#include "../../include/rs_crmath.h"

#ifndef RS_CRFAST
#define RS_CRFAST 1
#endif

namespace rs_crfast {
using rs_cr::DD;

// rounding-test margin M (relative to the leading double) and the bound on |k| for both fast paths
#define RS_CRFAST_M 0x1p-67
#define RS_CRFAST_KMAX 0x1p20

// c + a for double-doubles with |c.h| >= |a.h|
RS_CR_HD inline DD add_ord(DD c, DD a) {
    const DD s = rs_cr::quick_two_sum(c.h, a.h);
    return rs_cr::quick_two_sum(s.h, s.l + (c.l + a.l));
}
RS_CR_HD inline DD add_ord(double c, DD a) {
    const DD s = rs_cr::quick_two_sum(c, a.h);
    return rs_cr::quick_two_sum(s.h, s.l + a.l);
}

// sin(r) / r as a fast double-double: sin_poly's coefficients, their leading doubles down to z^4
RS_CR_HD inline DD sin_fast(DD r, DD z) {
    double t = -0x1.d1ab1c2dccea3p-94;
    t = fma(t, z.h, 0x1.3f3ccdd165fa9p-84);
    t = fma(t, z.h, -0x1.761b41316381ap-75);
    t = fma(t, z.h, 0x1.71b8ef6dcf572p-66);
    t = fma(t, z.h, -0x1.2f49b46814157p-57);
    t = fma(t, z.h, 0x1.952c77030ad4ap-49);
    t = fma(t, z.h, -0x1.ae7f3e733b81fp-41);
    t = fma(t, z.h, 0x1.6124613a86d09p-33);
    t = fma(t, z.h, -0x1.ae64567f544e4p-26);
    t = fma(t, z.h, 0x1.71de3a556c734p-19);
    DD p = add_ord(DD{-0x1.a01a01a01a01ap-13, -0x1.a01a01a01a01ap-73}, rs_cr::mul(z, t));
    p = add_ord(DD{0x1.1111111111111p-7, 0x1.1111111111111p-63}, rs_cr::mul(p, z));
    p = add_ord(DD{-0x1.5555555555555p-3, -0x1.5555555555555p-57}, rs_cr::mul(p, z));
    p = add_ord(0x1.0000000000000p+0, rs_cr::mul(p, z));
    return rs_cr::mul(r, p);
}
// cos(r) likewise, from cos_poly's coefficients
RS_CR_HD inline DD cos_fast(DD z) {
    double t = 0x1.0a18a2635085dp-98;
    t = fma(t, z.h, -0x1.88e85fc6a4e5ap-89);
    t = fma(t, z.h, 0x1.f2cf01972f578p-80);
    t = fma(t, z.h, -0x1.0ce396db7f853p-70);
    t = fma(t, z.h, 0x1.e542ba4020225p-62);
    t = fma(t, z.h, -0x1.6827863b97d97p-53);
    t = fma(t, z.h, 0x1.ae7f3e733b81fp-45);
    t = fma(t, z.h, -0x1.93974a8c07c9dp-37);
    t = fma(t, z.h, 0x1.1eed8eff8d898p-29);
    t = fma(t, z.h, -0x1.27e4fb7789f5cp-22);
    t = fma(t, z.h, 0x1.a01a01a01a01ap-16);
    DD p = add_ord(DD{-0x1.6c16c16c16c17p-10, 0x1.f49f49f49f49fp-65}, rs_cr::mul(z, t));
    p = add_ord(DD{0x1.5555555555555p-5, 0x1.5555555555555p-59}, rs_cr::mul(p, z));
    p = add_ord(-0x1.0000000000000p-1, rs_cr::mul(p, z));
    p = add_ord(0x1.0000000000000p+0, rs_cr::mul(p, z));
    return p;
}
// the rounding test: no real within M |v.h| of v rounds to another double than v.h
RS_CR_HD inline bool rounds_alone(DD v) {
    const double e = RS_CRFAST_M * fabs(v.h);
    return v.h + (v.l - e) == v.h + (v.l + e);
}
// where the fast series' error bound holds (false for NaN too)
RS_CR_HD inline bool fast_domain(double x, double k) { return fabs(k) < RS_CRFAST_KMAX && fabs(x) >= 0x1p-500; }

// rs_cr::sincos_cr, bit for bit
RS_CR_HD inline void sincos_cr_fast(double x, double* s, double* c) {
    if (!(x == x) || x == INFINITY || x == -INFINITY) { *s = x - x; *c = x - x; return; }
    if (x == 0.0) { *s = x; *c = 1.0; return; }
    int64_t k;
    const DD r = rs_cr::reduce_pio2(x, k);
    const DD z = rs_cr::mul(r, r);
    const DD sf = sin_fast(r, z), cf = cos_fast(z);
    double sr = sf.h, cr = cf.h;
    if (!(fast_domain(x, (double)k) && rounds_alone(sf) && rounds_alone(cf))) {
        sr = rs_cr::sin_poly(r, z).h;
        cr = rs_cr::cos_poly(z).h;
    }
    switch ((int)(k & 3)) {
    case 0: *s = sr; *c = cr; break;
    case 1: *s = cr; *c = -sr; break;
    case 2: *s = -sr; *c = -cr; break;
    default: *s = -cr; *c = sr; break;
    }
}

// rs_cr::sin_sign
RS_CR_HD inline int sin_sign_fast(double x) {
    if (x == 0.0 || !(x == x) || x == INFINITY || x == -INFINITY) return 0;
    const double k = rint(x * 0x1.45f306dc9c883p-1);
    const double t1 = x - k * 0x1.921fb54400000p+0;
    if (!(fabs(k) < RS_CRFAST_KMAX && fabs(t1) > fabs(k) * 0x1p-30)) return rs_cr::sin_sign(x);
    switch ((int)((int64_t)k & 3)) {
    case 0: return t1 > 0.0 ? 1 : -1;
    case 1: return 1;
    case 2: return t1 > 0.0 ? -1 : 1;
    default: return -1;
    }
}
// rs_cr::sin3_negative
RS_CR_HD inline bool sin3_negative_fast(double a, double b, double c) {
    const int p = sin_sign_fast(a) * sin_sign_fast(b) * sin_sign_fast(c);
    return p < 0;
}

// what the kernels call. RS_CRFAST=2 is a dev build for timing only, the ceiling of what the fast paths can recover:
// the platform's sincos and the sign of its plain sin, whose frames are wrong.
RS_CR_HD inline void sincos(double x, double* s, double* c) {
#if RS_CRFAST == 2
    ::sincos(x, s, c);
#elif RS_CRFAST
    sincos_cr_fast(x, s, c);
#else
    rs_cr::sincos_cr(x, s, c);
#endif
}
RS_CR_HD inline bool sin3_negative(double a, double b, double c) {
#if RS_CRFAST == 2
    return ((sin(a) < 0.0) != (sin(b) < 0.0)) != (sin(c) < 0.0);
#elif RS_CRFAST
    return sin3_negative_fast(a, b, c);
#else
    return rs_cr::sin3_negative(a, b, c);
#endif
}
}  // namespace rs_crfast
