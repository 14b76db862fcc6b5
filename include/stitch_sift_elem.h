/* Specified elementary functions for the SIFT extraction (vl/sift.c): exp, 2^x, and sin / cos on [0, 2 pi].
 *
 * VLFeat calls the platform's libm in four places whose value reaches a result: exp() for the Gaussian filter taps
 * (sift.c:135) and for the fast_expn table (:61), pow(2.0, sn / S) in a keypoint's sigma (:767), and sin / cos of the
 * descriptor's angle (:1306-1307).  The table entries and the sine / cosine are used as doubles, so the functions here
 * aim at the CORRECTLY ROUNDED double: every step is carried in double-double arithmetic (Dekker / Knuth error-free
 * sums and products, plain IEEE-754 +,-,*,/ in a fixed order, no FMA -- both sides are compiled with
 * -ffp-contract=off) and rounded once at the end; tests/test_sift_elem.py checks the results against 60-digit values.  A
 * libm that is correctly rounded on an argument agrees bit for bit; where one is not, it differs by one ulp.
 * The same text compiles for the host and for the device.
 */
#ifndef STITCH_SIFT_ELEM_H
#define STITCH_SIFT_ELEM_H
#include "stitch_elem.h"

typedef struct stitch_dd {
    double hi, lo;
} stitch_dd;

STITCH_HD stitch_dd stitch_dd_make(double hi, double lo) {
    stitch_dd r;
    r.hi = hi;
    r.lo = lo;
    return r;
}
/* a + b = hi + lo exactly (Knuth) */
STITCH_HD stitch_dd stitch_dd_two_sum(double a, double b) {
    const double s = a + b, bb = s - a;
    return stitch_dd_make(s, (a - (s - bb)) + (b - bb));
}
/* |a| >= |b| */
STITCH_HD stitch_dd stitch_dd_fast_two_sum(double a, double b) {
    const double s = a + b;
    return stitch_dd_make(s, b - (s - a));
}
/* a * b = hi + lo exactly (Dekker splitting; |a|, |b| far below 2^996) */
STITCH_HD stitch_dd stitch_dd_two_prod(double a, double b) {
    const double SPLIT = 134217729.0; /* 2^27 + 1 */
    double c = SPLIT * a;
    const double ah = c - (c - a), al = a - ah;
    c = SPLIT * b;
    const double bh = c - (c - b), bl = b - bh;
    const double p = a * b;
    return stitch_dd_make(p, ((ah * bh - p) + ah * bl + al * bh) + al * bl);
}
STITCH_HD stitch_dd stitch_dd_add(stitch_dd a, stitch_dd b) {
    stitch_dd s = stitch_dd_two_sum(a.hi, b.hi);
    const stitch_dd t = stitch_dd_two_sum(a.lo, b.lo);
    s.lo = s.lo + t.hi;
    s = stitch_dd_fast_two_sum(s.hi, s.lo);
    s.lo = s.lo + t.lo;
    return stitch_dd_fast_two_sum(s.hi, s.lo);
}
STITCH_HD stitch_dd stitch_dd_mul(stitch_dd a, stitch_dd b) {
    stitch_dd p = stitch_dd_two_prod(a.hi, b.hi);
    p.lo = p.lo + (a.hi * b.lo + a.lo * b.hi);
    return stitch_dd_fast_two_sum(p.hi, p.lo);
}
STITCH_HD stitch_dd stitch_dd_mul_d(stitch_dd a, double b) {
    stitch_dd p = stitch_dd_two_prod(a.hi, b);
    p.lo = p.lo + a.lo * b;
    return stitch_dd_fast_two_sum(p.hi, p.lo);
}
/* a / b for a small integer-valued b */
STITCH_HD stitch_dd stitch_dd_div_d(stitch_dd a, double b) {
    const double q1 = a.hi / b;
    const stitch_dd p = stitch_dd_two_prod(q1, b);
    const double r = ((a.hi - p.hi) - p.lo) + a.lo;
    return stitch_dd_fast_two_sum(q1, r / b);
}

/* ln 2 and pi / 2 as double-doubles */
#define STITCH_DD_LN2_HI 6.931471805599452862e-01
#define STITCH_DD_LN2_LO 2.319046813846299558e-17
#define STITCH_DD_PIO2_HI 1.570796326794896558e+00
#define STITCH_DD_PIO2_LO 6.123233995736766036e-17

/* e^r for a double-double |r| <= 0.36: Taylor by Horner from degree 30, q_k = 1 + (r / k) q_{k+1} */
STITCH_HD stitch_dd stitch_dd_exp_small(stitch_dd r) {
    stitch_dd q = stitch_dd_make(1.0, 0.0);
    for (int k = 30; k >= 1; --k) q = stitch_dd_add(stitch_dd_make(1.0, 0.0), stitch_dd_mul(stitch_dd_div_d(r, (double)k), q));
    return q;
}
STITCH_HD double stitch_sift_scale2(double v, long long n) { /* v * 2^n, |n| < 1000, no subnormal results wanted */
    return v * stitch_elem_bits_to_double((uint64_t)(1023 + n) << 52);
}
/* e^x, |x| < 700 */
STITCH_HD double stitch_sift_exp(double x) {
    if (!(x == x)) return x;
    if (x > 700.0) return stitch_elem_bits_to_double(0x7ff0000000000000ULL);
    if (x < -700.0) return 0.0;
    const double t = x * 1.4426950408889634;
    const double nd = (double)(long long)(t + (t < 0 ? -0.5 : 0.5));
    /* r = x - n ln 2 in double-double */
    const stitch_dd nl = stitch_dd_mul_d(stitch_dd_make(STITCH_DD_LN2_HI, STITCH_DD_LN2_LO), nd);
    const stitch_dd r = stitch_dd_add(stitch_dd_make(x, 0.0), stitch_dd_make(-nl.hi, -nl.lo));
    const stitch_dd q = stitch_dd_exp_small(r);
    return stitch_sift_scale2(q.hi + q.lo, (long long)nd);
}
/* 2^y (stands for pow(2.0, y)), |y| < 1000 */
STITCH_HD double stitch_sift_exp2(double y) {
    if (!(y == y)) return y;
    if (y > 1000.0) return stitch_elem_bits_to_double(0x7ff0000000000000ULL);
    if (y < -1000.0) return 0.0;
    const double nd = (double)(long long)(y + (y < 0 ? -0.5 : 0.5));
    const double f = y - nd; /* exact */
    const stitch_dd r = stitch_dd_mul_d(stitch_dd_make(STITCH_DD_LN2_HI, STITCH_DD_LN2_LO), f);
    const stitch_dd q = stitch_dd_exp_small(r);
    return stitch_sift_scale2(q.hi + q.lo, (long long)nd);
}
/* sin and cos of a in [-1, 8] (the angles of vl_sift_calc_keypoint_orientations lie in [0, 2 pi]):
 * a = k pi/2 + r, |r| <= pi/4 + tiny, Taylor series of sin r and cos r in double-double, quadrant by k. */
STITCH_HD void stitch_sift_sincos(double a, double* s_out, double* c_out) {
    if (!(a >= -1.0 && a <= 8.0)) { /* outside the specified range: not a number */
        *s_out = *c_out = stitch_elem_bits_to_double(0x7ff8000000000000ULL);
        return;
    }
    const double t = a * 0.63661977236758138;
    const double kd = (double)(long long)(t + (t < 0 ? -0.5 : 0.5));
    const stitch_dd kp = stitch_dd_mul_d(stitch_dd_make(STITCH_DD_PIO2_HI, STITCH_DD_PIO2_LO), kd);
    const stitch_dd r = stitch_dd_add(stitch_dd_make(a, 0.0), stitch_dd_make(-kp.hi, -kp.lo));
    const stitch_dd z = stitch_dd_mul(r, r);
    const stitch_dd mz = stitch_dd_make(-z.hi, -z.lo);
    const stitch_dd one = stitch_dd_make(1.0, 0.0);
    /* sin r = r (1 - z/(2*3) (1 - z/(4*5) (...))), cos r = 1 - z/(1*2) (1 - z/(3*4) (...)) */
    stitch_dd ps = one, pc = one;
    for (int k = 14; k >= 1; --k) {
        ps = stitch_dd_add(one, stitch_dd_mul(stitch_dd_div_d(mz, (double)((2 * k) * (2 * k + 1))), ps));
        pc = stitch_dd_add(one, stitch_dd_mul(stitch_dd_div_d(mz, (double)((2 * k - 1) * (2 * k))), pc));
    }
    ps = stitch_dd_mul(r, ps);
    const double sr = ps.hi + ps.lo, cr = pc.hi + pc.lo;
    const int q = (int)((long long)kd & 3);
    *s_out = q == 0 ? sr : q == 1 ? cr : q == 2 ? -sr : -cr;
    *c_out = q == 0 ? cr : q == 1 ? -sr : q == 2 ? -cr : sr;
}

#endif
