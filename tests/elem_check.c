/* TEST INFRASTRUCTURE ONLY.  The specified elementary functions of include/stitch_elem.h held against the correctly rounded
 * value (long double libm, rounded once to float) over the inputs the colour transfer really makes.  Compiled by
 * tests/test_oracle_golden.py and tests/golden/make_transfer_goldens.py into a scratch shared library:
 *   cc -O2 -ffp-contract=off -fopenmp -shared -fPIC -Iinclude tests/elem_check.c -lm */
#include <math.h>
#include <stdint.h>

#include "stitch_elem.h"

/* every l, m, s that transfer::RGBtoLab passes to log() (transfer.cpp:179-189), over all 2^24 colours.
 * out = { inputs, stitch_elem_logf != (float)logl, this platform's logf != (float)logl } */
void elem_check_logf(long long out[3]) {
    long long n = 0, bad = 0, bad_libm = 0;
#pragma omp parallel for schedule(static) reduction(+ : n, bad, bad_libm)
    for (int rgb = 0; rgb < (1 << 24); ++rgb) {
        const double R = (double)(float)(rgb >> 16), G = (double)(float)((rgb >> 8) & 255), B = (double)(float)(rgb & 255);
        float v[3];
        v[0] = (float)(0.3811 * R + 0.5783 * G + 0.0402 * B);
        v[1] = (float)(0.1967 * R + 0.7244 * G + 0.0782 * B);
        v[2] = (float)(0.0241 * R + 0.1288 * G + 0.8444 * B);
        for (int k = 0; k < 3; ++k) {
            const float x = v[k] == 0 ? 1.0f : v[k];
            const float want = (float)logl((long double)x);
            n++;
            if (stitch_elem_logf(x) != want) bad++;
            if (logf(x) != want) bad_libm++;
        }
    }
    out[0] = n;
    out[1] = bad;
    out[2] = bad_libm;
}

/* the given arguments of pow(10, .) (floats, as transfer::LabToRGB has them, transfer.cpp:208-214), result rounded to float
 * as the reference stores it.  out = { inputs, (float)stitch_elem_pow10 != (float)powl, (float)pow of this platform !=
 * (float)powl, NaN inputs (not compared) }; *worst = largest relative distance of stitch_elem_pow10 from powl, in double */
void elem_check_pow10(const float *y, long long count, long long out[4], double *worst) {
    long long n = 0, bad = 0, bad_libm = 0, nan = 0;
    double w = 0;
#pragma omp parallel for schedule(static) reduction(+ : n, bad, bad_libm, nan) reduction(max : w)
    for (long long i = 0; i < count; ++i) {
        if (!(y[i] == y[i])) {
            nan++;
            continue;
        }
        const long double exact = powl(10.0L, (long double)y[i]);
        const double mine = stitch_elem_pow10((double)y[i]);
        const float want = (float)exact;
        n++;
        if ((float)mine != want) bad++;
        if ((float)pow(10.0, (double)y[i]) != want) bad_libm++;
        if (exact > 0 && isfinite((double)exact)) {
            const double rel = (double)fabsl(((long double)mine - exact) / exact);
            if (rel > w) w = rel;
        }
    }
    out[0] = n;
    out[1] = bad;
    out[2] = bad_libm;
    out[3] = nan;
    *worst = w;
}
