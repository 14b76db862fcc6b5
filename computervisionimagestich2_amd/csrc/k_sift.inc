// k_sift.inc -- SIFT extraction (include/stitch.h, "SIFT"): VLFeat's vl/sift.c as ImageProcess::siftAlgorithm drives it
// (ImageProcess.cpp:44-99), restated bit for bit.  Host side in stitch_sift.inc; tests/sift_emulate.cpp compiles the
// sift_* functions of this file for the CPU.
//
// Everything a result depends on is a sift_* function that handles ONE sample (one filter output, one DoG position, one
// candidate, one gradient pixel, one histogram term): C float / double arithmetic in the reference's order and promotions, no
// FMA (-ffp-contract=off), VLFeat's own inline approximations restated, and the three libm values replaced by
// stitch_sift_elem.h.  The kernels only decide which lane runs which sample and in which order sums are formed:
//   k_sift_table      fast_expn's 257-entry table (sift.c:56-63), once per call
//   k_sift_load       u8 / f32 gray -> level s_min of octave 0 (the memcpy of sift.c:381)
//   k_sift_down       copy_and_downsample (sift.c:178-194, :458) from level min(s_min + S, s_max) of the previous octave
//   k_sift_conv       one column pass of vl_imconvcol_vf with transpose (imopv.c:118-201); two per smoothed level
//   k_sift_detect     DoG on the fly, the 26-neighbour test (sift.c:539-603) and the refinement (:612-772) of each candidate in
//                     place; one ballot word per wavefront says which positions are keypoints
//   k_sift_scan       exclusive scan of the ballot counts: keypoint index = position in the reference's scan order (s, y, x)
//   k_sift_emit       the keypoint records (a second refinement of the survivors only) at their scanned index
//   k_sift_grad       update_gradient (sift.c:791-876) for levels s_min+1 .. s_max-2, skipped when the octave has no keypoint
//   k_sift_orient     vl_sift_calc_keypoint_orientations (:903-1037), one wavefront per keypoint
//   k_sift_fscan      scan of the angle counts: feature row = octave, keypoint, angle -- the reference's insertion order
//   k_sift_desc       vl_sift_calc_keypoint_descriptor (:1267-1438), one wavefront per keypoint
//   k_sift_finish     counts and status
// Histogram sums keep the reference's order of terms without atomics: the 64 lanes form the terms of 64 consecutive pixels (ys
// outer, xs inner) into LDS, then the lane that owns a bin walks the 64 entries in order and adds those aimed at its bin.
#include "stitch_sift_elem.h"

constexpr int SIFT_MAXFRAMES = 16;
constexpr int SIFT_MAXHALF = 64;  // largest filter half-width (levels = 1 needs 45)
constexpr int SIFT_CONV_TX = 16;  // tile of k_sift_conv: 16 source columns x 64 source rows
constexpr int SIFT_CONV_TY = 64;
constexpr int SIFT_T = 256;
constexpr int SIFT_SCAN_T = 1024;
constexpr int SIFT_NBINS = 36;
constexpr int SIFT_DESC = 128;  // NBP * NBP * NBO = 4 * 4 * 8
enum { SIFT_H_KP_TOTAL = 0, SIFT_H_OCT_START, SIFT_H_OCT_N, SIFT_H_FEAT_TOTAL, SIFT_H_OCTAVES, SIFT_H_N = 8 };

struct SiftKeypoint {  // VlSiftKeypoint, vl/sift.h:19-31
    int32_t o, ix, iy, is;
    float x, y, s, sigma;
};

struct SiftFrame {
    const void* img;
    int w, h, pitch, is_f32;  // pitch in bytes
    float* oct;               // S + 3 Gaussian levels, each `lstride` floats apart (the size of octave 0)
    float* tmp;
    float* grad;  // S levels of interleaved (modulus, angle), each 2 * lstride floats apart
    size_t lstride;
    unsigned long long* mask;  // one ballot word per 64 positions of the octave
    int32_t* woff;             // keypoint index of each word's first keypoint
    int32_t* hdr;              // SIFT_H_*
    int32_t* nang;             // per keypoint: number of angles, first feature row
    int32_t* foff;
    double* ang;  // 4 per keypoint
    SiftKeypoint* kp;
    int32_t* f_kp;
    double* f_angle;
    float* f_desc;
    int32_t* counts;
    int32_t* status;
    int kp_cap, feat_cap;
};

struct SiftArgs {
    SiftFrame f[SIFT_MAXFRAMES];
    const double* expn;  // fast_expn's table
    int S, o;            // levels, current octave
    int src_lvl, dst_lvl, pass;  // k_sift_conv / k_sift_down
    double tp, te_bound, norm_thresh, magnif, sigma0;
    float wsigma;
};

struct SiftTaps {
    float c[2 * SIFT_MAXHALF + 1];
    int W;
};

// ---- VLFeat's inline helpers (vl/mathop.h) ---------------------------------------------------------------------------------
#define SIFT_PI 3.141592653589793 /* VL_PI */
#define SIFT_EPS_F 1.19209290E-07F
#define SIFT_EPS_D 2.220446049250313e-16

__host__ __device__ __forceinline__ float sift_mod_2pi_f(float x) {  // mathop.h:109-115
    while (x > (float)(2 * SIFT_PI)) x -= (float)(2 * SIFT_PI);
    while (x < 0.0F) x += (float)(2 * SIFT_PI);
    return x;
}
__host__ __device__ __forceinline__ long sift_floor_f(float x) {  // :134-140
    const long xi = (long)x;
    return (x >= 0 || (float)xi == x) ? xi : xi - 1;
}
__host__ __device__ __forceinline__ long sift_floor_d(double x) {  // :146-152
    const long xi = (long)x;
    return (x >= 0 || (double)xi == x) ? xi : xi - 1;
}
__host__ __device__ __forceinline__ float sift_abs_f(float x) { return x < 0 ? -x : (x == 0 ? 0.0f : x); }  // fabsf (-0 -> +0)
__host__ __device__ __forceinline__ double sift_abs_d(double x) { return x < 0 ? -x : (x == 0 ? 0.0 : x); }
__host__ __device__ __forceinline__ float sift_fast_atan2_f(float y, float x) {  // :407-424
    float angle, r;
    const float c3 = 0.1821F, c1 = 0.9675F;
    const float abs_y = sift_abs_f(y) + SIFT_EPS_F;
    if (x >= 0) {
        r = (x - abs_y) / (x + abs_y);
        angle = (float)(SIFT_PI / 4);
    } else {
        r = (x + abs_y) / (abs_y - x);
        angle = (float)(3 * SIFT_PI / 4);
    }
    angle += (c3 * r * r - c1) * r;
    return (y < 0) ? -angle : angle;
}
__host__ __device__ __forceinline__ float sift_fast_resqrt_f(float x) {  // :479-501
    const float xhalf = (float)0.5 * x;
    int32_t i;
    memcpy(&i, &x, 4);
    i = 0x5f3759df - (i >> 1);
    float u;
    memcpy(&u, &i, 4);
    u = u * ((float)1.5 - xhalf * u * u);
    u = u * ((float)1.5 - xhalf * u * u);
    return u;
}
__host__ __device__ __forceinline__ float sift_fast_sqrt_f(float x) { return ((double)x < 1e-8) ? 0 : x * sift_fast_resqrt_f(x); }  // :544-548
__host__ __device__ __forceinline__ double sift_fast_expn(const double* tab, double x) {  // sift.c:34-49
    if (x > 25.0) return 0.0;
    x *= 256 / 25.0;
    const int i = (int)sift_floor_d(x);
    const double r = x - i;
    const double a = tab[i], b = tab[i + 1];
    return a + r * (b - a);
}
__host__ __device__ __forceinline__ double sift_expn_entry(int k) { return stitch_sift_exp(-(double)k * (25.0 / 256)); }  // sift.c:61

// ---- smoothing ---------------------------------------------------------------------------------------------------------------
// The filter of _vl_sift_smooth (sift.c:125-141): returns the half-width, or -1 when it exceeds SIFT_MAXHALF.
__host__ __device__ inline int sift_make_taps(double sigma, float* taps) {
    double cw = 4.0 * sigma;
    long W = (long)cw;
    if ((double)W < cw) ++W;  // ceil
    if (W < 1) W = 1;
    if (W > SIFT_MAXHALF) return -1;
    float acc = 0;
    for (long j = 0; j < 2 * W + 1; ++j) {
        const float d = ((float)((int)j - (int)W)) / ((float)sigma);
        taps[j] = (float)stitch_sift_exp(-0.5 * (d * d));
        acc += taps[j];
    }
    for (long j = 0; j < 2 * W + 1; ++j) taps[j] /= acc;
    return (int)W;
}
// The smoothing schedule of an octave (sift.c:251-254, :390-406, :465-481), host only: sd[0] is the adjustment of level s_min
// (0: none), sd[1 + k] the step from level k to level k + 1 (S + 2 of them).  sqrt and pow here are the host's: sqrt is exact
// and the fixtures pin the resulting filters.
struct SiftPlan {
    double sigma0, sd_first[8], sd_next[8];
};
inline SiftPlan sift_plan(int S) {
    SiftPlan p;
    const int s_min = -1, s_max = S + 1;
    const double sigman = 0.5, sigmak = std::pow(2.0, 1.0 / S);
    p.sigma0 = 1.6 * sigmak;
    const double dsigma0 = p.sigma0 * std::sqrt(1.0 - 1.0 / (sigmak * sigmak));
    double sa = p.sigma0 * std::pow(sigmak, s_min), sb = sigman * std::pow(2.0, -0);
    p.sd_first[0] = sa > sb ? std::sqrt(sa * sa - sb * sb) : 0.0;
    const int s_best = std::min(s_min + S, s_max);
    sa = p.sigma0 * powf(sigmak, s_min);
    sb = p.sigma0 * powf(sigmak, s_best - S);
    p.sd_next[0] = sa > sb ? std::sqrt(sa * sa - sb * sb) : 0.0;
    for (int s = s_min + 1; s <= s_max; ++s) p.sd_first[s - s_min] = p.sd_next[s - s_min] = dsigma0 * std::pow(sigmak, s);
    return p;
}
// noctaves < 0 (sift.c:229-231, o_min = 0): max(floor(log2(min(w, h))) - 3, 1)
inline int sift_auto_octaves(int w, int h) {
    int m = std::min(w, h), l = 0;
    while (m > 1) {
        m >>= 1;
        ++l;
    }
    return std::max(l - 3, 1);
}
// One output of vl_imconvcol_vf (imopv.c:150-186): col[k * stride], k = 0 .. 2W, are the source samples of rows y-W .. y+W
// already clamped to the image; the reference walks the filter from its last tap down.
__host__ __device__ __forceinline__ float sift_conv_sample(const float* col, int stride, const float* taps, int W) {
    float acc = 0;
    for (int k = 0; k <= 2 * W; ++k) {
        const float v = col[k * stride], c = taps[2 * W - k];
        acc += v * c;
    }
    return acc;
}

// ---- detection ---------------------------------------------------------------------------------------------------------------
// DoG level d (0 .. S+1) = Gaussian level d+1 minus level d (sift.c:523-530); g points at Gaussian level 0 of the octave.
__host__ __device__ __forceinline__ float sift_dog(const float* g, size_t ls, int w, int x, int y, int d) {
    const size_t i = (size_t)d * ls + (size_t)y * w + x;
    return g[i + ls] - g[i];
}
// sift.c:544-577 at DoG level d, 1 <= x <= w-2, 1 <= y <= h-2
__host__ __device__ __forceinline__ bool sift_is_extremum(const float* g, size_t ls, int w, int x, int y, int d, double tp) {
    const float v = sift_dog(g, ls, w, x, y, d);
    const bool up = (double)v >= 0.8 * tp, dn = (double)v <= -0.8 * tp;
    if (!up && !dn) return false;
    bool gt = up, lt = dn;
    for (int ds = -1; ds <= 1; ++ds)
        for (int dy = -1; dy <= 1; ++dy)
            for (int dx = -1; dx <= 1; ++dx) {
                if (!(ds | dy | dx)) continue;
                const float n = sift_dog(g, ls, w, x + dx, y + dy, d + ds);
                gt = gt && v > n;
                lt = lt && v < n;
                if (!gt && !lt) return false;  // (most positions leave within a few neighbours)
            }
    return gt || lt;
}
// sift.c:612-772 for the candidate (x, y, s); s = d - 1 is the level index with s_min = -1.  2^(sn/S) is stitch_sift_exp2.
__host__ __device__ __forceinline__ bool sift_refine(const float* g, size_t ls, int w, int h, int x, int y, int s, int S, int o, double tp,
                                            double te_bound, double sigma0, SiftKeypoint* out) {
    const int s_min = -1, s_max = S + 1, d = s - s_min;
    double Dx = 0, Dy = 0, Ds = 0, Dxx = 0, Dyy = 0, Dss = 0, Dxy = 0, Dxs = 0, Dys = 0;
    double A[9], b[3];
    int dx = 0, dy = 0;
#define SIFT_AT(ddx, ddy, dds) sift_dog(g, ls, w, x + (ddx), y + (ddy), d + (dds))
#define SIFT_A(i, j) A[(i) + (j) * 3]
    for (int iter = 0; iter < 5; ++iter) {
        x += dx;
        y += dy;
        Dx = 0.5 * (SIFT_AT(+1, 0, 0) - SIFT_AT(-1, 0, 0));
        Dy = 0.5 * (SIFT_AT(0, +1, 0) - SIFT_AT(0, -1, 0));
        Ds = 0.5 * (SIFT_AT(0, 0, +1) - SIFT_AT(0, 0, -1));
        Dxx = (SIFT_AT(+1, 0, 0) + SIFT_AT(-1, 0, 0) - 2.0 * SIFT_AT(0, 0, 0));
        Dyy = (SIFT_AT(0, +1, 0) + SIFT_AT(0, -1, 0) - 2.0 * SIFT_AT(0, 0, 0));
        Dss = (SIFT_AT(0, 0, +1) + SIFT_AT(0, 0, -1) - 2.0 * SIFT_AT(0, 0, 0));
        Dxy = 0.25 * (SIFT_AT(+1, +1, 0) + SIFT_AT(-1, -1, 0) - SIFT_AT(-1, +1, 0) - SIFT_AT(+1, -1, 0));
        Dxs = 0.25 * (SIFT_AT(+1, 0, +1) + SIFT_AT(-1, 0, -1) - SIFT_AT(-1, 0, +1) - SIFT_AT(+1, 0, -1));
        Dys = 0.25 * (SIFT_AT(0, +1, +1) + SIFT_AT(0, -1, -1) - SIFT_AT(0, -1, +1) - SIFT_AT(0, +1, -1));
        SIFT_A(0, 0) = Dxx;
        SIFT_A(1, 1) = Dyy;
        SIFT_A(2, 2) = Dss;
        SIFT_A(0, 1) = SIFT_A(1, 0) = Dxy;
        SIFT_A(0, 2) = SIFT_A(2, 0) = Dxs;
        SIFT_A(1, 2) = SIFT_A(2, 1) = Dys;
        b[0] = -Dx;
        b[1] = -Dy;
        b[2] = -Ds;
        for (int j = 0; j < 3; ++j) {  // Gauss elimination, :669-712
            double maxa = 0, maxabsa = 0, tmp;
            int maxi = -1;
            for (int i = j; i < 3; ++i) {
                const double a = SIFT_A(i, j), absa = sift_abs_d(a);
                if (absa > maxabsa) {
                    maxa = a;
                    maxabsa = absa;
                    maxi = i;
                }
            }
            if (maxabsa < 1e-10f) {
                b[0] = 0;
                b[1] = 0;
                b[2] = 0;
                break;
            }
            const int i = maxi;
            for (int jj = j; jj < 3; ++jj) {
                tmp = SIFT_A(i, jj);
                SIFT_A(i, jj) = SIFT_A(j, jj);
                SIFT_A(j, jj) = tmp;
                SIFT_A(j, jj) /= maxa;
            }
            tmp = b[j];
            b[j] = b[i];
            b[i] = tmp;
            b[j] /= maxa;
            for (int ii = j + 1; ii < 3; ++ii) {
                const double xx = SIFT_A(ii, j);
                for (int jj = j; jj < 3; ++jj) SIFT_A(ii, jj) -= xx * SIFT_A(j, jj);
                b[ii] -= xx * b[j];
            }
        }
        for (int i = 2; i > 0; --i) {  // backward substitution
            const double xx = b[i];
            for (int ii = i - 1; ii >= 0; --ii) b[ii] -= xx * SIFT_A(ii, i);
        }
        dx = ((b[0] > 0.6 && x < w - 2) ? 1 : 0) + ((b[0] < -0.6 && x > 1) ? -1 : 0);
        dy = ((b[1] > 0.6 && y < h - 2) ? 1 : 0) + ((b[1] < -0.6 && y > 1) ? -1 : 0);
        if (dx == 0 && dy == 0) break;
    }
    const double val = SIFT_AT(0, 0, 0) + 0.5 * (Dx * b[0] + Dy * b[1] + Ds * b[2]);
    const double score = (Dxx + Dyy) * (Dxx + Dyy) / (Dxx * Dyy - Dxy * Dxy);
    const double xn = x + b[0], yn = y + b[1], sn = s + b[2];
#undef SIFT_AT
#undef SIFT_A
    const bool good = sift_abs_d(val) > tp && score < te_bound && score >= 0 && sift_abs_d(b[0]) < 1.5 && sift_abs_d(b[1]) < 1.5 &&
                      sift_abs_d(b[2]) < 1.5 && xn >= 0 && xn <= w - 1 && yn >= 0 && yn <= h - 1 && sn >= s_min && sn <= s_max;
    if (good && out) {
        const double xper = stitch_sift_scale2(1.0, o);
        out->o = o;
        out->ix = x;
        out->iy = y;
        out->is = s;
        out->s = (float)sn;
        out->x = (float)(xn * xper);
        out->y = (float)(yn * xper);
        out->sigma = (float)(sigma0 * stitch_sift_exp2(sn / S) * xper);
    }
    return good;
}

// ---- gradient (sift.c:805-874): modulus and angle of pixel (x, y) of Gaussian level plane `src` (w, h >= 2) ------------------
__host__ __device__ __forceinline__ void sift_grad_pixel(const float* src, int w, int h, int x, int y, float* mod, float* ang) {
    const float* p = src + (size_t)y * w + x;
    float gx, gy;
    if (x == 0)
        gx = p[1] - p[0];
    else if (x == w - 1)
        gx = p[0] - p[-1];
    else
        gx = (float)(0.5 * (p[1] - p[-1]));
    if (y == 0)
        gy = p[w] - p[0];
    else if (y == h - 1)
        gy = p[0] - p[-w];
    else
        gy = (float)(0.5 * (p[w] - p[-w]));
    *mod = sift_fast_sqrt_f(gx * gx + gy * gy);
    *ang = sift_mod_2pi_f((float)(sift_fast_atan2_f(gy, gx) + 2 * SIFT_PI));
}

// ---- orientations ------------------------------------------------------------------------------------------------------------
struct SiftGeom {  // the shared prologue of sift.c:916-925 and :1298-1310
    double x, y, sigma;
    int xi, yi, si;
};
__host__ __device__ __forceinline__ SiftGeom sift_geom(const SiftKeypoint& k, int o) {
    const double xper = stitch_sift_scale2(1.0, o);
    SiftGeom q;
    q.x = k.x / xper;
    q.y = k.y / xper;
    q.sigma = k.sigma / xper;
    q.xi = (int)(q.x + 0.5);
    q.yi = (int)(q.y + 0.5);
    q.si = k.is;
    return q;
}
__host__ __device__ __forceinline__ int sift_orient_window(const SiftGeom& q) {  // W of :925
    const double t = 3.0 * (1.5 * q.sigma);
    const double fl = (double)sift_floor_d(t);
    return (int)(fl > 1 ? fl : 1);
}
// The term of pixel (xi + xs, yi + ys) (:968-987): bins b0, b1 and what is added to each; false when outside the window.
__host__ __device__ __forceinline__ bool sift_orient_term(const SiftGeom& q, int W, int xs, int ys, float fmod, float fang, const double* tab,
                                                 int* b0, double* v0, int* b1, double* v1) {
    const double sigmaw = 1.5 * q.sigma;
    const double dx = (double)(q.xi + xs) - q.x, dy = (double)(q.yi + ys) - q.y;
    const double r2 = dx * dx + dy * dy;
    if (r2 >= W * W + 0.6) return false;
    const double wgt = sift_fast_expn(tab, r2 / (2 * sigmaw * sigmaw));
    const double mod = fmod, ang = fang;
    const double fbin = SIFT_NBINS * ang / (2 * SIFT_PI);
    const int bin = (int)sift_floor_d(fbin - 0.5);
    const double rbin = fbin - bin - 0.5;
    *b0 = (bin + SIFT_NBINS) % SIFT_NBINS;
    *v0 = (1 - rbin) * mod * wgt;
    *b1 = (bin + 1) % SIFT_NBINS;
    *v1 = (rbin)*mod * wgt;
    return true;
}
// :999-1036 on the finished histogram: smoothing, maximum, peaks; returns the number of angles
__host__ __device__ __forceinline__ int sift_orient_finish(double* hist, double* angles) {
    for (int iter = 0; iter < 6; iter++) {
        double prev = hist[SIFT_NBINS - 1];
        const double first = hist[0];
        int i;
        for (i = 0; i < SIFT_NBINS - 1; i++) {
            const double newh = (prev + hist[i] + hist[(i + 1) % SIFT_NBINS]) / 3.0;
            prev = hist[i];
            hist[i] = newh;
        }
        hist[i] = (prev + hist[i] + first) / 3.0;
    }
    double maxh = 0;
    for (int i = 0; i < SIFT_NBINS; ++i) maxh = maxh > hist[i] ? maxh : hist[i];  // VL_MAX(maxh, hist[i])
    int n = 0;
    for (int i = 0; i < SIFT_NBINS; ++i) {
        const double h0 = hist[i], hm = hist[(i - 1 + SIFT_NBINS) % SIFT_NBINS], hp = hist[(i + 1 + SIFT_NBINS) % SIFT_NBINS];
        if (h0 > 0.8 * maxh && h0 > hm && h0 > hp) {
            const double di = -0.5 * (hp - hm) / (hp + hm - 2 * h0);
            angles[n++] = 2 * SIFT_PI * (i + di + 0.5) / SIFT_NBINS;
            if (n == 4) break;
        }
    }
    return n;
}
// the bounds test of :940-947 (w, h of the octave)
__host__ __device__ __forceinline__ bool sift_orient_inside(const SiftGeom& q, int w, int h, int S) {
    return !(q.xi < 0 || q.xi > w - 1 || q.yi < 0 || q.yi > h - 1 || q.si < 0 || q.si > S - 1);
}

// ---- descriptor --------------------------------------------------------------------------------------------------------------
struct SiftDescFrame {  // per (keypoint, angle): sift.c:1306-1310
    double st0, ct0, SBP, angle0;
    int W;
};
__host__ __device__ __forceinline__ SiftDescFrame sift_desc_frame(const SiftGeom& q, double angle0, double magnif) {
    SiftDescFrame d;
    stitch_sift_sincos(angle0, &d.st0, &d.ct0);
    d.angle0 = angle0;
    d.SBP = magnif * q.sigma + SIFT_EPS_D;
    d.W = (int)sift_floor_d(1.4142135623730951 * d.SBP * (4 + 1) / 2.0 + 0.5);
    return d;
}
__host__ __device__ __forceinline__ bool sift_desc_inside(const SiftGeom& q, int w, int h, int S) {  // :1321-1328
    return !(q.xi < 0 || q.xi >= w || q.yi < 0 || q.yi >= h - 1 || q.si < 0 || q.si > S - 1);
}
struct SiftDescTerm {  // :1358-1387
    float wm, rbinx, rbiny, rbint;  // win and mod (multiplied first, as `win * mod * ...` is), the three remainders
    int binx, biny, bint;
};
__host__ __device__ __forceinline__ SiftDescTerm sift_desc_term(const SiftGeom& q, const SiftDescFrame& d, int dxi, int dyi, float mod,
                                                       float angle, float wsigma, const double* tab) {
    const float theta = sift_mod_2pi_f((float)(angle - d.angle0));
    const float dx = (float)(q.xi + dxi - q.x), dy = (float)(q.yi + dyi - q.y);
    const float nx = (float)((d.ct0 * dx + d.st0 * dy) / d.SBP);
    const float ny = (float)((-d.st0 * dx + d.ct0 * dy) / d.SBP);
    const float nt = (float)(8 * theta / (2 * SIFT_PI));
    const float win = (float)sift_fast_expn(tab, (nx * nx + ny * ny) / (2.0 * wsigma * wsigma));
    SiftDescTerm t;
    t.binx = (int)sift_floor_f((float)(nx - 0.5));
    t.biny = (int)sift_floor_f((float)(ny - 0.5));
    t.bint = (int)sift_floor_f(nt);
    t.rbinx = (float)(nx - (t.binx + 0.5));
    t.rbiny = (float)(ny - (t.biny + 0.5));
    t.rbint = nt - t.bint;
    t.wm = win * mod;
    return t;
}
// What the term adds to descriptor bin `bin` = (by + 2) * 32 + (bx + 2) * 8 + bt (:1393-1411); false when it adds nothing.
__host__ __device__ __forceinline__ bool sift_desc_weight(const SiftDescTerm& t, int bin, float* weight) {
    const int bt = bin & 7, bx = ((bin >> 3) & 3) - 2, by = (bin >> 5) - 2;
    const int dbinx = bx - t.binx, dbiny = by - t.biny, dbint = (bt - t.bint) & 7;
    if ((unsigned)dbinx > 1u || (unsigned)dbiny > 1u || dbint > 1) return false;
    *weight = t.wm * sift_abs_f(1 - dbinx - t.rbinx) * sift_abs_f(1 - dbiny - t.rbiny) * sift_abs_f(1 - dbint - t.rbint);
    return true;
}
// :1047-1063 and :1416-1436 on the 128 sums
__host__ __device__ __forceinline__ float sift_desc_normalize(float* d) {
    float norm = 0.0f;
    for (int i = 0; i < SIFT_DESC; ++i) norm += d[i] * d[i];
    norm = sift_fast_sqrt_f(norm) + SIFT_EPS_F;
    for (int i = 0; i < SIFT_DESC; ++i) d[i] /= norm;
    return norm;
}
__host__ __device__ __forceinline__ void sift_desc_finish(float* d, double norm_thresh) {
    const float norm = sift_desc_normalize(d);
    if (norm_thresh != 0 && norm < norm_thresh) {
        for (int i = 0; i < SIFT_DESC; ++i) d[i] = 0;
    } else {
        for (int i = 0; i < SIFT_DESC; ++i)
            if (d[i] > 0.2) d[i] = 0.2;
        sift_desc_normalize(d);
    }
}

#ifndef SIFT_HOST_EMULATION
// ================================================================ kernels ====================================================
__host__ __device__ __forceinline__ int sift_ow(const SiftFrame& f, int o) { return f.w >> o; }
__host__ __device__ __forceinline__ int sift_oh(const SiftFrame& f, int o) { return f.h >> o; }

__global__ void __launch_bounds__(320) k_sift_table(double* tab) {
    const int k = threadIdx.x;
    if (k < 257) tab[k] = sift_expn_entry(k);
    if (k == 257) tab[k] = 0;  // fast_expn(25) reads one entry past the table (times r = 0); the reference reads its neighbour in memory
}

__global__ void __launch_bounds__(SIFT_T) k_sift_load(SiftArgs a) {
    const SiftFrame& f = a.f[blockIdx.z];
    const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x < SIFT_H_N) f.hdr[threadIdx.x] = 0;
    if (x >= f.w || y >= f.h) return;
    const char* row = static_cast<const char*>(f.img) + (size_t)y * f.pitch;
    f.oct[(size_t)y * f.w + x] = f.is_f32 ? reinterpret_cast<const float*>(row)[x] : (float)reinterpret_cast<const unsigned char*>(row)[x];
}

// a.o is the NEW octave; the source is level a.src_lvl of octave a.o - 1
__global__ void __launch_bounds__(SIFT_T) k_sift_down(SiftArgs a) {
    const SiftFrame& f = a.f[blockIdx.z];
    const int w = sift_ow(f, a.o), h = sift_oh(f, a.o), sw = sift_ow(f, a.o - 1);
    const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (x >= w || y >= h) return;
    f.oct[(size_t)y * w + x] = f.oct[(size_t)a.src_lvl * f.lstride + (size_t)(2 * y) * sw + 2 * x];
}

// pass 0: level src_lvl (w x h) -> tmp, transposed (h x w); pass 1: tmp (h x w) -> level dst_lvl (w x h)
__global__ void __launch_bounds__(SIFT_T) k_sift_conv(SiftArgs a, SiftTaps t) {
    __shared__ float tile[(SIFT_CONV_TY + 2 * SIFT_MAXHALF) * (SIFT_CONV_TX + 1)];
    const SiftFrame& f = a.f[blockIdx.z];
    const int ow = sift_ow(f, a.o), oh = sift_oh(f, a.o);
    const int sw = a.pass ? oh : ow, sh = a.pass ? ow : oh;  // source width (contiguous) and height (filtered direction)
    const float* src = a.pass ? f.tmp : f.oct + (size_t)a.src_lvl * f.lstride;
    float* dst = a.pass ? f.oct + (size_t)a.dst_lvl * f.lstride : f.tmp;
    const int x0 = blockIdx.x * SIFT_CONV_TX, y0 = blockIdx.y * SIFT_CONV_TY;
    if (x0 >= sw || y0 >= sh) return;
    const int W = t.W, rows = SIFT_CONV_TY + 2 * W;
    for (int i = threadIdx.x; i < rows * SIFT_CONV_TX; i += SIFT_T) {
        const int r = i / SIFT_CONV_TX, c = i % SIFT_CONV_TX;
        const int sy = min(max(y0 - W + r, 0), sh - 1), sx = x0 + c;
        tile[r * (SIFT_CONV_TX + 1) + c] = sx < sw ? src[(size_t)sy * sw + sx] : 0.0f;
    }
    __syncthreads();
    for (int j = threadIdx.x; j < SIFT_CONV_TX * SIFT_CONV_TY; j += SIFT_T) {
        const int ly = j % SIFT_CONV_TY, lx = j / SIFT_CONV_TY;
        const int x = x0 + lx, y = y0 + ly;
        if (x < sw && y < sh) dst[(size_t)x * sh + y] = sift_conv_sample(tile + ly * (SIFT_CONV_TX + 1) + lx, SIFT_CONV_TX + 1, t.c, W);
    }
}

// position p of the octave in the reference's scan order: level s = p / (w h), then y, then x
__host__ __device__ __forceinline__ bool sift_position(const SiftFrame& f, const SiftArgs& a, size_t p, int* x, int* y, int* s, int* w, int* h) {
    *w = sift_ow(f, a.o);
    *h = sift_oh(f, a.o);
    const size_t plane = (size_t)*w * *h;
    if (p >= plane * a.S) return false;
    *s = (int)(p / plane);
    const size_t r = p - (size_t)*s * plane;
    *y = (int)(r / *w);
    *x = (int)(r - (size_t)*y * *w);
    return *x >= 1 && *x <= *w - 2 && *y >= 1 && *y <= *h - 2;
}

__global__ void __launch_bounds__(SIFT_T) k_sift_detect(SiftArgs a) {
    const SiftFrame& f = a.f[blockIdx.y];
    const size_t p = (size_t)blockIdx.x * SIFT_T + threadIdx.x;
    int x, y, s, w, h;
    if ((size_t)blockIdx.x * SIFT_T >= (size_t)sift_ow(f, a.o) * sift_oh(f, a.o) * a.S) return;
    bool key = false;
    if (sift_position(f, a, p, &x, &y, &s, &w, &h) && sift_is_extremum(f.oct, f.lstride, w, x, y, s + 1, a.tp))
        key = sift_refine(f.oct, f.lstride, w, h, x, y, s, a.S, a.o, a.tp, a.te_bound, a.sigma0, nullptr);
    const unsigned long long m = __ballot(key);
    if ((threadIdx.x & 63) == 0) f.mask[p >> 6] = m;
}

__global__ void __launch_bounds__(SIFT_SCAN_T) k_sift_scan(SiftArgs a) {
    __shared__ int part[SIFT_SCAN_T];
    const SiftFrame& f = a.f[blockIdx.x];
    const size_t npos = (size_t)sift_ow(f, a.o) * sift_oh(f, a.o) * a.S;
    const size_t nw = (npos + SIFT_T - 1) / SIFT_T * (SIFT_T / 64);  // words k_sift_detect wrote
    const size_t per = (nw + SIFT_SCAN_T - 1) / SIFT_SCAN_T, lo = min(nw, per * threadIdx.x), hi = min(nw, lo + per);
    int sum = 0;
    for (size_t i = lo; i < hi; ++i) sum += __popcll(f.mask[i]);
    part[threadIdx.x] = sum;
    __syncthreads();
    for (int d = 1; d < SIFT_SCAN_T; d <<= 1) {  // inclusive scan
        const int v = threadIdx.x >= d ? part[threadIdx.x - d] : 0;
        __syncthreads();
        part[threadIdx.x] += v;
        __syncthreads();
    }
    const int base = f.hdr[SIFT_H_KP_TOTAL], total = part[SIFT_SCAN_T - 1];
    int run = base + part[threadIdx.x] - sum;
    for (size_t i = lo; i < hi; ++i) {
        f.woff[i] = run;
        run += __popcll(f.mask[i]);
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        const int first = min(base, f.kp_cap), last = min(base + total, f.kp_cap);
        f.hdr[SIFT_H_OCT_START] = first;
        f.hdr[SIFT_H_OCT_N] = last - first;
        f.hdr[SIFT_H_KP_TOTAL] = base + total;
        f.hdr[SIFT_H_OCTAVES] = a.o + 1;
    }
}

__global__ void __launch_bounds__(SIFT_T) k_sift_emit(SiftArgs a) {
    const SiftFrame& f = a.f[blockIdx.y];
    const size_t p = (size_t)blockIdx.x * SIFT_T + threadIdx.x;
    if ((size_t)blockIdx.x * SIFT_T >= (size_t)sift_ow(f, a.o) * sift_oh(f, a.o) * a.S) return;
    const unsigned long long m = f.mask[p >> 6];
    const int lane = threadIdx.x & 63;
    if (!((m >> lane) & 1)) return;
    const int idx = f.woff[p >> 6] + __popcll(m & ((1ull << lane) - 1));
    if (idx >= f.kp_cap) return;
    int x, y, s, w, h;
    sift_position(f, a, p, &x, &y, &s, &w, &h);
    sift_refine(f.oct, f.lstride, w, h, x, y, s, a.S, a.o, a.tp, a.te_bound, a.sigma0, &f.kp[idx]);
}

__global__ void __launch_bounds__(SIFT_T) k_sift_grad(SiftArgs a) {
    const SiftFrame& f = a.f[blockIdx.z];
    if (f.hdr[SIFT_H_OCT_N] == 0) return;  // the reference computes gradients on the first keypoint's demand only
    const int w = sift_ow(f, a.o), h = sift_oh(f, a.o);
    const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (x >= w || y >= h || w < 2 || h < 2) return;
    for (int s = 0; s < a.S; ++s) {
        float mod, ang;
        sift_grad_pixel(f.oct + (size_t)(s + 1) * f.lstride, w, h, x, y, &mod, &ang);
        *reinterpret_cast<float2*>(f.grad + (size_t)s * 2 * f.lstride + 2 * ((size_t)y * w + x)) = make_float2(mod, ang);
    }
}

__global__ void __launch_bounds__(WAVE) k_sift_orient(SiftArgs a) {
    __shared__ double v0[WAVE], v1[WAVE], hist[SIFT_NBINS];
    __shared__ int b0[WAVE], b1[WAVE];
    const SiftFrame& f = a.f[blockIdx.y];
    const int w = sift_ow(f, a.o), h = sift_oh(f, a.o), lane = threadIdx.x;
    const int first = f.hdr[SIFT_H_OCT_START], n = f.hdr[SIFT_H_OCT_N];
    for (int k = first + blockIdx.x; k < first + n; k += gridDim.x) {
        const SiftGeom q = sift_geom(f.kp[k], a.o);
        if (!sift_orient_inside(q, w, h, a.S)) {
            if (lane == 0) f.nang[k] = 0;
            continue;
        }
        const int W = sift_orient_window(q);
        const int ya = max(-W, -q.yi), yb = min(W, h - 1 - q.yi), xa = max(-W, -q.xi), xb = min(W, w - 1 - q.xi);
        const int nx = xb - xa + 1, npix = nx * (yb - ya + 1);
        const float* g = f.grad + (size_t)q.si * 2 * f.lstride;
        double acc = 0;
        for (int base = 0; base < npix; base += WAVE) {
            const int i = base + lane;
            int c0 = -1, c1 = -1;
            double t0 = 0, t1 = 0;
            if (i < npix) {
                const int ys = ya + i / nx, xs = xa + i % nx;
                const float2 ma = *reinterpret_cast<const float2*>(g + 2 * ((size_t)(q.yi + ys) * w + (q.xi + xs)));
                if (!sift_orient_term(q, W, xs, ys, ma.x, ma.y, a.expn, &c0, &t0, &c1, &t1)) c0 = c1 = -1;
            }
            __syncthreads();
            b0[lane] = c0;
            b1[lane] = c1;
            v0[lane] = t0;
            v1[lane] = t1;
            __syncthreads();
            if (lane < SIFT_NBINS)
                for (int e = 0; e < WAVE; ++e) {
                    if (b0[e] == lane) acc += v0[e];
                    if (b1[e] == lane) acc += v1[e];
                }
        }
        __syncthreads();
        if (lane < SIFT_NBINS) hist[lane] = acc;
        __syncthreads();
        if (lane == 0) {
            double hh[SIFT_NBINS], ang[4];
            for (int i = 0; i < SIFT_NBINS; ++i) hh[i] = hist[i];
            const int na = sift_orient_finish(hh, ang);
            f.nang[k] = na;
            for (int j = 0; j < na; ++j) f.ang[4 * (size_t)k + j] = ang[j];
        }
    }
}

__global__ void __launch_bounds__(SIFT_SCAN_T) k_sift_fscan(SiftArgs a) {
    __shared__ int part[SIFT_SCAN_T];
    const SiftFrame& f = a.f[blockIdx.x];
    const int first = f.hdr[SIFT_H_OCT_START], n = f.hdr[SIFT_H_OCT_N];
    const int per = (n + SIFT_SCAN_T - 1) / SIFT_SCAN_T, lo = min(n, per * (int)threadIdx.x), hi = min(n, lo + per);
    int sum = 0;
    for (int i = lo; i < hi; ++i) sum += f.nang[first + i];
    part[threadIdx.x] = sum;
    __syncthreads();
    for (int d = 1; d < SIFT_SCAN_T; d <<= 1) {
        const int v = threadIdx.x >= d ? part[threadIdx.x - d] : 0;
        __syncthreads();
        part[threadIdx.x] += v;
        __syncthreads();
    }
    const int base = f.hdr[SIFT_H_FEAT_TOTAL];
    int run = base + part[threadIdx.x] - sum;
    for (int i = lo; i < hi; ++i) {
        f.foff[first + i] = run;
        run += f.nang[first + i];
    }
    __syncthreads();
    if (threadIdx.x == 0) f.hdr[SIFT_H_FEAT_TOTAL] = base + part[SIFT_SCAN_T - 1];
}

__global__ void __launch_bounds__(WAVE) k_sift_desc(SiftArgs a) {
    __shared__ float e_wm[WAVE], e_rx[WAVE], e_ry[WAVE], e_rt[WAVE], bins[SIFT_DESC];
    __shared__ int e_bin[WAVE];  // binx + 8, biny + 8, bint packed; -1: no term
    const SiftFrame& f = a.f[blockIdx.y];
    const int w = sift_ow(f, a.o), h = sift_oh(f, a.o), lane = threadIdx.x;
    const int first = f.hdr[SIFT_H_OCT_START], n = f.hdr[SIFT_H_OCT_N];
    for (int k = first + blockIdx.x; k < first + n; k += gridDim.x) {
        const SiftGeom q = sift_geom(f.kp[k], a.o);
        const int na = f.nang[k];
        for (int j = 0; j < na; ++j) {
            const int row = f.foff[k] + j;
            if (row >= f.feat_cap) break;
            const double angle0 = f.ang[4 * (size_t)k + j];
            float acc0 = 0, acc1 = 0;  // bins lane and lane + 64
            if (sift_desc_inside(q, w, h, a.S)) {
                const SiftDescFrame d = sift_desc_frame(q, angle0, a.magnif);
                const int ya = max(-d.W, 1 - q.yi), yb = min(d.W, h - q.yi - 2), xa = max(-d.W, 1 - q.xi), xb = min(d.W, w - q.xi - 2);
                const int nx = xb - xa + 1, npix = (nx > 0 && yb >= ya) ? nx * (yb - ya + 1) : 0;
                const float* g = f.grad + (size_t)q.si * 2 * f.lstride;
                for (int base = 0; base < npix; base += WAVE) {
                    const int i = base + lane;
                    SiftDescTerm t;
                    int packed = -1;
                    t.wm = t.rbinx = t.rbiny = t.rbint = 0;
                    if (i < npix) {
                        const int dyi = ya + i / nx, dxi = xa + i % nx;
                        const float2 ma = *reinterpret_cast<const float2*>(g + 2 * ((size_t)(q.yi + dyi) * w + (q.xi + dxi)));
                        t = sift_desc_term(q, d, dxi, dyi, ma.x, ma.y, a.wsigma, a.expn);
                        if (t.binx >= -3 && t.binx <= 1 && t.biny >= -3 && t.biny <= 1 && t.bint >= 0 && t.bint <= 8)
                            packed = (t.binx + 8) | ((t.biny + 8) << 8) | (t.bint << 16);
                    }
                    __syncthreads();
                    e_bin[lane] = packed;
                    e_wm[lane] = t.wm;
                    e_rx[lane] = t.rbinx;
                    e_ry[lane] = t.rbiny;
                    e_rt[lane] = t.rbint;
                    __syncthreads();
                    for (int e = 0; e < WAVE; ++e) {
                        const int pk = e_bin[e];
                        if (pk < 0) continue;
                        SiftDescTerm u;
                        u.binx = (pk & 255) - 8;
                        u.biny = ((pk >> 8) & 255) - 8;
                        u.bint = pk >> 16;
                        u.wm = e_wm[e];
                        u.rbinx = e_rx[e];
                        u.rbiny = e_ry[e];
                        u.rbint = e_rt[e];
                        float wgt;
                        if (sift_desc_weight(u, lane, &wgt)) acc0 += wgt;
                        if (sift_desc_weight(u, lane + 64, &wgt)) acc1 += wgt;
                    }
                }
                __syncthreads();
                bins[lane] = acc0;
                bins[lane + 64] = acc1;
                __syncthreads();
                if (lane == 0) {
                    float dd[SIFT_DESC];
                    for (int i = 0; i < SIFT_DESC; ++i) dd[i] = bins[i];
                    sift_desc_finish(dd, a.norm_thresh);
                    for (int i = 0; i < SIFT_DESC; ++i) bins[i] = dd[i];
                }
                __syncthreads();
                acc0 = bins[lane];
                acc1 = bins[lane + 64];
            }
            f.f_desc[(size_t)row * SIFT_DESC + lane] = acc0;
            f.f_desc[(size_t)row * SIFT_DESC + lane + 64] = acc1;
            if (lane == 0) {
                f.f_kp[row] = k;
                f.f_angle[row] = angle0;
            }
        }
    }
}

__global__ void __launch_bounds__(WAVE) k_sift_finish(SiftArgs a) {
    const SiftFrame& f = a.f[blockIdx.x];
    if (threadIdx.x != 0) return;
    const int nk = f.hdr[SIFT_H_KP_TOTAL], nf = f.hdr[SIFT_H_FEAT_TOTAL];
    f.counts[0] = min(nk, f.kp_cap);
    f.counts[1] = min(nf, f.feat_cap);
    f.status[0] = (nk > f.kp_cap || nf > f.feat_cap) ? 1 : 0;
    f.status[1] = nk;
    f.status[2] = nf;
    f.status[3] = f.hdr[SIFT_H_OCTAVES];
}
#endif  // SIFT_HOST_EMULATION
