// Host emulation of csrc/k_sift.inc for tests/test_sift_host.py: the sift_* functions of the kernel source -- every piece of
// arithmetic a result depends on -- are compiled for the CPU (no FMA contraction) and driven by plain loops in the reference's
// order, so that they can be compared with the recorded fixtures on a machine without a GPU.  What the kernels add on top
// (which lane takes which sample, the ballot / scan compaction, the ordered histogram walk) is pinned by tests/test_gpu_sift.py.
//   sift_emulate <in> <out>
//   in : int32 w, h, octaves, levels, flags (1: dump, 2: the image is float32); double peak, edge, norm, magnif, window; w * h
//        bytes (gray) or floats
//   out: records {int32 tag, int32 octave, int64 bytes, payload}: 1 Gaussian levels, 2 DoG levels, 3 gradient planes (only
//        with dump), 4 candidates (x, y, s int32), 5 keypoints (8 x 4 bytes), 6 feature keypoint index (int32, per frame),
//        7 angles (double), 8 descriptors (128 float); 9 = filter taps (double sigma, int32 W, pad, 2W+1 floats) per new
//        filter; 10 = fast_expn's table.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#define __device__
#define __host__
#define __global__
#define __forceinline__ inline
#define SIFT_HOST_EMULATION 1
#include "k_sift.inc"

static FILE* g_out;
static void record(int tag, int o, const void* p, size_t bytes) {
    const int32_t h[2] = {tag, o};
    const int64_t n = (int64_t)bytes;
    fwrite(h, 4, 2, g_out);
    fwrite(&n, 8, 1, g_out);
    if (bytes) fwrite(p, 1, bytes, g_out);
}

static void smooth(float* dst, float* tmp, const float* src, int w, int h, double sd) {
    SiftTaps t;
    t.W = sift_make_taps(sd, t.c);
    if (t.W < 0) exit(4);
    {
        std::vector<char> rec(16 + 4 * (2 * t.W + 1));
        memcpy(rec.data(), &sd, 8);
        memcpy(rec.data() + 8, &t.W, 4);
        memcpy(rec.data() + 16, t.c, 4 * (2 * t.W + 1));
        record(9, 0, rec.data(), rec.size());
    }
    const int W = t.W;
    std::vector<float> col(2 * W + 1);
    for (int x = 0; x < w; ++x)
        for (int y = 0; y < h; ++y) {
            for (int k = 0; k <= 2 * W; ++k) col[k] = src[(size_t)std::min(std::max(y - W + k, 0), h - 1) * w + x];
            tmp[(size_t)x * h + y] = sift_conv_sample(col.data(), 1, t.c, W);
        }
    for (int x = 0; x < h; ++x)  // the transposed image: h wide, w high
        for (int y = 0; y < w; ++y) {
            for (int k = 0; k <= 2 * W; ++k) col[k] = tmp[(size_t)std::min(std::max(y - W + k, 0), w - 1) * h + x];
            dst[(size_t)x * w + y] = sift_conv_sample(col.data(), 1, t.c, W);
        }
}

int main(int argc, char** argv) {
    if (argc < 3) return 2;
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 2;
    int32_t hd[5];
    double th[5];
    if (fread(hd, 4, 5, f) != 5 || fread(th, 8, 5, f) != 5) return 2;
    const int W0 = hd[0], H0 = hd[1], S = hd[3], dump = hd[4] & 1, is_f32 = hd[4] & 2;
    const int noct = hd[2] < 0 ? sift_auto_octaves(W0, H0) : hd[2];
    const size_t ls = (size_t)W0 * H0;
    std::vector<unsigned char> gray(is_f32 ? 0 : ls);
    std::vector<float> grayf(is_f32 ? ls : 0);
    if (is_f32 ? fread(grayf.data(), 4, ls, f) != ls : fread(gray.data(), 1, ls, f) != ls) return 2;
    fclose(f);
    g_out = fopen(argv[2], "wb");
    if (!g_out) return 2;
    const double tp = th[0], te = th[1], norm_thresh = th[2], magnif = th[3];
    const float wsigma = (float)th[4];
    const double te_bound = (te + 1) * (te + 1) / te;
    const SiftPlan plan = sift_plan(S);
    double tab[258];
    for (int k = 0; k < 257; ++k) tab[k] = sift_expn_entry(k);
    tab[257] = 0;  // as k_sift_table
    record(10, 0, tab, 257 * sizeof(double));
    std::vector<float> oct((S + 3) * ls), tmp(ls), grad(2 * (size_t)S * ls), dog;
    for (size_t i = 0; i < ls; ++i) oct[i] = is_f32 ? grayf[i] : (float)gray[i];  // k_sift_load
    std::vector<SiftKeypoint> all_kp;
    std::vector<int32_t> f_kp;
    std::vector<double> f_ang;
    std::vector<float> f_desc;
    for (int o = 0; o < noct; ++o) {
        const int w = W0 >> o, h = H0 >> o;
        if (w < 1 || h < 1) break;
        const double* sd = o ? plan.sd_next : plan.sd_first;
        if (o) {
            const int sw = W0 >> (o - 1);
            std::vector<float> base((size_t)w * h);
            for (int y = 0; y < h; ++y)
                for (int x = 0; x < w; ++x) base[(size_t)y * w + x] = oct[(size_t)S * ls + (size_t)(2 * y) * sw + 2 * x];
            std::copy(base.begin(), base.end(), oct.begin());
        }
        if (sd[0] > 0) smooth(oct.data(), tmp.data(), oct.data(), w, h, sd[0]);
        for (int l = 1; l <= S + 2; ++l) smooth(oct.data() + l * ls, tmp.data(), oct.data() + (l - 1) * ls, w, h, sd[l]);
        const size_t plane = (size_t)w * h;
        if (dump) {
            std::vector<float> g((S + 3) * plane);
            for (int l = 0; l < S + 3; ++l) std::copy(oct.begin() + l * ls, oct.begin() + l * ls + plane, g.begin() + l * plane);
            record(1, o, g.data(), g.size() * 4);
            dog.resize((S + 2) * plane);
            for (int d = 0; d < S + 2; ++d)
                for (int y = 0; y < h; ++y)
                    for (int x = 0; x < w; ++x) dog[d * plane + (size_t)y * w + x] = sift_dog(oct.data(), ls, w, x, y, d);
            record(2, o, dog.data(), dog.size() * 4);
        }
        std::vector<int32_t> cand;
        std::vector<SiftKeypoint> kp;
        for (int s = 0; s < S; ++s)
            for (int y = 1; y < h - 1; ++y)
                for (int x = 1; x < w - 1; ++x)
                    if (sift_is_extremum(oct.data(), ls, w, x, y, s + 1, tp)) {
                        cand.push_back(x);
                        cand.push_back(y);
                        cand.push_back(s);
                        SiftKeypoint k;
                        if (sift_refine(oct.data(), ls, w, h, x, y, s, S, o, tp, te_bound, plan.sigma0, &k)) kp.push_back(k);
                    }
        record(4, o, cand.data(), cand.size() * 4);
        record(5, o, kp.data(), kp.size() * sizeof(SiftKeypoint));
        if (kp.empty() || w < 2 || h < 2) continue;
        for (int s = 0; s < S; ++s)
            for (int y = 0; y < h; ++y)
                for (int x = 0; x < w; ++x) {
                    float* g = grad.data() + (size_t)s * 2 * ls + 2 * ((size_t)y * w + x);
                    sift_grad_pixel(oct.data() + (size_t)(s + 1) * ls, w, h, x, y, g, g + 1);
                }
        if (dump) {
            std::vector<float> g(2 * S * plane);
            for (int s = 0; s < S; ++s) std::copy(grad.begin() + s * 2 * ls, grad.begin() + s * 2 * ls + 2 * plane, g.begin() + s * 2 * plane);
            record(3, o, g.data(), g.size() * 4);
        }
        for (size_t ki = 0; ki < kp.size(); ++ki) {
            const SiftGeom q = sift_geom(kp[ki], o);
            double angles[4];
            int na = 0;
            if (sift_orient_inside(q, w, h, S)) {
                double hist[SIFT_NBINS] = {0};
                const int Wn = sift_orient_window(q);
                const float* g = grad.data() + (size_t)q.si * 2 * ls;
                for (int ys = std::max(-Wn, -q.yi); ys <= std::min(Wn, h - 1 - q.yi); ++ys)
                    for (int xs = std::max(-Wn, -q.xi); xs <= std::min(Wn, w - 1 - q.xi); ++xs) {
                        const float* px = g + 2 * ((size_t)(q.yi + ys) * w + (q.xi + xs));
                        int b0, b1;
                        double v0, v1;
                        if (!sift_orient_term(q, Wn, xs, ys, px[0], px[1], tab, &b0, &v0, &b1, &v1)) continue;
                        hist[b0] += v0;
                        hist[b1] += v1;
                    }
                na = sift_orient_finish(hist, angles);
            }
            for (int j = 0; j < na; ++j) {
                float d[SIFT_DESC] = {0};
                if (sift_desc_inside(q, w, h, S)) {
                    const SiftDescFrame df = sift_desc_frame(q, angles[j], magnif);
                    const float* g = grad.data() + (size_t)q.si * 2 * ls;
                    for (int dyi = std::max(-df.W, 1 - q.yi); dyi <= std::min(df.W, h - q.yi - 2); ++dyi)
                        for (int dxi = std::max(-df.W, 1 - q.xi); dxi <= std::min(df.W, w - q.xi - 2); ++dxi) {
                            const float* px = g + 2 * ((size_t)(q.yi + dyi) * w + (q.xi + dxi));
                            const SiftDescTerm t = sift_desc_term(q, df, dxi, dyi, px[0], px[1], wsigma, tab);
                            for (int dbx = 0; dbx < 2; ++dbx)
                                for (int dby = 0; dby < 2; ++dby)
                                    for (int dbt = 0; dbt < 2; ++dbt) {
                                        const int bx = t.binx + dbx, by = t.biny + dby;
                                        if (bx < -2 || bx >= 2 || by < -2 || by >= 2) continue;
                                        const int bin = (by + 2) * 32 + (bx + 2) * 8 + ((t.bint + dbt) % 8);
                                        float wgt;
                                        if (!sift_desc_weight(t, bin, &wgt)) return 3;  // the lane that owns `bin` must see this term
                                        d[bin] += wgt;
                                    }
                        }
                    sift_desc_finish(d, norm_thresh);
                }
                f_kp.push_back((int32_t)(all_kp.size() + ki));
                f_ang.push_back(angles[j]);
                f_desc.insert(f_desc.end(), d, d + SIFT_DESC);
            }
        }
        all_kp.insert(all_kp.end(), kp.begin(), kp.end());
    }
    record(6, -1, f_kp.data(), f_kp.size() * 4);
    record(7, -1, f_ang.data(), f_ang.size() * 8);
    record(8, -1, f_desc.data(), f_desc.size() * 4);
    fclose(g_out);
    return 0;
}
