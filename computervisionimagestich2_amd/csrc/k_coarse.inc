// Part of stitch_kernels.hpp (included there, inside namespace sk): every pyramid level below a size threshold -- REDUCE down
// to the top, the top-level blend and the collapse back up -- in ONE launch, one workgroup per pair (k_coarse).
//
// A pyramid of L levels costs about 6 launches per level, and from ~150 columns down a launch is nothing but its own
// start-up (4.5 us per dispatch, 15 us for a collapse level whose work-items walk a chain of dependent table look-ups): for
// the reference's own panorama (1081 x 527, ten levels) the seven coarsest levels were 35 launches and a third of the whole
// blend for 0.4 % of its pixels.  Here a workgroup of CO_THREADS work-items owns one pair and walks the coarse levels in
// phases separated by workgroup barriers; the planes stay where the other kernels keep them (global memory, resident in
// the L2), so the levels above find G and E of the first coarse level exactly where they would otherwise.
//
// The arithmetic is that of the per-level kernels, sample for sample and in the same order along every line:
//   x sweeps  k_vv_x_fwd / k_vv_x_bwd   (one line per work-item, both passes back to back: the state stays in registers)
//   y sweeps  k_vv_y_fwd / k_vv_y_bwd   (two adjacent columns per work-item, rows streamed ahead: stream_rows)
//   decimate  k_decimate                (one output sample per work-item and step)
//   top       k_blend_top
//   collapse  k_collapse                (expand_at + blend_ref per output sample)
// Van Vliet blur only (the Deriche variant keeps the per-level launches).
constexpr int CO_THREADS = 512;
struct CoarseLevel {
    float* g;  // 7 planes per pair [a0 a1 a2 b0 b1 b2 m], pitched; pair stride 7 * ps
    float* e;  // 3 planes per pair (collapse chain); pair stride 3 * ps
    const int32_t *ix, *iy;  // expand tables next-coarser level -> this level (unused at the top)
    const double *ax, *ay;
    int w, h, pitch;
    size_t ps;
};
struct CoarseArgs {
    CoarseLevel lv[CO_MAXL];  // lv[0] = the first coarse level, lv[n - 1] = the top of the pyramid
    int n;
    float* T;  // blur scratch: pair stride 7 * ps of lv[0]; within a pair's region, shaped like the level in work
    VVK k;
    unsigned long long* dbg;  // STITCH_COARSE_STAMP=1 (diagnostics): [CO_MAXL][8] s_memtime stamps of pair 0's workgroup
};

// one line of w samples: causal sweep src -> dst, then the anticausal sweep in place on dst (CImg.h:34906-34931)
__device__ __forceinline__ void coarse_x_line(const float* src, float* dst, int w, const VVK& k) {
    const double iplus = (double)src[w - 1];
    double v1, v2, v3;
    v1 = v2 = v3 = (double)src[0] / k.sumsq;
    const int nch = (w + 15) >> 4;
    f4 cur[4], nxt[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) cur[q] = *reinterpret_cast<const f4*>(src + 4 * q);  // rows are padded to a multiple of 64 floats
    for (int c = 0; c < nch; ++c) {
        const int cn = c + 1 < nch ? c + 1 : c;
#pragma unroll
        for (int q = 0; q < 4; ++q) nxt[q] = *reinterpret_cast<const f4*>(src + 16 * cn + 4 * q);
        float xs[16];
#pragma unroll
        for (int q = 0; q < 4; ++q) *reinterpret_cast<f4*>(xs + 4 * q) = cur[q];
        const int jn = min(16, w - 16 * c);
        if (jn == 16) {
#pragma unroll
            for (int u = 0; u < 16; ++u) {
                double v0 = (double)xs[u];
                v0 += v1 * k.f1;
                v0 += v2 * k.f2;
                v0 += v3 * k.f3;
                xs[u] = (float)v0;
                v3 = v2;
                v2 = v1;
                v1 = v0;
            }
        } else {
#pragma unroll
            for (int u = 0; u < 16; ++u)
                if (u < jn) {
                    double v0 = (double)xs[u];
                    v0 += v1 * k.f1;
                    v0 += v2 * k.f2;
                    v0 += v3 * k.f3;
                    xs[u] = (float)v0;
                    v3 = v2;
                    v2 = v1;
                    v1 = v0;
                }
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) *reinterpret_cast<f4*>(dst + 16 * c + 4 * q) = *reinterpret_cast<const f4*>(xs + 4 * q);
#pragma unroll
        for (int q = 0; q < 4; ++q) cur[q] = nxt[q];
    }
    __threadfence_block();  // the anticausal pass re-reads what this work-item just stored
    float first;
    triggs(k, iplus, v1, v2, v3, first);
#pragma unroll
    for (int q = 0; q < 4; ++q) cur[q] = *reinterpret_cast<const f4*>(dst + 16 * (nch - 1) + 4 * q);
    for (int c = nch - 1; c >= 0; --c) {
        const int cn = c > 0 ? c - 1 : 0;
#pragma unroll
        for (int q = 0; q < 4; ++q) nxt[q] = *reinterpret_cast<const f4*>(dst + 16 * cn + 4 * q);
        float xs[16];
#pragma unroll
        for (int q = 0; q < 4; ++q) *reinterpret_cast<f4*>(xs + 4 * q) = cur[q];
        const int jn = min(16, w - 16 * c);  // samples [0, jn) of this chunk exist; sample w-1 takes the boundary value
#pragma unroll
        for (int u = 15; u >= 0; --u)
            if (u < jn) {
                if (16 * c + u == w - 1)
                    xs[u] = first;
                else {
                    double v0 = (double)xs[u];
                    v0 *= k.sum;
                    v0 += v1 * k.f1;
                    v0 += v2 * k.f2;
                    v0 += v3 * k.f3;
                    xs[u] = (float)v0;
                    v3 = v2;
                    v2 = v1;
                    v1 = v0;
                }
            }
#pragma unroll
        for (int q = 0; q < 4; ++q) *reinterpret_cast<f4*>(dst + 16 * c + 4 * q) = *reinterpret_cast<const f4*>(xs + 4 * q);
#pragma unroll
        for (int q = 0; q < 4; ++q) cur[q] = nxt[q];
    }
}

// two adjacent columns, h rows, in place: causal sweep down, anticausal sweep up (Triggs boundary from the state in registers)
__device__ __forceinline__ void coarse_y_cols(float* p, int h, int pitch, const VVK& k) {
    const f2 last = *reinterpret_cast<const f2*>(p + (size_t)(h - 1) * pitch);  // iplus, read before the sweep
    const f2 x0 = *reinterpret_cast<const f2*>(p);
    Y2 s;
    s.a1 = s.a2 = s.a3 = (double)x0.x / k.sumsq;
    s.b1 = s.b2 = s.b3 = (double)x0.y / k.sumsq;
    stream_rows<true>(p, pitch, 0, h, [&](int y, f2 xv) { *reinterpret_cast<f2*>(p + (size_t)y * pitch) = y2_step_fwd(s, k, xv); });
    __threadfence_block();  // the way back re-reads the rows just stored
    float fa, fb;
    triggs(k, (double)last.x, s.a1, s.a2, s.a3, fa);
    triggs(k, (double)last.y, s.b1, s.b2, s.b3, fb);
    f2 first;
    first.x = fa;
    first.y = fb;
    *reinterpret_cast<f2*>(p + (size_t)(h - 1) * pitch) = first;
    if (h > 1)
        stream_rows<false>(p, pitch, h - 2, h - 1, [&](int y, f2 xv) { *reinterpret_cast<f2*>(p + (size_t)y * pitch) = y2_step_bwd(s, k, xv); });
}

__global__ __launch_bounds__(CO_THREADS) void k_coarse(CoarseArgs A) {
    __shared__ int tap_s0[CO_MAXSIDE], tap_n[CO_MAXSIDE];
    __shared__ float tap_d[3 * CO_MAXSIDE];
    const int pr = blockIdx.x, tid = threadIdx.x;
    auto stamp = [&](int level, int slot) {
        if (A.dbg && pr == 0 && tid == 0) A.dbg[level * 8 + slot] = __builtin_amdgcn_s_memtime();
    };
    stamp(0, 0);
    // ---- REDUCE: blur level i into T, decimate T into level i + 1 (ImageProcess.cpp:705-715) ---------------------------
    for (int li = 0; li + 1 < A.n; ++li) {
        const CoarseLevel& a = A.lv[li];
        const CoarseLevel& b = A.lv[li + 1];
        const float* g = a.g + (size_t)pr * 7 * a.ps;
        // a pair's scratch region is sized by the FIRST coarse level at every level: the workgroups of a launch walk the levels
        // independently of each other, so their regions may not move with the level
        float* T = A.T + (size_t)pr * 7 * A.lv[0].ps;
        const int lines = 7 * a.h;  // the seven planes are contiguous (ps = pitch * h): line L starts at L * pitch
        if (a.w > 1) {
            for (int line = tid; line < lines; line += CO_THREADS) coarse_x_line(g + (size_t)line * a.pitch, T + (size_t)line * a.pitch, a.w, A.k);
        } else {
            for (int i = tid; i < lines * (a.pitch >> 2); i += CO_THREADS) reinterpret_cast<f4*>(T)[i] = reinterpret_cast<const f4*>(g)[i];
        }
        __syncthreads();
        stamp(li, 1);
        if (a.h > 1) {
            const int half = a.pitch >> 1;
            for (int cp = tid; cp < 7 * half; cp += CO_THREADS) coarse_y_cols(T + (size_t)(cp / half) * a.ps + (cp % half) * 2, a.h, a.pitch, A.k);
        }
        __syncthreads();
        stamp(li, 2);
        {  // k_decimate: one output sample per work-item and step; the pitch padding is written as 0.  The overlap weights of
           // the level's columns and rows (make_taps: a 64-bit division each) are worked out once per level, into LDS.
            for (int i = tid; i < b.w + b.h; i += CO_THREADS) {
                const Taps t = i < b.w ? make_taps(i, a.w, b.w) : make_taps(i - b.w, a.h, b.h);
                tap_s0[i] = t.s0;
                tap_n[i] = t.n;
#pragma unroll
                for (int j = 0; j < 3; ++j) tap_d[3 * i + j] = t.d[j];  // a 2:1 step has two or three overlaps per output sample
            }
            __syncthreads();
            float* dst = b.g + (size_t)pr * 7 * b.ps;
            const float fw = (float)(unsigned)a.w, fh = (float)(unsigned)a.h;
            const int per_plane = b.h * b.pitch;
            for (int i = tid; i < 7 * per_plane; i += CO_THREADS) {
                const int pl = i / per_plane, r = i - pl * per_plane, y = r / b.pitch, x = r - y * b.pitch;
                float out = 0.f;
                if (x < b.w) {
                    const int xn = tap_n[x], yn = tap_n[b.w + y];
                    const float* p = T + (size_t)pl * a.ps + tap_s0[x] + (size_t)tap_s0[b.w + y] * a.pitch;
                    // every tap of the 3 x 3 window is fetched up front (addresses clamped to the taps that exist), then
                    // accumulated in k_decimate's order: x within a row, rows in increasing y
                    float v[3][3];
#pragma unroll
                    for (int j = 0; j < 3; ++j)
#pragma unroll
                        for (int t = 0; t < 3; ++t) v[j][t] = p[(size_t)(j < yn ? j : 0) * a.pitch + (t < xn ? t : 0)];
                    float acc_y = 0.f;
#pragma unroll
                    for (int j = 0; j < 3; ++j)
                        if (j < yn) {
                            float acc = 0.f;
#pragma unroll
                            for (int t = 0; t < 3; ++t)
                                if (t < xn) acc += v[j][t] * tap_d[3 * x + t];
                            acc /= fw;
                            acc_y += acc * tap_d[3 * (b.w + y) + j];
                        }
                    out = acc_y / fh;
                }
                dst[(size_t)pl * b.ps + (size_t)y * b.pitch + x] = out;
            }
        }
        __syncthreads();
        stamp(li, 3);
    }
    // ---- top level: E = a*m + b*(1-m) (k_blend_top) ---------------------------------------------------------------------
    {
        const CoarseLevel& t = A.lv[A.n - 1];
        const float* g = t.g + (size_t)pr * 7 * t.ps;
        float* e = t.e + (size_t)pr * 3 * t.ps;
        for (int i = tid; i < t.h * t.pitch; i += CO_THREADS) {
            const float m = g[i + 6 * t.ps];
#pragma unroll
            for (int c = 0; c < 3; ++c) e[i + c * t.ps] = blend_ref(g[i + c * t.ps], g[i + (3 + c) * t.ps], m);
        }
    }
    __syncthreads();
    stamp(A.n - 1, 4);
    // ---- collapse, coarse to fine (k_collapse<float, false>) -------------------------------------------------------------
    for (int li = A.n - 2; li >= 0; --li) {
        const CoarseLevel& a = A.lv[li];
        const CoarseLevel& nx = A.lv[li + 1];
        const float* g = a.g + (size_t)pr * 7 * a.ps;
        const float* gn = nx.g + (size_t)pr * 7 * nx.ps;
        const float* en = nx.e + (size_t)pr * 3 * nx.ps;
        float* e = a.e + (size_t)pr * 3 * a.ps;
        const ExpandTab tb{a.ix, a.ax, a.iy, a.ay};
        for (int i = tid; i < a.h * a.pitch; i += CO_THREADS) {
            const int y = i / a.pitch, x = i - y * a.pitch;
            if (x >= a.w) {
#pragma unroll
                for (int c = 0; c < 3; ++c) e[i + c * a.ps] = 0.f;
                continue;
            }
            const ExpandPos ep = expand_pos(tb, x, y, nx.w, nx.h, nx.pitch);
            const float m = g[i + 6 * a.ps];
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const float ea = expand_at(gn + c * nx.ps, ep), eb = expand_at(gn + (3 + c) * nx.ps, ep), ee = expand_at(en + c * nx.ps, ep);
                const float la = g[i + c * a.ps] - ea;
                const float lb = g[i + (3 + c) * a.ps] - eb;
                const float s_ = blend_ref(la, lb, m);
                float v = s_ + ee;
                if (v > 255.f)
                    v = 255.f;
                else if (v < 0.f)
                    v = 0.f;
                e[i + c * a.ps] = v;
            }
        }
        __syncthreads();
        stamp(li, 5);
    }
}

// ---- the same walk with every level in LDS (k_coarse_lds) ---------------------------------------------------------------------
// k_coarse keeps the planes in global memory: every phase of every level -- an x pass, a y pass, the taps, the decimation, a collapse
// level -- is then a chain of L2 round trips between two workgroup barriers, 1.3 to 7.8 us a phase whatever the level's size (phase
// stamps of round 4: 65 us for the five levels below 33 x 16, of which the arithmetic is a few).  Here the workgroup copies the first
// coarse level into LDS once, keeps G of every level, the blur scratch and the collapse chain E there, and writes back only what the
// levels above read: E of the first coarse level.  Rows are pitched to an odd number of floats, so that 64 lines (x passes, lane =
// line) and 64 columns (everything else, lane = column) both spread over the banks.  The arithmetic and its order per sample are
// k_coarse's; the host takes this form when the levels fit (coarse_lds_floats).
struct CoarseLds {
    int g[CO_MAXL], e[CO_MAXL];  // float offsets of a level's 7 planes G / 3 planes E in the dynamic LDS array
    int t;                       // blur scratch, shaped like the level in work
    int p[CO_MAXL];              // row pitch of a level in LDS (odd)
};
__device__ __forceinline__ void lds_x_line(const float* src, float* dst, int w, const VVK& k) {  // coarse_x_line
    const double iplus = (double)src[w - 1];
    double v1, v2, v3;
    v1 = v2 = v3 = (double)src[0] / k.sumsq;
    int j = 0;
    for (; j + 8 <= w; j += 8) {
        float xs[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) xs[u] = src[j + u];
#pragma unroll
        for (int u = 0; u < 8; ++u) xs[u] = x_step_fwd(xs[u], k, v1, v2, v3);
#pragma unroll
        for (int u = 0; u < 8; ++u) dst[j + u] = xs[u];
    }
    for (; j < w; ++j) dst[j] = x_step_fwd(src[j], k, v1, v2, v3);
    float first;
    triggs(k, iplus, v1, v2, v3, first);
    dst[w - 1] = first;  // sample w-1 takes the boundary value and leaves the state as triggs() set it
    j = w - 1;
    for (; j - 8 >= 0; j -= 8) {
        float xs[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) xs[u] = dst[j - 1 - u];
#pragma unroll
        for (int u = 0; u < 8; ++u) xs[u] = x_step_bwd(xs[u], k, v1, v2, v3);
#pragma unroll
        for (int u = 0; u < 8; ++u) dst[j - 1 - u] = xs[u];
    }
    for (--j; j >= 0; --j) dst[j] = x_step_bwd(dst[j], k, v1, v2, v3);
}
__device__ __forceinline__ void lds_y_col(float* p, int h, int pitch, const VVK& k) {  // one column, in place (coarse_y_cols)
    const double last = (double)p[(h - 1) * pitch];
    double v1, v2, v3;
    v1 = v2 = v3 = (double)p[0] / k.sumsq;
    int y = 0;
    for (; y + 8 <= h; y += 8) {
        float xs[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) xs[u] = p[(y + u) * pitch];
#pragma unroll
        for (int u = 0; u < 8; ++u) xs[u] = x_step_fwd(xs[u], k, v1, v2, v3);
#pragma unroll
        for (int u = 0; u < 8; ++u) p[(y + u) * pitch] = xs[u];
    }
    for (; y < h; ++y) p[y * pitch] = x_step_fwd(p[y * pitch], k, v1, v2, v3);
    float first;
    triggs(k, last, v1, v2, v3, first);
    p[(h - 1) * pitch] = first;
    y = h - 1;
    for (; y - 8 >= 0; y -= 8) {
        float xs[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) xs[u] = p[(y - 1 - u) * pitch];
#pragma unroll
        for (int u = 0; u < 8; ++u) xs[u] = x_step_bwd(xs[u], k, v1, v2, v3);
#pragma unroll
        for (int u = 0; u < 8; ++u) p[(y - 1 - u) * pitch] = xs[u];
    }
    for (--y; y >= 0; --y) p[y * pitch] = x_step_bwd(p[y * pitch], k, v1, v2, v3);
}
__global__ __launch_bounds__(CO_THREADS) void k_coarse_lds(CoarseArgs A, CoarseLds O) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    __shared__ int tap_s0[CO_MAXSIDE], tap_n[CO_MAXSIDE];
    __shared__ float tap_d[3 * CO_MAXSIDE];
    __shared__ int t_ix[CO_TABN], t_iy[CO_TABN];
    __shared__ double t_ax[CO_TABN], t_ay[CO_TABN];
    const int pr = blockIdx.x, tid = threadIdx.x;
    // ---- in: G of the first coarse level, the expand tables of every level but the top -------------------------------------
    {
        const CoarseLevel& a = A.lv[0];
        const float* g = a.g + (size_t)pr * 7 * a.ps;
        const int P = O.p[0], per = a.w * a.h;
        for (int i = tid; i < 7 * per; i += CO_THREADS) {
            const int pl = i / per, r = i - pl * per, y = r / a.w, x = r - y * a.w;
            sm[O.g[0] + (pl * a.h + y) * P + x] = g[(size_t)pl * a.ps + (size_t)y * a.pitch + x];
        }
        int ox = 0, oy = 0;
        for (int li = 0; li + 1 < A.n; ++li) {
            const CoarseLevel& v = A.lv[li];
            for (int i = tid; i < v.w; i += CO_THREADS) t_ix[ox + i] = v.ix[i], t_ax[ox + i] = v.ax[i];
            for (int i = tid; i < v.h; i += CO_THREADS) t_iy[oy + i] = v.iy[i], t_ay[oy + i] = v.ay[i];
            ox += v.w, oy += v.h;
        }
    }
    __syncthreads();
    // ---- REDUCE: blur level i into T, decimate T into level i + 1 (ImageProcess.cpp:705-715) ---------------------------
    for (int li = 0; li + 1 < A.n; ++li) {
        const CoarseLevel& a = A.lv[li];
        const CoarseLevel& b = A.lv[li + 1];
        const int P = O.p[li], Pb = O.p[li + 1];
        const float* G = sm + O.g[li];
        float* T = sm + O.t;
        const int lines = 7 * a.h;  // the seven planes are contiguous: line L starts at L * P
        if (a.w > 1) {
            for (int line = tid; line < lines; line += CO_THREADS) lds_x_line(G + line * P, T + line * P, a.w, A.k);
        } else {
            for (int line = tid; line < lines; line += CO_THREADS) T[line * P] = G[line * P];
        }
        __syncthreads();
        if (a.h > 1) {
            for (int c = tid; c < 7 * a.w; c += CO_THREADS) {
                const int pl = c / a.w, x = c - pl * a.w;
                lds_y_col(T + pl * a.h * P + x, a.h, P, A.k);
            }
        }
        // the overlap weights of the next level's columns and rows (make_taps: a 64-bit division each), once per level
        for (int i = tid; i < b.w + b.h; i += CO_THREADS) {
            const Taps t = i < b.w ? make_taps(i, a.w, b.w) : make_taps(i - b.w, a.h, b.h);
            tap_s0[i] = t.s0;
            tap_n[i] = t.n;
#pragma unroll
            for (int j = 0; j < 3; ++j) tap_d[3 * i + j] = t.d[j];
        }
        __syncthreads();
        {  // k_decimate: one output sample per work-item and step
            float* dst = sm + O.g[li + 1];
            const float fw = (float)(unsigned)a.w, fh = (float)(unsigned)a.h;
            const int per = b.w * b.h;
            for (int i = tid; i < 7 * per; i += CO_THREADS) {
                const int pl = i / per, r = i - pl * per, y = r / b.w, x = r - y * b.w;
                const int xn = tap_n[x], yn = tap_n[b.w + y];
                const float* p = T + (pl * a.h + tap_s0[b.w + y]) * P + tap_s0[x];
                float v[3][3];
#pragma unroll
                for (int j = 0; j < 3; ++j)
#pragma unroll
                    for (int t = 0; t < 3; ++t) v[j][t] = p[(j < yn ? j : 0) * P + (t < xn ? t : 0)];
                float acc_y = 0.f;
#pragma unroll
                for (int j = 0; j < 3; ++j)
                    if (j < yn) {
                        float acc = 0.f;
#pragma unroll
                        for (int t = 0; t < 3; ++t)
                            if (t < xn) acc += v[j][t] * tap_d[3 * x + t];
                        acc /= fw;
                        acc_y += acc * tap_d[3 * (b.w + y) + j];
                    }
                dst[(pl * b.h + y) * Pb + x] = acc_y / fh;
            }
        }
        __syncthreads();
    }
    // ---- top level: E = a*m + b*(1-m) (k_blend_top) ---------------------------------------------------------------------
    {
        const CoarseLevel& t = A.lv[A.n - 1];
        const int P = O.p[A.n - 1], pp = t.h * P;
        const float* g = sm + O.g[A.n - 1];
        float* e = sm + O.e[A.n - 1];
        for (int i = tid; i < t.w * t.h; i += CO_THREADS) {
            const int y = i / t.w, x = i - y * t.w, o = y * P + x;
            const float m = g[o + 6 * pp];
#pragma unroll
            for (int c = 0; c < 3; ++c) e[o + c * pp] = blend_ref(g[o + c * pp], g[o + (3 + c) * pp], m);
        }
    }
    __syncthreads();
    // ---- collapse, coarse to fine (k_collapse<float, false>) -------------------------------------------------------------
    int ox = 0, oy = 0;
    for (int li = 0; li + 2 < A.n; ++li) ox += A.lv[li].w, oy += A.lv[li].h;  // the tables of level n-2
    for (int li = A.n - 2; li >= 0; --li) {
        const CoarseLevel& a = A.lv[li];
        const CoarseLevel& nx = A.lv[li + 1];
        const int P = O.p[li], Pn = O.p[li + 1], pp = a.h * P, ppn = nx.h * Pn;
        const float* g = sm + O.g[li];
        const float* gn = sm + O.g[li + 1];
        const float* en = sm + O.e[li + 1];
        float* e = sm + O.e[li];
        const ExpandTab tb{t_ix + ox, t_ax + ox, t_iy + oy, t_ay + oy};
        for (int i = tid; i < a.w * a.h; i += CO_THREADS) {
            const int y = i / a.w, x = i - y * a.w, o = y * P + x;
            const ExpandPos ep = expand_pos(tb, x, y, nx.w, nx.h, Pn);
            const float m = g[o + 6 * pp];
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const float ea = expand_at(gn + c * ppn, ep), eb = expand_at(gn + (3 + c) * ppn, ep), ee = expand_at(en + c * ppn, ep);
                const float la = g[o + c * pp] - ea;
                const float lb = g[o + (3 + c) * pp] - eb;
                const float s_ = blend_ref(la, lb, m);
                float v = s_ + ee;
                if (v > 255.f)
                    v = 255.f;
                else if (v < 0.f)
                    v = 0.f;
                e[o + c * pp] = v;
            }
        }
        __syncthreads();
        if (li > 0) ox -= A.lv[li - 1].w, oy -= A.lv[li - 1].h;
    }
    // ---- out: E of the first coarse level, where the collapse of the level above reads it (padding columns as k_coarse: 0) ----
    {
        const CoarseLevel& a = A.lv[0];
        const int P = O.p[0], pp = a.h * P;
        const float* e = sm + O.e[0];
        float* eg = a.e + (size_t)pr * 3 * a.ps;
        for (int i = tid; i < 3 * a.h * a.pitch; i += CO_THREADS) {
            const int c = i / (a.h * a.pitch), r = i - c * a.h * a.pitch, y = r / a.pitch, x = r - y * a.pitch;
            eg[(size_t)c * a.ps + (size_t)y * a.pitch + x] = x < a.w ? e[c * pp + y * P + x] : 0.f;
        }
    }
}
