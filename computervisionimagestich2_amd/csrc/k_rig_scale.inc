// Part of stitch_kernels.hpp (included there, inside namespace sk, behind k_rig_formats.inc): a rig's output at the size its consumer
// wants (include/stitch_rig_scale.h, which states the rule restated here) -- the exact area average of a rectangle of many same-size
// planar images, written in any layout of k_rig_formats.inc, one launch.  It sits beside k_pack_many and uses its device functions.
//
// blockIdx.z = image, blockIdx.x = a strip of at most SC_STRIP output columns -- the host cuts the width into the fewest such strips
// and makes them equally wide, a multiple of four, so that no workgroup is left with a sliver --, blockIdx.y = a band of SC_BAND
// output rows (in turn where the grid is smaller).  The workgroup walks the band's source rows once: it stages a row's pixels of the
// strip in LDS (finished first, once per source pixel), every lane forms its output column's horizontal sum from there and adds
// wy * that sum to the accumulators of the one or two output rows the source row lies in.  A completed output row is divided once and goes through LDS to the store
// functions of k_rig_formats.inc, four pixels per work-item, so packed layouts leave in dwords.  Integers only, but for the
// quotient's estimate, which is checked; wave64, plain C++.
constexpr int SC_STRIP = 256;               // the most output columns per workgroup = its work-items
constexpr int SC_BAND = 8;                  // output rows per workgroup; even, so a 4:2:0 row pair stays inside a band
constexpr int SC_SRC = 8 * SC_STRIP + 1;    // the source pixels under a strip: w <= 8 ow, and one more where the strip starts inside one

// The target, the strips' width (a multiple of 4, at most SC_STRIP), and both axes' sizes divided by their gcd: source column x covers
// [x * rox, (x + 1) * rox), output column X covers [X * rw, (X + 1) * rw); rows likewise with roy, rh.
struct ScaleK {
    int ow, oh, sw;
    unsigned rw, rox, rh, roy;
};

// (2 S + D) div (2 D) for S <= 255 D, D <= 2^31 - 1: n = 2 S + D < 2^40 and m = 2 D < 2^32, the quotient at most 255.  The estimate is
// the float quotient: both conversions and the correctly rounded division are each off by at most 2^-24 relatively, so the estimate is
// within 2^-22 * 256 < 1 of n / m and its integer part is the quotient, one more or one less.  The remainder n - q m, exact in 64
// bits, says which: after at most one step either way 0 <= n - q m < m, which is the definition of the quotient.
__device__ __forceinline__ unsigned sc_div(unsigned long long n, unsigned m) {
    long long q = (long long)((float)n / (float)m);
    long long r = (long long)n - q * (long long)m;
    if (r < 0) --q, r += m;
    if (r >= (long long)m) ++q;
    return (unsigned)q;
}

__device__ __forceinline__ void sc_px(unsigned v, unsigned& r, unsigned& g, unsigned& b) { r = v & 255u, g = (v >> 8) & 255u, b = (v >> 16) & 255u; }

// Output row ya (4:2:0: the pair ya, yb; yb == ya on the clamped last row of an odd height) of the strip of columns X0 .. X1 - 1, by the
// first 64 work-items: group gi's four pixels from the LDS rows ra / rb (R | G << 8 | B << 16 per pixel) through k_pack_many's stores.
template <int FMT>
__device__ __forceinline__ void sc_emit(const FmtImage& e, const Nv12K& k, int ow, int oh, int X0, int X1, int ya, int yb, const unsigned* ra, const unsigned* rb) {
    using T = FmtTraits<FMT>;
    const int l = 4 * (int)threadIdx.x, x = X0 + l, npx = min(4, X1 - x);  // (X1 < ow: X1 - X0 is a multiple of 4)
    if (threadIdx.x >= SC_STRIP / 4 || npx <= 0) return;
    unsigned r[4], g[4], b[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) sc_px(ra[min(l + i, l + npx - 1)], r[i], g[i], b[i]);
    if constexpr (FMT == PIX_PLANAR) {
        const size_t pl = (size_t)ow * oh;
        uint8_t* d0 = e.data + (size_t)ya * ow + x;
        if (npx == 4 && fmt_aligned(d0, d0 + pl, d0 + 2 * pl, nullptr, 3u)) {
            *reinterpret_cast<unsigned*>(d0) = fmt_pack4(r[0], r[1], r[2], r[3]);
            *reinterpret_cast<unsigned*>(d0 + pl) = fmt_pack4(g[0], g[1], g[2], g[3]);
            *reinterpret_cast<unsigned*>(d0 + 2 * pl) = fmt_pack4(b[0], b[1], b[2], b[3]);
        } else {
            for (int i = 0; i < npx; ++i) d0[i] = (uint8_t)r[i], d0[pl + i] = (uint8_t)g[i], d0[2 * pl + i] = (uint8_t)b[i];
        }
    } else if constexpr (!T::yuv) {
        constexpr int bpp = T::bpp;
        uint8_t* drow = e.data + (size_t)ya * e.pitch;
        if (npx == 4 && fmt_aligned(drow, nullptr, nullptr, nullptr, 3u)) {
            fmt_store_4<FMT>(drow + (size_t)x * bpp, bpp == 4 && (reinterpret_cast<uintptr_t>(drow) & 15u) == 0, r, g, b);
        } else {
            for (int i = 0; i < npx; ++i) fmt_store_px<FMT>(drow + (size_t)(x + i) * bpp, r[i], g[i], b[i]);
        }
    } else if constexpr (T::c422) {
        uint8_t* drow = e.data + (size_t)ya * e.pitch;
        uint8_t* crow = fmt_crow<FMT>(e, ya, drow);
        unsigned Y[4], cb[4], cr[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) nv12_encode(k, (int)r[i], (int)g[i], (int)b[i], Y[i], cb[i], cr[i]);  // (behind the row's end: the last pixel again)
        const unsigned u0 = (cb[0] + cb[1] + 1u) >> 1, v0 = (cr[0] + cr[1] + 1u) >> 1, u1 = (cb[2] + cb[3] + 1u) >> 1, v1 = (cr[2] + cr[3] + 1u) >> 1;
        if (npx == 4 && fmt_aligned(drow, crow, nullptr, nullptr, 3u)) {
            if constexpr (T::two_planes) {
                *reinterpret_cast<unsigned*>(drow + x) = fmt_pack4(Y[0], Y[1], Y[2], Y[3]);
                *reinterpret_cast<unsigned*>(crow + x) = fmt_pack4(u0, v0, u1, v1);
            } else {
                unsigned* d = reinterpret_cast<unsigned*>(drow + 2 * (size_t)x);
                d[0] = FMT == PIX_YUYV ? fmt_pack4(Y[0], u0, Y[1], v0) : fmt_pack4(u0, Y[0], v0, Y[1]);
                d[1] = FMT == PIX_YUYV ? fmt_pack4(Y[2], u1, Y[3], v1) : fmt_pack4(u1, Y[2], v1, Y[3]);
            }
        } else {
            for (int i0 = 0; i0 < npx; i0 += 2) {  // one 2 x 1 pair; its second column is the first again on the clamped last column of an odd width
                const int xa = x + i0;
                uint8_t* c = crow + T::cstep * (xa / 2);
                if constexpr (T::two_planes) {
                    drow[xa] = (uint8_t)Y[i0];
                    drow[min(xa + 1, ow - 1)] = (uint8_t)Y[i0 + 1];
                } else {
                    c[T::yo] = (uint8_t)Y[i0];
                    c[T::yo + 2] = (uint8_t)Y[i0 + 1];
                }
                c[T::cbo] = (uint8_t)(i0 ? u1 : u0);
                c[T::cro] = (uint8_t)(i0 ? v1 : v0);
            }
        }
    } else {
        uint8_t* da = e.data + (size_t)ya * e.pitch;
        uint8_t* db = e.data + (size_t)yb * e.pitch;
        uint8_t* dc = e.data2 + (size_t)(ya / 2) * e.pitch2;
        unsigned Ya[4], Yb[4], cb[4], cr[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            unsigned u, v, r2, g2, b2;
            nv12_encode(k, (int)r[i], (int)g[i], (int)b[i], Ya[i], cb[i], cr[i]);
            sc_px(rb[min(l + i, l + npx - 1)], r2, g2, b2);
            nv12_encode(k, (int)r2, (int)g2, (int)b2, Yb[i], u, v);
            cb[i] += u, cr[i] += v;
        }
        const unsigned u0 = (cb[0] + cb[1] + 2u) >> 2, v0 = (cr[0] + cr[1] + 2u) >> 2, u1 = (cb[2] + cb[3] + 2u) >> 2, v1 = (cr[2] + cr[3] + 2u) >> 2;
        if (npx == 4 && fmt_aligned(da, db, dc, nullptr, 3u)) {
            *reinterpret_cast<unsigned*>(da + x) = fmt_pack4(Ya[0], Ya[1], Ya[2], Ya[3]);
            *reinterpret_cast<unsigned*>(db + x) = fmt_pack4(Yb[0], Yb[1], Yb[2], Yb[3]);
            *reinterpret_cast<unsigned*>(dc + x) = FMT == PIX_NV21 ? fmt_pack4(v0, u0, v1, u1) : fmt_pack4(u0, v0, u1, v1);
        } else {
            for (int i = 0; i < npx; ++i) da[x + i] = (uint8_t)Ya[i], db[x + i] = (uint8_t)Yb[i];  // (yb == ya: the same bytes again)
            for (int i0 = 0; i0 < npx; i0 += 2) {
                dc[2 * ((x + i0) / 2) + T::cbo] = (uint8_t)(i0 ? u1 : u0);
                dc[2 * ((x + i0) / 2) + T::cro] = (uint8_t)(i0 ? v1 : v0);
            }
        }
    }
}

// scratch: RIG_EQ_WORDS int32 per image as k_hist_many / k_lut_many leave them (FINISH only; the LUT is the second half)
template <int FMT, bool FINISH>
__global__ __launch_bounds__(SC_STRIP) void k_pack_scaled_many(const FmtImage* __restrict__ img, FmtRect rc, ScaleK sk, const int32_t* __restrict__ scratch, MixK mk, Nv12K k) {
    __shared__ int slut[256];
    __shared__ unsigned ssrc[SC_SRC];          // one finished source row under the strip, R | G << 8 | B << 16
    __shared__ unsigned sout[2][SC_STRIP];     // completed output rows, by the row's parity
    if constexpr (FINISH) {
        const int32_t* lut = scratch + (size_t)blockIdx.z * RIG_EQ_WORDS + 256;
        for (int i = threadIdx.x; i < 256; i += blockDim.x) slut[i] = lut[i];
        // (the first barrier of the row loop below comes before any pixel is finished)
    }
    const FmtImage e = img[blockIdx.z];
    const size_t pl = (size_t)rc.W * rc.H;
    const bool planes_agree = pl % 4 == 0;  // the three channels of a pixel then share their address's low bits
    const int ow = sk.ow, oh = sk.oh, tid = (int)threadIdx.x;
    const unsigned long long rw = sk.rw, rox = sk.rox, rh = sk.rh, roy = sk.roy;
    const unsigned m2 = 2u * (unsigned)(rw * rh);  // 2 D

    // the strip: output columns X0 .. X1 - 1 over source columns x_lo .. x_lo + nsrc - 1 (of the rectangle)
    const int X0 = (int)blockIdx.x * sk.sw, X1 = min(X0 + sk.sw, ow);
    const int x_lo = (int)((unsigned long long)X0 * rw / rox), nsrc = (int)(((unsigned long long)X1 * rw - 1) / rox) - x_lo + 1;  // <= SC_SRC
    // this lane's column: source columns xa .. xb (relative to x_lo), the first with weight wa, the last (if another) with wb, rox between
    const bool active = X0 + tid < X1;
    const unsigned long long cl = (unsigned long long)(active ? X0 + tid : X0) * rw, ch = cl + rw;
    const int xa = (int)(cl / rox) - x_lo, xb = (int)((ch - 1) / rox) - x_lo;
    const unsigned wa = (unsigned)(min(((unsigned long long)(xa + x_lo) + 1) * rox, ch) - cl), wb = xb > xa ? (unsigned)(ch - (unsigned long long)(xb + x_lo) * rox) : 0u;

    const int bands = (oh + SC_BAND - 1) / SC_BAND;
    for (int band = blockIdx.y; band < bands; band += gridDim.y) {
        const int Y0 = band * SC_BAND, Y1 = min(Y0 + SC_BAND, oh);
        const int y_lo = (int)((unsigned long long)Y0 * rh / roy), y_hi = (int)(((unsigned long long)Y1 * rh - 1) / roy);
        unsigned long long acc[2][3] = {{0ull, 0ull, 0ull}, {0ull, 0ull, 0ull}};  // output rows Y and Y + 1
        int Y = Y0;
        for (int y = y_lo; y <= y_hi; ++y) {
            __syncthreads();  // the row before has been summed, and an emitted output row stored
            const uint8_t* s0 = e.planar + (size_t)(rc.y0 + y) * rc.W + rc.x0 + x_lo;
            if constexpr (FINISH) {
                // The finish function is some hundreds of instructions per pixel and sets this loop's time: a pixel per work-item, so
                // that all of them compute (groups of four would leave half of them idle at a factor of two); the byte loads of
                // neighbouring lanes fall into the same cache lines.
                for (int c = tid; c < nsrc; c += SC_STRIP) {
                    unsigned r, g, b;
                    fmt_src_px<true>(s0 + c, pl, slut, mk, r, g, b);
                    ssrc[c] = r | (g << 8) | (b << 16);
                }
            } else {
                const int mis = planes_agree ? (int)(reinterpret_cast<uintptr_t>(s0) & 3u) : 0;  // s0 - mis is a dword's first byte
                for (int gi = tid; 4 * gi < mis + nsrc; gi += SC_STRIP) {
                    const int c0 = 4 * gi - mis;
                    if (planes_agree && c0 >= 0 && c0 + 4 <= nsrc) {
                        unsigned r[4], g[4], b[4];
                        fmt_src_4<FINISH>(s0 + c0, pl, slut, mk, r, g, b);
#pragma unroll
                        for (int i = 0; i < 4; ++i) ssrc[c0 + i] = r[i] | (g[i] << 8) | (b[i] << 16);
                    } else {
                        for (int c = max(c0, 0); c < min(c0 + 4, nsrc); ++c) {
                            unsigned r, g, b;
                            fmt_src_px<FINISH>(s0 + c, pl, slut, mk, r, g, b);
                            ssrc[c] = r | (g << 8) | (b << 16);
                        }
                    }
                }
            }
            __syncthreads();
            // the horizontal sums, each at most 255 rw: the inner pixels in two packed 16-bit fields (at most 7 * 255 each) and one for G
            unsigned long long hs[3];
            {
                unsigned rb = 0u, gg = 0u, r0, g0, b0, r1, g1, b1;
                for (int c = xa + 1; c < xb; ++c) {
                    const unsigned v = ssrc[c];
                    rb += v & 0x00ff00ffu;
                    gg += (v >> 8) & 255u;
                }
                sc_px(ssrc[xa], r0, g0, b0);
                sc_px(ssrc[xb], r1, g1, b1);
                hs[0] = (unsigned long long)wa * r0 + (unsigned long long)(unsigned)rox * (rb & 0xffffu) + (unsigned long long)wb * r1;
                hs[1] = (unsigned long long)wa * g0 + (unsigned long long)(unsigned)rox * gg + (unsigned long long)wb * g1;
                hs[2] = (unsigned long long)wa * b0 + (unsigned long long)(unsigned)rox * (rb >> 16) + (unsigned long long)wb * b1;
            }
            // source row y covers [y roy, (y + 1) roy), output row Y [Y rh, (Y + 1) rh): roy <= rh, so the row lies in Y, or in Y and Y + 1
            const unsigned long long s_lo = (unsigned long long)y * roy, s_hi = s_lo + roy, o_lo = (unsigned long long)Y * rh, o_hi = o_lo + rh;
            const unsigned w0 = (unsigned)(min(s_hi, o_hi) - max(s_lo, o_lo)), w1 = s_hi > o_hi ? (unsigned)(s_hi - o_hi) : 0u;
#pragma unroll
            for (int c = 0; c < 3; ++c) acc[0][c] += hs[c] * w0, acc[1][c] += hs[c] * w1;  // at most 255 D < 2^39 in the end
            if (s_hi >= o_hi) {  // block-uniform: row Y is complete (w1 of a row behind the band is dropped with it: that band stages the row again)
                const unsigned D = m2 >> 1;
                const unsigned r = sc_div(2 * acc[0][0] + D, m2), g = sc_div(2 * acc[0][1] + D, m2), b = sc_div(2 * acc[0][2] + D, m2);
                sout[Y & 1][tid] = r | (g << 8) | (b << 16);
#pragma unroll
                for (int c = 0; c < 3; ++c) acc[0][c] = acc[1][c], acc[1][c] = 0ull;
                constexpr bool c420 = FmtTraits<FMT>::yuv && !FmtTraits<FMT>::c422 && FMT != PIX_PLANAR;
                const bool pair_done = (Y & 1) != 0 || Y == oh - 1;
                if (!c420 || pair_done) {
                    __syncthreads();
                    if constexpr (c420)
                        sc_emit<FMT>(e, k, ow, oh, X0, X1, Y & ~1, Y, sout[0], sout[Y & 1]);
                    else
                        sc_emit<FMT>(e, k, ow, oh, X0, X1, Y, Y, sout[Y & 1], sout[Y & 1]);
                }
                ++Y;
            }
        }
    }
}
