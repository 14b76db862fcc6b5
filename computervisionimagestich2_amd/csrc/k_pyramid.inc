// Part of stitch_kernels.hpp (included there, inside namespace sk): Deriche blur, stand-alone decimation, expand / Laplacian / blend / collapse (B3', B4-B6).
// ---- B3': Deriche order 0, CImg.h:34779-34797 (all float).  The causal pass needs a line of temporaries Y; the
// anticausal pass adds Y back.  One line per work-item, y pass only coalesced; the x pass reuses the y kernel on
// a transposed view is NOT possible in place, so x runs one row per work-item straight from global memory
// (ex6 variant; not on the benchmarked path).
__global__ __launch_bounds__(64) void k_deriche(float* __restrict__ data, float* __restrict__ Y, int N, size_t off,
                                                size_t line_stride, long lines_per_plane, size_t ps, long lines, DRK k) {
    const long line = (long)blockIdx.x * WAVE + threadIdx.x;
    if (line >= lines) return;
    const long plane = line / lines_per_plane, li = line % lines_per_plane;
    float* ptrX = data + plane * ps + li * line_stride;
    float* ptrY = Y + plane * ps + li * line_stride;
    float xp = *ptrX, yb, yp;
    yb = yp = (float)(k.coefp * xp);
    for (int m = 0; m < N; ++m) {
        const float xc = ptrX[(size_t)m * off];
        const float yc = k.a0 * xc + k.a1 * xp - k.b1 * yp - k.b2 * yb;
        ptrY[(size_t)m * off] = yc;
        xp = xc;
        yb = yp;
        yp = yc;
    }
    float xn, xa, yn, ya;
    xn = xa = ptrX[(size_t)(N - 1) * off];
    yn = ya = k.coefn * xn;
    for (int n = N - 1; n >= 0; --n) {
        const float xc = ptrX[(size_t)n * off];
        const float yc = k.a2 * xn + k.a3 * xa - k.b1 * yn - k.b2 * ya;
        xa = xn;
        xn = xc;
        ya = yn;
        yn = yc;
        ptrX[(size_t)n * off] = ptrY[(size_t)n * off] + yc;
    }
}

// ---- B4: moving-average decimation, CImg.h:29539-29575 -------------------------------------------------------
// Output t of an axis accumulates, in increasing s, src[s]*(float)d into a float that starts at 0, where d is
// the overlap of [t*n_src,(t+1)*n_src) with [s*n_dst,(s+1)*n_dst), then divides once by (float)n_src.  x first
// (result rounded to float), then y -- both inside one work-item, which owns one output sample of one plane.
// yoff / soff: level row of the destination's / source's row 0 (0 for a whole level; a row band of a split pair passes its
// first rows, and the LEVEL's heights as h, h2, so that the overlap weights are the level's)
__global__ __launch_bounds__(256) void k_decimate(const float* __restrict__ src, int w, int h, int spitch, size_t sps,
                                                  float* __restrict__ dst, int w2, int h2, int dpitch, size_t dps, int yoff, int soff,
                                                  const unsigned* __restrict__ keep = nullptr) {
    const int x = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y, pl = blockIdx.z;
    if (x >= dpitch || mask_stands(keep, pl)) return;  // (a mask plane that stands is left as an earlier call wrote it)
    float out = 0.f;
    if (x < w2) {
        const Taps tx = make_taps(x, w, w2), ty = make_taps(y + yoff, h, h2);
        const float* p = src + pl * sps + tx.s0;
        const float fw = (float)(unsigned)w, fh = (float)(unsigned)h;
        float acc_y = 0.f;
        for (int j = 0; j < ty.n; ++j) {
            const float* row = p + (size_t)(ty.s0 - soff + j) * spitch;
            float acc = 0.f;
            for (int i = 0; i < tx.n; ++i) acc += row[i] * tx.d[i];
            acc /= fw;
            acc_y += acc * ty.d[j];
        }
        out = acc_y / fh;
    }
    dst[pl * dps + (size_t)y * dpitch + x] = out;
}

// ---- B5/B6: expand, Laplacian, per-level blend, collapse -----------------------------------------------------
// CImg.h:29618-29690 linear interpolation: out = (float)((1-alpha)*v1 + alpha*v2) in double with
// v2 = v1 at the last source sample; the x pass is rounded to float before the y pass.  Index/alpha tables are
// the reference's serial `curr = min(n_src-1, curr+f)` walk, computed on the host.  A source axis of length 1
// is nearest-neighbour (:29620, :29657).
struct ExpandTab {
    const int32_t* ix;
    const double* ax;
    const int32_t* iy;
    const double* ay;
};

__device__ __forceinline__ float lerp_ref(double alpha, float v1, float v2) {
    return (float)((1 - alpha) * (double)v1 + alpha * (double)v2);
}

struct ExpandPos {  // everything about (x,y) that does not depend on the plane
    int o11, o12, o21, o22;
    double ax, ay;
    bool x_nearest, y_nearest;
};
__device__ __forceinline__ ExpandPos expand_pos(const ExpandTab& tb, int x, int y, int sw, int sh, int spitch) {
    ExpandPos e;
    const int ix = tb.ix[x], iy = tb.iy[y];
    const int ix2 = ix < sw - 1 ? ix + 1 : ix, iy2 = iy < sh - 1 ? iy + 1 : iy;
    e.ax = tb.ax[x];
    e.ay = tb.ay[y];
    e.o11 = iy * spitch + ix;
    e.o12 = iy * spitch + ix2;
    e.o21 = iy2 * spitch + ix;
    e.o22 = iy2 * spitch + ix2;
    e.x_nearest = (sw == 1);
    e.y_nearest = (sh == 1);
    return e;
}
__device__ __forceinline__ float expand_at(const float* __restrict__ pl, const ExpandPos& e) {
    float r1, r2;
    if (e.x_nearest) {
        r1 = pl[e.o11];
        r2 = pl[e.o21];
    } else {
        r1 = lerp_ref(e.ax, pl[e.o11], pl[e.o12]);
        r2 = lerp_ref(e.ax, pl[e.o21], pl[e.o22]);
    }
    return e.y_nearest ? r1 : lerp_ref(e.ay, r1, r2);
}

// blend of one sample, ImageProcess.cpp:749-751: a*m is a float product, b*(1.0-m) and the sum are double.
__device__ __forceinline__ float blend_ref(float a, float b, float m) {
    const float am = a * m;
    return (float)((double)am + (double)b * (1.0 - (double)m));
}

// top level: E = a*m + b*(1-m) on the Gaussian top (no Laplacian, no clamp); E has 3 pitched planes.
__global__ __launch_bounds__(256) void k_blend_top(const float* __restrict__ g_all, int pitch, int h, size_t ps,
                                                   float* __restrict__ e_all) {
    const int x = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y;
    if (x >= pitch) return;
    const float* g = g_all + (size_t)blockIdx.z * 7 * ps;
    float* e = e_all + (size_t)blockIdx.z * 3 * ps;
    const size_t o = (size_t)y * pitch + x;
    const float m = g[o + 6 * ps];
#pragma unroll
    for (int c = 0; c < 3; ++c) e[o + c * ps] = blend_ref(g[o + c * ps], g[o + (3 + c) * ps], m);
}

// level l < L-1:  La = Ga_l - EXPAND(Ga_{l+1}), Lb likewise (float subtract, CImg.h:12096-12107);
// S = blend(La, Lb, m_l);  E_l = clamp(S + EXPAND(E_{l+1}), 0, 255) (ImageProcess.cpp:766-769).
// OUT = float planes (pitched, next collapse input) or the final dense canvas (float, or uint8_t by truncation).
template <typename OUT>
struct OutPtrs {
    OUT* p[MAXB];
    uint8_t* q[MAXB];  // optional second copy of a float mosaic as unsigned char (the reference's own output type,
                       // CImg<unsigned char>(CImg<float>): C-cast truncation), written by the level-0 collapse; nullptr = none
};
// One work-item owns one column of a strip of CROWS output rows.  EXPAND's x pass depends only on the source row,
// and consecutive output rows share their source rows (iy advances by at most one per output row when
// up-sampling), so the x-interpolated values of the two current source rows are kept in registers and only a newly
// entered source row is interpolated: the double-precision work per pixel halves, the values are the same floats.
// G_0 of a source-fused plan: evaluated from the pair's frames; otherwise read from the level's planes.
template <typename OUT>
__device__ __forceinline__ void level_ab(const PairArgs<OUT>& pa, int pr, int use_src, const float* g, size_t o, size_t ps, int x, int y,
                                         float a[3], float b[3]) {
    if (use_src) {  // branch-free: clamped addresses, zero selected afterwards
        const PairSrc<OUT> src(pa, pr);
        size_t fso = 0;
        bool fin;
        if (src.a_dense)
            fin = src.frame_at(x, y, fso);  // canvas a as it stands: no index plane
        else {
            const unsigned fo = reinterpret_cast<const unsigned*>(g)[o];  // k_src_index's byte offset in the slot of plane 0 (g: collapse_slot)
            fin = fo != off_outside<OUT>();
            fso = fo / sizeof(OUT);
        }
        fso = fin ? fso : 0;
        size_t mo = 0;
        const bool min_ = src.mosaic_at(x, y, mo);
        mo = min_ ? mo : 0;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float fa = src.frame_val(fso, c), fb = src.mosaic_val(mo, c);
            a[c] = fin ? fa : 0.f;
            b[c] = min_ ? fb : 0.f;
        }
    } else {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            a[c] = g[o + c * ps];
            b[c] = g[o + (3 + c) * ps];
        }
    }
}
__device__ __forceinline__ void level_ab(const NoPairArgs&, int, int, const float* g, size_t o, size_t ps, int, int, float a[3], float b[3]) {
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        a[c] = g[o + c * ps];
        b[c] = g[o + (3 + c) * ps];
    }
}
// everything a collapse launch of one level needs (kernel argument)
template <typename OUT, bool DENSE>
struct CollapseArgs {
    const float* g_all;  // level l: 7 planes per pair (plane 0 = the index plane when source-fused)
    int w, h, pitch;
    size_t ps;
    const float *gn_all, *en_all;  // level l+1: G (7 planes per pair) and E (3 planes per pair)
    int sw, sh, spitch;
    size_t sps;
    ExpandTab tb;
    OutPtrs<OUT> outs;
    int opitch;
    size_t ops;
    const SeamDev* seam_l0;  // level 0: the mask is the seam's step function
    typename CollapseSrc<OUT, DENSE>::type pa;
    int use_src, crows;
    int xa, xb;  // columns [xa, xb) are done four per work-item (collapse_cols4), the rest one per work-item
    int u8_words;  // level 0: rows of the unsigned char destination(s) start on 32-bit boundaries (w % 4 == 0, aligned buffers)
    int lockstep;  // k_collapse4: the three channel wavefronts of a workgroup meet at a barrier every row (see collapse_cols4)
    int swizzle;   // k_collapse4: column blocks handed to the XCDs in contiguous runs (see k_collapse4)
    // G column flags (g_cols) of this level and of level l+1, [7 planes per pair][tile columns]; nullptr: every column is stored.
    // A flagged column is not loaded: the address goes to the zeros that lie behind the level's last plane for good (its slack
    // rows, never written), zo / zon floats behind g_all / gn_all.  The loads themselves stay unconditional.
    const uint8_t *gz, *gzn;
    int gnc, gncn;
    unsigned zo, zon;
};
// Row-repeat flags of the level's mask plane (mask_rows), [pairs][nc tile columns][nr bands]: an argument of the MR instances of the
// collapse kernels only (levels 1 and 2 of a call with the flags on), so that every other instance is compiled as it was.  The mask
// sample of a flagged tile is loaded from row 0 of the same columns: an address select, the load stays unconditional.  The flag is
// looked up where a strip starts and where it enters a new 64-row band, and kept from row to row in between.
struct MaskRowsArg {
    const uint8_t* flags;
    int nc, nr;
};
__device__ __forceinline__ bool collapse_mask_row(const MaskRowsArg& mr, int pr, int x, int y) {
#if STITCH_MASK_ROWS_IGNORE & 4  // (hand-check libraries only: a collapse that reads the unstored tiles)
    return false;
#else
    return mask_row_flag(mr.flags, mr.nc, mr.nr, pr, x, y);
#endif
}
// the samples at columns x and x2 (x <= x2 <= x + 3) of a plane are both taken as zeros: either tile column is flagged
__device__ __forceinline__ bool g_span_flag(const uint8_t* __restrict__ flags, int nc, int plane, int x, int x2) {
    return flags != nullptr && (g_col_flag(flags, nc, plane, x) || g_col_flag(flags, nc, plane, x2));
}

// The level's slot that pair pr reads.  A source-fused level 0 reads ONE thing from its slot, the index plane (the mask is the seam's
// step, the six planes come from the frames), and that is the plane of the pair's owner (PairArgs::idx_pr); every other level: pr's own.
template <typename OUT, bool DENSE>
__device__ __forceinline__ int collapse_slot(const CollapseArgs<OUT, DENSE>& A, int pr) {
    return DENSE && A.use_src ? index_owner(A.pa, pr) : pr;
}
// one column x, rows [y0, y1) of pair pr
template <typename OUT, bool DENSE, bool MR = false>
__device__ __forceinline__ void collapse_cols1(const CollapseArgs<OUT, DENSE>& A, int x, int y0, int y1, int pr, MaskRowsArg mr = MaskRowsArg{}) {
    const int w = A.w, pitch = A.pitch, sw = A.sw, sh = A.sh, spitch = A.spitch, opitch = A.opitch;
    const size_t ps = A.ps, sps = A.sps, ops = A.ops;
    const ExpandTab& tb = A.tb;
    const SeamDev* __restrict__ seam_l0 = A.seam_l0;
    const float* g = A.g_all + (size_t)collapse_slot(A, pr) * 7 * ps;
    const float* gn = A.gn_all + (size_t)pr * 7 * sps;
    const float* en = A.en_all + (size_t)pr * 3 * sps;
    OUT* __restrict__ out = DENSE ? A.outs.p[pr] : A.outs.p[0] + (size_t)pr * 3 * ops;
    if (!DENSE && x >= w) {
        for (int y = y0; y < y1; ++y)
#pragma unroll
            for (int c = 0; c < 3; ++c) out[(size_t)y * opitch + x + c * ops] = OUT(0);
        return;
    }
    const int ix = tb.ix[x], ix2 = ix < sw - 1 ? ix + 1 : ix;
    const double ax = tb.ax[x];
    const bool x_nearest = (sw == 1), y_nearest = (sh == 1);
    // G column flags, looked up once per work-item: bit q = plane q of level l+1 at this column's two taps, bit 8 + q = plane q of
    // this level at column x; a flagged sample is read from the zeros behind the level's last plane (CollapseArgs::zo / zon)
    unsigned gzb = 0;
#pragma unroll
    for (int q = 0; q < 6; ++q) {
#if !(STITCH_G_IGNORE_COARSER & 2)  // (the two macros: see collapse_cols4)
        if (g_span_flag(A.gzn, A.gncn, pr * 7 + q, ix, ix2)) gzb |= 1u << q;
#endif
#if !(STITCH_G_IGNORE_OWN & 2)
        if (!DENSE && g_span_flag(A.gz, A.gnc, pr * 7 + q, x, x)) gzb |= 0x100u << q;
#endif
    }
    const size_t zn = (size_t)A.zon - (size_t)pr * 7 * sps, zg = (size_t)A.zo - (size_t)pr * 7 * ps;  // the zeros, from gn / g
    // x pass of one source row for the nine planes that are expanded: a0..a2, b0..b2 of G_{l+1}, then E_{l+1}
    auto xrow = [&](int row, float X[9]) {
        const size_t o1 = (size_t)row * spitch + ix, o2 = (size_t)row * spitch + ix2;
#pragma unroll
        for (int q = 0; q < 9; ++q) {
            const float* pl = q < 6 ? gn + q * sps : en + (q - 6) * sps;
            if (q < 6 && ((gzb >> q) & 1u) != 0)
                X[q] = x_nearest ? gn[zn] : lerp_ref(ax, gn[zn], gn[zn + 1]);
            else
                X[q] = x_nearest ? pl[o1] : lerp_ref(ax, pl[o1], pl[o2]);
        }
    };
    float X1[9], X2[9];
    int cur1 = -1, cur2 = -1;
    const float m_step = seam_l0 ? mask_step(seam_l0[pr], x) : 0.f;  // level 0: the mask is the step itself
    bool mrow = false;  // MR: row-repeat flag of the mask tile this row lies in
    for (int y = y0; y < y1; ++y) {
        const int iy = tb.iy[y], iy2 = iy < sh - 1 ? iy + 1 : iy;
        const double ay = tb.ay[y];
        if (iy != cur1) {
            if (iy == cur2) {
#pragma unroll
                for (int q = 0; q < 9; ++q) X1[q] = X2[q];
            } else
                xrow(iy, X1);
            cur1 = iy;
        }
        if (iy2 != cur2) {
            if (iy2 == cur1) {
#pragma unroll
                for (int q = 0; q < 9; ++q) X2[q] = X1[q];
            } else
                xrow(iy2, X2);
            cur2 = iy2;
        }
        const size_t o = (size_t)y * pitch + x;
        if constexpr (MR)
            if (y == y0 || (y & 63) == 0) mrow = collapse_mask_row(mr, pr, x, y);
        const float m = seam_l0 ? m_step : g[(MR && mrow ? (size_t)x : o) + 6 * ps];
        float ga[3], gb[3];
        if (!DENSE && gzb >= 0x100u) {  // some plane of this level is flagged at x: its samples come from the zeros
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                ga[c] = g[((gzb >> (8 + c)) & 1u) != 0 ? zg : o + c * ps];
                gb[c] = g[((gzb >> (11 + c)) & 1u) != 0 ? zg : o + (3 + c) * ps];
            }
        } else
            level_ab(A.pa, pr, A.use_src, g, o, ps, x, y, ga, gb);
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float ea = y_nearest ? X1[c] : lerp_ref(ay, X1[c], X2[c]);
            const float eb = y_nearest ? X1[3 + c] : lerp_ref(ay, X1[3 + c], X2[3 + c]);
            const float ee = y_nearest ? X1[6 + c] : lerp_ref(ay, X1[6 + c], X2[6 + c]);
            const float la = ga[c] - ea;
            const float lb = gb[c] - eb;
            const float s_ = blend_ref(la, lb, m);
            float v = s_ + ee;
            if (v > 255.f)
                v = 255.f;
            else if (v < 0.f)
                v = 0.f;
            if (DENSE) {  // the finished mosaic is not read again by this sequence
                __builtin_nontemporal_store(px_store<OUT>(v), &out[(size_t)y * opitch + x + c * ops]);
                if (sizeof(OUT) == 4 && A.outs.q[pr]) A.outs.q[pr][(size_t)y * opitch + x + c * ops] = px_store<uint8_t>(v);
            } else
                out[(size_t)y * opitch + x + c * ops] = px_store<OUT>(v);
        }
    }
}

// one column per work-item over the whole level (xa == xb) -- levels too small or too irregular for k_collapse4
template <typename OUT, bool DENSE, bool MR = false>
__global__ __launch_bounds__(256) void k_collapse(CollapseArgs<OUT, DENSE> A, MaskRowsArg mr = MaskRowsArg{}) {
    const int x = blockIdx.x * blockDim.x + threadIdx.x, y0 = blockIdx.y * A.crows, pr = blockIdx.z;
    if (x >= (DENSE ? A.w : A.pitch)) return;
    collapse_cols1<OUT, DENSE, MR>(A, x, y0, min(y0 + A.crows, A.h), pr, mr);
}

// ---- the same collapse, four columns and ONE channel per work-item ------------------------------------------------
// k_collapse moves 4 bytes per lane and access and spends as many instructions on addresses and table look-ups as on
// the arithmetic.  Here a work-item owns FOUR adjacent columns x0..x0+3 (x0 a multiple of 4) of a strip of rows of ONE
// colour channel; the three wavefronts of a workgroup are the three channels of the same 256 columns.  The level's own
// planes (G_l, the mask, the index plane of a source-fused level 0, the output) are moved 16 bytes per lane, table
// entries are read once per strip, and -- the point of the channel split -- the x-interpolated source rows a work-item
// keeps are 2 x 3 planes x 4 columns = 24 registers instead of 72, so that 7-8 wavefronts per SIMD are resident instead
// of 2-3: the kernel is a chain of dependent loads per row (index -> gather -> arithmetic -> store) and lives on the
// number of such chains in flight.  The channels of a tile share its index and mask loads through the CU's L1.
// The up-sampling step is (sw-1)/(w-1) < 1/2, and away from the ends of a row the x taps follow one pattern:
// ix[x0..x0+3] = s, s+1, s+1, s+2 (columns 2m, 2m+1 interpolate between samples m-1, m and m, m+1 while the accumulated
// step stays within half a sample of x/2), so the taps of the four columns are fixed elements of ONE 4-byte-aligned
// 16-byte load at s.  The host knows the tables and hands this path only the column range [xa, xb) where every group of
// four has that pattern (6144 -> all but the first 256 columns); the other columns run collapse_cols1 in the same launch.
// Arithmetic and its order per sample are k_collapse's (lerp_ref, blend_ref, clamp).
typedef float f4u __attribute__((ext_vector_type(4), aligned(4)));  // 16-byte access at 4-byte alignment (dword-aligned dwordx4)

// Four finished samples of one row.  A dense canvas row starts at y * w samples: with a width that is not a multiple of 4
// (every canvas the reference builds) the float store is a 16-byte access at 4-byte alignment (f4u) and the unsigned char
// store falls back to four byte stores (words = false); words = true: one aligned 32-bit store.
template <typename OUT>
__device__ __forceinline__ void store4(OUT* p, const float v[4], bool words);
template <>
__device__ __forceinline__ void store4<float>(float* p, const float v[4], bool) {
    __builtin_nontemporal_store(f4u{v[0], v[1], v[2], v[3]}, reinterpret_cast<f4u*>(p));
}
template <>
__device__ __forceinline__ void store4<uint8_t>(uint8_t* p, const float v[4], bool words) {
    if (words) {
        const unsigned w = (unsigned)(uint8_t)(int)v[0] | ((unsigned)(uint8_t)(int)v[1] << 8) | ((unsigned)(uint8_t)(int)v[2] << 16) |
                           ((unsigned)(uint8_t)(int)v[3] << 24);
        __builtin_nontemporal_store(w, reinterpret_cast<unsigned*>(p));
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) __builtin_nontemporal_store((uint8_t)(int)v[j], p + j);
    }
}

// Four adjacent columns x0..x0+3 of one channel plane of a dense image placed on the canvas by an integer shift (the mosaic;
// canvas a of a dense pair with a zero shift): range tests per column once, then one row = one or four loads.
template <typename PX>
struct Shift4 {
    __amdgpu_buffer_rsrc_t rs;
    int iw, ih, oy;
    bool all, col[4];  // x part of the range test for this lane's columns
    unsigned x0b;      // byte offset of column x0 within an image row (valid when col[0])
    __device__ __forceinline__ Shift4(const PX* plane, int iw_, int ih_, int ox, int oy_, int x0, int w) : iw(iw_), ih(ih_), oy(oy_) {
        rs = plane_rsrc(plane, (size_t)iw_ * ih_);
        all = true;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const long long mx = (long long)(x0 + j) + ox;
            col[j] = x0 + j < w && mx >= 0 && mx < iw;
            all = all && col[j];
        }
        x0b = (unsigned)((long long)x0 + ox) * (unsigned)sizeof(PX);
    }
    // raw bits of canvas row y (loads only: nothing here waits for them)
    __device__ __forceinline__ void issue(int y, float b[4]) const {
        const long long my = (long long)y + oy;
        const bool row_ok = my >= 0 && my < ih;  // wave-uniform
        const unsigned rowb = (unsigned)my * (unsigned)iw * (unsigned)sizeof(PX);
        if (row_ok) {
            if (sizeof(PX) == 4 && __all(all)) {  // the common case: four consecutive floats, dword-aligned
                const u4 v = __builtin_bit_cast(u4, __builtin_amdgcn_raw_buffer_load_b128(rs, rowb + x0b, 0, 0));
#pragma unroll
                for (int j = 0; j < 4; ++j) b[j] = __uint_as_float(v[j]);
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j) b[j] = buf_raw<PX>(rs, col[j] ? rowb + x0b + (unsigned)(j * sizeof(PX)) : off_outside<PX>());
            }
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) b[j] = 0.f;  // raw 0 = sample 0 in either pixel type
        }
    }
};
struct NoShift4 {
    template <typename PX>
    __device__ __forceinline__ NoShift4(const PX*, int, int, int, int, int, int) {}
    __device__ __forceinline__ void issue(int, float[4]) const {}
};
template <typename PX, bool ON>
struct Shift4If {
    typedef NoShift4 type;
};
template <typename PX>
struct Shift4If<PX, true> {
    typedef Shift4<PX> type;
};
// level-0 samples of channel c at four adjacent canvas columns of a source-fused plan (what k_compose / k_load_canvases would
// have stored).  AD (PairArgs::a_dense, stitch_blend_*): canvas a is a dense image too, there is no index plane.
template <typename PX, bool AD>
struct SrcRow4 {
    __amdgpu_buffer_rsrc_t fr;
    Shift4<PX> mo;
    typename Shift4If<PX, AD>::type fa;  // canvas a of a dense pair
    __device__ __forceinline__ SrcRow4(const PairArgs<PX>& pa, int pr, int c, int x0, int w)
        : mo(pa.mosaic[pr] + c * ((size_t)pa.mw[pr] * pa.mh[pr]), pa.mw[pr], pa.mh[pr], pa.ox[pr], pa.oy[pr], x0, w),
          fa(pa.frame[pr] + c * ((size_t)pa.fw[pr] * pa.fh[pr]), pa.fw[pr], pa.fh[pr], 0, 0, x0, w) {
        const size_t fe = (size_t)pa.fw[pr] * pa.fh[pr];
        fr = plane_rsrc(pa.frame[pr] + c * fe, fe);
    }
    // raw bits of a[j], b[j] of canvas row y; idx = the four byte offsets k_src_index left (or "outside"; unused with AD)
    // SIDE (collapse_cols4): 1 leaves b as it is and reads only a, 2 leaves a as it is and reads only b
    template <int SIDE = 0>
    __device__ __forceinline__ void issue(const u4 idx, int y, float a[4], float b[4]) const {
        if constexpr (SIDE != 2) {
            if constexpr (AD)
                fa.issue(y, a);
            else {
#pragma unroll
                for (int j = 0; j < 4; ++j) a[j] = buf_raw<PX>(fr, idx[j]);  // "outside" is beyond the plane: reads 0
            }
        }
        if constexpr (SIDE != 1) {
#if STITCH_C4_ABLATE == 3 || STITCH_C4_ABLATE >= 8  // the mosaic is not read
            for (int j = 0; j < 4; ++j) b[j] = (float)y;
#else
            mo.issue(y, b);
#endif
        }
    }
    // raw bits -> the values k_compose / k_load_canvases would have stored
    __device__ __forceinline__ void finish(float a[4], float b[4]) const {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            a[j] = AD ? raw_to_px<PX>(a[j]) : warped_px<PX>(raw_to_px<PX>(a[j]));
            b[j] = raw_to_px<PX>(b[j]);
        }
    }
};
struct NoSrcRow4 {
    __device__ __forceinline__ NoSrcRow4(const NoPairArgs&, int, int, int, int) {}
    template <int SIDE = 0>
    __device__ __forceinline__ void issue(const u4, int, float[4], float[4]) const {}
    __device__ __forceinline__ void finish(float[4], float[4]) const {}
};
template <typename OUT, bool DENSE, bool AD>
struct SrcRow4Of {
    typedef NoSrcRow4 type;
};
template <typename OUT, bool AD>
struct SrcRow4Of<OUT, true, AD> {
    typedef SrcRow4<OUT, AD> type;
};

#ifndef STITCH_C4_WAVES
#define STITCH_C4_WAVES 7  // <= 72 registers: 7 wavefronts per SIMD (measured, level 0 of 8 config-2 pairs: 4 -> 2.39 ms, 6 -> 1.75, 7 -> 1.67, 8 with spills -> 1.70)
#endif
#ifndef STITCH_C4_PREFETCH
#define STITCH_C4_PREFETCH 0
#endif
#ifndef STITCH_C4_ABLATE
#define STITCH_C4_ABLATE 0  // 1..3: counter experiments (scripts/experiments/r4_run21.sh), results are wrong
#endif
#ifndef STITCH_C4_OPAQUE_ALPHA
#define STITCH_C4_OPAQUE_ALPHA 1
#endif
// channel c of columns x0..x0+3, rows [y0, y1) of pair pr
// GEN: the four columns' taps are ANY non-decreasing offsets o_j = ix[x0 + j] - ix[x0] (0 <= o_j <= 2: the up-sampling step is
// below 1/2, so four columns never span more than three source samples) instead of the fixed 0, 1, 1, 2 -- the same 16-byte
// load, the tap pair of a column selected per lane.  Odd level widths need it: their step (sw - 1) / (w - 1) drifts by a whole
// sample over the row, so the fixed pattern holds for well under half of the columns (1 792 of 4 421), and with it every column
// group but the last few of a row qualifies.  About 30 more selects per source row; even widths keep the fixed pattern.
//
// SIDE (a level 0 whose mask is the seam's step, chosen per workgroup by k_collapse4): 0 reads both images; 1: the step is 1 at every
// column of the workgroup, only image a is read; 2: the step is 0, only image b.  blend_ref(la, lb, m) with m = 1 is la and with
// m = 0 is lb for finite samples, except that a kept term of +-0 takes its sign from the dropped one -- which the sum with ee erases
// unless ee is -0.  A row in which some lane has a kept term of +-0 under an ee of -0 (both by bit pattern) is therefore redone with
// the dropped image loaded and the full arithmetic; that block sits behind the row's last wait and loads what it needs itself.
typedef __attribute__((address_space(3))) f4 lds_f4;
template <typename OUT, bool DENSE, bool AD, bool GEN, bool MR = false, int SIDE = 0>
__device__ __forceinline__ void collapse_cols4(const CollapseArgs<OUT, DENSE>& A, int c, int x0, int y0, int y1, int pr, float* sh, MaskRowsArg mr = MaskRowsArg{}) {
    const int pitch = A.pitch, sh_ = A.sh, spitch = A.spitch, opitch = A.opitch;
    const size_t ps = A.ps, sps = A.sps, ops = A.ops;
    const ExpandTab& tb = A.tb;
    const SeamDev* __restrict__ seam_l0 = A.seam_l0;
    const float* g = A.g_all + (size_t)collapse_slot(A, pr) * 7 * ps;
    // A.lockstep == 2 (levels >= 1): the mask samples of a row are read by channel 0 and handed to the other two channels through LDS
    const bool share = !DENSE && !seam_l0 && A.lockstep == 2;
    // the three planes of level l+1 this channel expands: a_c, b_c of G_{l+1} and channel c of E_{l+1}
    const float* sa = A.gn_all + ((size_t)pr * 7 + c) * sps;
    const float* sb = sa + 3 * sps;
    const float* se = A.en_all + ((size_t)pr * 3 + c) * sps;
    OUT* __restrict__ out = (DENSE ? A.outs.p[pr] : A.outs.p[0] + (size_t)pr * 3 * ops) + c * ops;
    uint8_t* __restrict__ out8 = DENSE && A.outs.q[pr] ? A.outs.q[pr] + c * ops : nullptr;
    const bool use_src = DENSE && A.use_src;
    // table entries of the four columns; their taps are samples s0 .. s0+3 of a source row
    const int s0 = tb.ix[x0];
    int o1 = 1, o2 = 1, o3 = 2;
    bool e1 = false, e2 = false, e3 = false;  // GEN: the column's tap sits on the source row's last sample (its second tap is the same sample, CImg.h:29648)
    if constexpr (GEN) {
        const int4 ix4 = *reinterpret_cast<const int4*>(tb.ix + x0);  // x0 is a multiple of 4: one 16-byte load
        o1 = ix4.y - ix4.x, o2 = ix4.z - ix4.x, o3 = ix4.w - ix4.x;
#ifndef STITCH_C4_NO_ENDTAP  // (defined only to prove that test_collapse_row_end_tap_even_widths sees a wrong second tap)
        e1 = ix4.y >= A.sw - 1, e2 = ix4.z >= A.sw - 1, e3 = ix4.w >= A.sw - 1;
#endif  // (column x0 itself never: a group spans three samples)
    }
    // G column flags, looked up once per work-item: its four columns lie in one tile column of this level, their taps s0 .. s0+3 in
    // one or two of level l+1 (g_cols).  A flagged plane is read from the zeros behind the level's last plane instead, every row from
    // the same 16 bytes; the loads themselves stay unconditional.
    // (STITCH_G_IGNORE_COARSER / STITCH_G_IGNORE_OWN: defined only in hand-check libraries, to prove that the stale-data tests see a
    // collapse that ignores the coarser level's flags / the level's own.  A mask of the code that ignores them: 1 (what -DNAME alone
    // gives) collapse_cols4, 2 collapse_cols1, 4 k_collapse_px, 7 all three; see HISTORY.md)
#if STITCH_G_IGNORE_COARSER & 1
    const bool za = false, zb = false;
#else
    // (of the plane that is read: a one-sided form looks the other one up only where it redoes a row)
    const bool za = SIDE != 2 && g_span_flag(A.gzn, A.gncn, pr * 7 + c, s0, s0 + 3), zb = SIDE != 1 && g_span_flag(A.gzn, A.gncn, pr * 7 + 3 + c, s0, s0 + 3);
#endif
#if STITCH_G_IGNORE_OWN & 1
    const bool zga = false, zgb = false;
#else
    const bool zga = !DENSE && g_span_flag(A.gz, A.gnc, pr * 7 + c, x0, x0), zgb = !DENSE && g_span_flag(A.gz, A.gnc, pr * 7 + 3 + c, x0, x0);
#endif
    const unsigned zsa = (unsigned)((size_t)A.zon - ((size_t)pr * 7 + c) * sps), zsb = (unsigned)((size_t)A.zon - ((size_t)pr * 7 + 3 + c) * sps);
    const size_t zg = (size_t)A.zo - (size_t)pr * 7 * ps;
    double axs[4];
    {
        const double2 a01 = *reinterpret_cast<const double2*>(tb.ax + x0), a23 = *reinterpret_cast<const double2*>(tb.ax + x0 + 2);
        axs[0] = a01.x, axs[1] = a01.y, axs[2] = a23.x, axs[3] = a23.y;
    }
    // x pass of the 16 bytes of one plane's source row
    auto xl4 = [&](const f4 v, float X[4]) {
        if constexpr (GEN) {
            const float x_ = v.x, y_ = v.y, z_ = v.z, w_ = v.w;
            X[0] = lerp_ref(axs[0], x_, y_);
            const float a1 = o1 ? y_ : x_, a2 = o2 == 0 ? x_ : o2 == 1 ? y_ : z_, a3 = o3 == 0 ? x_ : o3 == 1 ? y_ : z_;
            X[1] = lerp_ref(axs[1], a1, e1 ? a1 : o1 ? z_ : y_);
            X[2] = lerp_ref(axs[2], a2, e2 ? a2 : o2 == 0 ? y_ : o2 == 1 ? z_ : w_);
            X[3] = lerp_ref(axs[3], a3, e3 ? a3 : o3 == 0 ? y_ : o3 == 1 ? z_ : w_);
        } else {
            X[0] = lerp_ref(axs[0], v.x, v.y);
            X[1] = lerp_ref(axs[1], v.y, v.z);
            X[2] = lerp_ref(axs[2], v.y, v.z);
            X[3] = lerp_ref(axs[3], v.z, v.w);
        }
    };
    // x pass of one source row for the three planes (a one-sided form: for the two it reads; X[q] of the other is never touched)
    auto xrow = [&](int row, float X[3][4]) {
        const unsigned o = (unsigned)row * (unsigned)spitch + (unsigned)s0;
#if STITCH_C4_ABLATE == 1 || STITCH_C4_ABLATE >= 8  // counter experiments only (wrong results): the coarser level is not read
        const f4 v[3] = {f4{0.f, 0.f, 0.f, (float)o}, f4{0.f, 0.f, 0.f, 1.f}, f4{0.f, 0.f, 0.f, 2.f}};
#else
        const f4 v[3] = {SIDE != 2 ? *reinterpret_cast<const f4u*>(sa + (za ? zsa : o)) : f4{0.f, 0.f, 0.f, 0.f},
                         SIDE != 1 ? *reinterpret_cast<const f4u*>(sb + (zb ? zsb : o)) : f4{0.f, 0.f, 0.f, 0.f}, *reinterpret_cast<const f4u*>(se + o)};
#endif
#if STITCH_C4_OPAQUE_ALPHA
        // registers are what bounds the number of resident wavefronts here: keep the four alphas, not also the four
        // (1 - alpha) the compiler would hoist out of the row loop (recomputed per source row: four v_add_f64)
#pragma unroll
        for (int j = 0; j < 4; ++j) asm volatile("" : "+v"(axs[j]));
#endif
#pragma unroll
        for (int q = 0; q < 3; ++q) {
            if ((q == 0 && SIDE == 2) || (q == 1 && SIDE == 1)) continue;
            xl4(v[q], X[q]);
        }
    };
    // X1 = X2 and back, of the planes that are read
    auto xcopy = [&](float D[3][4], const float S[3][4]) {
#pragma unroll
        for (int q = 0; q < 3; ++q) {
            if ((q == 0 && SIDE == 2) || (q == 1 && SIDE == 1)) continue;
#pragma unroll
            for (int j = 0; j < 4; ++j) D[q][j] = S[q][j];
        }
    };
    float X1[3][4], X2[3][4];
    int cur1 = -1, cur2 = -1;
    float m4[4] = {0.f, 0.f, 0.f, 0.f};
    if (seam_l0) {  // level 0: the mask is the step itself
        const SeamDev sd = seam_l0[pr];
#pragma unroll
        for (int j = 0; j < 4; ++j) m4[j] = mask_step(sd, x0 + j);
    }
    const typename SrcRow4Of<OUT, DENSE, AD>::type src(A.pa, pr, c, x0, A.w);
    // the level's own samples of one row, as raw bits: two planes (or the gathers of a source-fused level 0) + the mask
    bool mrow = false;  // MR: row-repeat flag of the mask tile a row lies in (the four columns lie in one tile column)
    auto row_issue = [&](int y, float ga[4], float gb[4], f4& vm) {
        const unsigned o = (unsigned)y * (unsigned)pitch + (unsigned)x0;
        if constexpr (MR)
            if (y == y0 || (y & 63) == 0) mrow = collapse_mask_row(mr, pr, x0, y);
        const unsigned om = MR && mrow ? (unsigned)x0 : o;
        if (use_src)
#if STITCH_C4_ABLATE == 2  // the index plane is not read (every lane gathers element 0 .. 3)
            src.issue(u4{0u, 4u, 8u, 12u}, y, ga, gb);
#elif STITCH_C4_ABLATE >= 6  // 6: only channel 0 reads the index plane, 7: nobody; the others form what it holds under the
            // "aligned" map of exp_collapse_fetch.py (frame sample (x - 2048, y) of a 4096-wide frame) -- the same gathers
        {
            const unsigned e = ((unsigned)y * 4096u + (unsigned)(x0 - 2048)) * 4u;
            const u4 calc = x0 >= 2048 ? u4{e, e + 4u, e + 8u, e + 12u} : u4{0xfffffff0u, 0xfffffff0u, 0xfffffff0u, 0xfffffff0u};
            src.issue(c == 0 && STITCH_C4_ABLATE == 6 ? *reinterpret_cast<const u4*>(g + o) : STITCH_C4_ABLATE >= 8 ? u4{0u, 4u, 8u, 12u} : calc, y, ga, gb);
        }
#else
        {
            u4 idx = {0u, 0u, 0u, 0u};
            if constexpr (!AD && SIDE != 2) idx = *reinterpret_cast<const u4*>(g + o);  // the index word is image a's
            src.template issue<SIDE>(idx, y, ga, gb);
        }
#endif
        else {
            if constexpr (SIDE != 2) {
                const f4 va = *reinterpret_cast<const f4*>(g + (zga ? zg : o + c * ps));
#pragma unroll
                for (int j = 0; j < 4; ++j) ga[j] = va[j];
            }
            if constexpr (SIDE != 1) {
                const f4 vb = *reinterpret_cast<const f4*>(g + (zgb ? zg : o + (3 + c) * ps));
#pragma unroll
                for (int j = 0; j < 4; ++j) gb[j] = vb[j];
            }
        }
        if (share) {
            if (c == 0) vm = *reinterpret_cast<const f4*>(g + om + 6 * ps);
        } else
#if STITCH_C4_ABLATE == 11  // only channel 0 reads the mask plane
        if (!seam_l0) vm = c == 0 ? *reinterpret_cast<const f4*>(g + o + 6 * ps) : f4{0.5f, 0.5f, 0.5f, 0.5f};
#elif STITCH_C4_ABLATE == 12  // nobody reads the mask plane
        if (!seam_l0) vm = f4{0.5f, 0.5f, 0.5f, (float)y};
#else
        if (!seam_l0) vm = *reinterpret_cast<const f4*>(g + om + 6 * ps);
#endif
    };
    float ga[4] = {0.f, 0.f, 0.f, 0.f}, gb[4] = {0.f, 0.f, 0.f, 0.f};  // (raw 0 = sample 0: what a one-sided form leaves of the other image)
    f4 vm = {0.f, 0.f, 0.f, 0.f};
#if STITCH_C4_PREFETCH
    // the row's loads are issued one row ahead of their use
    float gan[4], gbn[4];
    f4 vmn = {0.f, 0.f, 0.f, 0.f};
    row_issue(y0, gan, gbn, vmn);
#endif
    for (int y = y0; y < y1; ++y) {
        // A/B switch (STITCH_C4_LOCKSTEP=1): the channels of a workgroup read the same index / mask samples; keeping the three
        // wavefronts within a row of each other with a bare s_barrier was tried against the kernel's over-fetch and changes nothing
        // (FETCH_SIZE -0.7 %): the shared plane is served by the caches as it is.
        if (A.lockstep == 1) __builtin_amdgcn_s_barrier();
        const int iy = tb.iy[y], iy2 = iy < sh_ - 1 ? iy + 1 : iy;
        const double ay = tb.ay[y];
        if (iy != cur1) {
            if (iy == cur2)
                xcopy(X1, X2);
            else
                xrow(iy, X1);
            cur1 = iy;
        }
        if (iy2 != cur2) {
            if (iy2 == cur1)
                xcopy(X2, X1);
            else
                xrow(iy2, X2);
            cur2 = iy2;
        }
#if STITCH_C4_PREFETCH
#pragma unroll
        for (int j = 0; j < 4; ++j) ga[j] = gan[j], gb[j] = gbn[j];
        vm = vmn;
        if (y + 1 < y1) row_issue(y + 1, gan, gbn, vmn);  // behind the x pass: its loads are waited for at once
#else
        row_issue(y, ga, gb, vm);
#endif
        if (share) {  // two slots: channel 0 refills a slot only after the barrier of the row in between, which the others reach having read it
            lds_f4* slot = (lds_f4*)sh + (y & 1) * WAVE + (threadIdx.x & 63);
            if (c == 0) *slot = vm;
            asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
            vm = *slot;
        }
        if (use_src) src.finish(ga, gb);
        if (!seam_l0) {
#pragma unroll
            for (int j = 0; j < 4; ++j) m4[j] = vm[j];
        }
        float v4[4];
        if constexpr (SIDE == 0) {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const float ea = lerp_ref(ay, X1[0][j], X2[0][j]);
                const float eb = lerp_ref(ay, X1[1][j], X2[1][j]);
                const float ee = lerp_ref(ay, X1[2][j], X2[2][j]);
                const float la = ga[j] - ea;
                const float lb = gb[j] - eb;
                const float s_ = blend_ref(la, lb, m4[j]);
                float v = s_ + ee;
                if (v > 255.f)
                    v = 255.f;
                else if (v < 0.f)
                    v = 0.f;
                v4[j] = v;
            }
        } else {
            constexpr int K = SIDE == 1 ? 0 : 1;  // the plane that is kept
            const float* gk = SIDE == 1 ? ga : gb;
            bool redo = false;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const float ek = lerp_ref(ay, X1[K][j], X2[K][j]);
                const float ee = lerp_ref(ay, X1[2][j], X2[2][j]);
                const float lk = gk[j] - ek;  // blend_ref's value, but for the sign of a zero
                float v = lk + ee;
                redo = redo || ((__float_as_uint(lk) << 1) == 0u && __float_as_uint(ee) == 0x80000000u);
                if (v > 255.f)
                    v = 255.f;
                else if (v < 0.f)
                    v = 0.f;
                v4[j] = v;
            }
#ifndef STITCH_C4_NO_SIDE_REDO  // (defined only to prove that the signed-zero probe of stitch_dev_check_collapse_sides sees the missing sign)
            if (__builtin_expect(__any(redo), 0)) {
                // the row again with the dropped image: its sample, its two source rows of G_{l+1}, the full blend.  Everything of
                // that image is worked out here, from a column number the compiler cannot move out of the row loop: the main loop
                // keeps no register for it.
                int xr = x0;
                asm volatile("" : "+v"(xr));
                constexpr int D = 1 - K;
                const float* sd_ = D == 0 ? sa : sb;
                const unsigned zsd = D == 0 ? zsa : zsb;
#if STITCH_G_IGNORE_COARSER & 1
                const bool zd = false;
#else
                const bool zd = g_span_flag(A.gzn, A.gncn, pr * 7 + 3 * D + c, tb.ix[xr], tb.ix[xr] + 3);
#endif
                float gd[4] = {0.f, 0.f, 0.f, 0.f}, gu[4] = {0.f, 0.f, 0.f, 0.f};
                const unsigned o = (unsigned)y * (unsigned)pitch + (unsigned)xr;
                if (use_src) {
                    const typename SrcRow4Of<OUT, DENSE, AD>::type srd(A.pa, pr, c, xr, A.w);
                    u4 idx = {0u, 0u, 0u, 0u};
                    if constexpr (!AD && D == 0) idx = *reinterpret_cast<const u4*>(g + o);
                    if constexpr (D == 0) {
                        srd.template issue<1>(idx, y, gd, gu);
                        srd.finish(gd, gu);
                    } else {
                        srd.template issue<2>(idx, y, gu, gd);
                        srd.finish(gu, gd);
                    }
                } else {
                    const f4 vd = *reinterpret_cast<const f4*>(g + o + (3 * D + c) * ps);
#pragma unroll
                    for (int j = 0; j < 4; ++j) gd[j] = vd[j];
                }
                float D1[4], D2[4];
                const unsigned sr = (unsigned)tb.ix[xr];  // (= s0)
                xl4(*reinterpret_cast<const f4u*>(sd_ + (zd ? zsd : (unsigned)iy * (unsigned)spitch + sr)), D1);
                xl4(*reinterpret_cast<const f4u*>(sd_ + (zd ? zsd : (unsigned)iy2 * (unsigned)spitch + sr)), D2);
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const float ek = lerp_ref(ay, X1[K][j], X2[K][j]);
                    const float ed = lerp_ref(ay, D1[j], D2[j]);
                    const float ee = lerp_ref(ay, X1[2][j], X2[2][j]);
                    const float lk = gk[j] - ek;
                    const float ld = gd[j] - ed;
                    const float s_ = SIDE == 1 ? blend_ref(lk, ld, m4[j]) : blend_ref(ld, lk, m4[j]);
                    float v = s_ + ee;
                    if (v > 255.f)
                        v = 255.f;
                    else if (v < 0.f)
                        v = 0.f;
                    v4[j] = v;
                }
            }
#endif
        }
#if STITCH_C4_ABLATE == 4  // nothing is stored (unless a sample is a NaN: the compiler must keep the arithmetic)
        if (!(v4[0] != v4[0] || v4[3] != v4[3])) continue;
#endif
        if constexpr (DENSE)
        {
#if STITCH_C4_ABLATE == 5  // plain stores instead of non-temporal ones
            *reinterpret_cast<f4u*>(&out[(size_t)y * opitch + x0]) = f4u{v4[0], v4[1], v4[2], v4[3]};
            continue;
#endif
            store4<OUT>(&out[(size_t)y * opitch + x0], v4, A.u8_words != 0);
            if (sizeof(OUT) == 4 && out8) store4<uint8_t>(&out8[(size_t)y * opitch + x0], v4, A.u8_words != 0);
        }
        else
            *reinterpret_cast<f4*>(&out[(size_t)y * opitch + x0]) = f4{v4[0], v4[1], v4[2], v4[3]};
    }
}

// One launch per level, workgroups of three wavefronts: workgroups [0, nb4) of a strip row do columns [xa, xb), four
// columns per work-item, one channel per wavefront; the remaining workgroups do the other columns one per work-item
// (all channels), each over an eighth of the strip's rows (that part is small, and a work-item's rows are a serial
// chain of load latencies: short chains keep it off the launch's critical path).
constexpr int C4_SUB = 8, C4_THREADS = 3 * WAVE;
// four-column blocks per strip in the launch: with a block order, strips of eight blocks and more are padded to a multiple of 8
// (the extra workgroups return at once) so that every block of a strip is renumbered; narrower levels are left as they are
__host__ __device__ inline int c4_padded_blocks(int nb4, int swizzle) { return swizzle && nb4 >= 8 ? (nb4 + 7) & ~7 : nb4; }
// A level 0 whose mask is the seam's step (A.seam_l0) takes, per workgroup, the form of collapse_cols4 that reads only the image the
// step selects: the step is monotone in x, so equal values at the block's first and last column (c4_block_side, stitch_call_form.h:
// the rule stitch_plan_collapse_sides counts by) mean one value over the block.  The record is read on the device, in stream order:
// a captured call decides again on every replay.  -DSTITCH_NO_C4_SIDES: always both images (A/B libraries).
template <typename OUT, bool DENSE, bool AD = false, bool GEN = false, bool MR = false>
__global__ __launch_bounds__(C4_THREADS, STITCH_C4_WAVES) void k_collapse4(CollapseArgs<OUT, DENSE> A, int nb4, int ncb, MaskRowsArg mr = MaskRowsArg{}) {
    const int pr = blockIdx.z;
    __shared__ __attribute__((aligned(16))) float c4_sh[2 * WAVE * 4];
    const int nb4p = c4_padded_blocks(nb4, A.swizzle);
    if ((int)blockIdx.x < nb4p) {
        const int c = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);  // the channel is wave-uniform: plane bases stay scalar
        // Workgroups go to the 8 XCDs round-robin in launch order, each XCD with its own L2, and neighbouring column blocks share
        // the source lines their tap windows straddle: a block's taps span samples 128 b - 1 .. 128 b + 128 of level l+1, SIX
        // 128-byte lines where it owns four (round 4's counters: every read request of these kernels is a full line, 916 MB read
        // per pair at level 0 against 729 owned).  The first nb8 = nb4 rounded down to a multiple of 8 blocks of a strip are
        // therefore renumbered: within a group of eight strips every XCD gets ONE WHOLE STRIP (its blocks dispatched close together,
        // so the shared lines are fetched into that L2 once); strips past the last full group get contiguous runs of nb8 / 8 blocks.
        int blk = blockIdx.x, strip = blockIdx.y;
        const int nb8 = nb4p & ~7;
        const int S8 = (int)gridDim.y & ~7;
        if (A.swizzle >= 2 && blk < nb8 && (int)blockIdx.y < S8) {
            // swizzle 2: every XCD walks its OWN run of S8 / 8 adjacent strips top to bottom, whole strips one after the other: the
            // rows two strips share (the next level's halo rows, the slanted rows of a warped frame) meet in one L2 as well
            const unsigned first = gridDim.x * (blockIdx.y + gridDim.y * blockIdx.z);
            const int xcd = (int)((first + (unsigned)blk) & 7u), t = (int)blockIdx.y * (nb8 >> 3) + (blk >> 3);  // this XCD's t-th block of the pair
            strip = xcd * (S8 >> 3) + t / nb8;
            blk = t % nb8;
        } else if (A.swizzle && blk < nb8) {
            const unsigned first = gridDim.x * (blockIdx.y + gridDim.y * blockIdx.z);  // launch-order id of this strip's block 0
            const int xcd = (int)((first + (unsigned)blk) & 7u), k = blk >> 3, K = nb8 >> 3, s0 = (int)blockIdx.y & ~7;
            if (s0 + 8 <= (int)gridDim.y) {
                strip = s0 + xcd;
                blk = ((int)blockIdx.y - s0) * K + k;
            } else
                blk = xcd * K + k;
        }
        const int y0 = strip * A.crows, y1 = min(y0 + A.crows, A.h);
        const int x0 = A.xa + (blk * WAVE + (threadIdx.x & 63)) * 4;
        if (blk < nb4 && x0 < A.xb) {
            int side = 0;
#ifndef STITCH_NO_C4_SIDES
            if constexpr (DENSE) {
                if (A.seam_l0) {
                    const SeamDev& sd = A.seam_l0[pr];
                    const int xf = A.xa + blk * (4 * WAVE);
                    side = __builtin_amdgcn_readfirstlane(c4_block_side(sd.branch, sd.start, sd.thr, xf, min(xf + 4 * WAVE - 1, A.xb - 1)));
#ifdef STITCH_C4_WRONG_SIDE  // (defined only in a hand-check library, to prove that the tests see a one-sided block that reads the other image)
                    side = side ? 3 - side : 0;
#endif
                }
            }
#endif
            if constexpr (DENSE) {
                if (side == 1)
                    collapse_cols4<OUT, DENSE, AD, GEN, MR, 1>(A, c, x0, y0, y1, pr, c4_sh, mr);
                else if (side == 2)
                    collapse_cols4<OUT, DENSE, AD, GEN, MR, 2>(A, c, x0, y0, y1, pr, c4_sh, mr);
                else
                    collapse_cols4<OUT, DENSE, AD, GEN, MR, 0>(A, c, x0, y0, y1, pr, c4_sh, mr);
            } else
                collapse_cols4<OUT, DENSE, AD, GEN, MR>(A, c, x0, y0, y1, pr, c4_sh, mr);
        }
    } else {
        const int y0 = blockIdx.y * A.crows, y1 = min(y0 + A.crows, A.h);
        const int r = blockIdx.x - nb4p, cb = r % ncb, sub = r / ncb, rows = (A.crows + C4_SUB - 1) / C4_SUB;
        int x = cb * C4_THREADS + threadIdx.x;
        if (x >= A.xa) x += A.xb - A.xa;
        const int ya = y0 + sub * rows, yb = min(ya + rows, y1);
#if STITCH_C4_ABLATE == 9 || STITCH_C4_ABLATE == 10  // the one-column-per-work-item part does nothing
        if (A.h < 0)
#endif
        if (x < (DENSE ? A.w : A.pitch) && ya < yb) collapse_cols1<OUT, DENSE, MR>(A, x, ya, yb, pr, mr);
    }
}

// The collapse of one level >= 1 with ONE output pixel (three channels) per work-item and no strip: twice the double-precision
// work of k_collapse (no re-use of x-interpolated source rows), but a work-item's chain is two rounds of loads instead of a
// strip's worth of dependent table look-ups -- for the middle levels of a LONE pair (too small for k_collapse4, too large for
// k_coarse), where a launch's time is that chain: 15 -> 7 us per level.  Same expand_at / blend_ref arithmetic.
template <bool MR = false>
__global__ __launch_bounds__(256) void k_collapse_px(CollapseArgs<float, false> A, MaskRowsArg mr = MaskRowsArg{}) {
    const int x = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y, pr = blockIdx.z;
    if (x >= A.pitch) return;
    const float* g = A.g_all + (size_t)pr * 7 * A.ps;
    const float* gn = A.gn_all + (size_t)pr * 7 * A.sps;
    const float* en = A.en_all + (size_t)pr * 3 * A.sps;
    float* e = A.outs.p[0] + (size_t)pr * 3 * A.ops;
    const size_t i = (size_t)y * A.pitch + x;
    if (x >= A.w) {
#pragma unroll
        for (int c = 0; c < 3; ++c) e[i + c * A.ops] = 0.f;
        return;
    }
    const ExpandPos ep = expand_pos(A.tb, x, y, A.sw, A.sh, A.spitch);
    const int ix = A.tb.ix[x], ix2 = ix < A.sw - 1 ? ix + 1 : ix;  // the two x taps (expand_pos)
    const float m = g[(MR && collapse_mask_row(mr, pr, x, y) ? (size_t)x : i) + 6 * A.ps];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        // G column flags: a flagged sample is +0 and is not loaded (an interpolation between zeros is +0: the weights are in [0, 1])
#if STITCH_G_IGNORE_COARSER & 4  // (the two macros: see collapse_cols4)
        const bool za = false, zb = false;
#else
        const bool za = g_span_flag(A.gzn, A.gncn, pr * 7 + c, ix, ix2), zb = g_span_flag(A.gzn, A.gncn, pr * 7 + 3 + c, ix, ix2);
#endif
#if STITCH_G_IGNORE_OWN & 4
        const bool zga = false, zgb = false;
#else
        const bool zga = g_span_flag(A.gz, A.gnc, pr * 7 + c, x, x), zgb = g_span_flag(A.gz, A.gnc, pr * 7 + 3 + c, x, x);
#endif
        const float ea = za ? 0.f : expand_at(gn + c * A.sps, ep), eb = zb ? 0.f : expand_at(gn + (3 + c) * A.sps, ep), ee = expand_at(en + c * A.sps, ep);
        const float la = (zga ? 0.f : g[i + c * A.ps]) - ea;
        const float lb = (zgb ? 0.f : g[i + (3 + c) * A.ps]) - eb;
        const float s_ = blend_ref(la, lb, m);
        float v = s_ + ee;
        if (v > 255.f)
            v = 255.f;
        else if (v < 0.f)
            v = 0.f;
        e[i + c * A.ops] = v;
    }
}

// single-level pyramid (max side 2 or 3): the result is the top-level blend itself, cast to the output type
template <typename OUT>
__global__ void k_emit_top(const float* __restrict__ e_all, int w, int h, int pitch, size_t ps, OutPtrs<OUT> outs) {
    const int x = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y;
    if (x >= w) return;
    const float* e = e_all + (size_t)blockIdx.z * 3 * ps;
    OUT* __restrict__ out = outs.p[blockIdx.z];
    uint8_t* __restrict__ out8 = sizeof(OUT) == 4 ? outs.q[blockIdx.z] : nullptr;  // a float mosaic's unsigned char copy (out_u8)
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float v = e[(size_t)y * pitch + x + c * ps];
        out[(size_t)c * w * h + (size_t)y * w + x] = px_store<OUT>(v);
        if (out8) out8[(size_t)c * w * h + (size_t)y * w + x] = px_store<uint8_t>(v);
    }
}
