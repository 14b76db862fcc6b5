// Part of stitch_kernels.hpp (included there, inside namespace sk): the cylindrical projection with the source rows of an output
// tile staged in LDS (P1, P2; k_project in k_geometry.inc is the untiled form).
// The same projection for portrait / square frames (the reference's `flag == 0` branch), source rows tiled into LDS.
// k_project is bound by the vector L1: twelve tap loads per pixel, each touching its own cache line(s).  Here a workgroup
// owns an output tile of TW columns x TH rows.  The cylinder only stretches (1/k = sqrt(r^2 + dx^2)/r >= 1 and grows with
// |dx|), so the source samples of the tile lie in a box that its corner columns and rows bound: columns floor(u(x_first))
// .. ceil(u(x_last)), rows between the extremes of v over the corners.  The workgroup fetches that box once with coalesced
// 16-byte loads into LDS (three channels), then every work-item -- one output column, TH / (256 / TW) rows, so that the
// double-precision k of its column is evaluated once -- takes its four taps per channel from LDS.  Arithmetic per pixel and
// its order are k_project's / bilinear3's.  The host checks that the largest box of the frame fits the LDS budget.
// (Measured at 4096 x 4096: 0.069 ms u8 / 0.113 ms f32 against k_project's 0.107 / 0.146.  Tried and slower: four columns per
// work-item without LDS, 0.134 / 0.183 -- more cache lines per load instruction; the column terms from a table written by a
// kernel of its own, 0.073 / 0.134 -- the extra launch costs more than the redundant double-precision work it removes.)
template <typename PX>
struct Px4;
template <>
struct Px4<uint8_t> {
    typedef unsigned type;
    static __device__ __forceinline__ type pack(const uint8_t v[4]) { return (unsigned)v[0] | ((unsigned)v[1] << 8) | ((unsigned)v[2] << 16) | ((unsigned)v[3] << 24); }
};
template <>
struct Px4<float> {
    typedef f4 type;
    static __device__ __forceinline__ type pack(const float v[4]) { return f4{v[0], v[1], v[2], v[3]}; }
};
// The staged box is read through a pointer that is LDS by TYPE: with a generic pointer the compiler merged the (never taken)
// global fallback and the LDS taps into flat_load_ubyte / flat_load_dword -- twelve flat loads per pixel instead of ds_read.
#ifndef PJ_PACKED
#define PJ_PACKED 0
#endif
template <typename PX>
using lds_ptr = const __attribute__((address_space(3))) PX*;
struct ProjCol {
    float k, u;
};
struct ProjRow {  // a row's terms of the landscape branch: k, u and the refined reciprocal of k (pj_rcp)
    float k, u, rc, pad;
};
__device__ __forceinline__ ProjCol proj_col(int x, int w, float r) {  // Projection.cpp:33-37 for one column
    const float dst_x = (float)(x - w / 2);
    const double rd = (double)r, dx = (double)dst_x;
    ProjCol c;
    c.k = (float)(rd / sqrt(rd * rd + dx * dx));
    c.u = dst_x / c.k + (float)(w / 2);
    return c;
}
__device__ __forceinline__ float proj_v(int y, int h, float k) { return (float)(y - h / 2) / k + (float)(h / 2); }
// n / k as the compiler's own expansion of a float division computes it (v_rcp_f32, one refinement of the reciprocal, two of
// the quotient), without v_div_scale / v_div_fixup: those leave operands of this range -- |n| an integer below 2^24, k in
// (2^-20, 1] -- untouched, so the quotient is the correctly rounded one, bit for bit.  The reciprocal's part depends on k
// alone and is hoisted out of the pixel loop.
// Two pixels are carried side by side ({A, B}: independent chains for the scheduler to interleave) as plain scalars: packed
// f32 VALU instructions (v_pk_mul_f32 / v_pk_add_f32 / v_pk_fma_f32) issue slower on gfx950 than the two scalar ones they
// replace (measured here: the same loop on ext_vector_type(2) pairs gained nothing from halving its instruction count).
#if PJ_PACKED
typedef float f2v __attribute__((ext_vector_type(2)));
#else
struct f2v {
    float x, y;
};
__device__ __forceinline__ f2v operator*(f2v a, f2v b) { return f2v{a.x * b.x, a.y * b.y}; }
__device__ __forceinline__ f2v operator*(float a, f2v b) { return f2v{a * b.x, a * b.y}; }
__device__ __forceinline__ f2v operator+(f2v a, f2v b) { return f2v{a.x + b.x, a.y + b.y}; }
__device__ __forceinline__ f2v operator+(f2v a, float b) { return f2v{a.x + b, a.y + b}; }
__device__ __forceinline__ f2v operator-(f2v a, f2v b) { return f2v{a.x - b.x, a.y - b.y}; }
__device__ __forceinline__ f2v operator-(float a, f2v b) { return f2v{a - b.x, a - b.y}; }
#endif
__device__ __forceinline__ float pj_rcp(float k) {
    const float rc = __builtin_amdgcn_rcpf(k);
    return __builtin_fmaf(__builtin_fmaf(-k, rc, 1.0f), rc, rc);
}
__device__ __forceinline__ float pj_div(float n, float k, float rc) {
    const float q0 = n * rc;
    const float q1 = __builtin_fmaf(__builtin_fmaf(-k, q0, n), rc, q0);
    return __builtin_fmaf(__builtin_fmaf(-k, q1, n), rc, q1);
}
#if PJ_PACKED
__device__ __forceinline__ f2v pj_div2(f2v n, f2v k, f2v rc) {
    const f2v q0 = n * rc;
    const f2v q1 = __builtin_elementwise_fma(__builtin_elementwise_fma(-k, q0, n), rc, q0);
    return __builtin_elementwise_fma(__builtin_elementwise_fma(-k, q1, n), rc, q1);
}
#else
__device__ __forceinline__ f2v pj_div2(f2v n, f2v k, f2v rc) { return f2v{pj_div(n.x, k.x, rc.x), pj_div(n.y, k.y, rc.y)}; }
#endif
constexpr int PJ_CHUNK = 16;  // bytes per staging access
// output tile per workgroup: columns x rows, per pixel type (256 work-items: TH / (256 / TW) rows per work-item)
#ifndef STITCH_PJ_TW_U8
#define STITCH_PJ_TW_U8 128
#endif
#ifndef STITCH_PJ_TH_U8
#define STITCH_PJ_TH_U8 16
#endif
#ifndef STITCH_PJ_TW_F32
#define STITCH_PJ_TW_F32 64
#endif
#ifndef STITCH_PJ_TH_F32
#define STITCH_PJ_TH_F32 32
#endif
constexpr int PJ_TW_U8 = STITCH_PJ_TW_U8, PJ_TH_U8 = STITCH_PJ_TH_U8, PJ_TW_F32 = STITCH_PJ_TW_F32, PJ_TH_F32 = STITCH_PJ_TH_F32;
// Staging of a tile's source box (three channels, rows r0 .. r0+nrow-1, columns c0a .. c0a+ncol-1) into LDS with 16-byte
// loads: 32 lanes across a row's chunks, 8 rows per pass (no division by the run-time chunk count).  All loads of a work-item
// are issued before the first LDS store -- a loop of load -> store iterations put up to nine HBM round trips of a workgroup
// one behind the other, which was half of the float kernel's time (0.134 -> 0.067 ms at 4096 x 4096 with the staging ablated).
// A chunk that is not this lane's reads at an offset beyond the buffer: no traffic, the value is dropped.
// PJ_MAXP row passes are held in registers (boxes of up to 8 PJ_MAXP rows and 32 chunks per row; larger ones loop): the box of a
// TH-row tile has about 1.1 TH + 3 rows.
template <typename PX, int PJ_MAXP>
__device__ __forceinline__ void pj_stage(const PX* __restrict__ src, size_t pl, int w, int r0, int nrow, int c0a, int ncol, uint8_t* smem) {
    constexpr int CPX = PJ_CHUNK / (int)sizeof(PX);
    const __amdgpu_buffer_rsrc_t rs = plane_rsrc(src, 3 * pl);  // a chunk that runs past the last row reads 0
    const int cpr = ncol / CPX, lc = threadIdx.x & 31, lr = threadIdx.x >> 5;
    if (cpr <= 32 && nrow <= 8 * PJ_MAXP) {
        u4 v[3][PJ_MAXP];
#pragma unroll
        for (int c = 0; c < 3; ++c)
#pragma unroll
            for (int p = 0; p < PJ_MAXP; ++p) {
                const int rr = lr + 8 * p;
                const bool mine = rr < nrow && lc < cpr;
                const unsigned off = mine ? (unsigned)((c * pl + (size_t)(r0 + rr) * w + c0a + lc * CPX) * sizeof(PX)) : 0xfffffff0u;
                v[c][p] = __builtin_bit_cast(u4, __builtin_amdgcn_raw_buffer_load_b128(rs, off, 0, 0));
            }
#pragma unroll
        for (int c = 0; c < 3; ++c)
#pragma unroll
            for (int p = 0; p < PJ_MAXP; ++p) {
                const int rr = lr + 8 * p;
                if (rr < nrow && lc < cpr) *reinterpret_cast<u4*>(smem + ((size_t)(c * nrow + rr) * ncol + lc * CPX) * sizeof(PX)) = v[c][p];
            }
        return;
    }
    for (int c = 0; c < 3; ++c)
        for (int rr = lr; rr < nrow; rr += 8)
            for (int cc = lc; cc < cpr; cc += 32) {
                const unsigned off = (unsigned)((c * pl + (size_t)(r0 + rr) * w + c0a + cc * CPX) * sizeof(PX));
                *reinterpret_cast<u4*>(smem + ((size_t)(c * nrow + rr) * ncol + cc * CPX) * sizeof(PX)) =
                    __builtin_bit_cast(u4, __builtin_amdgcn_raw_buffer_load_b128(rs, off, 0, 0));
            }
}

// unsigned char frames: the box is staged PIXEL-INTERLEAVED, one dword per pixel (R | G << 8 | B << 16): the taps (xf, xf + 1) of
// a source row are one ds_read2_b32 for all three channels instead of six ds_read_u8 -- the tiled kernel was bound by the
// number of LDS instructions (twelve byte reads per pixel), not by VALU work or HBM.  A work-item loads the same 16 pixels
// of the three planes (16-byte loads) and interleaves them with v_perm_b32; 16 lanes across a row's chunks, 16 rows per pass,
// two passes' loads in flight.
__device__ __forceinline__ unsigned pj_rgbx(unsigned R, unsigned G, unsigned B, unsigned k) {  // byte k of each -> one pixel
    const unsigned t = __builtin_amdgcn_perm(G, R, 0x0c0c0000u | ((4u + k) << 8) | k);
    return __builtin_amdgcn_perm(B, t, 0x0c000100u | ((4u + k) << 16));
}
__device__ __forceinline__ void pj_stage_rgbx(const uint8_t* __restrict__ src, size_t pl, int w, int r0, int nrow, int c0a, int ncol, uint8_t* smem) {
    const __amdgpu_buffer_rsrc_t rs = plane_rsrc(src, 3 * pl);  // a chunk that runs past the last row reads 0
    const int cpr = ncol >> 4, lc = threadIdx.x & 15, lr = threadIdx.x >> 4;
    for (int rb = 0; rb < nrow; rb += 32)
        for (int cc = lc; cc < cpr; cc += 16) {
            u4 v[2][3];
#pragma unroll
            for (int p = 0; p < 2; ++p) {
                const int rr = rb + lr + 16 * p;
                const unsigned off = (unsigned)((r0 + rr) * w + c0a + cc * 16);
#pragma unroll
                for (int c = 0; c < 3; ++c)
                    v[p][c] = __builtin_bit_cast(u4, __builtin_amdgcn_raw_buffer_load_b128(rs, rr < nrow ? off + (unsigned)(c * pl) : 0xfffffff0u, 0, 0));
            }
#pragma unroll
            for (int p = 0; p < 2; ++p) {
                const int rr = rb + lr + 16 * p;
                if (rr < nrow) {
                    u4* out = reinterpret_cast<u4*>(smem + ((size_t)rr * ncol + cc * 16) * 4);
#pragma unroll
                    for (int m = 0; m < 4; ++m)
                        out[m] = u4{pj_rgbx(v[p][0][m], v[p][1][m], v[p][2][m], 0), pj_rgbx(v[p][0][m], v[p][1][m], v[p][2][m], 1),
                                    pj_rgbx(v[p][0][m], v[p][1][m], v[p][2][m], 2), pj_rgbx(v[p][0][m], v[p][1][m], v[p][2][m], 3)};
                }
            }
        }
}
// LDS bytes of a staged box of `px` pixels
template <typename PX>
__host__ __device__ constexpr size_t pj_box_bytes(size_t px) {
    return sizeof(PX) == 1 ? 4 * px + 4 : 3 * px * sizeof(PX);  // + 4: the (xf + 1) read of the box's last pixel
}
// Bilinear samples of two pixels A and B at once ({A, B} pairs; each operation an IEEE one of its own, in bilinear3's order): o?0 / o?1 = the pixel's (yf, xf) / (yc, xf) taps as indices into the staged box, sx? = 1 when
// the right-hand taps are the next column, 0 when they are the same one (xc == xf).
template <typename PX>
__device__ __forceinline__ void pj_bilinear2(lds_ptr<uint8_t> box, int plane_lds, int oA0, int oA1, int sxA, int oB0, int oB1, int sxB, f2v w_ld,
                                             f2v w_rd, f2v w_rt, f2v w_lt, f2v r[3]) {
    if constexpr (sizeof(PX) == 1) {
        const lds_ptr<unsigned> t = (lds_ptr<unsigned>)box;
        const unsigned Ald = t[oA0], An0 = t[oA0 + 1], Alt = t[oA1], An1 = t[oA1 + 1];
        const unsigned Bld = t[oB0], Bn0 = t[oB0 + 1], Blt = t[oB1], Bn1 = t[oB1 + 1];
        const unsigned Ard = sxA ? An0 : Ald, Art = sxA ? An1 : Alt, Brd = sxB ? Bn0 : Bld, Brt = sxB ? Bn1 : Blt;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const f2v ld = {(float)((Ald >> (8 * c)) & 255u), (float)((Bld >> (8 * c)) & 255u)};
            const f2v rd = {(float)((Ard >> (8 * c)) & 255u), (float)((Brd >> (8 * c)) & 255u)};
            const f2v rt = {(float)((Art >> (8 * c)) & 255u), (float)((Brt >> (8 * c)) & 255u)};
            const f2v lt = {(float)((Alt >> (8 * c)) & 255u), (float)((Blt >> (8 * c)) & 255u)};
            r[c] = w_ld * ld + w_rd * rd + w_rt * rt + w_lt * lt;
        }
    } else {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const lds_ptr<float> t = (lds_ptr<float>)box + c * plane_lds;
            const f2v ld = {t[oA0], t[oB0]}, rd = {t[oA0 + sxA], t[oB0 + sxB]}, lt = {t[oA1], t[oB1]}, rt = {t[oA1 + sxA], t[oB1 + sxB]};
            r[c] = w_ld * ld + w_rd * rd + w_rt * rt + w_lt * lt;
        }
    }
}
template <typename PX, int TH>
__device__ __forceinline__ void pj_stage_box(const PX* __restrict__ src, size_t pl, int w, int r0, int nrow, int c0a, int ncol, uint8_t* smem) {
    if constexpr (sizeof(PX) == 1)
        pj_stage_rgbx(src, pl, w, r0, nrow, c0a, ncol, smem);
    else
        pj_stage<PX, ((TH + TH / 8 + 11) / 8 > 4 ? (TH + TH / 8 + 11) / 8 : 4)>(src, pl, w, r0, nrow, c0a, ncol, smem);
}
// The staging policy of project_lds_tile / project_lds_tile_t: how a tile's source box gets into LDS.  This one is pj_stage_box on the
// planar source; k_rig_formats.inc has one that stages the same dwords straight from a packed or NV12 frame.  That one has no planar
// source (kPlanarSource = false), so a tile without a staged box cannot take the per-pixel form.  Such a tile is one of two kinds.
// A box over the LDS budget: the host's sizing rules it out for every tile.  An EMPTY box, c1 < c0: every source column of the tile
// lies outside the frame (edge tiles of wide frames at larger angles), so every pixel of it is 0, which is what the per-pixel form
// writes too -- pj_zero_px writes it without a source.
template <typename PX, int TH>
struct PjStagePlanar {
    static constexpr bool kPlanarSource = true;
    __device__ __forceinline__ void operator()(const PX* __restrict__ src, size_t pl, int w, int r0, int nrow, int c0a, int ncol, uint8_t* smem) const {
        pj_stage_box<PX, TH>(src, pl, w, r0, nrow, c0a, ncol, smem);
    }
};
// a finished sample into plane c: the row's offset is wave-uniform (one output row per wavefront and step), the lane adds its column
template <typename PX>
__device__ __forceinline__ void pj_store(__amdgpu_buffer_rsrc_t rd, unsigned x, unsigned row_c_elems, PX v);
template <>
__device__ __forceinline__ void pj_store<uint8_t>(__amdgpu_buffer_rsrc_t rd, unsigned x, unsigned row_c_elems, uint8_t v) {
    __builtin_amdgcn_raw_buffer_store_b8(v, rd, x, row_c_elems, 0);
}
template <>
__device__ __forceinline__ void pj_store<float>(__amdgpu_buffer_rsrc_t rd, unsigned x, unsigned row_c_elems, float v) {
    __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(v), rd, x * 4u, row_c_elems * 4u, 0);
}
// two finished pixels (rows y0 and y0 + 1 of column x) into the three planes, and the gray planes readFile derives from them
// (ImageProcess.cpp:20); the rows' offsets are wave-uniform, the lane adds its column
template <typename PX>
__device__ __forceinline__ void pj_emit2(__amdgpu_buffer_rsrc_t rd, int x, int y0, bool two, int w, size_t pl, const f2v r[3], bool in0, bool in1,
                                         uint8_t* __restrict__ gray, float* __restrict__ gray_f32) {
    PX oa[3], ob[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) oa[c] = in0 ? px_store<PX>(r[c].x) : PX(0), ob[c] = in1 ? px_store<PX>(r[c].y) : PX(0);
    const unsigned rowo = (unsigned)y0 * (unsigned)w;
#pragma unroll
    for (int c = 0; c < 3; ++c) pj_store<PX>(rd, (unsigned)x, rowo + (unsigned)c * (unsigned)pl, oa[c]);
    if (two) {
#pragma unroll
        for (int c = 0; c < 3; ++c) pj_store<PX>(rd, (unsigned)x, rowo + (unsigned)w + (unsigned)c * (unsigned)pl, ob[c]);
    }
    if constexpr (sizeof(PX) == 1) {
        if (gray || gray_f32) {
            const size_t off = (size_t)y0 * w + x;
            const uint8_t ga = gray_ref((uint8_t)oa[0], (uint8_t)oa[1], (uint8_t)oa[2]);
            if (gray) gray[off] = ga;
            if (gray_f32) gray_f32[off] = (float)ga;
            if (two) {
                const uint8_t gb = gray_ref((uint8_t)ob[0], (uint8_t)ob[1], (uint8_t)ob[2]);
                if (gray) gray[off + w] = gb;
                if (gray_f32) gray_f32[off + w] = (float)gb;
            }
        }
    }
}
// One pixel of the untiled form (k_project's arithmetic), for a tile whose box did not fit the LDS the host sized -- never
// the case when the host's estimate and the kernel's agree; kept out of line so that the tiled loop carries no trace of it.
template <typename PX>
__device__ __noinline__ void project_px_global(const PX* __restrict__ src, PX* __restrict__ dst, int w, int h, int flag, float r, int x, int y,
                                               uint8_t* __restrict__ gray, float* __restrict__ gray_f32) {
    const int width = flag ? h : w, height = flag ? w : h;
    const float dst_x = (float)((flag ? y : x) - width / 2), dst_y = (float)((flag ? x : y) - height / 2);
    const double rd = (double)r, dx = (double)dst_x;
    const float k = (float)(rd / sqrt(rd * rd + dx * dx));
    const float u = dst_x / k + (float)(width / 2), v = dst_y / k + (float)(height / 2);
    PX o[3] = {PX(0), PX(0), PX(0)};
    if (u >= 0 && u < (float)width && v >= 0 && v < (float)height) {
        if (flag)
            bilinear3<PX>(src, w, h, v, u, o);
        else
            bilinear3<PX>(src, w, h, u, v, o);
    }
    const size_t pl = (size_t)w * h, off = (size_t)y * w + x;
    dst[off] = o[0], dst[off + pl] = o[1], dst[off + 2 * pl] = o[2];
    if constexpr (sizeof(PX) == 1) {
        if (gray || gray_f32) {
            const uint8_t gv = gray_ref((uint8_t)o[0], (uint8_t)o[1], (uint8_t)o[2]);
            if (gray) gray[off] = gv;
            if (gray_f32) gray_f32[off] = (float)gv;
        }
    }
}
// One pixel of a tile whose source columns all lie outside the frame: 0 in the three planes (what project_px_global stores there).
template <typename PX>
__device__ __forceinline__ void pj_zero_px(PX* __restrict__ dst, size_t pl, size_t off) {
    dst[off] = PX(0), dst[off + pl] = PX(0), dst[off + 2 * pl] = PX(0);
}
// (The tile's work is a device function so that k_project_lds_many, k_rig.inc, runs it per image of a batch: blockIdx.x / .y
// address the tile.)
template <typename PX, int TW, int TH, typename STAGE = PjStagePlanar<PX, TH>>
__device__ __forceinline__ void project_lds_tile(const PX* __restrict__ src, PX* __restrict__ dst, int w, int h, float r,
                                                 uint8_t* __restrict__ gray, float* __restrict__ gray_f32, int lds_bytes, STAGE stage = STAGE()) {
    extern __shared__ __attribute__((aligned(16))) uint8_t pj_smem[];
    __shared__ ProjCol corner[4];
    constexpr int CPX = PJ_CHUNK / (int)sizeof(PX);  // pixels per staging chunk
    constexpr int RPT = TH / (256 / TW);             // rows per work-item
    const int xa = blockIdx.x * TW, ya = blockIdx.y * TH;
    const int xb = min(xa + TW, w) - 1, yb = min(ya + TH, h) - 1;
    // ---- the tile's source box: four columns decide it (first, last, nearest to and farthest from the axis), evaluated by
    // four work-items and shared ----
    if (threadIdx.x < 4) {
        const int xmid = w / 2, xnear = xa <= xmid && xmid <= xb ? xmid : (abs(xa - xmid) < abs(xb - xmid) ? xa : xb),
                  xfar = abs(xa - xmid) > abs(xb - xmid) ? xa : xb;
        const int xs = threadIdx.x == 0 ? xa : threadIdx.x == 1 ? xb : threadIdx.x == 2 ? xnear : xfar;
        corner[threadIdx.x] = proj_col(xs, w, r);
    }
    // meanwhile every work-item evaluates its own column (one output column, RPT rows per work-item)
    const int tx = threadIdx.x % TW, ty = __builtin_amdgcn_readfirstlane(threadIdx.x / TW);  // TW is a multiple of 64: a wavefront = one row
    const int x = min(xa + tx, xb);
    const ProjCol col = proj_col(x, w, r);
    __syncthreads();
    int c0 = (int)floorf(corner[0].u), c1 = (int)ceilf(corner[1].u);  // u grows with x
    c0 = max(c0, 0);
    c1 = min(c1, w - 1);
    // for a row, |v - h/2| grows with |dx|: the columns nearest to / farthest from the axis bound v over the tile
    const float kn = corner[2].k, kf = corner[3].k;
    const float v00 = proj_v(ya, h, kn), v01 = proj_v(ya, h, kf), v10 = proj_v(yb, h, kn), v11 = proj_v(yb, h, kf);
    int r0 = (int)floorf(fminf(fminf(v00, v01), fminf(v10, v11))), r1 = (int)ceilf(fmaxf(fmaxf(v00, v01), fmaxf(v10, v11)));
    r0 = max(r0, 0);
    r1 = min(r1, h - 1);
    const int c0a = c0 / CPX * CPX;                          // chunk-aligned first column
    const int ncol = ((c1 - c0a + 1) + CPX - 1) / CPX * CPX;  // staged columns per row
    const int nrow = max(r1 - r0 + 1, 0);
    const size_t pl = (size_t)w * h;
    const bool fits = c1 >= c0 && pj_box_bytes<PX>((size_t)nrow * ncol) <= (size_t)lds_bytes;  // the host sized lds_bytes for every tile
    if (!fits) {  // workgroup-uniform
        if (xa + tx <= xb)
            for (int q = 0; q < RPT; ++q) {
                const int y = ya + ty * RPT + q;
                if (y > yb) continue;
                if constexpr (STAGE::kPlanarSource)
                    project_px_global<PX>(src, dst, w, h, 0, r, xa + tx, y, gray, gray_f32);
                else
                    pj_zero_px<PX>(dst, pl, (size_t)y * w + xa + tx);
            }
        return;
    }
    stage(src, pl, w, r0, nrow, c0a, ncol, pj_smem);
    __syncthreads();
    if (xa + tx > xb) return;
    const float u = col.u;
    const bool xin = u >= 0 && u < (float)w;
    const int xf = (int)floorf(u);
    const float cx = ceilf(u);
    const int xc = cx >= (float)(w - 1) ? (w - 1) : (int)cx;
    const float a = u - (float)xf;
    const int lx = xin ? xf - c0a : 0, sx = xin && xc != xf ? 1 : 0;
    const __amdgpu_buffer_rsrc_t rd = plane_rsrc(dst, 3 * pl);  // planes below 4 GB (the host keeps 3 * w * h * sizeof(PX) under that)
    // two rows per step: the arithmetic of a pixel is what it was (every operation an IEEE one on its own, no contraction)
    static_assert(RPT % 2 == 0, "rows per work-item come in pairs");
    const f2v k2 = {col.k, col.k}, rc2 = {pj_rcp(col.k), pj_rcp(col.k)};
    const float hh = (float)(h / 2), oma = 1 - a;
    for (int q = 0; q < RPT; q += 2) {
        const int y0 = ya + ty * RPT + q;  // wave-uniform
        if (y0 > yb) break;
        const bool two = y0 < yb;
        const int y1 = two ? y0 + 1 : y0;
        const f2v n = {(float)(y0 - h / 2), (float)(y1 - h / 2)};
        const f2v v = pj_div2(n, k2, rc2) + hh;  // proj_v of the two rows
        const bool in0 = xin && v.x >= 0 && v.x < (float)h, in1 = xin && v.y >= 0 && v.y < (float)h;
        // branch-free: an outside pixel computes on the box's first sample and is replaced by 0
        const f2v vi = {in0 ? v.x : (float)r0, in1 ? v.y : (float)r0};
        const f2v fl = {floorf(vi.x), floorf(vi.y)};
        const int yf0 = (int)fl.x, yf1 = (int)fl.y;
        const float cy0 = ceilf(vi.x), cy1 = ceilf(vi.y);
        const int yc0 = cy0 >= (float)(h - 1) ? (h - 1) : (int)cy0, yc1 = cy1 >= (float)(h - 1) ? (h - 1) : (int)cy1;
        const f2v b = vi - fl, omb = 1 - b;
        const f2v w_ld = oma * omb, w_rd = a * omb, w_rt = a * b, w_lt = oma * b;
        const int oA0 = (yf0 - r0) * ncol + lx, oA1 = oA0 + (yc0 - yf0) * ncol;
        const int oB0 = (yf1 - r0) * ncol + lx, oB1 = oB0 + (yc1 - yf1) * ncol;
        f2v res[3];
        pj_bilinear2<PX>((lds_ptr<uint8_t>)pj_smem, nrow * ncol, oA0, oA1, sx, oB0, oB1, sx, w_ld, w_rd, w_rt, w_lt, res);
        pj_emit2<PX>(rd, x, y0, two, w, pl, res, in0, in1, gray, gray_f32);
    }
}
template <typename PX, int TW, int TH>
__global__ __launch_bounds__(256) void k_project_lds(const PX* __restrict__ src, PX* __restrict__ dst, int w, int h, float r,
                                                     uint8_t* __restrict__ gray, float* __restrict__ gray_f32, int lds_bytes) {
    project_lds_tile<PX, TW, TH>(src, dst, w, h, r, gray, gray_f32, lds_bytes);
}

// Landscape frames (the reference's `flag == 1` branch, Projection.cpp:24-26,30-49: the roles of the axes swap): k and the
// source ROW u depend on the output row alone, the source column v = (x - w/2)/k(y) + w/2 on both.  Same tiling; the per-row
// terms of a tile's TH rows are evaluated by TH work-items and shared through LDS, the tile's source box is bounded by its
// first and last row (u grows with y) and, for the columns, by its rows nearest to / farthest from the axis.
template <typename PX, int TW, int TH, typename STAGE = PjStagePlanar<PX, TH>>
__device__ __forceinline__ void project_lds_tile_t(const PX* __restrict__ src, PX* __restrict__ dst, int w, int h, float r,
                                                   uint8_t* __restrict__ gray, float* __restrict__ gray_f32, int lds_bytes, STAGE stage = STAGE()) {
    extern __shared__ __attribute__((aligned(16))) uint8_t pj_smem[];
    __shared__ ProjCol corner[4];
    __shared__ __attribute__((aligned(16))) ProjRow rowc[TH];
    constexpr int CPX = PJ_CHUNK / (int)sizeof(PX);
    constexpr int RPT = TH / (256 / TW);
    const int xa = blockIdx.x * TW, ya = blockIdx.y * TH;
    const int xb = min(xa + TW, w) - 1, yb = min(ya + TH, h) - 1;
    if (threadIdx.x < 4) {
        const int ymid = h / 2, ynear = ya <= ymid && ymid <= yb ? ymid : (abs(ya - ymid) < abs(yb - ymid) ? ya : yb),
                  yfar = abs(ya - ymid) > abs(yb - ymid) ? ya : yb;
        const int ys = threadIdx.x == 0 ? ya : threadIdx.x == 1 ? yb : threadIdx.x == 2 ? ynear : yfar;
        corner[threadIdx.x] = proj_col(ys, h, r);  // the "width" of this branch is the image height
    }
    if (threadIdx.x >= 64 && threadIdx.x < 64 + TH) {
        const ProjCol pc = proj_col(min(ya + (int)threadIdx.x - 64, yb), h, r);
        rowc[threadIdx.x - 64] = ProjRow{pc.k, pc.u, pj_rcp(pc.k), 0.f};
    }
    __syncthreads();
    int r0 = (int)floorf(corner[0].u), r1 = (int)ceilf(corner[1].u);  // u grows with y
    r0 = max(r0, 0);
    r1 = min(r1, h - 1);
    const float kn = corner[2].k, kf = corner[3].k;
    const float v00 = proj_v(xa, w, kn), v01 = proj_v(xa, w, kf), v10 = proj_v(xb, w, kn), v11 = proj_v(xb, w, kf);
    int c0 = (int)floorf(fminf(fminf(v00, v01), fminf(v10, v11))), c1 = (int)ceilf(fmaxf(fmaxf(v00, v01), fmaxf(v10, v11)));
    c0 = max(c0, 0);
    c1 = min(c1, w - 1);
    const int c0a = c0 / CPX * CPX;
    const int ncol = ((c1 - c0a + 1) + CPX - 1) / CPX * CPX;
    const int nrow = max(r1 - r0 + 1, 0);
    const size_t pl = (size_t)w * h;
    const bool fits = c1 >= c0 && pj_box_bytes<PX>((size_t)nrow * ncol) <= (size_t)lds_bytes;
    const int tx = threadIdx.x % TW, ty = __builtin_amdgcn_readfirstlane(threadIdx.x / TW);
    const int x = xa + tx;
    if (!fits) {  // workgroup-uniform; see k_project_lds
        if (x <= xb)
            for (int q = 0; q < RPT; ++q) {
                const int y = ya + ty * RPT + q;
                if (y > yb) continue;
                if constexpr (STAGE::kPlanarSource)
                    project_px_global<PX>(src, dst, w, h, 1, r, x, y, gray, gray_f32);
                else
                    pj_zero_px<PX>(dst, pl, (size_t)y * w + x);
            }
        return;
    }
    stage(src, pl, w, r0, nrow, c0a, ncol, pj_smem);
    __syncthreads();
    if (x > xb) return;
    const __amdgpu_buffer_rsrc_t rd = plane_rsrc(dst, 3 * pl);
    static_assert(RPT % 2 == 0, "rows per work-item come in pairs");
    const float nx = (float)(x - w / 2), hw = (float)(w / 2);
    for (int q = 0; q < RPT; q += 2) {
        const int y0 = ya + ty * RPT + q;  // wave-uniform
        if (y0 > yb) break;
        const bool two = y0 < yb;
        const ProjRow ra = rowc[y0 - ya], rb = rowc[(two ? y0 + 1 : y0) - ya];
        const f2v u = {ra.u, rb.u};
        const f2v v = pj_div2(f2v{nx, nx}, f2v{ra.k, rb.k}, f2v{ra.rc, rb.rc}) + hw;  // proj_v(x, w, k of the row)
        // width = h, height = w in this branch
        const bool in0 = u.x >= 0 && u.x < (float)h && v.x >= 0 && v.x < (float)w, in1 = u.y >= 0 && u.y < (float)h && v.y >= 0 && v.y < (float)w;
        // bilinear3(src, w, h, x = v, y = u); branch-free: an outside pixel computes on the box's first sample and is replaced by 0
        const f2v vi = {in0 ? v.x : (float)c0a, in1 ? v.y : (float)c0a}, ui = {in0 ? u.x : (float)r0, in1 ? u.y : (float)r0};
        const f2v flx = {floorf(vi.x), floorf(vi.y)}, fly = {floorf(ui.x), floorf(ui.y)};
        const int xf0 = (int)flx.x, xf1 = (int)flx.y, yf0 = (int)fly.x, yf1 = (int)fly.y;
        const float cx0 = ceilf(vi.x), cx1 = ceilf(vi.y), cy0 = ceilf(ui.x), cy1 = ceilf(ui.y);
        const int xc0 = cx0 >= (float)(w - 1) ? (w - 1) : (int)cx0, xc1 = cx1 >= (float)(w - 1) ? (w - 1) : (int)cx1;
        const int yc0 = cy0 >= (float)(h - 1) ? (h - 1) : (int)cy0, yc1 = cy1 >= (float)(h - 1) ? (h - 1) : (int)cy1;
        const f2v a = vi - flx, b = ui - fly, oma = 1 - a, omb = 1 - b;
        const f2v w_ld = oma * omb, w_rd = a * omb, w_rt = a * b, w_lt = oma * b;
        const int oA0 = (yf0 - r0) * ncol + (xf0 - c0a), oA1 = oA0 + (yc0 - yf0) * ncol;
        const int oB0 = (yf1 - r0) * ncol + (xf1 - c0a), oB1 = oB0 + (yc1 - yf1) * ncol;
        f2v res[3];
        pj_bilinear2<PX>((lds_ptr<uint8_t>)pj_smem, nrow * ncol, oA0, oA1, xc0 - xf0, oB0, oB1, xc1 - xf1, w_ld, w_rd, w_rt, w_lt, res);
        pj_emit2<PX>(rd, x, y0, two, w, pl, res, in0, in1, gray, gray_f32);
    }
}
template <typename PX, int TW, int TH>
__global__ __launch_bounds__(256) void k_project_lds_t(const PX* __restrict__ src, PX* __restrict__ dst, int w, int h, float r,
                                                       uint8_t* __restrict__ gray, float* __restrict__ gray_f32, int lds_bytes) {
    project_lds_tile_t<PX, TW, TH>(src, dst, w, h, r, gray, gray_f32, lds_bytes);
}
