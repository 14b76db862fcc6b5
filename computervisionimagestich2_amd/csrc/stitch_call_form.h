// The pair path's decisions, without HIP: what a plan of a canvas size holds (PlanShape, plan_shape) and which kernels reduce and
// collapse every level of a call with n pairs (CallForm, call_form).  Plain C++17: the library's host code (stitch_hip.hip) fills the
// shape, carves its arena from it and launches from the record; tests/call_form_dump.cpp prints the records on a machine without a GPU.
// Every rule of the path -- a threshold, a condition -- is written ONCE, here.  The band path's decisions (one pair split into row bands
// over ranks: BandShape, band_shape, BandForm, band_form) follow at the end of the file, under the same rule.
//
// REDUCE of level l (ImageProcess.cpp:705-715) is blur(G_l) into the scratch T, then decimate T into G_{l+1}.  The blur is a causal and
// an anticausal sweep along x, then along y.  call_form decides in four steps, so that no two places have to reach the same answer:
//   1  each level's sweep family and its zero-tile flags of T, from the plan and n alone (level_sweep);
//   2  what the sweeps of level l can record about G_{l+1}, and what the readers of G_{l+1} can take (produces_flags, reads_flags);
//   3  the G column flags and the mask-row flags of levels 1 and 2: on where 2 holds on both sides;
//   4  the kernels: causal x, anticausal x, causal y, anticausal y + decimation, the coarse launch, the collapse.
// A flag array is therefore never on without its producer or without its readers, and the collapse reads the record the reduce read.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "stitch.h"

#ifndef STITCH_CROWS
#define STITCH_CROWS 8
#endif

namespace sk {

// ---- constants the kernels and the decision share ---------------------------------------------------------------------------------
constexpr int TS = 64;                      // tile edge = the wavefront's width (stitch_kernels.hpp asserts it): a lane per column
constexpr int YCH = 8, YCOLS = 2 * TS;      // rows per chunk and columns per workgroup of the anticausal y sweeps
constexpr int XY_MAXNC = 1024;              // tile columns whose flags k_vv_xby_m keeps in LDS
constexpr int CROWS = STITCH_CROWS;         // rows per strip of the collapse, the unit
constexpr int CO_MAXL = 16;                 // levels of one k_coarse launch
constexpr int CO_MAXSIDE = 512;             // the host never hands k_coarse a level with w/2 + h/2 above this (tap tables in LDS)
constexpr int CO_TABN = 192;                // entries of the expand tables of all coarse levels together
constexpr int MAXB = 16;                    // pairs per plan / launch
constexpr int CO_LDS_BYTES = 144 * 1024;    // dynamic LDS k_coarse_lds may take (160 KB per CU, 15 KB of tables beside it)

// ---- thresholds of the decision, each with its one use ----------------------------------------------------------------------------
constexpr long CHAIN3_BLOCKS = 340;         // blocks up to which a sweep takes the chain + loader + storer kernels (k_vv_x_m, k_vv_y_m): each finds SIMDs of its own
constexpr long CHAIN3_BLOCKS_SRC = 1024;    // the same at a source-fused level 0, where the loader also hides the gathers
constexpr long CHIP_BANDS = 800;            // planes x 64-row bands of level 0 from which ONE pair fills the chip (config 5's 24576 x 16384)
constexpr int WF_MIN_SIDE = 1024;           // a level joins the batch's fused sweep from this width and height
constexpr long Y_LONE_WGS = 1536;           // workgroups of a y sweep below which SIMDs idle (fewer than 1.5 wavefronts each): one column per lane
constexpr int ZT_MAX_BANDS = 256;           // bands per plane the flag users address
// ---- defaults of the fused sweep's hand-off (a plan's STITCH_XBYF_WGS / STITCH_XBYF_SPIN_LIMIT move them; a band takes them as they are)
constexpr int WF_MAX_WGS = 2304;            // persistent workgroups: at most 9 per CU by LDS
constexpr unsigned WF_SPIN_LIMIT = 1u << 23;  // polls before a hand-off wait gives up, about 20 s; 2^20 (2-3 s) was reached once in a warm-up
constexpr int BAND_HALO = 2;                // rows of either neighbour a band holds of a level that an EXPAND reads

inline int round_up(int v, int m) { return (v + m - 1) / m * m; }
inline int tiles(int v) { return (v + TS - 1) / TS; }
// Row pitch of a level's planes in floats: the width rounded up to 64, plus -- for rows of 16 KB and more -- `pad` floats
// (STITCH_PITCH_PAD, rounded up to 64) so that the 64 rows of a tile do not start a power-of-two-ish number of bytes apart.
inline int level_pitch(int w, int pad) { return round_up(w, 64) + (pad > 0 && w >= 4096 ? round_up(pad, 64) : 0); }

// Tuning / A-B switches of a plan (listed in include/stitch.h; none changes a result bit): ONE snapshot of the environment,
// taken when a plan is created and again whenever a host-pointer entry point looks for an idle plan in the cache.  The
// snapshot is part of the cache key (PlanKey), so a caller who flips a switch between two calls gets a workspace built for
// the new setting, never a stale one.  All fields are ints (no padding: compared with memcmp); -1 = not set.
struct Tuning {
    int wavefront, no_fuse, no_src_fuse, no_zero_tiles, crows_l0, crows_ln, collapse4, xbyf_wgs, xbyf_spin_limit, xbyf_early, y2,
        recompute, stamp, gate64, coarse, single_fast, odd_dec, c4_gen, collapse_px, y1s, c4_lock, c4_swz, mover, src_lone, dec7, xbym, xbym_mpix, coarse_lds, pitch_pad, crows_wgs;
    static int env_int(const char* name) {
        const char* e = std::getenv(name);
        return e ? std::max(0, atoi(e)) : -1;
    }
    static Tuning from_env();  // (stitch_hip.hip: the one reader of the environment)
    static Tuning unset() {    // what from_env gives in an empty environment
        Tuning t;
        int* f = reinterpret_cast<int*>(&t);
        for (size_t i = 0; i < sizeof t / sizeof(int); ++i) f[i] = -1;
        t.no_fuse = t.no_src_fuse = t.no_zero_tiles = t.y2 = t.stamp = t.gate64 = 0;
        return t;
    }
    bool operator==(const Tuning& o) const { return std::memcmp(this, &o, sizeof o) == 0; }
};

struct Level {
    int w, h, pitch;
    size_t ps;         // plane stride in floats = pitch*h
    int c4_xa, c4_xb;  // columns [c4_xa, c4_xb) of this level go to k_collapse4 (multiples of 256; empty when equal)
    int c4_gen;        // != 0: [0, c4_xb) with per-lane tap offsets (k_collapse4 GEN) -- chosen where it covers more than the fixed pattern
    // device addresses, null in a bare shape (whoever carves the arena fills them in)
    float* g;          // 7 planes [a0 a1 a2 b0 b1 b2 m] + 64 slack rows
    float* e;          // 3 planes (collapse chain), levels >= 1
    int32_t *ix, *iy;  // expand tables level+1 -> level (levels < L-1)
    double *ax, *ay;
};

// CImg.h:29625-29637: idx/alpha of the linear up-sampling walk
inline void expand_table(int n_src, int n_dst, std::vector<int32_t>& idx, std::vector<double>& alpha) {
    idx.resize(n_dst);
    alpha.resize(n_dst);
    if (n_src == 1) {
        for (int x = 0; x < n_dst; ++x) idx[x] = 0, alpha[x] = 0;
        return;
    }
    const double fx = n_dst > 1 ? (n_src - 1.0) / (n_dst - 1) : 0;
    double curr = 0;
    for (int x = 0; x < n_dst; ++x) {
        idx[x] = (int32_t)(unsigned int)curr;
        alpha[x] = curr - (unsigned int)curr;
        const double nxt = curr + fx;
        curr = (n_src - 1.0) < nxt ? (n_src - 1.0) : nxt;
    }
}

// The longest run of 256-column blocks in which every group of four columns x0.. has the resize taps s, s+1, s+1, s+2 with
// s+3 inside the source row (see k_collapse4); [*xa, *xb) empty when there is none or the source level is a single row/column.
inline void regular_range(const std::vector<int32_t>& idx, int w, int sw, int sh, int* xa, int* xb) {
    *xa = *xb = 0;
    int best_a = 0, best_b = 0, run_a = -1;
    const int nblk = w / 256;
    for (int b = 0; b <= nblk; ++b) {
        bool reg = b < nblk && sw >= 2 && sh >= 2;
        for (int x0 = b * 256; reg && x0 < (b + 1) * 256; x0 += 4) {
            const int s_ = idx[x0];
            reg = idx[x0 + 1] == s_ + 1 && idx[x0 + 2] == s_ + 1 && idx[x0 + 3] == s_ + 2 && s_ + 3 <= sw - 1;
        }
        if (reg && run_a < 0) run_a = b;
        if (!reg && run_a >= 0) {
            if (b - run_a > best_b - best_a) best_a = run_a, best_b = b;
            run_a = -1;
        }
    }
    if (best_b > best_a) *xa = best_a * 256, *xb = best_b * 256;
}

// The columns [0, *xb) (a multiple of 256) in which every group of four columns x0.. has its taps inside ONE 16-byte load at
// ix[x0]: ix[x0 + 3] + 1 <= ix[x0] + 3 (always true for a step below 1/2; see k_collapse4, GEN).  The window may reach past the
// source row's last sample: the last group of an even width has the taps s, s+1, s+1, s+1 or s, s+1, s+1, s+2 with the row ending
// at s + 2, so element 3 of its window is the first sample of the next row (of the next plane, of whatever follows the planes in
// the arena) -- loaded, selected by no tap: a column whose first tap IS the row's last sample takes that sample twice, as the
// reference does (CImg.h:29648), whatever the window holds behind it.
inline void general_range(const std::vector<int32_t>& idx, int w, int sw, int sh, int* xb) {
    *xb = 0;
    if (sw < 4 || sh < 2) return;
    int x0 = 0;
    for (; x0 + 3 < w; x0 += 4) {
        const int s_ = idx[x0];
        if (!(idx[x0 + 1] >= s_ && idx[x0 + 2] >= idx[x0 + 1] && idx[x0 + 3] >= idx[x0 + 2] && idx[x0 + 3] - s_ <= 2 && s_ >= 0 && s_ + 1 <= sw - 1)) break;
    }
    *xb = x0 / 256 * 256;
}

// ---- the level-0 collapse of a call with the step mask: which image(s) a 256-column block of k_collapse4 reads --------------------
// The level-0 mask of such a call is the seam's step (k_sweeps.inc, mask_step): branch 0: 1 where (double)x < thr, otherwise 1 where
// x >= start -- one function of x for every row, monotone in x.  (constexpr: the kernel evaluates the same lines.)
constexpr int c4_step_at(int branch, int start, double thr, int x) { return branch == 0 ? ((double)x < thr ? 1 : 0) : (x >= start ? 1 : 0); }
// The block whose first and last live columns are xf and xl: 1 = the step is 1 on all of it (only image a is read), 2 = it is 0 (only
// image b), 0 = the step changes inside it (both).
constexpr int c4_block_side(int branch, int start, double thr, int xf, int xl) {
    return c4_step_at(branch, start, thr, xf) != c4_step_at(branch, start, thr, xl) ? 0 : c4_step_at(branch, start, thr, xf) ? 1 : 2;
}
// counts[0..2] = the blocks of columns [xa, xb) (k_collapse4's range of the launch: block b starts at xa + 256 b) that read only a, only
// b, both.  sides == 0 (no step mask, or a library that always reads both): every block reads both.
inline void c4_side_counts(int branch, int start, double thr, int xa, int xb, int sides, int counts[3]) {
    counts[0] = counts[1] = counts[2] = 0;
    for (int xf = xa; xf < xb; xf += 256) {
        const int side = sides ? c4_block_side(branch, start, thr, xf, std::min(xf + 255, xb - 1)) : 0;
        ++counts[side == 1 ? 0 : side == 2 ? 1 : 2];
    }
}

// Level sizes of a w x h canvas (ImageProcess.cpp:675-676, :706-707) -> the level count, 1..32.  0: a non-positive size;
// -1: a count outside 1..32; -(2 + i): level i has a zero dimension (the reference degenerates there).
inline int pyramid_sizes(int w, int h, int level_rule, int* lw, int* lh) {
    if (w <= 0 || h <= 0) return 0;
    const int len = level_rule ? (w < h ? w : h) : (w >= h ? w : h);
    int levels = 0;
    while ((len >> (levels + 1)) > 0) ++levels;  // floor(log2(len))
    if (levels < 1 || levels > 32) return -1;
    int cw = w, ch = h;
    for (int i = 0; i < levels; ++i) {
        if (cw <= 0 || ch <= 0) return -(2 + i);
        if (lw) lw[i] = cw;
        if (lh) lh[i] = ch;
        cw /= 2;
        ch /= 2;
    }
    return levels;
}

// What a plan of one canvas size is, before anything is allocated.
struct PlanShape {
    int cw = 0, ch = 0, L = 0;
    int cap = 1;  // pairs per launch sequence this workspace can hold (planes of pair b follow pair b-1)
    stitch_blend_opts opts{};
    Tuning tune{};  // the environment's switches as they were when the plan was created
    Level lv[32]{};
    bool blur_skip = false;  // sigma below the blur's threshold: REDUCE decimates G itself (CImg.h:35051 / :34800)
    bool no_fuse = false;    // STITCH_NO_FUSE=1: keep blur and decimation as separate kernels (A/B and tests)
    // level 0 (a, b AND the mask plane) is handed in by the caller (the coarse levels of a band-split pair): no seam scan, and so neither
    // the implicit mask nor source fusion (mask_opt and src_fuse are off), no G column or mask-row flags.  An input of plan_shape.
    bool planes_in = false;
    // level 0 is composed from the pairs' frames (k_compose) and its mask plane is written from a path per pair (k_mask_path,
    // include/stitch_seam_path.h): the stored-mask shape of planes_in, for up to `cap` pairs.  An input of plan_shape.
    bool masked = false;
    bool mask_stored() const { return planes_in || masked; }  // the level-0 mask is plane 6 in memory, never the seam's step
    // fused anticausal-x + causal-y wavefront sweep (k_vv_xbyf) for the first `wf_levels` levels
    int wf_levels = 0;
    // The causal x sweep of a wavefront level keeps only its state in front of every tile and the fused sweep re-runs it
    // tile by tile (k_vv_x_fwd<.., CKPT>, k_vv_xbyf MODE 1/2): the x-swept level is neither written nor read back.
    // STITCH_RECOMPUTE=0 keeps the two-pass form.
    int recompute = 0;        // 0 off, 1 every wavefront level, 2 the wavefront levels >= 1 only
    bool zero_tiles = false;  // zero-tile flags of T (STITCH_NO_ZERO_TILES=1: move the zeros like any other sample)
    bool mask_opt = false;    // level-0 mask handled implicitly (Van Vliet, both sweeps at level 0)
    bool src_fuse = false;    // pairs: level-0 planes evaluated from the frames by their consumers, k_compose never runs
    int coarse_from = 0;      // > 0: levels coarse_from .. L-1 run in ONE launch (k_coarse: REDUCE to the top, top blend, collapse back up)
    // rows per work-item strip of the collapse (collapse_rows): STITCH_CROWS_L0 / STITCH_CROWS_LN override
    int crows_ln = 0;  // 0 = per level
    int crows_l0 = 4 * CROWS;
    bool collapse4 = true;  // four columns per work-item in the collapse where possible (STITCH_COLLAPSE4=0: always k_collapse)
    // which buffers the plan has beside the levels' planes and tables
    bool has_wf = false;    // hand-off granules and band-queue heads (wf_yg, wf_ctrl): either fused sweep
    bool has_zt = false;    // zt, zi: zero-tile flags of T and of the index plane
    bool has_gz[2] = {false, false};  // G column flags of levels 1 and 2
    bool has_mr[2] = {false, false};  // row-repeat flags of the mask plane of levels 1 and 2
    // diagnostic stamp buffers asked for (the library clears one it could not allocate)
    bool stamp_wf = false, stamp_xy = false, stamp_co = false;
    int stamp_d7_level = -1;

    int l_end() const { return coarse_from > 0 ? coarse_from : L - 1; }  // levels [0, l_end) are reduced and collapsed level by level
};

struct StampRequest {  // STITCH_WAVEFRONT_STAMP is Tuning::stamp
    bool xy = false, co = false;
    int d7_level = -1;
};

// One pair whose level 0 alone fills the chip: a throughput case like a batch.
inline bool chip_filling(int h0) { return 7L * tiles(h0) >= CHIP_BANDS; }

// Fills the shape of a cw x ch plan for `cap` pairs; planes_in, masked: see PlanShape.  Returns pyramid_sizes' answer: the level count, or <= 0
// and an untouched shape.  The ONE writer of a shape: nothing sets a field of it afterwards.
inline int plan_shape(PlanShape& s, int cw, int ch, const stitch_blend_opts& o, int cap, const Tuning& tn, const StampRequest& st = StampRequest{},
                      bool planes_in = false, bool masked = false) {
    int lw[32], lh[32];
    const int L = pyramid_sizes(cw, ch, o.level_rule, lw, lh);
    if (L <= 0) return L;
    s = PlanShape{};
    s.cw = cw, s.ch = ch, s.L = L, s.cap = cap, s.opts = o, s.tune = tn;
    s.no_fuse = tn.no_fuse != 0;
    s.planes_in = planes_in;
    s.masked = masked;
    const bool stored = s.mask_stored();
    s.blur_skip = o.blur_kind == 0 ? (o.sigma < 0.5f) : (o.sigma < 0.1f);
    for (int l = 0; l < L; ++l) {
        Level& v = s.lv[l];
        v.w = lw[l];
        v.h = lh[l];
        v.pitch = level_pitch(v.w, tn.pitch_pad);
        v.ps = (size_t)v.pitch * v.h;
    }
    // resize tables' column ranges of the collapse (the tables themselves are uploaded by the library)
    for (int l = 0; l + 1 < L; ++l) {
        Level& v = s.lv[l];
        std::vector<int32_t> idx;
        std::vector<double> al;
        expand_table(lw[l + 1], v.w, idx, al);
        regular_range(idx, v.w, lw[l + 1], lh[l + 1], &v.c4_xa, &v.c4_xb);
        int gxb = 0;
        general_range(idx, v.w, lw[l + 1], lh[l + 1], &gxb);
        // STITCH_C4_GEN: 0 never, 1 where it gains two blocks or more, 2 / unset wherever it gains a block
        v.c4_gen = tn.c4_gen != 0 && gxb >= (v.c4_xb - v.c4_xa) + (tn.c4_gen == 1 ? 512 : 256);
        if (v.c4_gen) v.c4_xa = 0, v.c4_xb = gxb;
    }
    // wavefront sweep: STITCH_WAVEFRONT=<levels> (Van Vliet only), or
    // auto: the band pipeline pays where a launch has many bands in flight (planes x 64-row bands of level 0: 896 for two
    // 6144x4096 pairs, 1792 for one 24576x16384 pair) to hide its fill (bands x hand-off latency) and the levels have
    // enough tiles to stream; a lone 6144x4096 pair (448 bands) is faster unfused
    int wf = 0;
    if (tn.wavefront >= 0)
        wf = std::min(4, tn.wavefront);
    else if (cap >= 2 || chip_filling(lh[0]))
        while (wf < 2 && wf < L - 1 && lw[wf] >= WF_MIN_SIDE && lh[wf] >= WF_MIN_SIDE) ++wf;
    if (o.blur_kind != 0 || tn.no_fuse || o.sigma < 0.5f) wf = 0;
    wf = std::min(wf, L - 1);
    while (wf > 0 && (lw[wf - 1] < 2 || lh[wf - 1] < 2)) --wf;
    s.wf_levels = wf;
    // (a plan without fused-sweep levels keeps the hand-off buffers for k_vv_xby_m: one pair in flight, from STITCH_XBYM_MPIX megapixels per level)
    s.has_wf = wf > 0 || (o.blur_kind == 0 && !tn.no_fuse && o.sigma >= 0.5f && L >= 2);
    s.has_zt = wf > 0;
    for (int i = 0; i < 2; ++i) s.has_gz[i] = s.has_mr[i] = wf > 0 && i + 1 < L && !stored;  // (reads_flags: a stored level-0 mask knows no flags)
    // opt-in: level 0 re-run from the frames measured 3 % slower, the plane levels within noise
    if (tn.recompute >= 0 && wf > 0) s.recompute = std::min(2, tn.recompute);
    s.zero_tiles = wf > 0 && !tn.no_zero_tiles;
    s.stamp_wf = wf > 0 && tn.stamp;
    s.stamp_xy = s.has_wf && st.xy;
    s.stamp_d7_level = st.d7_level;
    // implicit level-0 mask: needs both Van Vliet sweeps at level 0 (the x sweeps then run per-plane bands at any height;
    // STITCH_GATE64=1 restores the old restriction to heights that are multiples of 64 for A/B runs)
    s.mask_opt = !stored && !s.no_fuse && o.blur_kind == 0 && !s.blur_skip && L >= 2 && lw[0] > 1 && lh[0] > 1 && !(tn.gate64 && lh[0] % 64);
    if (tn.crows_l0 >= 0) s.crows_l0 = std::max(1, tn.crows_l0);
    if (tn.crows_ln >= 0) s.crows_ln = std::max(1, tn.crows_ln);
    if (tn.collapse4 >= 0) s.collapse4 = tn.collapse4 != 0;
    s.src_fuse = s.mask_opt && !tn.no_src_fuse;  // STITCH_NO_SRC_FUSE: A/B and tests, keep S1 as its own kernel (k_compose)
    // coarse levels in one launch (k_coarse): from the first level l >= 1 whose sides are both at most STITCH_COARSE (default 40;
    // 0 = never), when at least two levels qualify.  One workgroup -- one CU -- per pair: measured on the reference's 1081 x 527
    // panorama, the levels from 33 x 16 down take 65 us in k_coarse against 124 us as 31 launches of their own (4.5 us of
    // start-up each, 15 us for a collapse level), but 67 x 32 already costs more in one CU (the collapse's ~220 double-precision
    // operations per pixel) than spread over the chip.  Van Vliet only.
    const int thr = std::min(tn.coarse >= 0 ? tn.coarse : 40, CO_MAXSIDE);
    int lc = 1;
    while (lc < L && std::max(lw[lc], lh[lc]) > thr) ++lc;
    if (thr > 0 && o.blur_kind == 0 && !s.blur_skip && lc <= L - 2 && L - lc <= CO_MAXL) s.coarse_from = lc;
    s.stamp_co = s.coarse_from > 0 && st.co;
    return L;
}

// ---- a call's form ----------------------------------------------------------------------------------------------------------------
enum Sweep : uint8_t {
    SW_NONE,     // the level is not reduced by itself: from coarse_from on, or the top
    SW_BATCH,    // k_vv_x_fwd, then the fused anticausal-x + causal-y sweep of row bands as pipeline stages (k_vv_xbyf)
    SW_LONE,     // the separate Van Vliet sweeps (k_sweeps.inc, k_sweeps1.inc), with k_vv_xby_m where `xby`
    SW_DERICHE,  // a copy and k_deriche per direction
};
enum XFwd : uint8_t { XF_COPY, XF_FWD, XF_M };  // G -> T as it stands (no x sweep) | k_vv_x_fwd, CKPT where `rcmp` | k_vv_x_m<true>; the source form where `src0`
enum XBwd : uint8_t { XB_NONE, XB_M, XB_BWD };  // in the fused sweep, or no x sweep | k_vv_x_m<false> | k_vv_x_bwd
enum YFwd : uint8_t { YF_NONE, YF_M, YF_FWD1S, YF_FWD1, YF_FWD };  // in the fused sweep, or no y sweep | k_vv_y_m | k_vv_y_fwd1s | k_vv_y_fwd1 | k_vv_y_fwd
enum YBwd : uint8_t { YB_NONE, YB_DEC, YB_DEC7, YB_BWD };  // no y sweep | k_vv_y_bwd_dec<rowz, YST, dec_zt, dec_odd> | k_vv_y_bwd_dec7<dec_odd> | k_vv_y_bwd

struct LevelForm {
    // REDUCE of the level (l < l_end)
    uint8_t sweep, x_fwd, x_bwd, y_fwd, y_bwd;
    bool do_x, do_y;
    bool rcmp;       // batch: the fused sweep re-runs the causal x sweep from checkpoints (MODE 1; MODE 2 where src0)
    bool stamp;      // batch: the diagnostic instance of k_vv_xbyf
    bool xby;        // lone: anticausal x and causal y in ONE launch of five-wavefront bands (k_vv_xby_m)
    bool src0;       // the causal x sweep evaluates level 0 from the frames
    bool mask_l0;    // level 0 with the implicit mask
    bool odd_dec;    // an odd width decimates inside the anticausal y sweep too
    bool zt, rowz;   // zero-tile flags of T; a chunk of YCH rows may straddle bands
    bool per_plane;  // blocks of the x sweeps: per-plane bands (Bands), or 64 stacked lines
    bool g_in, g_out, mr_in, mr_out;  // G column flags / mask-row flags of this level (read) and of the next (written)
    bool fill_mask;  // T flags of the mask plane mean "repeats row 0"
    bool dec_zt, dec_odd;  // template arguments of the decimating sweep
    bool decimate;   // k_decimate behind the sweeps
    int NR, NC, nbx;  // 64-row bands per plane, tile columns, blocks of the x sweeps
    // collapse of the level
    int crows, xa, xb;  // rows per strip; columns [xa, xb) four per work-item
    bool gen, px, c_mr;  // per-lane tap offsets; k_collapse_px for the rest; the MR instances
};

struct CallForm {
    int n, l_end;
    bool src, a_dense;
    bool wf_ctrl;  // the call clears the band-queue heads first and fetches the sticky time-out count last
    bool coarse, coarse_lds;
    int c4_lock, c4_swizzle;
    LevelForm lv[32];
};

// Van Vliet sweeps of a call take the chain + loader + storer kernels for `blocks` blocks
inline bool chain3(const PlanShape& s, long blocks, bool src0 = false) {
    return s.tune.mover != 0 && (blocks <= CHAIN3_BLOCKS || (src0 && blocks <= CHAIN3_BLOCKS_SRC));
}

// The fused anticausal-x + causal-y sweep of a call with n pairs: a per-CALL choice, like source fusion.  The band pipeline pays where
// a launch has many bands in flight to hide its fill: a batched plan asked for one pair runs the separate sweeps, which are faster for a
// lone pair (3.0 against 3.4 ms at 6144 x 4096) -- unless STITCH_WAVEFRONT or STITCH_SINGLE_FAST pins the form.
// (Until round 4 one pair that fills the chip -- config 5 -- took the batch's sweep too; the five-wavefront form with zero-tile flags is 2.6 %
// faster there, 22.3 against 22.9 ms per pair.  STITCH_XBYM=0 brings the old choice back.)
inline bool batch_sweep_call(const PlanShape& s, int n) {
    return s.tune.wavefront >= 0 || s.tune.single_fast > 0 || n >= 2 || (s.tune.xbym == 0 && chip_filling(s.lv[0].h));
}

// One pair in flight: the anticausal x and the causal y sweep of level l as ONE launch of five-wavefront bands (k_vv_xby_m) where the
// separate launches are bound by their bytes -- from STITCH_XBYM_MPIX megapixels per plane (default 20: 6144 x 4096).  Below that a level's time is
// its chain of rows and columns either way, and the fused form adds a hand-off per 64-row band.  STITCH_XBYM=0: never; =1: the first
// four levels of every lone pair, whatever their size (tests).  Levels shrink: level 0 qualifies whenever any level does.
inline bool lone_fused_level(const PlanShape& s, int n, int l) {
    const Level& a = s.lv[l];
    const long mpix = s.tune.xbym > 0 ? 0 : s.tune.xbym_mpix >= 0 ? s.tune.xbym_mpix : 20;
    return n == 1 && s.has_wf && l < 4 && s.opts.blur_kind == 0 && !s.blur_skip && s.tune.mover != 0 && s.tune.xbym != 0 && a.w > 1 && a.h > 1 &&
           (long)a.w * a.h >= mpix * 1000000L && tiles(a.h) < 4095 && !batch_sweep_call(s, n);
}

// Source fusion trades bytes for instructions: the consumers of level 0 gather their samples (64 four-byte gathers per lane and
// tile in the causal x sweep) instead of streaming planes.  A launch sequence over several pairs is bound by the bytes it moves
// and gains (12 % at config 2); ONE pair in flight is bound by the length of its recurrence chains, its sweeps have a SIMD to
// themselves, and the gathers land on the critical path: measured at 4421 x 2315 / 1081 x 527, materialised S1 2.14 / 0.81 ms,
// source-fused 2.27 / 0.84 ms per pair.  So the form is chosen per CALL: source-fused for launch sequences with enough canvas
// in them, materialised (k_compose / k_load_canvases; the implicit mask stays) otherwise.  STITCH_SINGLE_FAST=1 pins the fused
// forms everywhere (A/B runs, tests).
// Measured per launch sequence of n pairs, 1 and 4 sequences in flight (scripts/experiments/exp_srcfuse_n.py, ms per pair, fused /
// materialised): 1081 x 527: n = 2 0.255 / 0.239, n = 8 0.053 / 0.047 (4 in flight), n = 16 0.040 / 0.046; 4421 x 2315: n = 2
// 0.597 / 0.858 (4 in flight), n = 8 0.500 / 0.588.  The fused form pays from about 8 MPix of canvas per launch sequence.
// (A lone pair that fills the chip by itself is a throughput case too: 23.5 ms source-fused against 25.9 ms materialised.)
// What the caller's buffers add (32-bit offsets, an output that overlaps an input) is the caller's to check: `src` of call_form.
inline bool source_fused_call(const PlanShape& s, int n) {
    if (!s.src_fuse) return false;
    if (s.tune.single_fast > 0) return true;
    if (chip_filling(s.lv[0].h)) return true;
    // (round 4) one pair too: with the gathers on a loader wavefront (k_vv_x_m<.., SRC>) they are off the recurrence's issue stream,
    // and level 0 of a canvas this size is bound by bytes even alone.  STITCH_SRC_LONE_MPIX moves the threshold (0 = never).
    const long long lone_px = s.tune.src_lone >= 0 ? 1000000LL * s.tune.src_lone : 8000000LL;
    if (n == 1) return s.tune.mover != 0 && lone_px > 0 && (long long)s.lv[0].w * s.lv[0].h >= lone_px && s.opts.blur_kind == 0;
    return (long long)n * s.lv[0].w * s.lv[0].h >= 8000000LL;
}

// odd widths decimate inside the anticausal sweep too (three overlaps per output column); a width of 1 has no next level column
inline bool odd_decimate(const PlanShape& s, int l) {
    return (s.lv[l].w & 1) != 0 && s.lv[l].w >= 3 && !s.no_fuse && s.tune.odd_dec != 0;
}
// the anticausal y sweep of level l decimates (k_vv_y_bwd_dec, k_vv_y_bwd_dec7)
inline bool fused_decimate(const PlanShape& s, int l) { return !s.no_fuse && ((s.lv[l].w & 1) == 0 || odd_decimate(s, l)); }
// Zero-tile flags of T at level l, given a sweep that writes them (k_vv_xbyf, k_vv_xby_m): only where all three users run -- the causal
// x sweep, the fused sweep, the fused anticausal-y + decimation
inline bool zero_tile_level(const PlanShape& s, int l) {
    const Level& a = s.lv[l];
    return s.zero_tiles && tiles(a.h) <= ZT_MAX_BANDS && fused_decimate(s, l) && !(s.tune.gate64 && (a.h % TS || (a.w & 1)));
}

// stitch_plan_fast_paths: what the workspace was built for, whatever a call makes of it
inline int capability_mask(const PlanShape& s) {
    int f = 0;
    if (s.mask_opt) f |= STITCH_FAST_IMPLICIT_MASK;
    if (s.src_fuse) f |= STITCH_FAST_SOURCE_FUSED;
    if (s.wf_levels > 0) f |= STITCH_FAST_FUSED_SWEEP;
    if (s.wf_levels > 0 && zero_tile_level(s, 0)) f |= STITCH_FAST_ZERO_TILES;
    if (s.opts.blur_kind == 0 && !s.blur_skip && s.L >= 2 && fused_decimate(s, 0) && s.lv[0].h > 1) f |= STITCH_FAST_FUSED_DECIMATE;
    if (s.coarse_from > 0) f |= STITCH_FAST_COARSE_LEVELS;
    return f;
}

// Rows per strip of the collapse of level l in a call with n pairs.  A strip is one serial chain of rows per work-item (load -> arithmetic ->
// store, one row after the other) and re-uses the x-interpolated source rows best when it is long: 32 rows wherever the launch has
// workgroups enough to hide that chain behind each other -- every batch.  A launch with few workgroups lives on the chains alone: the
// strip of a ONE-pair call is halved until the launch has STITCH_CROWS_WGS workgroups (default 8192; 0 = round 3's rule: by the level's height alone) or
// is 4 rows high (one pair in flight, 6144 x 4096: level 0 32 -> 8 rows, levels >= 1 32 -> 4: 2.41 -> 2.33 ms; 4421 x 2315 1.30 -> 1.25;
// the rows two strips share are read once more per halving, which a lone pair does not notice).  STITCH_CROWS_L0 / _LN pin the height.
inline int collapse_rows(const PlanShape& s, int l, int n) {
    const Level& a = s.lv[l];
    int c;
    if (l == 0) {
        if (s.tune.crows_l0 >= 0) return s.crows_l0;
        c = a.h >= 2048 ? s.crows_l0 : a.h >= 1024 ? 16 : 8;
    } else {
        if (s.crows_ln > 0) return s.crows_ln;
        c = std::max(4, std::min(4 * CROWS, a.h / 32));
    }
    const long want = s.tune.crows_wgs >= 0 ? s.tune.crows_wgs : 8192;
    const long blocks = std::max(1, (a.c4_xb - a.c4_xa) / 256);
    // (one pair per call only: a batch has other workgroups to run meanwhile, and with four 4-pair sequences in flight shorter strips
    // measured 5 % slower, scripts/experiments/r4_run36.sh)
    while (n == 1 && c > 4 && blocks * ((a.h + c - 1) / c) < want) c /= 2;
    return c;
}

// Every coarse level in LDS where they fit (k_coarse_lds): G of all levels, the blur scratch, the collapse chain; rows pitched odd.
// Fills the float offsets of the levels (CoarseLds) and returns the floats taken; *fits: tables and planes fit the kernel's arrays.
inline size_t coarse_lds_layout(const PlanShape& s, int* p, int* g, int* e, int* t, bool* fits) {
    const int nl = s.L - s.coarse_from;
    int fl = 0, tabs_w = 0, tabs_h = 0;
    for (int i = 0; i < nl; ++i) {
        const Level& v = s.lv[s.coarse_from + i];
        p[i] = v.w | 1;
        g[i] = fl;
        fl += 7 * v.h * p[i];
        e[i] = fl;
        fl += 3 * v.h * p[i];
        if (i + 1 < nl) tabs_w += v.w, tabs_h += v.h;
    }
    *t = fl;
    fl += 7 * s.lv[s.coarse_from].h * p[0];
    *fits = sizeof(float) * (size_t)fl <= (size_t)CO_LDS_BYTES && tabs_w <= CO_TABN && tabs_h <= CO_TABN;
    return (size_t)fl;
}

// Step 1: the sweep family of level l and its T flags
inline void level_sweep(const PlanShape& s, int n, bool src, int l, LevelForm& f) {
    const Level& a = s.lv[l];
    const int np = 7 * n;
    f.do_x = a.w > 1 && !s.blur_skip;
    f.do_y = a.h > 1 && !s.blur_skip;
    f.NR = tiles(a.h);
    f.NC = tiles(a.w);
    f.src0 = src && l == 0;
    f.mask_l0 = l == 0 && s.mask_opt;
    f.odd_dec = odd_decimate(s, l);
    const bool both = f.do_x && f.do_y;
    if (s.opts.blur_kind != 0)
        f.sweep = SW_DERICHE;
    else
        f.sweep = both && l < s.wf_levels && batch_sweep_call(s, n) ? SW_BATCH : SW_LONE;
    f.xby = f.sweep == SW_LONE && both && lone_fused_level(s, n, l);
    f.stamp = f.sweep == SW_BATCH && s.stamp_wf && l == 0;
    f.rcmp = f.sweep == SW_BATCH && (s.recompute == 1 || (s.recompute == 2 && l >= 1)) && !f.stamp;
    // (the five-wavefront sweep of ONE pair carries the flags too where its x sweeps are the one-wavefront kernels anyway -- more bands
    // than the chain + loader + storer form takes: a pair of config 5's size)
    const bool writes_zt = f.sweep == SW_BATCH || (f.xby && s.has_zt && f.NC <= XY_MAXNC && !chain3(s, (long)np * f.NR, f.src0));
    f.zt = writes_zt && zero_tile_level(s, l);
    f.rowz = f.zt && (a.h % YCH) != 0;
}

// Step 2, the producer: the decimating sweep of level l can record all-zero tile columns of G_{l+1} -- k_vv_y_bwd_dec with T flags behind
// the batch's fused sweep, even width (the ODD instance advances by 63 columns; k_decimate's level has no T flags)
inline bool produces_flags(const PlanShape& s, int l, const LevelForm& f) { return f.sweep == SW_BATCH && f.zt && (s.lv[l].w & 1) == 0; }
// Step 2, the readers of G_l's column flags.  The x sweep of l must be plain k_vv_x_fwd: not its CKPT form nor k_vv_xbyf MODE 1, which
// fetch G_l again (no flags under STITCH_RECOMPUTE, nor in the stamped diagnostic build); not k_vv_x_m, which a small batch takes at an
// unfused level; not the copy of a width of 1.  The collapse (k_collapse4 / k_collapse / k_collapse_px of levels l-1 and l, all three)
// reads a flagged column from the level's slack rows, at a 32-bit offset from its plane: levels beyond that are left alone.  k_coarse
// and k_blend_top (levels from l_end on), the band path and the coarse levels of a split pair (planes_in) do not know the flags.
inline bool reads_flags(const PlanShape& s, int n, int l, const LevelForm& f) {
    const Level& b = s.lv[l];
    if (l >= s.l_end() || s.mask_stored() || s.recompute != 0 || s.stamp_wf || !f.do_x) return false;
    if (f.sweep != SW_BATCH && (f.sweep != SW_LONE || chain3(s, 7L * n * f.NR))) return false;
    return 7ull * s.cap * b.ps + 64ull * b.pitch < (1ull << 32);  // (in samples)
}

// The form of a call with n pairs (1 <= n <= cap) on a plan of shape s; src: level 0 is evaluated from the frames (source_fused_call
// and the caller's buffers allow it); a_dense: a blend of two dense canvases.  No allocation; decided once, before the first launch.
inline CallForm call_form(const PlanShape& s, int n, bool src, bool a_dense) {
    CallForm c{};
    c.n = n;
    c.l_end = s.l_end();
    c.src = src;
    c.a_dense = a_dense;
    c.wf_ctrl = s.wf_levels > 0 || lone_fused_level(s, n, 0);
    c.c4_lock = std::max(0, s.tune.c4_lock);
    c.c4_swizzle = s.tune.c4_swz < 0 ? 1 : s.tune.c4_swz;
    const int np = 7 * n;
    for (int l = 0; l < c.l_end; ++l) level_sweep(s, n, src, l, c.lv[l]);
    // Steps 2 and 3.  G column flags of levels 1 and 2: on where the level above produces them and this level reads them.
    // Row-repeat flags of the mask plane ride on them: the same producer launch below a level of even width AND even height (below an odd
    // height the decimation's overlap weights change from row to row and the rows do not repeat), on a plane whose T flags mean "repeats
    // row 0": level 0 with the implicit mask recorded in the flags, level 1 with these flags of its own.  The same readers: k_vv_x_fwd takes
    // a flagged tile from row 0 (at a fused level a band flagged throughout is skipped), k_vv_xbyf MODE 0 records such a band as a constant
    // band, k_vv_y_bwd_dec with fill_l0 re-reads row 0 of T for a flagged lane, the collapse's MR instances take the mask sample from row 0.
    // An unfused level 2 (a large batch) only redirects: k_vv_x_bwd, k_vv_y_fwd1 and its k_vv_y_bwd_dec work on T, which is stored in full.
    // STITCH_NO_G_FLAGS / STITCH_NO_MASK_ROWS (compile time, A/B libraries): never.  STITCH_NO_ZERO_TILES=1 turns all flags off.
    for (int l = 0; l < c.l_end; ++l) {
        LevelForm& f = c.lv[l];
        f.fill_mask = f.zt && (l == 0 ? f.mask_l0 : f.mr_in);
        if (l + 1 < c.l_end && l < 2) {
            LevelForm& nx = c.lv[l + 1];
#ifndef STITCH_NO_G_FLAGS
            f.g_out = nx.g_in = s.has_gz[l] && produces_flags(s, l, f) && reads_flags(s, n, l + 1, nx);
#endif
#ifndef STITCH_NO_MASK_ROWS
            f.mr_out = nx.mr_in = f.g_out && s.has_mr[l] && f.fill_mask && (s.lv[l].h & 1) == 0;
#endif
        }
    }
    // Step 4: the kernels
    for (int l = 0; l < c.l_end; ++l) {
        LevelForm& f = c.lv[l];
        const Level& a = s.lv[l];
        const long lines = (long)np * a.h;
        // blocks of the x sweeps: per-plane bands wherever a block's treatment depends on its plane (implicit mask, source-fused
        // level 0, flags), 64 stacked lines otherwise (fewer blocks when planes are shorter than 64 rows)
        f.per_plane = f.mask_l0 || f.src0 || f.zt || f.g_in;
        f.nbx = f.per_plane ? np * f.NR : (int)((lines + TS - 1) / TS);
        f.dec_zt = f.sweep == SW_BATCH || f.zt;
        f.dec_odd = (a.w & 1) != 0;
        const YBwd y_dec = fused_decimate(s, l) ? YB_DEC : YB_BWD;
        if (f.sweep == SW_BATCH) {
            f.x_fwd = XF_FWD;
            f.y_bwd = y_dec;
        } else if (f.sweep == SW_LONE) {
            // few enough blocks for a workgroup of three wavefronts each (chain, loader, storer: k_sweeps1.inc) to find SIMDs of its own:
            // the recurrence alone on one wavefront, the tiles' traffic -- and, at a source-fused level 0, the gathers -- on the others
            const bool x3 = f.do_x && !f.zt && !f.g_in && chain3(s, f.nbx, f.src0);
            f.x_fwd = !f.do_x ? XF_COPY : x3 ? XF_M : XF_FWD;
            f.x_bwd = !f.do_x || f.xby ? XB_NONE : x3 && chain3(s, f.nbx) ? XB_M : XB_BWD;
            if (f.do_y) {
                // fewer than 1.5 wavefronts per SIMD: the launch's time is one wavefront's chain of rows, i.e. its instructions per
                // row (k_sweeps1.inc): one column per work-item, rows through scalar offsets, the decimation on three consumer wavefronts
                const bool lone = (long)((a.pitch + YCOLS - 1) / YCOLS) * np < Y_LONE_WGS && !s.tune.y2, small_plane = a.ps * sizeof(float) < 0x7fffffffULL;
                // (k_vv_y_fwd1s: 56 rows in flight; a sweep that moves more than ~1 GB is bound by bytes and streams better on flat addresses:
                // 4421 x 2315 level 0 129 -> 98 us, 6144 x 4096 level 0 266 -> 271)
                const bool y1s = lone && small_plane && s.tune.y1s != 0 && (s.tune.y1s >= 2 || a.ps * np * sizeof(float) * 2 < (1000u << 20));
                f.y_fwd = f.xby ? YF_NONE : lone && chain3(s, (long)(a.pitch / TS) * np) ? YF_M : y1s ? YF_FWD1S : lone ? YF_FWD1 : YF_FWD;
                // loader + two chains + four consumers, free-running (k_vv_y_bwd_dec7) where the launch leaves SIMDs idle; the two-wavefront
                // kernel otherwise, and wherever T has flags
                f.y_bwd = y_dec == YB_DEC && !f.zt && lone && small_plane && s.tune.dec7 != 0 ? YB_DEC7 : y_dec;
            }
        }
        f.decimate = f.y_bwd == YB_NONE || f.y_bwd == YB_BWD;
    }
    if (s.coarse_from > 0) {
        int p[CO_MAXL], g[CO_MAXL], e[CO_MAXL], t;
        bool fits;
        coarse_lds_layout(s, p, g, e, &t, &fits);
        c.coarse = true;
        c.coarse_lds = s.tune.coarse_lds != 0 && !s.stamp_co && fits;
    }
    // the collapse: four columns per work-item on the column range whose taps follow the regular pattern (Level::c4_xa, c4_xb), one
    // column per work-item on the rest, in ONE launch (k_collapse4); levels without such a range run k_collapse, or -- levels >= 1 of a
    // launch that leaves most SIMDs with at most a wavefront or two -- k_collapse_px
    for (int l = 0; l < c.l_end; ++l) {
        LevelForm& f = c.lv[l];
        const Level& a = s.lv[l];
        f.crows = collapse_rows(s, l, n);
        if (s.collapse4) f.xa = a.c4_xa, f.xb = a.c4_xb;
        f.gen = a.c4_gen && s.collapse4;
        f.px = l >= 1 && (long)n * a.pitch * a.h <= 4096L * 64 * 2 && s.tune.collapse_px != 0;
        f.c_mr = f.mr_in;
    }
    return c;
}

// ---- the mask pyramid that stands (include/stitch_mask_keep.h) --------------------------------------------------------------------
// The mask planes of G_1 .. G_{l_end} of a slot, their row-repeat flags and the level-0 blur handed down to them are a function of the
// slot's seam record, the plan and the call's FORM: which tiles of a mask plane are stored at all (under mr_out a flagged tile is not, and
// the memory keeps what an earlier call left), which flags exist.  The form word states that part of a call; a slot's pyramid stands only
// under the word it was written under, and only where the word has MK_KEEP_OK: every kernel between G_l and G_{l+1} that the call's
// LevelForms select knows the skip (mask_stands, k_sweeps.inc).  A call without MK_KEEP_OK computes every mask plane and, because it
// stores everything its own form stores, takes the slots' records over with its own word -- under which nothing ever stands.
constexpr uint32_t MK_KEEP_OK = 1u, MK_MASK_L0 = 2u;
constexpr int MK_LEVEL_BIT = 2, MK_LEVELS = 8, MK_LEND_BIT = MK_LEVEL_BIT + 3 * MK_LEVELS;  // three bits per level below MK_LEVELS, then l_end (< 32)
constexpr uint32_t mask_keep_level_bits(bool mr_out, bool mr_in, bool fill_mask) { return (mr_out ? 1u : 0u) | (mr_in ? 2u : 0u) | (fill_mask ? 4u : 0u); }
// REDUCE of a level runs only kernels that know the skip: the batch's k_vv_x_fwd + k_vv_xbyf MODE 0 (plain and STAMP) + k_vv_y_bwd_dec, or
// the separate sweeps -- k_vv_x_fwd / k_vv_x_bwd or k_vv_x_m, k_vv_y_fwd / k_vv_y_fwd1 / k_vv_y_fwd1s / k_vv_y_m, k_vv_y_bwd_dec /
// k_vv_y_bwd_dec7 or k_vv_y_bwd + k_decimate: the coarser levels of a large batch take the few-workgroup forms too (a copy in place of
// an x sweep and k_vv_y_bwd touch the scratch T alone).  Not the five-wavefront sweep of one pair in flight (k_vv_xby_m), not the
// STITCH_RECOMPUTE modes, not Deriche.
inline bool mask_keep_level(const LevelForm& f) {
    if (f.sweep == SW_BATCH) return !f.rcmp && f.x_fwd == XF_FWD && (f.y_bwd == YB_DEC || f.y_bwd == YB_BWD);
    return f.sweep == SW_LONE && !f.xby && !f.rcmp;
}
// The form word of a call.  pathed: the mask plane comes from seam paths (k_mask_path), by another rule than the record's.
inline uint32_t mask_keep_word(const PlanShape& s, const CallForm& c, bool pathed) {
    uint32_t w = ((uint32_t)c.l_end & 31u) << MK_LEND_BIT;
    bool ok = !pathed && !s.mask_stored() && c.l_end >= 1 && c.lv[0].mask_l0;  // the implicit level-0 mask: no k_mask, nothing of the mask at level 0 in memory
    if (c.l_end >= 1 && c.lv[0].mask_l0) w |= MK_MASK_L0;
    for (int l = 0; l < c.l_end; ++l) {
        const LevelForm& f = c.lv[l];
        const uint32_t b = mask_keep_level_bits(f.mr_out, f.mr_in, f.fill_mask);
        if (l < MK_LEVELS)
            w |= b << (MK_LEVEL_BIT + 3 * l);
        else if (b)
            ok = false;  // (call_form sets these bits below level 4 only: the flags of levels 1 and 2, T flags of the fused levels)
        ok = ok && mask_keep_level(f);
    }
#ifdef STITCH_NO_MASK_KEEP  // (the A/B library: every mask plane on every call)
    ok = false;
#endif
    return ok ? w | MK_KEEP_OK : w;
}

// ---- the band path: ONE pair split into row bands over ranks (stitch_band.inc) ---------------------------------------------------
// What a band of a cw x ch canvas holds (BandShape, band_shape) and what each entry point launches at each level (BandForm, band_form).
// The split levels l < Ls are reduced and collapsed band by band by the caller's sequence of operations (pipeline.BandStitcher.steps);
// the levels from Ls up run through an ordinary plan whose level 0 is handed in (plan_shape with planes_in).
struct BandLevel {
    int w = 0, h_full = 0, rows = 0, row0 = 0, pitch = 0;
    int halo = 0;   // halo rows either side: BAND_HALO on levels >= 1 (sources of an EXPAND) of a band with neighbours, else none
    size_t ps = 0;  // plane stride in floats: pitch * (rows + 2 * halo)
    int c4_xa = 0, c4_xb = 0;  // as Level's
    int sh_eff = 0;  // the source height the collapse's `iy < sh - 1 ? iy + 1 : iy` clamps at: the LEVEL's last row only
    // device addresses, null in a bare shape
    float* g = nullptr;  // 7 planes (base = first halo row); origin = g + halo * pitch
    float* e = nullptr;  // 3 planes, levels 1..Ls-1
    int32_t *ix = nullptr, *iy = nullptr;  // resize tables level+1 -> level, rows in band-local source coordinates
    double *ax = nullptr, *ay = nullptr;
    int ph() const { return rows + 2 * halo; }  // rows per plane in memory
    float* origin_g() const { return g + (size_t)halo * pitch; }
    float* origin_e() const { return e + (size_t)halo * pitch; }
};

struct BandShape {
    int cw = 0, ch = 0, rank = 0, nranks = 1, Ls = 0, L = 0;
    BandLevel lv[32];  // 0..Ls (level Ls: this rank's band of the first replicated level, the decimation's output)
    // the switches read at creation
    bool zero_tiles = true;  // STITCH_NO_ZERO_TILES
    bool src_l0 = true;      // level 0 source-fused (index plane + gathers, implicit mask) or, STITCH_BAND_PLANES=1, seven stored planes
    bool plain_dec = false;  // STITCH_BAND_PLAIN=1: anticausal y sweep and decimation as two kernels (A/B)
};
// (the one writer of the field after band_shape: stitch_band_set_level0's value arrives here with the next compose)
inline void band_set_src_l0(BandShape& s, bool source_fused) { s.src_l0 = source_fused; }

enum BandRefusal { BAND_OK = 0, BAND_BAD_RANK, BAND_BAD_PYRAMID, BAND_BAD_SPLIT, BAND_BAD_ROWS, BAND_BAD_WIDTH, BAND_BAD_HALO };
struct BandWhy {  // what the refusal's message names
    int level = 0, row = 0, src_a = 0, src_b = 0;
};

// The y tables of the EXPAND of level l+1 into this band's rows of level l: the reference's tables for the whole level
// (CImg.h:29625-29637), rows re-based to what this rank holds of level l+1 -- its band with its halo rows (source row 0 of the buffer =
// row0_{l+1} - halo), or all rows when l+1 is the first replicated level.  Returns the first row whose taps leave what the rank holds
// (*why names it), or -1.
inline int band_row_table(const BandShape& s, int l, std::vector<int32_t>& iy, std::vector<double>& ay, BandWhy* why = nullptr) {
    const BandLevel &v = s.lv[l], &nx = s.lv[l + 1];
    std::vector<int32_t> idx;
    std::vector<double> al;
    expand_table(nx.h_full, v.h_full, idx, al);
    const bool top_src = l + 1 == s.Ls;
    const int src_base = top_src ? 0 : nx.row0 - nx.halo, src_rows = top_src ? nx.h_full : nx.ph();
    iy.resize(v.rows);
    ay.assign(al.begin() + v.row0, al.begin() + v.row0 + v.rows);
    int bad = -1;
    for (int y = 0; y < v.rows; ++y) {
        const int gi = idx[v.row0 + y], gi2 = gi < nx.h_full - 1 ? gi + 1 : gi;
        iy[y] = gi - src_base;
        if (bad < 0 && (iy[y] < 0 || gi2 - src_base >= src_rows)) {
            bad = y;
            if (why) *why = BandWhy{l, v.row0 + y, gi, gi2};
        }
    }
    return bad;
}

// Fills the shape of rank `rank` of `nranks` of a cw x ch canvas whose first `split_levels` levels are split (the root variant's pyramid:
// level_rule 0).  Rank r owns rows [r * h_l / N, (r + 1) * h_l / N) of every split level: even row counts, so that the 2:1 decimation
// never straddles two ranks, and at least 2 * BAND_HALO of them.  A refusal leaves *why for the message.
inline BandRefusal band_shape(BandShape& s, int cw, int ch, int rank, int nranks, int split_levels, bool zero_tiles, bool src_l0, bool plain_dec,
                              BandWhy* why = nullptr) {
    BandWhy w0;
    BandWhy& y = why ? *why : w0;
    if (nranks < 1 || rank < 0 || rank >= nranks) return BAND_BAD_RANK;
    int lw[32], lh[32];
    const int L = pyramid_sizes(cw, ch, 0, lw, lh);
    if (L <= 0) return BAND_BAD_PYRAMID;
    const int Ls = split_levels;
    y.level = L;
    if (Ls < 1 || Ls > L - 1) return BAND_BAD_SPLIT;
    for (int l = 0; l <= Ls; ++l) {
        const int q = l < Ls ? 2 * nranks : nranks;  // split levels: even band heights (the 2:1 decimation stays inside a band)
        y.level = l, y.row = lh[l], y.src_a = lw[l];
        if (lh[l] % q != 0 || lh[l] / nranks < (l < Ls ? 2 * BAND_HALO : 1)) return BAND_BAD_ROWS;
        if (lw[l] < 2) return BAND_BAD_WIDTH;
    }
    s = BandShape{};
    s.cw = cw, s.ch = ch, s.rank = rank, s.nranks = nranks, s.Ls = Ls, s.L = L;
    s.zero_tiles = zero_tiles, s.plain_dec = plain_dec;
    band_set_src_l0(s, src_l0);
    for (int l = 0; l <= Ls; ++l) {
        BandLevel& v = s.lv[l];
        v.w = lw[l], v.h_full = lh[l], v.rows = lh[l] / nranks, v.row0 = rank * v.rows, v.pitch = round_up(v.w, 64);
        v.halo = l == 0 || nranks == 1 ? 0 : BAND_HALO;  // a band without neighbours has nobody's rows to hold
        v.ps = (size_t)v.pitch * v.ph();
    }
    std::vector<int32_t> idx;
    std::vector<double> al;
    for (int l = 0; l < Ls; ++l) {
        BandLevel& v = s.lv[l];
        const BandLevel& nx = s.lv[l + 1];
        expand_table(nx.w, v.w, idx, al);
        regular_range(idx, v.w, nx.w, nx.h_full, &v.c4_xa, &v.c4_xb);
        v.sh_eff = l + 1 == Ls ? nx.h_full : (rank == nranks - 1 ? nx.rows + nx.halo : (1 << 30));
        if (band_row_table(s, l, idx, al, &y) >= 0) return BAND_BAD_HALO;
    }
    return BAND_OK;
}

// Zero-tile flags of T at level l of a band, as in a plan and under its conditions: every user of T is a fused form (so only behind
// BO_XY_FWD), the two finest levels, an even width, at most ZT_MAX_BANDS bands per plane; and no halo rows (the flags know a plane of
// `rows` rows), the fused decimation (the two-kernel form reads every tile), level 0 only as the index plane.  The same condition
// holds for the index plane's own flags at level 0 (zi).
inline bool band_zero_tile_level(const BandShape& s, int l) {
    const BandLevel& a = s.lv[l];
    return l < 2 && (l > 0 || s.src_l0) && (a.w & 1) == 0 && tiles(a.rows) <= ZT_MAX_BANDS && a.halo == 0 && s.zero_tiles && !s.plain_dec;
}

// The entry points of a band that launch (stitch.h: stitch_band_compose_*, _reduce_x, _reduce_xy_fwd, _reduce_y_fwd, _reduce_y_fwd_cols,
// _reduce_y_bwd, _reduce_y_bwd_cols, _collapse_*)
enum BandOp : uint8_t { BO_COMPOSE, BO_X, BO_XY_FWD, BO_Y_FWD, BO_Y_FWD_COLS, BO_Y_BWD, BO_Y_BWD_COLS, BO_COLLAPSE };

// The level whose T flags are live behind `op` at `level`, given the level whose flags were live before (-1: none).  One buffer: a
// level's flags live from the causal x sweep of its BO_XY_FWD to its anticausal y sweep; the separate x sweeps leave none.
inline int band_zt_after(const BandShape& s, int zt_live, BandOp op, int level) {
    if (op == BO_XY_FWD && band_zero_tile_level(s, level)) return level;
    if ((op == BO_X || op == BO_XY_FWD) && zt_live == level) return -1;
    return zt_live;
}

struct DecInstance {  // k_vv_y_bwd_dec<rowz, YST, zt, odd, xch>
    bool rowz, zt, odd, xch;
};

struct BandForm {
    bool admitted;  // the level takes the operation in this form (one plane at a time: stored planes; column chunks: the fused decimation)
    int zt_after;   // band_zt_after
    // BO_X, BO_XY_FWD: the x sweeps (k_vv_x_fwd, k_vv_x_bwd); BO_COMPOSE: zi alone
    bool src0;       // level 0 from the frames through the index plane, the mask implicit (every operation: MaskL0 goes with it)
    bool zi;         // the index plane's zero-tile flags
    bool per_plane;  // blocks: per-plane bands (Bands{bands_nr, bands_h}), or 64 stacked lines
    int nbx, bands_nr, bands_h;
    bool zt;         // T flags: written by BO_XY_FWD, read by BO_Y_BWD / BO_Y_BWD_COLS
    // BO_XY_FWD: the fused sweep (k_vv_xbyf)
    bool banded;     // the BANDED instance: halo rows or a resume state (it carries more scalars through the tile loop, a few per cent slower)
    int NR, NC, wgs;
    // the y sweeps
    int np;          // planes per launch
    bool xch;        // a column range with the chunk's own state arrays
    uint8_t y_bwd;   // YB_DEC, or YB_BWD with k_decimate behind it
    DecInstance dec;
    bool decimate;
    // BO_COLLAPSE
    int crows, strips, cols, xa, xb;  // [xa, xb): before the caller's addresses clamp it
    bool top_src;    // the source level is the replicated one: all rows, dense planes
};

// What `op` launches at `level`; zt_live: the level whose T flags are live (the band's state); plane: -1 all seven, or one (BO_Y_FWD, BO_Y_BWD).
inline BandForm band_form(const BandShape& s, BandOp op, int level, int zt_live = -1, int plane = -1) {
    BandForm f{};
    const BandLevel& a = s.lv[level];
    const bool zt_on = band_zero_tile_level(s, level);
    f.admitted = true;
    f.zt_after = band_zt_after(s, zt_live, op, level);
    f.src0 = level == 0 && s.src_l0;
    f.zi = f.src0 && zt_on;
    f.NR = tiles(a.rows);
    f.NC = tiles(a.w);
    f.np = plane < 0 ? 7 : 1;
    switch (op) {
    case BO_COMPOSE:
        break;
    case BO_XY_FWD:
        f.zt = zt_on;
        // a level without halo rows that starts at the image's first row is exactly a plan's launch: the plain instance
        f.banded = a.halo != 0 || s.rank > 0;
        f.wgs = (int)std::min<long>(7L * f.NR, WF_MAX_WGS);
        [[fallthrough]];
    case BO_X:  // halo rows are swept along x too (their contents are never used)
        f.per_plane = f.src0 || f.zt;  // a block's treatment depends on its plane
        f.bands_nr = tiles(a.ph()), f.bands_h = a.ph();
        f.nbx = f.per_plane ? 7 * f.bands_nr : (int)((7L * a.ph() + TS - 1) / TS);
        break;
    case BO_Y_FWD:
        f.admitted = !(f.src0 && plane >= 0);  // one plane at a time needs the stored planes
        break;
    case BO_Y_FWD_COLS:
        f.xch = true;
        break;
    case BO_Y_BWD:
    case BO_Y_BWD_COLS: {
        const bool fused = (a.w & 1) == 0 && !s.plain_dec;  // (odd widths keep the stand-alone decimation here)
        f.xch = op == BO_Y_BWD_COLS;
        f.admitted = !f.xch || fused;  // the odd-width decimation overlaps workgroups by two columns
        f.zt = zt_live == level && plane < 0 && zt_on;
        f.y_bwd = fused ? YB_DEC : YB_BWD;
        f.decimate = !fused;
        // ZT = true whatever f.zt: the band path has one instance per (rowz, xch) and hands it an empty flag record where there are no
        // flags (the pair path launches the ZT = false instance there)
        f.dec = DecInstance{f.zt && (a.rows % YCH) != 0, true, false, f.xch};
        break;
    }
    case BO_COLLAPSE:
        f.crows = std::max(4, std::min(32, a.rows / 8));  // (a rule of the band's own: by the band's rows, whatever the launch's workgroups)
        f.strips = (a.rows + f.crows - 1) / f.crows;
        f.cols = level == 0 ? a.w : a.pitch;
        f.xa = a.c4_xa, f.xb = a.c4_xb;
        f.top_src = level + 1 == s.Ls;
        break;
    }
    return f;
}

}  // namespace sk
