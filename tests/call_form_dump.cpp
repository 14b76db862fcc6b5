// The pair path's decision (csrc/stitch_call_form.h) on a machine without a GPU, for tests/test_call_form_host.py.
//   call_form_dump dump FILE    one case per line -> one JSON object per line: the plan's shape and the call's per-level records
//   call_form_dump band FILE    one band per line (cw ch rank nranks split_levels zero_tiles src_l0 plain_dec kinds) -> its shape and the
//                               record of every call of the sequence; kinds: see level_calls
//   call_form_dump bandcheck FILE  the grid's canvases -> every admissible band's sequences against the invariants of band_violated
//   call_form_dump check FILE   a grid (lines "w ...", "h ...", "cap ...", "set NAME=VALUE ...") -> every case's records against the
//                               invariants below; prints "cases N violations M" and the first violations
// A case line: cw ch cap n src a_dense sigma blur_kind level_rule planes_in [NAME=VALUE ...]; src -1 = what the library takes for
// buffers that allow source fusion.  NAME is a switch of include/stitch.h without its STITCH_ prefix, VALUE its environment string.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "stitch_call_form.h"

using namespace sk;

Tuning Tuning::from_env() { return unset(); }  // (never called here: switches arrive as numbers)

struct Field {
    const char* name;
    int Tuning::*field;
    bool flag;  // read as "set and > 0"
};
static const Field FIELDS[] = {
    {"WAVEFRONT", &Tuning::wavefront, false}, {"NO_FUSE", &Tuning::no_fuse, true}, {"NO_SRC_FUSE", &Tuning::no_src_fuse, true},
    {"NO_ZERO_TILES", &Tuning::no_zero_tiles, true}, {"CROWS_L0", &Tuning::crows_l0, false}, {"CROWS_LN", &Tuning::crows_ln, false},
    {"COLLAPSE4", &Tuning::collapse4, false}, {"XBYF_WGS", &Tuning::xbyf_wgs, false}, {"XBYF_SPIN_LIMIT", &Tuning::xbyf_spin_limit, false},
    {"XBYF_EARLY", &Tuning::xbyf_early, false}, {"Y2", &Tuning::y2, true}, {"RECOMPUTE", &Tuning::recompute, false},
    {"WAVEFRONT_STAMP", &Tuning::stamp, true}, {"GATE64", &Tuning::gate64, true}, {"COARSE", &Tuning::coarse, false},
    {"SINGLE_FAST", &Tuning::single_fast, false}, {"ODD_DEC", &Tuning::odd_dec, false}, {"C4_GEN", &Tuning::c4_gen, false},
    {"COLLAPSE_PX", &Tuning::collapse_px, false}, {"Y1S", &Tuning::y1s, false}, {"C4_LOCKSTEP", &Tuning::c4_lock, false},
    {"C4_SWIZZLE", &Tuning::c4_swz, false}, {"MOVER", &Tuning::mover, false}, {"SRC_LONE_MPIX", &Tuning::src_lone, false},
    {"DEC7", &Tuning::dec7, false}, {"XBYM", &Tuning::xbym, false}, {"XBYM_MPIX", &Tuning::xbym_mpix, false},
    {"COARSE_LDS", &Tuning::coarse_lds, false}, {"PITCH_PAD", &Tuning::pitch_pad, false}, {"CROWS_WGS", &Tuning::crows_wgs, false},
};
static_assert(sizeof(FIELDS) / sizeof(FIELDS[0]) == sizeof(Tuning) / sizeof(int), "one entry per switch of Tuning");

struct Setting {
    Tuning tune = Tuning::unset();
    StampRequest stamps;
};

static bool apply_setting(Setting& st, const std::string& tok) {
    const size_t eq = tok.find('=');
    if (eq == std::string::npos) return false;
    const std::string name = tok.substr(0, eq);
    const int v = std::max(0, atoi(tok.c_str() + eq + 1));
    if (name == "XBYM_STAMP") return st.stamps.xy = true;
    if (name == "COARSE_STAMP") return st.stamps.co = true;
    if (name == "D7_STAMP") return st.stamps.d7_level = v, true;
    for (const Field& f : FIELDS)
        if (name == f.name) return st.tune.*(f.field) = f.flag ? v > 0 : v, true;
    return false;
}

static const char* SWEEP[] = {"none", "batch", "lone", "deriche"};
static const char* XFWD[] = {"copy", "k_vv_x_fwd", "k_vv_x_m"};
static const char* XBWD[] = {"none", "k_vv_x_m", "k_vv_x_bwd"};
static const char* YFWD[] = {"none", "k_vv_y_m", "k_vv_y_fwd1s", "k_vv_y_fwd1", "k_vv_y_fwd"};
static const char* YBWD[] = {"none", "k_vv_y_bwd_dec", "k_vv_y_bwd_dec7", "k_vv_y_bwd"};

static void dump(const PlanShape& s, const CallForm& c) {
    std::printf("{\"L\":%d,\"l_end\":%d,\"wf_levels\":%d,\"recompute\":%d,\"zero_tiles\":%d,\"mask_opt\":%d,\"src_fuse\":%d,\"no_fuse\":%d,\"blur_skip\":%d,"
                "\"coarse_from\":%d,\"collapse4\":%d,\"has_wf\":%d,\"has_zt\":%d,\"has_gz\":[%d,%d],\"has_mr\":[%d,%d],\"fast_paths\":%d,"
                "\"n\":%d,\"src\":%d,\"a_dense\":%d,\"wf_ctrl\":%d,\"coarse\":%d,\"coarse_lds\":%d,\"c4_lock\":%d,\"c4_swizzle\":%d,\"levels\":[",
                s.L, c.l_end, s.wf_levels, s.recompute, s.zero_tiles, s.mask_opt, s.src_fuse, s.no_fuse, s.blur_skip, s.coarse_from, s.collapse4, s.has_wf,
                s.has_zt, s.has_gz[0], s.has_gz[1], s.has_mr[0], s.has_mr[1], capability_mask(s), c.n, c.src, c.a_dense, c.wf_ctrl, c.coarse, c.coarse_lds,
                c.c4_lock, c.c4_swizzle);
    for (int l = 0; l < c.l_end; ++l) {
        const LevelForm& f = c.lv[l];
        const Level& a = s.lv[l];
        std::printf("%s{\"w\":%d,\"h\":%d,\"pitch\":%d,\"sweep\":\"%s\",\"x_fwd\":\"%s\",\"x_bwd\":\"%s\",\"y_fwd\":\"%s\",\"y_bwd\":\"%s\",\"do_x\":%d,\"do_y\":%d,"
                    "\"rcmp\":%d,\"stamp\":%d,\"xby\":%d,\"src0\":%d,\"mask_l0\":%d,\"odd_dec\":%d,\"zt\":%d,\"rowz\":%d,\"per_plane\":%d,\"g_in\":%d,\"g_out\":%d,"
                    "\"mr_in\":%d,\"mr_out\":%d,\"fill_mask\":%d,\"dec_zt\":%d,\"dec_odd\":%d,\"decimate\":%d,\"NR\":%d,\"NC\":%d,\"nbx\":%d,\"crows\":%d,\"xa\":%d,"
                    "\"xb\":%d,\"gen\":%d,\"px\":%d,\"c_mr\":%d}",
                    l ? "," : "", a.w, a.h, a.pitch, SWEEP[f.sweep], XFWD[f.x_fwd], XBWD[f.x_bwd], YFWD[f.y_fwd], YBWD[f.y_bwd], f.do_x, f.do_y, f.rcmp, f.stamp,
                    f.xby, f.src0, f.mask_l0, f.odd_dec, f.zt, f.rowz, f.per_plane, f.g_in, f.g_out, f.mr_in, f.mr_out, f.fill_mask, f.dec_zt, f.dec_odd,
                    f.decimate, f.NR, f.NC, f.nbx, f.crows, f.xa, f.xb, f.gen, f.px, f.c_mr);
    }
    std::printf("]}\n");
}

// The invariants of a call's form.  The first seven were run-time checks of the launch path while two places decided the flags.
static const char* violated(const PlanShape& s, const CallForm& c) {
    bool any_batch = false;
    for (int l = 0; l < c.l_end; ++l) any_batch = any_batch || c.lv[l].sweep == SW_BATCH;
    for (int l = 0; l < 32; ++l) {
        const LevelForm& f = c.lv[l];
        const Level& a = s.lv[l];
        if (l >= c.l_end) {
            static const LevelForm zero{};
            if (std::memcmp(&f, &zero, sizeof f) != 0) return "a record at a level that is not reduced by itself";
            continue;
        }
        const bool batch = f.sweep == SW_BATCH, even_w = (a.w & 1) == 0, even_h = (a.h & 1) == 0;
        if (f.g_out && !(batch && f.zt && even_w)) return "G column flags without their producer";
        if (f.g_in && !f.do_x) return "G column flags without their reader";
        if (f.mr_out && !(batch && f.fill_mask && f.g_out && even_w && even_h)) return "mask row flags without their producer";
        if (f.mr_in && !(f.g_in && f.do_x && (batch || !f.zt))) return "mask row flags without their reader";
        if (f.mr_in && (f.rcmp || f.src0 || f.stamp)) return "mask row flags in front of a sweep that does not know them";
        if (batch && ((f.mask_l0 && f.zt) || (l > 0 && f.fill_mask && f.mr_in)) != f.fill_mask) return "the mask plane's T flags read in another sense than they are written";
        if (f.c_mr != f.mr_in) return "collapse: mask row flags decided otherwise than in the reduce";
        if ((f.g_in || f.mr_in) && (l < 1 || l > 2)) return "flags read outside levels 1 and 2";
        if ((f.g_out || f.mr_out) && (l > 1 || l + 1 >= c.l_end)) return "flags written outside levels 1 and 2, or for a level that is not reduced by itself";
        if (f.g_in != (l > 0 && c.lv[l - 1].g_out) || f.mr_in != (l > 0 && c.lv[l - 1].mr_out)) return "flags read are not the flags written";
        if (f.mr_in && !f.g_in) return "mask row flags without G column flags";
        if (f.g_in && !s.has_gz[l - 1]) return "G column flags without their array";
        if (f.mr_in && !s.has_mr[l - 1]) return "mask row flags without their array";
        if ((f.g_in || f.mr_in) && !(f.x_fwd == XF_FWD && !f.rcmp && !f.src0)) return "flags in front of a causal x sweep other than plain k_vv_x_fwd";
        if (f.zt && (f.NR > 256 || !s.has_zt)) return "zero-tile flags beyond 256 bands or without their array";
        if (f.rowz && !f.zt) return "rowz without zero-tile flags";
        if (f.rowz && !f.dec_zt) return "an instance of k_vv_y_bwd_dec the library does not have";
        if (f.zt && f.y_bwd != YB_DEC) return "zero-tile flags without the decimating sweep that reads them";
        if (f.x_fwd == XF_M && (f.zt || f.g_in)) return "k_vv_x_m in front of flags";
        if (f.xby && (c.n != 1 || any_batch || !s.has_wf)) return "k_vv_xby_m in a batch, beside the batch's sweep, or without hand-off buffers";
        if (batch && !s.has_wf) return "k_vv_xbyf without hand-off buffers";
        if ((batch || f.xby) && !c.wf_ctrl) return "a fused sweep whose band queue nobody clears";
        if (f.rcmp && !batch) return "recompute outside the batch's sweep";
        if (f.g_in && !(7ull * s.cap * a.ps + 64ull * a.pitch < (1ull << 32))) return "G column flags beyond the 32-bit sample offset";
        if (f.decimate == (f.y_bwd == YB_DEC || f.y_bwd == YB_DEC7)) return "decimated twice or never";
        if (f.xb < f.xa || f.xa % 256 || f.xb % 256 || f.xb > a.pitch || f.crows < 1) return "collapse: a column range or strip height out of range";
    }
    if (c.coarse != (s.coarse_from > 0) || (c.coarse_lds && !c.coarse)) return "the coarse launch";
    return nullptr;
}

static std::vector<int> ints(std::istringstream& in) {
    std::vector<int> v;
    for (int x; in >> x;) v.push_back(x);
    return v;
}

// ---- the band path (BandShape, band_form) ------------------------------------------------------------------------------------------
// The operations pipeline.BandStitcher.steps issues at one split level, by the level's form there: 's' the three separate sweeps,
// 'f' the fused sweep (levels 0 and 1; the separate sweeps elsewhere), 'p' the y sweeps plane by plane, 'c' the y sweeps in column chunks
// (even widths with the fused decimation; the separate sweeps elsewhere); and, issued by tests/test_gpu_band.py alone, 'x' the fused sweep
// with the decimating sweep over a column range behind it (levels 0 and 1 where 'c' applies; 'f' elsewhere)
struct BandCall {
    BandOp op;
    int plane;
};
static std::vector<BandCall> level_calls(const BandShape& s, int l, char kind) {
    std::vector<BandCall> v;
    if (kind == 'x' && l < 2) return {{BO_XY_FWD, -1}, {(s.lv[l].w & 1) == 0 && !s.plain_dec ? BO_Y_BWD_COLS : BO_Y_BWD, -1}};
    if (kind == 'f' && l < 2) return {{BO_XY_FWD, -1}, {BO_Y_BWD, -1}};
    v.push_back({BO_X, -1});
    if (kind == 'p') {
        for (int pl = 0; pl < 7; ++pl) v.push_back({BO_Y_FWD, pl});
        for (int pl = 0; pl < 7; ++pl) v.push_back({BO_Y_BWD, pl});
    } else if (kind == 'c' && (s.lv[l].w & 1) == 0 && !s.plain_dec) {
        for (int c = 0; c < 2; ++c) v.push_back({BO_Y_FWD_COLS, -1});
        for (int c = 0; c < 2; ++c) v.push_back({BO_Y_BWD_COLS, -1});
    } else {
        v.push_back({BO_Y_FWD, -1});
        v.push_back({BO_Y_BWD, -1});
    }
    return v;
}
static const char* BAND_OPS[] = {"compose", "x", "xy_fwd", "y_fwd", "y_fwd_cols", "y_bwd", "y_bwd_cols", "collapse"};

// the kernels of a record, as the library instantiates them
static std::string band_kernels(const BandForm& f, BandOp op) {
    char buf[160];
    const char* xf = f.src0 ? "k_vv_x_fwd<PX,1>" : "k_vv_x_fwd<float,0>";
    switch (op) {
    case BO_COMPOSE: return f.src0 ? "k_src_index k_seam" : "k_compose k_seam k_mask";
    case BO_X: return std::string(xf) + " k_vv_x_bwd";
    case BO_XY_FWD: return std::string(xf) + (f.banded ? " k_vv_xbyf<0,float,0,1>" : " k_vv_xbyf<0,float,0,0>");
    case BO_Y_FWD:
    case BO_Y_FWD_COLS: return f.xch ? "k_vv_y_fwd<1>" : "k_vv_y_fwd<0>";
    case BO_Y_BWD:
    case BO_Y_BWD_COLS:
        if (f.y_bwd != YB_DEC) return "k_vv_y_bwd k_decimate";
        std::snprintf(buf, sizeof buf, "k_vv_y_bwd_dec<%d,YST,%d,%d,%d>", f.dec.rowz, f.dec.zt, f.dec.odd, f.dec.xch);
        return buf;
    case BO_COLLAPSE: return f.xb > f.xa ? "k_collapse4" : "k_collapse";
    }
    return "";
}

static void dump_band_form(const BandForm& f, BandOp op, int level, int plane, bool first) {
    std::printf("%s{\"op\":\"%s\",\"level\":%d,\"plane\":%d,\"kernels\":\"%s\",\"zt_after\":%d,\"src0\":%d,\"zi\":%d,\"zt\":%d", first ? "" : ",", BAND_OPS[op], level, plane,
                band_kernels(f, op).c_str(), f.zt_after, f.src0, f.zi, f.zt);
    if (op == BO_X || op == BO_XY_FWD) std::printf(",\"per_plane\":%d,\"nbx\":%d,\"bands\":[%d,%d]", f.per_plane, f.nbx, f.bands_nr, f.bands_h);
    if (op == BO_XY_FWD) std::printf(",\"banded\":%d,\"NR\":%d,\"NC\":%d,\"wgs\":%d", f.banded, f.NR, f.NC, f.wgs);
    if (op >= BO_Y_FWD && op <= BO_Y_BWD_COLS) std::printf(",\"np\":%d,\"xch\":%d", f.np, f.xch);
    if (op == BO_Y_BWD || op == BO_Y_BWD_COLS) std::printf(",\"decimate\":%d", f.decimate);
    if (op == BO_COLLAPSE) std::printf(",\"crows\":%d,\"strips\":%d,\"cols\":%d,\"xa\":%d,\"xb\":%d,\"top_src\":%d", f.crows, f.strips, f.cols, f.xa, f.xb, f.top_src);
    std::printf("}");
}

// One band: its shape and the records of every call of the sequence `kinds` (one letter per split level, the last one repeated)
static void dump_band(const BandShape& s, const std::string& kinds) {
    std::printf("{\"rank\":%d,\"nranks\":%d,\"Ls\":%d,\"L\":%d,\"levels\":[", s.rank, s.nranks, s.Ls, s.L);
    for (int l = 0; l <= s.Ls; ++l) {
        const BandLevel& v = s.lv[l];
        std::printf("%s{\"w\":%d,\"h_full\":%d,\"rows\":%d,\"row0\":%d,\"pitch\":%d,\"halo\":%d,\"c4\":[%d,%d],\"sh_eff\":%d}", l ? "," : "", v.w, v.h_full, v.rows, v.row0, v.pitch,
                    v.halo, v.c4_xa, v.c4_xb, v.sh_eff);
    }
    std::printf("],\"calls\":[");
    int zt = -1;
    dump_band_form(band_form(s, BO_COMPOSE, 0), BO_COMPOSE, 0, -1, true);
    for (int l = 0; l < s.Ls; ++l)
        for (const BandCall& c : level_calls(s, l, kinds[std::min<size_t>(l, kinds.size() - 1)])) {
            const BandForm f = band_form(s, c.op, l, zt, c.plane);
            dump_band_form(f, c.op, l, c.plane, false);
            zt = f.zt_after;
        }
    for (int l = s.Ls - 1; l >= 0; --l) dump_band_form(band_form(s, BO_COLLAPSE, l), BO_COLLAPSE, l, -1, false);
    std::printf("]}\n");
}

// The invariants of a band's sequence of calls; nullptr when they hold
static const char* band_violated(const BandShape& s, const std::string& kinds) {
    // what the flag buffer and T hold, followed apart from band_zt_after: the level whose flags were written last, and whether T is
    // still the T they describe
    int zt = -1, flag_level = -1;
    bool flags_fresh = false, owed = false;  // owed: flags written that their level's anticausal sweep has yet to read
    if (band_form(s, BO_COMPOSE, 0).zi && !(s.src_l0 && s.zero_tiles)) return "index-plane flags without the index plane";
    for (int l = 0; l < s.Ls; ++l) {
        const BandLevel& a = s.lv[l];
        const bool even_w = (a.w & 1) == 0;
        for (const BandCall& c : level_calls(s, l, kinds[std::min<size_t>(l, kinds.size() - 1)])) {
            const BandForm f = band_form(s, c.op, l, zt, c.plane);
            zt = f.zt_after;
            if (!f.admitted) return "the sequence issues a call the level does not admit";
            if (c.op == BO_X || c.op == BO_XY_FWD) {
                if (owed) return "flags written and never read";
                flags_fresh = c.op == BO_XY_FWD && f.zt;
                if (flags_fresh) flag_level = l, owed = true;
                if (f.zt && !(even_w && f.NR <= ZT_MAX_BANDS && a.halo == 0 && s.zero_tiles && !s.plain_dec && l < 2 && f.bands_h == a.rows))
                    return "T flags at a level that cannot have them";
                if (f.per_plane != (f.src0 || f.zt) || f.nbx != (f.per_plane ? 7 * tiles(a.ph()) : (int)((7L * a.ph() + TS - 1) / TS)) || f.nbx < 1)
                    return "blocks of the x sweeps";
                if (c.op == BO_X && f.zt) return "the separate x sweeps write flags";
            }
            if (c.op == BO_XY_FWD) {
                if (f.banded != (a.halo != 0 || s.rank > 0)) return "BANDED otherwise than with halo rows or a resume state";
                if (f.wgs < 1 || f.wgs > WF_MAX_WGS || f.wgs > 7 * f.NR || a.w < 2 || a.rows < 2) return "workgroups of the fused sweep";
                if ((size_t)f.NC > (size_t)(s.lv[0].pitch / TS)) return "hand-off granules beyond level 0's";
            }
            if (c.op == BO_Y_BWD || c.op == BO_Y_BWD_COLS) {
                if (f.zt && !(flags_fresh && flag_level == l)) return "flags read that this level did not write, or behind another sweep";
                if (owed && !f.zt) return "flags written are not read by the level's anticausal sweep";
                owed = false;
                if (f.y_bwd == YB_DEC && !(even_w && !s.plain_dec)) return "the fused decimation at an odd width or under STITCH_BAND_PLAIN";
                if (f.xch && !(f.y_bwd == YB_DEC && even_w && !s.plain_dec)) return "XCH at an odd width or without the fused decimation";
                if (f.y_bwd == YB_DEC && !(f.dec.zt && !f.dec.odd && f.dec.xch == f.xch && (!f.dec.rowz || (f.zt && a.rows % YCH)))) return "an instance of k_vv_y_bwd_dec the band path does not have";
                if (f.zt && (a.rows % YCH) && !f.dec.rowz) return "flags of a height that YCH does not divide without the per-row look-up";
                if (f.decimate == (f.y_bwd == YB_DEC)) return "decimated twice or never";
            }
            if ((c.op == BO_Y_FWD || c.op == BO_Y_BWD) && f.np != (c.plane < 0 ? 7 : 1)) return "planes of a y sweep";
        }
        // the collapse
        const BandForm f = band_form(s, BO_COLLAPSE, l);
        if (f.xa < 0 || f.xb < f.xa || f.xb > f.cols || f.xa % 256 || f.xb % 256 || f.cols != (l == 0 ? a.w : a.pitch)) return "collapse: [xa, xb) outside the level";
        if (f.crows < 1 || f.strips * f.crows < a.rows || (f.strips - 1) * f.crows >= a.rows) return "collapse: strips do not cover the band";
        if (f.top_src != (l + 1 == s.Ls)) return "collapse: the replicated source";
    }
    if (owed) return "flags written and never read";
    return nullptr;
}

// The y taps of every EXPAND of a band, computed apart from band_row_table: inside what the rank holds, and the kernels' clamp
// `iy < sh_eff - 1 ? iy + 1 : iy` lands on the level's tap (whatever the switches and the sequence)
static const char* band_rows_violated(const BandShape& s) {
    for (int l = 0; l < s.Ls; ++l) {
        const BandLevel &a = s.lv[l], &nx = s.lv[l + 1];
        const bool top_src = l + 1 == s.Ls;
        std::vector<int32_t> idx;
        std::vector<double> al;
        expand_table(nx.h_full, a.h_full, idx, al);
        const int base = top_src ? 0 : nx.row0 - nx.halo, held = top_src ? nx.h_full : nx.rows + 2 * nx.halo;
        for (int y = 0; y < a.rows; ++y) {
            const int gi = idx[a.row0 + y], gi2 = std::min(gi + 1, nx.h_full - 1), iy = gi - base;
            if (iy < 0 || gi2 - base >= held) return "a row's taps outside the band's halo";
            if ((iy < a.sh_eff - 1 ? iy + 1 : iy) != gi2 - base) return "sh_eff clamps elsewhere than the level's last row";
        }
    }
    return nullptr;
}

// bandcheck: every admissible band of the grid's canvases; ranks 1..8, every rank, every split, the switches, every sequence
static int band_check_grid(const std::vector<int>& ws, const std::vector<int>& hs) {
    long shapes = 0, cases = 0, bad = 0, refused_halo = 0;
    std::vector<std::string> seqs;
    for (const char* a : {"s", "f", "p", "c", "x"})
        for (const char* b : {"s", "f", "p", "c", "x"})
            for (const char* c : {"s", "p", "c"}) seqs.push_back(std::string(a) + b + c);
    for (int w : ws)
        for (int h : hs)
            for (int nranks = 1; nranks <= 8; ++nranks)
                for (int Ls = 1; Ls < 32; ++Ls) {
                    BandShape probe;
                    if (band_shape(probe, w, h, 0, nranks, Ls, true, true, false) == BAND_BAD_SPLIT) break;
                    for (int rank = 0; rank < nranks; ++rank)
                        for (int sw = 0; sw < 8; ++sw) {  // STITCH_NO_ZERO_TILES, STITCH_BAND_PLANES / stitch_band_set_level0, STITCH_BAND_PLAIN
                            BandShape s;
                            const BandRefusal no = band_shape(s, w, h, rank, nranks, Ls, !(sw & 1), !(sw & 2), (sw & 4) != 0);
                            refused_halo += no == BAND_BAD_HALO;
                            if (no != BAND_OK) continue;
                            ++shapes;
                            if (const char* why = sw == 0 ? band_rows_violated(s) : nullptr)
                                if (++bad <= 20) std::printf("%dx%d rank %d of %d Ls %d: %s\n", w, h, rank, nranks, Ls, why);
                            for (const std::string& q : seqs) {
                                if (s.src_l0 && q[0] == 'p') continue;  // one plane at a time: the caller stores level 0 (BandStitcher does)
                                ++cases;
                                if (const char* why = band_violated(s, q))
                                    if (++bad <= 20) std::printf("%dx%d rank %d of %d Ls %d switches %d sequence %s: %s\n", w, h, rank, nranks, Ls, sw, q.c_str(), why);
                            }
                        }
                }
    std::printf("bands %ld cases %ld refused_for_halo %ld violations %ld\n", shapes, cases, refused_halo, bad);
    return bad ? 1 : 0;
}

int main(int argc, char** argv) {
    if (argc != 3) return std::fprintf(stderr, "usage: %s dump|check FILE\n", argv[0]), 2;
    std::ifstream file(argv[2]);
    if (!file) return std::fprintf(stderr, "cannot read %s\n", argv[2]), 2;
    const bool check = std::strcmp(argv[1], "check") == 0 || std::strcmp(argv[1], "bandcheck") == 0;
    if (std::strcmp(argv[1], "band") == 0) {
        for (std::string line; std::getline(file, line);) {
            std::istringstream in(line);
            int cw, ch, rank, nranks, Ls, zt, src, plain;
            std::string kinds;
            if (!(in >> cw >> ch >> rank >> nranks >> Ls >> zt >> src >> plain >> kinds)) continue;
            BandShape s;
            const BandRefusal no = band_shape(s, cw, ch, rank, nranks, Ls, zt != 0, src != 0, plain != 0);
            if (no != BAND_OK)
                std::printf("{\"refused\":%d}\n", (int)no);
            else
                dump_band(s, kinds);
        }
        return 0;
    }
    std::vector<int> ws, hs, caps;
    std::vector<Setting> settings;
    for (std::string line; std::getline(file, line);) {
        std::istringstream in(line);
        if (!check) {
            int cw, ch, cap, n, src, a_dense, blur, rule, planes_in;
            float sigma;
            if (!(in >> cw >> ch >> cap >> n >> src >> a_dense >> sigma >> blur >> rule >> planes_in)) continue;
            Setting st;
            for (std::string tok; in >> tok;)
                if (!apply_setting(st, tok)) return std::fprintf(stderr, "unknown setting %s\n", tok.c_str()), 2;
            PlanShape s;
            if (plan_shape(s, cw, ch, stitch_blend_opts{sigma, blur, rule, 0}, cap, st.tune, st.stamps, planes_in != 0) <= 0) {
                std::printf("null\n");
                continue;
            }
            dump(s, call_form(s, n, src < 0 ? source_fused_call(s, n) : src != 0, a_dense != 0));
            continue;
        }
        std::string key;
        in >> key;
        if (key == "w") ws = ints(in);
        else if (key == "h") hs = ints(in);
        else if (key == "cap") caps = ints(in);
        else if (key == "set") {
            Setting st;
            for (std::string tok; in >> tok;)
                if (!apply_setting(st, tok)) return std::fprintf(stderr, "unknown setting %s\n", tok.c_str()), 2;
            settings.push_back(st);
        }
    }
    if (!check) return 0;
    if (std::strcmp(argv[1], "bandcheck") == 0) return band_check_grid(ws, hs);
    long cases = 0, bad = 0;
    for (int w : ws)
        for (int h : hs)
            for (int blur = 0; blur < 2; ++blur)
                for (int rule = 0; rule < 2; ++rule)
                    for (float sigma : {0.25f, 2.0f})
                        for (int cap : caps)
                            for (const Setting& st : settings) {
                                PlanShape s, handed;  // handed: the coarse levels of a split pair, level 0 handed in as planes
                                if (plan_shape(s, w, h, stitch_blend_opts{sigma, blur, rule, 0}, cap, st.tune, st.stamps) <= 0) continue;
                                plan_shape(handed, w, h, stitch_blend_opts{sigma, blur, rule, 0}, cap, st.tune, st.stamps, true);
                                for (int n : {1, 2, cap}) {
                                    if (n > cap) continue;
                                    for (int form = 0; form < 4; ++form) {  // source-fused or not, pairs or a dense blend, and the coarse levels of a split pair
                                        const bool src = (form & 1) && s.src_fuse, dense = form == 2 || form == 3;
                                        if (((form & 1) && !s.src_fuse) || (dense && n > 1)) continue;
                                        for (int planes_in = 0; planes_in < (form == 0 && n == 1 ? 2 : 1); ++planes_in) {
                                            const PlanShape& sh = planes_in ? handed : s;
                                            const CallForm c = call_form(sh, n, src, dense);
                                            ++cases;
                                            if (const char* why = violated(sh, c)) {
                                                if (++bad <= 20)
                                                    std::printf("%dx%d cap %d n %d blur %d rule %d sigma %g src %d dense %d planes_in %d: %s\n", w, h, cap, n, blur, rule, sigma, src,
                                                                dense, planes_in, why);
                                            }
                                        }
                                    }
                                }
                            }
    std::printf("cases %ld violations %ld\n", cases, bad);
    return bad ? 1 : 0;
}
