// The pair path's decision (csrc/stitch_call_form.h) on a machine without a GPU, for tests/test_call_form_host.py.
//   call_form_dump dump FILE    one case per line -> one JSON object per line: the plan's shape and the call's per-level records
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

int main(int argc, char** argv) {
    if (argc != 3) return std::fprintf(stderr, "usage: %s dump|check FILE\n", argv[0]), 2;
    std::ifstream file(argv[2]);
    if (!file) return std::fprintf(stderr, "cannot read %s\n", argv[2]), 2;
    const bool check = std::strcmp(argv[1], "check") == 0;
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
            if (plan_shape(s, cw, ch, stitch_blend_opts{sigma, blur, rule, 0}, cap, st.tune, st.stamps) <= 0) {
                std::printf("null\n");
                continue;
            }
            s.planes_in = planes_in != 0;
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
    long cases = 0, bad = 0;
    for (int w : ws)
        for (int h : hs)
            for (int blur = 0; blur < 2; ++blur)
                for (int rule = 0; rule < 2; ++rule)
                    for (float sigma : {0.25f, 2.0f})
                        for (int cap : caps)
                            for (const Setting& st : settings) {
                                PlanShape s;
                                if (plan_shape(s, w, h, stitch_blend_opts{sigma, blur, rule, 0}, cap, st.tune, st.stamps) <= 0) continue;
                                for (int n : {1, 2, cap}) {
                                    if (n > cap) continue;
                                    for (int form = 0; form < 4; ++form) {  // source-fused or not, pairs or a dense blend, and the coarse levels of a split pair
                                        const bool src = (form & 1) && s.src_fuse, dense = form == 2 || form == 3;
                                        if (((form & 1) && !s.src_fuse) || (dense && n > 1)) continue;
                                        for (int planes_in = 0; planes_in < (form == 0 && n == 1 ? 2 : 1); ++planes_in) {
                                            s.planes_in = planes_in != 0;
                                            const CallForm c = call_form(s, n, src, dense);
                                            ++cases;
                                            if (const char* why = violated(s, c)) {
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
