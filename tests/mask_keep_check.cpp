// The form word of the mask pyramids that stand (csrc/stitch_call_form.h: mask_keep_word, mask_keep_level), compiled by the host compiler
// alone and checked over a grid of canvases, capacities, n and switch sets (tests/test_mask_keep_host.py writes the grid):
//   a  two calls on one plan whose LevelForms agree in mask_l0, mr_out, mr_in and fill_mask at every level have equal words but for MK_KEEP_OK;
//   b  two calls that differ in one of these at any level have different words;
//   c  MK_KEEP_OK is clear whenever a level selects a kernel outside the set that knows the skip -- the set restated here by name --,
//      for a pathed call, and on a plan whose level-0 mask is a stored plane.
// Usage: mask_keep_check GRID      (lines: "w ...", "h ...", "cap ...", "set NAME=VALUE ...")
//        mask_keep_check word CW CH CAP N SRC [NAME=VALUE ...]   -> the word, keep_ok and the per-level mask fields of one call
#include <cstdio>
#include <fstream>
#include <iostream>
#include <sstream>
#include <string>

#include "stitch_call_form.h"

using namespace sk;

Tuning Tuning::from_env() { return unset(); }  // (never called here: switches arrive as numbers)

struct Field {
    const char* name;
    int Tuning::*f;
};
// the switches the grid's settings name (tests/switch_table.py, tests/g_flags_ref.py)
static const Field FIELDS[] = {
    {"WAVEFRONT", &Tuning::wavefront}, {"NO_FUSE", &Tuning::no_fuse}, {"NO_SRC_FUSE", &Tuning::no_src_fuse}, {"NO_ZERO_TILES", &Tuning::no_zero_tiles},
    {"RECOMPUTE", &Tuning::recompute}, {"SINGLE_FAST", &Tuning::single_fast}, {"ODD_DEC", &Tuning::odd_dec}, {"Y1S", &Tuning::y1s}, {"MOVER", &Tuning::mover},
    {"DEC7", &Tuning::dec7}, {"XBYM", &Tuning::xbym}, {"XBYM_MPIX", &Tuning::xbym_mpix}, {"Y2", &Tuning::y2}, {"GATE64", &Tuning::gate64}, {"COARSE", &Tuning::coarse},
    {"SRC_LONE_MPIX", &Tuning::src_lone}, {"WAVEFRONT_STAMP", &Tuning::stamp},
};

static bool apply_setting(Tuning& t, const std::string& tok) {
    const size_t eq = tok.find('=');
    if (eq == std::string::npos) return false;
    for (const Field& f : FIELDS)
        if (tok.substr(0, eq) == f.name) {
            t.*(f.f) = atoi(tok.c_str() + eq + 1);
            return true;
        }
    return false;
}

// the rule of (c), by kernel: what REDUCE of the level launches, and whether every one of them knows the skip
static bool level_supported(const LevelForm& f) {
    if (f.sweep == SW_DERICHE) return false;  // k_deriche
    if (f.rcmp) return false;                 // k_vv_x_fwd<.., CKPT>, k_vv_xbyf MODE 1 / 2
    if (f.xby) return false;                  // k_vv_xby_m
    // k_vv_x_fwd, k_vv_x_bwd, k_vv_x_m, k_vv_xbyf MODE 0, k_vv_y_fwd, k_vv_y_fwd1, k_vv_y_fwd1s, k_vv_y_m, k_vv_y_bwd_dec, k_vv_y_bwd_dec7,
    // k_vv_y_bwd + k_decimate, a copy
    return f.sweep == SW_BATCH || f.sweep == SW_LONE;
}

static bool same_mask_fields(const CallForm& a, const CallForm& b) {
    if (a.l_end != b.l_end) return false;
    for (int l = 0; l < a.l_end; ++l)
        if (a.lv[l].mask_l0 != b.lv[l].mask_l0 || a.lv[l].mr_out != b.lv[l].mr_out || a.lv[l].mr_in != b.lv[l].mr_in || a.lv[l].fill_mask != b.lv[l].fill_mask) return false;
    return true;
}

static std::vector<int> ints(std::istringstream& in) {
    std::vector<int> v;
    int x;
    while (in >> x) v.push_back(x);
    return v;
}

int main(int argc, char** argv) {
    if (argc >= 7 && std::string(argv[1]) == "word") {
        Tuning t = Tuning::unset();
        for (int i = 7; i < argc; ++i)
            if (!apply_setting(t, argv[i])) return 2;
        stitch_blend_opts o{2.0f, 0, 1, 0};
        PlanShape s;
        if (plan_shape(s, atoi(argv[2]), atoi(argv[3]), o, atoi(argv[4]), t) <= 0) return 3;
        const int n = atoi(argv[5]), src = atoi(argv[6]);
        const CallForm c = call_form(s, n, src < 0 ? source_fused_call(s, n) : src != 0, false);
        const uint32_t w = mask_keep_word(s, c, false);
        std::printf("{\"word\": %u, \"keep_ok\": %d, \"levels\": [", w, (w & MK_KEEP_OK) ? 1 : 0);
        for (int l = 0; l < c.l_end; ++l)
            std::printf("%s[%d, %d, %d, %d]", l ? ", " : "", c.lv[l].mask_l0, c.lv[l].mr_out, c.lv[l].mr_in, c.lv[l].fill_mask);
        std::printf("]}\n");
        return 0;
    }
    if (argc != 2) return 2;
    std::ifstream in(argv[1]);
    std::vector<int> ws, hs, caps;
    std::vector<Tuning> sets;
    std::string line;
    while (std::getline(in, line)) {
        std::istringstream ls(line);
        std::string key;
        ls >> key;
        if (key == "w") ws = ints(ls);
        else if (key == "h") hs = ints(ls);
        else if (key == "cap") caps = ints(ls);
        else if (key == "set") {
            Tuning t = Tuning::unset();
            std::string tok;
            while (ls >> tok)
                if (!apply_setting(t, tok)) {
                    std::printf("unknown setting %s\n", tok.c_str());
                    return 2;
                }
            sets.push_back(t);
        }
    }
    long cases = 0, violations = 0, keeps = 0;
    auto bad = [&](const char* what, int w, int h, int cap, size_t set, int n, int m) {
        if (++violations <= 20) std::printf("%s: %d x %d cap %d set %zu n %d / %d\n", what, w, h, cap, set, n, m);
    };
    for (size_t si = 0; si < sets.size(); ++si)
        for (int w : ws)
            for (int h : hs)
                for (int cap : caps)
                    for (int kind = 0; kind < 3; ++kind) {  // blur_kind 0 / 1, a stored level-0 mask
                        stitch_blend_opts o{2.0f, kind == 1 ? 1 : 0, 1, 0};
                        PlanShape s;
                        if (plan_shape(s, w, h, o, cap, sets[si], StampRequest{}, false, kind == 2) <= 0) continue;
                        std::vector<CallForm> forms;
                        std::vector<int> ns;
                        for (int n : {1, 2, 3, cap})
                            if (n <= cap)
                                for (int src = 0; src < 2; ++src) {
                                    if (src && !s.src_fuse) continue;
                                    forms.push_back(call_form(s, n, src != 0, false));
                                    ns.push_back(n);
                                }
                        for (size_t i = 0; i < forms.size(); ++i) {
                            const uint32_t wi = mask_keep_word(s, forms[i], false);
                            ++cases;
                            bool supported = forms[i].l_end >= 1 && forms[i].lv[0].mask_l0 && !s.mask_stored();
                            for (int l = 0; l < forms[i].l_end; ++l) supported = supported && level_supported(forms[i].lv[l]);
                            if ((wi & MK_KEEP_OK) && !supported) bad("keep_ok with a kernel that does not know the skip", w, h, cap, si, ns[i], 0);
                            if (!(wi & MK_KEEP_OK) && supported) bad("keep_ok clear although every kernel knows the skip", w, h, cap, si, ns[i], 0);
                            if (mask_keep_word(s, forms[i], true) & MK_KEEP_OK) bad("keep_ok on a pathed call", w, h, cap, si, ns[i], 0);
                            if ((mask_keep_word(s, forms[i], true) | MK_KEEP_OK) != (wi | MK_KEEP_OK)) bad("pathed changes more than keep_ok", w, h, cap, si, ns[i], 0);
                            keeps += (wi & MK_KEEP_OK) ? 1 : 0;
                            for (size_t j = i + 1; j < forms.size(); ++j) {
                                const uint32_t wj = mask_keep_word(s, forms[j], false);
                                const bool same = same_mask_fields(forms[i], forms[j]);
                                if (same && (wi | MK_KEEP_OK) != (wj | MK_KEEP_OK)) bad("equal mask fields, different words", w, h, cap, si, ns[i], ns[j]);
                                if (!same && (wi | MK_KEEP_OK) == (wj | MK_KEEP_OK)) bad("different mask fields, equal words", w, h, cap, si, ns[i], ns[j]);
                            }
                        }
                    }
    std::printf("cases %ld keeps %ld violations %ld\n", cases, keeps, violations);
    return violations ? 1 : 0;
}
