// Host emulation of csrc/k_exposure.inc for tests/test_exposure_host.py: the device functions themselves -- the element map, the
// composition, the tile redo, the span reduction and the walk -- compiled for the CPU without FMA contraction.  The functions of
// a workgroup are written as phases between barriers (EX_THREADS); here each phase runs for thread 0 .. 255 in turn, and the
// block scan is the sequential one the .inc keeps for this build.  What the launches of stitch_exposure.inc do around them (the
// span sums in double, the guess, the order of the passes) is restated in emu_stats.  emu_plain is the yardstick: a plain
// float loop, as transfer.cpp:128-164 and k_tr_stats accumulate.
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <vector>
#define EX_HOST
#define EX_THREADS(t) for (int t = 0; t < EX_T; ++t)
#define EX_PER_THREAD(type, name) type name[EX_T]
#define EX_MINE(name, t) name[t]
#define EX_SYNC()
#define EX_ATOMIC_MIN(p, v) (*(p) = *(p) < (v) ? *(p) : (v))
#define EX_DEV static inline
#include "k_exposure.inc"

static ExShared g_sh;

extern "C" {

void emu_constants(int out[4]) {
    out[0] = EX_TILE;
    out[1] = EX_SPAN;
    out[2] = EX_MAX_RESTARTS;
    out[3] = EX_T;
}

// the map of one element under the state `state` (its sign and binade) -> c[2], lo[2], hi[2]
void emu_elem_map(float x, float state, int32_t out[6]) {
    const ExMap m = ex_elem_map(x, ex_scale(ex_bits(state) >> 23));
    std::memcpy(out, &m, sizeof m);
}

void emu_compose(const int32_t f[6], const int32_t g[6], int32_t out[6]) {
    ExMap a, b;
    std::memcpy(&a, f, sizeof a);
    std::memcpy(&b, g, sizeof b);
    const ExMap h = ex_compose(a, b);
    std::memcpy(out, &h, sizeof h);
}

// 1 and the state behind the map where it is valid at `state`, else 0
int emu_apply(const int32_t m6[6], float state, float* out) {
    ExMap m;
    std::memcpy(&m, m6, sizeof m);
    const uint32_t bits = ex_bits(state), key = bits >> 23;
    const int32_t S = (int32_t)((bits & 0x7fffffu) | 0x800000u);
    if (!ex_key_normal(key) || !ex_valid(m, S)) return 0;
    *out = ex_float((key << 23) | ((uint32_t)(S + ex_pick(m.c[0], m.c[1], S & 1)) & 0x7fffffu));
    return 1;
}

float emu_redo(const float* p, size_t b, size_t e, float acc, int pass, float mean, uint32_t diag[4]) { return ex_redo(g_sh, p, b, e, acc, pass, mean, diag); }

void emu_span_map(const float* p, size_t b, size_t e, int pass, float mean, float guess, int32_t out[6]) {
    const ExMap m = ex_span_map(g_sh, p, b, e, pass, mean, ex_bits(guess) >> 23);
    std::memcpy(out, &m, sizeof m);
}

// One pass over a plane in form 2.  guesses (optional): per span a float that replaces the launch's guess where it is not NaN.
static float pass_form2(const float* p, size_t n, int pass, float mean, const float* guesses, uint32_t diag[4]) {
    const size_t spans = (n + EX_SPAN - 1) / EX_SPAN;
    std::vector<double> sums(spans);
    for (size_t s = 0; s < spans; ++s) {  // k_ex_span_sums
        double v = 0.0;
        for (size_t i = s * EX_SPAN; i < n && i < (s + 1) * EX_SPAN; ++i) v += (double)ex_addend(p[i], pass, mean);
        sums[s] = v;
    }
    std::vector<ExSpanEntry> table(spans);
    for (size_t s = 0; s < spans; ++s) {  // k_ex_span_maps
        double v = 0.0;
        for (size_t k = 0; k < s; ++k) v += sums[k];
        float g = (float)v;
        if (guesses && guesses[s] == guesses[s]) g = guesses[s];
        const uint32_t key = ex_bits(g) >> 23;
        const size_t b = s * EX_SPAN, e = b + EX_SPAN < n ? b + EX_SPAN : n;
        table[s].key = ex_key_normal(key) ? key : EX_NO_GUESS;
        table[s].m = ex_key_normal(key) ? ex_span_map(g_sh, p, b, e, pass, mean, key) : ex_identity();
    }
    float acc = 0.f;
    for (size_t s = 0; s < spans; ++s) {  // k_ex_walk
        const size_t b = s * EX_SPAN, e = b + EX_SPAN < n ? b + EX_SPAN : n;
        acc = ex_walk_span(g_sh, table[s], p, b, e, acc, pass, mean, diag);
    }
    return acc;
}

// mean and sd of one plane: form 1 (single workgroup) or 2 (spans + walk); diag[4] is added to
void emu_stats(const float* p, size_t n, float cnt, int form, const float* guesses, float* mean_out, float* sd_out, uint32_t diag[4]) {
    float acc = form == 1 ? ex_redo(g_sh, p, 0, n, 0.f, 0, 0.f, diag) : pass_form2(p, n, 0, 0.f, guesses, diag);
    const float mean = acc / cnt;
    acc = form == 1 ? ex_redo(g_sh, p, 0, n, 0.f, 1, mean, diag) : pass_form2(p, n, 1, mean, guesses, diag);
    *mean_out = mean;
    *sd_out = std::sqrt(acc / cnt);
}

float emu_plain_sum(const float* p, size_t b, size_t e, float acc, int pass, float mean) {
    for (size_t i = b; i < e; ++i) acc += pass ? (p[i] - mean) * (p[i] - mean) : p[i];
    return acc;
}

void emu_plain(const float* p, size_t n, float cnt, float* mean_out, float* sd_out) {
    const float mean = emu_plain_sum(p, 0, n, 0.f, 0, 0.f) / cnt;
    *mean_out = mean;
    *sd_out = std::sqrt(emu_plain_sum(p, 0, n, 0.f, 1, mean) / cnt);
}

}  // extern "C"
