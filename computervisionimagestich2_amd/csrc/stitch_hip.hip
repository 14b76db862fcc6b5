// libstitch_hip.so -- host side of the C ABI in include/stitch.h: argument checks, device workspace (plans),
// launch sequencing on HIP streams, per-stage event timing.  All arithmetic is in stitch_kernels.hpp (and the k_*.inc parts it includes).
// Built for gfx950 only (hipcc --offload-arch=gfx950 -ffp-contract=off); there is no CPU path in this library.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <algorithm>
#include <cstring>
#include <atomic>
#include <condition_variable>
#include <functional>
#include <list>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "stitch.h"
#include "stitch_g_flags.h"
#include "stitch_index_plane.h"
#include "stitch_mask_keep.h"
#include "stitch_collapse_sides.h"
#include "stitch_src_runs.h"
#include "stitch_handoff.h"
#include "stitch_mask_rows.h"
#include "stitch_panorama.h"
#include "stitch_rig.h"
#include "stitch_exposure.h"
#include "stitch_rig_exposure.h"
#include "stitch_rig_exposure_temporal.h"
#include "stitch_calibrate.h"
#include "stitch_rig_seams.h"
#include "stitch_rig_crop.h"
#include "stitch_rig_formats.h"
#include "stitch_rig_formats_yuv.h"
#include "stitch_rig_monitor.h"
#include "stitch_rig_scale.h"
#include "stitch_seam_path.h"
#include "stitch_seam_anchor.h"
#include "stitch_kernels.hpp"

#pragma clang fp contract(off)

using namespace sk;

namespace {

thread_local std::string g_err;

// The HIP runtime multiplexes streams onto 4 hardware queues unless GPU_MAX_HW_QUEUES says otherwise, and launch sequences on
// streams that share a queue serialise behind each other (four sequences in flight: 1.50 ms per pair on 4 queues, 1.31 on 8).
// The variable is read when the runtime initialises, so it has to be in the environment before the process's first HIP call:
// stitch_init() (below, C ABI) puts it there -- called by whoever owns the process start-up (the C++ adaptor's static
// initialiser, the Python package's import, bench.py), never from a library constructor: setenv() races with getenv() in a host
// that already runs threads, and a dlopen() after HIP is up would change nothing anyway.

int fail(int code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_err = buf;
    return code;
}

#define HIPCHK(expr)                                                                                              \
    do {                                                                                                          \
        hipError_t e_ = (expr);                                                                                   \
        if (e_ != hipSuccess) return fail(STITCH_ERR_HIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), \
                                          __FILE__, __LINE__);                                                   \
    } while (0)

int need_device() {
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n <= 0) {
        (void)hipGetLastError();
        return fail(STITCH_ERR_NO_DEVICE, "no HIP device visible (hipGetDeviceCount: %s); this library has no CPU path",
                    e == hipSuccess ? "0 devices" : hipGetErrorString(e));
    }
    return STITCH_OK;
}

inline hipStream_t as_stream(void* s) { return reinterpret_cast<hipStream_t>(s); }
inline size_t align256(size_t v) { return (v + 255) & ~size_t(255); }
constexpr double kPI = 3.14159265358979323846;  // cimg::PI

// Projection.cpp:24-28: flag, width/height swap, tanVal rounded to float, r = (width/2.0)/tanVal stored to float
struct ProjParams {
    int flag, width, height;
    float r;
};
ProjParams proj_params(int w, int h, float fov_deg) {
    ProjParams p;
    p.flag = w > h;
    p.width = p.flag ? h : w;
    p.height = p.flag ? w : h;
    const float tanVal = (float)std::tan((double)fov_deg * kPI / 180.0);
    p.r = (float)((p.width / 2.0) / tanVal);
    return p;
}

// CImg.h:35053-35065 + :34889-34903
VVK make_vvk(float sigma) {
    const float nsigma = sigma >= 0 ? sigma : -sigma;
    const double nnsigma = nsigma < 0.5f ? 0.5f : nsigma, m0 = 1.16680, m1 = 1.10783, m2 = 1.40586, m1sq = m1 * m1,
                 m2sq = m2 * m2,
                 q = (nnsigma < 3.556 ? -0.2568 + 0.5784 * nnsigma + 0.0561 * nnsigma * nnsigma
                                      : 2.5091 + 0.9804 * (nnsigma - 3.556)),
                 qsq = q * q, scale = (m0 + q) * (m1sq + m2sq + 2 * m1 * q + qsq),
                 b1 = -q * (2 * m0 * m1 + m1sq + m2sq + (2 * m0 + 4 * m1) * q + 3 * qsq) / scale,
                 b2 = qsq * (m0 + 2 * m1 + 3 * q) / scale, b3 = -qsq * q / scale, B = (m0 * (m1sq + m2sq)) / scale;
    const double sumsq = B, sum = sumsq * sumsq, a1 = -b1, a2 = -b2, a3 = -b3,
                 scaleM = 1.0 / ((1.0 + a1 - a2 + a3) * (1.0 - a1 - a2 - a3) * (1.0 + a2 + (a1 - a3) * a3));
    VVK k;
    k.f1 = a1;
    k.f2 = a2;
    k.f3 = a3;
    k.sumsq = sumsq;
    k.sum = sum;
    k.den = 1.0 - a1 - a2 - a3;
    k.M[0] = scaleM * (-a3 * a1 + 1.0 - a3 * a3 - a2);
    k.M[1] = scaleM * (a3 + a1) * (a2 + a3 * a1);
    k.M[2] = scaleM * a3 * (a1 + a3 * a2);
    k.M[3] = scaleM * (a1 + a3 * a2);
    k.M[4] = -scaleM * (a2 - 1.0) * (a2 + a3 * a1);
    k.M[5] = -scaleM * a3 * (a3 * a1 + a3 * a3 + a2 - 1.0);
    k.M[6] = scaleM * (a3 * a1 + a2 + a1 * a1 - a2 * a2);
    k.M[7] = scaleM * (a1 * a2 + a3 * a2 * a2 - a1 * a3 * a3 - a3 * a3 * a3 - a3 * a2 + a3);
    k.M[8] = scaleM * a3 * (a1 + a3 * a2);
    return k;
}

// CImg.h:34801-34816,34840-34841 (float throughout; std::exp(float) is the float overload)
DRK make_drk(float sigma) {
    const float nsigma = sigma >= 0 ? sigma : -sigma;
    const float nnsigma = nsigma < 0.1f ? 0.1f : nsigma, alpha = 1.695f / nnsigma, ema = std::exp(-alpha),
                ema2 = std::exp(-2 * alpha), b1 = -2 * ema, b2 = ema2;
    const float kk = (1 - ema) * (1 - ema) / (1 + 2 * alpha * ema - ema2);
    DRK k;
    k.a0 = kk;
    k.a1 = kk * (alpha - 1) * ema;
    k.a2 = kk * (alpha + 1) * ema;
    k.a3 = -kk * ema2;
    k.b1 = b1;
    k.b2 = b2;
    k.coefp = (k.a0 + k.a1) / (1 + b1 + b2);
    k.coefn = (k.a2 + k.a3) / (1 + b1 + b2);
    return k;
}

// pyramid_sizes (stitch_call_form.h) with the reasons spelled out
int pyramid_levels(int w, int h, int level_rule, int* lw, int* lh) {
    const int levels = pyramid_sizes(w, h, level_rule, lw, lh);
    if (levels == 0) return fail(STITCH_ERR_ARG, "pyramid: non-positive size %dx%d", w, h);
    if (levels == -1) return fail(STITCH_ERR_PYRAMID, "pyramid: %dx%d gives 0 levels", w, h);  // (an int's side cannot give more than 32)
    if (levels < 0)
        return fail(STITCH_ERR_PYRAMID, "pyramid: level %d of %dx%d has a zero dimension (the reference degenerates here)", -levels - 2, w, h);
    return levels;
}

constexpr int WF_CTRL_WORDS = 4 * 16 + 16;  // band-queue heads of up to 4 levels (64 bytes apart) + the abort word
constexpr int IDX_HEAD_WORDS = 64, IDX_TODO_WORD = 16;  // in front of a plan's seam records: three counts, from word 16 the slots' todo words (k_index_keys)
constexpr int MK_COUNT_WORD = 32, MK_TODO_WORD = 48;    // in the same head: the mask pyramids' two counts, the time-out count k_mask_keys saw last, and the slots' mask_todo words
constexpr int WF_STICKY_WORDS = 16;         // behind them, outside what a launch sequence clears: the plan's count of timed-out waits and,
                                            // from word 2, its three 64-bit hand-off counts (stitch_plan_handoff_counts)

struct ProfRec {
    int stage, level;
    hipEvent_t a, b;
};

}  // namespace

// A plan: its shape (stitch_call_form.h: sizes, switches, which forms it was built for) and the device memory carved for it.
struct stitch_plan : PlanShape {
    int device = 0;
    int last_n = 0;         // pairs of the last call
    CallForm last_form{};   // the form of the last call (which flag arrays it wrote: stitch_plan_g_flag_counts, stitch_plan_mask_row_counts)
    void* arena = nullptr;
    size_t arena_bytes = 0;
    float* T = nullptr;   // blur scratch, 7 planes of level 0 + slack
    float* T2 = nullptr;  // Deriche temporaries (blur_kind 1 only)
    double* state = nullptr;
    u64* wf_yg = nullptr;
    size_t wf_yg_bytes = 0;
    unsigned* wf_ctrl = nullptr;   // per level one band-queue head (16 words apart), then the abort flag
    uint8_t* zi = nullptr;         // [cap][tiles][bands] of level 0: "every pixel of the tile lies outside the frame" (k_src_index)
    uint8_t* zt = nullptr;         // zero-tile flags of T, [7*cap][bands][tiles] of level 0 (ZeroTiles); reused level by level
    uint8_t* gz[2] = {nullptr, nullptr};  // G column flags of levels 1 and 2, [7*cap][tile columns] (g_cols)
    uint8_t* mr[2] = {nullptr, nullptr};  // row-repeat flags of the mask plane of levels 1 and 2, [cap][tile columns][bands] (mask_rows)
    const float* zero_page = nullptr;  // 4 KB of zeros in the arena (k_vv_xby_m's loader reads a flagged tile from here)
    int wf_max_wgs = WF_MAX_WGS;  // persistent workgroups of the fused sweep (STITCH_XBYF_WGS)
    unsigned wf_spin_limit = WF_SPIN_LIMIT;  // polls before a hand-off wait gives up (STITCH_XBYF_SPIN_LIMIT)
    int wf_early_read = 1;  // STITCH_XBYF_EARLY=0: poll for the hand-off only when it is needed
    double* ckpt = nullptr;  // STITCH_RECOMPUTE: [3][tiles of level 0][lines of level 0]
    unsigned long long* d7_dbg = nullptr;  // STITCH_D7_STAMP=<level>: k_vv_y_bwd_dec7's per-chunk stamps of one workgroup at that level (diagnostics)
    int d7_dbg_chunks = 0;
    unsigned long long* xy_dbg = nullptr;  // STITCH_XBYM_STAMP=1: k_vv_xby_m's per-tile stamps of one band of the last level-0 launch (diagnostics)
    int xy_dbg_nc = 0;
    unsigned long long* wf_dbg = nullptr;  // STITCH_WAVEFRONT_STAMP=1: [wf_max_wgs][8] segment cycle sums (diagnostics)
    // pinned copy of the plan's sticky count of timed-out hand-off waits, refreshed at the end of every call.  The device
    // word only grows (no launch sequence clears it), so the last copy covers every earlier queued call as well.
    unsigned* h_wf_abort = nullptr;
    unsigned wf_abort_seen = 0;  // count already acknowledged by stitch_plan_clear_fault
    float* side = nullptr;  // [cap][pitch0] x-blurred level-0 mask rows (implicit level-0 mask)
    unsigned long long* co_dbg = nullptr;  // STITCH_COARSE_STAMP=1: k_coarse's phase stamps of the last launch (diagnostics)
    SeamDev* d_seam = nullptr;
    SeamDev* h_seam = nullptr;  // pinned
    // The level-0 index planes in the plan's slots (k_index_keys): per slot what its plane and `zi` bytes were computed from, and in
    // front of the seam records IDX_HEAD_WORDS words -- the last call's three counts, then per slot "compute the plane in this call".
    // The head travels to the pinned copy with the seam records.
    IndexKey* idx_keys = nullptr;
    unsigned* idx_head = nullptr;    // device: IDX_HEAD_WORDS words in front of d_seam
    unsigned* h_idx_head = nullptr;  // pinned: the same words in front of h_seam (the allocation h_seam lives in)
    bool last_idx = false;           // the last call went through k_index_keys (stitch_plan_index_counts)
    // The mask pyramids in the plan's slots (k_mask_keys, include/stitch_mask_keep.h): per slot the seam record and the form word its mask
    // planes were computed under; in the head, the last call's two counts and per slot "compute the mask planes in this call".
    MaskKey* mask_keys = nullptr;
    // The same planes in 16-byte runs (SrcRuns, k_compose.inc), [cap][bands][tiles] of level 0: written by k_src_runs behind k_src_index,
    // valid exactly where the slot's IndexKey is.  last_runs: the last call's sweep was handed them; last_owner: that call's idx_pr.
    SrcRuns runs{};
    size_t runs_bytes = 0;  // bases, patches and classes are one region of the arena, starting at runs.bases
    bool last_runs = false;
    int last_owner[MAXB] = {};
    // the last call's level-0 launch of k_collapse4 (stitch_plan_collapse_sides): its column range as the caller's addresses left it,
    // and whether its workgroups chose a form by the seam's step
    int c4_l0_xa = 0, c4_l0_xb = 0;
    bool c4_l0_sides = false;
    hipStream_t last_stream = nullptr;
    bool pending = false;
    VVK vvk{};
    DRK drk{};
    bool profiling = false;
    int prof_only = -1;  // >= 0: record events only around launches of this kernel id
    std::vector<ProfRec> recs;
    std::vector<hipEvent_t> free_events;
};

Tuning sk::Tuning::from_env() {
    Tuning t{};
    t.wavefront = env_int("STITCH_WAVEFRONT");
    t.no_fuse = env_int("STITCH_NO_FUSE") > 0;
    t.no_src_fuse = env_int("STITCH_NO_SRC_FUSE") > 0;
    t.no_zero_tiles = env_int("STITCH_NO_ZERO_TILES") > 0;
    t.crows_l0 = env_int("STITCH_CROWS_L0");
    t.crows_ln = env_int("STITCH_CROWS_LN");
    t.collapse4 = env_int("STITCH_COLLAPSE4");
    t.xbyf_wgs = env_int("STITCH_XBYF_WGS");
    t.xbyf_spin_limit = env_int("STITCH_XBYF_SPIN_LIMIT");
    t.xbyf_early = env_int("STITCH_XBYF_EARLY");
    t.y2 = env_int("STITCH_Y2") > 0;
    t.recompute = env_int("STITCH_RECOMPUTE");
    t.stamp = env_int("STITCH_WAVEFRONT_STAMP") > 0;
    t.gate64 = env_int("STITCH_GATE64") > 0;
    t.coarse = env_int("STITCH_COARSE");
    t.single_fast = env_int("STITCH_SINGLE_FAST");
    t.odd_dec = env_int("STITCH_ODD_DEC");
    t.c4_gen = env_int("STITCH_C4_GEN");
    t.collapse_px = env_int("STITCH_COLLAPSE_PX");
    t.y1s = env_int("STITCH_Y1S");
    t.c4_lock = env_int("STITCH_C4_LOCKSTEP");
    t.c4_swz = env_int("STITCH_C4_SWIZZLE");
    t.mover = env_int("STITCH_MOVER");
    t.src_lone = env_int("STITCH_SRC_LONE_MPIX");
    t.dec7 = env_int("STITCH_DEC7");
    t.xbym = env_int("STITCH_XBYM");
    t.xbym_mpix = env_int("STITCH_XBYM_MPIX");
    t.coarse_lds = env_int("STITCH_COARSE_LDS");
    t.pitch_pad = env_int("STITCH_PITCH_PAD");
    t.crows_wgs = env_int("STITCH_CROWS_WGS");
    return t;
}

namespace {

struct StageTimer {  // records a pair of events around a group of launches when profiling is on
    stitch_plan* p;
    hipStream_t s;
    ProfRec r{};
    bool on;
    StageTimer(stitch_plan* plan, hipStream_t st, int stage, int level)
        : p(plan), s(st), on(plan->profiling && (plan->prof_only < 0 || plan->prof_only == stage)) {
        if (!on) return;
        r.stage = stage;
        r.level = level;
        auto get = [&](hipEvent_t& e) {
            if (!p->free_events.empty()) {
                e = p->free_events.back();
                p->free_events.pop_back();
            } else
                (void)hipEventCreate(&e);
        };
        get(r.a);
        get(r.b);
        (void)hipEventRecord(r.a, s);
    }
    ~StageTimer() {
        if (!on) return;
        (void)hipEventRecord(r.b, s);
        p->recs.push_back(r);
    }
};

dim3 grid_xy(int pitch_or_w, int h, int z = 1) { return dim3((pitch_or_w + 255) / 256, h, z); }

int launch_check(const char* what) {
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(STITCH_ERR_HIP, "launch of %s failed: %s", what, hipGetErrorString(e));
    return STITCH_OK;
}

// The hand-off buffers and limits of a fused sweep: a plan's (level l's queue head) or a band's
struct Handoff {
    u64* yg;
    unsigned *head, *abort, *sticky;
    unsigned spin_limit;
    int early_read;
};
Handoff handoff_of(const stitch_plan* p, int l) {
    return Handoff{p->wf_yg, p->wf_ctrl + (size_t)l * 16, p->wf_ctrl + WF_CTRL_WORDS - 16, p->wf_ctrl + WF_CTRL_WORDS, p->wf_spin_limit, p->wf_early_read};
}

// The hand-off record of a fused sweep (k_vv_xbyf, k_vv_xby_m) of np planes of NR x NC tiles, behind the clear of its granules: every
// polled word is cleared in front of the launch (never told apart by a per-launch argument: a captured graph replays frozen arguments,
// and stale tags from the previous replay would match at once)
Wavefront wavefront_of(const Handoff& h, int np, int NR, int NC, const ZeroTiles& zt, hipStream_t s) {
    Wavefront wf{};
    wf.yg = h.yg;
    wf.counter = h.head;
    wf.abort = h.abort;
    wf.sticky = h.sticky;
    wf.spin_limit = h.spin_limit;
    wf.NR = NR;
    wf.NC = NC;
    wf.NP = np;
    wf.epoch = 1;
    wf.zt = zt;
    wf.early_read = h.early_read;
    const size_t gran_words = (size_t)wf.NP * wf.NC * WF_GRAN * WAVE;
    k_clear_words<<<(int)std::min<size_t>((gran_words + 255) / 256, 2048), 256, 0, s>>>(h.yg, gran_words);
    return wf;
}

// The batch's fused anticausal-x + causal-y sweep: the diagnostic instance, the two that re-run the causal x sweep (MODE 2 from the
// frames), the plain one, and a band's (BANDED: rows y0 .. of planes ph rows high, from a resume state)
template <typename PX>
void launch_xbyf(int wg, hipStream_t s, bool stamp, bool rcmp, bool src0, bool banded, float* T, int w, int h, int pitch, const VVK& k, double* state, long lines,
                 double* state_y, const Wavefront& wf, const Recompute& rcv, const PairArgs<PX>& pa) {
    if (stamp)
        k_vv_xbyf<true><<<wg, 64, 0, s>>>(T, w, h, pitch, k, state, lines, state_y, wf, rcv, NoPairArgs{});
    else if (rcmp && src0)
        k_vv_xbyf<false, PX, 2><<<wg, 64, 0, s>>>(T, w, h, pitch, k, state, lines, state_y, wf, rcv, pa);
    else if (rcmp)
        k_vv_xbyf<false, float, 1><<<wg, 64, 0, s>>>(T, w, h, pitch, k, state, lines, state_y, wf, rcv, NoPairArgs{});
    else if (banded)
        k_vv_xbyf<false, float, 0, true><<<wg, 64, 0, s>>>(T, w, h, pitch, k, state, lines, state_y, wf, rcv, NoPairArgs{});
    else
        k_vv_xbyf<false><<<wg, 64, 0, s>>>(T, w, h, pitch, k, state, lines, state_y, wf, rcv, NoPairArgs{});
}

// The source and the destination of the fused anticausal-y sweep + decimation: np planes of T (h rows of a level h_full rows high) into
// the planes of the next level
struct DecPlanes {
    float* p;
    int w, h, pitch;
    size_t ps;
    int h_full;
};
// k_vv_y_bwd_dec<rowz, YST, zt, odd, xch> of the record, every instance either path has (the odd one: three-tap x decimation,
// workgroups overlap by two columns; xch: columns from x0 with the chunk's own state arrays, `cols` of them)
void launch_y_bwd_dec(const DecInstance& i, int np, hipStream_t s, const DecPlanes& a, const DecPlanes& b, const VVK& k, const double* ystate, const ZeroTiles& zt,
                      const double* resume, double* state_out, int x0, int cols, int fill_l0, const ZeroTiles& gout, const ZeroTiles& mout,
                      const unsigned* keep = nullptr) {
    const dim3 g = i.odd ? dim3((b.w + WAVE - 2) / (WAVE - 1), np) : dim3((cols + YCOLS - 1) / YCOLS, np);
    auto go = [&](auto R, auto Z, auto O, auto X) {
        k_vv_y_bwd_dec<decltype(R)::value, YST, decltype(Z)::value, decltype(O)::value, decltype(X)::value>
            <<<g, 128, 0, s>>>(a.p, a.w, a.h, a.pitch, a.ps, k, ystate, b.p, b.w, b.h, b.pitch, b.ps, zt, resume, state_out, a.h_full, b.h_full, x0, fill_l0, gout, mout, keep);
    };
    const std::true_type y{};
    const std::false_type no{};
    if (i.xch)
        i.rowz ? go(y, y, no, y) : go(no, y, no, y);
    else if (!i.zt)
        i.odd ? go(no, no, y, no) : go(no, no, no, no);
    else if (i.rowz)
        i.odd ? go(y, y, y, no) : go(y, y, no, no);
    else
        i.odd ? go(no, y, y, no) : go(no, y, no, no);
}

// One level of the collapse: the clamp of [xa, xb) by the caller's addresses at level 0, the grid, the instance.  Columns [xa, xb) go
// four per work-item (k_collapse4: dense, GEN, MR instances), the rest of `cols` one per work-item in the same launch; a level without
// such a range runs k_collapse, or k_collapse_px where the record says so.  whole_words (a band): the range stands only where every
// destination row is whole groups of four samples and the buffer is aligned to one; a plan's rule otherwise (u8_words: rows start on
// 32-bit boundaries).
struct CollapseKind {
    bool dense, gen, px, mr, whole_words;
};
template <typename OUT, bool L0>
void launch_collapse(CollapseArgs<OUT, L0>& A, const CollapseKind& kd, int cols, int strips, int n, const MaskRowsArg& mra, hipStream_t s) {
    if constexpr (L0) {  // what the caller's addresses take away from the record
        if (kd.whole_words) {
            if ((A.w % 4) != 0 || (reinterpret_cast<uintptr_t>(A.outs.p[0]) % (4 * sizeof(OUT))) != 0) A.xa = A.xb = 0;
        } else {
            A.u8_words = (A.w % 4) == 0;  // unsigned char rows start on 32-bit boundaries
            for (int i = 0; i < n; ++i) {
                if (sizeof(OUT) == 1) A.u8_words = A.u8_words && (reinterpret_cast<uintptr_t>(A.outs.p[i]) % 4) == 0;
                A.u8_words = A.u8_words && (reinterpret_cast<uintptr_t>(A.outs.q[i]) % 4) == 0;
                if (sizeof(OUT) == 4 && (reinterpret_cast<uintptr_t>(A.outs.p[i]) % 4) != 0) A.xa = A.xb = 0;  // a float canvas that is not even 4-byte aligned
            }
        }
    }
    const int xa = A.xa, xb = A.xb, rest = cols - (xb - xa);
    const int nb4 = ((xb - xa) / 4 + WAVE - 1) / WAVE, ncb = (rest + C4_THREADS - 1) / C4_THREADS;
    const dim3 g4(c4_padded_blocks(nb4, A.swizzle) + ncb * C4_SUB, strips, n), g1 = grid_xy(cols, strips, n);
    if constexpr (L0) {
        if (xb > xa && kd.dense && kd.gen)
            k_collapse4<OUT, true, true, true><<<g4, C4_THREADS, 0, s>>>(A, nb4, ncb);
        else if (xb > xa && kd.dense)
            k_collapse4<OUT, true, true><<<g4, C4_THREADS, 0, s>>>(A, nb4, ncb);
        else if (xb > xa && kd.gen)
            k_collapse4<OUT, true, false, true><<<g4, C4_THREADS, 0, s>>>(A, nb4, ncb);
        else if (xb > xa)
            k_collapse4<OUT, true><<<g4, C4_THREADS, 0, s>>>(A, nb4, ncb);
        else
            k_collapse<OUT, true><<<g1, 256, 0, s>>>(A);
    } else if (kd.mr) {  // the instances that take the mask sample of a flagged tile from row 0
        if (xb > xa && kd.gen)
            k_collapse4<float, false, false, true, true><<<g4, C4_THREADS, 0, s>>>(A, nb4, ncb, mra);
        else if (xb > xa)
            k_collapse4<float, false, false, false, true><<<g4, C4_THREADS, 0, s>>>(A, nb4, ncb, mra);
        else if (kd.px)
            k_collapse_px<true><<<grid_xy(A.pitch, A.h, n), 256, 0, s>>>(A, mra);
        else
            k_collapse<float, false, true><<<g1, 256, 0, s>>>(A, mra);
    } else if (xb > xa && kd.gen)
        k_collapse4<float, false, false, true><<<g4, C4_THREADS, 0, s>>>(A, nb4, ncb);
    else if (xb > xa)
        k_collapse4<float, false><<<g4, C4_THREADS, 0, s>>>(A, nb4, ncb);
    else if (kd.px)
        k_collapse_px<<<grid_xy(A.pitch, A.h, n), 256, 0, s>>>(A);
    else
        k_collapse<float, false><<<g1, 256, 0, s>>>(A);
}

// REDUCE for every level (ImageProcess.cpp:705-715): blur(G_l) into T, decimate T into G_{l+1}.  Which kernels: the call's form
// (stitch_call_form.h); here are their arguments.
template <typename PX>
int run_reduce(stitch_plan* p, const CallForm& c, hipStream_t s, const PairArgs<PX>& pa, const ZeroTiles& zi, const SrcRuns& sr = SrcRuns{}, const unsigned* keep = nullptr) {
    const int n = c.n, np = 7 * n;  // planes in flight: every launch covers all pairs of the batch
    if (c.wf_ctrl) k_clear_words<<<1, 256, 0, s>>>((u64*)p->wf_ctrl, WF_CTRL_WORDS / 2);  // band-queue heads + abort flag
    for (int l = 0; l < c.l_end; ++l) {
        const LevelForm& f = c.lv[l];
        const Level& a = p->lv[l];
        const Level& b = p->lv[l + 1];
        const long lines = (long)np * a.h;
        MaskL0 mk{};
        if (f.mask_l0) mk = MaskL0{p->d_seam, p->side, a.h, 1};
        mk.h = a.h, mk.keep = keep;  // the slots' mask_todo words, for every kernel of the level that takes MaskL0 (mask_stands)
        const ZeroTiles none{};
        const ZeroTiles zt = f.zt ? ZeroTiles{p->zt, a.h, f.NR, f.NC} : none;
        // G column flags and row-repeat flags of the mask plane: of this level for its readers, of the next for the sweep that produces them
        const ZeroTiles gin = f.g_in ? g_cols(p->gz[l - 1], a.w) : none, gout = f.g_out ? g_cols(p->gz[l], b.w) : none;
        const ZeroTiles min_ = f.mr_in ? mask_rows(p->mr[l - 1], a.w, a.h) : none, mout = f.mr_out ? mask_rows(p->mr[l], b.w, b.h) : none;
        const Bands bd = f.per_plane ? Bands{f.NR, a.h} : Bands{};
        const int xstage = f.src0 ? STITCH_K_VV_X_FWD_SRC : STITCH_K_VV_X_FWD;
        // the x-sweep state lives in state[0 .. 4*lines); the y state a fused sweep leaves goes behind it
        double* state_y = p->state + 4 * (size_t)p->cap * 7 * (a.h + 64);
        const double* ystate = f.sweep == SW_BATCH || f.xby ? state_y : p->state;  // where the causal y sweep leaves its state for the anticausal one
        const dim3 gy((a.pitch + YCOLS - 1) / YCOLS, np), gy1(a.pitch / WAVE, np);

        if (f.x_fwd == XF_COPY)
            HIPCHK(hipMemcpyAsync(p->T, a.g, sizeof(float) * a.ps * np, hipMemcpyDeviceToDevice, s));
        else {
            StageTimer t(p, s, xstage, l);
            if (f.x_fwd == XF_M) {
                if (f.src0)
                    k_vv_x_m<true, PX, true><<<f.nbx, 192, 0, s>>>(a.g, p->T, a.w, a.pitch, lines, p->vvk, p->state, mk, bd, pa);
                else
                    k_vv_x_m<true><<<f.nbx, 192, 0, s>>>(a.g, p->T, a.w, a.pitch, lines, p->vvk, p->state, mk, bd, NoPairArgs{});
            } else if (f.src0) {
                if (f.rcmp)
                    k_vv_x_fwd<PX, true, true><<<f.nbx, 64, 0, s>>>(a.g, p->T, a.w, a.pitch, lines, p->vvk, p->state, mk, pa, zt, zi, p->ckpt, bd);
                else
                    k_vv_x_fwd<PX, true><<<f.nbx, 64, 0, s>>>(a.g, p->T, a.w, a.pitch, lines, p->vvk, p->state, mk, pa, zt, zi, nullptr, bd, none, sr);
            } else if (f.rcmp)
                k_vv_x_fwd<PX, false, true><<<f.nbx, 64, 0, s>>>(a.g, p->T, a.w, a.pitch, lines, p->vvk, p->state, mk, NoPairArgs{}, zt, none, p->ckpt, bd);
            else
                k_vv_x_fwd<PX, false><<<f.nbx, 64, 0, s>>>(a.g, p->T, a.w, a.pitch, lines, p->vvk, p->state, mk, NoPairArgs{}, zt, gin, nullptr, bd, min_);
        }
        if (f.x_bwd != XB_NONE || f.x_fwd == XF_M) {  // (the stage is timed behind k_vv_x_m even where the fused sweep takes its work)
            StageTimer t(p, s, STITCH_K_VV_X_BWD, l);
            if (f.x_bwd == XB_M)
                k_vv_x_m<false><<<f.nbx, 192, 0, s>>>(p->T, p->T, a.w, a.pitch, lines, p->vvk, p->state, mk, bd, NoPairArgs{});
            else if (f.x_bwd == XB_BWD)
                k_vv_x_bwd<<<f.nbx, 64, 0, s>>>(p->T, a.w, a.pitch, lines, p->vvk, p->state, mk, bd);
        }
        int fill_l0 = 0;
        if (f.sweep == SW_BATCH) {
            Wavefront wf = wavefront_of(handoff_of(p, l), np, f.NR, f.NC, zt, s);
            wf.mask_l0 = f.mask_l0 ? (f.zt ? 2 : 1) : 0;  // 2: the mask blur below the first band is recorded in the flags, not stored
            if (f.fill_mask && l > 0) wf.mr = min_;
            fill_l0 = f.fill_mask;  // flagged tiles of the mask planes repeat the plane's row 0
            StageTimer t(p, s, STITCH_K_VV_XBYF, l);
            const int wg = (int)std::min<long>((long)wf.NP * wf.NR, p->wf_max_wgs);  // one persistent wavefront per row band; at most 9 workgroups per CU by LDS
            Recompute rcv{};
            if (f.rcmp) {
                rcv.in = a.g;
                rcv.ckpt = p->ckpt;
                rcv.seam = p->d_seam;
                if (f.src0) rcv.zi = zi;
            }
            if (f.stamp) wf.dbg = p->wf_dbg;  // diagnostic build: per-segment cycle sums of the level-0 launch
            launch_xbyf<PX>(wg, s, f.stamp, f.rcmp, f.src0, false, p->T, a.w, a.h, a.pitch, p->vvk, p->state, lines, state_y, wf, rcv, pa);
        } else if (f.xby) {
            Wavefront wf = wavefront_of(handoff_of(p, l), np, f.NR, f.NC, zt, s);
            wf.mask_l0 = f.mask_l0;
            if (p->xy_dbg && l == 0) wf.dbg = p->xy_dbg, p->xy_dbg_nc = wf.NC;
            StageTimer t(p, s, STITCH_K_VV_XBYF, l);
            // two workgroups per CU by LDS: every band of a lone 6144 x 4096 pair (448) is resident at once
            k_vv_xby_m<<<(int)std::min<long>((long)wf.NP * wf.NR, XY_WGS), XY_THREADS, 0, s>>>(p->T, a.w, a.h, a.pitch, p->vvk, p->state, lines, state_y, wf, p->zero_page);
        } else if (f.sweep == SW_DERICHE) {
            if (f.do_x) {
                StageTimer t(p, s, xstage, l);
                k_deriche<<<(int)((lines + 63) / 64), 64, 0, s>>>(p->T, p->T2, a.w, 1, a.pitch, a.h, a.ps, lines, p->drk);
            }
            if (f.do_y) {
                StageTimer t(p, s, STITCH_K_VV_Y_FWD, l);
                const long cols = (long)np * a.w;
                k_deriche<<<(int)((cols + 63) / 64), 64, 0, s>>>(p->T, p->T2, a.h, a.pitch, 1, a.w, a.ps, cols, p->drk);
            }
        }
        if (f.y_fwd != YF_NONE) {
            StageTimer t(p, s, STITCH_K_VV_Y_FWD, l);
            if (f.y_fwd == YF_M)
                k_vv_y_m<true><<<gy1, 192, 0, s>>>(p->T, a.h, a.pitch, a.ps, p->vvk, p->state, mk);
            else if (f.y_fwd == YF_FWD1S)
                k_vv_y_fwd1s<8><<<gy1, 64, 0, s>>>(p->T, a.h, a.pitch, a.ps, p->vvk, p->state, mk, nullptr);
            else if (f.y_fwd == YF_FWD1)
                k_vv_y_fwd1<<<gy1, 64, 0, s>>>(p->T, a.h, a.pitch, a.ps, p->vvk, p->state, mk, nullptr);
            else
                k_vv_y_fwd<<<gy, 64, 0, s>>>(p->T, a.h, a.pitch, a.ps, p->vvk, p->state, mk, nullptr);
        }
        if (f.y_bwd != YB_NONE) {
            StageTimer t(p, s, STITCH_K_VV_Y_BWD, l);
            if (f.y_bwd == YB_DEC)
                launch_y_bwd_dec(DecInstance{f.rowz, f.dec_zt, f.dec_odd, false}, np, s, DecPlanes{p->T, a.w, a.h, a.pitch, a.ps, a.h}, DecPlanes{b.g, b.w, b.h, b.pitch, b.ps, b.h},
                                 p->vvk, ystate, zt, nullptr, nullptr, 0, a.pitch, fill_l0, gout, mout, keep);
            else if (f.y_bwd == YB_BWD)
                k_vv_y_bwd<<<gy, 64, 0, s>>>(p->T, a.h, a.pitch, a.ps, p->vvk, ystate, nullptr, nullptr);
            else if (f.dec_odd)
                k_vv_y_bwd_dec7<true><<<dim3((b.w + WAVE - 2) / (WAVE - 1), np), D7_THREADS, 0, s>>>(p->T, a.w, a.h, a.pitch, a.ps, p->vvk, ystate, b.g, b.w, b.h, b.pitch, b.ps, nullptr, 0, keep);
            else {
                unsigned long long* dbg = p->d7_dbg && l == p->stamp_d7_level ? p->d7_dbg : nullptr;
                if (dbg) p->d7_dbg_chunks = (a.h + YCH - 1) / YCH;
                k_vv_y_bwd_dec7<false><<<gy, D7_THREADS, 0, s>>>(p->T, a.w, a.h, a.pitch, a.ps, p->vvk, ystate, b.g, b.w, b.h, b.pitch, b.ps, dbg, dbg ? Tuning::env_int("STITCH_D7_STAMP_MODE") : 0, keep);
            }
        }
        if (f.decimate) {
            StageTimer t(p, s, STITCH_K_DECIMATE, l);
            k_decimate<<<grid_xy(b.pitch, b.h, np), 256, 0, s>>>(p->T, a.w, a.h, a.pitch, a.ps, b.g, b.w, b.h, b.pitch, b.ps, 0, 0, keep);
        }
    }
    if (c.coarse) {  // every remaining level in one launch, one workgroup per pair; leaves E of level coarse_from
        StageTimer t(p, s, STITCH_K_COARSE, p->coarse_from);
        CoarseArgs ca{};
        ca.n = p->L - p->coarse_from;
        for (int i = 0; i < ca.n; ++i) {
            const Level& v = p->lv[p->coarse_from + i];
            ca.lv[i] = CoarseLevel{v.g, v.e, v.ix, v.iy, v.ax, v.ay, v.w, v.h, v.pitch, v.ps};
        }
        ca.T = p->T;
        ca.k = p->vvk;
        ca.dbg = p->co_dbg;
        if (c.coarse_lds) {
            CoarseLds lo{};
            bool fits;
            const size_t lds_bytes = sizeof(float) * coarse_lds_layout(*p, lo.p, lo.g, lo.e, &lo.t, &fits);
            static std::once_flag once;  // more than 64 KB of dynamic LDS is opt-in per function
            std::call_once(once, [] { (void)hipFuncSetAttribute(reinterpret_cast<const void*>(k_coarse_lds), hipFuncAttributeMaxDynamicSharedMemorySize, CO_LDS_BYTES); });
            k_coarse_lds<<<n, CO_THREADS, lds_bytes, s>>>(ca, lo);
        } else
            k_coarse<<<n, CO_THREADS, 0, s>>>(ca);
    }
    if (c.wf_ctrl) HIPCHK(hipMemcpyAsync(p->h_wf_abort, p->wf_ctrl + WF_CTRL_WORDS, sizeof(unsigned), hipMemcpyDeviceToHost, s));
    return launch_check("reduce");
}

template <typename OUT>
int run_collapse(stitch_plan* p, const CallForm& c, const OutPtrs<OUT>& outs, hipStream_t s, const PairArgs<OUT>& pa) {
    const int L = p->L, n = c.n;
    if (!c.coarse) {
        const Level& t = p->lv[L - 1];
        StageTimer tm(p, s, STITCH_K_COLLAPSE_TOP, L - 1);
        k_blend_top<<<grid_xy(t.pitch, t.h, n), 256, 0, s>>>(t.g, t.pitch, t.h, t.ps, t.e);
        if (L == 1) k_emit_top<OUT><<<grid_xy(t.w, t.h, n), 256, 0, s>>>(t.e, t.w, t.h, t.pitch, t.ps, outs);  // writes out_u8 too
    }
    // with k_coarse the chain arrives collapsed down to level coarse_from
    for (int l = c.l_end - 1; l >= 0; --l) {
        const LevelForm& f = c.lv[l];
        const Level& a = p->lv[l];
        const Level& nx = p->lv[l + 1];
        StageTimer tm(p, s, l == 0 ? STITCH_K_COLLAPSE_L0 : STITCH_K_COLLAPSE, l);
        // G column flags of this level and of the one it expands, row-repeat flags of this level's mask plane
        const ZeroTiles none{};
        const ZeroTiles gz = f.g_in ? g_cols(p->gz[l - 1], a.w) : none, gzn = f.g_out ? g_cols(p->gz[l], nx.w) : none;
        const ZeroTiles mrz = f.c_mr ? mask_rows(p->mr[l - 1], a.w, a.h) : none;
        const int cols = l == 0 ? a.w : a.pitch, strips = (a.h + f.crows - 1) / f.crows;
        const MaskRowsArg mra{mrz.flags, mrz.NC, mrz.NR};
        if (l == 0) {  // level 0: the mask is the seam's step function itself (never read from memory)
            CollapseArgs<OUT, true> A{a.g, a.w, a.h, a.pitch, a.ps, nx.g, nx.e, nx.w, nx.h, nx.pitch, nx.ps, {a.ix, a.ax, a.iy, a.ay}, outs,
                                      a.w, (size_t)a.w * a.h, p->mask_stored() ? nullptr : p->d_seam, pa, c.src ? 1 : 0, f.crows, f.xa, f.xb, 1,
                                      c.c4_lock, c.c4_swizzle};
            A.gzn = gzn.flags, A.gncn = gzn.NC, A.zon = (unsigned)(7 * (size_t)p->cap * nx.ps);
            launch_collapse(A, CollapseKind{c.src && c.a_dense, f.gen, false, false, false}, cols, strips, n, mra, s);
            p->c4_l0_xa = A.xa, p->c4_l0_xb = A.xb;
#ifdef STITCH_NO_C4_SIDES
            p->c4_l0_sides = false;
#else
            p->c4_l0_sides = A.seam_l0 != nullptr;
#endif
        } else {
            OutPtrs<float> eo{};
            eo.p[0] = a.e;
            CollapseArgs<float, false> A{a.g, a.w, a.h, a.pitch, a.ps, nx.g, nx.e, nx.w, nx.h, nx.pitch, nx.ps, {a.ix, a.ax, a.iy, a.ay}, eo,
                                         a.pitch, a.ps, nullptr, NoPairArgs{}, 0, f.crows, f.xa, f.xb, 1, c.c4_lock, c.c4_swizzle};
            A.gz = gz.flags, A.gnc = gz.NC, A.zo = (unsigned)(7 * (size_t)p->cap * a.ps);
            A.gzn = gzn.flags, A.gncn = gzn.NC, A.zon = (unsigned)(7 * (size_t)p->cap * nx.ps);
            launch_collapse(A, CollapseKind{false, f.gen, f.px, f.c_mr, false}, cols, strips, n, mra, s);
        }
    }
    return launch_check("collapse");
}

template <typename PX>
int run_seam_mask(stitch_plan* p, int n, hipStream_t s, const PairArgs<PX>& pa, bool src, const SeamInts* given, const PathArgs* paths, unsigned mask_form) {
    const Level& a = p->lv[0];
    if (paths) {  // include/stitch_seam_path.h (a masked plan): no scan -- zeroed records that carry the branch, and the mask plane from the paths
        {
            StageTimer t(p, s, STITCH_K_SEAM, 0);
            k_seam_pathed<<<1, 64, 0, s>>>(*paths, n, p->d_seam);
        }
        StageTimer t(p, s, STITCH_K_MASK, 0);
        k_mask_path<<<grid_xy(a.pitch / 4, a.h, n), 256, 0, s>>>(a.g, a.w, a.pitch, a.ps, *paths);
    } else if (given) {  // include/stitch_rig_seams.h: the records from the caller's integers instead of the scan
        StageTimer t(p, s, STITCH_K_SEAM, 0);
        k_seam_given<<<1, 64, 0, s>>>(*given, n, a.w, p->opts.seam_rule, p->d_seam);
    } else {
        StageTimer t(p, s, STITCH_K_SEAM, 0);
        // 256 work-items, not 1024: a 16-wavefront workgroup waits for a CU with that much room when other batches fill the chip
        // (1.7 ms per launch with four batches in flight)
        // (one pair per call: nothing else competes for the CU, and the scan is a chain of dependent map evaluations and gathers per
        // work-item -- 6 of them instead of 24 at 6144 columns)
        k_seam<PX><<<n, n == 1 ? 1024 : 256, 0, s>>>(a.g, a.w, a.h, a.pitch, a.ps, p->opts.seam_rule, p->d_seam, pa, src ? 1 : 0);
    }
    if (!p->mask_opt && !paths) {
        StageTimer t(p, s, STITCH_K_MASK, 0);
        k_mask<<<grid_xy(a.pitch, a.h, n), 256, 0, s>>>(a.g, a.w, a.pitch, a.ps, p->d_seam);
    }
    // whose mask pyramid stands: decided behind the records, in stream order (a captured sequence decides again on every replay)
    k_mask_keys<<<1, 64, 0, s>>>(p->d_seam, n, p->cap, mask_form, p->mask_keys, p->idx_head + MK_TODO_WORD, p->wf_ctrl ? p->wf_ctrl + WF_CTRL_WORDS : nullptr,
                                 p->idx_head + MK_COUNT_WORD);
    // (with the words in front of them: the index planes' and the mask pyramids' counts of this call)
    HIPCHK(hipMemcpyAsync(p->h_idx_head, p->idx_head, sizeof(unsigned) * IDX_HEAD_WORDS + sizeof(SeamDev) * n, hipMemcpyDeviceToHost, s));
    return launch_check("seam/mask");
}

int check_plan_call(stitch_plan* p, const void* a, const void* b, const void* out) {
    if (!p || !a || !b || !out) return fail(STITCH_ERR_ARG, "null plan or buffer");
    int dev = -1;
    HIPCHK(hipGetDevice(&dev));
    if (dev != p->device) return fail(STITCH_ERR_ARG, "plan belongs to device %d, current device is %d", p->device, dev);
    return STITCH_OK;
}

// Pairs i and j of a call have the same index plane: the fields of IndexKey, by bit pattern (one pixel type per call)
template <typename PX>
bool same_index_key(const PairArgs<PX>& pa, int i, int j) {
    return std::memcmp(pa.map[i].p, pa.map[j].p, sizeof pa.map[i].p) == 0 && std::memcmp(&pa.offx[i], &pa.offx[j], sizeof(float)) == 0 &&
           std::memcmp(&pa.offy[i], &pa.offy[j], sizeof(float)) == 0 && pa.fw[i] == pa.fw[j] && pa.fh[i] == pa.fh[j];
}

// The launch sequence of n pairs (or of one dense-canvas blend, pa.a_dense): S1, seam scan, REDUCE, collapse.
// given: the pairs' seams as their four integers (stitch_dev_pairs_seamed_*), or nullptr for the scan.
// paths: the pairs' seam paths and branches (stitch_dev_pairs_pathed_*, a masked plan: src is false), which replace scan and step mask.
template <typename PX>
int run_pairs(stitch_plan* p, const PairArgs<PX>& pa, const OutPtrs<PX>& outs, int n, hipStream_t s, bool src, const SeamInts* given = nullptr,
              const PathArgs* paths = nullptr) {
    const Level& a = p->lv[0];
    int rc;
    const CallForm c = call_form(*p, n, src, pa.a_dense != 0);  // every kernel choice of REDUCE and the collapse, before the first launch
    for (int i = 0; i < n; ++i) {  // a PairArgs that did not go through set_index_owners (all zeros: every pair reading slot 0) stops here
        const int o = pa.idx_pr[i];
        if (o < 0 || o > i || pa.idx_pr[o] != o || !same_index_key(pa, i, o)) return fail(STITCH_ERR_ARG, "pairs: pair %d names slot %d as the owner of its index plane", i, o);
    }
    // source-fused: level 0 is a function of the inputs, evaluated by its three consumers (a warped frame through an index
    // plane, dense images as pure shifts)
    ZeroTiles zi{};
    if (src && p->zero_tiles && !pa.a_dense) {
        zi.flags = p->zi;
        zi.h = a.h;
        zi.NR = (a.h + TS - 1) / TS;
        zi.NC = (a.w + TS - 1) / TS;
    }
    // the index planes in 16-byte runs for k_vv_x_fwd<PX, true>; the forms that gather elsewhere (k_vv_x_m, the CKPT sweep) do without
    SrcRuns runs{}, sr{};  // what k_src_runs writes; what this call's sweep is handed
#ifndef STITCH_NO_SRC_RUNS  // (the A/B library: every frame tile through the full index plane)
    runs = p->runs;
    if (src && !pa.a_dense && c.lv[0].src0 && c.lv[0].x_fwd == XF_FWD && !c.lv[0].rcmp) sr = runs;
#endif
    {
        StageTimer t(p, s, STITCH_K_COMPOSE, 0);
        if (src) {
            if (!pa.a_dense) {
                // the index plane of a slot is computed where the slot's record (IndexKey) does not describe this call's pair already,
                // and once for pairs of the call with equal keys; decided on the device, in stream order (k_index_keys)
                unsigned* todo = p->idx_head + IDX_TODO_WORD;
                k_index_keys<PX><<<1, 64, 0, s>>>(pa, n, p->idx_keys, todo, p->idx_head);
                if (zi.flags) k_zi_preset<<<dim3(4, n), 256, 0, s>>>(zi.flags, zi.NR * zi.NC, todo);
                k_src_index<PX><<<grid_xy(a.pitch, std::min((a.h + SI_ROWS - 1) / SI_ROWS, SI_WGY), n), 256, 0, s>>>(pa, a.g, a.w, a.h, a.pitch, a.ps, zi, 0, todo);
                // and the same plane in 16-byte runs, every tile of a computed slot -- whichever form this call's sweep takes: a later call
                // that finds the slot's record unchanged may take the other
                if (runs.cls) k_src_runs<PX><<<dim3(runs.NC, std::min(runs.NR, SR_WGY), n), 64, 0, s>>>(pa, a.g, a.h, a.pitch, a.ps, runs, todo);
            }  // (a dense pair has no index plane and writes nothing into the slot: the record stands)
        } else {
            if (pa.a_dense)
                k_load_canvases<PX><<<grid_xy(a.pitch, a.h), 256, 0, s>>>(pa.frame[0], pa.mosaic[0], a.g, a.w, a.h, a.pitch, a.ps);
            else
                k_compose<PX><<<grid_xy(a.pitch, a.h, n), 256, 0, s>>>(pa, a.g, a.w, a.h, a.pitch, a.ps, 0);
            k_index_forget<<<1, 64, 0, s>>>(p->idx_keys, n);  // level 0 of slots 0 .. n-1 now holds planes, not an index
        }
    }
    p->last_idx = src && !pa.a_dense;
    p->last_runs = sr.cls != nullptr;
    for (int i = 0; i < MAXB; ++i) p->last_owner[i] = pa.idx_pr[i];
    // the mask planes of a slot are computed where the slot's record (MaskKey) does not describe this call's seam and form already
    // (k_mask_keys); a call whose form does not know the skip hands no words on: its kernels compute every plane
    const unsigned mask_form = mask_keep_word(*p, c, paths != nullptr);
    if ((rc = run_seam_mask<PX>(p, n, s, pa, src, given, paths, mask_form))) return rc;
    p->last_form = c;
    if ((rc = run_reduce<PX>(p, c, s, pa, zi, sr, (mask_form & MK_KEEP_OK) ? p->idx_head + MK_TODO_WORD : nullptr))) return rc;
    if ((rc = run_collapse<PX>(p, c, outs, s, pa))) return rc;
    p->last_stream = s;
    p->pending = true;
    p->last_n = n;
    return STITCH_OK;
}

inline bool ranges_overlap(const void* a, size_t na, const void* b, size_t nb) {
    const uintptr_t x = reinterpret_cast<uintptr_t>(a), y = reinterpret_cast<uintptr_t>(b);
    return x < y + nb && y < x + na;
}

// blendTwoImages on two dense canvases: a pair whose "frame" is canvas a as it stands and whose "mosaic" is canvas b with a
// zero shift (PairArgs::a_dense).  Source-fused plans read both canvases where level 0 is needed -- no level-0 planes, no mask
// plane, no index plane; otherwise k_load_canvases materialises level 0.
template <typename PX>
int dev_blend(stitch_plan* p, const PX* d_a, const PX* d_b, PX* d_out, void* stream) {
    int rc = check_plan_call(p, d_a, d_b, d_out);
    if (rc) return rc;
    if (p->masked) return fail(STITCH_ERR_ARG, "blend: a masked plan takes stitch_dev_pairs_pathed_* alone (include/stitch_seam_path.h)");
    PairArgs<PX> pa{};
    pa.frame[0] = d_a;
    pa.mosaic[0] = d_b;
    pa.out[0] = d_out;
    pa.fw[0] = pa.mw[0] = p->cw;
    pa.fh[0] = pa.mh[0] = p->ch;
    pa.a_dense = 1;
    set_index_owners(pa, 1, nullptr);
    OutPtrs<PX> outs{};
    outs.p[0] = d_out;
    const size_t bytes = sizeof(PX) * (size_t)3 * p->cw * p->ch;
    // source-fused: a and b are read again by the causal x sweep and by the level-0 collapse WHILE d_out is written, so an output
    // that overlaps an input takes the materialised form (k_load_canvases copies both canvases before anything is written)
    const bool src = source_fused_call(*p, 1) && (unsigned long long)p->cw * p->ch * sizeof(PX) < 0xfffffff0ULL &&  // 32-bit byte offsets into a channel plane
                     !ranges_overlap(d_out, bytes, d_a, bytes) && !ranges_overlap(d_out, bytes, d_b, bytes);
    return run_pairs<PX>(p, pa, outs, 1, as_stream(stream), src);
}

// The four integers of a stated seam against a canvas of width cw (include/stitch_rig_seams.h): counts within the row, the
// overlap within a, and each sum a possible sum of n distinct columns of 0 .. cw-1.
int seam_check_sums(long long sum_a_x, long long n_a, long long sum_ov_x, long long n_ov, int cw, const char* what, int index) {
    auto possible = [cw](long long sum, long long n) { return sum >= n * (n - 1) / 2 && sum <= n * cw - n * (n + 1) / 2; };
    if (cw < 1 || n_ov < 1 || n_ov > n_a || n_a > cw || sum_ov_x > sum_a_x || !possible(sum_a_x, n_a) || !possible(sum_ov_x, n_ov))
        return fail(STITCH_ERR_ARG,
                    "%s %d: the sums %lld / %lld (a) and %lld / %lld (overlap) are not those of a middle row of %d columns (1 <= n_ov <= n_a <= cw, "
                    "sum_ov_x <= sum_a_x, n(n-1)/2 <= sum <= n*cw - n(n+1)/2)",
                    what, index, sum_a_x, n_a, sum_ov_x, n_ov, cw);
    return STITCH_OK;
}

// the n descriptors of a call as the kernels' argument and the outputs' addresses
template <typename PX>
int pair_args_of(const stitch_pair_desc* d, int n, PairArgs<PX>& pa, OutPtrs<PX>& outs) {
    for (int i = 0; i < n; ++i) {
        if (!d[i].frame || !d[i].mosaic || !d[i].out || d[i].fw <= 0 || d[i].fh <= 0 || d[i].mw <= 0 || d[i].mh <= 0)
            return fail(STITCH_ERR_ARG, "pairs: descriptor %d has a null buffer or a non-positive size", i);
        pa.frame[i] = static_cast<const PX*>(d[i].frame);
        pa.mosaic[i] = static_cast<const PX*>(d[i].mosaic);
        pa.out[i] = static_cast<PX*>(d[i].out);
        outs.p[i] = pa.out[i];
        outs.q[i] = sizeof(PX) == 4 ? static_cast<uint8_t*>(d[i].out_u8) : nullptr;
        if (sizeof(PX) == 1 && d[i].out_u8) return fail(STITCH_ERR_ARG, "pairs: out_u8 is for float frames (descriptor %d)", i);
        std::memcpy(pa.map[i].p, d[i].p, sizeof pa.map[i].p);
        pa.fw[i] = d[i].fw;
        pa.fh[i] = d[i].fh;
        pa.mw[i] = d[i].mw;
        pa.mh[i] = d[i].mh;
        pa.ox[i] = d[i].ox;
        pa.oy[i] = d[i].oy;
        pa.offx[i] = d[i].offx;
        pa.offy[i] = d[i].offy;
    }
    return STITCH_OK;
}

// n independent pairs (n <= plan capacity) through one launch sequence: every kernel covers all n pairs.
// seams (stitch_dev_pairs_seamed_*): n host records whose four integers replace the scan, checked here before anything is enqueued.
template <typename PX>
int dev_pairs(stitch_plan* p, const stitch_pair_desc* d, int n, void* stream, const stitch_seam* seams = nullptr) {
    if (!p || !d) return fail(STITCH_ERR_ARG, "null plan or descriptor array");
    if (n < 1 || n > p->cap) return fail(STITCH_ERR_ARG, "pairs: n=%d outside 1..%d (plan capacity)", n, p->cap);
    if (p->masked) return fail(STITCH_ERR_ARG, "pairs: a masked plan takes stitch_dev_pairs_pathed_* alone (include/stitch_seam_path.h)");
    int dev = -1;
    HIPCHK(hipGetDevice(&dev));
    if (dev != p->device) return fail(STITCH_ERR_ARG, "plan belongs to device %d, current device is %d", p->device, dev);
    PairArgs<PX> pa{};
    OutPtrs<PX> outs{};
    int rc_args = pair_args_of<PX>(d, n, pa, outs);
    if (rc_args) return rc_args;
    // one index plane per distinct key of the call: a pair's owner is the first pair with the same key
    int owner[MAXB];
    for (int i = 0; i < n; ++i) {
        owner[i] = i;
#ifndef STITCH_NO_INDEX_REUSE
        for (int j = 0; j < i && owner[i] == i; ++j)
            if (same_index_key(pa, i, j)) owner[i] = j;
#endif
    }
    set_index_owners(pa, n, owner);
    bool src = source_fused_call(*p, n);
    for (int i = 0; i < n; ++i)  // 32-bit element indices and byte offsets into one channel plane
        src = src && (unsigned long long)d[i].fw * d[i].fh * sizeof(PX) < 0xfffffff0ULL && (unsigned long long)d[i].mw * d[i].mh * sizeof(PX) < 0xfffffff0ULL;
    // source-fused: the frames are read again while the mosaics are written (see dev_blend): no output of the call may overlap an input of it
    const size_t ob = sizeof(PX) * (size_t)3 * p->cw * p->ch;
    for (int i = 0; src && i < n; ++i)
        for (int j = 0; src && j < n; ++j)
            src = !ranges_overlap(d[i].out, ob, d[j].frame, sizeof(PX) * (size_t)3 * d[j].fw * d[j].fh) &&
                  !ranges_overlap(d[i].out, ob, d[j].mosaic, sizeof(PX) * (size_t)3 * d[j].mw * d[j].mh);
    SeamInts given{};
    for (int i = 0; seams && i < n; ++i) {
        const int rc = seam_check_sums(seams[i].sum_a_x, seams[i].n_a, seams[i].sum_ov_x, seams[i].n_ov, p->cw, "pairs_seamed: pair", i);
        if (rc) return rc;
        given.v[i][0] = seams[i].sum_a_x;
        given.v[i][1] = seams[i].n_a;
        given.v[i][2] = seams[i].sum_ov_x;
        given.v[i][3] = seams[i].n_ov;
    }
    return run_pairs<PX>(p, pa, outs, n, as_stream(stream), src, seams ? &given : nullptr);
}

template <typename PX>
int dev_pair(stitch_plan* p, const PX* d_frame, int fw, int fh, const double pm[8], float offx, float offy,
             const PX* d_mosaic, int mw, int mh, int ox, int oy, PX* d_out, void* stream) {
    if (!pm) return fail(STITCH_ERR_ARG, "pair: null map");
    stitch_pair_desc d{};
    d.frame = d_frame;
    d.fw = fw;
    d.fh = fh;
    std::memcpy(d.p, pm, sizeof d.p);
    d.offx = offx;
    d.offy = offy;
    d.mosaic = d_mosaic;
    d.mw = mw;
    d.mh = mh;
    d.ox = ox;
    d.oy = oy;
    d.out = d_out;
    return dev_pairs<PX>(p, &d, 1, stream);
}

void seam_to_public(const SeamDev& d, stitch_seam* o) {
    if (!o) return;
    o->sum_a_x = d.sum_a_x;
    o->n_a = d.n_a;
    o->sum_ov_x = d.sum_ov_x;
    o->n_ov = d.n_ov;
    o->ratio = d.ratio;
    o->ov = d.ov;
    o->branch = d.branch;
    o->start = d.start;
}

// The form a projection of w x h frames runs, decided from the size and from whether the source addresses are 4-byte aligned:
// source rows tiled into LDS (k_project_lds; k_project_lds_t for landscape frames, where the axes swap roles) when the largest
// source box of a tile fits the budget -> the LDS bytes of a launch; otherwise (widths that are not a multiple of 4,
// STITCH_PROJECT1=1) 0: k_project.
template <typename PX>
size_t project_lds_bytes(int w, int h, const ProjParams& pp, bool src_aligned4) {
    constexpr int TW = sizeof(PX) == 1 ? PJ_TW_U8 : PJ_TW_F32, TH = sizeof(PX) == 1 ? PJ_TH_U8 : PJ_TH_F32, CPX = PJ_CHUNK / (int)sizeof(PX);
    size_t lds = 0;
    // (float landscape frames stay with k_project: there a wavefront's taps of a row already share their cache lines -- the
    // source row depends on the output row alone -- and it runs at 0.52 of the roofline, 0.073 ms at 4096 x 3072 against 0.092
    // through LDS; unsigned char: 0.063 -> 0.050)
    const bool tiled = (w % 4) == 0 && (unsigned long long)w * h * 3 * sizeof(PX) < 0xfffffff0ULL && src_aligned4 &&
                       !(pp.flag && sizeof(PX) == 4) && !(Tuning::env_int("STITCH_PROJECT1") > 0);
    if (!tiled) return 0;
    // the box of a tile, as the kernel derives it, over the tiles that can have the largest one (those farthest from the
    // axis and from the middle: the four corner tiles), plus a margin of two rows and two chunks.  `along` = the axis k
    // depends on (columns for portrait frames, rows for landscape ones), `across` the other.
    const int n_al = pp.flag ? h : w, n_ac = pp.flag ? w : h;
    auto k_of = [&](int i) {
        const float d = (float)(i - n_al / 2);
        const double rd = (double)pp.r, dd = (double)d;
        return (float)(rd / std::sqrt(rd * rd + dd * dd));
    };
    auto u_of = [&](int i) { return (float)(i - n_al / 2) / k_of(i) + (float)(n_al / 2); };
    auto v_of = [&](int j, float k) { return (float)(j - n_ac / 2) / k + (float)(n_ac / 2); };
    const int t_al = pp.flag ? TH : TW, t_ac = pp.flag ? TW : TH;  // tile extent along / across
    const int nt_al = (n_al + t_al - 1) / t_al, nt_ac = (n_ac + t_ac - 1) / t_ac;
    for (int bc : {0, nt_ac - 1})
        for (int ba : {0, nt_al - 1}) {
            const int ia = ba * t_al, ib = std::min(ia + t_al, n_al) - 1, ja = bc * t_ac, jb = std::min(ja + t_ac, n_ac) - 1;
            const int mid = n_al / 2, inear = ia <= mid && mid <= ib ? mid : (std::abs(ia - mid) < std::abs(ib - mid) ? ia : ib),
                      ifar = std::abs(ia - mid) > std::abs(ib - mid) ? ia : ib;
            const float kn = k_of(inear), kf = k_of(ifar);
            const float vs[4] = {v_of(ja, kn), v_of(ja, kf), v_of(jb, kn), v_of(jb, kf)};
            const float vmin = std::min(std::min(vs[0], vs[1]), std::min(vs[2], vs[3])), vmax = std::max(std::max(vs[0], vs[1]), std::max(vs[2], vs[3]));
            const long n_across = (long)std::ceil(vmax) - (long)std::floor(vmin) + 1, n_along = (long)std::ceil(u_of(ib)) - (long)std::floor(u_of(ia)) + 1;
            const long rows = (pp.flag ? n_along : n_across) + 2;
            const long cols = ((pp.flag ? n_across : n_along) + 2 * CPX + CPX - 1) / CPX * CPX;
            lds = std::max(lds, pj_box_bytes<PX>((size_t)rows * cols));
        }
    return lds <= 60 * 1024 ? lds : 0;
}

template <typename PX>
int dev_project(const PX* d_src, int w, int h, float fov_deg, PX* d_dst, void* stream, uint8_t* d_gray = nullptr,
                float* d_gray_f32 = nullptr) {
    int rc = need_device();
    if (rc) return rc;
    if (!d_src || !d_dst || w <= 0 || h <= 0) return fail(STITCH_ERR_ARG, "project: null buffer or bad size %dx%d", w, h);
    const ProjParams pp = proj_params(w, h, fov_deg);
    constexpr int TW = sizeof(PX) == 1 ? PJ_TW_U8 : PJ_TW_F32, TH = sizeof(PX) == 1 ? PJ_TH_U8 : PJ_TH_F32;
    const size_t lds = project_lds_bytes<PX>(w, h, pp, (reinterpret_cast<uintptr_t>(d_src) % 4) == 0);
    const bool tiled = lds > 0;
    const dim3 tgrid((w + TW - 1) / TW, (h + TH - 1) / TH);
    if (tiled && !pp.flag)
        k_project_lds<PX, TW, TH><<<tgrid, 256, lds, as_stream(stream)>>>(d_src, d_dst, w, h, pp.r, d_gray, d_gray_f32, (int)lds);
    else if (tiled)
        k_project_lds_t<PX, TW, TH><<<tgrid, 256, lds, as_stream(stream)>>>(d_src, d_dst, w, h, pp.r, d_gray, d_gray_f32, (int)lds);
    else
        k_project<PX><<<grid_xy(w, h), 256, 0, as_stream(stream)>>>(d_src, d_dst, w, h, pp.flag, pp.width, pp.height, pp.r, d_gray,
                                                                    d_gray_f32);
    return launch_check("k_project");
}

template <typename PX>
int dev_warp(const PX* d_src, int sw, int sh, const double pm[8], float offx, float offy, PX* d_canvas, int cw, int ch,
             void* stream) {
    int rc = need_device();
    if (rc) return rc;
    if (!d_src || !d_canvas || !pm || sw <= 0 || sh <= 0 || cw <= 0 || ch <= 0) return fail(STITCH_ERR_ARG, "warp: bad argument");
    MapP m;
    std::memcpy(m.p, pm, sizeof m.p);
    k_warp<PX><<<grid_xy(cw, ch), 256, 0, as_stream(stream)>>>(d_src, sw, sh, m, offx, offy, d_canvas, cw, ch);
    return launch_check("k_warp");
}

template <typename PX>
int dev_move(const PX* d_src, int sw, int sh, int ox, int oy, PX* d_canvas, int cw, int ch, void* stream) {
    int rc = need_device();
    if (rc) return rc;
    if (!d_src || !d_canvas || sw <= 0 || sh <= 0 || cw <= 0 || ch <= 0) return fail(STITCH_ERR_ARG, "move: bad argument");
    k_move<PX><<<grid_xy(cw, ch), 256, 0, as_stream(stream)>>>(d_src, sw, sh, ox, oy, d_canvas, cw, ch);
    return launch_check("k_move");
}

// RAII device buffer for the host-pointer entry points.  Blocks come from the device's stream-ordered memory pool with its
// release threshold lifted (once per device), so that a caller that stitches frame after frame -- the reference's matching()
// loop through the C++ adaptor -- re-uses the same device memory instead of paying hipMalloc + hipFree (both synchronise
// the device) on every call; stitch_trim() hands the pool's memory back.
void keep_pool_memory() {
    static std::mutex mu;
    static bool done[64] = {false};
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return;
    std::lock_guard<std::mutex> g(mu);
    if (done[dev]) return;
    hipMemPool_t pool;
    if (hipDeviceGetDefaultMemPool(&pool, dev) == hipSuccess) {
        uint64_t keep = UINT64_MAX;
        (void)hipMemPoolSetAttribute(pool, hipMemPoolAttrReleaseThreshold, &keep);
    }
    (void)hipGetLastError();
    done[dev] = true;
}
struct DevBuf {
    void* p = nullptr;
    ~DevBuf() {
        if (p) (void)hipFreeAsync(p, nullptr);
    }
    int alloc(size_t bytes) {
        keep_pool_memory();
        HIPCHK(hipMallocAsync(&p, bytes, nullptr));
        return STITCH_OK;
    }
    template <typename T>
    T* as() {
        return static_cast<T*>(p);
    }
};

// Host <-> device copies of the host-pointer entry points.  The caller's buffers are ordinary pageable memory (CImg's
// new[]), which the runtime moves at about 10 GB/s through one staging thread -- 70 ms for the 704 MB of a 4096 x 4096
// float pair, fifty times the blend itself.  Large copies are therefore cut into chunks and spread over a few persistent
// worker threads, each with its own pair of pinned staging buffers and its own stream: the workers' memcpy()s run side by
// side and overlap the DMA of earlier chunks.  Small copies go straight through hipMemcpy.
class HostCopier {
  public:
    static HostCopier& get() {
        static HostCopier* c = new HostCopier();  // never destroyed: its threads are parked on its condition variable until the process ends
        return *c;
    }
    // returns a HIP error code (0 = ok); both calls return when the data has arrived
    int h2d(void* dev, const void* host, size_t bytes) { return run(static_cast<char*>(dev), const_cast<char*>(static_cast<const char*>(host)), bytes, true); }
    int d2h(void* host, const void* dev, size_t bytes) { return run(const_cast<char*>(static_cast<const char*>(dev)), static_cast<char*>(host), bytes, false); }
    void release() {  // stitch_trim(): pinned buffers are given back, the threads stay parked
        std::lock_guard<std::mutex> g(call_mu_);
        for (auto& w : workers_)
            for (auto& b : w->buf)
                if (b) {
                    (void)hipHostFree(b);
                    b = nullptr;
                }
    }

  private:
    static constexpr size_t CHUNK = 8u << 20, DIRECT_BELOW = 4u << 20;
    struct Worker {
        std::thread th;
        hipStream_t stream = nullptr;
        hipEvent_t ev[2] = {nullptr, nullptr};
        char* buf[2] = {nullptr, nullptr};
    };
    std::vector<Worker*> workers_;
    std::mutex call_mu_, mu_;  // one copy at a time; job hand-off
    std::condition_variable cv_, done_cv_;
    // the current job
    char *dev_ = nullptr, *host_ = nullptr;
    size_t bytes_ = 0;
    bool to_dev_ = true;
    int device_ = 0, generation_ = 0, pending_ = 0;
    std::atomic<size_t> next_{0};
    std::atomic<int> err_{0};

    HostCopier() {
        int n = 4;
        if (const char* e = std::getenv("STITCH_COPY_THREADS")) n = std::max(0, std::min(16, atoi(e)));
        for (int i = 0; i < n; ++i) {
            Worker* w = new Worker();
            workers_.push_back(w);
            w->th = std::thread([this, w] { loop(w); });
            w->th.detach();  // parked on the condition variable for the life of the process
        }
    }
    int run(char* dev, char* host, size_t bytes, bool to_dev) {
        if (bytes < DIRECT_BELOW || workers_.empty())
            return (int)(to_dev ? hipMemcpy(dev, host, bytes, hipMemcpyHostToDevice) : hipMemcpy(host, dev, bytes, hipMemcpyDeviceToHost));
        std::lock_guard<std::mutex> call(call_mu_);
        hipError_t e = hipStreamSynchronize(nullptr);  // the kernels that produced / will consume the device buffer run on the null stream
        if (e != hipSuccess) return (int)e;
        if ((e = hipGetDevice(&device_)) != hipSuccess) return (int)e;
        {
            std::lock_guard<std::mutex> g(mu_);
            dev_ = dev, host_ = host, bytes_ = bytes, to_dev_ = to_dev;
            next_ = 0;
            err_ = 0;
            pending_ = (int)workers_.size();
            ++generation_;
        }
        cv_.notify_all();
        std::unique_lock<std::mutex> g(mu_);
        done_cv_.wait(g, [this] { return pending_ == 0; });
        return err_.load();
    }
    void loop(Worker* w) {
        int seen = 0;
        for (;;) {
            {
                std::unique_lock<std::mutex> g(mu_);
                cv_.wait(g, [&] { return generation_ != seen; });
                seen = generation_;
            }
            work(w);
            {
                std::lock_guard<std::mutex> g(mu_);
                --pending_;
            }
            done_cv_.notify_all();
        }
    }
    void fail(hipError_t e) {
        int z = 0;
        err_.compare_exchange_strong(z, (int)e);
    }
    void work(Worker* w) {
        hipError_t e = hipSetDevice(device_);
        if (e == hipSuccess && !w->stream) e = hipStreamCreateWithFlags(&w->stream, hipStreamNonBlocking);
        for (int i = 0; i < 2 && e == hipSuccess; ++i) {
            if (!w->ev[i]) e = hipEventCreateWithFlags(&w->ev[i], hipEventDisableTiming);
            if (e == hipSuccess && !w->buf[i]) e = hipHostMalloc((void**)&w->buf[i], CHUNK);
        }
        if (e != hipSuccess) return fail(e);
        bool busy[2] = {false, false};
        size_t off_of[2] = {0, 0}, len_of[2] = {0, 0};
        int slot = 0;
        auto drain = [&](int s_) {  // the DMA that last used slot s_ has finished; D2H: its bytes go on to the caller's buffer
            if (!busy[s_]) return;
            if ((e = hipEventSynchronize(w->ev[s_])) != hipSuccess) return fail(e);
            if (!to_dev_) std::memcpy(host_ + off_of[s_], w->buf[s_], len_of[s_]);
            busy[s_] = false;
        };
        for (;;) {
            const size_t off = next_.fetch_add(CHUNK);
            if (off >= bytes_ || err_.load()) break;
            const size_t len = std::min(CHUNK, bytes_ - off);
            drain(slot);
            if (to_dev_) {
                std::memcpy(w->buf[slot], host_ + off, len);
                e = hipMemcpyAsync(dev_ + off, w->buf[slot], len, hipMemcpyHostToDevice, w->stream);
            } else
                e = hipMemcpyAsync(w->buf[slot], dev_ + off, len, hipMemcpyDeviceToHost, w->stream);
            if (e == hipSuccess) e = hipEventRecord(w->ev[slot], w->stream);
            if (e != hipSuccess) return fail(e);
            busy[slot] = true, off_of[slot] = off, len_of[slot] = len;
            slot ^= 1;
        }
        drain(slot);
        drain(slot ^ 1);
    }
};
#define H2D(dst, src, bytes)                                                                                                   \
    do {                                                                                                                       \
        int e_ = HostCopier::get().h2d(dst, src, bytes);                                                                       \
        if (e_) return fail(STITCH_ERR_HIP, "host-to-device copy of %zu bytes failed: %s", (size_t)(bytes), hipGetErrorString((hipError_t)e_)); \
    } while (0)
#define D2H(dst, src, bytes)                                                                                                   \
    do {                                                                                                                       \
        int e_ = HostCopier::get().d2h(dst, src, bytes);                                                                       \
        if (e_) return fail(STITCH_ERR_HIP, "device-to-host copy of %zu bytes failed: %s", (size_t)(bytes), hipGetErrorString((hipError_t)e_)); \
    } while (0)

template <typename PX>
int host_project(const PX* src, int w, int h, float fov_deg, PX* dst) {
    int rc = need_device();
    if (rc) return rc;
    if (!src || !dst || w <= 0 || h <= 0) return fail(STITCH_ERR_ARG, "project: null buffer or bad size %dx%d", w, h);
    const size_t bytes = sizeof(PX) * (size_t)w * h * 3;
    DevBuf s, d;
    if ((rc = s.alloc(bytes)) || (rc = d.alloc(bytes))) return rc;
    H2D(s.p, src, bytes);
    if ((rc = dev_project<PX>(s.as<PX>(), w, h, fov_deg, d.as<PX>(), nullptr))) return rc;
    D2H(dst, d.p, bytes);
    return STITCH_OK;
}

template <typename PX>
int host_warp(const PX* src, int sw, int sh, const double pm[8], float offx, float offy, PX* canvas, int cw, int ch) {
    int rc = need_device();
    if (rc) return rc;
    if (!src || !canvas || !pm || sw <= 0 || sh <= 0 || cw <= 0 || ch <= 0) return fail(STITCH_ERR_ARG, "warp: bad argument");
    const size_t sb = sizeof(PX) * (size_t)sw * sh * 3, cb = sizeof(PX) * (size_t)cw * ch * 3;
    DevBuf s, c;
    if ((rc = s.alloc(sb)) || (rc = c.alloc(cb))) return rc;
    H2D(s.p, src, sb);
    H2D(c.p, canvas, cb);
    if ((rc = dev_warp<PX>(s.as<PX>(), sw, sh, pm, offx, offy, c.as<PX>(), cw, ch, nullptr))) return rc;
    D2H(canvas, c.p, cb);
    return STITCH_OK;
}

template <typename PX>
int host_move(const PX* src, int sw, int sh, int ox, int oy, PX* canvas, int cw, int ch) {
    int rc = need_device();
    if (rc) return rc;
    if (!src || !canvas || sw <= 0 || sh <= 0 || cw <= 0 || ch <= 0) return fail(STITCH_ERR_ARG, "move: bad argument");
    const size_t sb = sizeof(PX) * (size_t)sw * sh * 3, cb = sizeof(PX) * (size_t)cw * ch * 3;
    DevBuf s, c;
    if ((rc = s.alloc(sb)) || (rc = c.alloc(cb))) return rc;
    H2D(s.p, src, sb);
    H2D(c.p, canvas, cb);
    if ((rc = dev_move<PX>(s.as<PX>(), sw, sh, ox, oy, c.as<PX>(), cw, ch, nullptr))) return rc;
    D2H(canvas, c.p, cb);
    return STITCH_OK;
}

// Workspaces of the host-pointer entry points are kept between calls: creating one costs a device allocation of the whole
// pyramid (1.9 GB at 6144 x 4096), its clearing, the resize tables and two pinned allocations -- more than the blend itself
// below about 2000 x 2000.  A small LRU keyed by (device, canvas, options) holds idle plans; a call takes one out (so that
// concurrent callers never share a workspace) and puts it back when it is done.  STITCH_PLAN_CACHE=<n> sets the number of
// idle plans kept (default 8, 0 = none); stitch_trim() destroys them.
struct PlanKey {
    int dev, cw, ch;
    stitch_blend_opts o;
    Tuning t;  // the tuning switches the plan was built under (Tuning): a changed environment never meets a stale plan
    bool operator==(const PlanKey& k) const {
        return dev == k.dev && cw == k.cw && ch == k.ch && o.sigma == k.o.sigma && o.blur_kind == k.o.blur_kind && o.level_rule == k.o.level_rule &&
               o.seam_rule == k.o.seam_rule && t == k.t;
    }
};
std::mutex g_plan_mu;
std::list<std::pair<PlanKey, stitch_plan*>> g_idle_plans;  // most recently used first
size_t plan_cache_limit() {
    static const size_t n = [] {
        const char* e = std::getenv("STITCH_PLAN_CACHE");
        return e ? (size_t)std::max(0, atoi(e)) : (size_t)8;
    }();
    return n;
}
struct PlanLease {
    stitch_plan* p = nullptr;
    PlanKey key{};
    bool healthy = false;  // the leased call got as far as a status the plan survives (finish()); otherwise the plan is destroyed
    int acquire(int cw, int ch, const stitch_blend_opts* opts) {
        stitch_blend_opts o;
        stitch_blend_opts_default(&o);
        if (opts) o = *opts;
        int dev = 0;
        HIPCHK(hipGetDevice(&dev));
        key = PlanKey{dev, cw, ch, o, Tuning::from_env()};
        {
            std::lock_guard<std::mutex> g(g_plan_mu);
            for (auto it = g_idle_plans.begin(); it != g_idle_plans.end(); ++it)
                if (it->first == key) {
                    p = it->second;
                    g_idle_plans.erase(it);
                    return STITCH_OK;
                }
        }
        return stitch_plan_create(cw, ch, opts, &p);
    }
    // outcome of the leased call's stitch_plan_status: a failed seam scan leaves the workspace as good as before
    int finish(int rc) {
        healthy = rc == STITCH_OK || rc == STITCH_ERR_EMPTY_MIDROW || rc == STITCH_ERR_ZERO_OVERLAP;
        return rc;
    }
    ~PlanLease() {
        if (!p) return;
        // wait for the plan's last call and acknowledge its faults BEFORE the cache mutex is taken: other threads' host-pointer
        // calls only ever block on the list operations below, never on this plan's GPU work
        const bool keep = healthy && plan_cache_limit() > 0 && stitch_plan_clear_fault(p) == STITCH_OK;
        std::vector<stitch_plan*> evict;
        if (keep) {
            std::lock_guard<std::mutex> g(g_plan_mu);
            g_idle_plans.emplace_front(key, p);
            p = nullptr;
            while (g_idle_plans.size() > plan_cache_limit()) {
                evict.push_back(g_idle_plans.back().second);
                g_idle_plans.pop_back();
            }
        }
        if (p) stitch_plan_destroy(p);  // a call that failed part-way (or a timed-out hand-off) never goes back into the cache
        for (auto* e : evict) stitch_plan_destroy(e);
    }
};

template <typename PX>
int host_blend(const PX* a, const PX* b, int w, int h, const stitch_blend_opts* opts, PX* out, stitch_seam* seam_out) {
    int rc = need_device();
    if (rc) return rc;
    if (!a || !b || !out || w <= 0 || h <= 0) return fail(STITCH_ERR_ARG, "blend: null buffer or bad size %dx%d", w, h);
    PlanLease pg;
    if ((rc = pg.acquire(w, h, opts))) return rc;
    const size_t bytes = sizeof(PX) * (size_t)w * h * 3;
    DevBuf da, db, dout;
    if ((rc = da.alloc(bytes)) || (rc = db.alloc(bytes)) || (rc = dout.alloc(bytes))) return rc;
    H2D(da.p, a, bytes);
    H2D(db.p, b, bytes);
    if ((rc = dev_blend<PX>(pg.p, da.as<PX>(), db.as<PX>(), dout.as<PX>(), nullptr))) return rc;
    if ((rc = pg.finish(stitch_plan_status(pg.p, seam_out)))) return rc;
    D2H(out, dout.p, bytes);
    return STITCH_OK;
}

template <typename PX>
int host_pair(const PX* frame, int fw, int fh, const double pm[8], float offx, float offy, const PX* mosaic, int mw, int mh,
              int ox, int oy, int cw, int ch, const stitch_blend_opts* opts, PX* out, stitch_seam* seam_out) {
    int rc = need_device();
    if (rc) return rc;
    if (!frame || !mosaic || !out || !pm || fw <= 0 || fh <= 0 || mw <= 0 || mh <= 0 || cw <= 0 || ch <= 0)
        return fail(STITCH_ERR_ARG, "pair: bad argument");
    PlanLease pg;
    if ((rc = pg.acquire(cw, ch, opts))) return rc;
    const size_t fb = sizeof(PX) * (size_t)fw * fh * 3, mb = sizeof(PX) * (size_t)mw * mh * 3,
                 ob = sizeof(PX) * (size_t)cw * ch * 3;
    DevBuf df, dm, dout;
    if ((rc = df.alloc(fb)) || (rc = dm.alloc(mb)) || (rc = dout.alloc(ob))) return rc;
    H2D(df.p, frame, fb);
    H2D(dm.p, mosaic, mb);
    if ((rc = dev_pair<PX>(pg.p, df.as<PX>(), fw, fh, pm, offx, offy, dm.as<PX>(), mw, mh, ox, oy, dout.as<PX>(), nullptr)))
        return rc;
    if ((rc = pg.finish(stitch_plan_status(pg.p, seam_out)))) return rc;
    D2H(out, dout.p, ob);
    return STITCH_OK;
}

// planes of n bytes that can be moved as 32-bit words (the four-pixels-per-work-item kernels); STITCH_BYTE_KERNELS=1: never
bool words_ok(const void* base, size_t n) {
    return (n % 4) == 0 && (reinterpret_cast<uintptr_t>(base) % 4) == 0 && !(Tuning::env_int("STITCH_BYTE_KERNELS") > 0);
}

// The mix's divides by `den` as multiplications by its reciprocal plus one fma correction -- only where that is PROVEN equal for
// every operand the kernels can meet (k_equalize.inc, MixK): Y and Yeq are floats (float)(t/1000) clamped, t = 0 .. 323850.
// Both quotients of ImageProcess.cpp:261, a = Y*num and a = Yeq, are compared in both forms for all of them (~2 ms, once per
// (num, den); the last few verdicts are kept).  STITCH_NO_FASTDIV=1: always divide.
MixK mix_params(double num, double den) {
    MixK k{num, den, 0.0};
    static const bool off = Tuning::env_int("STITCH_NO_FASTDIV") > 0;  // read once per process
    if (off || !(den == den) || den == 0.0 || std::isinf(den) || !(num == num) || std::isinf(num)) return k;
    struct Verdict {
        double num, den;
        bool ok;
    };
    static std::mutex mu;
    static std::vector<Verdict> seen;
    {
        std::lock_guard<std::mutex> g(mu);
        for (const Verdict& v : seen)
            if (std::memcmp(&v.num, &num, sizeof num) == 0 && std::memcmp(&v.den, &den, sizeof den) == 0) {
                if (v.ok) k.rden = 1.0 / den;
                return k;
            }
    }
    const double rden = 1.0 / den;
    auto quot = [&](double a) {
        const double q = a * rden;
        return std::fma(std::fma(-q, den, a), rden, q);
    };
    bool ok = std::isfinite(rden) && rden != 0.0;
    for (unsigned t = 0; ok && t <= 323850u; ++t) {
        float y = (float)((double)t * 0.001);
        y = y < 256.f ? y : 255.f;
        const double a1 = (double)y * num, a2 = (double)y;
        const double d1 = a1 / den, d2 = a2 / den, f1 = quot(a1), f2 = quot(a2);
        ok = std::memcmp(&d1, &f1, sizeof d1) == 0 && std::memcmp(&d2, &f2, sizeof d2) == 0;
    }
    {
        std::lock_guard<std::mutex> g(mu);
        if (seen.size() >= 16) seen.erase(seen.begin());
        seen.push_back(Verdict{num, den, ok});
    }
    if (ok) k.rden = rden;
    return k;
}

int eq_grid(size_t n) {
    size_t g = (n + 255) / 256;
    return (int)(g < 2048 ? (g ? g : 1) : 2048);  // memory-bound: cap the grid and stride (guide 6, guideline 11)
}

// E1-E3 (+ optional fused M1).  Scratch (256-bin histogram + LUT) comes from the stream-ordered allocator, so
// concurrent calls on different streams do not share state.
int dev_equalize_impl(uint8_t* d_img, int w, int h, int32_t* d_hist_out, bool fuse_mix, double num, double den, void* stream) {
    int rc = need_device();
    if (rc) return rc;
    if (!d_img || w <= 0 || h <= 0) return fail(STITCH_ERR_ARG, "equalize: null buffer or bad size %dx%d", w, h);
    if ((long long)w * h > 0x7fffffffLL) return fail(STITCH_ERR_ARG, "equalize: w*h overflows int (the reference's int product)");
    hipStream_t s = as_stream(stream);
    int32_t* scratch = nullptr;
    HIPCHK(hipMallocAsync((void**)&scratch, sizeof(int32_t) * 512, s));
    int32_t *hist = scratch, *lut = scratch + 256;
    HIPCHK(hipMemsetAsync(hist, 0, sizeof(int32_t) * 256, s));
    const size_t n = (size_t)w * h;
    const bool v4 = words_ok(d_img, n);
    if (v4)
        // every workgroup ends with 256 global atomics on the same 256 words: 512 workgroups (measured at 25 MPix: 2048 -> 50 us,
        // 1024 -> 31, 512 -> 29, 256 -> 38)
        k_hist4<<<std::min(eq_grid(n / 4), 512), HIST_WAVES * 64, 0, s>>>(d_img, n, hist);
    else
        k_hist<<<eq_grid(n), HIST_WAVES * 64, 0, s>>>(d_img, n, hist);
    k_lut<<<1, 256, 0, s>>>(hist, w, h, lut);
    if (fuse_mix) {
        if (v4)
            k_equalize_apply4<true><<<eq_grid(n / 4), 256, 0, s>>>(d_img, n, lut, mix_params(num, den));
        else
            k_equalize_apply<true><<<eq_grid(n), 256, 0, s>>>(d_img, n, lut, mix_params(num, den));
    } else {
        if (v4)
            k_equalize_apply4<false><<<eq_grid(n / 4), 256, 0, s>>>(d_img, n, lut, MixK{0.0, 1.0, 0.0});
        else
            k_equalize_apply<false><<<eq_grid(n), 256, 0, s>>>(d_img, n, lut, MixK{0.0, 1.0, 0.0});
    }
    if (d_hist_out) HIPCHK(hipMemcpyAsync(d_hist_out, hist, sizeof(int32_t) * 256, hipMemcpyDeviceToDevice, s));
    HIPCHK(hipFreeAsync(scratch, s));
    return launch_check("equalize");
}

template <typename PX>
int dev_step(const PX* d_frame, int fw, int fh, const double p_fwd[8], const double p_bwd[8], const PX* d_mosaic, int mw, int mh,
                    const stitch_blend_opts* opts, PX* d_out, size_t out_capacity, stitch_step_geom* geom_out, stitch_seam* seam_out,
                    void* stream) {
    int rc = need_device();
    if (rc) return rc;
    if (!d_frame || !d_mosaic || !d_out || !p_fwd || !p_bwd) return fail(STITCH_ERR_ARG, "step: null argument");
    stitch_step_geom g;
    if ((rc = stitch_step_geometry(fw, fh, p_fwd, mw, mh, &g))) return rc;
    if (geom_out) *geom_out = g;
    if (out_capacity < (size_t)3 * g.cw * g.ch)
        return fail(STITCH_ERR_ARG, "step: the new mosaic is %d x %d x 3 = %zu samples, the output buffer holds %zu", g.cw, g.ch,
                    (size_t)3 * g.cw * g.ch, out_capacity);
    PlanLease lease;  // idle workspace of this canvas size, or a new one; goes back to the cache when the step is done
    if ((rc = lease.acquire(g.cw, g.ch, opts))) return rc;
    if ((rc = dev_pair<PX>(lease.p, d_frame, fw, fh, p_bwd, g.min_x, g.min_y, d_mosaic, mw, mh, g.ox, g.oy, d_out, stream))) return rc;
    return lease.finish(stitch_plan_status(lease.p, seam_out));
}

}  // namespace

// =========================================== C ABI ==========================================================
extern "C" {

int stitch_abi_version(void) { return STITCH_ABI_VERSION; }
int stitch_init(void) {
    if (std::getenv("GPU_MAX_HW_QUEUES")) return 0;
    return setenv("GPU_MAX_HW_QUEUES", "8", /*overwrite=*/0) == 0 ? 1 : 0;
}
const char* stitch_last_error(void) { return g_err.c_str(); }

int stitch_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) {
        (void)hipGetLastError();
        return 0;
    }
    return n;
}

int stitch_set_device(int ordinal) {
    int rc = need_device();
    if (rc) return rc;
    HIPCHK(hipSetDevice(ordinal));
    return STITCH_OK;
}

void stitch_trim(void) {
    std::vector<stitch_plan*> all;
    {
        std::lock_guard<std::mutex> g(g_plan_mu);
        for (auto& e : g_idle_plans) all.push_back(e.second);
        g_idle_plans.clear();
    }
    for (auto* p : all) stitch_plan_destroy(p);
    HostCopier::get().release();
    int dev = 0;
    hipMemPool_t pool;
    if (hipGetDevice(&dev) == hipSuccess && hipDeviceSynchronize() == hipSuccess && hipDeviceGetDefaultMemPool(&pool, dev) == hipSuccess)
        (void)hipMemPoolTrimTo(pool, 0);
    (void)hipGetLastError();
}

int stitch_plan_cache_query(int cw, int ch, const stitch_blend_opts* opts, int* fused_sweep_levels) {
    stitch_blend_opts o;
    stitch_blend_opts_default(&o);
    if (opts) o = *opts;
    int dev = 0;
    HIPCHK(hipGetDevice(&dev));
    const PlanKey key{dev, cw, ch, o, Tuning::from_env()};
    int n = 0;
    std::lock_guard<std::mutex> g(g_plan_mu);
    for (auto& e : g_idle_plans)
        if (e.first == key) {
            if (n == 0 && fused_sweep_levels) *fused_sweep_levels = e.second->wf_levels;
            ++n;
        }
    return n;
}

void stitch_blend_opts_default(stitch_blend_opts* o) {
    if (!o) return;
    o->sigma = 2.0f;
    o->blur_kind = 0;
    o->level_rule = 0;
    o->seam_rule = 0;
}

int stitch_pyramid_levels(int w, int h, int level_rule, int* level_w, int* level_h) {
    return pyramid_levels(w, h, level_rule, level_w, level_h);
}

int stitch_project_u8(const uint8_t* src, int w, int h, float fov_deg, uint8_t* dst) { return host_project(src, w, h, fov_deg, dst); }
int stitch_project_f32(const float* src, int w, int h, float fov_deg, float* dst) { return host_project(src, w, h, fov_deg, dst); }
int stitch_warp_u8(const uint8_t* src, int sw, int sh, const double p[8], float offx, float offy, uint8_t* canvas, int cw, int ch) {
    return host_warp(src, sw, sh, p, offx, offy, canvas, cw, ch);
}
int stitch_warp_f32(const float* src, int sw, int sh, const double p[8], float offx, float offy, float* canvas, int cw, int ch) {
    return host_warp(src, sw, sh, p, offx, offy, canvas, cw, ch);
}
int stitch_move_u8(const uint8_t* src, int sw, int sh, int ox, int oy, uint8_t* canvas, int cw, int ch) {
    return host_move(src, sw, sh, ox, oy, canvas, cw, ch);
}
int stitch_move_f32(const float* src, int sw, int sh, int ox, int oy, float* canvas, int cw, int ch) {
    return host_move(src, sw, sh, ox, oy, canvas, cw, ch);
}
int stitch_blend_u8(const uint8_t* a, const uint8_t* b, int w, int h, const stitch_blend_opts* opts, uint8_t* out,
                    stitch_seam* seam_out) {
    return host_blend(a, b, w, h, opts, out, seam_out);
}
int stitch_blend_f32(const float* a, const float* b, int w, int h, const stitch_blend_opts* opts, float* out, stitch_seam* seam_out) {
    return host_blend(a, b, w, h, opts, out, seam_out);
}
int stitch_pair_u8(const uint8_t* frame, int fw, int fh, const double p[8], float offx, float offy, const uint8_t* mosaic, int mw,
                   int mh, int ox, int oy, int cw, int ch, const stitch_blend_opts* opts, uint8_t* out, stitch_seam* seam_out) {
    return host_pair(frame, fw, fh, p, offx, offy, mosaic, mw, mh, ox, oy, cw, ch, opts, out, seam_out);
}
int stitch_pair_f32(const float* frame, int fw, int fh, const double p[8], float offx, float offy, const float* mosaic, int mw,
                    int mh, int ox, int oy, int cw, int ch, const stitch_blend_opts* opts, float* out, stitch_seam* seam_out) {
    return host_pair(frame, fw, fh, p, offx, offy, mosaic, mw, mh, ox, oy, cw, ch, opts, out, seam_out);
}

int stitch_equalize_u8(uint8_t* img, int w, int h, int32_t hist_out[256]) {
    int rc = need_device();
    if (rc) return rc;
    if (!img || w <= 0 || h <= 0) return fail(STITCH_ERR_ARG, "equalize: null buffer or bad size %dx%d", w, h);
    const size_t bytes = (size_t)w * h * 3;
    DevBuf d, dh;
    if ((rc = d.alloc(bytes)) || (rc = dh.alloc(sizeof(int32_t) * 256))) return rc;
    H2D(d.p, img, bytes);
    if ((rc = dev_equalize_impl(d.as<uint8_t>(), w, h, dh.as<int32_t>(), false, 0, 1, nullptr))) return rc;
    D2H(img, d.p, bytes);
    if (hist_out) D2H(hist_out, dh.p, sizeof(int32_t) * 256);
    return STITCH_OK;
}

int stitch_lummix_u8(uint8_t* result, const uint8_t* equalized, int w, int h, double num, double den) {
    int rc = need_device();
    if (rc) return rc;
    if (!result || !equalized || w <= 0 || h <= 0) return fail(STITCH_ERR_ARG, "lummix: null buffer or bad size %dx%d", w, h);
    const size_t bytes = (size_t)w * h * 3;
    DevBuf r, e;
    if ((rc = r.alloc(bytes)) || (rc = e.alloc(bytes))) return rc;
    H2D(r.p, result, bytes);
    H2D(e.p, equalized, bytes);
    if ((rc = stitch_dev_lummix_u8(r.as<uint8_t>(), e.as<uint8_t>(), w, h, num, den, nullptr))) return rc;
    D2H(result, r.p, bytes);
    return STITCH_OK;
}

int stitch_finish_u8(uint8_t* result, int w, int h, double num, double den, int32_t hist_out[256]) {
    int rc = need_device();
    if (rc) return rc;
    if (!result || w <= 0 || h <= 0) return fail(STITCH_ERR_ARG, "finish: null buffer or bad size %dx%d", w, h);
    const size_t bytes = (size_t)w * h * 3;
    DevBuf d, dh;
    if ((rc = d.alloc(bytes)) || (rc = dh.alloc(sizeof(int32_t) * 256))) return rc;
    H2D(d.p, result, bytes);
    if ((rc = dev_equalize_impl(d.as<uint8_t>(), w, h, dh.as<int32_t>(), true, num, den, nullptr))) return rc;
    D2H(result, d.p, bytes);
    if (hist_out) D2H(hist_out, dh.p, sizeof(int32_t) * 256);
    return STITCH_OK;
}

int stitch_dev_project_u8(const uint8_t* d_src, int w, int h, float fov_deg, uint8_t* d_dst, void* stream) {
    return dev_project(d_src, w, h, fov_deg, d_dst, stream);
}
int stitch_dev_project_f32(const float* d_src, int w, int h, float fov_deg, float* d_dst, void* stream) {
    return dev_project(d_src, w, h, fov_deg, d_dst, stream);
}
int stitch_dev_warp_u8(const uint8_t* d_src, int sw, int sh, const double p[8], float offx, float offy, uint8_t* d_canvas, int cw,
                       int ch, void* stream) {
    return dev_warp(d_src, sw, sh, p, offx, offy, d_canvas, cw, ch, stream);
}
int stitch_dev_warp_f32(const float* d_src, int sw, int sh, const double p[8], float offx, float offy, float* d_canvas, int cw,
                        int ch, void* stream) {
    return dev_warp(d_src, sw, sh, p, offx, offy, d_canvas, cw, ch, stream);
}
int stitch_dev_move_u8(const uint8_t* d_src, int sw, int sh, int ox, int oy, uint8_t* d_canvas, int cw, int ch, void* stream) {
    return dev_move(d_src, sw, sh, ox, oy, d_canvas, cw, ch, stream);
}
int stitch_dev_move_f32(const float* d_src, int sw, int sh, int ox, int oy, float* d_canvas, int cw, int ch, void* stream) {
    return dev_move(d_src, sw, sh, ox, oy, d_canvas, cw, ch, stream);
}

static int plan_create(int cw, int ch, const stitch_blend_opts* opts, int max_pairs, bool planes_in, stitch_plan** plan_out, bool masked = false);
int stitch_plan_create(int cw, int ch, const stitch_blend_opts* opts, stitch_plan** plan_out) {
    return stitch_plan_create_batched(cw, ch, opts, 1, plan_out);
}

int stitch_plan_create_batched(int cw, int ch, const stitch_blend_opts* opts, int max_pairs, stitch_plan** plan_out) {
    return plan_create(cw, ch, opts, max_pairs, false, plan_out);
}

// Fill the shape (plan_shape, stitch_call_form.h), carve one arena for it, upload the resize tables.  planes_in: the coarse levels of a
// band-split pair (stitch_band_create); masked: include/stitch_seam_path.h.
static int plan_create(int cw, int ch, const stitch_blend_opts* opts, int max_pairs, bool planes_in, stitch_plan** plan_out, bool masked) {
    if (!plan_out) return fail(STITCH_ERR_ARG, "plan_create: null plan_out");
    if (max_pairs < 1 || max_pairs > MAXB) return fail(STITCH_ERR_ARG, "plan_create: max_pairs must be 1..%d", MAXB);
    *plan_out = nullptr;
    int rc = need_device();
    if (rc) return rc;
    stitch_blend_opts o;
    stitch_blend_opts_default(&o);
    if (opts) o = *opts;
    if (o.blur_kind < 0 || o.blur_kind > 1 || o.level_rule < 0 || o.level_rule > 1 || o.seam_rule < 0 || o.seam_rule > 1 ||
        !(o.sigma >= 0))
        return fail(STITCH_ERR_ARG, "plan_create: bad blend options");
    const int L = pyramid_levels(cw, ch, o.level_rule, nullptr, nullptr);
    if (L < 0) return L;

    stitch_plan* p = new stitch_plan();
    const Tuning tn = Tuning::from_env();
    StampRequest stamps;
    stamps.xy = std::getenv("STITCH_XBYM_STAMP") != nullptr;
    stamps.co = std::getenv("STITCH_COARSE_STAMP") != nullptr;
    if (std::getenv("STITCH_D7_STAMP")) stamps.d7_level = atoi(std::getenv("STITCH_D7_STAMP"));
    plan_shape(*p, cw, ch, o, max_pairs, tn, stamps, planes_in, masked);
    const size_t B = (size_t)max_pairs;
    p->vvk = make_vvk(o.sigma);
    p->drk = make_drk(o.sigma);
    if (hipGetDevice(&p->device) != hipSuccess) {
        delete p;
        return fail(STITCH_ERR_HIP, "hipGetDevice failed");
    }
    // carve one arena
    size_t off = 0;
    auto take = [&](size_t bytes) {
        const size_t o2 = off;
        off += align256(bytes);
        return o2;
    };
    size_t g_off[32], e_off[32], ix_off[32], ax_off[32], iy_off[32], ay_off[32];
    for (int l = 0; l < L; ++l) {
        const Level& v = p->lv[l];
        g_off[l] = take(sizeof(float) * (v.ps * 7 * B + (size_t)v.pitch * 64));
        e_off[l] = l >= 1 || L == 1 ? take(sizeof(float) * v.ps * 3 * B) : 0;
        if (l + 1 < L) {
            ix_off[l] = take(sizeof(int32_t) * v.w);
            ax_off[l] = take(sizeof(double) * v.w);
            iy_off[l] = take(sizeof(int32_t) * v.h);
            ay_off[l] = take(sizeof(double) * v.h);
        }
    }
    const Level& v0 = p->lv[0];
    const size_t t_bytes = sizeof(float) * (v0.ps * 7 * B + (size_t)v0.pitch * 64);
    const size_t t_off = take(t_bytes);
    const size_t t2_off = o.blur_kind == 1 ? take(t_bytes) : 0;
    const int NC0 = tiles(v0.w), NR0 = tiles(v0.h);
    // hand-off granules, sized for level 0
    const size_t yg_off = p->has_wf ? take(sizeof(u64) * B * 7 * NC0 * WF_GRAN * WAVE) : 0;
    const size_t wfc_off = p->has_wf ? take(sizeof(unsigned) * (WF_CTRL_WORDS + WF_STICKY_WORDS)) : 0;
    const size_t zi_off = take((size_t)B * NR0 * NC0);
    const size_t zt_off = p->has_zt ? take((size_t)7 * B * NR0 * NC0) : 0;
    size_t gz_off[2] = {0, 0}, mr_off[2] = {0, 0};
    for (int i = 0; i < 2; ++i) gz_off[i] = p->has_gz[i] ? take((size_t)7 * B * tiles(p->lv[i + 1].w)) : 0;
    for (int i = 0; i < 2; ++i) mr_off[i] = p->has_mr[i] ? take((size_t)B * tiles(p->lv[i + 1].w) * tiles(p->lv[i + 1].h)) : 0;
    const size_t ck_off = p->recompute ? take(sizeof(double) * 3 * NC0 * 7 * B * (size_t)(v0.h + 64)) : 0;
    // x-sweep state [4][lines] followed by the y state the wavefront kernel leaves [4][planes][pitch]
    const size_t state_n = 4 * 7 * B * (size_t)(v0.h + 64) + 4 * 7 * B * (size_t)std::max(v0.h + 64, v0.pitch);
    const size_t st_off = take(sizeof(double) * state_n);
    static_assert(sizeof(unsigned) * IDX_HEAD_WORDS % alignof(SeamDev) == 0 && IDX_TODO_WORD + MAXB <= MK_COUNT_WORD && MK_COUNT_WORD + 3 <= MK_TODO_WORD &&
                      MK_TODO_WORD + MAXB <= IDX_HEAD_WORDS,
                  "the words in front of the seam records: three counts, the index planes' todo words, the mask pyramids' counts and todo words");
    static_assert(MAXB <= 32 && WF_STAND_WORD >= 8 && WF_STAND_WORD < WF_STICKY_WORDS, "one bit per slot in a word behind the sticky count and its three 64-bit counts");
    const size_t seam_off = take(sizeof(unsigned) * IDX_HEAD_WORDS + sizeof(SeamDev) * B);
    const size_t ik_off = take(sizeof(IndexKey) * B);  // zero at creation: no slot holds a plane
    const size_t mk_off = take(sizeof(MaskKey) * B);   // zero at creation: no slot holds a mask pyramid
    const size_t side_off = take(sizeof(float) * B * v0.pitch);
    const size_t zp_off = take(4096);  // zeros for good (k_vv_xby_m's loader reads a flagged tile from here)
    // the index planes in 16-byte runs: per tile 4 KB of bases, 512 B of patch records, one class byte (a plan that can be source-fused)
    const size_t sr_tiles = !planes_in && p->src_fuse ? (size_t)B * NR0 * NC0 : 0;
    const size_t sr_base_off = take(sr_tiles * 4 * WAVE * sizeof(u4)), sr_patch_off = take(sr_tiles * src_runs::SR_MAX_PATCHES * sizeof(uint2)), sr_cls_off = take(sr_tiles), sr_live_off = take(sr_tiles);
    p->runs_bytes = off - sr_base_off;
    p->arena_bytes = off;
    if (hipMalloc(&p->arena, off) != hipSuccess) {
        (void)hipGetLastError();
        delete p;
        return fail(STITCH_ERR_HIP, "plan_create: hipMalloc of %zu bytes failed", off);
    }
    char* base = static_cast<char*>(p->arena);
    for (int l = 0; l < L; ++l) {
        Level& v = p->lv[l];
        v.g = reinterpret_cast<float*>(base + g_off[l]);
        v.e = (l >= 1 || L == 1) ? reinterpret_cast<float*>(base + e_off[l]) : nullptr;
        if (l + 1 < L) {
            v.ix = reinterpret_cast<int32_t*>(base + ix_off[l]);
            v.ax = reinterpret_cast<double*>(base + ax_off[l]);
            v.iy = reinterpret_cast<int32_t*>(base + iy_off[l]);
            v.ay = reinterpret_cast<double*>(base + ay_off[l]);
        }
    }
    p->T = reinterpret_cast<float*>(base + t_off);
    p->T2 = o.blur_kind == 1 ? reinterpret_cast<float*>(base + t2_off) : nullptr;
    p->state = reinterpret_cast<double*>(base + st_off);
    p->idx_head = reinterpret_cast<unsigned*>(base + seam_off);
    p->d_seam = reinterpret_cast<SeamDev*>(p->idx_head + IDX_HEAD_WORDS);
    p->idx_keys = reinterpret_cast<IndexKey*>(base + ik_off);
    p->mask_keys = reinterpret_cast<MaskKey*>(base + mk_off);
    p->side = reinterpret_cast<float*>(base + side_off);
    p->zero_page = reinterpret_cast<const float*>(base + zp_off);
    if (sr_tiles) p->runs = SrcRuns{reinterpret_cast<unsigned*>(base + sr_base_off), reinterpret_cast<uint2*>(base + sr_patch_off), reinterpret_cast<uint8_t*>(base + sr_cls_off), reinterpret_cast<uint8_t*>(base + sr_live_off), NR0, NC0, 1};
    if (p->has_wf) {
        p->wf_yg = reinterpret_cast<u64*>(base + yg_off);
        p->wf_yg_bytes = sizeof(u64) * B * 7 * NC0 * WF_GRAN * WAVE;
        p->wf_ctrl = reinterpret_cast<unsigned*>(base + wfc_off);
        if (tn.xbyf_spin_limit >= 0) p->wf_spin_limit = (unsigned)tn.xbyf_spin_limit;
    }
    if (p->has_zt) {
        p->zt = reinterpret_cast<uint8_t*>(base + zt_off);
        p->zi = reinterpret_cast<uint8_t*>(base + zi_off);
        for (int i = 0; i < 2; ++i) p->gz[i] = p->has_gz[i] ? reinterpret_cast<uint8_t*>(base + gz_off[i]) : nullptr;
        for (int i = 0; i < 2; ++i) p->mr[i] = p->has_mr[i] ? reinterpret_cast<uint8_t*>(base + mr_off[i]) : nullptr;
        if (p->recompute) p->ckpt = reinterpret_cast<double*>(base + ck_off);
        if (tn.xbyf_wgs >= 0) p->wf_max_wgs = std::max(1, tn.xbyf_wgs);
        if (tn.xbyf_early >= 0) p->wf_early_read = tn.xbyf_early != 0;
    }
    // the diagnostic stamp buffers the shape asks for; one that cannot be had is struck from the shape
    auto stamp_buffer = [](unsigned long long** d, size_t words) {
        if (hipMalloc((void**)d, sizeof(unsigned long long) * words) == hipSuccess && hipMemset(*d, 0, sizeof(unsigned long long) * words) == hipSuccess) return true;
        (void)hipGetLastError();
        *d = nullptr;
        return false;
    };
    if (std::getenv("STITCH_D7_STAMP")) stamp_buffer(&p->d7_dbg, 7 * ((size_t)(v0.h + YCH - 1) / YCH + 1) + 8);
    if (p->stamp_xy) p->stamp_xy = stamp_buffer(&p->xy_dbg, (size_t)5 * NC0);
    if (p->stamp_wf) p->stamp_wf = stamp_buffer(&p->wf_dbg, (size_t)p->wf_max_wgs * 8);  // one record per persistent workgroup, sized from the workgroup count actually used
    if (p->stamp_co) p->stamp_co = stamp_buffer(&p->co_dbg, (size_t)CO_MAXL * 8);
    // the slack rows and pitch padding are read by partial tiles: give them defined (zero) contents once
    if (hipMemset(p->arena, 0, off) != hipSuccess || hipHostMalloc((void**)&p->h_idx_head, sizeof(unsigned) * IDX_HEAD_WORDS + sizeof(SeamDev) * B) != hipSuccess) {
        stitch_plan_destroy(p);
        return fail(STITCH_ERR_HIP, "plan_create: workspace initialisation failed");
    }
#ifdef STITCH_ZP_POISON  // (defined only to prove that a test reads flagged tiles from here: the page is then anything but zero)
    (void)hipMemset(base + zp_off, 0x3f, 4096);
#endif
    // resize tables (CImg.h:29625-29637), computed on the host once per plan
    for (int l = 0; l + 1 < L; ++l) {
        Level& v = p->lv[l];
        std::vector<int32_t> idx;
        std::vector<double> al;
        expand_table(p->lv[l + 1].w, v.w, idx, al);
        (void)hipMemcpy(v.ix, idx.data(), sizeof(int32_t) * v.w, hipMemcpyHostToDevice);
        (void)hipMemcpy(v.ax, al.data(), sizeof(double) * v.w, hipMemcpyHostToDevice);
        expand_table(p->lv[l + 1].h, v.h, idx, al);
        (void)hipMemcpy(v.iy, idx.data(), sizeof(int32_t) * v.h, hipMemcpyHostToDevice);
        if (hipMemcpy(v.ay, al.data(), sizeof(double) * v.h, hipMemcpyHostToDevice) != hipSuccess) {
            stitch_plan_destroy(p);
            return fail(STITCH_ERR_HIP, "plan_create: table upload failed");
        }
    }
    std::memset(p->h_idx_head, 0, sizeof(unsigned) * IDX_HEAD_WORDS + sizeof(SeamDev) * B);
    p->h_seam = reinterpret_cast<SeamDev*>(p->h_idx_head + IDX_HEAD_WORDS);
    if (p->has_wf) {
        if (hipHostMalloc((void**)&p->h_wf_abort, sizeof(unsigned)) != hipSuccess) {
            stitch_plan_destroy(p);
            return fail(STITCH_ERR_HIP, "plan_create: pinned allocation failed");
        }
        *p->h_wf_abort = 0;
    }
    *plan_out = p;
    return STITCH_OK;
}

void stitch_plan_destroy(stitch_plan* p) {
    if (!p) return;
    if (p->pending && p->last_stream != nullptr) (void)hipStreamSynchronize(p->last_stream);
    else if (p->pending) (void)hipDeviceSynchronize();
    for (auto& r : p->recs) {
        (void)hipEventDestroy(r.a);
        (void)hipEventDestroy(r.b);
    }
    for (auto e : p->free_events) (void)hipEventDestroy(e);
    if (p->arena) (void)hipFree(p->arena);
    if (p->h_idx_head) (void)hipHostFree(p->h_idx_head);  // (h_seam lies in it)
    if (p->h_wf_abort) (void)hipHostFree(p->h_wf_abort);
    if (p->d7_dbg) {
        const int nc = p->d7_dbg_chunks;
        std::vector<unsigned long long> h((size_t)7 * std::max(nc, 1) + 8);
        if (nc > 8 && hipMemcpy(h.data(), p->d7_dbg, sizeof(unsigned long long) * (7 * nc + 6), hipMemcpyDeviceToHost) == hipSuccess) {
            static const char* nm[7] = {"loader", "chain 0", "chain 1", "cons 0", "cons 1", "cons 2", "cons 3"};
            const unsigned long long t0 = h[0];
            std::fprintf(stderr, "[k_vv_y_bwd_dec7 stamps, level %d, %d chunks, middle workgroup of plane 0: ticks since the loader's first chunk, every %d-th chunk; then ticks per chunk over the middle half]\n",
                         p->stamp_d7_level, nc, std::max(1, nc / 16));
            for (int wv = 0; wv < 7; ++wv) {
                std::fprintf(stderr, "  %-8s", nm[wv]);
                const int c0 = wv >= 3 ? wv - 3 : 0, step = wv >= 3 ? 4 : 1;  // consumer c stamps chunks c, c+4, ...
                for (int j = 0; j < nc; j += std::max(1, nc / 16)) {
                    const int jj = c0 + (j / step) * step;
                    if (jj < nc) std::fprintf(stderr, " %7.0f", (double)h[(size_t)wv * nc + jj] - (double)t0);
                }
                const int ja = c0 + (nc / 4 / step) * step, jb = c0 + (3 * nc / 4 / step) * step;
                if (jb > ja && jb < nc) std::fprintf(stderr, " | %.1f per chunk", ((double)h[(size_t)wv * nc + jb] - (double)h[(size_t)wv * nc + ja]) / (jb - ja));
                std::fprintf(stderr, "\n");
            }
            if (h[(size_t)7 * nc + 1])
                std::fprintf(stderr, "  chain 0, ticks per chunk by segment: top + prefetch %.0f | rows 0-3 %.0f | release %.0f | rows 4-7 %.0f | write back %.0f | tail + back edge %.0f\n",
                             (double)h[(size_t)7 * nc + 0] / nc, (double)h[(size_t)7 * nc + 1] / nc, (double)h[(size_t)7 * nc + 2] / nc, (double)h[(size_t)7 * nc + 3] / nc,
                             (double)h[(size_t)7 * nc + 4] / nc, (double)h[(size_t)7 * nc + 5] / nc);
        }
        (void)hipFree(p->d7_dbg);
    }
    if (p->xy_dbg) {
        const int nc = p->xy_dbg_nc;
        std::vector<unsigned long long> h((size_t)5 * std::max(nc, 1));
        if (nc > 0 && hipMemcpy(h.data(), p->xy_dbg, sizeof(unsigned long long) * 5 * nc, hipMemcpyDeviceToHost) == hipSuccess) {
            static const char* nm[5] = {"x chain", "y chain", "loader", "storer", "courier"};
            const unsigned long long t0 = h[2 * (size_t)nc];  // the loader's first tile
            std::fprintf(stderr, "[k_vv_xby_m stamps, middle band of plane 0, last level-0 launch: ticks since the loader's first tile / 1000, per tile]\n");
            for (int wv = 0; wv < 5; ++wv) {
                std::fprintf(stderr, "  %-8s", nm[wv]);
                for (int j = 0; j < nc; j += std::max(1, nc / 24)) std::fprintf(stderr, " %6.1f", ((double)h[(size_t)wv * nc + j] - (double)t0) * 1e-3);
                std::fprintf(stderr, " | last %6.1f\n", ((double)h[(size_t)wv * nc + nc - 1] - (double)t0) * 1e-3);
            }
        }
        (void)hipFree(p->xy_dbg);
    }
    if (p->co_dbg) {
        unsigned long long h[CO_MAXL * 8];
        if (hipMemcpy(h, p->co_dbg, sizeof h, hipMemcpyDeviceToHost) == hipSuccess) {
            // s_memtime counts at 100 MHz: 10 ns per tick
            const int nl = p->L - p->coarse_from;
            std::fprintf(stderr, "[k_coarse stamps, pair 0 of the last launch, us] levels %d..%d:", p->coarse_from, p->L - 1);
            for (int i = 0; i + 1 < nl; ++i) {
                const unsigned long long t0 = i == 0 ? h[0] : h[(i - 1) * 8 + 3];
                std::fprintf(stderr, " | %dx%d x %.1f y %.1f dec %.1f", p->lv[p->coarse_from + i].w, p->lv[p->coarse_from + i].h, (h[i * 8 + 1] - t0) * 0.01,
                             (h[i * 8 + 2] - h[i * 8 + 1]) * 0.01, (h[i * 8 + 3] - h[i * 8 + 2]) * 0.01);
            }
            std::fprintf(stderr, " | top %.1f | collapse", (h[(nl - 1) * 8 + 4] - h[(nl - 2) * 8 + 3]) * 0.01);
            unsigned long long prev = h[(nl - 1) * 8 + 4];
            for (int i = nl - 2; i >= 0; --i) {
                std::fprintf(stderr, " %.1f", (h[i * 8 + 5] - prev) * 0.01);
                prev = h[i * 8 + 5];
            }
            std::fprintf(stderr, " | total %.1f\n", (prev - h[0]) * 0.01);
        }
        (void)hipFree(p->co_dbg);
    }
    if (p->wf_dbg) {
        const size_t nwg = (size_t)p->wf_max_wgs;
        std::vector<unsigned long long> hsum(nwg * 8);
        if (hipMemcpy(hsum.data(), p->wf_dbg, sizeof(unsigned long long) * nwg * 8, hipMemcpyDeviceToHost) == hipSuccess) {
            double tot[8] = {0};
            for (size_t i = 0; i < nwg; ++i)
                for (int j = 0; j < 8; ++j) tot[j] += (double)hsum[i * 8 + j];
            static const char* nm[8] = {"claim", "tile-fetch", "x-sweep", "y-wait", "y-sweep", "store", "-", "-"};
            double all = 0;
            for (int j = 0; j < 6; ++j) all += tot[j];
            std::fprintf(stderr, "[wavefront stamps, last level-0 launch, share of workgroup time]");
            for (int j = 0; j < 6; ++j) std::fprintf(stderr, " %s %.1f%%", nm[j], 100.0 * tot[j] / all);
            std::fprintf(stderr, " | mean cycles per workgroup %.0f\n", all / (double)nwg);
        }
        (void)hipFree(p->wf_dbg);
    }
    delete p;
}

size_t stitch_plan_workspace_bytes(const stitch_plan* p) { return p ? p->arena_bytes : 0; }
const void* stitch_plan_workspace_base(const stitch_plan* p) { return p ? p->arena : nullptr; }

int stitch_plan_levels(const stitch_plan* p, int* level_w, int* level_h) {
    if (!p) return fail(STITCH_ERR_ARG, "null plan");
    for (int l = 0; l < p->L; ++l) {
        if (level_w) level_w[l] = p->lv[l].w;
        if (level_h) level_h[l] = p->lv[l].h;
    }
    return p->L;
}

int stitch_dev_blend_u8(stitch_plan* plan, const uint8_t* d_a, const uint8_t* d_b, uint8_t* d_out, void* stream) {
    return dev_blend(plan, d_a, d_b, d_out, stream);
}
int stitch_dev_blend_f32(stitch_plan* plan, const float* d_a, const float* d_b, float* d_out, void* stream) {
    return dev_blend(plan, d_a, d_b, d_out, stream);
}
int stitch_dev_pair_u8(stitch_plan* plan, const uint8_t* d_frame, int fw, int fh, const double p[8], float offx, float offy,
                       const uint8_t* d_mosaic, int mw, int mh, int ox, int oy, uint8_t* d_out, void* stream) {
    return dev_pair(plan, d_frame, fw, fh, p, offx, offy, d_mosaic, mw, mh, ox, oy, d_out, stream);
}
int stitch_dev_pair_f32(stitch_plan* plan, const float* d_frame, int fw, int fh, const double p[8], float offx, float offy,
                        const float* d_mosaic, int mw, int mh, int ox, int oy, float* d_out, void* stream) {
    return dev_pair(plan, d_frame, fw, fh, p, offx, offy, d_mosaic, mw, mh, ox, oy, d_out, stream);
}

int stitch_plan_status_at(stitch_plan* p, int index, stitch_seam* seam_out) {
    if (!p) return fail(STITCH_ERR_ARG, "null plan");
    if (index < 0 || index >= std::max(1, p->last_n))
        return fail(STITCH_ERR_ARG, "status: index %d outside the %d pair(s) of the plan's last call", index, p->last_n);
    if (p->pending) {
        HIPCHK(hipStreamSynchronize(p->last_stream));
        p->pending = false;
    }
    if (p->h_wf_abort && *p->h_wf_abort != p->wf_abort_seen)
        return fail(STITCH_ERR_HIP,
                    "fused sweep: %u hand-off wait(s) timed out in this or an earlier queued call on the plan (every result since the "
                    "last stitch_plan_clear_fault is invalid)",
                    *p->h_wf_abort - p->wf_abort_seen);
    const SeamDev& sd = p->h_seam[index];
    seam_to_public(sd, seam_out);
    if (sd.status == -2) return fail(STITCH_ERR_EMPTY_MIDROW, "blend: channel 0 of a's middle row is empty (pair %d)", index);
    if (sd.status == -3) return fail(STITCH_ERR_ZERO_OVERLAP, "blend: a and b do not overlap on the middle row (pair %d)", index);
    return STITCH_OK;
}

int stitch_plan_status(stitch_plan* p, stitch_seam* seam_out) { return stitch_plan_status_at(p, 0, seam_out); }

int stitch_plan_set_handoff_spin_limit(stitch_plan* p, unsigned polls) {
    if (!p) return fail(STITCH_ERR_ARG, "null plan");
    p->wf_spin_limit = polls;
    return STITCH_OK;
}

int stitch_plan_handoff_counts(stitch_plan* p, uint64_t out[3]) {
    if (!p || !out) return fail(STITCH_ERR_ARG, "null plan or output");
    if (p->pending) {
        HIPCHK(hipStreamSynchronize(p->last_stream));
        p->pending = false;
    }
    out[0] = out[1] = out[2] = 0;
    // the 64-bit words behind the sticky count (Wavefront::sticky): like it, no launch sequence clears them
    if (p->wf_ctrl) HIPCHK(hipMemcpy(out, p->wf_ctrl + WF_CTRL_WORDS + 2, 3 * sizeof(uint64_t), hipMemcpyDeviceToHost));
    return STITCH_OK;
}

int stitch_plan_g_flag_counts(stitch_plan* p, uint64_t out[2]) {
    if (!p || !out) return fail(STITCH_ERR_ARG, "null plan or output");
    if (p->pending) {
        HIPCHK(hipStreamSynchronize(p->last_stream));
        p->pending = false;
    }
    for (int i = 0; i < 2; ++i) {
        out[i] = 0;
        if (!p->last_form.lv[i].g_out || !p->gz[i] || p->last_n <= 0) continue;  // (the bytes of a call without flags are an earlier call's)
        std::vector<uint8_t> h((size_t)7 * p->last_n * ((p->lv[i + 1].w + TS - 1) / TS));
        HIPCHK(hipMemcpy(h.data(), p->gz[i], h.size(), hipMemcpyDeviceToHost));
        for (uint8_t f : h) out[i] += f != 0;
    }
    return STITCH_OK;
}

int stitch_plan_index_counts(stitch_plan* p, uint32_t out[3]) {
    if (!p || !out) return fail(STITCH_ERR_ARG, "null plan or output");
    if (p->pending) {
        HIPCHK(hipStreamSynchronize(p->last_stream));
        p->pending = false;
    }
    for (int i = 0; i < 3; ++i) out[i] = p->last_idx ? p->h_idx_head[i] : 0u;  // (the words of a call without an index plane are an earlier call's)
    return STITCH_OK;
}

int stitch_plan_mask_keep_counts(stitch_plan* p, uint32_t out[2]) {
    if (!p || !out) return fail(STITCH_ERR_ARG, "null plan or output");
    if (p->pending) {
        HIPCHK(hipStreamSynchronize(p->last_stream));
        p->pending = false;
    }
    for (int i = 0; i < 2; ++i) out[i] = p->last_n > 0 && !p->planes_in ? p->h_idx_head[MK_COUNT_WORD + i] : 0u;
    return STITCH_OK;
}

int stitch_plan_src_run_counts(stitch_plan* p, uint32_t out[4]) {
    if (!p || !out) return fail(STITCH_ERR_ARG, "null plan or output");
    if (p->pending) {
        HIPCHK(hipStreamSynchronize(p->last_stream));
        p->pending = false;
    }
    for (int i = 0; i < 4; ++i) out[i] = 0;
    if (!p->last_runs) return STITCH_OK;  // (the arrays of a call that was not handed them are an earlier call's)
    const size_t nt = (size_t)p->runs.NR * p->runs.NC;
    std::vector<uint8_t> cls(nt), live(nt);
    for (int i = 0; i < p->last_n; ++i) {
        if (p->last_owner[i] != i) continue;  // a pair that reads an earlier pair's plane
        HIPCHK(hipMemcpy(cls.data(), p->runs.cls + i * nt, nt, hipMemcpyDeviceToHost));
        HIPCHK(hipMemcpy(live.data(), p->runs.live + i * nt, nt, hipMemcpyDeviceToHost));
        for (size_t t = 0; t < nt; ++t) ++out[!live[t] ? 0 : cls[t] == 0 ? 1 : cls[t] == src_runs::SR_GENERAL ? 3 : 2];
    }
    return STITCH_OK;
}

int stitch_src_run_classes(const double p[8], float offx, float offy, int fw, int fh, int cw, int ch, int px_bytes, uint32_t counts[4], uint8_t* cls) {
    if (!p || !counts || fw <= 0 || fh <= 0 || cw <= 0 || ch <= 0 || (px_bytes != 4 && px_bytes != 1) || (unsigned long long)fw * fh * px_bytes >= 0xfffffff0ULL)
        return fail(STITCH_ERR_ARG, "src_run_classes: null map or counts, a non-positive size, a sample size other than 4 or 1, or a plane of 4 GB");
    src_runs::host_classes(p, offx, offy, fw, fh, cw, ch, (unsigned)px_bytes, counts, cls);
    return STITCH_OK;
}

int stitch_plan_src_runs_fill(stitch_plan* p, int byte) {
    if (!p) return fail(STITCH_ERR_ARG, "null plan");
    if (p->pending) {
        HIPCHK(hipStreamSynchronize(p->last_stream));
        p->pending = false;
    }
    if (p->runs.cls) HIPCHK(hipMemset(p->runs.bases, byte, p->runs_bytes));
    HIPCHK(hipDeviceSynchronize());
    return STITCH_OK;
}

int stitch_plan_collapse_sides(stitch_plan* p, int pair, int counts[3]) {
    if (!p || !counts) return fail(STITCH_ERR_ARG, "null plan or output");
    if (pair < 0 || pair >= std::max(1, p->last_n))
        return fail(STITCH_ERR_ARG, "collapse_sides: pair %d outside the %d pair(s) of the plan's last call", pair, p->last_n);
    if (p->pending) {
        HIPCHK(hipStreamSynchronize(p->last_stream));
        p->pending = false;
    }
    const SeamDev& sd = p->h_seam[pair];
    c4_side_counts(sd.branch, sd.start, sd.thr, p->c4_l0_xa, p->last_n > 0 ? p->c4_l0_xb : p->c4_l0_xa, p->c4_l0_sides ? 1 : 0, counts);
    return STITCH_OK;
}

int stitch_plan_mask_row_counts(stitch_plan* p, uint64_t out[2]) {
    if (!p || !out) return fail(STITCH_ERR_ARG, "null plan or output");
    if (p->pending) {
        HIPCHK(hipStreamSynchronize(p->last_stream));
        p->pending = false;
    }
    for (int i = 0; i < 2; ++i) {
        out[i] = 0;
        if (!p->last_form.lv[i].mr_out || !p->mr[i] || p->last_n <= 0) continue;  // (the bytes of a call without flags are an earlier call's)
        const ZeroTiles m = mask_rows(p->mr[i], p->lv[i + 1].w, p->lv[i + 1].h);
        std::vector<uint8_t> h((size_t)p->last_n * m.NC * m.NR);
        HIPCHK(hipMemcpy(h.data(), p->mr[i], h.size(), hipMemcpyDeviceToHost));
        for (uint8_t f : h) out[i] += f != 0;
    }
    return STITCH_OK;
}

int stitch_plan_clear_fault(stitch_plan* p) {
    if (!p) return fail(STITCH_ERR_ARG, "null plan");
    if (p->pending) {
        HIPCHK(hipStreamSynchronize(p->last_stream));
        p->pending = false;
    }
    if (p->h_wf_abort) p->wf_abort_seen = *p->h_wf_abort;
    // no slot's index plane is taken on trust after a fault
    HIPCHK(hipMemsetAsync(p->idx_keys, 0, sizeof(IndexKey) * p->cap, p->last_stream));
    HIPCHK(hipMemsetAsync(p->mask_keys, 0, sizeof(MaskKey) * p->cap, p->last_stream));  // nor does a mask pyramid stand
    HIPCHK(hipStreamSynchronize(p->last_stream));
    return STITCH_OK;
}

int stitch_plan_capacity(const stitch_plan* p) { return p ? p->cap : 0; }
int stitch_plan_coarse_from(const stitch_plan* p) { return p ? p->coarse_from : 0; }
int stitch_plan_fast_paths(const stitch_plan* p) { return p ? capability_mask(*p) : 0; }
int stitch_plan_fused_sweep_levels(const stitch_plan* p) { return p ? p->wf_levels : 0; }
int stitch_plan_collapse_range(const stitch_plan* p, int level, int* xa, int* xb, int* per_lane_taps) {
    if (!p || level < 0 || level + 1 >= p->L || !xa || !xb || !per_lane_taps) return fail(STITCH_ERR_ARG, "plan_collapse_range: bad argument");
    const Level& v = p->lv[level];
    *xa = p->collapse4 ? v.c4_xa : 0;
    *xb = p->collapse4 ? v.c4_xb : 0;
    *per_lane_taps = p->collapse4 ? v.c4_gen : 0;
    return STITCH_OK;
}
int stitch_plan_call_forms(const stitch_plan* p, int n_pairs) {
    if (!p || n_pairs < 1 || n_pairs > p->cap) return 0;
    const CallForm c = call_form(*p, n_pairs, source_fused_call(*p, n_pairs), false);
    int f = 0;
    if (c.src) f |= STITCH_FAST_SOURCE_FUSED;
    if (c.lv[0].sweep == SW_BATCH || c.lv[0].xby) f |= STITCH_FAST_FUSED_SWEEP;  // k_vv_xbyf; one pair in flight: k_vv_xby_m
    if (mask_keep_word(*p, c, false) & MK_KEEP_OK) f |= STITCH_CALL_MASK_KEEP;  // include/stitch_mask_keep.h
    return f;
}

int stitch_dev_pairs_u8(stitch_plan* plan, const stitch_pair_desc* pairs, int n, void* stream) {
    return dev_pairs<uint8_t>(plan, pairs, n, stream);
}
int stitch_dev_pairs_f32(stitch_plan* plan, const stitch_pair_desc* pairs, int n, void* stream) {
    return dev_pairs<float>(plan, pairs, n, stream);
}

int stitch_plan_set_profiling(stitch_plan* p, int enabled) {
    if (!p) return fail(STITCH_ERR_ARG, "null plan");
    p->profiling = enabled != 0;
    p->prof_only = -1;
    return STITCH_OK;
}

int stitch_plan_set_profiling_kernel(stitch_plan* p, int kernel_id) {
    if (!p) return fail(STITCH_ERR_ARG, "null plan");
    if (kernel_id < 0 || kernel_id >= STITCH_K_COUNT) return fail(STITCH_ERR_ARG, "bad kernel id %d", kernel_id);
    p->profiling = true;
    p->prof_only = kernel_id;
    return STITCH_OK;
}

int stitch_plan_read_profile(stitch_plan* p, double stage_ms[STITCH_K_COUNT], int stage_launches[STITCH_K_COUNT],
                             double level0_ms[STITCH_K_COUNT]) {
    if (!p) return fail(STITCH_ERR_ARG, "null plan");
    if (p->pending) {
        HIPCHK(hipStreamSynchronize(p->last_stream));
        p->pending = false;
    }
    for (int i = 0; i < STITCH_K_COUNT; ++i) {
        if (stage_ms) stage_ms[i] = 0;
        if (stage_launches) stage_launches[i] = 0;
        if (level0_ms) level0_ms[i] = 0;
    }
    for (auto& r : p->recs) {
        float ms = 0;
        HIPCHK(hipEventElapsedTime(&ms, r.a, r.b));
        if (stage_ms) stage_ms[r.stage] += ms;
        if (stage_launches) stage_launches[r.stage] += 1;
        if (level0_ms && r.level == 0) level0_ms[r.stage] += ms;
        p->free_events.push_back(r.a);
        p->free_events.push_back(r.b);
    }
    p->recs.clear();
    return STITCH_OK;
}

int stitch_dev_equalize_u8(uint8_t* d_img, int w, int h, int32_t* d_hist256, void* stream) {
    return dev_equalize_impl(d_img, w, h, d_hist256, false, 0, 1, stream);
}

int stitch_dev_lummix_u8(uint8_t* d_result, const uint8_t* d_equalized, int w, int h, double num, double den, void* stream) {
    int rc = need_device();
    if (rc) return rc;
    if (!d_result || !d_equalized || w <= 0 || h <= 0) return fail(STITCH_ERR_ARG, "lummix: null buffer or bad size %dx%d", w, h);
    const size_t n = (size_t)w * h;
    k_lummix<<<eq_grid(n), 256, 0, as_stream(stream)>>>(d_result, d_equalized, n, mix_params(num, den));
    return launch_check("k_lummix");
}

int stitch_dev_finish_u8(uint8_t* d_result, int w, int h, double num, double den, int32_t* d_hist256, void* stream) {
    return dev_equalize_impl(d_result, w, h, d_hist256, true, num, den, stream);
}

// ---- SURVEY.md 8(f) rows 1 and 2 -------------------------------------------------------------------------------
int stitch_dev_gray_u8(const uint8_t* d_rgb, int w, int h, uint8_t* d_gray, float* d_gray_f32, void* stream) {
    int rc = need_device();
    if (rc) return rc;
    if (!d_rgb || (!d_gray && !d_gray_f32) || w <= 0 || h <= 0) return fail(STITCH_ERR_ARG, "gray: bad argument");
    const size_t n = (size_t)w * h;
    k_gray<<<eq_grid(n), 256, 0, as_stream(stream)>>>(d_rgb, n, d_gray, d_gray_f32);
    return launch_check("k_gray");
}
// ---- l-alpha-beta colour transfer ---------------------------------------------------------------------------------
int stitch_dev_transfer_u8(const uint8_t* d_src, int sw, int sh, const uint8_t* d_tem, int tw, int th, uint8_t* d_out, float* d_stats12,
                           void* stream) {
    int rc = need_device();
    if (rc) return rc;
    if (!d_src || !d_tem || !d_out || sw <= 0 || sh <= 0 || tw <= 0 || th <= 0) return fail(STITCH_ERR_ARG, "transfer: null buffer or bad size");
    if ((long long)sw * sh > 0x7fffffffLL || (long long)tw * th > 0x7fffffffLL)
        return fail(STITCH_ERR_ARG, "transfer: w*h overflows int (the reference's int product)");
    const size_t ns = (size_t)sw * sh, nt = (size_t)tw * th;
    TrK k{};
    k.a1 = (float)(1.0 / std::sqrt(3.0));
    k.b1 = (float)(1.0 / std::sqrt(6.0));
    k.c1 = (float)(1.0 / std::sqrt(2.0));
    k.a2 = (float)(std::sqrt(3.0) / 3.0);
    k.b2 = (float)(std::sqrt(6.0) / 6.0);
    k.c2 = (float)(std::sqrt(2.0) / 2.0);
    k.ln10 = 2.302585092994046;  // log(10)
    hipStream_t s = as_stream(stream);
    float* scratch = nullptr;
    HIPCHK(hipMallocAsync((void**)&scratch, sizeof(float) * (3 * (ns + nt) + 16), s));
    float *lab_s = scratch, *lab_t = scratch + 3 * ns, *stats = scratch + 3 * (ns + nt);
    k_tr_to_lab<<<eq_grid(ns), 256, 0, s>>>(d_src, ns, k, lab_s);
    k_tr_to_lab<<<eq_grid(nt), 256, 0, s>>>(d_tem, nt, k, lab_t);
    k_tr_stats<<<6, 64, 0, s>>>(lab_s, ns, (float)(sw * sh), lab_t, nt, (float)(tw * th), stats);
    k_tr_apply<<<eq_grid(ns), 256, 0, s>>>(lab_s, ns, stats, k, d_out);
    if (d_stats12) HIPCHK(hipMemcpyAsync(d_stats12, stats, sizeof(float) * 12, hipMemcpyDeviceToDevice, s));
    HIPCHK(hipFreeAsync(scratch, s));
    return launch_check("transfer");
}
int stitch_transfer_u8(const uint8_t* src, int sw, int sh, const uint8_t* tem, int tw, int th, uint8_t* out, float stats_out[12]) {
    int rc = need_device();
    if (rc) return rc;
    if (!src || !tem || !out || sw <= 0 || sh <= 0 || tw <= 0 || th <= 0) return fail(STITCH_ERR_ARG, "transfer: null buffer or bad size");
    const size_t bs = (size_t)3 * sw * sh, bt = (size_t)3 * tw * th;
    DevBuf a, b, o, st;
    if ((rc = a.alloc(bs)) || (rc = b.alloc(bt)) || (rc = o.alloc(bs)) || (rc = st.alloc(sizeof(float) * 12))) return rc;
    HIPCHK(hipMemcpy(a.p, src, bs, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(b.p, tem, bt, hipMemcpyHostToDevice));
    if ((rc = stitch_dev_transfer_u8(a.as<uint8_t>(), sw, sh, b.as<uint8_t>(), tw, th, o.as<uint8_t>(), st.as<float>(), nullptr))) return rc;
    HIPCHK(hipMemcpy(out, o.p, bs, hipMemcpyDeviceToHost));
    if (stats_out) HIPCHK(hipMemcpy(stats_out, st.p, sizeof(float) * 12, hipMemcpyDeviceToHost));
    return STITCH_OK;
}

// ---- BMP <-> planar RGB ------------------------------------------------------------------------------------------
static int le32(const uint8_t* p) { return (int)((uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24)); }
int stitch_bmp_parse(const uint8_t* f, size_t n, stitch_bmp_info* info) {
    // CImg.h:48401-48441, for the layouts this path meets; every quantity as the reference derives it
    if (!f || !info) return fail(STITCH_ERR_ARG, "bmp_parse: null argument");
    if (n < 54 || f[0] != 'B' || f[1] != 'M') return fail(STITCH_ERR_ARG, "bmp_parse: not a BMP file");
    int file_size = le32(f + 0x02);
    const int offset = le32(f + 0x0A), header_size = le32(f + 0x0E), dx = le32(f + 0x12), dy = le32(f + 0x16), compression = le32(f + 0x1E),
              bpp = f[0x1C] + (f[0x1D] << 8);
    if (!file_size || file_size == offset) file_size = (int)n;
    if (compression) return fail(STITCH_ERR_ARG, "bmp_parse: compressed BMP (compression=%d) is not supported", compression);
    if (bpp != 24 && bpp != 32) return fail(STITCH_ERR_ARG, "bmp_parse: only 24- and 32-bit BMP is supported (bpp=%d)", bpp);
    if (dx <= 0 || dy == 0 || dy == INT32_MIN) return fail(STITCH_ERR_ARG, "bmp_parse: bad size %d x %d", dx, dy);
    const int h = dy < 0 ? -dy : dy;
    const long long dx_bytes = (long long)dx * bpp / 8;
    const int align_bytes = (int)((4 - dx_bytes % 4) % 4);
    const unsigned long long want = (unsigned long long)h * (unsigned long long)(dx_bytes + align_bytes);
    const unsigned long long avail_hdr = (unsigned long long)(long long)file_size - (unsigned long long)(long long)offset;
    unsigned long long buf = std::min(want, avail_hdr);
    long long pos = 54;
    if (header_size > 40) pos += header_size - 40;
    const long long xoffset = (long long)offset - 14 - header_size;
    if (xoffset > 0) pos += xoffset;
    if (pos < 0 || (unsigned long long)pos > n) return fail(STITCH_ERR_ARG, "bmp_parse: pixel data starts beyond the file");
    buf = std::min(buf, (unsigned long long)n - (unsigned long long)pos);
    info->width = dx;
    info->height = h;
    info->bpp = bpp;
    info->top_down = dy < 0;
    info->data_pos = (uint64_t)pos;
    info->stride = (uint64_t)(dx_bytes + align_bytes);
    info->data_bytes = buf;
    return STITCH_OK;
}
size_t stitch_bmp_file_bytes(int w, int h) {
    if (w <= 0 || h <= 0) return 0;
    return 54 + (((size_t)3 * w + 3) & ~(size_t)3) * (size_t)h;
}
static int bmp_align(const void* p, unsigned long long pos) {
    const unsigned long long a = (unsigned long long)reinterpret_cast<uintptr_t>(p) + pos;
    return (a & 3) == 0 ? 4 : (a & 1) == 0 ? 2 : 1;
}
int stitch_dev_bmp_decode_u8(const uint8_t* d_file, size_t n, const stitch_bmp_info* bi, uint8_t* d_planar, void* stream) {
    int rc = need_device();
    if (rc) return rc;
    if (!d_file || !bi || !d_planar) return fail(STITCH_ERR_ARG, "bmp_decode: null argument");
    if (bi->width <= 0 || bi->height <= 0 || (bi->bpp != 24 && bi->bpp != 32) || bi->stride < (uint64_t)bi->width * (bi->bpp / 8) ||
        (bi->stride & 3) || bi->data_pos > n || bi->data_bytes > n - bi->data_pos)
        return fail(STITCH_ERR_ARG, "bmp_decode: inconsistent stitch_bmp_info (use stitch_bmp_parse)");
    BmpGeom g{};
    g.w = bi->width;
    g.h = bi->height;
    g.bp = bi->bpp / 8;
    g.top_down = bi->top_down;
    g.data_pos = bi->data_pos;
    g.stride = bi->stride;
    g.data_bytes = bi->data_bytes;
    g.planar_vec = (g.w % 4 == 0) && (reinterpret_cast<uintptr_t>(d_planar) % 4 == 0);
    const dim3 grid((g.w + BMP_SEG - 1) / BMP_SEG, g.h);
    hipStream_t s = as_stream(stream);
    switch (bmp_align(d_file, g.data_pos)) {  // stride and a segment's byte offset are multiples of 4
        case 4: k_bmp_decode<4><<<grid, 256, 0, s>>>(d_file, g, d_planar); break;
        case 2: k_bmp_decode<2><<<grid, 256, 0, s>>>(d_file, g, d_planar); break;
        default: k_bmp_decode<1><<<grid, 256, 0, s>>>(d_file, g, d_planar); break;
    }
    return launch_check("k_bmp_decode");
}
int stitch_dev_bmp_encode_u8(const uint8_t* d_planar, int w, int h, uint8_t* d_file, size_t cap, void* stream) {
    int rc = need_device();
    if (rc) return rc;
    const size_t total = stitch_bmp_file_bytes(w, h);
    if (!d_planar || !d_file || !total) return fail(STITCH_ERR_ARG, "bmp_encode: bad argument");
    if (total > 0xffffffffULL) return fail(STITCH_ERR_ARG, "bmp_encode: %d x %d does not fit the format's 32-bit file size", w, h);
    if (cap < total) return fail(STITCH_ERR_ARG, "bmp_encode: buffer of %zu bytes, file needs %zu", cap, total);
    BmpGeom g{};
    g.w = w;
    g.h = h;
    g.bp = 3;
    g.stride = ((unsigned long long)3 * w + 3) & ~3ULL;
    g.planar_vec = (w % 4 == 0) && (reinterpret_cast<uintptr_t>(d_planar) % 4 == 0);
    BmpHeader hd{};  // CImg.h:52633-52664
    const unsigned buf_size = (unsigned)(total - 54), file_size = (unsigned)total;
    hd.b[0] = 'B';
    hd.b[1] = 'M';
    for (int i = 0; i < 4; ++i) {
        hd.b[0x02 + i] = (uint8_t)(file_size >> (8 * i));
        hd.b[0x12 + i] = (uint8_t)((unsigned)w >> (8 * i));
        hd.b[0x16 + i] = (uint8_t)((unsigned)h >> (8 * i));
        hd.b[0x22 + i] = (uint8_t)(buf_size >> (8 * i));
    }
    hd.b[0x0A] = 0x36;
    hd.b[0x0E] = 0x28;
    hd.b[0x1A] = 1;
    hd.b[0x1C] = 24;
    hd.b[0x27] = 0x1;
    hd.b[0x2B] = 0x1;
    const dim3 grid((unsigned)((g.stride + BMP_SEG * 3 - 1) / (BMP_SEG * 3)), h);
    hipStream_t s = as_stream(stream);
    switch (bmp_align(d_file, 54)) {
        case 4: k_bmp_encode<4><<<grid, 256, 0, s>>>(d_planar, g, hd, d_file); break;
        case 2: k_bmp_encode<2><<<grid, 256, 0, s>>>(d_planar, g, hd, d_file); break;
        default: k_bmp_encode<1><<<grid, 256, 0, s>>>(d_planar, g, hd, d_file); break;
    }
    return launch_check("k_bmp_encode");
}
int stitch_bmp_decode_u8(const uint8_t* file, size_t n, uint8_t* planar) {
    int rc = need_device();
    if (rc) return rc;
    stitch_bmp_info bi;
    if ((rc = stitch_bmp_parse(file, n, &bi))) return rc;
    if (!planar) return fail(STITCH_ERR_ARG, "bmp_decode: null output");
    const size_t out = (size_t)3 * bi.width * bi.height;
    DevBuf f, p;
    if ((rc = f.alloc(n)) || (rc = p.alloc(out))) return rc;
    HIPCHK(hipMemcpy(f.p, file, n, hipMemcpyHostToDevice));
    if ((rc = stitch_dev_bmp_decode_u8(f.as<uint8_t>(), n, &bi, p.as<uint8_t>(), nullptr))) return rc;
    HIPCHK(hipMemcpy(planar, p.p, out, hipMemcpyDeviceToHost));
    return STITCH_OK;
}
int stitch_bmp_encode_u8(const uint8_t* planar, int w, int h, uint8_t* file, size_t cap) {
    int rc = need_device();
    if (rc) return rc;
    const size_t total = stitch_bmp_file_bytes(w, h);
    if (!planar || !file || !total) return fail(STITCH_ERR_ARG, "bmp_encode: bad argument");
    if (cap < total) return fail(STITCH_ERR_ARG, "bmp_encode: buffer of %zu bytes, file needs %zu", cap, total);
    DevBuf f, p;
    if ((rc = f.alloc(total)) || (rc = p.alloc((size_t)3 * w * h))) return rc;
    HIPCHK(hipMemcpy(p.p, planar, (size_t)3 * w * h, hipMemcpyHostToDevice));
    if ((rc = stitch_dev_bmp_encode_u8(p.as<uint8_t>(), w, h, f.as<uint8_t>(), total, nullptr))) return rc;
    HIPCHK(hipMemcpy(file, f.p, total, hipMemcpyDeviceToHost));
    return STITCH_OK;
}
int stitch_dev_project_gray_u8(const uint8_t* d_src, int w, int h, float fov_deg, uint8_t* d_projected, uint8_t* d_gray,
                               float* d_gray_f32, void* stream) {
    return dev_project<uint8_t>(d_src, w, h, fov_deg, d_projected, stream, d_gray, d_gray_f32);
}
int stitch_gray_u8(const uint8_t* rgb, int w, int h, uint8_t* gray, float* gray_f32) {
    int rc = need_device();
    if (rc) return rc;
    if (!rgb || (!gray && !gray_f32) || w <= 0 || h <= 0) return fail(STITCH_ERR_ARG, "gray: bad argument");
    const size_t n = (size_t)w * h;
    DevBuf d, g, f;
    if ((rc = d.alloc(n * 3)) || (rc = g.alloc(n)) || (rc = f.alloc(n * sizeof(float)))) return rc;
    HIPCHK(hipMemcpy(d.p, rgb, n * 3, hipMemcpyHostToDevice));
    if ((rc = stitch_dev_gray_u8(d.as<uint8_t>(), w, h, g.as<uint8_t>(), f.as<float>(), nullptr))) return rc;
    if (gray) HIPCHK(hipMemcpy(gray, g.p, n, hipMemcpyDeviceToHost));
    if (gray_f32) HIPCHK(hipMemcpy(gray_f32, f.p, n * sizeof(float), hipMemcpyDeviceToHost));
    return STITCH_OK;
}
int stitch_project_gray_u8(const uint8_t* src, int w, int h, float fov_deg, uint8_t* projected, uint8_t* gray, float* gray_f32) {
    int rc = need_device();
    if (rc) return rc;
    if (!src || !projected || w <= 0 || h <= 0) return fail(STITCH_ERR_ARG, "project_gray: bad argument");
    const size_t n = (size_t)w * h;
    DevBuf s, d, g, f;
    if ((rc = s.alloc(n * 3)) || (rc = d.alloc(n * 3)) || (rc = g.alloc(n)) || (rc = f.alloc(n * sizeof(float)))) return rc;
    HIPCHK(hipMemcpy(s.p, src, n * 3, hipMemcpyHostToDevice));
    if ((rc = stitch_dev_project_gray_u8(s.as<uint8_t>(), w, h, fov_deg, d.as<uint8_t>(), g.as<uint8_t>(), f.as<float>(), nullptr)))
        return rc;
    HIPCHK(hipMemcpy(projected, d.p, n * 3, hipMemcpyDeviceToHost));
    if (gray) HIPCHK(hipMemcpy(gray, g.p, n, hipMemcpyDeviceToHost));
    if (gray_f32) HIPCHK(hipMemcpy(gray_f32, f.p, n * sizeof(float), hipMemcpyDeviceToHost));
    return STITCH_OK;
}

// Canvas sizing of one stitch step, ImageProcess.cpp:206-216 with getMin/MaxX/YAfterWarping (:532-594): float
// arithmetic exactly as written there (the map itself in double, rounded to float per corner).  Host only.
static float map_x(const double p[8], float x, float y) { return (float)(p[0] * (double)x + p[1] * (double)y + p[2] * (double)x * (double)y + p[3]); }
static float map_y(const double p[8], float x, float y) { return (float)(p[4] * (double)x + p[5] * (double)y + p[6] * (double)x * (double)y + p[7]); }
int stitch_canvas_bbox(int fw, int fh, const double p_fwd[8], int result_w, int result_h, float* min_x, float* min_y, int* new_w,
                       int* new_h) {
    if (!p_fwd || !min_x || !min_y || !new_w || !new_h || fw <= 0 || fh <= 0 || result_w <= 0 || result_h <= 0)
        return fail(STITCH_ERR_ARG, "canvas_bbox: bad argument");
    const float cx[4] = {0.f, (float)(fw - 1), 0.f, (float)(fw - 1)}, cy[4] = {0.f, 0.f, (float)(fh - 1), (float)(fh - 1)};
    float mnx = map_x(p_fwd, cx[0], cy[0]), mxx = mnx, mny = map_y(p_fwd, cx[0], cy[0]), mxy = mny;
    for (int i = 1; i < 4; ++i) {  // strict comparisons in the reference's corner order (0,0) (w-1,0) (0,h-1) (w-1,h-1)
        const float X = map_x(p_fwd, cx[i], cy[i]), Y = map_y(p_fwd, cx[i], cy[i]);
        if (X < mnx) mnx = X;
        if (X > mxx) mxx = X;
        if (Y < mny) mny = Y;
        if (Y > mxy) mxy = Y;
    }
    mnx = (mnx < 0) ? mnx : 0;                                  // :207
    mny = (mny < 0) ? mny : 0;                                  // :209
    mxx = (mxx >= (float)result_w) ? mxx : (float)result_w;    // :211
    mxy = (mxy >= (float)result_h) ? mxy : (float)result_h;    // :213
    *min_x = mnx;
    *min_y = mny;
    *new_w = (int)std::ceil(mxx - mnx);  // :215 (float subtraction)
    *new_h = (int)std::ceil(mxy - mny);
    return STITCH_OK;
}
int stitch_step_geometry(int fw, int fh, const double p_fwd[8], int mw, int mh, stitch_step_geom* g) {
    if (!g) return fail(STITCH_ERR_ARG, "step_geometry: null output");
    int rc = stitch_canvas_bbox(fw, fh, p_fwd, mw, mh, &g->min_x, &g->min_y, &g->cw, &g->ch);
    if (rc) return rc;
    g->ox = (int)g->min_x;  // movingImageByOffset(result, b, min_x, min_y): float arguments to int parameters (ImageProcess.cpp:224)
    g->oy = (int)g->min_y;
    if (g->cw <= 0 || g->ch <= 0) return fail(STITCH_ERR_ARG, "step_geometry: empty canvas %d x %d", g->cw, g->ch);
    return STITCH_OK;
}
int stitch_dev_step_u8(const uint8_t* d_frame, int fw, int fh, const double p_fwd[8], const double p_bwd[8], const uint8_t* d_mosaic, int mw,
                       int mh, const stitch_blend_opts* opts, uint8_t* d_out, size_t out_capacity, stitch_step_geom* geom_out,
                       stitch_seam* seam_out, void* stream) {
    return dev_step<uint8_t>(d_frame, fw, fh, p_fwd, p_bwd, d_mosaic, mw, mh, opts, d_out, out_capacity, geom_out, seam_out, stream);
}
int stitch_dev_step_f32(const float* d_frame, int fw, int fh, const double p_fwd[8], const double p_bwd[8], const float* d_mosaic, int mw, int mh,
                        const stitch_blend_opts* opts, float* d_out, size_t out_capacity, stitch_step_geom* geom_out, stitch_seam* seam_out,
                        void* stream) {
    return dev_step<float>(d_frame, fw, fh, p_fwd, p_bwd, d_mosaic, mw, mh, opts, d_out, out_capacity, geom_out, seam_out, stream);
}
// updateFeaturesByHomography / updateFeaturesByOffset, ImageProcess.cpp:622-640, on arrays of keypoint coordinates
int stitch_map_points(float* x, float* y, int32_t* ix, int32_t* iy, int n, const double p_fwd[8], float offx, float offy) {
    if (!x || !y || !p_fwd || n < 0) return fail(STITCH_ERR_ARG, "map_points: bad argument");
    for (int i = 0; i < n; ++i) {
        const float cx = x[i], cy = y[i];
        x[i] = map_x(p_fwd, cx, cy) - offx;
        y[i] = map_y(p_fwd, cx, cy) - offy;
        if (ix) ix[i] = (int32_t)x[i];
        if (iy) iy[i] = (int32_t)y[i];
    }
    return STITCH_OK;
}
int stitch_shift_points(float* x, float* y, int32_t* ix, int32_t* iy, int n, int ox, int oy) {
    if (!x || !y || n < 0) return fail(STITCH_ERR_ARG, "shift_points: bad argument");
    for (int i = 0; i < n; ++i) {
        x[i] -= (float)ox;
        y[i] -= (float)oy;
        if (ix) ix[i] = (int32_t)x[i];
        if (iy) iy[i] = (int32_t)y[i];
    }
    return STITCH_OK;
}

int stitch_dev_synth_u8(uint8_t* d_dst, int w, int h, int frame_id, void* stream) {
    int rc = need_device();
    if (rc) return rc;
    if (!d_dst || w <= 0 || h <= 0 || w >= (1 << 18) || h >= (1 << 18)) return fail(STITCH_ERR_ARG, "synth: bad argument");
    k_synth<uint8_t><<<grid_xy(w, h, 3), 256, 0, as_stream(stream)>>>(d_dst, w, h, frame_id);
    return launch_check("k_synth");
}
int stitch_dev_synth_f32(float* d_dst, int w, int h, int frame_id, void* stream) {
    int rc = need_device();
    if (rc) return rc;
    if (!d_dst || w <= 0 || h <= 0 || w >= (1 << 18) || h >= (1 << 18)) return fail(STITCH_ERR_ARG, "synth: bad argument");
    k_synth<float><<<grid_xy(w, h, 3), 256, 0, as_stream(stream)>>>(d_dst, w, h, frame_id);
    return launch_check("k_synth");
}
int stitch_dev_check_fastdiv(float w, unsigned long long* tested, unsigned long long* mismatches) {
    int rc = need_device();
    if (rc) return rc;
    if (!(w >= 2.0f && w < 16777216.0f) || w != std::floor(w) || !tested || !mismatches) return fail(STITCH_ERR_ARG, "check_fastdiv: w must be an integer value in [2, 2^24)");
    unsigned long long* d = nullptr;
    HIPCHK(hipMalloc((void**)&d, 2 * sizeof(unsigned long long)));
    HIPCHK(hipMemset(d, 0, 2 * sizeof(unsigned long long)));
    k_check_fastdiv<<<4096, 256>>>(w, d, d + 1);
    unsigned long long h[2] = {0, 0};
    const hipError_t e = hipMemcpy(h, d, sizeof h, hipMemcpyDeviceToHost);
    (void)hipFree(d);
    if (e != hipSuccess) return fail(STITCH_ERR_HIP, "check_fastdiv: %s", hipGetErrorString(e));
    *mismatches = h[0];
    *tested = h[1];
    return STITCH_OK;
}
int stitch_dev_check_collapse_taps(int w, int h, int probe, unsigned long long* compared, unsigned long long* mismatches) {
    int rc = need_device();
    if (rc) return rc;
    if (w < 256 || (w & 1) || h < 4 || (h & 1) || w > 16384 || h > 16384 || probe < 0 || probe > 1 || !compared || !mismatches)
        return fail(STITCH_ERR_ARG, "check_collapse_taps: even w >= 256, even h >= 4 (both <= 16384), probe 0 or 1");
    const int sw = w / 2, sh = h / 2, pitch = round_up(w, 64), spitch = round_up(sw, 64);
    const size_t ps = (size_t)pitch * h, sps = (size_t)spitch * sh;
    std::vector<int32_t> ix, iy;
    std::vector<double> ax, ay;
    expand_table(sw, w, ix, ax);
    expand_table(sh, h, iy, ay);
    int xa = 0, xb = 0, gxb = 0;
    regular_range(ix, w, sw, sh, &xa, &xb);
    general_range(ix, w, sw, sh, &gxb);
    if (gxb < 256) return fail(STITCH_ERR_ARG, "check_collapse_taps: no block of this width takes the four-column path");
    // level l: a, b and the mask; level l+1: G (a, b) and E.  probe 0: pseudo-random finite samples of both signs.  probe 1, the signed-zero
    // probe: G_l = -0, G_{l+1} = +0 (every Laplacian sample -0), E_{l+1} = -0 except the FIRST sample of every row = 5: a column whose first tap
    // is a row's last sample must come out -0 (the reference takes that sample twice: -0 + 0 * -0); had it taken the sample the 16-byte
    // window holds behind it (the next row's 5) the sum would be +0.
    std::vector<float> g(7 * ps + (size_t)pitch * 64, 0.f), gn(7 * sps + (size_t)spitch * 64, 0.f), en(3 * sps + (size_t)spitch * 64, 0.f);
    uint32_t lcg = 0x5717C4EDu ^ (uint32_t)(w * 31 + h);
    auto rnd = [&]() {
        lcg = lcg * 1664525u + 1013904223u;
        return ((int)(lcg >> 8) % 60001 - 30000) / 117.0f;
    };
    for (size_t q = 0; q < 7; ++q)
        for (int y = 0; y < h; ++y)
            for (int x = 0; x < w; ++x) g[q * ps + (size_t)y * pitch + x] = q == 6 ? (probe ? 0.5f : (float)((x * 7 + y * 3) % 11) / 10.f) : probe ? -0.0f : rnd();
    for (size_t q = 0; q < 7; ++q)
        for (int y = 0; y < sh; ++y)
            for (int x = 0; x < sw; ++x) gn[q * sps + (size_t)y * spitch + x] = probe ? 0.0f : rnd();
    for (size_t q = 0; q < 3; ++q)
        for (int y = 0; y < sh; ++y)
            for (int x = 0; x < spitch; ++x) en[q * sps + (size_t)y * spitch + x] = probe ? (x == 0 ? 5.0f : -0.0f) : (x < sw ? rnd() : 0.f);
    const size_t bytes[] = {g.size() * 4, gn.size() * 4, en.size() * 4, 3 * ps * 4, 3 * ps * 4, (size_t)w * 4, (size_t)w * 8, (size_t)h * 4, (size_t)h * 8};
    size_t off[10] = {0};
    for (int i = 0; i < 9; ++i) off[i + 1] = off[i] + align256(bytes[i]);
    char* base = nullptr;
    HIPCHK(hipMalloc((void**)&base, off[9] + 256));
    auto up = [&](int i, const void* src) { return hipMemcpy(base + off[i], src, bytes[i], hipMemcpyHostToDevice) == hipSuccess; };
    bool ok = up(0, g.data()) && up(1, gn.data()) && up(2, en.data()) && up(5, ix.data()) && up(6, ax.data()) && up(7, iy.data()) && up(8, ay.data()) &&
              hipMemset(base + off[3], 0xff, 2 * align256(bytes[3])) == hipSuccess;
    std::vector<float> o1(3 * ps), o2(3 * ps);
    if (ok) {
        const ExpandTab tb{(const int32_t*)(base + off[5]), (const double*)(base + off[6]), (const int32_t*)(base + off[7]), (const double*)(base + off[8])};
        const int crows = 8, strips = (h + crows - 1) / crows;
        for (int v = 0; v < 2; ++v) {  // v = 0: k_collapse4 with per-lane taps on [0, gxb), one column per work-item behind; v = 1: k_collapse everywhere
            OutPtrs<float> eo{};
            eo.p[0] = (float*)(base + off[3 + v]);
            CollapseArgs<float, false> A{(const float*)(base + off[0]), w, h, pitch, ps, (const float*)(base + off[1]), (const float*)(base + off[2]), sw, sh, spitch, sps,
                                         tb, eo, pitch, ps, nullptr, NoPairArgs{}, 0, crows, 0, v == 0 ? gxb : 0, 1, 0, 1};
            launch_collapse(A, CollapseKind{false, true, false, false, false}, pitch, strips, 1, MaskRowsArg{}, nullptr);
        }
        ok = hipDeviceSynchronize() == hipSuccess && hipMemcpy(o1.data(), base + off[3], bytes[3], hipMemcpyDeviceToHost) == hipSuccess &&
             hipMemcpy(o2.data(), base + off[4], bytes[4], hipMemcpyDeviceToHost) == hipSuccess;
    }
    const hipError_t e = ok ? hipSuccess : hipGetLastError();
    (void)hipFree(base);
    if (!ok) return fail(STITCH_ERR_HIP, "check_collapse_taps: %s", hipGetErrorString(e));
    unsigned long long n = 0, bad = 0;
    for (size_t q = 0; q < 3; ++q)
        for (int y = 0; y < h; ++y)
            for (int x = 0; x < w; ++x, ++n) {
                uint32_t a, b;
                std::memcpy(&a, &o1[q * ps + (size_t)y * pitch + x], 4);
                std::memcpy(&b, &o2[q * ps + (size_t)y * pitch + x], 4);
                bad += a != b;
            }
    *compared = n;
    *mismatches = bad;
    return STITCH_OK;
}
int stitch_dev_check_collapse_sides(int w, int h, int probe, int branch, int seam_x, unsigned long long* compared, unsigned long long* mismatches,
                                    int counts[3]) {
    int rc = need_device();
    if (rc) return rc;
    if (w < 256 || (w & 1) || h < 4 || (h & 1) || w > 16384 || h > 16384 || probe < 0 || probe > 1 || branch < 0 || branch > 1 || seam_x < 0 || seam_x > w ||
        !compared || !mismatches)
        return fail(STITCH_ERR_ARG, "check_collapse_sides: even w >= 256, even h >= 4 (both <= 16384), probe 0 or 1, branch 0 or 1, 0 <= seam_x <= w");
    const int sw = w / 2, sh = h / 2, pitch = round_up(w, 64), spitch = round_up(sw, 64);
    const size_t ps = (size_t)pitch * h, sps = (size_t)spitch * sh, ops = (size_t)w * h;
    std::vector<int32_t> ix, iy;
    std::vector<double> ax, ay;
    expand_table(sw, w, ix, ax);
    expand_table(sh, h, iy, ay);
    int gxb = 0;
    general_range(ix, w, sw, sh, &gxb);
    if (gxb < 256) return fail(STITCH_ERR_ARG, "check_collapse_sides: no block of this width takes the four-column path");
    // level 0: the six materialised planes of a and b (the mask plane is not read: the mask is the step); level 1: G (a, b) and E.
    // probe 0: pseudo-random finite samples of both signs.  probe 1, the signed-zero probe: G_1 = +0 and the level-0 samples +0 or -0 in
    // a pattern of their own per image, so every Laplacian term (sample - 0) is +0 or -0 and kept and dropped terms meet in all four sign
    // pairs; E_1 alternates, from sample to sample, -0, -1e-45 (the smallest denormal: its interpolation with a zero underflows to -0 or
    // stays a tiny negative) and +0, shifted by one per row.  blend_ref's zero takes its sign from the dropped term and keeps it through
    // the sum with an ee of -0: a one-sided form that does not redo those rows leaves wrong signs on both sides of the seam.
    std::vector<float> g(7 * ps + (size_t)pitch * 64, 0.f), gn(7 * sps + (size_t)spitch * 64, 0.f), en(3 * sps + (size_t)spitch * 64, 0.f);
    uint32_t lcg = 0x51DE5u ^ (uint32_t)(w * 31 + h);
    auto rnd = [&]() {
        lcg = lcg * 1664525u + 1013904223u;
        return ((int)(lcg >> 8) % 60001 - 30000) / 117.0f;
    };
    for (size_t q = 0; q < 6; ++q)
        for (int y = 0; y < h; ++y)
            for (int x = 0; x < w; ++x)
                g[q * ps + (size_t)y * pitch + x] = !probe ? rnd() : ((q < 3 ? (x + y + (int)q) % 3 : (x / 3 + y + (int)q) % 2) == 0 ? -0.0f : 0.0f);
    if (!probe)
        for (size_t q = 0; q < 6; ++q)
            for (int y = 0; y < sh; ++y)
                for (int x = 0; x < sw; ++x) gn[q * sps + (size_t)y * spitch + x] = rnd();
    for (size_t q = 0; q < 3; ++q)
        for (int y = 0; y < sh; ++y)
            for (int x = 0; x < sw; ++x) {
                const int k = (x + y + (int)q) % 3;
                en[q * sps + (size_t)y * spitch + x] = !probe ? rnd() : k == 0 ? -0.0f : k == 1 ? -1.401298464e-45f : 0.0f;
            }
    SeamDev sd{};
    sd.branch = branch, sd.start = seam_x, sd.thr = (double)seam_x;
    const size_t bytes[] = {g.size() * 4, gn.size() * 4, en.size() * 4, 3 * ops * 4, 3 * ops * 4, (size_t)w * 4, (size_t)w * 8, (size_t)h * 4, (size_t)h * 8, sizeof sd};
    size_t off[11] = {0};
    for (int i = 0; i < 10; ++i) off[i + 1] = off[i] + align256(bytes[i]);
    char* base = nullptr;
    HIPCHK(hipMalloc((void**)&base, off[10] + 256));
    auto up = [&](int i, const void* src) { return hipMemcpy(base + off[i], src, bytes[i], hipMemcpyHostToDevice) == hipSuccess; };
    bool ok = up(0, g.data()) && up(1, gn.data()) && up(2, en.data()) && up(5, ix.data()) && up(6, ax.data()) && up(7, iy.data()) && up(8, ay.data()) && up(9, &sd) &&
              hipMemset(base + off[3], 0xff, 2 * align256(bytes[3])) == hipSuccess;
    std::vector<float> o1(3 * ops), o2(3 * ops);
    int got[3] = {0, 0, 0};
    if (ok) {
        const ExpandTab tb{(const int32_t*)(base + off[5]), (const double*)(base + off[6]), (const int32_t*)(base + off[7]), (const double*)(base + off[8])};
        const int crows = 8, strips = (h + crows - 1) / crows;
        for (int v = 0; v < 2; ++v) {  // v = 0: k_collapse4 with per-lane taps on [0, gxb), one column per work-item behind; v = 1: k_collapse everywhere
            OutPtrs<float> eo{};
            eo.p[0] = (float*)(base + off[3 + v]);
            CollapseArgs<float, true> A{(const float*)(base + off[0]), w, h, pitch, ps, (const float*)(base + off[1]), (const float*)(base + off[2]), sw, sh, spitch, sps,
                                        tb, eo, w, ops, (const SeamDev*)(base + off[9]), PairArgs<float>{}, 0, crows, 0, v == 0 ? gxb : 0, 1, 0, 1};
            launch_collapse(A, CollapseKind{false, true, false, false, false}, w, strips, 1, MaskRowsArg{}, nullptr);
            if (v == 0) {
#ifdef STITCH_NO_C4_SIDES
                c4_side_counts(sd.branch, sd.start, sd.thr, A.xa, A.xb, 0, got);
#else
                c4_side_counts(sd.branch, sd.start, sd.thr, A.xa, A.xb, 1, got);
#endif
            }
        }
        ok = hipDeviceSynchronize() == hipSuccess && hipMemcpy(o1.data(), base + off[3], bytes[3], hipMemcpyDeviceToHost) == hipSuccess &&
             hipMemcpy(o2.data(), base + off[4], bytes[4], hipMemcpyDeviceToHost) == hipSuccess;
    }
    const hipError_t e = ok ? hipSuccess : hipGetLastError();
    (void)hipFree(base);
    if (!ok) return fail(STITCH_ERR_HIP, "check_collapse_sides: %s", hipGetErrorString(e));
    *compared = (unsigned long long)o1.size();
    *mismatches = 0;
    for (size_t i = 0; i < o1.size(); ++i) {
        uint32_t a, b;
        std::memcpy(&a, &o1[i], 4);
        std::memcpy(&b, &o2[i], 4);
        *mismatches += a != b;
    }
    if (counts) counts[0] = got[0], counts[1] = got[1], counts[2] = got[2];
    return STITCH_OK;
}
int stitch_dev_quantize_u8(const float* d_src, uint8_t* d_dst, size_t n, void* stream) {
    int rc = need_device();
    if (rc) return rc;
    if (!d_src || !d_dst || n == 0) return fail(STITCH_ERR_ARG, "quantize: bad argument");
    k_quantize<<<eq_grid((n + 3) / 4), 256, 0, as_stream(stream)>>>(d_src, d_dst, n);
    return launch_check("k_quantize");
}

}  // extern "C"

#include "stitch_band.inc"
#include "stitch_match.inc"
#include "stitch_ransac.inc"
#include "stitch_sift.inc"
#include "stitch_chain.inc"
#include "stitch_panorama.inc"
#include "stitch_rig.inc"
#include "stitch_exposure.inc"
#include "stitch_rig_exposure.inc"
#include "stitch_calibrate.inc"
#include "stitch_rig_seams.inc"
#include "stitch_rig_crop.inc"
#include "stitch_rig_formats.inc"
#include "stitch_rig_monitor.inc"
#include "stitch_seam_path.inc"
#include "stitch_rig_seam_paths.inc"
#include "stitch_rig_scale.inc"
