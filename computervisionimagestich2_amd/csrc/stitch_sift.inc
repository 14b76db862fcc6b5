// stitch_sift.inc -- host side of the SIFT extraction (include/stitch.h, "SIFT"; kernels in k_sift.inc).
// Included at the end of stitch_hip.hip (one translation unit).
//
// A launch sequence covers up to SIFT_MAXFRAMES frames, which may differ in size: every grid is sized for the largest frame and
// a workgroup outside its own frame's extent returns.  Per octave: the hand-over (k_sift_down), two k_sift_conv per smoothed
// level, k_sift_detect / _scan / _emit, k_sift_grad, k_sift_orient, k_sift_fscan, k_sift_desc -- with 2 levels 15 launches for
// an octave after the first; octave 0 has no hand-over but two more k_sift_conv for the adjustment of level s_min: 16.
// Keypoint and feature counts stay on the device (the per-frame header); scratch is stream-ordered; nothing here waits.
namespace {

static_assert(sizeof(SiftKeypoint) == sizeof(StitchSiftKeypoint), "keypoint record");
constexpr int kSiftMaxDim = 16384;
constexpr int kSiftWaveGrid = 2048;  // workgroups of k_sift_orient / k_sift_desc at most (one wavefront each, keypoints strided)

// The filters depend on the number of levels only: built once per S and kept (first[k] / next[k]: the filter of sd_first[k] /
// sd_next[k]; W = 0 where the schedule has no smoothing, -1 where the filter would be wider than the kernel's tile allows).
// An equal sigma reuses the previous filter, as _vl_sift_smooth does.
struct SiftFilters {
    SiftPlan plan;
    SiftTaps first[8], next[8];
};
const SiftFilters& sift_filters(int S) {
    static std::mutex mu;
    static SiftFilters cache[6];
    static bool have[6] = {false, false, false, false, false, false};
    std::lock_guard<std::mutex> lock(mu);
    SiftFilters& f = cache[S];
    if (!have[S]) {
        f.plan = sift_plan(S);
        double last_sd = 0;
        const SiftTaps* last = nullptr;
        for (int pass = 0; pass < 2; ++pass)
            for (int k = 0; k <= S + 2; ++k) {
                const double sd = pass ? f.plan.sd_next[k] : f.plan.sd_first[k];
                SiftTaps& t = pass ? f.next[k] : f.first[k];
                if (!(sd > 0)) {
                    t.W = 0;
                } else if (last && sd == last_sd) {
                    t = *last;
                } else {
                    t.W = sift_make_taps(sd, t.c);
                    last_sd = sd;
                    last = &t;
                }
            }
        have[S] = true;
    }
    return f;
}

struct SiftCfg {
    StitchSiftOpts o;
    const SiftFilters* filt;
};

int sift_cfg(const StitchSiftOpts* opts, SiftCfg* c) {
    const StitchSiftOpts def = STITCH_SIFT_OPTS_DEFAULT;
    c->o = opts ? *opts : def;
    if (c->o.first_octave != 0) return fail(STITCH_ERR_ARG, "sift: first_octave = %d (only 0 is supported)", c->o.first_octave);
    if (c->o.levels < 1 || c->o.levels > 5) return fail(STITCH_ERR_ARG, "sift: levels = %d (1 .. 5)", c->o.levels);
    if (c->o.octaves > 16) return fail(STITCH_ERR_ARG, "sift: octaves = %d (at most 16)", c->o.octaves);
    for (double v : {c->o.peak_thresh, c->o.edge_thresh, c->o.norm_thresh, c->o.magnif, c->o.window_size})
        if (!std::isfinite(v)) return fail(STITCH_ERR_ARG, "sift: an option is not finite");
    if (!(c->o.magnif > 0) || !(c->o.window_size > 0) || !(c->o.edge_thresh > 0))
        return fail(STITCH_ERR_ARG, "sift: magnif, window_size and edge_thresh must be positive");
    c->filt = &sift_filters(c->o.levels);
    return STITCH_OK;
}

int sift_check(const stitch_sift_desc& d, int i) {
    if (!d.image || d.width < 1 || d.height < 1 || d.width > kSiftMaxDim || d.height > kSiftMaxDim)
        return fail(STITCH_ERR_ARG, "sift: frame %d is %d x %d (1 .. %d)", i, d.width, d.height, kSiftMaxDim);
    if (d.pitch < d.width * (d.is_f32 ? 4 : 1)) return fail(STITCH_ERR_ARG, "sift: frame %d has pitch %d", i, d.pitch);
    if (d.kp_cap < 0 || d.feat_cap < 0 || !d.counts || !d.status) return fail(STITCH_ERR_ARG, "sift: frame %d lacks counts / status or has a negative capacity", i);
    if ((d.kp_cap && !d.keypoints) || (d.feat_cap && (!d.feat_kp || !d.feat_angle || !d.feat_desc)))
        return fail(STITCH_ERR_ARG, "sift: frame %d lacks an output buffer", i);
    return STITCH_OK;
}

int sift_octaves(const stitch_sift_desc& d, const SiftCfg& c) {
    return c.o.octaves < 0 ? sift_auto_octaves(d.width, d.height) : c.o.octaves;
}

int sift_smooth(SiftArgs& a, int n, int src, int dst, const SiftTaps& t, int max_w, int max_h, hipStream_t s) {
    if (t.W < 0) return fail(STITCH_ERR_ARG, "sift: a filter of the schedule is wider than %d taps", 2 * SIFT_MAXHALF + 1);
    a.src_lvl = src;
    a.dst_lvl = dst;
    int rc;
    a.pass = 0;
    k_sift_conv<<<dim3((max_w + SIFT_CONV_TX - 1) / SIFT_CONV_TX, (max_h + SIFT_CONV_TY - 1) / SIFT_CONV_TY, n), SIFT_T, 0, s>>>(a, t);
    if ((rc = launch_check("k_sift_conv"))) return rc;
    a.pass = 1;
    k_sift_conv<<<dim3((max_h + SIFT_CONV_TX - 1) / SIFT_CONV_TX, (max_w + SIFT_CONV_TY - 1) / SIFT_CONV_TY, n), SIFT_T, 0, s>>>(a, t);
    return launch_check("k_sift_conv");
}

int sift_enqueue(const stitch_sift_desc* d, int n, const SiftCfg& c, char* scratch, hipStream_t s);

int sift_launch(const stitch_sift_desc* d, int n, const SiftCfg& c, hipStream_t s) {
    const int S = c.o.levels;
    size_t bytes = align256(258 * sizeof(double));
    for (int i = 0; i < n; ++i) {
        const size_t ls = (size_t)d[i].width * d[i].height, words = (ls * S + SIFT_T - 1) / SIFT_T * (SIFT_T / 64), k = (size_t)d[i].kp_cap;
        bytes += align256(ls * (S + 3) * 4) + align256(ls * 4) + align256(ls * 2 * S * 4) + align256(words * 8) + align256(words * 4) +
                 align256(SIFT_H_N * 4) + 2 * align256(k * 4 + 4) + align256(k * 4 * 8 + 8);
    }
    char* scratch = nullptr;
    keep_pool_memory();
    HIPCHK(hipMallocAsync((void**)&scratch, bytes, s));
    const int rc = sift_enqueue(d, n, c, scratch, s);
    const hipError_t e = hipFreeAsync(scratch, s);  // on the error path too
    if (rc) return rc;
    if (e != hipSuccess) return fail(STITCH_ERR_HIP, "hipFreeAsync failed: %s", hipGetErrorString(e));
    return STITCH_OK;
}

int sift_enqueue(const stitch_sift_desc* d, int n, const SiftCfg& c, char* scratch, hipStream_t s) {
    const int S = c.o.levels;
    int max_oct = 0;
    for (int i = 0; i < n; ++i) max_oct = std::max(max_oct, sift_octaves(d[i], c));
    size_t off = 0;
    auto take = [&](size_t b) {
        char* p = scratch + off;
        off += align256(b);
        return p;
    };
    SiftArgs all;
    std::memset(&all, 0, sizeof all);
    double* tab = reinterpret_cast<double*>(take(258 * sizeof(double)));
    all.expn = tab;
    all.S = S;
    all.tp = c.o.peak_thresh;
    all.te_bound = (c.o.edge_thresh + 1) * (c.o.edge_thresh + 1) / c.o.edge_thresh;
    all.norm_thresh = c.o.norm_thresh;
    all.magnif = c.o.magnif;
    all.sigma0 = c.filt->plan.sigma0;
    all.wsigma = (float)c.o.window_size;
    int noct[SIFT_MAXFRAMES];
    for (int i = 0; i < n; ++i) {
        SiftFrame& f = all.f[i];
        const size_t ls = (size_t)d[i].width * d[i].height, words = (ls * S + SIFT_T - 1) / SIFT_T * (SIFT_T / 64), k = (size_t)d[i].kp_cap;
        f.img = d[i].image;
        f.w = d[i].width;
        f.h = d[i].height;
        f.pitch = d[i].pitch;
        f.is_f32 = d[i].is_f32 != 0;
        f.lstride = ls;
        f.oct = reinterpret_cast<float*>(take(ls * (S + 3) * 4));
        f.tmp = reinterpret_cast<float*>(take(ls * 4));
        f.grad = reinterpret_cast<float*>(take(ls * 2 * S * 4));
        f.mask = reinterpret_cast<unsigned long long*>(take(words * 8));
        f.woff = reinterpret_cast<int32_t*>(take(words * 4));
        f.hdr = reinterpret_cast<int32_t*>(take(SIFT_H_N * 4));
        f.nang = reinterpret_cast<int32_t*>(take(k * 4 + 4));
        f.foff = reinterpret_cast<int32_t*>(take(k * 4 + 4));
        f.ang = reinterpret_cast<double*>(take(k * 4 * 8 + 8));
        f.kp = reinterpret_cast<SiftKeypoint*>(d[i].keypoints);
        f.f_kp = d[i].feat_kp;
        f.f_angle = d[i].feat_angle;
        f.f_desc = d[i].feat_desc;
        f.counts = d[i].counts;
        f.status = d[i].status;
        f.kp_cap = d[i].kp_cap;
        f.feat_cap = d[i].feat_cap;
        noct[i] = sift_octaves(d[i], c);
    }
    int rc = STITCH_OK;
    int max_w = 0, max_h = 0;
    for (int i = 0; i < n; ++i) {
        max_w = std::max(max_w, d[i].width);
        max_h = std::max(max_h, d[i].height);
    }
    k_sift_table<<<1, 320, 0, s>>>(tab);
    if ((rc = launch_check("k_sift_table"))) return rc;
    k_sift_load<<<dim3((max_w + 63) / 64, (max_h + 3) / 4, n), SIFT_T, 0, s>>>(all);
    if ((rc = launch_check("k_sift_load"))) return rc;
    for (int o = 0; o < max_oct; ++o) {
        // the frames that have this octave (an octave of no pixels has nothing to find: the reference walks an empty plane)
        SiftArgs a = all;
        int m = 0, ow = 0, oh = 0, kcap = 0;
        size_t npos = 0;
        for (int i = 0; i < n; ++i)
            if (o < noct[i] && (all.f[i].w >> o) >= 1 && (all.f[i].h >> o) >= 1) {
                a.f[m++] = all.f[i];
                ow = std::max(ow, all.f[i].w >> o);
                oh = std::max(oh, all.f[i].h >> o);
                kcap = std::max(kcap, all.f[i].kp_cap);
                npos = std::max(npos, (size_t)(all.f[i].w >> o) * (all.f[i].h >> o) * S);
            }
        if (!m) break;
        a.o = o;
        const SiftTaps* taps = o ? c.filt->next : c.filt->first;
        if (o) {
            a.src_lvl = std::min(S, S + 2);  // level min(s_min + S, s_max) - s_min
            k_sift_down<<<dim3((ow + 63) / 64, (oh + 3) / 4, m), SIFT_T, 0, s>>>(a);
            if ((rc = launch_check("k_sift_down"))) return rc;
        }
        if (taps[0].W != 0 && (rc = sift_smooth(a, m, 0, 0, taps[0], ow, oh, s))) return rc;
        for (int l = 1; l <= S + 2; ++l)
            if ((rc = sift_smooth(a, m, l - 1, l, taps[l], ow, oh, s))) return rc;
        const unsigned pblocks = (unsigned)((npos + SIFT_T - 1) / SIFT_T);
        k_sift_detect<<<dim3(pblocks, m), SIFT_T, 0, s>>>(a);
        if ((rc = launch_check("k_sift_detect"))) return rc;
        k_sift_scan<<<m, SIFT_SCAN_T, 0, s>>>(a);
        if ((rc = launch_check("k_sift_scan"))) return rc;
        k_sift_emit<<<dim3(pblocks, m), SIFT_T, 0, s>>>(a);
        if ((rc = launch_check("k_sift_emit"))) return rc;
        k_sift_grad<<<dim3((ow + 63) / 64, (oh + 3) / 4, m), SIFT_T, 0, s>>>(a);
        if ((rc = launch_check("k_sift_grad"))) return rc;
        const unsigned wgrid = (unsigned)std::max(1, std::min(kcap, kSiftWaveGrid));
        k_sift_orient<<<dim3(wgrid, m), WAVE, 0, s>>>(a);
        if ((rc = launch_check("k_sift_orient"))) return rc;
        k_sift_fscan<<<m, SIFT_SCAN_T, 0, s>>>(a);
        if ((rc = launch_check("k_sift_fscan"))) return rc;
        k_sift_desc<<<dim3(wgrid, m), WAVE, 0, s>>>(a);
        if ((rc = launch_check("k_sift_desc"))) return rc;
    }
    k_sift_finish<<<n, WAVE, 0, s>>>(all);
    return launch_check("k_sift_finish");
}

}  // namespace

extern "C" {

int stitch_dev_sift_many(const stitch_sift_desc* frames, int n, const StitchSiftOpts* opts, void* stream) {
    int rc = need_device();
    if (rc) return rc;
    if (n < 0 || (n > 0 && !frames)) return fail(STITCH_ERR_ARG, "sift: bad list of frames (n = %d)", n);
    SiftCfg c;
    if ((rc = sift_cfg(opts, &c))) return rc;
    for (int i = 0; i < n; ++i)
        if ((rc = sift_check(frames[i], i))) return rc;
    for (int i = 0; i < n; i += SIFT_MAXFRAMES)
        if ((rc = sift_launch(frames + i, std::min(SIFT_MAXFRAMES, n - i), c, as_stream(stream)))) return rc;
    return STITCH_OK;
}

int stitch_sift(const uint8_t* gray, int width, int height, const StitchSiftOpts* opts, StitchSiftKeypoint* keypoints, int kp_cap,
                int32_t* feat_kp, double* feat_angle, float* feat_desc, int feat_cap, int32_t counts[2],
                int32_t status[STITCH_SIFT_STATUS]) {
    int rc = need_device();
    if (rc) return rc;
    if (!gray || width < 1 || height < 1 || kp_cap < 0 || feat_cap < 0 || !counts || !status) return fail(STITCH_ERR_ARG, "sift: bad argument");
    const size_t k = (size_t)kp_cap, m = (size_t)feat_cap;
    DevBuf img, dk, fk, fa, fd, cs;
    if ((rc = img.alloc((size_t)width * height)) || (rc = dk.alloc(k * sizeof(StitchSiftKeypoint) + 8)) || (rc = fk.alloc(m * 4 + 8)) ||
        (rc = fa.alloc(m * 8 + 8)) || (rc = fd.alloc(m * STITCH_DESCRIPTOR_DIM * 4 + 8)) || (rc = cs.alloc(8 * sizeof(int32_t))))
        return rc;
    HIPCHK(hipMemcpy(img.p, gray, (size_t)width * height, hipMemcpyHostToDevice));
    stitch_sift_desc d;
    std::memset(&d, 0, sizeof d);
    d.image = img.p;
    d.width = width;
    d.height = height;
    d.pitch = width;
    d.keypoints = dk.as<StitchSiftKeypoint>();
    d.kp_cap = kp_cap;
    d.feat_cap = feat_cap;
    d.feat_kp = fk.as<int32_t>();
    d.feat_angle = fa.as<double>();
    d.feat_desc = fd.as<float>();
    d.counts = cs.as<int32_t>();
    d.status = cs.as<int32_t>() + 2;
    if ((rc = stitch_dev_sift_many(&d, 1, opts, nullptr))) return rc;
    int32_t h[6];
    HIPCHK(hipMemcpy(h, cs.p, sizeof h, hipMemcpyDeviceToHost));
    counts[0] = h[0];
    counts[1] = h[1];
    for (int i = 0; i < STITCH_SIFT_STATUS; ++i) status[i] = h[2 + i];
    if (h[0] && keypoints) HIPCHK(hipMemcpy(keypoints, dk.p, (size_t)h[0] * sizeof(StitchSiftKeypoint), hipMemcpyDeviceToHost));
    if (h[1]) {
        HIPCHK(hipMemcpy(feat_kp, fk.p, (size_t)h[1] * 4, hipMemcpyDeviceToHost));
        HIPCHK(hipMemcpy(feat_angle, fa.p, (size_t)h[1] * 8, hipMemcpyDeviceToHost));
        HIPCHK(hipMemcpy(feat_desc, fd.p, (size_t)h[1] * STITCH_DESCRIPTOR_DIM * 4, hipMemcpyDeviceToHost));
    }
    return STITCH_OK;
}

int stitch_sift_filter(double sigma, float* taps) { return sift_make_taps(sigma, taps); }

void stitch_sift_expn_table(double* tab257) {
    for (int k = 0; k < 257; ++k) tab257[k] = sift_expn_entry(k);
}

void stitch_sift_elem(double x, double out[4]) {
    out[0] = stitch_sift_exp(x);
    out[1] = stitch_sift_exp2(x);
    stitch_sift_sincos(x, &out[2], &out[3]);
}

}  // extern "C"
