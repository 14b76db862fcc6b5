// stitch_calibrate.inc -- a rig calibrated from several captures (include/stitch_calibrate.h; kernels in k_calibrate.inc).
// Included at the end of stitch_hip.hip (one translation unit).
//
// The chain restates pipeline.py's calibrate_from_sets on top of the C entry points of the stages.  It is the whole-panorama
// chain (stitch_panorama.inc) over n_sets captures, without a pixel of the mosaic: no stitch step, no transfer, no finish pass;
// the SIFT front end, the all-pairs matching and a step's two estimations are the same code (stitch_chain.inc).  Per call the
// host waits as often as the whole-panorama chain does, whatever n_sets is: (1) the SIFT heads of all frames, then the descriptor
// rows written, for the std::map order; (2) the per-capture and pooled match counts, for the stitch order; (3) per step the two
// maps, their info rows and the step's support.  What changes against one capture: a camera's key points of all captures lie in
// one array (capture k's rows from base[k][camera] on), so one k_map_points / k_shift_points launch moves them all, and
// k_pool_select builds the step's list over those arrays from the captures' matcher lists.
struct stitch_calibration {
    int n_sets = 0, n = 0, start = 0, w = 0, h = 0;
    std::vector<int32_t> wh;       // n (width, height) pairs
    std::vector<stitch_panorama_step> steps;
    std::vector<int32_t> counts;   // n_sets matrices of n x n, then the pooled one
    std::vector<int32_t> support;  // per step and capture: {pairs in the chosen list, inliers of the forward map}
};

namespace {

struct CalCfg {
    PanoCfg c;
    int threshold;  // of the pooled counts
};

// Everything that can be refused without a device: the limits, the options.  *out is cleared first.
int cal_check(int n_sets, int n, const stitch_calibrate_opts* opts, stitch_calibration** out, CalCfg* cfg) {
    if (out) *out = nullptr;
    if (!out) return fail(STITCH_ERR_ARG, "calibrate: null argument");
    if (n < 1 || n > kPanoMaxFrames) return fail(STITCH_ERR_ARG, "calibrate: %d cameras (1 .. %d)", n, kPanoMaxFrames);
    if (n_sets < 1 || n_sets > STITCH_CALIBRATE_MAX_SETS) return fail(STITCH_ERR_ARG, "calibrate: %d captures (1 .. %d)", n_sets, STITCH_CALIBRATE_MAX_SETS);
    if (n_sets * n > STITCH_CALIBRATE_MAX_FRAMES)
        return fail(STITCH_ERR_ARG, "calibrate: %d captures of %d cameras are %d frames (at most %d)", n_sets, n, n_sets * n, STITCH_CALIBRATE_MAX_FRAMES);
    int rc = pano_cfg(opts ? opts->pano : nullptr, nullptr, &cfg->c);
    if (rc) return rc;
    const int pt = opts ? opts->pooled_threshold : 0;
    if (pt < 0) return fail(STITCH_ERR_ARG, "calibrate: pooled_threshold = %d", pt);
    if (!pt && (long long)n_sets * cfg->c.o.match_threshold > 0x7fffffffLL) return fail(STITCH_ERR_ARG, "calibrate: n_sets * match_threshold overflows int");
    cfg->threshold = pt ? pt : n_sets * cfg->c.o.match_threshold;
    return STITCH_OK;
}

// Camera i has one decoded size in every capture; wh receives it.
int cal_check_frames(const stitch_frame_u8* frames, int n_sets, int n, std::vector<int32_t>* wh) {
    if (!frames) return fail(STITCH_ERR_ARG, "calibrate: no frames");
    for (int k = 0; k < n_sets; ++k)
        for (int i = 0; i < n; ++i) {
            const stitch_frame_u8& f = frames[(size_t)k * n + i];
            if (!f.data || f.width <= 0 || f.height <= 0)
                return fail(STITCH_ERR_ARG, "calibrate: capture %d camera %d has no data or a bad size %d x %d", k, i, f.width, f.height);
            if (k == 0) {
                wh->push_back(f.width);
                wh->push_back(f.height);
            } else if (f.width != (*wh)[2 * i] || f.height != (*wh)[2 * i + 1]) {
                return fail(STITCH_ERR_ARG, "calibrate: capture %d camera %d is %d x %d, in capture 0 it is %d x %d", k, i, f.width, f.height, (*wh)[2 * i],
                            (*wh)[2 * i + 1]);
            }
        }
    return STITCH_OK;
}

// Per camera the rows of all captures and per frame its base in the camera's pooled arrays.
int cal_bases(const std::vector<int>& rows, int n_sets, int n, std::vector<int>* base, std::vector<int>* total) {
    base->assign((size_t)n_sets * n, 0);
    total->assign((size_t)n, 0);
    for (int i = 0; i < n; ++i) {
        long long at = 0;
        for (int k = 0; k < n_sets; ++k) {
            (*base)[(size_t)k * n + i] = (int)at;
            at += rows[(size_t)k * n + i];
            if (at > 0x3fffffffLL) return fail(STITCH_ERR_CAPACITY, "calibrate: camera %d has more than 2^30 feature rows over the captures", i);
        }
        (*total)[i] = (int)at;
    }
    return STITCH_OK;
}

// Everything from the ordered features on: counts, pooled counts, order, steps.  feats: n_sets * n sets, capture-major (only
// d_desc and n are read); X / Y: per camera this call's pooled arrays (NULL for a camera without a row), updated in place.
int cal_steps(const stitch_feature_set* feats, const std::vector<float*>& X, const std::vector<float*>& Y, const std::vector<int>& base,
              const std::vector<int>& total, const CalCfg& c, PanoArena& A, hipStream_t s, stitch_calibration* K) {
    const int n_sets = K->n_sets, n = K->n, nn = n * n;
    int rc = STITCH_OK;
    auto F = [&](int k, int i) -> const stitch_feature_set& { return feats[(size_t)k * n + i]; };
    // ---- every capture's ordered pairs in one matcher call; one more count matrix for the pooled counts ----
    PairLists L;
    if ((rc = chain_match_all(feats, n_sets, n, c.c.o.ratio, 1, A, s, &L))) return rc;
    k_pool_counts<<<(unsigned)std::min((nn + 255) / 256, 64), 256, 0, s>>>(L.d_counts, n_sets, nn, L.d_counts + (size_t)n_sets * nn);
    if ((rc = launch_check("k_pool_counts"))) return rc;
    // ---- read-back 2: the counts of every capture and the pooled ones, in one copy ----
    K->counts.assign((size_t)(n_sets + 1) * nn, 0);
    HIPCHK(hipMemcpyAsync(K->counts.data(), L.d_counts, L.count_bytes, hipMemcpyDeviceToHost, s));
    if ((rc = pano_sync(s))) return rc;
    const int32_t* pooled = K->counts.data() + (size_t)n_sets * nn;
    std::vector<int32_t> order((size_t)2 * n * std::max(n - 1, 1));
    int start = 0, n_steps = 0;
    if ((rc = stitch_stitch_order(pooled, n, c.threshold, &start, order.data(), &n_steps))) return rc;
    K->start = start;
    int rw = K->wh[2 * start], rh = K->wh[2 * start + 1];  // the projection keeps a frame's size
    K->w = rw;
    K->h = rh;
    if (!n_steps) return STITCH_OK;

    // ---- the captures' shares of every step, uploaded once ----
    std::vector<PoolSeg> seg((size_t)n_steps * n_sets);
    for (int t = 0; t < n_steps; ++t) {
        const int src = order[2 * t], dst = order[2 * t + 1];
        for (int k = 0; k < n_sets; ++k)
            seg[(size_t)t * n_sets + k] = PoolSeg{L.list_of(k, src, dst), L.count_of(k, src, dst), L.list_of(k, dst, src), L.count_of(k, dst, src),
                                                 F(k, dst).n,            F(k, src).n,             base[(size_t)k * n + src], base[(size_t)k * n + dst]};
    }
    int max_n = 1;
    for (int i = 0; i < n; ++i) max_n = std::max(max_n, total[i]);
    PoolSeg* d_seg = nullptr;
    int32_t *d_sel = nullptr, *d_inl = nullptr;
    StepBlock B;  // behind it: per capture 2 int32 of support (read back with the step), then n_sets + 1 offsets
    const size_t back_bytes = StepBlock::kHead + sizeof(int32_t) * 2 * n_sets;
    if ((rc = A.take(&d_seg, sizeof(PoolSeg) * seg.size())) || (rc = A.take(&d_sel, sizeof(int32_t) * 2 * max_n)) || (rc = A.take(&d_inl, sizeof(int32_t) * max_n)) ||
        (rc = A.take(&B.d, back_bytes + sizeof(int32_t) * (n_sets + 1))))
        return rc;
    int32_t *d_support = B.behind(), *d_seg_off = d_support + 2 * n_sets;
    PanoWait seg_in_use{s};  // `seg` is read by its upload
    HIPCHK(hipMemcpyAsync(d_seg, seg.data(), sizeof(PoolSeg) * seg.size(), hipMemcpyHostToDevice, s));

    std::vector<unsigned char> got(back_bytes);
    int pre = start;
    for (int t = 0; t < n_steps; ++t) {
        const int src = order[2 * t], dst = order[2 * t + 1];
        const int32_t t_sd = pooled[(size_t)src * n + dst], t_ds = pooled[(size_t)dst * n + src], chosen = t_sd > t_ds ? t_sd : t_ds;
        if (chosen > STITCH_CALIBRATE_MAX_PAIRS)
            return fail(STITCH_ERR_CAPACITY, "cameras %d -> %d: the pooled list has %d pairs (at most %d)", src, dst, chosen, STITCH_CALIBRATE_MAX_PAIRS);
        const int cap = std::max(std::max(total[src], total[dst]), 1);
        k_pool_select<<<(unsigned)std::min((cap + 255) / 256, 64), 256, 0, s>>>(d_seg + (size_t)t * n_sets, n_sets, cap, d_sel, B.sel_count(), d_seg_off);
        if ((rc = launch_check("k_pool_select"))) return rc;
        if ((rc = chain_step_fit(X[src], Y[src], X[dst], Y[dst], d_sel, B.sel_count(), cap, c.c.o.ransac, B.p16(), B.info10(), d_inl, s))) return rc;
        k_step_support<<<1, WAVE, 0, s>>>(d_inl, cap, B.info10(), d_seg_off, n_sets, d_support);
        if ((rc = launch_check("k_step_support"))) return rc;
        // ---- read-back 3: 16 doubles, 10 ints and the support ----
        stitch_panorama_step st;
        bool ok = false;
        if ((rc = chain_step_read(B, back_bytes, src, dst, s, got.data(), &st, &ok))) return rc;
        if (!ok)
            return fail(STITCH_ERR_NO_MAP, "cameras %d -> %d: no map (RANSAC status %d / %d, %d pooled pairs)", src, dst, st.info[0][0], st.info[1][0], st.info[0][1]);
        if ((rc = stitch_step_geometry(K->wh[2 * dst], K->wh[2 * dst + 1], st.p_fwd, rw, rh, &st.geom))) return rc;
        // :226-227 for every capture at once
        if ((rc = stitch_dev_map_points(X[dst], Y[dst], nullptr, nullptr, total[dst], st.p_fwd, st.geom.min_x, st.geom.min_y, s))) return rc;
        if ((rc = stitch_dev_shift_points(X[pre], Y[pre], nullptr, nullptr, total[pre], st.geom.ox, st.geom.oy, s))) return rc;
        pre = dst;
        rw = st.geom.cw;
        rh = st.geom.ch;
        K->steps.push_back(st);
        const int32_t* sup = reinterpret_cast<const int32_t*>(got.data() + StepBlock::kHead);
        K->support.insert(K->support.end(), sup, sup + 2 * n_sets);
    }
    K->w = rw;
    K->h = rh;
    return STITCH_OK;
}

std::unique_ptr<stitch_calibration> cal_new(int n_sets, int n, const std::vector<int32_t>& wh) {
    std::unique_ptr<stitch_calibration> K(new stitch_calibration());
    K->n_sets = n_sets;
    K->n = n;
    K->wh = wh;
    return K;
}

int cal_from_frames(const stitch_frame_u8* frames, int n_sets, int n, const std::vector<int32_t>& wh, const CalCfg& c, void* stream,
                    stitch_calibration** out) {
    const int nf = n_sets * n;
    hipStream_t s = as_stream(stream);
    PanoArena A(s);
    std::unique_ptr<stitch_calibration> K = cal_new(n_sets, n, wh);
    int rc = STITCH_OK;
    size_t max_px = 0;
    for (int i = 0; i < n; ++i) max_px = std::max(max_px, (size_t)wh[2 * i] * wh[2 * i + 1]);
    uint8_t* proj = nullptr;  // nobody reads the projected colours: every frame's land in one block, in stream order
    if ((rc = A.take(&proj, 3 * max_px))) return rc;
    SiftOrder S;
    S.blocks.push_back(proj);
    auto colour_dst = [&](int, uint8_t** p) -> int { *p = proj; return STITCH_OK; };
    auto name = [&](int f) { return "capture " + std::to_string(f / n) + " camera " + std::to_string(f % n); };
    if ((rc = chain_sift_order(frames, nf, c.c.o, c.c.feat_cap, colour_dst, name, A, s, &S))) return rc;
    // a camera's x / y rows of all captures lie in one array, capture k's from base[k][camera] on; the descriptors are per frame
    std::vector<int> base, total;
    if ((rc = cal_bases(S.kept, n_sets, n, &base, &total))) return rc;
    std::vector<float*> X((size_t)n, nullptr), Y((size_t)n, nullptr);
    for (int i = 0; i < n; ++i)
        if (total[i] && ((rc = A.take(&X[i], sizeof(float) * total[i])) || (rc = A.take(&Y[i], sizeof(float) * total[i])))) return rc;
    std::vector<stitch_feature_set> feats((size_t)nf);
    auto place = [&](int f, float** od, float** ox, float** oy) -> int {
        if (!S.kept[f]) return STITCH_OK;
        *ox = X[f % n] + base[f];
        *oy = Y[f % n] + base[f];
        return A.take(od, sizeof(float) * STITCH_DESCRIPTOR_DIM * S.kept[f]);
    };
    if ((rc = chain_gather(S, nf, place, feats.data(), A, s))) return rc;
    return chain_publish(cal_steps(feats.data(), X, Y, base, total, c, A, s, K.get()), s, K, out);
}

}  // namespace

extern "C" {

void stitch_calibrate_opts_default(stitch_calibrate_opts* o) {
    if (!o) return;
    std::memset(o, 0, sizeof *o);
}

int stitch_dev_calibrate_u8(const stitch_frame_u8* frames, int n_sets, int n, const stitch_calibrate_opts* opts, void* stream, stitch_calibration** out) {
    CalCfg c;
    std::vector<int32_t> wh;
    int rc = cal_check(n_sets, n, opts, out, &c);
    if (rc || (rc = cal_check_frames(frames, n_sets, n, &wh)) || (rc = need_device())) return rc;
    return cal_from_frames(frames, n_sets, n, wh, c, stream, out);
}

int stitch_dev_calibrate_from_features_u8(const int32_t* frame_wh, const stitch_feature_set* feats, int n_sets, int n, const stitch_calibrate_opts* opts,
                                          void* stream, stitch_calibration** out) {
    CalCfg c;
    int rc = cal_check(n_sets, n, opts, out, &c);
    if (rc) return rc;
    if (!frame_wh || !feats) return fail(STITCH_ERR_ARG, "calibrate: no frame sizes or no feature sets");
    const int nf = n_sets * n;
    for (int i = 0; i < n; ++i)
        if (frame_wh[2 * i] <= 0 || frame_wh[2 * i + 1] <= 0) return fail(STITCH_ERR_ARG, "calibrate: camera %d has a bad size %d x %d", i, frame_wh[2 * i], frame_wh[2 * i + 1]);
    std::vector<int> rows((size_t)nf);
    for (int f = 0; f < nf; ++f) {
        if (feature_set_lacks_array(feats[f]))
            return fail(STITCH_ERR_ARG, "calibrate: the feature set of capture %d camera %d lacks an array", f / n, f % n);
        rows[f] = feats[f].n;
    }
    std::vector<int> base, total;
    if ((rc = cal_bases(rows, n_sets, n, &base, &total)) || (rc = need_device())) return rc;
    hipStream_t s = as_stream(stream);
    PanoArena A(s);
    std::unique_ptr<stitch_calibration> K = cal_new(n_sets, n, std::vector<int32_t>(frame_wh, frame_wh + 2 * n));
    // the steps move key points: they work on this call's pooled copies of x / y
    std::vector<float*> X((size_t)n, nullptr), Y((size_t)n, nullptr);
    for (int i = 0; i < n; ++i)
        if (total[i] && ((rc = A.take(&X[i], sizeof(float) * total[i])) || (rc = A.take(&Y[i], sizeof(float) * total[i])))) return rc;
    for (int f = 0; f < nf; ++f) {
        if (!rows[f]) continue;
        const size_t b = sizeof(float) * rows[f];
        HIPCHK(hipMemcpyAsync(X[f % n] + base[f], feats[f].d_x, b, hipMemcpyDeviceToDevice, s));
        HIPCHK(hipMemcpyAsync(Y[f % n] + base[f], feats[f].d_y, b, hipMemcpyDeviceToDevice, s));
    }
    return chain_publish(cal_steps(feats, X, Y, base, total, c, A, s, K.get()), s, K, out);
}

int stitch_calibrate_u8(const stitch_frame_u8* frames, int n_sets, int n, const stitch_calibrate_opts* opts, stitch_calibration** out) {
    CalCfg c;  // refused arguments are refused before a frame goes up
    std::vector<int32_t> wh;
    int rc = cal_check(n_sets, n, opts, out, &c);
    if (rc || (rc = cal_check_frames(frames, n_sets, n, &wh)) || (rc = need_device())) return rc;
    std::vector<DevBuf> up;
    std::vector<stitch_frame_u8> dev;
    if ((rc = chain_upload_frames(frames, n_sets * n, &up, &dev))) return rc;
    return cal_from_frames(dev.data(), n_sets, n, wh, c, nullptr, out);
}

int stitch_calibration_info(const stitch_calibration* cal, int* n_sets, int* n, int* start, int* n_steps, int* width, int* height) {
    if (!cal) return fail(STITCH_ERR_ARG, "calibration_info: null handle");
    if (n_sets) *n_sets = cal->n_sets;
    if (n) *n = cal->n;
    if (start) *start = cal->start;
    if (n_steps) *n_steps = (int)cal->steps.size();
    if (width) *width = cal->w;
    if (height) *height = cal->h;
    return STITCH_OK;
}

int stitch_calibration_step_at(const stitch_calibration* cal, int k, stitch_panorama_step* step) {
    if (!cal || !step || k < 0 || k >= (int)cal->steps.size()) return fail(STITCH_ERR_ARG, "calibration_step_at: bad argument (step %d)", k);
    *step = cal->steps[k];
    return STITCH_OK;
}

int stitch_calibration_counts(const stitch_calibration* cal, int32_t* per_capture, int32_t* pooled) {
    if (!cal) return fail(STITCH_ERR_ARG, "calibration_counts: null handle");
    const size_t nn = (size_t)cal->n * cal->n, per = nn * cal->n_sets;
    if (per_capture) std::memcpy(per_capture, cal->counts.data(), sizeof(int32_t) * per);
    if (pooled) std::memcpy(pooled, cal->counts.data() + per, sizeof(int32_t) * nn);
    return STITCH_OK;
}

int stitch_calibration_step_support(const stitch_calibration* cal, int k, int32_t* pairs, int32_t* inliers) {
    if (!cal || k < 0 || k >= (int)cal->steps.size()) return fail(STITCH_ERR_ARG, "calibration_step_support: bad argument (step %d)", k);
    for (int c = 0; c < cal->n_sets; ++c) {
        const int32_t* sup = &cal->support[((size_t)k * cal->n_sets + c) * 2];
        if (pairs) pairs[c] = sup[0];
        if (inliers) inliers[c] = sup[1];
    }
    return STITCH_OK;
}

int stitch_rig_from_calibration(const stitch_calibration* cal, const stitch_rig_opts* opts, const stitch_exposure_opts* exposure, stitch_rig** out) {
    if (out) *out = nullptr;
    if (!cal || !out) return fail(STITCH_ERR_ARG, "rig_from_calibration: null argument");
    return rig_create(cal->wh.data(), cal->n, cal->start, cal->steps.data(), (int)cal->steps.size(), opts, exposure, out);
}

void stitch_calibration_destroy(stitch_calibration* cal) { delete cal; }

}  // extern "C"
