// stitch_calibrate.inc -- a rig calibrated from several captures (include/stitch_calibrate.h; kernels in k_calibrate.inc).
// Included at the end of stitch_hip.hip (one translation unit).
//
// The chain restates pipeline.py's calibrate_from_sets on top of the C entry points of the stages; it is pano_from_frames and
// pano_steps (stitch_panorama.inc) over n_sets captures, without a pixel of the mosaic: no stitch step, no transfer, no finish
// pass.  Per call the host waits as often as the whole-panorama chain does, whatever n_sets is: (1) the SIFT heads of all frames,
// then the descriptor rows written, for the std::map order; (2) the per-capture and pooled match counts, for the stitch order;
// (3) per step the two maps, their info rows and the step's support.  What changes against one capture: a camera's key points of
// all captures lie in one array (capture k's rows from base[k][camera] on), so one k_map_points / k_shift_points launch moves
// them all, and k_pool_select builds the step's list over those arrays from the captures' matcher lists.
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
    // ---- every capture's ordered pairs in one matcher call; the lists stay on the device ----
    int32_t* d_counts = nullptr;  // n_sets matrices, then the pooled one
    const size_t count_bytes = sizeof(int32_t) * (size_t)(n_sets + 1) * nn;
    if ((rc = A.take(&d_counts, count_bytes))) return rc;
    HIPCHK(hipMemsetAsync(d_counts, 0, count_bytes, s));
    std::vector<size_t> list_off((size_t)n_sets * nn, 0);
    size_t lists_total = 0;
    for (int k = 0; k < n_sets; ++k)
        for (int i = 0; i < n; ++i)
            for (int j = 0; j < n; ++j)
                if (i != j) {
                    list_off[(size_t)k * nn + i * n + j] = lists_total;
                    lists_total += align256(sizeof(int32_t) * 2 * std::max(F(k, j).n, 1));
                }
    char* d_lists = nullptr;
    if ((rc = A.take(&d_lists, lists_total))) return rc;
    auto list_of = [&](int k, int i, int j) { return reinterpret_cast<int32_t*>(d_lists + list_off[(size_t)k * nn + i * n + j]); };
    auto count_of = [&](int k, int i, int j) { return d_counts + (size_t)k * nn + i * n + j; };
    {
        std::vector<stitch_match_desc> md;
        for (int k = 0; k < n_sets; ++k)
            for (int i = 0; i < n; ++i)
                for (int j = 0; j < n; ++j)
                    if (i != j)
                        md.push_back(stitch_match_desc{F(k, i).d_desc, F(k, j).d_desc, F(k, i).n, F(k, j).n, nullptr, nullptr, list_of(k, i, j), count_of(k, i, j)});
        if ((rc = stitch_dev_match_l1_ratio_many(md.data(), (int)md.size(), c.c.o.ratio, s))) return rc;
    }
    k_pool_counts<<<(unsigned)std::min((nn + 255) / 256, 64), 256, 0, s>>>(d_counts, n_sets, nn, d_counts + (size_t)n_sets * nn);
    if ((rc = launch_check("k_pool_counts"))) return rc;
    // ---- read-back 2: the counts of every capture and the pooled ones, in one copy ----
    K->counts.assign((size_t)(n_sets + 1) * nn, 0);
    HIPCHK(hipMemcpyAsync(K->counts.data(), d_counts, count_bytes, hipMemcpyDeviceToHost, s));
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
            seg[(size_t)t * n_sets + k] = PoolSeg{list_of(k, src, dst), count_of(k, src, dst), list_of(k, dst, src), count_of(k, dst, src),
                                                 F(k, dst).n,          F(k, src).n,          base[(size_t)k * n + src], base[(size_t)k * n + dst]};
    }
    int max_n = 1;
    for (int i = 0; i < n; ++i) max_n = std::max(max_n, total[i]);
    PoolSeg* d_seg = nullptr;
    int32_t *d_sel = nullptr, *d_inl = nullptr;
    char* d_maps = nullptr;  // 16 doubles, 10 int32, the selected count, a pad; per capture 2 int32 of support; n_sets + 1 offsets
    const size_t head_bytes = 16 * sizeof(double) + 12 * sizeof(int32_t), back_bytes = head_bytes + sizeof(int32_t) * 2 * n_sets;
    if ((rc = A.take(&d_seg, sizeof(PoolSeg) * seg.size())) || (rc = A.take(&d_sel, sizeof(int32_t) * 2 * max_n)) || (rc = A.take(&d_inl, sizeof(int32_t) * max_n)) ||
        (rc = A.take(&d_maps, back_bytes + sizeof(int32_t) * (n_sets + 1))))
        return rc;
    double* d_p16 = reinterpret_cast<double*>(d_maps);
    int32_t* d_info10 = reinterpret_cast<int32_t*>(d_maps + 16 * sizeof(double));
    int32_t* d_sel_count = d_info10 + 2 * STITCH_RANSAC_INFO;
    int32_t* d_support = reinterpret_cast<int32_t*>(d_maps + head_bytes);
    int32_t* d_seg_off = d_support + 2 * n_sets;
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
        k_pool_select<<<(unsigned)std::min((cap + 255) / 256, 64), 256, 0, s>>>(d_seg + (size_t)t * n_sets, n_sets, cap, d_sel, d_sel_count, d_seg_off);
        if ((rc = launch_check("k_pool_select"))) return rc;
        stitch_ransac_desc r[2];
        std::memset(r, 0, sizeof r);
        const float* none = reinterpret_cast<const float*>(d_sel);  // a camera without a row: no list entry names one
        for (int e = 0; e < 2; ++e) {
            r[e].src_x = X[src] ? X[src] : none;
            r[e].src_y = Y[src] ? Y[src] : none;
            r[e].dst_x = X[dst] ? X[dst] : none;
            r[e].dst_y = Y[dst] ? Y[dst] : none;
            r[e].pairs = d_sel;
            r[e].count = d_sel_count;
            r[e].n_max = cap;
            r[e].mirror = e == 0;
            r[e].p = d_p16 + 8 * e;
            r[e].info = d_info10 + STITCH_RANSAC_INFO * e;
        }
        r[0].inliers = d_inl;
        if ((rc = stitch_dev_ransac_many(r, 2, c.c.o.ransac, s))) return rc;
        k_step_support<<<1, WAVE, 0, s>>>(d_inl, cap, d_info10, d_seg_off, n_sets, d_support);
        if ((rc = launch_check("k_step_support"))) return rc;
        // ---- read-back 3: 16 doubles, 10 ints and the support ----
        HIPCHK(hipMemcpyAsync(got.data(), d_maps, back_bytes, hipMemcpyDeviceToHost, s));
        if ((rc = pano_sync(s))) return rc;
        stitch_panorama_step st;
        std::memset(&st, 0, sizeof st);
        st.src = src;
        st.dst = dst;
        std::memcpy(st.p_fwd, got.data(), sizeof st.p_fwd);
        std::memcpy(st.p_bwd, got.data() + sizeof st.p_fwd, sizeof st.p_bwd);
        std::memcpy(st.info, got.data() + 16 * sizeof(double), sizeof st.info);
        if (st.info[0][0] != STITCH_RANSAC_OK || st.info[1][0] != STITCH_RANSAC_OK)
            return fail(STITCH_ERR_NO_MAP, "cameras %d -> %d: no map (RANSAC status %d / %d, %d pooled pairs)", src, dst, st.info[0][0], st.info[1][0], st.info[0][1]);
        if ((rc = stitch_step_geometry(K->wh[2 * dst], K->wh[2 * dst + 1], st.p_fwd, rw, rh, &st.geom))) return rc;
        // :226-227 for every capture at once
        if ((rc = stitch_dev_map_points(X[dst], Y[dst], nullptr, nullptr, total[dst], st.p_fwd, st.geom.min_x, st.geom.min_y, s))) return rc;
        if ((rc = stitch_dev_shift_points(X[pre], Y[pre], nullptr, nullptr, total[pre], st.geom.ox, st.geom.oy, s))) return rc;
        pre = dst;
        rw = st.geom.cw;
        rh = st.geom.ch;
        K->steps.push_back(st);
        const int32_t* sup = reinterpret_cast<const int32_t*>(got.data() + head_bytes);
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
    // ---- a. projection + gray per frame, one SIFT call over the frames of every capture ----
    const size_t kc = (size_t)std::max(c.c.o.kp_cap, 1), fc = (size_t)std::max(c.c.feat_cap, 1);
    size_t max_px = 0;
    for (int i = 0; i < n; ++i) max_px = std::max(max_px, (size_t)wh[2 * i] * wh[2 * i + 1]);
    uint8_t* proj = nullptr;  // nobody reads the projected colours: every frame's land in one block, in stream order
    int32_t* d_heads = nullptr;
    if ((rc = A.take(&proj, 3 * max_px)) || (rc = A.take(&d_heads, sizeof(int32_t) * 8 * nf))) return rc;
    std::vector<stitch_sift_desc> sd((size_t)nf);
    std::vector<void*> sift_blocks(1, proj);
    for (int f = 0; f < nf; ++f) {
        const int w = frames[f].width, h = frames[f].height;
        uint8_t* gray = nullptr;
        stitch_sift_desc& d = sd[f];
        std::memset(&d, 0, sizeof d);
        if ((rc = A.take(&gray, (size_t)w * h)) || (rc = A.take(&d.keypoints, kc * sizeof(StitchSiftKeypoint))) || (rc = A.take(&d.feat_kp, fc * sizeof(int32_t))) ||
            (rc = A.take(&d.feat_angle, fc * sizeof(double))) || (rc = A.take(&d.feat_desc, fc * STITCH_DESCRIPTOR_DIM * sizeof(float))))
            return rc;
        for (void* p : {(void*)gray, (void*)d.keypoints, (void*)d.feat_kp, (void*)d.feat_angle, (void*)d.feat_desc}) sift_blocks.push_back(p);
        if ((rc = stitch_dev_project_gray_u8(frames[f].data, w, h, c.c.o.fov_deg, proj, gray, nullptr, s))) return rc;
        d.image = gray;
        d.width = w;
        d.height = h;
        d.pitch = w;
        d.is_f32 = 0;
        d.kp_cap = c.c.o.kp_cap;
        d.feat_cap = c.c.feat_cap;
        d.counts = d_heads + 8 * f;
        d.status = d_heads + 8 * f + 2;
    }
    if ((rc = stitch_dev_sift_many(sd.data(), nf, c.c.o.sift, s))) return rc;
    // ---- b. read-back 1: the heads of all frames, then the descriptor rows that were written ----
    std::vector<int32_t> heads((size_t)8 * nf);
    HIPCHK(hipMemcpyAsync(heads.data(), d_heads, sizeof(int32_t) * 8 * nf, hipMemcpyDeviceToHost, s));
    if ((rc = pano_sync(s))) return rc;
    std::vector<size_t> row0((size_t)nf + 1, 0);
    for (int f = 0; f < nf; ++f) {
        const int32_t* hd = &heads[(size_t)8 * f];
        if (hd[2] != STITCH_SIFT_OK)
            return fail(STITCH_ERR_CAPACITY, "capture %d camera %d: SIFT capacities too small (%d keypoints, %d features found)", f / n, f % n, hd[3], hd[4]);
        row0[f + 1] = row0[f] + (size_t)hd[1];
    }
    const size_t rows_total = row0[nf];
    std::vector<float> rows(rows_total * STITCH_DESCRIPTOR_DIM);
    for (int f = 0; f < nf; ++f) {
        const size_t cnt = row0[f + 1] - row0[f];
        if (cnt)
            HIPCHK(hipMemcpyAsync(rows.data() + row0[f] * STITCH_DESCRIPTOR_DIM, sd[f].feat_desc, cnt * STITCH_DESCRIPTOR_DIM * sizeof(float), hipMemcpyDeviceToHost, s));
    }
    if ((rc = pano_sync(s))) return rc;
    // the map order on the host; only the index arrays go back up, in one copy
    std::vector<int32_t> index(std::max<size_t>(rows_total, 1));
    std::vector<int> kept((size_t)nf, 0);
    for (int f = 0; f < nf; ++f)
        if ((rc = stitch_feature_order(rows.data() + row0[f] * STITCH_DESCRIPTOR_DIM, (int)(row0[f + 1] - row0[f]), index.data() + row0[f], &kept[f]))) return rc;
    std::vector<int> base, total;
    if ((rc = cal_bases(kept, n_sets, n, &base, &total))) return rc;
    std::vector<float*> X((size_t)n, nullptr), Y((size_t)n, nullptr);
    for (int i = 0; i < n; ++i)
        if (total[i] && ((rc = A.take(&X[i], sizeof(float) * total[i])) || (rc = A.take(&Y[i], sizeof(float) * total[i])))) return rc;
    int32_t* d_index = nullptr;
    if ((rc = A.take(&d_index, sizeof(int32_t) * index.size()))) return rc;
    PanoWait index_in_use{s};
    HIPCHK(hipMemcpyAsync(d_index, index.data(), sizeof(int32_t) * index.size(), hipMemcpyHostToDevice, s));
    std::vector<stitch_feature_set> feats((size_t)nf);
    for (int f0 = 0; f0 < nf; f0 += PANO_MAXFRAMES) {
        const int m = std::min(PANO_MAXFRAMES, nf - f0);
        FeatGatherArgs ga;
        std::memset(&ga, 0, sizeof ga);
        int max_rows = 0;
        for (int j = 0; j < m; ++j) {
            const int f = f0 + j, cam = f % n;
            float* od = nullptr;
            if (kept[f] && (rc = A.take(&od, sizeof(float) * STITCH_DESCRIPTOR_DIM * kept[f]))) return rc;
            float *ox = kept[f] ? X[cam] + base[f] : nullptr, *oy = kept[f] ? Y[cam] + base[f] : nullptr;
            feats[f] = stitch_feature_set{od, ox, oy, kept[f]};
            FeatGatherFrame& g = ga.f[j];
            g.desc = sd[f].feat_desc;
            g.fkp = sd[f].feat_kp;
            g.kp = reinterpret_cast<const SiftKeypoint*>(sd[f].keypoints);
            g.index = d_index + row0[f];
            g.out_desc = od;
            g.out_x = ox;
            g.out_y = oy;
            g.n = kept[f];
            g.n_rows = heads[(size_t)8 * f + 1];
            g.n_kp = heads[(size_t)8 * f];
            max_rows = std::max(max_rows, kept[f]);
        }
        if (max_rows) {
            k_feat_gather<<<dim3((unsigned)((max_rows + PANO_GATHER_T / WAVE - 1) / (PANO_GATHER_T / WAVE)), (unsigned)m), PANO_GATHER_T, 0, s>>>(ga);
            if ((rc = launch_check("k_feat_gather"))) return rc;
        }
    }
    for (void* p : sift_blocks) A.release(p);  // freed in stream order, behind the gather
    rc = cal_steps(feats.data(), X, Y, base, total, c, A, s, K.get());
    const int rc2 = pano_sync(s);  // what the arena frees next is idle
    if (rc) return rc;
    if (rc2) return rc2;
    *out = K.release();
    return STITCH_OK;
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
        if (feats[f].n < 0 || (feats[f].n > 0 && (!feats[f].d_desc || !feats[f].d_x || !feats[f].d_y)))
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
    rc = cal_steps(feats, X, Y, base, total, c, A, s, K.get());
    const int rc2 = pano_sync(s);
    if (rc) return rc;
    if (rc2) return rc2;
    *out = K.release();
    return STITCH_OK;
}

int stitch_calibrate_u8(const stitch_frame_u8* frames, int n_sets, int n, const stitch_calibrate_opts* opts, stitch_calibration** out) {
    CalCfg c;  // refused arguments are refused before a frame goes up
    std::vector<int32_t> wh;
    int rc = cal_check(n_sets, n, opts, out, &c);
    if (rc || (rc = cal_check_frames(frames, n_sets, n, &wh)) || (rc = need_device())) return rc;
    const int nf = n_sets * n;
    std::vector<DevBuf> up((size_t)nf);
    std::vector<stitch_frame_u8> dev((size_t)nf);
    for (int f = 0; f < nf; ++f) {
        const size_t bytes = (size_t)3 * frames[f].width * frames[f].height;
        if ((rc = up[f].alloc(bytes))) return rc;
        H2D(up[f].p, frames[f].data, bytes);
        dev[f] = stitch_frame_u8{up[f].as<uint8_t>(), frames[f].width, frames[f].height};
    }
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
