// stitch_panorama.inc -- the whole panorama as one call (include/stitch_panorama.h; kernels in k_panorama.inc).
// Included in stitch_hip.hip (one translation unit) behind stitch_chain.inc, which holds the call's scratch, the SIFT front end,
// the all-pairs matching and a step's two estimations.
//
// The chain restates pipeline.py's panorama_from_frames / panorama_from_features step for step on top of the C entry points of
// the stages.  Per call the host waits three times for data: (1) the SIFT heads and the descriptor rows written, for the
// std::map order; (2) the n x n match counts, for the stitch order; (3) per step the two maps and their info rows, for the
// canvas of the step.  Where it differs from the Python chain no bit can change: descriptors and key points stay on the device
// (only the index array of the map order goes up, k_feat_gather builds the ordered sets), and a step takes its two lists from
// the all-pairs matching of (2) instead of matching the pair again -- descriptors never change after SIFT, so they are the lists
// pair_maps would recompute.
struct stitch_panorama {
    int w = 0, h = 0, start = 0, keep = 0;
    uint8_t* final_px = nullptr;
    std::vector<stitch_panorama_step> steps;
    std::vector<uint8_t*> step_px;  // with keep: one per step
    // include/stitch_exposure.h: twelve statistics per step, and with keep each step's recoloured frame with its size
    int exposure_mode = 0;
    std::vector<float> exposure_stats;
    std::vector<uint8_t*> exposure_px;
    std::vector<int> exposure_wh;
    // device copies enqueued by stitch_panorama_copy and not yet waited for: one event each, behind the copy on its stream
    mutable std::mutex mu;
    mutable std::vector<hipEvent_t> copies;
    ~stitch_panorama() {
        for (hipEvent_t e : copies) {  // no copy may still read a mosaic when it is freed
            (void)hipEventSynchronize(e);
            (void)hipEventDestroy(e);
        }
        if (final_px) (void)hipFreeAsync(final_px, nullptr);
        for (uint8_t* p : step_px)
            if (p) (void)hipFreeAsync(p, nullptr);
        for (uint8_t* p : exposure_px)
            if (p) (void)hipFreeAsync(p, nullptr);
    }
};

namespace {

constexpr int kPanoMaxFrames = 64;

struct PanoCfg {
    stitch_panorama_opts o;
    int feat_cap;
    stitch_exposure_opts ex;  // mode 0: the chain without a transfer
};

int pano_cfg(const stitch_panorama_opts* opts, const stitch_exposure_opts* exposure, PanoCfg* c) {
    c->ex = stitch_exposure_opts{0, 0, 0};
    if (exposure) {
        c->ex = *exposure;
        int rc = chain_check_exposure(c->ex, "panorama");
        if (rc) return rc;
    }
    if (opts)
        c->o = *opts;
    else
        stitch_panorama_opts_default(&c->o);
    if (c->o.kp_cap < 0 || c->o.feat_cap < 0) return fail(STITCH_ERR_ARG, "panorama: negative capacity (kp_cap %d, feat_cap %d)", c->o.kp_cap, c->o.feat_cap);
    if ((long long)c->o.kp_cap * 2 > 0x7fffffffLL / STITCH_DESCRIPTOR_DIM) return fail(STITCH_ERR_ARG, "panorama: kp_cap = %d is too large", c->o.kp_cap);
    c->feat_cap = c->o.feat_cap ? c->o.feat_cap : 2 * c->o.kp_cap;
    if (std::isnan(c->o.ratio)) return fail(STITCH_ERR_ARG, "panorama: ratio is NaN");
    return STITCH_OK;
}

// What every entry point starts with: *out cleared, a device, then the frames.
int pano_check_frames(const stitch_frame_u8* frames, int n, stitch_panorama** out) {
    if (out) *out = nullptr;
    int rc = need_device();
    if (rc) return rc;
    if (!out || !frames || n < 1 || n > kPanoMaxFrames) return fail(STITCH_ERR_ARG, "panorama: %d frames (1 .. %d) or a null argument", n, kPanoMaxFrames);
    for (int i = 0; i < n; ++i)
        if (!frames[i].data || frames[i].width <= 0 || frames[i].height <= 0)
            return fail(STITCH_ERR_ARG, "panorama: frame %d has no data or a bad size %d x %d", i, frames[i].width, frames[i].height);
    return STITCH_OK;
}

int dev_points_args(const float* x, const float* y, int n, const char* what) {
    if (n < 0 || (n > 0 && (!x || !y))) return fail(STITCH_ERR_ARG, "%s: bad argument", what);
    return STITCH_OK;
}

// The longer-list rule on the device, then both estimations: forward (the mirrored list) first.  sd / ds are the matcher's lists
// for (data = src, queries = dst) and (data = dst, queries = src).  d_sel (2 * cap int32) and d_sel_count are scratch.
int pano_select_and_fit(const int32_t* d_sd, const int32_t* d_count_sd, const int32_t* d_ds, const int32_t* d_count_ds, const float* src_x,
                        const float* src_y, int n_src, const float* dst_x, const float* dst_y, int n_dst, int32_t* d_sel, int32_t* d_sel_count,
                        const stitch_ransac_opts* ransac, double* d_p16, int32_t* d_info10, hipStream_t s) {
    const int cap = std::max(std::max(n_src, n_dst), 1);
    k_pair_select<<<(unsigned)std::min((cap + 255) / 256, 64), 256, 0, s>>>(d_sd, d_count_sd, n_dst, d_ds, d_count_ds, n_src, 0, cap, d_sel, d_sel_count);
    int rc = launch_check("k_pair_select");
    if (rc) return rc;
    return chain_step_fit(src_x, src_y, dst_x, dst_y, d_sel, d_sel_count, cap, ransac, d_p16, d_info10, nullptr, s);
}

// Everything from the ordered features on: counts, order, steps, finish.  x / y of `feats` are this call's own arrays (the steps
// update them in place); proj[i] is frame i projected, or NULL where it has not been projected yet.
int pano_steps(const stitch_frame_u8* frames, std::vector<uint8_t*>& proj, const stitch_feature_set* feats, std::vector<float*>& fx,
               std::vector<float*>& fy, int n, const PanoCfg& c, PanoArena& A, hipStream_t s, stitch_panorama* P) {
    int rc = STITCH_OK;
    // ---- all ordered pairs in one matcher call; the lists stay on the device ----
    PairLists L;
    if ((rc = chain_match_all(feats, 1, n, c.o.ratio, 0, A, s, &L))) return rc;
    // ---- read-back 2: the counts ----
    std::vector<int32_t> counts((size_t)n * n);
    HIPCHK(hipMemcpyAsync(counts.data(), L.d_counts, L.count_bytes, hipMemcpyDeviceToHost, s));
    if ((rc = pano_sync(s))) return rc;
    std::vector<int32_t> order((size_t)2 * n * std::max(n - 1, 1));
    int start = 0, n_steps = 0;
    if ((rc = stitch_stitch_order(counts.data(), n, c.o.match_threshold, &start, order.data(), &n_steps))) return rc;
    P->start = start;

    auto projected = [&](int i) -> int {
        if (proj[i]) return STITCH_OK;
        int rc_ = A.take(&proj[i], (size_t)3 * frames[i].width * frames[i].height);
        if (rc_) return rc_;
        return stitch_dev_project_u8(frames[i].data, frames[i].width, frames[i].height, c.o.fov_deg, proj[i], s);
    };
    if ((rc = projected(start))) return rc;
    uint8_t* result = proj[start];
    int rw = frames[start].width, rh = frames[start].height;
    bool result_is_step = false;
    int pre = start;

    int max_n = 1;
    for (int i = 0; i < n; ++i) max_n = std::max(max_n, feats[i].n);
    int32_t* d_sel = nullptr;
    StepBlock B;
    if ((rc = A.take(&d_sel, sizeof(int32_t) * 2 * max_n)) || (rc = A.take(&B.d, StepBlock::kHead))) return rc;

    float* d_ex_stats = nullptr;  // twelve per step
    P->exposure_mode = c.ex.mode;
    if (c.ex.mode && n_steps) {
        if ((rc = A.take(&d_ex_stats, sizeof(float) * 12 * n_steps))) return rc;
        P->exposure_stats.assign((size_t)12 * n_steps, 0.f);
    }

    for (int k = 0; k < n_steps; ++k) {
        const int src = order[2 * k], dst = order[2 * k + 1];
        if ((rc = pano_select_and_fit(L.list_of(0, src, dst), L.count_of(0, src, dst), L.list_of(0, dst, src), L.count_of(0, dst, src), fx[src], fy[src],
                                      feats[src].n, fx[dst], fy[dst], feats[dst].n, d_sel, B.sel_count(), c.o.ransac, B.p16(), B.info10(), s)))
            return rc;
        // ---- read-back 3: 16 doubles and 10 ints ----
        unsigned char got[StepBlock::kBack];
        stitch_panorama_step st;
        bool ok = false;
        if ((rc = chain_step_read(B, sizeof got, src, dst, s, got, &st, &ok))) return rc;
        if (!ok) return fail(STITCH_ERR_NO_MAP, "frames %d -> %d: no map (RANSAC status %d / %d, %d pairs)", src, dst, st.info[0][0], st.info[1][0], st.info[0][1]);
        if ((rc = projected(dst))) return rc;
        const int fw = frames[dst].width, fh = frames[dst].height;
        if ((rc = stitch_step_geometry(fw, fh, st.p_fwd, rw, rh, &st.geom))) return rc;
        const size_t samples = (size_t)3 * st.geom.cw * st.geom.ch;
        uint8_t* next = nullptr;
        if ((rc = A.take(&next, samples))) return rc;
        if (c.ex.mode) {
            // ImageProcess.cpp:180-182, switched on: the frame about to be warped takes the colour statistics of what is
            // already stitched, in place on its stored projection (a later step that warps or reads it again sees the result)
            if ((rc = projected(src))) return rc;
            const uint8_t* tem = c.ex.mode == 1 ? proj[src] : result;
            const int tw = c.ex.mode == 1 ? frames[src].width : rw, th = c.ex.mode == 1 ? frames[src].height : rh;
            if ((rc = stitch_dev_transfer_form_u8(proj[dst], fw, fh, tem, tw, th, proj[dst], d_ex_stats + 12 * k, c.ex.stats_form, c.ex.keep_black, nullptr, s)))
                return rc;
            if (c.o.keep_steps) {
                uint8_t* copy = nullptr;
                if ((rc = A.take(&copy, (size_t)3 * fw * fh))) return rc;
                HIPCHK(hipMemcpyAsync(copy, proj[dst], (size_t)3 * fw * fh, hipMemcpyDeviceToDevice, s));
                A.give_up(copy);
                P->exposure_px.push_back(copy);
                P->exposure_wh.push_back(fw);
                P->exposure_wh.push_back(fh);
            }
        }
        if ((rc = stitch_dev_step_u8(proj[dst], fw, fh, st.p_fwd, st.p_bwd, result, rw, rh, c.o.blend, next, samples, &st.geom, &st.seam, s))) return rc;
        // :226-227: the warped frame's key points go through the forward map, those of the frame warped before move by the offsets
        if ((rc = stitch_dev_map_points(fx[dst], fy[dst], nullptr, nullptr, feats[dst].n, st.p_fwd, st.geom.min_x, st.geom.min_y, s))) return rc;
        if ((rc = stitch_dev_shift_points(fx[pre], fy[pre], nullptr, nullptr, feats[pre].n, st.geom.ox, st.geom.oy, s))) return rc;
        pre = dst;
        if (result_is_step && !c.o.keep_steps) A.release(result);  // the step that read it has completed
        result = next;
        rw = st.geom.cw;
        rh = st.geom.ch;
        result_is_step = true;
        P->steps.push_back(st);
        if (c.o.keep_steps) {
            A.give_up(next);
            P->step_px.push_back(next);
        }
    }
    // the callers wait for the stream before the handle leaves them
    if (d_ex_stats) HIPCHK(hipMemcpyAsync(P->exposure_stats.data(), d_ex_stats, sizeof(float) * 12 * n_steps, hipMemcpyDeviceToHost, s));
    // ---- the finish pass works on a copy where the last step's mosaic is kept ----
    uint8_t* fin = result;
    const size_t bytes = (size_t)3 * rw * rh;
    if (result_is_step && c.o.keep_steps) {
        if ((rc = A.take(&fin, bytes))) return rc;
        HIPCHK(hipMemcpyAsync(fin, result, bytes, hipMemcpyDeviceToDevice, s));
    }
    if (c.o.finish && (rc = stitch_dev_finish_u8(fin, rw, rh, c.o.num, c.o.den, nullptr, s))) return rc;
    A.give_up(fin);
    for (uint8_t*& p : proj)
        if (p == fin) p = nullptr;
    P->final_px = fin;
    P->w = rw;
    P->h = rh;
    P->keep = c.o.keep_steps != 0;
    return STITCH_OK;
}

}  // namespace

extern "C" {

void stitch_panorama_opts_default(stitch_panorama_opts* o) {
    if (!o) return;
    std::memset(o, 0, sizeof *o);
    o->ratio = 0.5;
    o->match_threshold = 20;
    o->fov_deg = 15.0f;
    o->kp_cap = 4096;
    o->feat_cap = 0;
    o->finish = 1;
    o->num = 19.0;
    o->den = 20.0;
    o->keep_steps = 0;
}

int stitch_feature_order(const float* desc, int n, int32_t* index, int* n_kept) {
    if (n < 0 || !n_kept || (n > 0 && (!desc || !index))) return fail(STITCH_ERR_ARG, "feature_order: bad argument");
    constexpr int D = STITCH_DESCRIPTOR_DIM;
    std::vector<int32_t> ord((size_t)n);
    for (int i = 0; i < n; ++i) ord[i] = i;
    std::stable_sort(ord.begin(), ord.end(), [desc](int32_t a, int32_t b) {
        const float *x = desc + (size_t)a * D, *y = desc + (size_t)b * D;
        for (int k = 0; k < D; ++k) {  // std::vector<float>'s operator<: the first component that differs under float <
            if (x[k] < y[k]) return true;
            if (y[k] < x[k]) return false;
        }
        return false;
    });
    int m = 0;
    for (int i = 0; i < n; ++i) {
        bool same = i > 0;
        if (same) {
            const float *x = desc + (size_t)ord[i - 1] * D, *y = desc + (size_t)ord[i] * D;
            for (int k = 0; k < D && same; ++k) same = x[k] == y[k];
        }
        if (!same) index[m++] = ord[i];
    }
    *n_kept = m;
    return STITCH_OK;
}

int stitch_stitch_order(const int32_t* counts, int n, int threshold, int* start, int32_t* src_dst_pairs, int* n_steps) {
    if (!counts || n < 1 || !start || !n_steps || (n > 1 && !src_dst_pairs)) return fail(STITCH_ERR_ARG, "stitch_order: bad argument");
    std::vector<char> mat((size_t)n * n, 0);
    std::vector<std::vector<int>> nxt((size_t)n);
    auto M = [&](int i, int j) -> char& { return mat[(size_t)i * n + j]; };
    for (int i = 0; i < n; ++i)  // :117-137
        for (int j = 0; j < n; ++j) {
            if (i == j) continue;
            if (M(j, i)) {
                M(i, j) = 1;
                nxt[i].push_back(j);
                continue;
            }
            if (counts[(size_t)i * n + j] >= threshold) {
                M(i, j) = 1;
                nxt[i].push_back(j);
            }
        }
    // getMiddleIndex (:353-393): walk from an edge frame (exactly one neighbour; frame 0 without one), take the middle of the walk
    int edge = 0;
    for (int i = 0; i < n; ++i)
        if (nxt[i].size() == 1) {
            edge = i;
            break;
        }
    int next_one = edge;
    std::vector<int> que;
    for (int index = 0; index < n; ++index) {
        if (que.empty()) que.push_back(edge);
        for (int i = 0; i < n; ++i) {
            if (next_one == i) continue;
            if (M(next_one, i)) {
                if (i < (int)que.size()) continue;  // the reference compares the frame index with the queue POSITIONS (:377-382)
                if (i != edge) que.push_back(i);
                next_one = i;
                break;
            }
        }
    }
    *start = que[que.size() / 2];
    int steps = 0;
    std::vector<int> wait(1, *start);
    for (size_t head = 0; head < wait.size(); ++head) {  // :139-175, a FIFO
        const int src = wait[head];
        for (size_t r = nxt[src].size(); r-- > 0;) {
            const int dst = nxt[src][r];
            if (!M(src, dst)) continue;
            M(src, dst) = M(dst, src) = 0;
            wait.push_back(dst);
            src_dst_pairs[2 * steps] = src;
            src_dst_pairs[2 * steps + 1] = dst;
            ++steps;
        }
    }
    *n_steps = steps;
    return STITCH_OK;
}

int stitch_dev_map_points(float* d_x, float* d_y, int32_t* d_ix, int32_t* d_iy, int n, const double p_fwd[8], float offx, float offy,
                          void* stream) {
    int rc = need_device();
    if (rc) return rc;
    if (!p_fwd) return fail(STITCH_ERR_ARG, "dev_map_points: bad argument");
    if ((rc = dev_points_args(d_x, d_y, n, "dev_map_points"))) return rc;
    if (n == 0) return STITCH_OK;
    MapP m;
    std::memcpy(m.p, p_fwd, sizeof m.p);
    k_map_points<<<(unsigned)((n + 255) / 256), 256, 0, as_stream(stream)>>>(d_x, d_y, d_ix, d_iy, n, m, offx, offy);
    return launch_check("k_map_points");
}

int stitch_dev_shift_points(float* d_x, float* d_y, int32_t* d_ix, int32_t* d_iy, int n, int ox, int oy, void* stream) {
    int rc = need_device();
    if (rc) return rc;
    if ((rc = dev_points_args(d_x, d_y, n, "dev_shift_points"))) return rc;
    if (n == 0) return STITCH_OK;
    k_shift_points<<<(unsigned)((n + 255) / 256), 256, 0, as_stream(stream)>>>(d_x, d_y, d_ix, d_iy, n, ox, oy);
    return launch_check("k_shift_points");
}

int stitch_dev_pair_maps(const stitch_feature_set* src, const stitch_feature_set* dst, double ratio, const stitch_ransac_opts* ransac,
                         double* d_p16, int32_t* d_info10, void* stream) {
    int rc = need_device();
    if (rc) return rc;
    if (!src || !dst || !d_p16 || !d_info10 || src->n < 0 || dst->n < 0) return fail(STITCH_ERR_ARG, "pair_maps: bad argument");
    for (const stitch_feature_set* f : {src, dst})
        if (feature_set_lacks_array(*f)) return fail(STITCH_ERR_ARG, "pair_maps: a feature set lacks an array");
    hipStream_t s = as_stream(stream);
    PanoArena A(s);
    const int cap = std::max(std::max(src->n, dst->n), 1);
    int32_t *d_sd = nullptr, *d_ds = nullptr, *d_sel = nullptr, *d_cnt = nullptr;
    if ((rc = A.take(&d_sd, sizeof(int32_t) * 2 * std::max(dst->n, 1))) || (rc = A.take(&d_ds, sizeof(int32_t) * 2 * std::max(src->n, 1))) ||
        (rc = A.take(&d_sel, sizeof(int32_t) * 2 * cap)) || (rc = A.take(&d_cnt, sizeof(int32_t) * 4)))
        return rc;
    const stitch_match_desc md[2] = {{src->d_desc, dst->d_desc, src->n, dst->n, nullptr, nullptr, d_sd, d_cnt},
                                     {dst->d_desc, src->d_desc, dst->n, src->n, nullptr, nullptr, d_ds, d_cnt + 1}};
    if ((rc = stitch_dev_match_l1_ratio_many(md, 2, ratio, s))) return rc;
    return pano_select_and_fit(d_sd, d_cnt, d_ds, d_cnt + 1, src->d_x, src->d_y, src->n, dst->d_x, dst->d_y, dst->n, d_sel, d_cnt + 2, ransac, d_p16,
                               d_info10, s);
}

}  // extern "C"

namespace {

int pano_from_features(const stitch_frame_u8* frames, const stitch_feature_set* feats, int n, const stitch_panorama_opts* opts,
                       const stitch_exposure_opts* exposure, void* stream, stitch_panorama** out) {
    int rc = pano_check_frames(frames, n, out);
    if (rc) return rc;
    if (!feats) return fail(STITCH_ERR_ARG, "panorama: no feature sets");
    for (int i = 0; i < n; ++i)
        if (feature_set_lacks_array(feats[i])) return fail(STITCH_ERR_ARG, "panorama: feature set %d lacks an array", i);
    PanoCfg c;
    if ((rc = pano_cfg(opts, exposure, &c))) return rc;
    hipStream_t s = as_stream(stream);
    PanoArena A(s);
    std::unique_ptr<stitch_panorama> P(new stitch_panorama());
    // the steps move key points: they work on this call's copy of x / y (one block, x then y per frame)
    std::vector<float*> fx((size_t)n, nullptr), fy((size_t)n, nullptr);
    for (int i = 0; i < n; ++i) {
        if (!feats[i].n) continue;
        const size_t b = sizeof(float) * feats[i].n;
        if ((rc = A.take(&fx[i], b)) || (rc = A.take(&fy[i], b))) return rc;
        HIPCHK(hipMemcpyAsync(fx[i], feats[i].d_x, b, hipMemcpyDeviceToDevice, s));
        HIPCHK(hipMemcpyAsync(fy[i], feats[i].d_y, b, hipMemcpyDeviceToDevice, s));
    }
    std::vector<uint8_t*> proj((size_t)n, nullptr);
    return chain_publish(pano_steps(frames, proj, feats, fx, fy, n, c, A, s, P.get()), s, P, out);
}

int pano_from_frames(const stitch_frame_u8* frames, int n, const stitch_panorama_opts* opts, const stitch_exposure_opts* exposure, void* stream,
                     stitch_panorama** out) {
    int rc = pano_check_frames(frames, n, out);
    if (rc) return rc;
    PanoCfg c;
    if ((rc = pano_cfg(opts, exposure, &c))) return rc;
    hipStream_t s = as_stream(stream);
    PanoArena A(s);
    std::unique_ptr<stitch_panorama> P(new stitch_panorama());
    // every frame's projected colours are kept: the steps warp them
    std::vector<uint8_t*> proj((size_t)n, nullptr);
    auto colour_dst = [&](int i, uint8_t** p) -> int {
        const int rc_ = A.take(&proj[i], (size_t)3 * frames[i].width * frames[i].height);
        *p = proj[i];
        return rc_;
    };
    SiftOrder S;
    if ((rc = chain_sift_order(frames, n, c.o, c.feat_cap, colour_dst, [](int i) { return "frame " + std::to_string(i); }, A, s, &S))) return rc;
    // a frame's ordered rows: its own three blocks; the steps update x / y in place
    std::vector<stitch_feature_set> feats((size_t)n);
    std::vector<float*> fx((size_t)n, nullptr), fy((size_t)n, nullptr);
    auto place = [&](int i, float** od, float** ox, float** oy) -> int {
        const size_t k = (size_t)S.kept[i];
        int rc_ = STITCH_OK;
        if (k && ((rc_ = A.take(od, sizeof(float) * STITCH_DESCRIPTOR_DIM * k)) || (rc_ = A.take(&fx[i], sizeof(float) * k)) || (rc_ = A.take(&fy[i], sizeof(float) * k))))
            return rc_;
        *ox = fx[i];
        *oy = fy[i];
        return STITCH_OK;
    };
    if ((rc = chain_gather(S, n, place, feats.data(), A, s))) return rc;
    return chain_publish(pano_steps(frames, proj, feats.data(), fx, fy, n, c, A, s, P.get()), s, P, out);
}

int pano_from_host_frames(const stitch_frame_u8* frames, int n, const stitch_panorama_opts* opts, const stitch_exposure_opts* exposure,
                          stitch_panorama** out) {
    int rc = pano_check_frames(frames, n, out);
    if (rc) return rc;
    PanoCfg c;  // refused options are refused before a frame goes up
    if ((rc = pano_cfg(opts, exposure, &c))) return rc;
    std::vector<DevBuf> up;
    std::vector<stitch_frame_u8> dev;
    if ((rc = chain_upload_frames(frames, n, &up, &dev))) return rc;
    return pano_from_frames(dev.data(), n, opts, exposure, nullptr, out);
}

}  // namespace

extern "C" {

int stitch_dev_panorama_from_features_u8(const stitch_frame_u8* frames, const stitch_feature_set* feats, int n, const stitch_panorama_opts* opts,
                                         void* stream, stitch_panorama** out) {
    return pano_from_features(frames, feats, n, opts, nullptr, stream, out);
}

int stitch_dev_panorama_u8(const stitch_frame_u8* frames, int n, const stitch_panorama_opts* opts, void* stream, stitch_panorama** out) {
    return pano_from_frames(frames, n, opts, nullptr, stream, out);
}

int stitch_panorama_u8(const stitch_frame_u8* frames, int n, const stitch_panorama_opts* opts, stitch_panorama** out) {
    return pano_from_host_frames(frames, n, opts, nullptr, out);
}

int stitch_panorama_info(const stitch_panorama* pano, int* width, int* height, int* start, int* n_steps) {
    if (!pano) return fail(STITCH_ERR_ARG, "panorama_info: null handle");
    if (width) *width = pano->w;
    if (height) *height = pano->h;
    if (start) *start = pano->start;
    if (n_steps) *n_steps = (int)pano->steps.size();
    return STITCH_OK;
}

int stitch_panorama_step_at(const stitch_panorama* pano, int k, stitch_panorama_step* step) {
    if (!pano || !step || k < 0 || k >= (int)pano->steps.size()) return fail(STITCH_ERR_ARG, "panorama_step_at: bad argument (step %d)", k);
    *step = pano->steps[k];
    return STITCH_OK;
}

const void* stitch_panorama_pixels(const stitch_panorama* pano) { return pano ? pano->final_px : nullptr; }

const void* stitch_panorama_step_pixels(const stitch_panorama* pano, int k) {
    return pano && k >= 0 && k < (int)pano->step_px.size() ? pano->step_px[k] : nullptr;
}

int stitch_panorama_copy(const stitch_panorama* pano, int k, void* dst, size_t capacity, int dst_is_device, void* stream) {
    if (!pano || !dst || k < -1 || k >= (int)pano->steps.size()) return fail(STITCH_ERR_ARG, "panorama_copy: bad argument (step %d)", k);
    const void* src = k < 0 ? pano->final_px : stitch_panorama_step_pixels(pano, k);
    if (!src) return fail(STITCH_ERR_ARG, "panorama_copy: step %d was not kept (keep_steps = 0)", k);
    const size_t bytes = k < 0 ? (size_t)3 * pano->w * pano->h : (size_t)3 * pano->steps[k].geom.cw * pano->steps[k].geom.ch;
    if (capacity < bytes) return fail(STITCH_ERR_ARG, "panorama_copy: %zu bytes needed, the destination holds %zu", bytes, capacity);
    hipStream_t s = as_stream(stream);
    HIPCHK(hipMemcpyAsync(dst, src, bytes, dst_is_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, s));
    if (!dst_is_device) {
        HIPCHK(hipStreamSynchronize(s));
        return STITCH_OK;
    }
    hipEvent_t done = nullptr;  // stitch_panorama_destroy waits for it before the mosaic is freed
    HIPCHK(hipEventCreateWithFlags(&done, hipEventDisableTiming));
    const hipError_t e = hipEventRecord(done, s);
    if (e != hipSuccess) {
        (void)hipEventDestroy(done);
        (void)hipStreamSynchronize(s);
        return fail(STITCH_ERR_HIP, "hipEventRecord failed: %s", hipGetErrorString(e));
    }
    std::lock_guard<std::mutex> lock(pano->mu);
    pano->copies.push_back(done);
    return STITCH_OK;
}

void stitch_panorama_destroy(stitch_panorama* pano) { delete pano; }

}  // extern "C"
