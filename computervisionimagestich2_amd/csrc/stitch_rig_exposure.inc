// stitch_rig_exposure.inc -- exposure-matched rig replay (include/stitch_rig_exposure.h; kernels in k_rig_exposure.inc, DESIGN.md
// 15).  Included at the end of stitch_hip.hip (one translation unit), behind stitch_rig.inc and stitch_exposure.inc.  The replay
// itself is rig_stitch of stitch_rig.inc, which runs rig_ex_transfer before every step of a rig that was made with a mode.
namespace {

constexpr int kTransferManyMax = 1024;

// Pair i of a many-image transfer in the tables: images 2 i (the source) and 2 i + 1 (the template), planes 6 i .. 6 i + 5 in the
// order l, alpha, beta of the source, then of the template; stats = [mean_src[3], sd_src[3], mean_tem[3], sd_tem[3]].
void ex_fill_pair(ExImage* img, ExPlane* planes, int i, const uint8_t* src, size_t ns, float* lab_s, const uint8_t* tem, size_t nt, float* lab_t, uint8_t* out,
                  float* stats) {
    img[2 * i] = ExImage{src, lab_s, out, stats, (unsigned long long)ns};
    img[2 * i + 1] = ExImage{tem, lab_t, nullptr, nullptr, (unsigned long long)nt};
    for (int c = 0; c < 6; ++c) {
        const bool is_t = c >= 3;
        const size_t n = is_t ? nt : ns;
        planes[6 * i + c] = ExPlane{(is_t ? lab_t : lab_s) + (size_t)(c % 3) * n, (unsigned long long)n, stats + (is_t ? 6 : 0) + c % 3, stats + (is_t ? 9 : 3) + c % 3,
                                    (float)(int)n, 0u};  // the count is the reference's int product as a float
    }
}

// One transfer over `count` pairs of the tables, every source of ns pixels and every template of nt, in two parts: the conversions
// and the statistics (the launches of stitch_dev_transfer_form_u8 up to its apply pass, each over all images or planes), and the
// apply pass, which reads the statistics its ExImage names -- the ones just measured, or (include/stitch_rig_exposure_temporal.h)
// their filtered twins.  sums / table (form 2): 6 * count rows of ceil(max(ns, nt) / EX_SPAN).
int ex_stats_many(const ExImage* d_img, const ExPlane* d_planes, int count, size_t ns, size_t nt, int form, double* sums, ExSpanEntry* table, uint32_t* d_diag,
                  hipStream_t s) {
    int rc = STITCH_OK;
    const TrK k = ex_constants();
    const size_t longest = std::max(ns, nt);
    const unsigned n_planes = 6u * (unsigned)count;
    k_tr_to_lab_many<<<dim3((unsigned)eq_grid(longest), 2u * (unsigned)count), 256, 0, s>>>(d_img, k);
    if ((rc = launch_check("k_tr_to_lab_many"))) return rc;
    if (d_diag) HIPCHK(hipMemsetAsync(d_diag, 0, sizeof(uint32_t) * EX_DIAG_N * n_planes, s));
    if (form == STITCH_STATS_SERIAL) {
        k_ex_stats_serial_many<<<n_planes, 64, 0, s>>>(d_planes);
        if ((rc = launch_check("k_ex_stats_serial_many"))) return rc;
    } else if (form == STITCH_STATS_SCAN) {
        k_ex_walk_many<<<n_planes, EX_T, 0, s>>>(d_planes, 0, 0, nullptr, d_diag);
        if ((rc = launch_check("k_ex_walk_many"))) return rc;
    } else {
        const int max_spans = (int)((longest + EX_SPAN - 1) / EX_SPAN);
        const dim3 grid((unsigned)max_spans, n_planes);
        for (int pass = 0; pass < 2; ++pass) {
            k_ex_span_sums_many<<<grid, EX_T, 0, s>>>(d_planes, pass, max_spans, sums);
            if ((rc = launch_check("k_ex_span_sums_many"))) return rc;
            k_ex_span_maps_many<<<grid, EX_T, 0, s>>>(d_planes, pass, max_spans, sums, table);
            if ((rc = launch_check("k_ex_span_maps_many"))) return rc;
            k_ex_walk_many<<<n_planes, EX_T, 0, s>>>(d_planes, pass, max_spans, table, d_diag);
            if ((rc = launch_check("k_ex_walk_many"))) return rc;
        }
    }
    return STITCH_OK;
}

int ex_apply_many(const ExImage* d_img, int count, size_t ns, int keep_black, hipStream_t s) {
    k_ex_apply_many<<<dim3((unsigned)eq_grid(ns), (unsigned)count), 256, 0, s>>>(d_img, 2, ex_constants(), keep_black);
    return launch_check("k_ex_apply_many");
}

int ex_transfer_many(const ExImage* d_img, const ExPlane* d_planes, int count, size_t ns, size_t nt, int form, int keep_black, double* sums, ExSpanEntry* table,
                     uint32_t* d_diag, hipStream_t s) {
    const int rc = ex_stats_many(d_img, d_planes, count, ns, nt, form, sums, table, d_diag, s);
    return rc ? rc : ex_apply_many(d_img, count, ns, keep_black, s);
}

// include/stitch_rig_exposure_temporal.h: the apply with given statistics over `count` images of n pixels, image i with the record at
// d_stats + i * stats_stride (a rig's fixed record serves every set of a step: stride 0), one launch.
int ex_transfer_given_many(const ExGiven* d_img, int count, size_t n, const float* d_stats, int stats_stride, int keep_black, hipStream_t s) {
    k_ex_transfer_given_many<<<dim3((unsigned)eq_grid(n), (unsigned)count), 256, 0, s>>>(d_img, (unsigned long long)n, d_stats, stats_stride, ex_constants(), keep_black);
    return launch_check("k_ex_transfer_given_many");
}

// ... and the filter of `count` records, one wavefront.  d_failed, d_prev, first_step: a rig's (k_ex_stats_filter); NULL, NULL, 0 otherwise.
int ex_stats_filter(const float* d_m, size_t m_stride, float* d_u, size_t u_stride, int count, int keep, float* d_state12, int32_t* d_has, int32_t* d_failed,
                    const SeamDev* d_prev, int first_step, hipStream_t s) {
    k_ex_stats_filter<<<1, 64, 0, s>>>(d_m, m_stride, d_u, u_stride, count, (float)keep / 256.0f, d_state12, d_has, d_failed, d_prev, first_step);
    return launch_check("k_ex_stats_filter");
}

// a record the filter would take up, and the only kind a caller may give: twelve finite values, the six sds > 0
bool ex_stats_valid(const float* m) {
    for (int j = 0; j < 12; ++j)
        if (!std::isfinite(m[j]) || (j % 6 >= 3 && !(m[j] > 0.0f))) return false;
    return true;
}

// ---- the rig's side (declared in stitch_rig.inc) ---------------------------------------------------------------------------
// The template of step k for set 0 of a sequence, the distance to the next set's, and its size.
void rig_ex_template(const stitch_rig* R, int k, const uint8_t** base, size_t* stride, int* tw, int* th) {
    const stitch_panorama_step& st = R->steps[k];
    const int f = R->ex.mode == 1 ? st.src : R->start;
    if (R->ex.mode == 1 || k == 0) {  // a projected frame: mode 1's src, or the mosaic before step 0
        *base = R->proj[f];
        *stride = (size_t)3 * R->fw[f] * R->fh[f];
        *tw = R->fw[f];
        *th = R->fh[f];
    } else {  // the mosaic step k - 1 wrote
        *base = R->mosaic[(k - 1) & 1];
        *stride = R->mosaic_bytes;
        *tw = R->steps[k - 1].geom.cw;
        *th = R->steps[k - 1].geom.ch;
    }
}

// Scratch of a rig with a mode: see the byte formula in include/stitch_rig_exposure.h.
int rig_ex_workspaces(stitch_rig* R) {
    const size_t S = (size_t)R->max_sets, K = R->steps.size();
    if (!R->ex_lab) HIPCHK(hipMalloc((void**)&R->ex_lab, sizeof(float) * S * 3 * (R->ex_src_px + R->ex_tem_px)));
    if (!R->ex_stats) HIPCHK(hipMalloc((void**)&R->ex_stats, sizeof(float) * 16 * S * K));
    if (R->ex.stats_form == STITCH_STATS_SPANS) {
        const size_t spans = (std::max(R->ex_src_px, R->ex_tem_px) + EX_SPAN - 1) / EX_SPAN;
        if (!R->ex_sums) HIPCHK(hipMalloc((void**)&R->ex_sums, sizeof(double) * 6 * S * spans));
        if (!R->ex_table) HIPCHK(hipMalloc(&R->ex_table, sizeof(ExSpanEntry) * 6 * S * spans));
    }
    return STITCH_OK;
}

// include/stitch_rig_exposure_temporal.h: which of the two options is at work in a replay.  Fixed statistics win over smoothing.
bool rig_et_fixed(const stitch_rig* R) { return R->ex.mode && !R->et_fixed.empty(); }
bool rig_et_smoothed(const stitch_rig* R) { return R->ex.mode && R->et_keep >= 0 && R->et_fixed.empty(); }

// What a replay with a transfer needs beyond rig_workspaces: the transfer's scratch where rig_workspaces left it out because the
// first replay found fixed statistics, and under smoothing the second buffer of records.
int rig_et_workspaces(stitch_rig* R) {
    if (!R->ex.mode || R->steps.empty() || rig_et_fixed(R)) return STITCH_OK;
    const int rc = rig_ex_workspaces(R);  // (takes only what is missing)
    if (rc) return rc;
    if (rig_et_smoothed(R) && !R->ex_used) HIPCHK(hipMalloc((void**)&R->ex_used, sizeof(float) * 16 * (size_t)R->max_sets * R->steps.size()));
    if (rig_et_smoothed(R) && !R->et_failed) HIPCHK(hipMalloc((void**)&R->et_failed, sizeof(int32_t) * (size_t)R->max_sets));
    return STITCH_OK;
}

// The tables of all steps: per step 2 * max_sets images, then per step 6 * max_sets planes.  Set i of a sequence is pair i of its
// step, so a sequence of m < max_sets sets reads a prefix.  Under smoothing the states follow: 12 floats per step, then one flag per
// step.  With fixed statistics the block is another one: per step max_sets ExGiven, then 12 floats per step.
size_t rig_ex_images_bytes(const stitch_rig* R) {
    const size_t KS = R->steps.size() * (size_t)R->max_sets;
    return rig_et_fixed(R) ? KS * sizeof(ExGiven) : KS * (2 * sizeof(ExImage) + 6 * sizeof(ExPlane));
}
size_t rig_ex_table_bytes(const stitch_rig* R) {
    if (!R->ex.mode) return 0;
    const size_t K = R->steps.size();
    return rig_ex_images_bytes(R) + (rig_et_fixed(R) ? K * 12 * sizeof(float) : rig_et_smoothed(R) ? K * (12 * sizeof(float) + sizeof(int32_t)) : 0);
}

void rig_ex_fill_tables(const stitch_rig* R, unsigned char* host, const std::vector<float>& state, const std::vector<int32_t>& has) {
    const int S = R->max_sets, K = (int)R->steps.size();
    if (rig_et_fixed(R)) {
        ExGiven* img = reinterpret_cast<ExGiven*>(host);
        for (int k = 0; k < K; ++k) {
            const int f = R->steps[k].dst;
            for (int i = 0; i < S; ++i) {
                uint8_t* frame = R->proj[f] + (size_t)i * 3 * R->fw[f] * R->fh[f];
                img[(size_t)k * S + i] = ExGiven{frame, frame};
            }
        }
        std::memcpy(host + rig_ex_images_bytes(R), R->et_fixed.data(), sizeof(float) * 12 * K);
        return;
    }
    ExImage* img = reinterpret_cast<ExImage*>(host);
    ExPlane* planes = reinterpret_cast<ExPlane*>(host + (size_t)K * S * 2 * sizeof(ExImage));
    const bool smoothed = rig_et_smoothed(R);
    for (int k = 0; k < K; ++k) {
        const int f = R->steps[k].dst;
        const size_t ns = (size_t)R->fw[f] * R->fh[f];
        const uint8_t* tem = nullptr;
        size_t tem_stride = 0;
        int tw = 0, th = 0;
        rig_ex_template(R, k, &tem, &tem_stride, &tw, &th);
        const size_t nt = (size_t)tw * th;
        for (int i = 0; i < S; ++i) {
            uint8_t* frame = R->proj[f] + (size_t)i * 3 * ns;
            ex_fill_pair(img + (size_t)k * S * 2, planes + (size_t)k * S * 6, i, frame, ns, R->ex_lab + (size_t)i * 3 * R->ex_src_px, tem + (size_t)i * tem_stride, nt,
                         R->ex_lab + (size_t)S * 3 * R->ex_src_px + (size_t)i * 3 * R->ex_tem_px, frame, R->ex_stats + ((size_t)i * K + k) * 16);
            // the planes' statistics go where they went; the apply pass reads their filtered twins
            if (smoothed) img[((size_t)k * S + i) * 2].stats = R->ex_used + ((size_t)i * K + k) * 16;
        }
    }
    if (smoothed) {  // the state the replay starts from: the rig's, a primed one, or none
        float* st = reinterpret_cast<float*>(host + rig_ex_images_bytes(R));
        int32_t* hs = reinterpret_cast<int32_t*>(st + (size_t)12 * K);
        for (int k = 0; k < K; ++k) {
            hs[k] = (size_t)k < has.size() && has[k] ? 1 : 0;
            for (int j = 0; j < 12; ++j) st[12 * k + j] = hs[k] ? state[(size_t)12 * k + j] : 0.0f;
        }
    }
}

int rig_ex_transfer(stitch_rig* R, unsigned char* d_tables, int k, int m, hipStream_t s) {
    const int S = R->max_sets, K = (int)R->steps.size(), f = R->steps[k].dst;
    const size_t ns = (size_t)R->fw[f] * R->fh[f];
    if (rig_et_fixed(R))  // the step's record for every set: source bytes in, recoloured bytes out, nothing else
        return ex_transfer_given_many(reinterpret_cast<const ExGiven*>(d_tables) + (size_t)k * S, m, ns,
                                      reinterpret_cast<const float*>(d_tables + rig_ex_images_bytes(R)) + (size_t)12 * k, 0, R->ex.keep_black, s);
    const ExImage* d_img = reinterpret_cast<const ExImage*>(d_tables) + (size_t)k * S * 2;
    const ExPlane* d_planes = reinterpret_cast<const ExPlane*>(d_tables + (size_t)K * S * 2 * sizeof(ExImage)) + (size_t)k * S * 6;
    const uint8_t* tem = nullptr;
    size_t tem_stride = 0;
    int tw = 0, th = 0;
    rig_ex_template(R, k, &tem, &tem_stride, &tw, &th);
    if (!rig_et_smoothed(R))
        return ex_transfer_many(d_img, d_planes, m, ns, (size_t)tw * th, R->ex.stats_form, R->ex.keep_black, R->ex_sums, static_cast<ExSpanEntry*>(R->ex_table), nullptr, s);
    // smoothing: the statistics as ever, the step's filter over the m sets in their order, then the apply pass on what it wrote
    int rc = ex_stats_many(d_img, d_planes, m, ns, (size_t)tw * th, R->ex.stats_form, R->ex_sums, static_cast<ExSpanEntry*>(R->ex_table), nullptr, s);
    if (rc) return rc;
    float* d_state = reinterpret_cast<float*>(d_tables + rig_ex_images_bytes(R));
    const size_t rec = (size_t)16 * K;  // from a set's record of step k to the next set's
    // a set that the content seam scan of an earlier step refused takes no further part in the filter: the scans of step k - 1 are
    // still in its plan (step k's blend, which may run on the same plan, is queued behind this launch)
    const SeamDev* d_prev = k > 0 && !R->sp_mode && R->fixed.empty() ? R->plans[R->plan_of_step[k - 1]]->d_seam : nullptr;
    if ((rc = ex_stats_filter(R->ex_stats + (size_t)16 * k, rec, R->ex_used + (size_t)16 * k, rec, m, R->et_keep, d_state + (size_t)12 * k,
                              reinterpret_cast<int32_t*>(d_state + (size_t)12 * K) + k, R->et_failed, d_prev, k == 0, s)))
        return rc;
    return ex_apply_many(d_img, m, ns, R->ex.keep_black, s);
}

// The states as the replay's last filter launches left them, to the host: 12 floats per step, then one flag per step.
int rig_et_collect(const stitch_rig* R, const unsigned char* d_tables, std::vector<float>* state, std::vector<int32_t>* has, hipStream_t s) {
    const size_t K = R->steps.size();
    state->assign(12 * K, 0.0f);
    has->assign(K, 0);
    const unsigned char* at = d_tables + rig_ex_images_bytes(R);
    HIPCHK(hipMemcpyAsync(state->data(), at, sizeof(float) * 12 * K, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(has->data(), at + sizeof(float) * 12 * K, sizeof(int32_t) * K, hipMemcpyDeviceToHost, s));
    return STITCH_OK;
}

int rig_et_handle(const stitch_rig* rig, const char* what) {
    if (!rig) return fail(STITCH_ERR_ARG, "%s: null handle", what);
    if (!rig->ex.mode) return fail(STITCH_ERR_ARG, "%s: the rig was made without a transfer (mode 0)", what);
    return STITCH_OK;
}

// n_steps records of a caller's, each one the filter would take up
int rig_et_records(const stitch_rig* rig, const float* stats12, int n_steps, const char* what) {
    const int ns = (int)rig->steps.size();
    if (n_steps != ns || (ns > 0 && !stats12)) return fail(STITCH_ERR_ARG, "%s: %d records%s, the rig has %d steps", what, n_steps, stats12 ? "" : " (null)", ns);
    for (int k = 0; k < ns; ++k)
        if (!ex_stats_valid(stats12 + (size_t)12 * k)) return fail(STITCH_ERR_ARG, "%s: step %d: a value is not finite or a standard deviation is not above 0", what, k);
    return STITCH_OK;
}

}  // namespace

extern "C" {

int stitch_rig_create_exposure(const int32_t* frame_wh, int n, int start, const stitch_panorama_step* steps, int n_steps, const stitch_rig_opts* opts,
                               const stitch_exposure_opts* exposure, stitch_rig** out) {
    return rig_create(frame_wh, n, start, steps, n_steps, opts, exposure, out);
}

int stitch_rig_from_panorama_exposure(const stitch_panorama* pano, const stitch_frame_u8* frames, int n, const stitch_rig_opts* opts,
                                      const stitch_exposure_opts* exposure, stitch_rig** out) {
    return rig_from_panorama(pano, frames, n, opts, exposure, out);
}

int stitch_dev_rig_stitch_exposure_u8(stitch_rig* rig, const stitch_frame_u8* frames, int n_sets, uint8_t* const* d_out, int32_t* set_status,
                                      stitch_seam* seams, float* stats, void* stream) {
    if (rig && (rig->in_fmt || rig->out_fmt)) return fail(STITCH_ERR_ARG, "rig_stitch: the rig has formats set (include/stitch_rig_formats.h): call stitch_dev_rig_stitch_fmt_u8");
    return rig_stitch(rig, frames, n_sets, d_out, set_status, seams, stats, stream);
}

int stitch_dev_transfer_many_u8(const uint8_t* const* d_src, const uint8_t* const* d_tem, uint8_t* const* d_out, int count, int sw, int sh, int tw, int th,
                                int stats_form, int keep_black, float* d_stats12, uint32_t* d_diag, void* stream) {
    int rc = need_device();
    if (rc) return rc;
    if (!d_src || !d_tem || !d_out || count < 1 || count > kTransferManyMax || sw <= 0 || sh <= 0 || tw <= 0 || th <= 0)
        return fail(STITCH_ERR_ARG, "transfer_many: null table, %d pairs (1 .. %d) or bad size %dx%d / %dx%d", count, kTransferManyMax, sw, sh, tw, th);
    if ((long long)sw * sh > 0x7fffffffLL || (long long)tw * th > 0x7fffffffLL)
        return fail(STITCH_ERR_ARG, "transfer_many: w*h overflows int (the reference's int product)");
    if (stats_form < 0 || stats_form > 2) return fail(STITCH_ERR_ARG, "transfer_many: stats_form %d (0 .. 2)", stats_form);
    for (int i = 0; i < count; ++i)
        if (!d_src[i] || !d_tem[i] || !d_out[i]) return fail(STITCH_ERR_ARG, "transfer_many: pair %d has a null buffer", i);
    const size_t ns = (size_t)sw * sh, nt = (size_t)tw * th, spans = (std::max(ns, nt) + EX_SPAN - 1) / EX_SPAN;
    const size_t img_bytes = sizeof(ExImage) * 2 * count, tab_bytes = img_bytes + sizeof(ExPlane) * 6 * count;
    hipStream_t s = as_stream(stream);
    std::vector<unsigned char> tab(tab_bytes);
    PanoArena A(s);
    unsigned char* d_tab = nullptr;
    float *lab = nullptr, *stats = d_stats12;
    double* sums = nullptr;
    ExSpanEntry* table = nullptr;
    if ((rc = A.take(&d_tab, tab_bytes)) || (rc = A.take(&lab, sizeof(float) * 3 * (ns + nt) * count))) return rc;
    if (!stats && (rc = A.take(&stats, sizeof(float) * 12 * count))) return rc;
    if (stats_form == STITCH_STATS_SPANS && ((rc = A.take(&sums, sizeof(double) * 6 * count * spans)) || (rc = A.take(&table, sizeof(ExSpanEntry) * 6 * count * spans))))
        return rc;
    ExImage* img = reinterpret_cast<ExImage*>(tab.data());
    ExPlane* planes = reinterpret_cast<ExPlane*>(tab.data() + img_bytes);
    for (int i = 0; i < count; ++i) {
        float* lab_s = lab + (size_t)i * 3 * (ns + nt);
        ex_fill_pair(img, planes, i, d_src[i], ns, lab_s, d_tem[i], nt, lab_s + 3 * ns, d_out[i], stats + (size_t)12 * i);
    }
    PanoWait wait{s};  // `tab` is read by its upload, and what the arena frees is idle
    HIPCHK(hipMemcpyAsync(d_tab, tab.data(), tab_bytes, hipMemcpyHostToDevice, s));
    return ex_transfer_many(reinterpret_cast<const ExImage*>(d_tab), reinterpret_cast<const ExPlane*>(d_tab + img_bytes), count, ns, nt, stats_form, keep_black, sums,
                            table, d_diag, s);
}

// ---- include/stitch_rig_exposure_temporal.h ----
int stitch_dev_transfer_given_many_u8(const uint8_t* const* d_src, uint8_t* const* d_out, int count, int w, int h, const float* d_stats12, int keep_black,
                                      void* stream) {
    if (!d_src || !d_out || !d_stats12 || count < 1 || count > kTransferManyMax || w <= 0 || h <= 0)
        return fail(STITCH_ERR_ARG, "transfer_given_many: null table or statistics, %d images (1 .. %d) or bad size %dx%d", count, kTransferManyMax, w, h);
    if ((long long)w * h > 0x7fffffffLL) return fail(STITCH_ERR_ARG, "transfer_given_many: w*h overflows int (the reference's int product)");
    for (int i = 0; i < count; ++i)
        if (!d_src[i] || !d_out[i]) return fail(STITCH_ERR_ARG, "transfer_given_many: image %d has a null buffer", i);
    int rc = need_device();
    if (rc) return rc;
    hipStream_t s = as_stream(stream);
    std::vector<ExGiven> tab((size_t)count);
    for (int i = 0; i < count; ++i) tab[i] = ExGiven{d_src[i], d_out[i]};
    PanoArena A(s);
    ExGiven* d_tab = nullptr;
    if ((rc = A.take(&d_tab, sizeof(ExGiven) * count))) return rc;
    PanoWait wait{s};  // `tab` is read by its upload, and what the arena frees is idle
    HIPCHK(hipMemcpyAsync(d_tab, tab.data(), sizeof(ExGiven) * count, hipMemcpyHostToDevice, s));
    return ex_transfer_given_many(d_tab, count, (size_t)w * h, d_stats12, 12, keep_black, s);
}

int stitch_dev_stats_filter_f32(const float* d_measured, int count, int keep, float* d_state12, int32_t* d_has, float* d_used, void* stream) {
    if (!d_measured || !d_state12 || !d_has || !d_used || count < 1)
        return fail(STITCH_ERR_ARG, "stats_filter: null buffer or %d records (1 or more)", count);
    if (keep < 0 || keep > STITCH_EXPOSURE_KEEP_MAX) return fail(STITCH_ERR_ARG, "stats_filter: keep %d (0 .. %d)", keep, STITCH_EXPOSURE_KEEP_MAX);
    const int rc = need_device();
    if (rc) return rc;
    return ex_stats_filter(d_measured, 12, d_used, 12, count, keep, d_state12, d_has, nullptr, nullptr, 0, as_stream(stream));
}

int stitch_rig_set_exposure_smoothing(stitch_rig* rig, int keep) {
    const int rc = rig_et_handle(rig, "rig_set_exposure_smoothing");
    if (rc) return rc;
    if (keep < 0 || keep > STITCH_EXPOSURE_KEEP_MAX) return fail(STITCH_ERR_ARG, "rig_set_exposure_smoothing: keep %d (0 .. %d)", keep, STITCH_EXPOSURE_KEEP_MAX);
    rig->et_keep = keep;
    return STITCH_OK;
}

int stitch_rig_reset_exposure_state(stitch_rig* rig) {
    const int rc = rig_et_handle(rig, "rig_reset_exposure_state");
    if (rc) return rc;
    rig->et_state.clear();
    rig->et_has.clear();
    return STITCH_OK;
}

int stitch_rig_clear_exposure_smoothing(stitch_rig* rig) {
    const int rc = rig_et_handle(rig, "rig_clear_exposure_smoothing");
    if (rc) return rc;
    rig->et_keep = -1;
    return stitch_rig_reset_exposure_state(rig);
}

int stitch_rig_prime_exposure_state(stitch_rig* rig, const float* stats12, int n_steps) {
    int rc = rig_et_handle(rig, "rig_prime_exposure_state");
    if (rc || (rc = rig_et_records(rig, stats12, n_steps, "rig_prime_exposure_state"))) return rc;
    rig->et_state.assign(stats12, stats12 + (size_t)12 * n_steps);
    rig->et_has.assign((size_t)n_steps, 1);
    return STITCH_OK;
}

int stitch_rig_exposure_smoothing(const stitch_rig* rig, int* keep, int32_t* has) {
    const int rc = rig_et_handle(rig, "rig_exposure_smoothing");
    if (rc) return rc;
    if (keep) *keep = rig->et_keep;
    for (size_t k = 0; has && k < rig->steps.size(); ++k) has[k] = k < rig->et_has.size() && rig->et_has[k] ? 1 : 0;
    return STITCH_OK;
}

int stitch_rig_exposure_state(const stitch_rig* rig, float* out, int n_steps) {
    const int rc = rig_et_handle(rig, "rig_exposure_state");
    if (rc) return rc;
    const int ns = (int)rig->steps.size();
    if (n_steps != ns || (ns > 0 && !out)) return fail(STITCH_ERR_ARG, "rig_exposure_state: room for %d records%s, the rig has %d steps", n_steps, out ? "" : " (null)", ns);
    for (int k = 0; k < ns; ++k)
        for (int j = 0; j < 12; ++j) out[12 * k + j] = (size_t)k < rig->et_has.size() && rig->et_has[k] ? rig->et_state[(size_t)12 * k + j] : 0.0f;
    return STITCH_OK;
}

int stitch_rig_fix_exposure(stitch_rig* rig, const float* stats12, int n_steps) {
    int rc = rig_et_handle(rig, "rig_fix_exposure");
    if (rc || (rc = rig_et_records(rig, stats12, n_steps, "rig_fix_exposure"))) return rc;
    rig->et_fixed.assign(stats12, stats12 + (size_t)12 * n_steps);
    return STITCH_OK;
}

int stitch_rig_clear_fixed_exposure(stitch_rig* rig) {
    const int rc = rig_et_handle(rig, "rig_clear_fixed_exposure");
    if (rc) return rc;
    rig->et_fixed.clear();
    return STITCH_OK;
}

int stitch_rig_fixed_exposure(const stitch_rig* rig, float* out, int* n_steps) {
    const int rc = rig_et_handle(rig, "rig_fixed_exposure");
    if (rc) return rc;
    if (n_steps) *n_steps = (int)(rig->et_fixed.size() / 12);
    if (out) std::copy(rig->et_fixed.begin(), rig->et_fixed.end(), out);
    return STITCH_OK;
}

int stitch_rig_last_used_stats(const stitch_rig* rig, float* out, size_t cap_floats, int* n_sets, int* n_steps) {
    const int rc = rig_et_handle(rig, "rig_last_used_stats");
    if (rc) return rc;
    if (n_sets) *n_sets = rig->et_last_sets;
    if (n_steps) *n_steps = (int)rig->steps.size();
    if (out) std::copy_n(rig->et_last_used.begin(), std::min(cap_floats, rig->et_last_used.size()), out);
    return STITCH_OK;
}

}  // extern "C"
