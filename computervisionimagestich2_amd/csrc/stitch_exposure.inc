// stitch_exposure.inc -- exposure-matched panoramas (include/stitch_exposure.h; kernels in k_exposure.inc, DESIGN.md 14).
// Included at the end of stitch_hip.hip (one translation unit).  The chain itself is pano_steps of stitch_panorama.inc, which
// runs one stitch_dev_transfer_form_u8 per step where the mode asks for it.
namespace {

// Mean and sd of the planes of `a` in the given form, enqueued on s.  Form 2 takes its span sums and span table from the arena
// (stream-ordered, freed when the caller's arena goes).  No workgroup waits for another: the launches of one stream are the order.
int ex_run_stats(const ExArgs& a, int n_planes, int form, uint32_t* d_diag, PanoArena& A, hipStream_t s) {
    int rc = STITCH_OK;
    if (d_diag) HIPCHK(hipMemsetAsync(d_diag, 0, sizeof(uint32_t) * EX_DIAG_N * n_planes, s));
    if (form == STITCH_STATS_SERIAL) {
        k_ex_stats_serial<<<n_planes, 64, 0, s>>>(a);
        return launch_check("k_ex_stats_serial");
    }
    if (form == STITCH_STATS_SCAN) {
        k_ex_walk<<<n_planes, EX_T, 0, s>>>(a, 0, 0, nullptr, d_diag);
        return launch_check("k_ex_walk");
    }
    size_t max_spans = 1;
    for (int i = 0; i < n_planes; ++i) max_spans = std::max(max_spans, (size_t)((a.n[i] + EX_SPAN - 1) / EX_SPAN));
    double* sums = nullptr;
    ExSpanEntry* table = nullptr;
    if ((rc = A.take(&sums, sizeof(double) * max_spans * n_planes)) || (rc = A.take(&table, sizeof(ExSpanEntry) * max_spans * n_planes))) return rc;
    const dim3 grid((unsigned)max_spans, (unsigned)n_planes);
    for (int pass = 0; pass < 2; ++pass) {
        k_ex_span_sums<<<grid, EX_T, 0, s>>>(a, pass, (int)max_spans, sums);
        if ((rc = launch_check("k_ex_span_sums"))) return rc;
        k_ex_span_maps<<<grid, EX_T, 0, s>>>(a, pass, (int)max_spans, sums, table);
        if ((rc = launch_check("k_ex_span_maps"))) return rc;
        k_ex_walk<<<n_planes, EX_T, 0, s>>>(a, pass, (int)max_spans, table, d_diag);
        if ((rc = launch_check("k_ex_walk"))) return rc;
    }
    return STITCH_OK;
}

// The transfer's constants, as stitch_dev_transfer_u8 forms them.
TrK ex_constants() {
    TrK k{};
    k.a1 = (float)(1.0 / std::sqrt(3.0));
    k.b1 = (float)(1.0 / std::sqrt(6.0));
    k.c1 = (float)(1.0 / std::sqrt(2.0));
    k.a2 = (float)(std::sqrt(3.0) / 3.0);
    k.b2 = (float)(std::sqrt(6.0) / 6.0);
    k.c2 = (float)(std::sqrt(2.0) / 2.0);
    k.ln10 = 2.302585092994046;  // log(10)
    return k;
}

}  // namespace

extern "C" {

void stitch_exposure_opts_default(stitch_exposure_opts* o) {
    if (!o) return;
    o->mode = 1;
    o->stats_form = STITCH_STATS_SPANS;
    o->keep_black = 1;
}

int stitch_dev_running_stats_f32(const float* const* d_planes, const size_t* lengths, const float* counts, int n_planes, int form, float* d_mean,
                                 float* d_sd, uint32_t* d_diag, void* stream) {
    int rc = need_device();
    if (rc) return rc;
    if (!d_planes || !lengths || !counts || !d_mean || !d_sd || n_planes < 1 || n_planes > 6)
        return fail(STITCH_ERR_ARG, "running_stats: a null argument or %d planes (1 .. 6)", n_planes);
    if (form < 0 || form > 2) return fail(STITCH_ERR_ARG, "running_stats: form %d (0 .. 2)", form);
    ExArgs a;
    std::memset(&a, 0, sizeof a);
    for (int i = 0; i < n_planes; ++i) {
        if (!d_planes[i] || lengths[i] < 1 || lengths[i] > ((size_t)1 << 40)) return fail(STITCH_ERR_ARG, "running_stats: plane %d is null, empty or too long", i);
        a.p[i] = d_planes[i];
        a.n[i] = lengths[i];
        a.cnt[i] = counts[i];
        a.mean[i] = d_mean + i;
        a.sd[i] = d_sd + i;
    }
    hipStream_t s = as_stream(stream);
    PanoArena A(s);
    return ex_run_stats(a, n_planes, form, d_diag, A, s);
}

int stitch_dev_transfer_form_u8(const uint8_t* d_src, int sw, int sh, const uint8_t* d_tem, int tw, int th, uint8_t* d_out, float* d_stats12,
                                int stats_form, int keep_black, uint32_t* d_diag, void* stream) {
    int rc = need_device();
    if (rc) return rc;
    if (!d_src || !d_tem || !d_out || sw <= 0 || sh <= 0 || tw <= 0 || th <= 0) return fail(STITCH_ERR_ARG, "transfer: null buffer or bad size");
    if ((long long)sw * sh > 0x7fffffffLL || (long long)tw * th > 0x7fffffffLL)
        return fail(STITCH_ERR_ARG, "transfer: w*h overflows int (the reference's int product)");
    if (stats_form < 0 || stats_form > 2) return fail(STITCH_ERR_ARG, "transfer: stats_form %d (0 .. 2)", stats_form);
    const size_t ns = (size_t)sw * sh, nt = (size_t)tw * th;
    const TrK k = ex_constants();
    hipStream_t s = as_stream(stream);
    PanoArena A(s);
    float* scratch = nullptr;
    if ((rc = A.take(&scratch, sizeof(float) * (3 * (ns + nt) + 16)))) return rc;
    float *lab_s = scratch, *lab_t = scratch + 3 * ns, *stats = scratch + 3 * (ns + nt);
    k_tr_to_lab<<<eq_grid(ns), 256, 0, s>>>(d_src, ns, k, lab_s);
    k_tr_to_lab<<<eq_grid(nt), 256, 0, s>>>(d_tem, nt, k, lab_t);
    if ((rc = launch_check("k_tr_to_lab"))) return rc;
    ExArgs a;
    std::memset(&a, 0, sizeof a);
    for (int i = 0; i < 6; ++i) {  // stats = [mean_src[3], sd_src[3], mean_tem[3], sd_tem[3]]
        const bool is_t = i >= 3;
        a.n[i] = is_t ? nt : ns;
        a.p[i] = (is_t ? lab_t : lab_s) + (size_t)(i % 3) * a.n[i];
        a.cnt[i] = is_t ? (float)(tw * th) : (float)(sw * sh);
        a.mean[i] = stats + (is_t ? 6 : 0) + i % 3;
        a.sd[i] = stats + (is_t ? 9 : 3) + i % 3;
    }
    if ((rc = ex_run_stats(a, 6, stats_form, d_diag, A, s))) return rc;
    k_ex_apply<<<eq_grid(ns), 256, 0, s>>>(lab_s, ns, stats, k, keep_black ? d_src : nullptr, d_out);
    if ((rc = launch_check("k_ex_apply"))) return rc;
    if (d_stats12) HIPCHK(hipMemcpyAsync(d_stats12, stats, sizeof(float) * 12, hipMemcpyDeviceToDevice, s));
    return STITCH_OK;
}

int stitch_dev_panorama_exposure_from_features_u8(const stitch_frame_u8* frames, const stitch_feature_set* feats, int n, const stitch_panorama_opts* opts,
                                                  const stitch_exposure_opts* exposure, void* stream, stitch_panorama** out) {
    return pano_from_features(frames, feats, n, opts, exposure, stream, out);
}

int stitch_dev_panorama_exposure_u8(const stitch_frame_u8* frames, int n, const stitch_panorama_opts* opts, const stitch_exposure_opts* exposure,
                                    void* stream, stitch_panorama** out) {
    return pano_from_frames(frames, n, opts, exposure, stream, out);
}

int stitch_panorama_exposure_u8(const stitch_frame_u8* frames, int n, const stitch_panorama_opts* opts, const stitch_exposure_opts* exposure,
                                stitch_panorama** out) {
    return pano_from_host_frames(frames, n, opts, exposure, out);
}

int stitch_panorama_exposure_stats(const stitch_panorama* pano, int k, float stats[12]) {
    if (!pano || !stats || k < 0 || k >= (int)pano->steps.size()) return fail(STITCH_ERR_ARG, "panorama_exposure_stats: bad argument (step %d)", k);
    if (!pano->exposure_mode) return fail(STITCH_ERR_ARG, "panorama_exposure_stats: the panorama was made without a transfer (mode 0)");
    std::memcpy(stats, pano->exposure_stats.data() + (size_t)12 * k, sizeof(float) * 12);
    return STITCH_OK;
}

int stitch_panorama_exposure_frame_copy(const stitch_panorama* pano, int k, void* dst, size_t capacity, int dst_is_device, void* stream) {
    if (!pano || !dst || k < 0 || k >= (int)pano->steps.size()) return fail(STITCH_ERR_ARG, "panorama_exposure_frame_copy: bad argument (step %d)", k);
    if (k >= (int)pano->exposure_px.size()) return fail(STITCH_ERR_ARG, "panorama_exposure_frame_copy: step %d's frame was not kept (mode 0 or keep_steps = 0)", k);
    const size_t bytes = (size_t)3 * pano->exposure_wh[2 * k] * pano->exposure_wh[2 * k + 1];
    if (capacity < bytes) return fail(STITCH_ERR_ARG, "panorama_exposure_frame_copy: %zu bytes needed, the destination holds %zu", bytes, capacity);
    hipStream_t s = as_stream(stream);
    HIPCHK(hipMemcpyAsync(dst, pano->exposure_px[k], bytes, dst_is_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));  // the handle may be destroyed at once
    return STITCH_OK;
}

}  // extern "C"
