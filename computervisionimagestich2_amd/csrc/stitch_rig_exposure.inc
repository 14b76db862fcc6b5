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

// One transfer over `count` pairs of the tables, every source of ns pixels and every template of nt: the launches of
// stitch_dev_transfer_form_u8, each over all images or planes.  sums / table (form 2): 6 * count rows of ceil(max(ns, nt) / EX_SPAN).
int ex_transfer_many(const ExImage* d_img, const ExPlane* d_planes, int count, size_t ns, size_t nt, int form, int keep_black, double* sums, ExSpanEntry* table,
                     uint32_t* d_diag, hipStream_t s) {
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
    k_ex_apply_many<<<dim3((unsigned)eq_grid(ns), (unsigned)count), 256, 0, s>>>(d_img, 2, k, keep_black);
    return launch_check("k_ex_apply_many");
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

// The tables of all steps: per step 2 * max_sets images, then per step 6 * max_sets planes.  Set i of a sequence is pair i of its
// step, so a sequence of m < max_sets sets reads a prefix.
size_t rig_ex_table_bytes(const stitch_rig* R) {
    return R->ex.mode ? R->steps.size() * (size_t)R->max_sets * (2 * sizeof(ExImage) + 6 * sizeof(ExPlane)) : 0;
}

void rig_ex_fill_tables(const stitch_rig* R, unsigned char* host) {
    const int S = R->max_sets, K = (int)R->steps.size();
    ExImage* img = reinterpret_cast<ExImage*>(host);
    ExPlane* planes = reinterpret_cast<ExPlane*>(host + (size_t)K * S * 2 * sizeof(ExImage));
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
        }
    }
}

int rig_ex_transfer(stitch_rig* R, const unsigned char* d_tables, int k, int m, hipStream_t s) {
    const int S = R->max_sets, K = (int)R->steps.size(), f = R->steps[k].dst;
    const ExImage* d_img = reinterpret_cast<const ExImage*>(d_tables) + (size_t)k * S * 2;
    const ExPlane* d_planes = reinterpret_cast<const ExPlane*>(d_tables + (size_t)K * S * 2 * sizeof(ExImage)) + (size_t)k * S * 6;
    const uint8_t* tem = nullptr;
    size_t tem_stride = 0;
    int tw = 0, th = 0;
    rig_ex_template(R, k, &tem, &tem_stride, &tw, &th);
    return ex_transfer_many(d_img, d_planes, m, (size_t)R->fw[f] * R->fh[f], (size_t)tw * th, R->ex.stats_form, R->ex.keep_black, R->ex_sums,
                            static_cast<ExSpanEntry*>(R->ex_table), nullptr, s);
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

}  // extern "C"
