// stitch_rig_seams.inc -- fixed seams for a rig: given or geometric, with coverage masks (include/stitch_rig_seams.h; kernels in
// k_rig_seams.inc).  Included at the end of stitch_hip.hip (one translation unit).
//
// A stated seam is its four integers; everything else of the record comes from seam_finish (k_compose.inc), the function that ends
// the device's scan, compiled for the host here -- so the host's record, the record k_seam_given writes and the record a scan with
// these sums would have written are one computation.
namespace {

int rig_seam_rule(const stitch_rig* R) { return R->has_blend ? R->blend.seam_rule : 0; }

// checked sums -> the public record under `rule`
int seam_from_sums(long long sum_a_x, long long n_a, long long sum_ov_x, long long n_ov, int rule, int cw, const char* what, int index, stitch_seam* out) {
    const int rc = seam_check_sums(sum_a_x, n_a, sum_ov_x, n_ov, cw, what, index);
    if (rc) return rc;
    seam_to_public(seam_finish((int)sum_a_x, (int)n_a, (int)sum_ov_x, (int)n_ov, rule, cw), out);
    return STITCH_OK;
}

inline int cover_wpr(int w) { return (w + 63) / 64; }
inline dim3 cover_grid(int wpr, int h) { return dim3((unsigned)((wpr + 3) / 4), (unsigned)h); }

// The coverage planes of a rig and the scan of every step over them, on the current device, once.  Waits for `s` when it computes.
int rig_cover(stitch_rig* R, hipStream_t s) {
    int dev = -1;
    HIPCHK(hipGetDevice(&dev));
    if (R->cover_device >= 0) {
        if (dev != R->cover_device) return fail(STITCH_ERR_ARG, "rig: its coverage planes belong to device %d, the current device is %d", R->cover_device, dev);
        return STITCH_OK;
    }
    const int ns = (int)R->steps.size();
    std::vector<size_t> proj_at((size_t)R->n, 0), step_at((size_t)ns, 0);
    std::vector<int> first;  // the frames that own a C_proj plane: one per distinct size
    size_t words = 0;
    for (int f : R->needed) {
        int owner = -1;
        for (int g : first)
            if (R->fw[g] == R->fw[f] && R->fh[g] == R->fh[f]) owner = g;
        if (owner >= 0) {
            proj_at[f] = proj_at[owner];
            continue;
        }
        first.push_back(f);
        proj_at[f] = words;
        words += (size_t)cover_wpr(R->fw[f]) * R->fh[f];
    }
    for (int k = 0; k < ns; ++k) {
        step_at[k] = words;
        words += (size_t)3 * cover_wpr(R->steps[k].geom.cw) * R->steps[k].geom.ch;
    }
    unsigned long long* base = nullptr;
    HIPCHK(hipMalloc((void**)&base, sizeof(unsigned long long) * words + sizeof(SeamDev) * std::max(ns, 1)));
    struct Guard {
        void* p;
        ~Guard() {
            if (p) (void)hipFree(p);
        }
    } guard{base};
    SeamDev* d_seams = reinterpret_cast<SeamDev*>(base + words);
    for (int f : first) {
        const ProjParams pp = proj_params(R->fw[f], R->fh[f], R->fov_deg);
        const int wpr = cover_wpr(R->fw[f]);
        k_cover_proj<<<cover_grid(wpr, R->fh[f]), 256, 0, s>>>(base + proj_at[f], wpr, R->fw[f], R->fh[f], pp.flag, pp.width, pp.height, pp.r);
    }
    const unsigned long long* m_cov = base + proj_at[R->start];
    int mw = R->fw[R->start], mh = R->fh[R->start];
    for (int k = 0; k < ns; ++k) {
        const stitch_panorama_step& st = R->steps[k];
        CoverStep c;
        std::memcpy(c.map.p, st.p_bwd, sizeof c.map.p);
        c.offx = st.geom.min_x;
        c.offy = st.geom.min_y;
        c.fw = R->fw[st.dst];
        c.fh = R->fh[st.dst];
        c.fwpr = cover_wpr(c.fw);
        c.mw = mw;
        c.mh = mh;
        c.mwpr = cover_wpr(mw);
        c.ox = st.geom.ox;
        c.oy = st.geom.oy;
        c.cw = st.geom.cw;
        c.ch = st.geom.ch;
        c.wpr = cover_wpr(c.cw);
        const size_t plane = (size_t)c.wpr * c.ch;
        unsigned long long *A = base + step_at[k], *B = A + plane, *U = B + plane;
        k_cover_step<<<cover_grid(c.wpr, c.ch), 256, 0, s>>>(c, base + proj_at[st.dst], m_cov, A, B, U);
        k_cover_seam<<<1, 256, 0, s>>>(A, B, c.cw, c.ch, c.wpr, rig_seam_rule(R), d_seams + k);
        m_cov = U;
        mw = c.cw;
        mh = c.ch;
    }
    int rc = launch_check("rig coverage");
    if (rc) return rc;
    std::vector<SeamDev> seams((size_t)ns);
    if (ns) HIPCHK(hipMemcpyAsync(seams.data(), d_seams, sizeof(SeamDev) * ns, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    guard.p = nullptr;
    R->cover = base;
    R->cover_proj = proj_at;
    R->cover_step = step_at;
    R->cover_seams = seams;
    R->cover_device = dev;
    return STITCH_OK;
}

template <typename PX>
int pairs_seamed(stitch_plan* plan, const stitch_pair_desc* pairs, int n, const stitch_seam* seams, void* stream) {
    if (!seams) return fail(STITCH_ERR_ARG, "pairs_seamed: null seam array");
    return dev_pairs<PX>(plan, pairs, n, stream, seams);
}

}  // namespace

extern "C" {

int stitch_seam_from_sums(int32_t sum_a_x, int32_t n_a, int32_t sum_ov_x, int32_t n_ov, int seam_rule, int cw, stitch_seam* out) {
    if (!out || seam_rule < 0 || seam_rule > 1) return fail(STITCH_ERR_ARG, "seam_from_sums: null output or seam_rule %d outside 0 .. 1", seam_rule);
    return seam_from_sums(sum_a_x, n_a, sum_ov_x, n_ov, seam_rule, cw, "seam_from_sums: record", 0, out);
}

int stitch_dev_pairs_seamed_u8(stitch_plan* plan, const stitch_pair_desc* pairs, int n, const stitch_seam* seams, void* stream) {
    return pairs_seamed<uint8_t>(plan, pairs, n, seams, stream);
}
int stitch_dev_pairs_seamed_f32(stitch_plan* plan, const stitch_pair_desc* pairs, int n, const stitch_seam* seams, void* stream) {
    return pairs_seamed<float>(plan, pairs, n, seams, stream);
}

int stitch_rig_fix_seams(stitch_rig* rig, const stitch_seam* seams, int n_steps) {
    if (!rig) return fail(STITCH_ERR_ARG, "rig_fix_seams: null handle");
    const int ns = (int)rig->steps.size();
    if (n_steps != ns || (ns > 0 && !seams)) return fail(STITCH_ERR_ARG, "rig_fix_seams: %d records%s, the rig has %d steps", n_steps, seams ? "" : " (null)", ns);
    std::vector<stitch_seam> fixed((size_t)ns);
    for (int k = 0; k < ns; ++k) {
        const int rc = seam_from_sums(seams[k].sum_a_x, seams[k].n_a, seams[k].sum_ov_x, seams[k].n_ov, rig_seam_rule(rig), rig->steps[k].geom.cw,
                                      "rig_fix_seams: step", k, &fixed[k]);
        if (rc) return rc;
    }
    rig->fixed = fixed;
    return STITCH_OK;
}

int stitch_rig_clear_seams(stitch_rig* rig) {
    if (!rig) return fail(STITCH_ERR_ARG, "rig_clear_seams: null handle");
    rig->fixed.clear();
    return STITCH_OK;
}

int stitch_rig_seams(const stitch_rig* rig, stitch_seam* out, int cap) {
    if (!rig || cap < 0 || (cap > 0 && !out)) return fail(STITCH_ERR_ARG, "rig_seams: null handle, or a capacity of %d without an output", cap);
    const int nf = (int)rig->fixed.size();
    for (int k = 0; k < std::min(nf, cap); ++k) out[k] = rig->fixed[k];
    return nf;
}

int stitch_dev_rig_geometric_seams(stitch_rig* rig, stitch_seam* seams_out, void* stream) {
    if (!rig) return fail(STITCH_ERR_ARG, "rig_geometric_seams: null handle");
    int rc = need_device();
    if (rc) return rc;
    if ((rc = rig_cover(rig, as_stream(stream)))) return rc;
    HIPCHK(hipStreamSynchronize(as_stream(stream)));  // the planes may have been there: the call waits either way
    const int ns = (int)rig->steps.size();
    std::vector<stitch_seam> fixed((size_t)ns);
    for (int k = 0; k < ns; ++k) {
        const SeamDev& sd = rig->cover_seams[k];
        if (sd.status == -2)
            return fail(STITCH_ERR_EMPTY_MIDROW, "rig_geometric_seams: step %d (frame %d): the warped frame's footprint misses the canvas's middle row", k,
                        rig->steps[k].dst);
        if (sd.status == -3)
            return fail(STITCH_ERR_ZERO_OVERLAP, "rig_geometric_seams: step %d (frame %d): the footprints of the frame and of the mosaic do not overlap on the middle row",
                        k, rig->steps[k].dst);
        if ((rc = seam_from_sums(sd.sum_a_x, sd.n_a, sd.sum_ov_x, sd.n_ov, rig_seam_rule(rig), rig->steps[k].geom.cw, "rig_geometric_seams: step", k, &fixed[k])))
            return rc;
    }
    rig->fixed = fixed;
    for (int k = 0; seams_out && k < ns; ++k) seams_out[k] = fixed[k];
    return STITCH_OK;
}

int stitch_rig_step_canvas(const stitch_rig* rig, int step, int* cw, int* ch) {
    if (!rig || !cw || !ch) return fail(STITCH_ERR_ARG, "rig_step_canvas: null argument");
    const int ns = (int)rig->steps.size();
    if (step < -1 || step >= ns) return fail(STITCH_ERR_ARG, "rig_step_canvas: step %d outside -1 .. %d", step, ns - 1);
    *cw = step < 0 ? rig->out_w : rig->steps[step].geom.cw;
    *ch = step < 0 ? rig->out_h : rig->steps[step].geom.ch;
    return STITCH_OK;
}

int stitch_dev_rig_coverage_u8(stitch_rig* rig, int step, int which, uint8_t* d_mask, void* stream) {
    if (!rig || !d_mask) return fail(STITCH_ERR_ARG, "rig_coverage: null handle or mask");
    const int ns = (int)rig->steps.size();
    if (step < -1 || step >= ns)
        return fail(STITCH_ERR_ARG, "rig_coverage: step %d outside -1 .. %d", step, ns - 1);
    if (which < 0 || which > 2) return fail(STITCH_ERR_ARG, "rig_coverage: which = %d (0: the warped frame, 1: the moved mosaic, 2: either)", which);
    int rc = need_device();
    if (rc) return rc;
    hipStream_t s = as_stream(stream);
    if ((rc = rig_cover(rig, s))) return rc;
    if (ns == 0) {
        const int w = rig->fw[rig->start], h = rig->fh[rig->start];
        k_cover_bytes<<<grid_xy(w, h), 256, 0, s>>>(rig->cover + rig->cover_proj[rig->start], cover_wpr(w), w, h, d_mask);
    } else {
        const int k = step < 0 ? ns - 1 : step, w = rig->steps[k].geom.cw, h = rig->steps[k].geom.ch, wpr = cover_wpr(w);
        k_cover_bytes<<<grid_xy(w, h), 256, 0, s>>>(rig->cover + rig->cover_step[k] + (size_t)which * wpr * h, wpr, w, h, d_mask);
    }
    return launch_check("k_cover_bytes");
}

}  // extern "C"
