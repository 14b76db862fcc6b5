// stitch_rig_seam_paths.inc -- path seams for a rig (include/stitch_seam_path.h, which is the specification; the pair calls in
// stitch_seam_path.inc, kernels in k_seam_path.inc).  Included at the end of stitch_hip.hip (one translation unit).
//
// The rig's side is three hooks that rig_stitch (stitch_rig.inc) calls only while a mode is set: the workspaces once per rig, per
// step one finder sequence over the m sets in flight (mode 1) and the blend along the paths on the masked twin of the step's plan --
// from the pair descriptors the step's blend would have received -- and the one copy that takes a sequence's paths to the host.
// Anchored (include/stitch_seam_anchor.h), the same hooks: the step's dynamic programmes take the temporal term -- PER_CALL in the one
// launch over the sets, every set on the rig's anchor; PER_SET one launch of one workgroup per set, set i on set i - 1's rows of
// sp_paths and set 0 on the rig's anchor -- and the collect hook makes the last set's rows the rig's anchor by a device copy.
namespace {

// the rows of a set's paths, step after step
void rig_sp_rows(stitch_rig* R) {
    if (!R->sp_row_at.empty() || R->steps.empty()) return;
    size_t rows = 0;
    for (const stitch_panorama_step& st : R->steps) {
        R->sp_row_at.push_back(rows);
        rows += (size_t)st.geom.ch;
    }
    R->sp_rows = rows;
}

int rig_sp_prepare(stitch_rig* R, hipStream_t s) {
    const int ns = (int)R->steps.size();
    int rc = rig_cover(R, s);  // the branch of a step is that of its geometric seam; mode 1 reads the planes as well
    if (rc) return rc;
    for (int k = 0; k < ns; ++k) {
        const SeamDev& sd = R->cover_seams[k];
        if (sd.status == -2)
            return fail(STITCH_ERR_EMPTY_MIDROW, "rig seam paths: step %d (frame %d): the warped frame's footprint misses the canvas's middle row", k, R->steps[k].dst);
        if (sd.status == -3)
            return fail(STITCH_ERR_ZERO_OVERLAP, "rig seam paths: step %d (frame %d): the footprints of the frame and of the mosaic do not overlap on the middle row", k,
                        R->steps[k].dst);
    }
    rig_sp_rows(R);
    if (R->sp_plans.empty()) {
        std::vector<stitch_plan*> twins;
        for (const stitch_plan* p : R->plans) {
            stitch_plan* t = nullptr;
            if ((rc = stitch_plan_create_masked(p->cw, p->ch, R->blend_ptr(), R->max_sets, &t))) {
                for (stitch_plan* q : twins) stitch_plan_destroy(q);
                return rc;
            }
            twins.push_back(t);
        }
        R->sp_plans = twins;
    }
    if (R->sp_mode == 2) {
        if (!R->sp_fixed_dev) HIPCHK(hipMalloc((void**)&R->sp_fixed_dev, sizeof(int32_t) * R->sp_rows));
        if (!R->sp_fixed_up) {
            HIPCHK(hipMemcpyAsync(R->sp_fixed_dev, R->sp_fixed.data(), sizeof(int32_t) * R->sp_rows, hipMemcpyHostToDevice, s));
            HIPCHK(hipStreamSynchronize(s));  // sp_fixed may change as soon as the call returns
            R->sp_fixed_up = true;
        }
        return STITCH_OK;
    }
    if (!R->sp_paths) HIPCHK(hipMalloc((void**)&R->sp_paths, sizeof(int32_t) * R->sp_rows * R->max_sets));
    if (!R->sp_costs) HIPCHK(hipMalloc((void**)&R->sp_costs, sizeof(unsigned long long) * ns * R->max_sets));
    if (!R->sp_scratch) {
        size_t states = 0;
        for (const stitch_panorama_step& st : R->steps) states = std::max(states, (size_t)(st.geom.cw + 1) * st.geom.ch);
        HIPCHK(hipMalloc(&R->sp_scratch, (sizeof(unsigned) + 1) * states * R->max_sets));
    }
    if (!R->sa_active()) return STITCH_OK;
    if (!R->sa_dev) HIPCHK(hipMalloc((void**)&R->sa_dev, sizeof(int32_t) * R->sp_rows));
    if (!R->sa_moved) HIPCHK(hipMalloc((void**)&R->sa_moved, sizeof(unsigned long long) * ns * R->max_sets));
    if (R->sa_live && !R->sa_prime.empty()) {
        HIPCHK(hipMemcpyAsync(R->sa_dev, R->sa_prime.data(), sizeof(int32_t) * R->sp_rows, hipMemcpyHostToDevice, s));
        HIPCHK(hipStreamSynchronize(s));  // sa_prime is released below
    }
    R->sa_prime.clear();
    return STITCH_OK;
}

// the dynamic programmes of step k over the m sets in flight, with the temporal term
int rig_sa_dp(stitch_rig* R, const unsigned* d_cost, uint8_t* d_pred, int k, int m, hipStream_t s) {
    const int ns = (int)R->steps.size(), cw = R->steps[k].geom.cw, ch = R->steps[k].geom.ch;
    const size_t states = (size_t)(cw + 1) * ch;
    int32_t* paths = R->sp_paths + R->sp_row_at[k];
    uint64_t* costs = reinterpret_cast<uint64_t*>(R->sp_costs) + k;
    unsigned long long* moved = R->sa_moved + k;
    const int32_t* own = R->sa_live ? R->sa_dev + R->sp_row_at[k] : nullptr;
    SeamAnchor an{nullptr, own, 0, (unsigned)R->sa_opts.weight, (unsigned)R->sa_opts.cap, moved, (size_t)ns};
    if (R->sa_opts.policy == STITCH_SEAM_ANCHOR_PER_CALL)
        return seam_path_dp(d_cost, m, cw, ch, R->sp_opts.max_step, d_pred, paths, R->sp_rows, costs, (size_t)ns, s, &an);
    for (int i = 0; i < m; ++i) {  // set i reads the rows set i - 1 wrote: the launches follow each other on the stream
        an.base = i ? paths + (size_t)(i - 1) * R->sp_rows : own;
        an.moved = moved + (size_t)i * ns;
        int rc = seam_path_dp(d_cost + states * i, 1, cw, ch, R->sp_opts.max_step, d_pred + states * i, paths + (size_t)i * R->sp_rows, R->sp_rows, costs + (size_t)i * ns,
                              (size_t)ns, s, &an);
        if (rc) return rc;
    }
    return STITCH_OK;
}

int rig_sp_step(stitch_rig* R, const stitch_pair_desc* pd, int k, int m, hipStream_t s) {
    const int ns = (int)R->steps.size(), cw = R->steps[k].geom.cw, ch = R->steps[k].geom.ch, wpr = cover_wpr(cw);
    const int branch = R->cover_seams[k].branch;
    const int32_t* paths[MAXB];
    int32_t branches[MAXB];
    if (R->sp_mode == 1) {
        const unsigned long long* A = R->cover + R->cover_step[k];
        const size_t states = (size_t)(cw + 1) * ch;
        unsigned* d_cost = static_cast<unsigned*>(R->sp_scratch);
        uint8_t* d_pred = reinterpret_cast<uint8_t*>(d_cost + states * R->max_sets);
        SeamPathArgs a;
        for (int i = 0; i < m; ++i) a.p[i] = seam_path_pair(pd[i], A, A + (size_t)wpr * ch, branch);
        for (int i = m; i < MAXB; ++i) a.p[i] = a.p[0];
        k_seam_path_cost_step<<<dim3((unsigned)ch, (unsigned)m), SP_CT, 0, s>>>(a, cw, ch, wpr, R->sp_opts.margin, d_cost);
        int rc = launch_check("k_seam_path_cost_step");
        if (rc) return rc;
        if (R->sa_active()) {
            if ((rc = rig_sa_dp(R, d_cost, d_pred, k, m, s))) return rc;
        } else if ((rc = seam_path_dp(d_cost, m, cw, ch, R->sp_opts.max_step, d_pred, R->sp_paths + R->sp_row_at[k], R->sp_rows,
                                      reinterpret_cast<uint64_t*>(R->sp_costs) + k, (size_t)ns, s)))
            return rc;
    }
    for (int i = 0; i < m; ++i) {
        paths[i] = R->sp_mode == 1 ? R->sp_paths + (size_t)i * R->sp_rows + R->sp_row_at[k] : R->sp_fixed_dev + R->sp_row_at[k];
        branches[i] = branch;
    }
    return stitch_dev_pairs_pathed_u8(R->sp_plans[R->plan_of_step[k]], pd, m, paths, branches, s);
}

// (h_moved arrives zeroed; last: this is the call's last sequence)
int rig_sp_collect(stitch_rig* R, int32_t* h_paths, uint64_t* h_costs, uint64_t* h_moved, int m, bool last, hipStream_t s) {
    const size_t ns = R->steps.size();
    if (R->sp_mode == 2) {  // the fixed paths are every set's; no cost is computed
        for (int i = 0; i < m; ++i) std::memcpy(h_paths + (size_t)i * R->sp_rows, R->sp_fixed.data(), sizeof(int32_t) * R->sp_rows);
        std::fill(h_costs, h_costs + ns * m, (uint64_t)0);
        return STITCH_OK;
    }
    HIPCHK(hipMemcpyAsync(h_paths, R->sp_paths, sizeof(int32_t) * R->sp_rows * m, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(h_costs, R->sp_costs, sizeof(uint64_t) * ns * m, hipMemcpyDeviceToHost, s));
    if (!R->sa_active()) return STITCH_OK;
    HIPCHK(hipMemcpyAsync(h_moved, R->sa_moved, sizeof(uint64_t) * ns * m, hipMemcpyDeviceToHost, s));
    // the last set's rows become the anchor before the next sequence overwrites sp_paths: PER_SET after every sequence, PER_CALL --
    // whose sets all read the previous call's -- after the last
    if (R->sa_opts.policy == STITCH_SEAM_ANCHOR_PER_SET || last) {
        HIPCHK(hipMemcpyAsync(R->sa_dev, R->sp_paths + (size_t)(m - 1) * R->sp_rows, sizeof(int32_t) * R->sp_rows, hipMemcpyDeviceToDevice, s));
        if (R->sa_opts.policy == STITCH_SEAM_ANCHOR_PER_SET) R->sa_live = true;
    }
    return STITCH_OK;
}

}  // namespace

extern "C" {

int stitch_rig_set_seam_paths(stitch_rig* rig, const stitch_seam_path_opts* opts) {
    if (!rig) return fail(STITCH_ERR_ARG, "rig_set_seam_paths: null handle");
    stitch_seam_path_opts o;
    stitch_seam_path_opts_default(&o);
    if (opts) o = *opts;
    if (!seam_path_opts_ok(o))
        return fail(STITCH_ERR_ARG, "rig_set_seam_paths: max_step %d outside 1 .. %d or margin %d outside 0 .. %d", o.max_step, SP_MAXK, o.margin, SP_MAXM);
    for (size_t k = 0; k < rig->steps.size(); ++k)
        if (rig->steps[k].geom.cw > SP_MAXW || rig->steps[k].geom.ch > 65535)
            return fail(STITCH_ERR_ARG, "rig_set_seam_paths: step %zu has a canvas of %d x %d, the finder takes up to %d x 65535", k, rig->steps[k].geom.cw,
                        rig->steps[k].geom.ch, SP_MAXW);
    rig->sp_mode = 1;
    rig->sp_opts = o;
    return STITCH_OK;
}

int stitch_rig_fix_seam_paths(stitch_rig* rig, const int32_t* const* paths, int n_steps) {
    if (!rig) return fail(STITCH_ERR_ARG, "rig_fix_seam_paths: null handle");
    const int ns = (int)rig->steps.size();
    if (n_steps != ns || (ns > 0 && !paths)) return fail(STITCH_ERR_ARG, "rig_fix_seam_paths: %d paths%s, the rig has %d steps", n_steps, paths ? "" : " (null)", ns);
    for (int k = 0; k < ns; ++k)
        if (!paths[k]) return fail(STITCH_ERR_ARG, "rig_fix_seam_paths: step %d has no path", k);
    rig_sp_rows(rig);
    std::vector<int32_t> fixed(rig->sp_rows);
    for (int k = 0; k < ns; ++k) std::memcpy(fixed.data() + rig->sp_row_at[k], paths[k], sizeof(int32_t) * rig->steps[k].geom.ch);
    rig->sp_fixed.swap(fixed);
    rig->sp_fixed_up = false;
    rig->sp_mode = 2;
    return STITCH_OK;
}

int stitch_rig_clear_seam_paths(stitch_rig* rig) {
    if (!rig) return fail(STITCH_ERR_ARG, "rig_clear_seam_paths: null handle");
    rig->sp_mode = 0;
    rig->sp_last.clear();
    rig->sp_last_cost.clear();
    rig->sp_last_sets = 0;
    rig->sa_last_moved.clear();
    rig->sa_has = false;  // include/stitch_seam_anchor.h: the anchor goes, its options stay
    rig->sa_prime.clear();
    return STITCH_OK;
}

int stitch_rig_seam_paths(const stitch_rig* rig, int* mode, stitch_seam_path_opts* opts) {
    if (!rig) return fail(STITCH_ERR_ARG, "rig_seam_paths: null handle");
    if (mode) *mode = rig->sp_mode;
    if (opts) *opts = rig->sp_opts;
    return STITCH_OK;
}

int stitch_rig_last_seam_paths(const stitch_rig* rig, int set, int step, int32_t* out, int cap, uint64_t* cost) {
    if (!rig || cap < 0 || (cap > 0 && !out)) return fail(STITCH_ERR_ARG, "rig_last_seam_paths: null handle, or a capacity of %d without an output", cap);
    const int ns = (int)rig->steps.size();
    if (set < 0 || set >= rig->sp_last_sets || step < 0 || step >= ns)
        return fail(STITCH_ERR_ARG, "rig_last_seam_paths: set %d, step %d: the last replay along paths had %d sets of %d steps", set, step, rig->sp_last_sets, ns);
    const int ch = rig->steps[step].geom.ch;
    const int32_t* from = rig->sp_last.data() + (size_t)set * rig->sp_rows + rig->sp_row_at[step];
    for (int y = 0; y < std::min(ch, cap); ++y) out[y] = from[y];
    if (cost) *cost = rig->sp_last_cost[(size_t)set * ns + step];
    return ch;
}

// ---- include/stitch_seam_anchor.h ----
int stitch_rig_set_seam_anchor(stitch_rig* rig, const stitch_seam_anchor_opts* opts) {
    if (!rig || !opts) return fail(STITCH_ERR_ARG, "rig_set_seam_anchor: null handle or options");
    if (!seam_anchor_opts_ok(*opts))
        return fail(STITCH_ERR_ARG, "rig_set_seam_anchor: weight %d below 0, cap %d below 1, or weight * cap above %d", opts->weight, opts->cap, STITCH_SEAM_ANCHOR_MAX);
    if (opts->policy != STITCH_SEAM_ANCHOR_PER_SET && opts->policy != STITCH_SEAM_ANCHOR_PER_CALL)
        return fail(STITCH_ERR_ARG, "rig_set_seam_anchor: policy %d (1: per set, 2: per call)", opts->policy);
    rig->sa_opts = *opts;
    return STITCH_OK;
}

int stitch_rig_prime_seam_anchor(stitch_rig* rig, const int32_t* const* paths, int n_steps) {
    if (!rig) return fail(STITCH_ERR_ARG, "rig_prime_seam_anchor: null handle");
    const int ns = (int)rig->steps.size();
    if (n_steps != ns || (ns > 0 && !paths)) return fail(STITCH_ERR_ARG, "rig_prime_seam_anchor: %d paths%s, the rig has %d steps", n_steps, paths ? "" : " (null)", ns);
    for (int k = 0; k < ns; ++k)
        if (!paths[k]) return fail(STITCH_ERR_ARG, "rig_prime_seam_anchor: step %d has no path", k);
    if (ns == 0) return STITCH_OK;  // nothing to anchor
    rig_sp_rows(rig);
    std::vector<int32_t> prime(rig->sp_rows);
    for (int k = 0; k < ns; ++k) std::memcpy(prime.data() + rig->sp_row_at[k], paths[k], sizeof(int32_t) * rig->steps[k].geom.ch);
    rig->sa_prime.swap(prime);
    rig->sa_has = true;
    return STITCH_OK;
}

int stitch_rig_reset_seam_anchor(stitch_rig* rig) {
    if (!rig) return fail(STITCH_ERR_ARG, "rig_reset_seam_anchor: null handle");
    rig->sa_has = false;
    rig->sa_prime.clear();
    return STITCH_OK;
}

int stitch_rig_clear_seam_anchor(stitch_rig* rig) {
    if (!rig) return fail(STITCH_ERR_ARG, "rig_clear_seam_anchor: null handle");
    rig->sa_opts = stitch_seam_anchor_opts{0, 0, 0};
    return stitch_rig_reset_seam_anchor(rig);
}

int stitch_rig_seam_anchor(const stitch_rig* rig, stitch_seam_anchor_opts* opts, int* has_anchor) {
    if (!rig) return fail(STITCH_ERR_ARG, "rig_seam_anchor: null handle");
    if (opts) *opts = rig->sa_opts;
    if (has_anchor) *has_anchor = rig->sa_has ? 1 : 0;
    return STITCH_OK;
}

int stitch_rig_last_seam_moved(const stitch_rig* rig, int set, int step, uint64_t* moved) {
    if (!rig || !moved) return fail(STITCH_ERR_ARG, "rig_last_seam_moved: null handle or output");
    const int ns = (int)rig->steps.size();
    if (set < 0 || set >= rig->sp_last_sets || step < 0 || step >= ns)
        return fail(STITCH_ERR_ARG, "rig_last_seam_moved: set %d, step %d: the last replay along paths had %d sets of %d steps", set, step, rig->sp_last_sets, ns);
    *moved = rig->sa_last_moved[(size_t)set * ns + step];
    return STITCH_OK;
}

}  // extern "C"
