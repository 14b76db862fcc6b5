// stitch_rig.inc -- a calibrated rig: the recorded steps of one panorama replayed on many frame sets (include/stitch_rig.h;
// kernels in k_rig.inc).  Included at the end of stitch_hip.hip (one translation unit).
//
// The replay restates pipeline.py's stitch_chain for up to max_sets sets per launch sequence: the projections of a frame index,
// every step (stitch_dev_pairs_u8 on a batched workspace the rig owns) and the finish pass are each ONE launch sequence over
// the sets.  No bit can differ from the single-set chain: a pair of a batch does not depend on its neighbours, and the
// many-image kernels run the single-image kernels' device functions per image.
struct stitch_rig {
    // ---- the description (host only) ----
    int n = 0, start = 0, max_sets = 16, finish = 1;
    float fov_deg = 15.0f;
    double num = 19.0, den = 20.0;
    bool has_blend = false;
    stitch_blend_opts blend{};
    std::vector<int32_t> fw, fh;
    std::vector<stitch_panorama_step> steps;
    std::vector<int> needed;  // the frames the replay projects: the start and every step's dst, each once
    int out_w = 0, out_h = 0;
    // ---- the workspaces, from the first stitch call on ----
    int device = -1;
    std::vector<stitch_plan*> plans;   // one per distinct canvas size
    std::vector<int> plan_of_step;
    std::vector<uint8_t*> proj;        // per frame: max_sets projected frames (NULL for a frame no step uses)
    uint8_t* mosaic[2] = {nullptr, nullptr};  // max_sets mosaics each, `mosaic_bytes` apart
    size_t mosaic_bytes = 0;
    // ---- the colour transfer before every step (include/stitch_rig_exposure.h; stitch_rig_exposure.inc) ----
    stitch_exposure_opts ex{0, 0, 0};  // mode 0: the replay as it is
    size_t ex_src_px = 0, ex_tem_px = 0;  // the largest frame a step warps, the largest template
    float* ex_lab = nullptr;              // max_sets * 3 * ex_src_px floats of frames, then max_sets * 3 * ex_tem_px of templates
    float* ex_stats = nullptr;            // 16 floats per set and step, set-major
    double* ex_sums = nullptr;            // form 2: per span of 6 * max_sets planes of the longest plane
    void* ex_table = nullptr;             // form 2: the span table (ExSpanEntry)
    // ---- temporal exposure (include/stitch_rig_exposure_temporal.h; stitch_rig_exposure.inc): nothing below is at work in mode 0 ----
    int et_keep = -1;                     // smoothing: the filter keeps et_keep / 256 of its state; -1: no smoothing
    std::vector<float> et_state;          // ... its state between replays, 12 floats per step, and per step whether it has one
    std::vector<int32_t> et_has;          //     (both empty: no step has; a replay takes them up and a completed one leaves them)
    float* ex_used = nullptr;             // ... the records the apply passes read, laid out as ex_stats; from the first smoothed replay on
    int32_t* et_failed = nullptr;         // ... per set of a sequence whether an earlier step's seam scan refused it (k_ex_stats_filter)
    std::vector<float> et_fixed;          // fixed statistics, 12 floats per step (empty: none); they win over smoothing
    std::vector<float> et_last_used;      // what the apply passes of the last replay with an option read: 12 floats per set and step
    int et_last_sets = 0;
    // ---- fixed seams and coverage (include/stitch_rig_seams.h; stitch_rig_seams.inc) ----
    std::vector<stitch_seam> fixed;  // one record per step, or empty: content seams
    int cover_device = -1;           // the device of the coverage planes, -1: not computed yet
    unsigned long long* cover = nullptr;         // every plane, one block: C_proj per distinct frame size, then A, B, A | B per step
    std::vector<size_t> cover_proj, cover_step;  // word offsets: per frame (its size's plane), per step (A; B and A | B follow)
    std::vector<SeamDev> cover_seams;            // the scan of every step over coverage
    // ---- the crop of the output (include/stitch_rig_crop.h; stitch_rig_crop.inc) ----
    int crop_mode = 0;  // 0: the whole canvas, 1: the rectangle of the finished canvas, 2: the finish pass on the rectangle
    stitch_rect crop{0, 0, 0, 0};
    uint8_t* crop_full = nullptr;  // max_sets full canvases the last step writes, `crop_full_bytes` apart; from the first cropped call on
    size_t crop_full_bytes = 0;
    // ---- frames and outputs in camera layouts (include/stitch_rig_formats.h; stitch_rig_formats.inc) ----
    int in_fmt = 0, out_fmt = 0, matrix = 0;  // (0, 0): planar both ways, the replay as it is
    std::vector<uint8_t*> fmt_in;  // per projected frame: max_sets planar frames the input is converted to; from the first such call on
    uint8_t* fmt_out = nullptr;    // max_sets planar outputs the last step (or the crop copy) writes, `fmt_out_bytes` apart; likewise
    size_t fmt_out_bytes = 0;
    std::vector<char> fmt_form;    // per frame index: STITCH_RIG_INPUT_* of the last completed call with images (empty: none yet)
    // ---- the alignment monitor (include/stitch_rig_monitor.h; stitch_rig_monitor.inc) ----
    int mon_radius = -1;                     // -1: no monitor, the replay as it is
    int mon_dom_radius = -1;                 // the radius the domains below were computed at, -1: not computed yet
    unsigned long long* mon_dom = nullptr;   // D_k of every step as bit planes, one block, then 4 words of bounding box per step
    std::vector<size_t> mon_dom_at;          // word offsets per step
    size_t mon_dom_words = 0;
    std::vector<stitch_rect> mon_box;        // per step: what a residual launch covers (w = 0: an empty domain)
    unsigned long long* mon_rec = nullptr;   // the records of the sequence in flight: max_sets sets, set-major then step
    std::vector<uint64_t> mon_last;          // the records of the last monitored replay, and whose they are
    int mon_last_sets = 0, mon_last_radius = -1;
    // ---- path seams (include/stitch_seam_path.h; stitch_rig_seam_paths.inc) ----
    int sp_mode = 0;                          // 0: none, the replay as it is; 1: every set finds its own paths; 2: fixed paths
    stitch_seam_path_opts sp_opts{2, 8};
    std::vector<size_t> sp_row_at;            // per step: where its ch rows start among a set's rows; sp_rows: the rows of a set
    size_t sp_rows = 0;
    std::vector<int32_t> sp_fixed;            // mode 2: sp_rows columns, step after step
    bool sp_fixed_up = false;                 // ... and whether sp_fixed_dev holds them
    std::vector<stitch_plan*> sp_plans;       // the masked twins of `plans`, from the first replay with paths on
    int32_t* sp_fixed_dev = nullptr;          // sp_rows columns
    int32_t* sp_paths = nullptr;              // mode 1: the paths of the sequence in flight, max_sets sets of sp_rows columns
    unsigned long long* sp_costs = nullptr;   // ... and their costs, max_sets sets of one word per step
    void* sp_scratch = nullptr;               // ... and the finder's costs and predecessors of one step, sized for the largest
    std::vector<int32_t> sp_last;             // the paths of the last replay with paths, set-major, and their costs
    std::vector<uint64_t> sp_last_cost;
    int sp_last_sets = 0;
    // ---- anchored path seams (include/stitch_seam_anchor.h; stitch_rig_seam_paths.inc): at work while sp_mode == 1 and a policy is set ----
    stitch_seam_anchor_opts sa_opts{0, 0, 0};  // policy 0: no options set
    bool sa_has = false;                      // the rig has an anchor: sa_dev holds it, or sa_prime does until the next replay takes it up
    bool sa_live = false;                     // ... during a replay: sa_dev holds the anchor of the next set to anchor on it
    std::vector<int32_t> sa_prime;            // a primed anchor not yet on the device: sp_rows columns (empty: none is waiting)
    int32_t* sa_dev = nullptr;                // the anchor: sp_rows columns, step after step
    unsigned long long* sa_moved = nullptr;   // `moved` of the sequence in flight, max_sets sets of one word per step
    std::vector<uint64_t> sa_last_moved;      // ... and of the last replay with paths, beside sp_last_cost
    // ---- the output scale (include/stitch_rig_scale.h; stitch_rig_scale.inc): 0, 0 is no scale, the replay as it is ----
    int scale_w = 0, scale_h = 0;             // (its planar calls use fmt_out / crop_full as a formatted output does)
    bool sa_active() const { return sp_mode == 1 && sa_opts.policy != 0; }
    const stitch_blend_opts* blend_ptr() const { return has_blend ? &blend : nullptr; }
    ~stitch_rig() {
        for (stitch_plan* p : sp_plans) stitch_plan_destroy(p);  // waits for the plan's last call
        for (void* p : {(void*)sp_fixed_dev, (void*)sp_paths, (void*)sp_costs, sp_scratch, (void*)sa_dev, (void*)sa_moved})
            if (p) (void)hipFree(p);
        if (crop_full) (void)hipFree(crop_full);
        if (fmt_out) (void)hipFree(fmt_out);
        for (uint8_t* p : fmt_in)
            if (p) (void)hipFree(p);
        if (cover) (void)hipFree(cover);
        if (mon_dom) (void)hipFree(mon_dom);
        if (mon_rec) (void)hipFree(mon_rec);
        for (void* p : {(void*)ex_lab, (void*)ex_stats, (void*)ex_sums, ex_table, (void*)ex_used, (void*)et_failed})
            if (p) (void)hipFree(p);
        for (stitch_plan* p : plans) stitch_plan_destroy(p);  // waits for the plan's last call
        for (uint8_t* p : proj)
            if (p) (void)hipFree(p);
        for (uint8_t* p : mosaic)
            if (p) (void)hipFree(p);
    }
};

namespace {

constexpr int kRigMaxSets = 16, kRigMaxImages = 65535;

// The transfer of a rig with a mode (stitch_rig_exposure.inc): its scratch, its plane and image tables -- one block for the whole
// call, valid for every sequence, since it names the rig's own buffers only -- and step k's transfer over the m sets in flight.
int rig_ex_workspaces(stitch_rig* R);
size_t rig_ex_table_bytes(const stitch_rig* R);
// include/stitch_rig_exposure_temporal.h: with fixed statistics the block holds the step's records and step k's transfer is one launch
// that measures nothing; under smoothing it also holds the filter's states -- the ones the replay starts from go up in it, the
// filter launches between a step's statistics and its apply pass rewrite them there, and rig_et_collect copies them back.
void rig_ex_fill_tables(const stitch_rig* R, unsigned char* host, const std::vector<float>& state, const std::vector<int32_t>& has);
int rig_ex_transfer(stitch_rig* R, unsigned char* d_tables, int k, int m, hipStream_t s);
bool rig_et_fixed(const stitch_rig* R);
bool rig_et_smoothed(const stitch_rig* R);
int rig_et_workspaces(stitch_rig* R);
int rig_et_collect(const stitch_rig* R, const unsigned char* d_tables, std::vector<float>* state, std::vector<int32_t>* has, hipStream_t s);

// The crop of a rig that has one (stitch_rig_crop.inc): the full-canvas buffers its last step writes, and the copy of the rectangle
// out of the m buffers of a sequence (the src entries of the table) to the caller's (the dst entries), one launch.
int rig_crop_workspace(stitch_rig* R);
int rig_crop_copy(const stitch_rig* R, const RigImage* d_tab, int m, hipStream_t s);

// A call with images (stitch_rig_formats.inc; NULL: the planar calls).  The call has checked its images; its device table holds, per
// sequence, m entries per projected frame (a formatted input) and then m for the outputs (a formatted output).
struct RigFmtCall {
    const stitch_image* frames;
    const stitch_image* out;
    std::vector<char> fused;    // per frame index: its projection stages the packed source itself (rig_fmt_workspace decides)
    std::vector<FmtImage> tab;  // filled by rig_fmt_tables
    FmtImage* d_tab = nullptr;
};
int rig_fmt_workspace(stitch_rig* R, RigFmtCall* fc, int n_sets);
void rig_fmt_tables(const stitch_rig* R, RigFmtCall* fc, const RigImage* h_tab, int n_sets);
int rig_fmt_unpack(const stitch_rig* R, const FmtImage* d_tab, int m, int w, int h, hipStream_t s);
int rig_fmt_project(const stitch_rig* R, const FmtImage* d_tab, int m, int w, int h, hipStream_t s);  // the fused form of rig_project_many
// the end of a sequence with a formatted output: histogram and LUT where the rig finishes, the crop copy of mode 2, then the one pack
int rig_fmt_finish_pack(const stitch_rig* R, const RigImage* h_tab, const RigImage* d_tab, const FmtImage* d_fmt, int32_t* d_eq, int m, hipStream_t s);

// The output scale of a rig that has one (stitch_rig_scale.inc): the size rule against the rig's present source size, and the one
// launch that ends a sequence in place of the pack -- m images' rectangle rc, finished where d_eq holds their LUTs, scaled and written
// in the rig's output format (planar included).
int rig_scale_check(const stitch_rig* R, const char* who);
int rig_scale_pack(const stitch_rig* R, const FmtImage* d_fmt, int m, const FmtRect& rc, const int32_t* d_eq, const MixK& mk, hipStream_t s);

// The monitor of a rig that has one (stitch_rig_monitor.inc): its domains and record buffer, the zeroing of a sequence's records,
// step k's residual launch over the m sets in flight from the step's pair descriptors, the copy of a sequence's records to the host.
int rig_mon_prepare(stitch_rig* R, hipStream_t s);
int rig_mon_begin(stitch_rig* R, int m, hipStream_t s);
int rig_mon_step(stitch_rig* R, const stitch_pair_desc* pd, int k, int m, hipStream_t s);
int rig_mon_collect(stitch_rig* R, uint64_t* host, int m, hipStream_t s);

// Path seams of a rig that has a mode (stitch_rig_seam_paths.inc): the masked plans, the coverage planes and the path buffers; step k's
// blend over the m sets in flight -- behind the finder in mode 1 -- from the step's pair descriptors; the copy of a sequence's paths
// and costs to the host.
int rig_sp_prepare(stitch_rig* R, hipStream_t s);
int rig_sp_step(stitch_rig* R, const stitch_pair_desc* pd, int k, int m, hipStream_t s);
int rig_sp_collect(stitch_rig* R, int32_t* h_paths, uint64_t* h_costs, uint64_t* h_moved, int m, bool last, hipStream_t s);

bool same_bits(float a, float b) { return std::memcmp(&a, &b, sizeof a) == 0; }

// The sets of a call cut into launch sequences: pipeline.sequence_sizes(n_sets, max_sets, 1), balanced sizes in set order.
std::vector<int> rig_sequences(int n_sets, int max_sets) {
    const int m = (n_sets + max_sets - 1) / max_sets;
    std::vector<int> sizes((size_t)m);
    for (int i = 0; i < m; ++i) sizes[i] = n_sets / m + (i < n_sets % m ? 1 : 0);
    return sizes;
}

// `count` same-size images through one projection launch.  d_tab is the device copy of h_tab (already enqueued); the form is
// chosen once, from the size and the alignment of ALL sources, and is per image exactly dev_project's.
int rig_project_many(const RigImage* h_tab, const RigImage* d_tab, int count, int w, int h, float fov_deg, hipStream_t s) {
    const ProjParams pp = proj_params(w, h, fov_deg);
    bool aligned = true;
    for (int i = 0; i < count; ++i) aligned = aligned && (reinterpret_cast<uintptr_t>(h_tab[i].src) % 4) == 0;
    const size_t lds = project_lds_bytes<uint8_t>(w, h, pp, aligned);
    constexpr int TW = PJ_TW_U8, TH = PJ_TH_U8;
    const dim3 tgrid((w + TW - 1) / TW, (h + TH - 1) / TH, (unsigned)count);
    if (lds && !pp.flag)
        k_project_lds_many<TW, TH><<<tgrid, 256, lds, s>>>(d_tab, w, h, pp.r, (int)lds);
    else if (lds)
        k_project_lds_t_many<TW, TH><<<tgrid, 256, lds, s>>>(d_tab, w, h, pp.r, (int)lds);
    else
        k_project_many<<<grid_xy(w, h, count), 256, 0, s>>>(d_tab, w, h, pp.flag, pp.width, pp.height, pp.r);
    return launch_check("k_project_many");
}

// The first two launches of the finish pass on `count` same-size mosaics (the dst entries of the table): histogram and LUT.
// d_scratch: RIG_EQ_WORDS int32 per mosaic, the bins zeroed.  -> whether the word form ran: only when every mosaic allows it
// (words_ok).  Shared with the pack of stitch_rig_formats.inc, which applies the LUT itself.
bool rig_hist_lut_many(const RigImage* h_tab, const RigImage* d_tab, int32_t* d_scratch, int count, int w, int h, hipStream_t s) {
    const size_t n = (size_t)w * h;
    bool v4 = true;
    for (int i = 0; i < count; ++i) v4 = v4 && words_ok(h_tab[i].dst, n);
    if (v4)
        k_hist_many<true><<<dim3((unsigned)std::min(eq_grid(n / 4), 512), (unsigned)count), HIST_WAVES * 64, 0, s>>>(d_tab, n, d_scratch);
    else
        k_hist_many<false><<<dim3((unsigned)eq_grid(n), (unsigned)count), HIST_WAVES * 64, 0, s>>>(d_tab, n, d_scratch);
    k_lut_many<<<(unsigned)count, 256, 0, s>>>(d_scratch, w, h);
    return v4;
}

// `count` same-size mosaics through the finish pass in three launches: the two above, then the apply pass in the same form.
int rig_finish_many(const RigImage* h_tab, const RigImage* d_tab, int32_t* d_scratch, int count, int w, int h, double num, double den, hipStream_t s) {
    const size_t n = (size_t)w * h;
    const MixK mk = mix_params(num, den);
    if (rig_hist_lut_many(h_tab, d_tab, d_scratch, count, w, h, s))
        k_finish_apply_many<true><<<dim3((unsigned)eq_grid(n / 4), (unsigned)count), 256, 0, s>>>(d_tab, n, d_scratch, mk);
    else
        k_finish_apply_many<false><<<dim3((unsigned)eq_grid(n), (unsigned)count), 256, 0, s>>>(d_tab, n, d_scratch, mk);
    return launch_check("finish_many");
}

int rig_cfg(const stitch_rig_opts* opts, stitch_rig* R) {
    stitch_rig_opts o;
    if (opts)
        o = *opts;
    else
        stitch_rig_opts_default(&o);
    if (o.max_sets < 1 || o.max_sets > kRigMaxSets) return fail(STITCH_ERR_ARG, "rig: max_sets = %d outside 1 .. %d", o.max_sets, kRigMaxSets);
    R->max_sets = o.max_sets;
    R->finish = o.finish != 0;
    R->fov_deg = o.fov_deg;
    R->num = o.num;
    R->den = o.den;
    R->has_blend = o.blend != nullptr;
    if (o.blend) R->blend = *o.blend;
    return STITCH_OK;
}

// The workspaces, on the current device.  On failure the rig keeps what it has; the destructor frees it.
int rig_workspaces(stitch_rig* R) {
    int dev = -1;
    HIPCHK(hipGetDevice(&dev));
    if (R->device >= 0) {
        if (dev != R->device) return fail(STITCH_ERR_ARG, "rig: its workspaces belong to device %d, the current device is %d", R->device, dev);
        return STITCH_OK;
    }
    const int ns = (int)R->steps.size();
    if (R->plan_of_step.empty()) {
        std::vector<stitch_plan*> plans;
        std::vector<int> of((size_t)ns, -1);
        int rc = STITCH_OK;
        for (int k = 0; k < ns && !rc; ++k) {
            const stitch_step_geom& g = R->steps[k].geom;
            for (int j = 0; j < k && of[k] < 0; ++j)
                if (R->steps[j].geom.cw == g.cw && R->steps[j].geom.ch == g.ch) of[k] = of[j];
            if (of[k] >= 0) continue;
            stitch_plan* p = nullptr;
            if ((rc = stitch_plan_create_batched(g.cw, g.ch, R->blend_ptr(), R->max_sets, &p))) break;
            of[k] = (int)plans.size();
            plans.push_back(p);
        }
        if (rc) {
            for (stitch_plan* p : plans) stitch_plan_destroy(p);
            return rc;
        }
        R->plans = plans;
        R->plan_of_step = of;
    }
    if (R->proj.empty()) R->proj.assign((size_t)R->n, nullptr);
    for (int f : R->needed)  // (zero steps: the start frame is projected straight into the caller's buffers)
        if (ns && !R->proj[f]) HIPCHK(hipMalloc((void**)&R->proj[f], (size_t)R->max_sets * 3 * R->fw[f] * R->fh[f]));
    // steps 0 .. ns-2 write a rig buffer (the last one writes the caller's), in turn: a step never writes the buffer it reads
    R->mosaic_bytes = 0;
    for (int k = 0; k + 1 < ns; ++k) R->mosaic_bytes = std::max(R->mosaic_bytes, align256((size_t)3 * R->steps[k].geom.cw * R->steps[k].geom.ch));
    for (int b = 0; b < std::min(2, ns - 1); ++b)
        if (!R->mosaic[b]) HIPCHK(hipMalloc((void**)&R->mosaic[b], (size_t)R->max_sets * R->mosaic_bytes));
    if (R->ex.mode && ns && !rig_et_fixed(R)) {  // (fixed statistics need none of it: rig_et_workspaces takes it once they are cleared)
        const int rc = rig_ex_workspaces(R);
        if (rc) return rc;
    }
    R->device = dev;
    return STITCH_OK;
}

// The seam records of the plans' last calls, read before a plan is used again and before the call returns.
struct RigOutcome {
    stitch_rig* R;
    int32_t* set_status;
    stitch_seam* seams;
    int n_steps;
    std::vector<int> pending_step;  // per plan: the step whose records are unread, or -1
    int set0 = 0, m = 0;            // the sequence in flight
    int hip_fault = STITCH_OK;
    std::string hip_text;
    std::vector<int> fail_step;  // per set: the first step whose seam scan failed, or n_steps
    // a replay along paths (include/stitch_seam_path.h): the steps ran on the masked plans, and the records are the geometric ones
    const std::vector<stitch_plan*>* plans;
    bool pathed;
    RigOutcome(stitch_rig* r, int n_sets, int32_t* st, stitch_seam* sm)
        : R(r), set_status(st), seams(sm), n_steps((int)r->steps.size()), pending_step(r->plans.size(), -1), fail_step((size_t)n_sets, (int)r->steps.size()),
          plans(r->sp_mode ? &r->sp_plans : &r->plans), pathed(r->sp_mode != 0) {}
    // waits for the plan's last call
    void read(int pi) {
        const int k = pending_step[pi];
        if (k < 0) return;
        pending_step[pi] = -1;
        for (int i = 0; i < m; ++i) {
            stitch_seam sm;
            std::memset(&sm, 0, sizeof sm);
            const int rc = stitch_plan_status_at((*plans)[pi], i, &sm);
            if (pathed) seam_to_public(R->cover_seams[k], &sm);
            const int set = set0 + i;
            if (rc == STITCH_ERR_HIP) {  // a sticky hand-off time-out (or a failed wait): nothing of this call counts
                if (!hip_fault) {
                    hip_fault = rc;
                    hip_text = g_err;
                }
                (void)stitch_plan_clear_fault((*plans)[pi]);
                return;
            }
            if (seams) seams[(size_t)set * n_steps + k] = sm;
            if (rc != STITCH_OK && k < fail_step[set]) {  // plans are read in plan order, not in step order
                set_status[set] = rc;
                fail_step[set] = k;
            }
        }
    }
    void read_all() {
        for (size_t pi = 0; pi < pending_step.size(); ++pi) read((int)pi);
    }
    // every return path: no plan keeps an unread call or an unacknowledged fault behind
    ~RigOutcome() {
        for (size_t pi = 0; pi < pending_step.size(); ++pi)
            if (pending_step[pi] >= 0 && stitch_plan_status_at((*plans)[pi], 0, nullptr) == STITCH_ERR_HIP) (void)stitch_plan_clear_fault((*plans)[pi]);
    }
};

int rig_many_args(const void* a, const void* b, int count, int w, int h, const char* what) {
    if (!a || !b || count < 1 || count > kRigMaxImages || w <= 0 || h <= 0)
        return fail(STITCH_ERR_ARG, "%s: null table, %d images (1 .. %d) or bad size %dx%d", what, count, kRigMaxImages, w, h);
    return STITCH_OK;
}

// stitch_rig_create, and stitch_rig_create_exposure with its options (NULL: mode 0)
int rig_create(const int32_t* frame_wh, int n, int start, const stitch_panorama_step* steps, int n_steps, const stitch_rig_opts* opts,
               const stitch_exposure_opts* exposure, stitch_rig** out) {
    if (out) *out = nullptr;
    if (!out || !frame_wh || n_steps < 0 || (n_steps > 0 && !steps)) return fail(STITCH_ERR_ARG, "rig: null argument or %d steps", n_steps);
    if (n < 1 || n > kPanoMaxFrames) return fail(STITCH_ERR_ARG, "rig: %d frames (1 .. %d)", n, kPanoMaxFrames);
    std::unique_ptr<stitch_rig> R(new stitch_rig());
    int rc = rig_cfg(opts, R.get());
    if (rc) return rc;
    if (exposure) {
        if ((rc = chain_check_exposure(*exposure, "rig"))) return rc;
        if (exposure->mode) R->ex = *exposure;
    }
    R->n = n;
    for (int i = 0; i < n; ++i) {
        const int w = frame_wh[2 * i], h = frame_wh[2 * i + 1];
        if (w <= 0 || h <= 0) return fail(STITCH_ERR_ARG, "rig: frame %d has a bad size %d x %d", i, w, h);
        R->fw.push_back(w);
        R->fh.push_back(h);
    }
    if (start < 0 || start >= n) return fail(STITCH_ERR_ARG, "rig: start frame %d outside 0 .. %d", start, n - 1);
    R->start = start;
    R->needed.push_back(start);
    int mw = R->fw[start], mh = R->fh[start];  // the projection keeps a frame's size
    for (int k = 0; k < n_steps; ++k) {
        const stitch_panorama_step& st = steps[k];
        if (st.dst < 0 || st.dst >= n) return fail(STITCH_ERR_ARG, "rig: step %d warps frame %d, outside 0 .. %d", k, st.dst, n - 1);
        for (int j = 0; j < 8; ++j)
            if (!std::isfinite(st.p_fwd[j]) || !std::isfinite(st.p_bwd[j])) return fail(STITCH_ERR_ARG, "rig: step %d has a map coefficient that is not finite", k);
        stitch_step_geom g;
        if ((rc = stitch_step_geometry(R->fw[st.dst], R->fh[st.dst], st.p_fwd, mw, mh, &g))) return rc;
        const stitch_step_geom& r = st.geom;
        if (!same_bits(g.min_x, r.min_x) || !same_bits(g.min_y, r.min_y) || g.cw != r.cw || g.ch != r.ch || g.ox != r.ox || g.oy != r.oy)
            return fail(STITCH_ERR_ARG,
                        "rig: step %d records the canvas %d x %d, offsets (%.9g, %.9g) / (%d, %d); its forward map on a %d x %d mosaic gives %d x %d, "
                        "(%.9g, %.9g) / (%d, %d)",
                        k, r.cw, r.ch, (double)r.min_x, (double)r.min_y, r.ox, r.oy, mw, mh, g.cw, g.ch, (double)g.min_x, (double)g.min_y, g.ox, g.oy);
        if (R->ex.mode) {
            // the template of the step's transfer: the projected frame src, which must have been placed (`needed` holds the
            // frames placed so far), or the running mosaic before the step
            if (R->ex.mode == 1 && std::find(R->needed.begin(), R->needed.end(), st.src) == R->needed.end())
                return fail(STITCH_ERR_ARG, "rig: step %d takes frame %d as its template, which is neither the start frame nor warped by an earlier step", k,
                            st.src);
            const long long f_px = (long long)R->fw[st.dst] * R->fh[st.dst];
            const long long t_px = R->ex.mode == 1 ? (long long)R->fw[st.src] * R->fh[st.src] : (long long)mw * mh;
            if (f_px > 0x7fffffffLL || t_px > 0x7fffffffLL) return fail(STITCH_ERR_ARG, "rig: step %d: w*h of the frame or of the template overflows int", k);
            R->ex_src_px = std::max(R->ex_src_px, (size_t)f_px);
            R->ex_tem_px = std::max(R->ex_tem_px, (size_t)t_px);
        }
        if (std::find(R->needed.begin(), R->needed.end(), st.dst) == R->needed.end()) R->needed.push_back(st.dst);
        R->steps.push_back(st);
        mw = g.cw;
        mh = g.ch;
    }
    R->out_w = mw;
    R->out_h = mh;
    *out = R.release();
    return STITCH_OK;
}

int rig_from_panorama(const stitch_panorama* pano, const stitch_frame_u8* frames, int n, const stitch_rig_opts* opts, const stitch_exposure_opts* exposure,
                      stitch_rig** out) {
    if (out) *out = nullptr;
    if (!pano || !frames || !out) return fail(STITCH_ERR_ARG, "rig_from_panorama: null argument");
    if (n < 1 || n > kPanoMaxFrames) return fail(STITCH_ERR_ARG, "rig: %d frames (1 .. %d)", n, kPanoMaxFrames);
    std::vector<int32_t> wh;
    for (int i = 0; i < n; ++i) {
        wh.push_back(frames[i].width);
        wh.push_back(frames[i].height);
    }
    return rig_create(wh.data(), n, pano->start, pano->steps.data(), (int)pano->steps.size(), opts, exposure, out);
}

}  // namespace

extern "C" {

void stitch_rig_opts_default(stitch_rig_opts* o) {
    if (!o) return;
    std::memset(o, 0, sizeof *o);
    o->fov_deg = 15.0f;
    o->finish = 1;
    o->num = 19.0;
    o->den = 20.0;
    o->max_sets = kRigMaxSets;
}

int stitch_rig_create(const int32_t* frame_wh, int n, int start, const stitch_panorama_step* steps, int n_steps, const stitch_rig_opts* opts,
                      stitch_rig** out) {
    return rig_create(frame_wh, n, start, steps, n_steps, opts, nullptr, out);
}

int stitch_rig_from_panorama(const stitch_panorama* pano, const stitch_frame_u8* frames, int n, const stitch_rig_opts* opts, stitch_rig** out) {
    return rig_from_panorama(pano, frames, n, opts, nullptr, out);
}

int stitch_rig_info(const stitch_rig* rig, int* width, int* height, int* n_frames, int* n_steps, int* max_sets) {
    if (!rig) return fail(STITCH_ERR_ARG, "rig_info: null handle");
    if (width) *width = rig->out_w;
    if (height) *height = rig->out_h;
    if (n_frames) *n_frames = rig->n;
    if (n_steps) *n_steps = (int)rig->steps.size();
    if (max_sets) *max_sets = rig->max_sets;
    return STITCH_OK;
}

const stitch_plan* stitch_rig_step_plan(const stitch_rig* rig, int k) {
    return rig && k >= 0 && k < (int)rig->plan_of_step.size() ? rig->plans[rig->plan_of_step[k]] : nullptr;
}

}  // extern "C"

namespace {

// stitch_dev_rig_stitch_u8, and stitch_dev_rig_stitch_exposure_u8 with its statistics (a host array, or NULL)
int rig_stitch(stitch_rig* rig, const stitch_frame_u8* frames, int n_sets, uint8_t* const* d_out, int32_t* set_status, stitch_seam* seams, float* stats,
               void* stream, RigFmtCall* fc = nullptr) {
    int rc;
    if (rig && rig->scale_w && (rc = rig_scale_check(rig, "rig_stitch"))) return rc;  // include/stitch_rig_scale.h: before a device is needed
    if ((rc = need_device())) return rc;
    if (!rig || !frames || !d_out || !set_status || n_sets < 1) return fail(STITCH_ERR_ARG, "rig_stitch: null argument or %d sets", n_sets);
    stitch_rig* R = rig;
    if (stats && !R->ex.mode) return fail(STITCH_ERR_ARG, "rig_stitch: statistics asked of a rig made without a transfer (mode 0)");
    const int n = R->n, ns = (int)R->steps.size();
    // include/stitch_rig_crop.h: a cropped rig writes the rectangle to d_out, and its last step a full canvas of the rig's own
    const bool cropped = R->crop_mode != 0;
    const bool scaled = R->scale_w != 0;  // include/stitch_rig_scale.h: d_out takes the scaled size
    const size_t out_bytes = scaled ? (size_t)3 * R->scale_w * R->scale_h : cropped ? (size_t)3 * R->crop.w * R->crop.h : (size_t)3 * R->out_w * R->out_h;
    const bool with_images = fc != nullptr;
    const bool fin = fc && rig->in_fmt, fout = (fc && rig->out_fmt) || scaled;  // (a call with images has checked them itself)
    for (int i = 0; i < n_sets && !fc; ++i) {
        if (!d_out[i]) return fail(STITCH_ERR_ARG, "rig_stitch: set %d has no output buffer", i);
        for (int f = 0; f < n; ++f) {
            const stitch_frame_u8& fr = frames[(size_t)i * n + f];
            if (fr.width != R->fw[f] || fr.height != R->fh[f])
                return fail(STITCH_ERR_ARG, "rig_stitch: set %d frame %d is %d x %d, the rig was made for %d x %d", i, f, fr.width, fr.height, R->fw[f], R->fh[f]);
        }
        for (int f : R->needed) {
            const stitch_frame_u8& fr = frames[(size_t)i * n + f];
            if (!fr.data) return fail(STITCH_ERR_ARG, "rig_stitch: set %d frame %d has no data", i, f);
            const size_t fb = (size_t)3 * fr.width * fr.height;
            for (int j = 0; j < n_sets; ++j)
                if (d_out[j] && ranges_overlap(d_out[j], out_bytes, fr.data, fb)) return fail(STITCH_ERR_ARG, "rig_stitch: the output of set %d overlaps frame %d of set %d", j, f, i);
        }
        for (int j = 0; j < i; ++j)
            if (ranges_overlap(d_out[j], out_bytes, d_out[i], out_bytes)) return fail(STITCH_ERR_ARG, "rig_stitch: the outputs of sets %d and %d overlap", j, i);
    }
    // a planar call of a rig with a scale ends as a call with images does: its outputs are planar images of the scaled size, which
    // the one scaled pack launch per sequence writes from the rig's own buffers
    std::vector<stitch_image> scaled_out;
    RigFmtCall scaled_call{nullptr, nullptr, {}, {}, nullptr};
    if (scaled && !fc) {
        for (int i = 0; i < n_sets; ++i) scaled_out.push_back(stitch_image{d_out[i], nullptr, R->scale_w, R->scale_h, 0, 0});
        scaled_call.out = scaled_out.data();
        fc = &scaled_call;
    }
    if ((rc = rig_workspaces(R))) return rc;
    if ((rc = rig_et_workspaces(R))) return rc;
    if (cropped && (rc = rig_crop_workspace(R))) return rc;
    if ((fin || fout) && (rc = rig_fmt_workspace(R, fc, n_sets))) return rc;
    hipStream_t s = as_stream(stream);
    // include/stitch_rig_monitor.h: a failed call leaves no records behind, a completed one its own
    const bool monitored = R->mon_radius >= 0 && ns > 0;
    if (R->mon_radius >= 0) {
        R->mon_last.clear();
        R->mon_last_sets = 0;
    }
    if (monitored && (rc = rig_mon_prepare(R, s))) return rc;
    const size_t mon_words = monitored ? (size_t)(2 + 3 * (2 * R->mon_radius + 1) * (2 * R->mon_radius + 1)) * ns : 0;  // per set
    std::vector<uint64_t> h_mon(mon_words * n_sets);  // written by the records' copies: waited for like h_stats
    // include/stitch_seam_path.h: likewise, a failed call leaves no paths behind
    const bool pathed = R->sp_mode != 0 && ns > 0;
    if (R->sp_mode) {
        R->sp_last.clear();
        R->sp_last_cost.clear();
        R->sp_last_sets = 0;
        R->sa_last_moved.clear();
    }
    // include/stitch_seam_anchor.h: the anchor is the replay's from here on, and the rig's again once the replay has completed
    const bool anchored = pathed && R->sa_active();
    if (anchored) {
        R->sa_live = R->sa_has;
        R->sa_has = false;
    }
    if (pathed && (rc = rig_sp_prepare(R, s))) return rc;
    // include/stitch_rig_exposure_temporal.h: the filter's states are the replay's from here on, and the rig's again once it has
    // completed with every set's status STITCH_OK; a failed call leaves no used statistics behind
    const bool ex_fixed = ns > 0 && rig_et_fixed(R), smoothed = ns > 0 && rig_et_smoothed(R);
    std::vector<float> et_state, h_used(smoothed ? (size_t)16 * ns * n_sets : 0);
    std::vector<int32_t> et_has;
    if (R->ex.mode) {
        R->et_last_used.clear();
        R->et_last_sets = 0;
    }
    if (smoothed) {
        et_state.swap(R->et_state);
        et_has.swap(R->et_has);
    }
    std::vector<int32_t> h_paths(pathed ? R->sp_rows * n_sets : 0);
    std::vector<uint64_t> h_pcost(pathed ? (size_t)ns * n_sets : 0), h_moved(pathed ? (size_t)ns * n_sets : 0);
    for (int i = 0; i < n_sets; ++i) set_status[i] = STITCH_OK;

    // ---- the pointer tables of the whole call, uploaded once: per sequence one slice per projected frame, then the outputs ----
    const int n_need = (int)R->needed.size();
    const std::vector<int> seqs = rig_sequences(n_sets, R->max_sets);
    // (a cropped rig: the outputs' entries name the full canvas as their source, and one more slice names it as a destination)
    std::vector<RigImage> tab((size_t)(n_need + (cropped ? 2 : 1)) * n_sets);
    auto full_of = [&](int i) { return R->crop_full + (size_t)i * R->crop_full_bytes; };  // set i of a sequence
    // set `set`, the i-th of its sequence: where its output goes, and frame f as the projection reads it
    // (a formatted output whose pack reads the full canvases has no buffer of its own: NULL, which nothing reads)
    auto out_of = [&](int set, int i) { return !fout ? d_out[set] : R->fmt_out ? R->fmt_out + (size_t)i * R->fmt_out_bytes : nullptr; };
    auto src_of = [&](int set, int i, int f) {  // (NULL: the projection stages the packed frame itself)
        return !fin ? (const uint8_t*)frames[(size_t)set * n + f].data : fc->fused[f] ? nullptr : R->fmt_in[f] + (size_t)i * 3 * R->fw[f] * R->fh[f];
    };
    {
        size_t at = 0;
        int set0 = 0;
        for (int m : seqs) {
            for (int f : R->needed)
                for (int i = 0; i < m; ++i) {
                    // zero steps: the start frame is projected straight into the caller's buffer
                    uint8_t* dst = ns == 0 ? (cropped ? full_of(i) : out_of(set0 + i, i)) : R->proj[f] + (size_t)i * 3 * R->fw[f] * R->fh[f];
                    tab[at++] = RigImage{src_of(set0 + i, i, f), dst};
                }
            for (int i = 0; i < m; ++i) tab[at++] = RigImage{cropped ? full_of(i) : nullptr, out_of(set0 + i, i)};
            for (int i = 0; cropped && i < m; ++i) tab[at++] = RigImage{nullptr, full_of(i)};
            set0 += m;
        }
    }
    // a rig with a mode: the plane and image tables of its transfers go up behind the pointer table, in the same copy
    const size_t tab_bytes = sizeof(RigImage) * tab.size(), ex_at = (tab_bytes + 15) & ~size_t(15), ex_bytes = ns ? rig_ex_table_bytes(R) : 0;
    std::vector<unsigned char> up;
    if (ex_bytes) {
        up.resize(ex_at + ex_bytes);
        std::memcpy(up.data(), tab.data(), tab_bytes);
        rig_ex_fill_tables(R, up.data() + ex_at, et_state, et_has);
    }
    const size_t up_bytes = ex_bytes ? up.size() : tab_bytes;
    const void* up_from = ex_bytes ? (const void*)up.data() : (const void*)tab.data();
    std::vector<float> h_stats(stats && !ex_fixed ? (size_t)16 * ns * n_sets : 0);  // 16 floats per set and step, as on the device
    if (fc) rig_fmt_tables(R, fc, tab.data(), n_sets);
    PanoArena A(s);
    unsigned char* d_up = nullptr;
    int32_t* d_eq = nullptr;
    if ((rc = A.take(&d_up, up_bytes))) return rc;
    if (fc && !fc->tab.empty() && (rc = A.take(&fc->d_tab, sizeof(FmtImage) * fc->tab.size()))) return rc;
    RigImage* d_tab = reinterpret_cast<RigImage*>(d_up);
    if (R->finish && (rc = A.take(&d_eq, sizeof(int32_t) * RIG_EQ_WORDS * n_sets))) return rc;
    // the tables are read by their upload, h_stats is written by the statistics' copies, and what the arena frees is idle: every
    // return path below waits for the stream
    PanoWait wait{s};
    RigOutcome O(R, n_sets, set_status, seams);  // destroyed before the wait: reads what is pending
    HIPCHK(hipMemcpyAsync(d_up, up_from, up_bytes, hipMemcpyHostToDevice, s));
    if (fc && fc->d_tab) HIPCHK(hipMemcpyAsync(fc->d_tab, fc->tab.data(), sizeof(FmtImage) * fc->tab.size(), hipMemcpyHostToDevice, s));
    size_t fat = 0;  // the place in the images' table
    if (R->finish) HIPCHK(hipMemsetAsync(d_eq, 0, sizeof(int32_t) * RIG_EQ_WORDS * n_sets, s));

    size_t at = 0;
    int set0 = 0;
    std::vector<stitch_pair_desc> pd((size_t)R->max_sets);
    for (int m : seqs) {
        O.set0 = set0;
        O.m = m;
        for (int f : R->needed) {
            if (fin && fc->fused[f]) {
                if ((rc = rig_fmt_project(R, fc->d_tab + fat, m, R->fw[f], R->fh[f], s))) return rc;
            } else {
                if (fin && (rc = rig_fmt_unpack(R, fc->d_tab + fat, m, R->fw[f], R->fh[f], s))) return rc;
                if ((rc = rig_project_many(tab.data() + at, d_tab + at, m, R->fw[f], R->fh[f], R->fov_deg, s))) return rc;
            }
            if (fin) fat += m;
            at += m;
        }
        const uint8_t* cur = ns ? R->proj[R->start] : nullptr;
        size_t cur_stride = (size_t)3 * R->fw[R->start] * R->fh[R->start];
        int mw = R->fw[R->start], mh = R->fh[R->start];
        if (monitored && (rc = rig_mon_begin(R, m, s))) return rc;
        for (int k = 0; k < ns; ++k) {
            const stitch_panorama_step& st = R->steps[k];
            const int pi = R->plan_of_step[k], f = st.dst;
            O.read(pi);  // the same workspace twice: its seam records are read before they are overwritten
            const bool last = k + 1 == ns;
            for (int i = 0; i < m; ++i) {
                stitch_pair_desc& d = pd[i];
                std::memset(&d, 0, sizeof d);
                d.frame = R->proj[f] + (size_t)i * 3 * R->fw[f] * R->fh[f];
                d.fw = R->fw[f];
                d.fh = R->fh[f];
                std::memcpy(d.p, st.p_bwd, sizeof d.p);
                d.offx = st.geom.min_x;
                d.offy = st.geom.min_y;
                d.mosaic = cur + (size_t)i * cur_stride;
                d.mw = mw;
                d.mh = mh;
                d.ox = st.geom.ox;
                d.oy = st.geom.oy;
                d.out = !last ? R->mosaic[k & 1] + (size_t)i * R->mosaic_bytes : cropped ? full_of(i) : out_of(set0 + i, i);
            }
            // include/stitch_rig_exposure.h: frame f of the m sets takes its template's colour statistics, in place
            if (ex_bytes && (rc = rig_ex_transfer(R, d_up + ex_at, k, m, s))) return rc;
            if (monitored && (rc = rig_mon_step(R, pd.data(), k, m, s))) return rc;  // the blend's own inputs, before it runs
            if (pathed) {  // include/stitch_seam_path.h: the blend along each set's own path, or along the step's fixed one
                if ((rc = rig_sp_step(R, pd.data(), k, m, s))) return rc;
            } else if (!R->fixed.empty()) {  // include/stitch_rig_seams.h: the step's fixed record for each of the m sets
                const std::vector<stitch_seam> given((size_t)m, R->fixed[k]);
                if ((rc = stitch_dev_pairs_seamed_u8(R->plans[pi], pd.data(), m, given.data(), s))) return rc;
            } else if ((rc = stitch_dev_pairs_u8(R->plans[pi], pd.data(), m, s)))
                return rc;
            O.pending_step[pi] = k;
            cur = R->mosaic[k & 1];
            cur_stride = R->mosaic_bytes;
            mw = st.geom.cw;
            mh = st.geom.ch;
        }
        if (fout) {
            if ((rc = rig_fmt_finish_pack(R, tab.data() + at, d_tab + at, fc->d_tab + fat, R->finish ? d_eq + (size_t)RIG_EQ_WORDS * set0 : nullptr, m, s))) return rc;
            fat += m;
            if (cropped) at += m;
        } else if (!cropped) {
            if (R->finish && (rc = rig_finish_many(tab.data() + at, d_tab + at, d_eq + (size_t)RIG_EQ_WORDS * set0, m, R->out_w, R->out_h, R->num, R->den, s))) return rc;
        } else {
            // mode 1 finishes the full canvases and copies; mode 2 copies and finishes the rectangles as images of their own
            int32_t* eq = R->finish ? d_eq + (size_t)RIG_EQ_WORDS * set0 : nullptr;
            if (R->finish && R->crop_mode == 1 && (rc = rig_finish_many(tab.data() + at + m, d_tab + at + m, eq, m, R->out_w, R->out_h, R->num, R->den, s))) return rc;
            if ((rc = rig_crop_copy(R, d_tab + at, m, s))) return rc;
            if (R->finish && R->crop_mode == 2 && (rc = rig_finish_many(tab.data() + at, d_tab + at, eq, m, R->crop.w, R->crop.h, R->num, R->den, s))) return rc;
            at += m;
        }
        at += m;
        // the sequence's statistics leave the device in one copy, behind its last transfer; the next sequence overwrites them
        if (!h_stats.empty())
            HIPCHK(hipMemcpyAsync(h_stats.data() + (size_t)16 * ns * set0, R->ex_stats, sizeof(float) * 16 * ns * m, hipMemcpyDeviceToHost, s));
        if (smoothed)  // ... and so do the records its apply passes read
            HIPCHK(hipMemcpyAsync(h_used.data() + (size_t)16 * ns * set0, R->ex_used, sizeof(float) * 16 * ns * m, hipMemcpyDeviceToHost, s));
        if (monitored && (rc = rig_mon_collect(R, h_mon.data() + mon_words * set0, m, s))) return rc;  // likewise
        if (pathed && (rc = rig_sp_collect(R, h_paths.data() + R->sp_rows * set0, h_pcost.data() + (size_t)ns * set0, h_moved.data() + (size_t)ns * set0, m, set0 + m == n_sets, s)))
            return rc;
        O.read_all();  // the next sequence uses the same workspaces
        if (O.hip_fault) break;
        set0 += m;
    }
    if (O.hip_fault) {
        for (int i = 0; i < n_sets; ++i) set_status[i] = O.hip_fault;
        return fail(O.hip_fault, "rig_stitch: %s", O.hip_text.c_str());
    }
    if (smoothed && (rc = rig_et_collect(R, d_up + ex_at, &et_state, &et_has, s))) return rc;  // behind the last sequence's filters
    HIPCHK(hipStreamSynchronize(s));  // the finish pass of the last sequence (read_all waited for the steps only)
    for (size_t j = 0; j < h_stats.size() / 16; ++j) std::memcpy(stats + 12 * j, h_stats.data() + 16 * j, sizeof(float) * 12);
    if (ex_fixed || smoothed) {  // include/stitch_rig_exposure_temporal.h: what the apply passes read, kept once the replay has completed
        R->et_last_used.resize((size_t)12 * ns * n_sets);
        for (size_t j = 0; j < (size_t)ns * n_sets; ++j)
            std::memcpy(R->et_last_used.data() + 12 * j, ex_fixed ? R->et_fixed.data() + 12 * (j % ns) : h_used.data() + 16 * j, sizeof(float) * 12);
        R->et_last_sets = n_sets;
        if (ex_fixed && stats) std::memcpy(stats, R->et_last_used.data(), sizeof(float) * R->et_last_used.size());  // nothing was measured
    }
    if (smoothed && std::all_of(set_status, set_status + n_sets, [](int32_t v) { return v == STITCH_OK; })) {
        R->et_state.swap(et_state);
        R->et_has.swap(et_has);
    }
    if (with_images) {  // include/stitch_rig_formats_yuv.h: the form each frame index took, kept once the replay has completed
        R->fmt_form.assign((size_t)n, (char)STITCH_RIG_INPUT_NONE);
        if (fin)
            for (int f : R->needed) R->fmt_form[f] = (char)(fc->fused[f] ? STITCH_RIG_INPUT_FUSED : STITCH_RIG_INPUT_CONVERTED);
    }
    if (R->mon_radius >= 0) {
        R->mon_last.swap(h_mon);
        R->mon_last_sets = n_sets;
        R->mon_last_radius = R->mon_radius;
    }
    if (R->sp_mode) {
        R->sp_last.swap(h_paths);
        R->sp_last_cost.swap(h_pcost);
        R->sa_last_moved.swap(h_moved);
        R->sp_last_sets = n_sets;
        if (anchored) R->sa_has = true;  // the last set's paths, copied behind the last sequence
    }
    for (int i = 0; i < n_sets; ++i)
        if (set_status[i] != STITCH_OK)
            return fail(set_status[i], "rig_stitch: set %d, step %d (frame %d): %s", i, O.fail_step[i], R->steps[O.fail_step[i]].dst,
                        set_status[i] == STITCH_ERR_EMPTY_MIDROW ? "channel 0 of the warped canvas's middle row is empty"
                                                                 : "the two canvases do not overlap on the middle row");
    return STITCH_OK;
}

}  // namespace

extern "C" {

int stitch_dev_rig_stitch_u8(stitch_rig* rig, const stitch_frame_u8* frames, int n_sets, uint8_t* const* d_out, int32_t* set_status,
                             stitch_seam* seams, void* stream) {
    if (rig && (rig->in_fmt || rig->out_fmt)) return fail(STITCH_ERR_ARG, "rig_stitch: the rig has formats set (include/stitch_rig_formats.h): call stitch_dev_rig_stitch_fmt_u8");
    return rig_stitch(rig, frames, n_sets, d_out, set_status, seams, nullptr, stream);
}

void stitch_rig_destroy(stitch_rig* rig) { delete rig; }

int stitch_dev_project_many_u8(const uint8_t* const* d_src, uint8_t* const* d_dst, int count, int w, int h, float fov_deg, void* stream) {
    int rc = need_device();
    if (rc) return rc;
    if ((rc = rig_many_args(d_src, d_dst, count, w, h, "project_many"))) return rc;
    std::vector<RigImage> tab((size_t)count);
    for (int i = 0; i < count; ++i) {
        if (!d_src[i] || !d_dst[i]) return fail(STITCH_ERR_ARG, "project_many: image %d has a null buffer", i);
        tab[i] = RigImage{d_src[i], d_dst[i]};
    }
    hipStream_t s = as_stream(stream);
    PanoArena A(s);
    RigImage* d_tab = nullptr;
    if ((rc = A.take(&d_tab, sizeof(RigImage) * count))) return rc;
    PanoWait wait{s};  // `tab` is read by its upload
    HIPCHK(hipMemcpyAsync(d_tab, tab.data(), sizeof(RigImage) * count, hipMemcpyHostToDevice, s));
    return rig_project_many(tab.data(), d_tab, count, w, h, fov_deg, s);
}

int stitch_dev_finish_many_u8(uint8_t* const* d_result, int count, int w, int h, double num, double den, void* stream) {
    int rc = need_device();
    if (rc) return rc;
    if ((rc = rig_many_args(d_result, d_result, count, w, h, "finish_many"))) return rc;
    if ((long long)w * h > 0x7fffffffLL) return fail(STITCH_ERR_ARG, "finish_many: w*h overflows int (the reference's int product)");
    std::vector<RigImage> tab((size_t)count);
    for (int i = 0; i < count; ++i) {
        if (!d_result[i]) return fail(STITCH_ERR_ARG, "finish_many: mosaic %d has a null buffer", i);
        tab[i] = RigImage{nullptr, d_result[i]};
    }
    hipStream_t s = as_stream(stream);
    PanoArena A(s);
    RigImage* d_tab = nullptr;
    int32_t* d_eq = nullptr;
    if ((rc = A.take(&d_tab, sizeof(RigImage) * count)) || (rc = A.take(&d_eq, sizeof(int32_t) * RIG_EQ_WORDS * count))) return rc;
    PanoWait wait{s};  // `tab` is read by its upload
    HIPCHK(hipMemcpyAsync(d_tab, tab.data(), sizeof(RigImage) * count, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemsetAsync(d_eq, 0, sizeof(int32_t) * RIG_EQ_WORDS * count, s));
    return rig_finish_many(tab.data(), d_tab, d_eq, count, w, h, num, den, s);
}

}  // extern "C"
