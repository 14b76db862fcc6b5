// stitch_seam_path.inc -- path seams: a masked plan, the blend along given paths, the finder (include/stitch_seam_path.h, which is
// the specification; kernels in k_seam_path.inc).  Included at the end of stitch_hip.hip (one translation unit).
namespace {

inline bool seam_path_opts_ok(const stitch_seam_path_opts& o) { return o.max_step >= 1 && o.max_step <= SP_MAXK && o.margin >= 0 && o.margin <= SP_MAXM; }

inline bool seam_anchor_opts_ok(const stitch_seam_anchor_opts& o) {
    return o.weight >= 0 && o.cap >= 1 && (long long)o.weight * o.cap <= STITCH_SEAM_ANCHOR_MAX;
}

// the finder's second launch over the costs of n pairs: one workgroup per pair, its two rows of states in dynamic LDS
// (an: include/stitch_seam_anchor.h, the anchored instantiation; null: the finder as it is)
int seam_path_dp(const unsigned* d_cost, int n, int cw, int ch, int max_step, uint8_t* d_pred, int32_t* d_paths, size_t path_stride, uint64_t* d_costs,
                 size_t cost_stride, hipStream_t s, const SeamAnchor* an = nullptr) {
    const size_t lds = sizeof(unsigned long long) * 2 * (size_t)(cw + 1);
    if (an) {
        static std::once_flag once_anchored;
        std::call_once(once_anchored, [] {
            (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&k_seam_path_dp<SeamAnchor>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                      (int)(sizeof(unsigned long long) * 2 * (SP_MAXW + 1)));
        });
        k_seam_path_dp<SeamAnchor><<<(unsigned)n, SP_DT, lds, s>>>(d_cost, cw, ch, max_step, d_pred, d_paths, path_stride, reinterpret_cast<unsigned long long*>(d_costs),
                                                               cost_stride, *an);
        return launch_check("k_seam_path_dp (anchored)");
    }
    static std::once_flag once;  // more than 64 KB of dynamic LDS is opt-in per function
    std::call_once(once, [] {
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&k_seam_path_dp<>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)(sizeof(unsigned long long) * 2 * (SP_MAXW + 1)));
    });
    k_seam_path_dp<><<<(unsigned)n, SP_DT, lds, s>>>(d_cost, cw, ch, max_step, d_pred, d_paths, path_stride, reinterpret_cast<unsigned long long*>(d_costs), cost_stride);
    return launch_check("k_seam_path_dp");
}

SeamPathPair seam_path_pair(const stitch_pair_desc& d, const void* cov_a, const void* cov_b, int branch) {
    SeamPathPair q;
    std::memset(&q, 0, sizeof q);
    q.frame = static_cast<const uint8_t*>(d.frame);
    q.mosaic = static_cast<const uint8_t*>(d.mosaic);
    q.cov_a = cov_a;
    q.cov_b = cov_b;
    std::memcpy(q.map.p, d.p, sizeof q.map.p);
    q.offx = d.offx, q.offy = d.offy;
    q.fw = d.fw, q.fh = d.fh, q.mw = d.mw, q.mh = d.mh, q.ox = d.ox, q.oy = d.oy;
    q.branch = branch;
    return q;
}

// n pairs on a masked plan through run_pairs, the launch sequence of every pair call: S1 into the level-0 planes (never source-fused),
// the mask plane and the records from the paths in place of scan and step mask (run_seam_mask), REDUCE, collapse.
template <typename PX>
int dev_pairs_pathed(stitch_plan* p, const stitch_pair_desc* d, int n, const int32_t* const* d_paths, const int32_t* branches, void* stream) {
    if (!p || !d || !d_paths || !branches) return fail(STITCH_ERR_ARG, "pairs_pathed: null plan, descriptor array, path table or branch array");
    if (!p->masked) return fail(STITCH_ERR_ARG, "pairs_pathed: the plan is not a masked plan (stitch_plan_create_masked)");
    if (n < 1 || n > p->cap) return fail(STITCH_ERR_ARG, "pairs_pathed: n=%d outside 1..%d (plan capacity)", n, p->cap);
    PathArgs ph{};
    for (int i = 0; i < n; ++i) {
        if (!d_paths[i]) return fail(STITCH_ERR_ARG, "pairs_pathed: pair %d has no path", i);
        if (branches[i] != 0 && branches[i] != 1) return fail(STITCH_ERR_ARG, "pairs_pathed: pair %d has branch %d (0 or 1)", i, branches[i]);
        ph.path[i] = d_paths[i];
        ph.branch[i] = branches[i];
    }
    for (int i = n; i < MAXB; ++i) ph.path[i] = ph.path[0], ph.branch[i] = ph.branch[0];
    int dev = -1;
    HIPCHK(hipGetDevice(&dev));
    if (dev != p->device) return fail(STITCH_ERR_ARG, "plan belongs to device %d, current device is %d", p->device, dev);
    PairArgs<PX> pa{};
    OutPtrs<PX> outs{};
    int rc = pair_args_of<PX>(d, n, pa, outs);
    if (rc) return rc;
    set_index_owners(pa, n, nullptr);
    return run_pairs<PX>(p, pa, outs, n, as_stream(stream), false, nullptr, &ph);
}

}  // namespace

extern "C" {

void stitch_seam_path_opts_default(stitch_seam_path_opts* o) {
    if (!o) return;
    o->max_step = 2;
    o->margin = 8;
}

int stitch_plan_create_masked(int cw, int ch, const stitch_blend_opts* opts, int max_pairs, stitch_plan** plan_out) {
    return plan_create(cw, ch, opts, max_pairs, false, plan_out, true);
}

int stitch_plan_is_masked(const stitch_plan* p) {
    if (!p) return fail(STITCH_ERR_ARG, "null plan");
    return p->masked ? 1 : 0;
}

int stitch_dev_pairs_pathed_u8(stitch_plan* plan, const stitch_pair_desc* pairs, int n, const int32_t* const* d_paths, const int32_t* branches, void* stream) {
    return dev_pairs_pathed<uint8_t>(plan, pairs, n, d_paths, branches, stream);
}
int stitch_dev_pairs_pathed_f32(stitch_plan* plan, const stitch_pair_desc* pairs, int n, const int32_t* const* d_paths, const int32_t* branches, void* stream) {
    return dev_pairs_pathed<float>(plan, pairs, n, d_paths, branches, stream);
}

}  // extern "C"

namespace {

// the finder of n pairs; d_anchors, ao, d_moved: all null, or the anchored call's (include/stitch_seam_anchor.h), checked by it
int pairs_seam_path(const stitch_pair_desc* pairs, int n, int cw, int ch, const uint8_t* const* d_cov_a, const uint8_t* const* d_cov_b, const int32_t* branches,
                    const stitch_seam_path_opts* opts, int32_t* d_paths, uint64_t* d_costs, void* stream, const int32_t* const* d_anchors,
                    const stitch_seam_anchor_opts* ao, uint64_t* d_moved) {
    if (!pairs || !d_cov_a || !d_cov_b || !branches || !d_paths || !d_costs) return fail(STITCH_ERR_ARG, "pairs_seam_path: null argument");
    stitch_seam_path_opts o;
    stitch_seam_path_opts_default(&o);
    if (opts) o = *opts;
    if (!seam_path_opts_ok(o))
        return fail(STITCH_ERR_ARG, "pairs_seam_path: max_step %d outside 1 .. %d or margin %d outside 0 .. %d", o.max_step, SP_MAXK, o.margin, SP_MAXM);
    if (n < 1 || n > kRigMaxImages) return fail(STITCH_ERR_ARG, "pairs_seam_path: %d pairs (1 .. %d)", n, kRigMaxImages);
    if (cw < 1 || ch < 1 || cw > SP_MAXW || ch > 65535) return fail(STITCH_ERR_ARG, "pairs_seam_path: bad canvas %d x %d (1 .. %d x 1 .. 65535)", cw, ch, SP_MAXW);
    for (int i = 0; i < n; ++i) {
        const stitch_pair_desc& d = pairs[i];
        if (!d.frame || !d.mosaic || !d_cov_a[i] || !d_cov_b[i]) return fail(STITCH_ERR_ARG, "pairs_seam_path: pair %d has no frame, no mosaic or no mask", i);
        if (d.fw < 1 || d.fh < 1 || d.mw < 1 || d.mh < 1) return fail(STITCH_ERR_ARG, "pairs_seam_path: pair %d has a bad size %d x %d / %d x %d", i, d.fw, d.fh, d.mw, d.mh);
        if (branches[i] != 0 && branches[i] != 1) return fail(STITCH_ERR_ARG, "pairs_seam_path: pair %d has branch %d (0 or 1)", i, branches[i]);
    }
    int rc = need_device();
    if (rc) return rc;
    hipStream_t s = as_stream(stream);
    std::vector<SeamPathPair> tab((size_t)n);
    for (int i = 0; i < n; ++i) tab[i] = seam_path_pair(pairs[i], d_cov_a[i], d_cov_b[i], branches[i]);
    const size_t states = (size_t)(cw + 1) * ch * n;
    PanoArena A(s);
    SeamPathPair* d_tab = nullptr;
    unsigned* d_cost = nullptr;
    uint8_t* d_pred = nullptr;
    if ((rc = A.take(&d_tab, sizeof(SeamPathPair) * n)) || (rc = A.take(&d_cost, sizeof(unsigned) * states)) || (rc = A.take(&d_pred, states))) return rc;
    const int32_t** d_atab = nullptr;
    if (d_anchors && (rc = A.take(&d_atab, sizeof(int32_t*) * n))) return rc;
    PanoWait wait{s};  // `tab` (and the caller's anchor table) is read by its upload
    HIPCHK(hipMemcpyAsync(d_tab, tab.data(), sizeof(SeamPathPair) * n, hipMemcpyHostToDevice, s));
    if (d_anchors) HIPCHK(hipMemcpyAsync(d_atab, d_anchors, sizeof(int32_t*) * n, hipMemcpyHostToDevice, s));
    k_seam_path_cost<<<dim3((unsigned)ch, (unsigned)n), SP_CT, 0, s>>>(d_tab, cw, ch, o.margin, d_cost);
    if ((rc = launch_check("k_seam_path_cost"))) return rc;
    if (!d_anchors) return seam_path_dp(d_cost, n, cw, ch, o.max_step, d_pred, d_paths, (size_t)ch, d_costs, 1, s);
    const SeamAnchor an{d_atab, nullptr, 0, (unsigned)ao->weight, (unsigned)ao->cap, reinterpret_cast<unsigned long long*>(d_moved), 1};
    return seam_path_dp(d_cost, n, cw, ch, o.max_step, d_pred, d_paths, (size_t)ch, d_costs, 1, s, &an);
}

}  // namespace

extern "C" {

int stitch_dev_pairs_seam_path_u8(const stitch_pair_desc* pairs, int n, int cw, int ch, const uint8_t* const* d_cov_a, const uint8_t* const* d_cov_b,
                                  const int32_t* branches, const stitch_seam_path_opts* opts, int32_t* d_paths, uint64_t* d_costs, void* stream) {
    return pairs_seam_path(pairs, n, cw, ch, d_cov_a, d_cov_b, branches, opts, d_paths, d_costs, stream, nullptr, nullptr, nullptr);
}

int stitch_dev_pairs_seam_path_anchored_u8(const stitch_pair_desc* pairs, int n, int cw, int ch, const uint8_t* const* d_cov_a, const uint8_t* const* d_cov_b,
                                           const int32_t* branches, const stitch_seam_path_opts* opts, const int32_t* const* d_anchors,
                                           const stitch_seam_anchor_opts* aopts, int32_t* d_paths, uint64_t* d_costs, uint64_t* d_moved, void* stream) {
    if (!d_anchors || !aopts || !d_moved) return fail(STITCH_ERR_ARG, "pairs_seam_path_anchored: null anchor table, anchor options or moved array");
    if (!seam_anchor_opts_ok(*aopts))
        return fail(STITCH_ERR_ARG, "pairs_seam_path_anchored: weight %d below 0, cap %d below 1, or weight * cap above %d", aopts->weight, aopts->cap, STITCH_SEAM_ANCHOR_MAX);
    return pairs_seam_path(pairs, n, cw, ch, d_cov_a, d_cov_b, branches, opts, d_paths, d_costs, stream, d_anchors, aopts, d_moved);
}

}  // extern "C"
