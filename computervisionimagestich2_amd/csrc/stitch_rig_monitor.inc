// stitch_rig_monitor.inc -- a rig's alignment monitor: overlap residuals over integer shifts (include/stitch_rig_monitor.h, which is
// the specification; kernels in k_rig_monitor.inc).  Included at the end of stitch_hip.hip (one translation unit).
//
// The rig's side is four hooks that rig_stitch (stitch_rig.inc) calls only while a monitor is set: the domains once per rig and
// radius, the zeroing of a sequence's records, one launch per step over the m sets in flight -- from the pair descriptors the
// step's blend is about to receive -- and the one copy that takes a sequence's records to the host.
namespace {

inline bool residual_radius_ok(int r) { return r >= 0 && r <= RES_MAXR; }
inline int residual_words(int r) { return 2 + 3 * (2 * r + 1) * (2 * r + 1); }
inline dim3 residual_grid(int x0, int y0, int x1, int y1, int n) {
    return dim3((unsigned)((x1 - x0 + RES_TW - 1) / RES_TW), (unsigned)((y1 - y0 + RES_TH - 1) / RES_TH), (unsigned)n);
}

// D_k of step k at radius r into `plane` (the step's wpr * ch words) and its box into d_box (4 words, zeroed here)
int rig_mon_domain(const stitch_rig* R, int k, int r, unsigned long long* plane, unsigned* d_box, hipStream_t s) {
    const int cw = R->steps[k].geom.cw, ch = R->steps[k].geom.ch, wpr = cover_wpr(cw);
    const size_t words = (size_t)wpr * ch;
    const unsigned long long* A = R->cover + R->cover_step[k];
    HIPCHK(hipMemsetAsync(d_box, 0, sizeof(unsigned) * 4, s));
    k_residual_domain<<<(unsigned)((words + 255) / 256), 256, 0, s>>>(A, A + words, cw, ch, wpr, r, plane, d_box);
    return launch_check("k_residual_domain");
}

// the box a launch covers: the domain's bounding box inside the margin r (empty: w = 0)
stitch_rect residual_box(const unsigned b[4], int cw, int ch, int r) {
    if (!b[2]) return stitch_rect{0, 0, 0, 0};
    const int x0 = std::max(cw - (int)b[0], r), y0 = std::max(ch - (int)b[1], r), x1 = std::min((int)b[2], cw - r), y1 = std::min((int)b[3], ch - r);
    if (x1 <= x0 || y1 <= y0) return stitch_rect{0, 0, 0, 0};
    return stitch_rect{x0 & ~63, y0, x1 - (x0 & ~63), y1 - y0};  // whole domain words per tile row (the margin test is per pixel)
}

ResPair residual_pair(const stitch_pair_desc& d) {
    ResPair p;
    std::memset(&p, 0, sizeof p);
    p.frame = static_cast<const uint8_t*>(d.frame);
    p.mosaic = static_cast<const uint8_t*>(d.mosaic);
    std::memcpy(p.map.p, d.p, sizeof p.map.p);
    p.offx = d.offx;
    p.offy = d.offy;
    p.fw = d.fw;
    p.fh = d.fh;
    p.mw = d.mw;
    p.mh = d.mh;
    p.ox = d.ox;
    p.oy = d.oy;
    return p;
}

// The monitor's device state for the rig's radius, on the current device: the coverage planes if the rig has none yet, D_k and its
// box for every step, the records of one sequence.  Waits for `s` when it computes.
int rig_mon_prepare(stitch_rig* R, hipStream_t s) {
    const int ns = (int)R->steps.size(), r = R->mon_radius;
    if (!ns) return STITCH_OK;
    int rc = rig_cover(R, s);
    if (rc) return rc;
    if (!R->mon_dom) {
        std::vector<size_t> at((size_t)ns);
        size_t words = 0;
        for (int k = 0; k < ns; ++k) {
            at[k] = words;
            words += (size_t)cover_wpr(R->steps[k].geom.cw) * R->steps[k].geom.ch;
        }
        HIPCHK(hipMalloc((void**)&R->mon_dom, sizeof(unsigned long long) * words + sizeof(unsigned) * 4 * ns));
        R->mon_dom_at = at;
        R->mon_dom_words = words;
    }
    if (R->mon_dom_radius != r) {
        unsigned* d_box = reinterpret_cast<unsigned*>(R->mon_dom + R->mon_dom_words);
        for (int k = 0; k < ns; ++k)
            if ((rc = rig_mon_domain(R, k, r, R->mon_dom + R->mon_dom_at[k], d_box + 4 * k, s))) return rc;
        std::vector<unsigned> box((size_t)4 * ns);
        HIPCHK(hipMemcpyAsync(box.data(), d_box, sizeof(unsigned) * box.size(), hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
        R->mon_box.resize((size_t)ns);
        for (int k = 0; k < ns; ++k) R->mon_box[k] = residual_box(&box[4 * (size_t)k], R->steps[k].geom.cw, R->steps[k].geom.ch, r);
        R->mon_dom_radius = r;
    }
    if (!R->mon_rec) HIPCHK(hipMalloc((void**)&R->mon_rec, sizeof(unsigned long long) * RES_MAXWORDS * ns * R->max_sets));
    return STITCH_OK;
}

// a sequence of m sets begins: its records, set-major then step, are zero
int rig_mon_begin(stitch_rig* R, int m, hipStream_t s) {
    HIPCHK(hipMemsetAsync(R->mon_rec, 0, sizeof(unsigned long long) * residual_words(R->mon_radius) * R->steps.size() * m, s));
    return STITCH_OK;
}

// step k of the m sets in flight, from the descriptors its blend receives
int rig_mon_step(stitch_rig* R, const stitch_pair_desc* pd, int k, int m, hipStream_t s) {
    const stitch_rect& b = R->mon_box[k];
    if (b.w < 1) return STITCH_OK;  // an empty domain: the records stay zero
    const int ns = (int)R->steps.size(), r = R->mon_radius, words = residual_words(r);
    const int cw = R->steps[k].geom.cw, ch = R->steps[k].geom.ch;
    ResArgs a;
    for (int i = 0; i < m; ++i) {
        ResPair& p = a.p[i] = residual_pair(pd[i]);
        p.domain = R->mon_dom + R->mon_dom_at[k];
        p.rec = R->mon_rec + ((size_t)i * ns + k) * words;
        p.x0 = b.x0;
        p.y0 = b.y0;
        p.x1 = b.x0 + b.w;
        p.y1 = b.y0 + b.h;
    }
    for (int i = m; i < MAXB; ++i) a.p[i] = a.p[0];
    k_pairs_residual_step<<<residual_grid(b.x0, b.y0, b.x0 + b.w, b.y0 + b.h, m), 256, 0, s>>>(a, cw, ch, cover_wpr(cw), r);
    return launch_check("k_pairs_residual_step");
}

// the sequence's records leave the device in one copy, behind its last step
int rig_mon_collect(stitch_rig* R, uint64_t* host, int m, hipStream_t s) {
    HIPCHK(hipMemcpyAsync(host, R->mon_rec, sizeof(uint64_t) * residual_words(R->mon_radius) * R->steps.size() * m, hipMemcpyDeviceToHost, s));
    return STITCH_OK;
}

}  // namespace

extern "C" {

int stitch_residual_words(int radius) { return residual_radius_ok(radius) ? residual_words(radius) : 0; }

int stitch_dev_pairs_residual_u8(const stitch_pair_desc* pairs, int n, int cw, int ch, const uint8_t* const* d_domain, int radius, uint64_t* d_records,
                                 void* stream) {
    if (!pairs || !d_domain || !d_records) return fail(STITCH_ERR_ARG, "pairs_residual: null argument");
    if (!residual_radius_ok(radius)) return fail(STITCH_ERR_ARG, "pairs_residual: radius %d outside 0 .. %d", radius, RES_MAXR);
    if (n < 1 || n > kRigMaxImages) return fail(STITCH_ERR_ARG, "pairs_residual: %d pairs (1 .. %d)", n, kRigMaxImages);
    if (cw < 1 || ch < 1 || (long long)cw * ch > 0x7fffffffLL || ch > 65535 * RES_TH)
        return fail(STITCH_ERR_ARG, "pairs_residual: bad canvas %d x %d (sizes >= 1, w * h <= 2^31 - 1, h <= %d)", cw, ch, 65535 * RES_TH);
    for (int i = 0; i < n; ++i) {
        const stitch_pair_desc& d = pairs[i];
        if (!d.frame || !d.mosaic || !d_domain[i]) return fail(STITCH_ERR_ARG, "pairs_residual: pair %d has no frame, no mosaic or no mask", i);
        if (d.fw < 1 || d.fh < 1 || d.mw < 1 || d.mh < 1) return fail(STITCH_ERR_ARG, "pairs_residual: pair %d has a bad size %d x %d / %d x %d", i, d.fw, d.fh, d.mw, d.mh);
    }
    int rc = need_device();
    if (rc) return rc;
    hipStream_t s = as_stream(stream);
    const int words = residual_words(radius);
    HIPCHK(hipMemsetAsync(d_records, 0, sizeof(uint64_t) * words * n, s));
    if (cw <= 2 * radius || ch <= 2 * radius) return STITCH_OK;  // no pixel keeps its shifted reads inside the canvas
    std::vector<ResPair> tab((size_t)n);
    for (int i = 0; i < n; ++i) {
        ResPair& p = tab[i] = residual_pair(pairs[i]);
        p.domain = d_domain[i];
        p.rec = reinterpret_cast<unsigned long long*>(d_records) + (size_t)i * words;
        p.x0 = p.y0 = radius;
        p.x1 = cw - radius;
        p.y1 = ch - radius;
    }
    PanoArena A(s);
    ResPair* d_tab = nullptr;
    if ((rc = A.take(&d_tab, sizeof(ResPair) * n))) return rc;
    PanoWait wait{s};  // `tab` is read by its upload
    HIPCHK(hipMemcpyAsync(d_tab, tab.data(), sizeof(ResPair) * n, hipMemcpyHostToDevice, s));
    k_pairs_residual<true><<<residual_grid(radius, radius, cw - radius, ch - radius, n), 256, 0, s>>>(d_tab, cw, ch, 0, radius);
    return launch_check("k_pairs_residual");
}

int stitch_rig_set_monitor(stitch_rig* rig, int radius) {
    if (!rig || !residual_radius_ok(radius)) return fail(STITCH_ERR_ARG, "rig_set_monitor: null handle or radius %d outside 0 .. %d", radius, RES_MAXR);
    rig->mon_radius = radius;
    return STITCH_OK;
}

int stitch_rig_clear_monitor(stitch_rig* rig) {
    if (!rig) return fail(STITCH_ERR_ARG, "rig_clear_monitor: null handle");
    rig->mon_radius = -1;
    rig->mon_last.clear();
    rig->mon_last_sets = 0;
    return STITCH_OK;
}

int stitch_rig_monitor(const stitch_rig* rig, int* radius) {
    if (!rig) return fail(STITCH_ERR_ARG, "rig_monitor: null handle");
    if (radius) *radius = rig->mon_radius;
    return STITCH_OK;
}

int stitch_rig_residuals(const stitch_rig* rig, uint64_t* out, size_t cap_words, int* n_sets, int* n_steps, int* radius) {
    if (!rig) return fail(STITCH_ERR_ARG, "rig_residuals: null handle");
    if (n_sets) *n_sets = rig->mon_last_sets;
    if (n_steps) *n_steps = (int)rig->steps.size();
    if (radius) *radius = rig->mon_last_sets ? rig->mon_last_radius : rig->mon_radius;
    if (out) {
        if (cap_words < rig->mon_last.size()) return fail(STITCH_ERR_ARG, "rig_residuals: room for %zu words, the records take %zu", cap_words, rig->mon_last.size());
        if (!rig->mon_last.empty()) std::memcpy(out, rig->mon_last.data(), sizeof(uint64_t) * rig->mon_last.size());
    }
    return STITCH_OK;
}

int stitch_dev_rig_residual_domain_u8(stitch_rig* rig, int step, int radius, uint8_t* d_mask, void* stream) {
    if (!rig || !d_mask) return fail(STITCH_ERR_ARG, "rig_residual_domain: null handle or mask");
    const int ns = (int)rig->steps.size();
    if (ns == 0) return fail(STITCH_ERR_ARG, "rig_residual_domain: the rig has no steps");
    if (step < -1 || step >= ns) return fail(STITCH_ERR_ARG, "rig_residual_domain: step %d outside -1 .. %d", step, ns - 1);
    if (!residual_radius_ok(radius)) return fail(STITCH_ERR_ARG, "rig_residual_domain: radius %d outside 0 .. %d", radius, RES_MAXR);
    int rc = need_device();
    if (rc) return rc;
    hipStream_t s = as_stream(stream);
    if ((rc = rig_cover(rig, s))) return rc;
    const int k = step < 0 ? ns - 1 : step, w = rig->steps[k].geom.cw, h = rig->steps[k].geom.ch, wpr = cover_wpr(w);
    PanoArena A(s);  // a plane of its own: the rig's, if it has them, may be of another radius, and stay as they are
    unsigned long long* plane = nullptr;
    if ((rc = A.take(&plane, sizeof(unsigned long long) * ((size_t)wpr * h + 2)))) return rc;
    if ((rc = rig_mon_domain(rig, k, radius, plane, reinterpret_cast<unsigned*>(plane + (size_t)wpr * h), s))) return rc;
    k_cover_bytes<<<grid_xy(w, h), 256, 0, s>>>(plane, wpr, w, h, d_mask);
    return launch_check("k_cover_bytes");
}

int stitch_residual_best_shift(const uint64_t* record, int radius, int zero_mean, int* dx_out, int* dy_out) {
    if (!record || !residual_radius_ok(radius)) return fail(STITCH_ERR_ARG, "residual_best_shift: null record or radius %d outside 0 .. %d", radius, RES_MAXR);
    const uint64_t n = record[0], sum_b = record[1];
    if (n == 0) return fail(STITCH_ERR_ZERO_OVERLAP, "residual_best_shift: the record's domain is empty");
    typedef unsigned __int128 u128;
    u128 best = 0;
    int bx = 0, by = 0;
    bool have = false;
    for (int dy = -radius, j = 0; dy <= radius; ++dy)
        for (int dx = -radius; dx <= radius; ++dx, ++j) {
            const uint64_t sum_a = record[2 + 3 * j], ssd = record[4 + 3 * j];
            u128 score = ssd;
            if (zero_mean) {
                const u128 d = sum_a > sum_b ? sum_a - sum_b : sum_b - sum_a;
                score = (u128)n * ssd - d * d;  // n * sum d^2 >= (sum d)^2
            }
            const int d2 = dx * dx + dy * dy, b2 = bx * bx + by * by;
            // (rows come in ascending dy, then dx: an exact tie at the same distance keeps the earlier one)
            if (!have || score < best || (score == best && d2 < b2)) {
                have = true;
                best = score;
                bx = dx;
                by = dy;
            }
        }
    if (dx_out) *dx_out = bx;
    if (dy_out) *dy_out = by;
    return STITCH_OK;
}

}  // extern "C"
