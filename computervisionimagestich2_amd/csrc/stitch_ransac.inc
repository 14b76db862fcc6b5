// stitch_ransac.inc -- host side of the map estimation (include/stitch.h, "RANSAC"; kernels in k_ransac.inc).
// Included at the end of stitch_hip.hip (one translation unit).
//
// A launch sequence covers up to RANSAC_MAXLISTS lists with six kernels (k_ransac.inc lists them).  The consensus count cuts the
// points into `nslabs` slabs across workgroups so that 72 rounds -- two wavefronts -- still spread over the chip.  Scratch is
// stream-ordered: allocated and freed on the caller's stream; nothing here waits for the device.
namespace {

constexpr int kRansacTargetWgs = 2048;  // workgroups of k_ransac_count aimed at (one wavefront each: 8 per CU)
constexpr int kRansacMinSlab = 64;      // points per slab at least
constexpr int kRansacMaxRounds = 16384;
constexpr int kRansacMaxPairs = 1 << 24;

// The smallest float s with sqrtf(s) >= t, or 0 when no sum of squares can pass `sqrtf(s) < t` (t <= 0 or NaN).  sqrtf is
// correctly rounded, hence monotone: bisection over the bit patterns of the non-negative floats (+inf included) finds it.
float ransac_s_star(float t) {
    if (!(t > 0)) return 0.0f;
    uint32_t lo = 0, hi = 0x7f800000u;  // sqrtf(+inf) = +inf >= t always holds at hi
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo) / 2;
        float s;
        std::memcpy(&s, &mid, sizeof s);
        if (std::sqrt(s) >= t)
            hi = mid;
        else
            lo = mid + 1;
    }
    float s;
    std::memcpy(&s, &lo, sizeof s);
    return s;
}

struct RansacCfg {
    int rounds, draw_cap;
    uint32_t seed;
    float s_star;
};

int ransac_cfg(const stitch_ransac_opts* o, RansacCfg* c) {
    const int rounds = o && o->rounds ? o->rounds : STITCH_RANSAC_ROUNDS;
    if (rounds < 1 || rounds > kRansacMaxRounds) return fail(STITCH_ERR_ARG, "ransac: rounds = %d (1 .. %d)", rounds, kRansacMaxRounds);
    if (o && o->max_draws < 0) return fail(STITCH_ERR_ARG, "ransac: max_draws = %d", o->max_draws);
    c->rounds = rounds;
    c->draw_cap = o && o->max_draws ? o->max_draws : 32 * rounds + 4096;
    c->seed = o ? o->seed : STITCH_RANSAC_SEED;
    c->s_star = ransac_s_star(o ? o->threshold : STITCH_RANSAC_THRESHOLD);
    return STITCH_OK;
}

int ransac_check(const stitch_ransac_desc& d, int i) {
    if (d.n_max < 0 || d.n_max > kRansacMaxPairs) return fail(STITCH_ERR_ARG, "ransac: list %d has n_max = %d", i, d.n_max);
    if (!d.p || !d.info) return fail(STITCH_ERR_ARG, "ransac: list %d has no p or info buffer", i);
    if (d.n_max > 0 && (!d.src_x || !d.src_y || !d.dst_x || !d.dst_y)) return fail(STITCH_ERR_ARG, "ransac: list %d lacks a coordinate array", i);
    return STITCH_OK;
}

int ransac_launch(const stitch_ransac_desc* d, int n, const RansacCfg& c, hipStream_t s) {
    const size_t K = (size_t)c.rounds;
    int max_n = 0;
    size_t bytes = 0;
    for (int i = 0; i < n; ++i) {
        const size_t m = (size_t)d[i].n_max;
        max_n = std::max(max_n, d[i].n_max);
        bytes += align256(K * 8 * sizeof(double)) + align256(m * 4 * sizeof(double)) + align256(m * 4 * sizeof(float)) +
                 align256(K * 4 * sizeof(int32_t)) + align256(K * sizeof(int32_t)) + align256(8 * sizeof(int32_t)) +
                 (d[i].inliers ? 0 : align256(m * sizeof(int32_t)));
    }
    char* scratch = nullptr;
    HIPCHK(hipMallocAsync((void**)&scratch, bytes, s));
    RansacArgs a;
    std::memset(&a, 0, sizeof a);
    const int kblocks = (c.rounds + RANSAC_ROUND_T - 1) / RANSAC_ROUND_T;
    a.rounds = c.rounds;
    a.nslabs = std::max(1, std::min(kRansacTargetWgs / (n * kblocks), (max_n + kRansacMinSlab - 1) / kRansacMinSlab));
    a.slab = std::max(1, (max_n + a.nslabs - 1) / a.nslabs);
    a.draw_cap = c.draw_cap;
    a.seed = c.seed;
    a.s_star = c.s_star;
    size_t off = 0;
    auto take = [&](size_t b) {
        char* p = scratch + off;
        off += align256(b);
        return p;
    };
    for (int i = 0; i < n; ++i) {
        RansacList& l = a.l[i];
        const size_t m = (size_t)d[i].n_max;
        l.src_x = d[i].src_x;
        l.src_y = d[i].src_y;
        l.dst_x = d[i].dst_x;
        l.dst_y = d[i].dst_y;
        l.pairs = d[i].pairs;
        l.count = d[i].count;
        l.p = d[i].p;
        l.info = d[i].info;
        l.n_max = d[i].n_max;
        l.mirror = d[i].mirror != 0;
        l.hyp = reinterpret_cast<double*>(take(K * 8 * sizeof(double)));
        l.U = reinterpret_cast<double*>(take(m * 4 * sizeof(double)));
        l.pts = reinterpret_cast<float*>(take(m * 4 * sizeof(float)));
        l.idx = reinterpret_cast<int32_t*>(take(K * 4 * sizeof(int32_t)));
        l.cnt = reinterpret_cast<int32_t*>(take(K * sizeof(int32_t)));
        l.hdr = reinterpret_cast<int32_t*>(take(8 * sizeof(int32_t)));
        l.inliers = d[i].inliers ? d[i].inliers : reinterpret_cast<int32_t*>(take(m * sizeof(int32_t)));
    }
    int rc = STITCH_OK;
    const unsigned prep = (unsigned)std::max(1, std::min(64, (std::max(max_n, c.rounds) + RANSAC_PREP_T - 1) / RANSAC_PREP_T));
    k_ransac_prepare<<<dim3(prep, (unsigned)n), RANSAC_PREP_T, 0, s>>>(a);
    if ((rc = launch_check("k_ransac_prepare"))) return rc;  // (scratch is not freed: the stream is broken anyway)
    k_ransac_sample<<<(unsigned)n, WAVE, 0, s>>>(a);
    if ((rc = launch_check("k_ransac_sample"))) return rc;
    k_ransac_hyp<<<dim3((unsigned)kblocks, (unsigned)n), RANSAC_ROUND_T, 0, s>>>(a);
    if ((rc = launch_check("k_ransac_hyp"))) return rc;
    k_ransac_count<<<dim3((unsigned)kblocks, (unsigned)a.nslabs, (unsigned)n), RANSAC_ROUND_T, 0, s>>>(a);
    if ((rc = launch_check("k_ransac_count"))) return rc;
    k_ransac_select<<<(unsigned)n, RANSAC_SELECT_T, 0, s>>>(a);
    if ((rc = launch_check("k_ransac_select"))) return rc;
    k_ransac_fit<<<(unsigned)n, RANSAC_FIT_T, 0, s>>>(a);
    if ((rc = launch_check("k_ransac_fit"))) return rc;
    HIPCHK(hipFreeAsync(scratch, s));
    return STITCH_OK;
}

}  // namespace

extern "C" {

int stitch_dev_ransac_many(const stitch_ransac_desc* descs, int n, const stitch_ransac_opts* opts, void* stream) {
    int rc = need_device();
    if (rc) return rc;
    if (n < 0 || (n > 0 && !descs)) return fail(STITCH_ERR_ARG, "ransac: bad list of lists (n = %d)", n);
    RansacCfg c;
    if ((rc = ransac_cfg(opts, &c))) return rc;
    for (int i = 0; i < n; ++i)
        if ((rc = ransac_check(descs[i], i))) return rc;
    for (int i = 0; i < n; i += RANSAC_MAXLISTS)
        if ((rc = ransac_launch(descs + i, std::min(RANSAC_MAXLISTS, n - i), c, as_stream(stream)))) return rc;
    return STITCH_OK;
}

int stitch_ransac(const float* src_x, const float* src_y, const float* dst_x, const float* dst_y, int n, int mirror,
                  const stitch_ransac_opts* opts, double p[8], int32_t* inliers, int32_t info[STITCH_RANSAC_INFO]) {
    int rc = need_device();
    if (rc) return rc;
    if (n < 0 || n > kRansacMaxPairs) return fail(STITCH_ERR_ARG, "ransac: n = %d", n);
    if (!p || !info || (n > 0 && (!src_x || !src_y || !dst_x || !dst_y))) return fail(STITCH_ERR_ARG, "ransac: missing buffer");
    const size_t m = (size_t)n, col = align256(m * sizeof(float));
    DevBuf xy, dp, di, dl;
    if (n && (rc = xy.alloc(4 * col))) return rc;
    if ((rc = dp.alloc(8 * sizeof(double))) || (rc = di.alloc(STITCH_RANSAC_INFO * sizeof(int32_t)))) return rc;
    if (n && inliers && (rc = dl.alloc(m * sizeof(int32_t)))) return rc;
    const float* host[4] = {src_x, src_y, dst_x, dst_y};
    float* dev[4] = {nullptr, nullptr, nullptr, nullptr};
    for (int k = 0; k < 4 && n; ++k) {
        dev[k] = reinterpret_cast<float*>(static_cast<char*>(xy.p) + k * col);
        HIPCHK(hipMemcpy(dev[k], host[k], m * sizeof(float), hipMemcpyHostToDevice));
    }
    stitch_ransac_desc d;
    std::memset(&d, 0, sizeof d);
    d.src_x = dev[0];
    d.src_y = dev[1];
    d.dst_x = dev[2];
    d.dst_y = dev[3];
    d.n_max = n;
    d.mirror = mirror;
    d.p = dp.as<double>();
    d.inliers = dl.as<int32_t>();
    d.info = di.as<int32_t>();
    if ((rc = stitch_dev_ransac_many(&d, 1, opts, nullptr))) return rc;
    HIPCHK(hipMemcpy(p, dp.p, 8 * sizeof(double), hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(info, di.p, STITCH_RANSAC_INFO * sizeof(int32_t), hipMemcpyDeviceToHost));
    if (n && inliers) HIPCHK(hipMemcpy(inliers, dl.p, m * sizeof(int32_t), hipMemcpyDeviceToHost));
    return STITCH_OK;
}

void stitch_ransac_rand(uint32_t seed, int32_t* out, int n) {
    int32_t state[31];
    RansacRand g{state, 0, 0};
    g.seed(seed);
    for (int i = 0; i < n; ++i) out[i] = g.next();
}

}  // extern "C"
