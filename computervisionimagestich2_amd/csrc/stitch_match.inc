// stitch_match.inc -- host side of the descriptor matcher (include/stitch.h, "descriptor matching"; kernels in k_match.inc).
// Included at the end of stitch_hip.hip (one translation unit).
//
// A launch sequence covers up to MATCH_MAXSETS sets: k_match_partial over (query blocks, slabs, sets), k_match_merge over
// (query blocks, 1, sets), k_match_compact over sets.  The data set of each entry is cut into `nslabs` slabs (one count for the
// launch, a slab length per set) so that a small problem -- a few hundred descriptors per frame -- still spreads over the chip.
// Scratch (the per-slab top-2 partials and the per-query verdicts) is stream-ordered: allocated and freed on the caller's stream.
namespace {

constexpr int kMatchTargetWgs = 1536;  // two rounds of k_match_partial's workgroups on 256 CUs (three resident per CU)
constexpr int kMatchMinSlab = 16;      // data rows per slab at least: a workgroup loads 128 KB of queries

int match_check(const stitch_match_desc& d, int i) {
    if (d.n_db < 0 || d.n_query < 0) return fail(STITCH_ERR_ARG, "match: set %d has negative sizes %d x %d", i, d.n_db, d.n_query);
    if (!d.count) return fail(STITCH_ERR_ARG, "match: set %d has no count buffer", i);
    if (d.n_query > 0 && (!d.query || !d.pairs)) return fail(STITCH_ERR_ARG, "match: set %d has no query or pair buffer", i);
    if (d.n_db > 0 && d.n_query > 0 && !d.db) return fail(STITCH_ERR_ARG, "match: set %d has no data buffer", i);
    return STITCH_OK;
}

int match_launch(const stitch_match_desc* d, int n, double ratio, hipStream_t s) {
    int max_nq = 0, max_nd = 0, qblocks = 0;
    for (int i = 0; i < n; ++i) {
        max_nq = std::max(max_nq, d[i].n_query);
        max_nd = std::max(max_nd, d[i].n_db);
        qblocks += (d[i].n_query + MATCH_QB - 1) / MATCH_QB;
    }
    const int nslabs = qblocks == 0 ? 1
                                    : std::max(1, std::min((kMatchTargetWgs + qblocks - 1) / qblocks,
                                                           (max_nd + kMatchMinSlab - 1) / kMatchMinSlab));
    size_t bytes = 0;
    for (int i = 0; i < n; ++i) bytes += align256((size_t)nslabs * d[i].n_query * 3 * sizeof(float)) + align256((size_t)d[i].n_query * 4);
    char* scratch = nullptr;
    if (bytes) HIPCHK(hipMallocAsync((void**)&scratch, bytes, s));
    MatchArgs a;
    std::memset(&a, 0, sizeof a);
    a.nslabs = nslabs;
    a.ratio = ratio;
    size_t off = 0;
    for (int i = 0; i < n; ++i) {
        MatchSet& m = a.s[i];
        const size_t nq = (size_t)d[i].n_query;
        m.db = d[i].db;
        m.query = d[i].query;
        m.nn = d[i].nn;
        m.dist2 = d[i].dist2;
        m.pairs = d[i].pairs;
        m.count = d[i].count;
        m.n_db = d[i].n_db;
        m.n_query = d[i].n_query;
        m.slab = (d[i].n_db + nslabs - 1) / nslabs;
        m.slab = (m.slab + MATCH_UNROLL - 1) / MATCH_UNROLL * MATCH_UNROLL;
        m.part_d = reinterpret_cast<float*>(scratch + off);
        m.part_i = reinterpret_cast<int32_t*>(scratch + off + (size_t)nslabs * nq * 2 * sizeof(float));
        off += align256((size_t)nslabs * nq * 3 * sizeof(float));
        m.acc = reinterpret_cast<int32_t*>(scratch + off);
        off += align256(nq * 4);
    }
    int rc = STITCH_OK;
    if (max_nq > 0) {
        const unsigned qb = (unsigned)((max_nq + MATCH_QB - 1) / MATCH_QB);
        k_match_partial<<<dim3(qb, (unsigned)nslabs, (unsigned)n), MATCH_QB, 0, s>>>(a);
        if ((rc = launch_check("k_match_partial"))) return rc;  // (scratch is not freed: the stream is broken anyway)
        k_match_merge<<<dim3(qb, 1, (unsigned)n), MATCH_QB, 0, s>>>(a);
        if ((rc = launch_check("k_match_merge"))) return rc;
    }
    k_match_compact<<<(unsigned)n, MATCH_COMPACT_T, 0, s>>>(a);
    if ((rc = launch_check("k_match_compact"))) return rc;
    if (scratch) HIPCHK(hipFreeAsync(scratch, s));
    return STITCH_OK;
}

}  // namespace

extern "C" {

int stitch_dev_match_l1_ratio_many(const stitch_match_desc* descs, int n, double ratio, void* stream) {
    int rc = need_device();
    if (rc) return rc;
    if (n < 0 || (n > 0 && !descs)) return fail(STITCH_ERR_ARG, "match: bad set list (n = %d)", n);
    if (std::isnan(ratio)) return fail(STITCH_ERR_ARG, "match: ratio is NaN");
    for (int i = 0; i < n; ++i)
        if ((rc = match_check(descs[i], i))) return rc;
    for (int i = 0; i < n; i += MATCH_MAXSETS)
        if ((rc = match_launch(descs + i, std::min(MATCH_MAXSETS, n - i), ratio, as_stream(stream)))) return rc;
    return STITCH_OK;
}

int stitch_dev_match_l1_ratio(const float* d_db, int n_db, const float* d_query, int n_query, double ratio, int32_t* d_nn,
                              float* d_dist2, int32_t* d_pairs, int32_t* d_count, void* stream) {
    const stitch_match_desc d = {d_db, d_query, n_db, n_query, d_nn, d_dist2, d_pairs, d_count};
    return stitch_dev_match_l1_ratio_many(&d, 1, ratio, stream);
}

int stitch_match_l1_ratio(const float* db, int n_db, const float* query, int n_query, double ratio, int32_t* nn, float* dist2,
                          int32_t* pairs, int32_t* count) {
    int rc = need_device();
    if (rc) return rc;
    const stitch_match_desc h = {db, query, n_db, n_query, nn, dist2, pairs, count};
    if ((rc = match_check(h, 0))) return rc;
    const size_t nd = (size_t)std::max(n_db, 0), nq = (size_t)std::max(n_query, 0), row = STITCH_DESCRIPTOR_DIM * sizeof(float);
    DevBuf x, y, dn, dd, dp, dc;
    if ((rc = dc.alloc(sizeof(int32_t)))) return rc;
    if (nd && (rc = x.alloc(nd * row))) return rc;
    if (nq && ((rc = y.alloc(nq * row)) || (rc = dp.alloc(nq * 2 * sizeof(int32_t))))) return rc;
    if (nq && nn && (rc = dn.alloc(nq * sizeof(int32_t)))) return rc;
    if (nq && dist2 && (rc = dd.alloc(nq * 2 * sizeof(float)))) return rc;
    if (nd && nq) HIPCHK(hipMemcpy(x.p, db, nd * row, hipMemcpyHostToDevice));
    if (nq) HIPCHK(hipMemcpy(y.p, query, nq * row, hipMemcpyHostToDevice));
    if ((rc = stitch_dev_match_l1_ratio(x.as<float>(), n_db, y.as<float>(), n_query, ratio, dn.as<int32_t>(), dd.as<float>(),
                                        dp.as<int32_t>(), dc.as<int32_t>(), nullptr)))
        return rc;
    int32_t c = 0;
    HIPCHK(hipMemcpy(&c, dc.p, sizeof c, hipMemcpyDeviceToHost));
    *count = c;
    if (c > 0) HIPCHK(hipMemcpy(pairs, dp.p, (size_t)c * 2 * sizeof(int32_t), hipMemcpyDeviceToHost));
    if (nq && nn) HIPCHK(hipMemcpy(nn, dn.p, nq * sizeof(int32_t), hipMemcpyDeviceToHost));
    if (nq && dist2) HIPCHK(hipMemcpy(dist2, dd.p, nq * 2 * sizeof(float), hipMemcpyDeviceToHost));
    return STITCH_OK;
}

}  // extern "C"
