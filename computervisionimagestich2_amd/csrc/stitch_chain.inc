// stitch_chain.inc -- what the host chains share (stitch_panorama.inc, stitch_rig.inc, stitch_exposure.inc,
// stitch_rig_exposure.inc, stitch_calibrate.inc): the stream-ordered scratch of a call, the SIFT front end from frames to ordered
// feature sets, the all-pairs matching and the two estimations of a step with their device block.  Host code only; included in
// stitch_hip.hip (one translation unit) before the chains.
#include <memory>

namespace {

// Stream-ordered blocks of one call: whatever is still listed when the call ends -- on every error path too -- is freed on the
// call's stream.  give_up() hands a block over to the result handle.
struct PanoArena {
    hipStream_t s;
    std::vector<void*> blocks;
    explicit PanoArena(hipStream_t s_) : s(s_) {}
    ~PanoArena() {
        for (void* p : blocks) (void)hipFreeAsync(p, s);
    }
    template <typename T>
    int take(T** out, size_t bytes) {
        void* p = nullptr;
        keep_pool_memory();
        HIPCHK(hipMallocAsync(&p, std::max<size_t>(bytes, 4), s));
        blocks.push_back(p);
        *out = static_cast<T*>(p);
        return STITCH_OK;
    }
    void forget(void* p) { blocks.erase(std::remove(blocks.begin(), blocks.end(), p), blocks.end()); }
    void give_up(void* p) { forget(p); }
    void release(void* p) {
        forget(p);
        (void)hipFreeAsync(p, s);
    }
};

int pano_sync(hipStream_t s) {
    HIPCHK(hipStreamSynchronize(s));
    return STITCH_OK;
}

// Declared behind a host buffer that an enqueued copy reads: no return path lets the buffer go before the copy has run.
struct PanoWait {
    hipStream_t s;
    bool armed = true;  // false: a member that waits only once its owner has enqueued the copy
    ~PanoWait() {
        if (armed) (void)hipStreamSynchronize(s);
    }
};

// The tail of a chain: wait for the stream (what the arena frees next is idle, every host buffer has been read by its upload),
// then the handle leaves the call unless the chain or the wait failed.
template <typename T>
int chain_publish(int rc, hipStream_t s, std::unique_ptr<T>& handle, T** out) {
    const int rc2 = pano_sync(s);
    if (rc) return rc;
    if (rc2) return rc2;
    *out = handle.release();
    return STITCH_OK;
}

int chain_check_exposure(const stitch_exposure_opts& ex, const char* who) {
    if (ex.mode < 0 || ex.mode > 2) return fail(STITCH_ERR_ARG, "%s: exposure mode %d (0 .. 2)", who, ex.mode);
    if (ex.stats_form < 0 || ex.stats_form > 2) return fail(STITCH_ERR_ARG, "%s: exposure stats_form %d (0 .. 2)", who, ex.stats_form);
    return STITCH_OK;
}

bool feature_set_lacks_array(const stitch_feature_set& f) { return f.n < 0 || (f.n > 0 && (!f.d_desc || !f.d_x || !f.d_y)); }

// Host frames as device frames on the null stream; `up` owns the blocks.
int chain_upload_frames(const stitch_frame_u8* frames, int nf, std::vector<DevBuf>* up, std::vector<stitch_frame_u8>* dev) {
    up->resize((size_t)nf);
    dev->resize((size_t)nf);
    for (int f = 0; f < nf; ++f) {
        const size_t bytes = (size_t)3 * frames[f].width * frames[f].height;
        int rc = (*up)[f].alloc(bytes);
        if (rc) return rc;
        H2D((*up)[f].p, frames[f].data, bytes);
        (*dev)[f] = stitch_frame_u8{(*up)[f].as<uint8_t>(), frames[f].width, frames[f].height};
    }
    return STITCH_OK;
}

// ---- the SIFT front end: frames in, ordered feature sets out, descriptors and key points never leave the device -------------
// Phase A's result, which phase B works from.  `index` is read by its upload in phase B, so the wait is declared behind it and
// runs before the vector goes.  Two phases, because a caller may need `kept` to decide where the ordered rows go.
struct SiftOrder {
    std::vector<stitch_sift_desc> sd;
    std::vector<int32_t> heads;  // per frame {counts[2], status[4], -, -}
    std::vector<size_t> row0;    // frame f's part of the index array starts at row0[f]
    std::vector<int> kept;       // rows of frame f in the map order
    std::vector<void*> blocks;   // what chain_gather releases behind its launches; a caller may list blocks of its own first
    std::vector<int32_t> index;  // the map order: per frame its output rows' input rows
    int32_t* d_index = nullptr;
    PanoWait index_in_use{nullptr, false};
};

// Phase A: projection + gray per frame and one SIFT call over all of them; read-back 1 (the heads, then the descriptor rows
// written); the std::map order on the host.  colour_dst(f, &p) says where frame f's projected colours go (it may take the block,
// and may name the same one for every frame); name(f) names frame f in the capacity error.
template <typename ColourDst, typename FrameName>
int chain_sift_order(const stitch_frame_u8* frames, int n, const stitch_panorama_opts& o, int feat_cap, ColourDst colour_dst, FrameName name, PanoArena& A,
                     hipStream_t s, SiftOrder* S) {
    int rc = STITCH_OK;
    const size_t kc = (size_t)std::max(o.kp_cap, 1), fc = (size_t)std::max(feat_cap, 1);
    int32_t* d_heads = nullptr;
    if ((rc = A.take(&d_heads, sizeof(int32_t) * 8 * n))) return rc;
    S->sd.resize((size_t)n);
    for (int f = 0; f < n; ++f) {
        const int w = frames[f].width, h = frames[f].height;
        uint8_t *proj = nullptr, *gray = nullptr;
        stitch_sift_desc& d = S->sd[f];
        std::memset(&d, 0, sizeof d);
        if ((rc = colour_dst(f, &proj)) || (rc = A.take(&gray, (size_t)w * h)) || (rc = A.take(&d.keypoints, kc * sizeof(StitchSiftKeypoint))) ||
            (rc = A.take(&d.feat_kp, fc * sizeof(int32_t))) || (rc = A.take(&d.feat_angle, fc * sizeof(double))) ||
            (rc = A.take(&d.feat_desc, fc * STITCH_DESCRIPTOR_DIM * sizeof(float))))
            return rc;
        for (void* p : {(void*)gray, (void*)d.keypoints, (void*)d.feat_kp, (void*)d.feat_angle, (void*)d.feat_desc}) S->blocks.push_back(p);
        if ((rc = stitch_dev_project_gray_u8(frames[f].data, w, h, o.fov_deg, proj, gray, nullptr, s))) return rc;
        d.image = gray;
        d.width = w;
        d.height = h;
        d.pitch = w;
        d.is_f32 = 0;
        d.kp_cap = o.kp_cap;
        d.feat_cap = feat_cap;
        d.counts = d_heads + 8 * f;
        d.status = d_heads + 8 * f + 2;
    }
    if ((rc = stitch_dev_sift_many(S->sd.data(), n, o.sift, s))) return rc;
    S->heads.resize((size_t)8 * n);
    HIPCHK(hipMemcpyAsync(S->heads.data(), d_heads, sizeof(int32_t) * 8 * n, hipMemcpyDeviceToHost, s));
    if ((rc = pano_sync(s))) return rc;
    S->row0.assign((size_t)n + 1, 0);
    for (int f = 0; f < n; ++f) {
        const int32_t* hd = &S->heads[(size_t)8 * f];
        if (hd[2] != STITCH_SIFT_OK)
            return fail(STITCH_ERR_CAPACITY, "%s: SIFT capacities too small (%d keypoints, %d features found)", name(f).c_str(), hd[3], hd[4]);
        S->row0[f + 1] = S->row0[f] + (size_t)hd[1];
    }
    const std::vector<size_t>& row0 = S->row0;
    std::vector<float> rows(row0[n] * STITCH_DESCRIPTOR_DIM);
    for (int f = 0; f < n; ++f) {
        const size_t cnt = row0[f + 1] - row0[f];
        if (cnt)
            HIPCHK(hipMemcpyAsync(rows.data() + row0[f] * STITCH_DESCRIPTOR_DIM, S->sd[f].feat_desc, cnt * STITCH_DESCRIPTOR_DIM * sizeof(float), hipMemcpyDeviceToHost, s));
    }
    if ((rc = pano_sync(s))) return rc;
    // the map order on the host
    S->index.resize(std::max<size_t>(row0[n], 1));
    S->kept.assign((size_t)n, 0);
    for (int f = 0; f < n; ++f)
        if ((rc = stitch_feature_order(rows.data() + row0[f] * STITCH_DESCRIPTOR_DIM, (int)(row0[f + 1] - row0[f]), S->index.data() + row0[f], &S->kept[f]))) return rc;
    return STITCH_OK;
}

// Phase B: only the index arrays go back up, in one copy, and k_feat_gather builds the ordered sets, PANO_MAXFRAMES frames per
// launch.  place(f, &desc, &x, &y) says where frame f's S.kept[f] rows go (it may take the blocks; nothing for a frame without
// a row); feats[f] receives them.  The SIFT blocks go in stream order behind the launches.
template <typename Place>
int chain_gather(SiftOrder& S, int n, Place place, stitch_feature_set* feats, PanoArena& A, hipStream_t s) {
    int rc = STITCH_OK;
    if ((rc = A.take(&S.d_index, sizeof(int32_t) * S.index.size()))) return rc;
    S.index_in_use.s = s;
    S.index_in_use.armed = true;
    HIPCHK(hipMemcpyAsync(S.d_index, S.index.data(), sizeof(int32_t) * S.index.size(), hipMemcpyHostToDevice, s));
    for (int f0 = 0; f0 < n; f0 += PANO_MAXFRAMES) {
        const int m = std::min(PANO_MAXFRAMES, n - f0);
        FeatGatherArgs ga;
        std::memset(&ga, 0, sizeof ga);
        int max_rows = 0;
        for (int j = 0; j < m; ++j) {
            const int f = f0 + j;
            FeatGatherFrame& g = ga.f[j];
            if ((rc = place(f, &g.out_desc, &g.out_x, &g.out_y))) return rc;
            feats[f] = stitch_feature_set{g.out_desc, g.out_x, g.out_y, S.kept[f]};
            g.desc = S.sd[f].feat_desc;
            g.fkp = S.sd[f].feat_kp;
            g.kp = reinterpret_cast<const SiftKeypoint*>(S.sd[f].keypoints);
            g.index = S.d_index + S.row0[f];
            g.n = S.kept[f];
            g.n_rows = S.heads[(size_t)8 * f + 1];
            g.n_kp = S.heads[(size_t)8 * f];
            max_rows = std::max(max_rows, S.kept[f]);
        }
        if (max_rows) {
            k_feat_gather<<<dim3((unsigned)((max_rows + PANO_GATHER_T / WAVE - 1) / (PANO_GATHER_T / WAVE)), (unsigned)m), PANO_GATHER_T, 0, s>>>(ga);
            if ((rc = launch_check("k_feat_gather"))) return rc;
        }
    }
    for (void* p : S.blocks) A.release(p);
    return STITCH_OK;
}

// ---- all ordered pairs of every capture in one matcher call; the lists stay on the device ----------------------------------
struct PairLists {
    int n = 0;
    int32_t* d_counts = nullptr;  // n_sets matrices of n x n, then the extra ones
    size_t count_bytes = 0;
    char* d_lists = nullptr;
    std::vector<size_t> off;
    int32_t* list_of(int k, int i, int j) const { return reinterpret_cast<int32_t*>(d_lists + off[((size_t)k * n + i) * n + j]); }
    int32_t* count_of(int k, int i, int j) const { return d_counts + ((size_t)k * n + i) * n + j; }
};

// feats: n_sets * n sets, capture-major (only d_desc and n are read).  The counts are zeroed, `extra` matrices included.
int chain_match_all(const stitch_feature_set* feats, int n_sets, int n, double ratio, int extra, PanoArena& A, hipStream_t s, PairLists* L) {
    int rc = STITCH_OK;
    L->n = n;
    L->count_bytes = sizeof(int32_t) * (size_t)(n_sets + extra) * n * n;
    if ((rc = A.take(&L->d_counts, L->count_bytes))) return rc;
    HIPCHK(hipMemsetAsync(L->d_counts, 0, L->count_bytes, s));
    L->off.assign((size_t)n_sets * n * n, 0);
    size_t total = 0;
    for (int k = 0; k < n_sets; ++k)
        for (int i = 0; i < n; ++i)
            for (int j = 0; j < n; ++j)
                if (i != j) {
                    L->off[((size_t)k * n + i) * n + j] = total;
                    total += align256(sizeof(int32_t) * 2 * std::max(feats[(size_t)k * n + j].n, 1));
                }
    if ((rc = A.take(&L->d_lists, total))) return rc;
    std::vector<stitch_match_desc> md;
    for (int k = 0; k < n_sets; ++k)
        for (int i = 0; i < n; ++i)
            for (int j = 0; j < n; ++j) {
                const stitch_feature_set &a = feats[(size_t)k * n + i], &b = feats[(size_t)k * n + j];
                if (i != j) md.push_back(stitch_match_desc{a.d_desc, b.d_desc, a.n, b.n, nullptr, nullptr, L->list_of(k, i, j), L->count_of(k, i, j)});
            }
    return stitch_dev_match_l1_ratio_many(md.data(), (int)md.size(), ratio, s);
}

// ---- a step: the two estimations over the selected list, and the device block they and the selection write -----------------
// The one place that knows the block's layout: p_fwd, p_bwd and info as a stitch_panorama_step holds them, the selected count and
// a pad; what a chain keeps behind that (`behind`) is its own.
struct StepBlock {
    static constexpr size_t kMaps = sizeof(stitch_panorama_step::p_fwd) + sizeof(stitch_panorama_step::p_bwd);
    static constexpr size_t kBack = kMaps + sizeof(stitch_panorama_step::info);  // what a step reads back
    static constexpr size_t kHead = kBack + 2 * sizeof(int32_t);
    char* d = nullptr;
    double* p16() const { return reinterpret_cast<double*>(d); }
    int32_t* info10() const { return reinterpret_cast<int32_t*>(d + kMaps); }
    int32_t* sel_count() const { return reinterpret_cast<int32_t*>(d + kBack); }
    int32_t* behind() const { return reinterpret_cast<int32_t*>(d + kHead); }
};

// Both estimations of a step over the list d_sel (capacity cap, *d_sel_count pairs): forward (the mirrored list) first.
int chain_step_fit(const float* src_x, const float* src_y, const float* dst_x, const float* dst_y, const int32_t* d_sel, const int32_t* d_sel_count, int cap,
                   const stitch_ransac_opts* ransac, double* d_p16, int32_t* d_info10, int32_t* d_inliers, hipStream_t s) {
    stitch_ransac_desc r[2];
    std::memset(r, 0, sizeof r);
    // a frame without features has no coordinate arrays: its lists are empty, the estimation never reads a point, and the
    // descriptor only needs an address
    const float* none = reinterpret_cast<const float*>(d_sel);
    for (int k = 0; k < 2; ++k) {
        r[k].src_x = src_x ? src_x : none;
        r[k].src_y = src_y ? src_y : none;
        r[k].dst_x = dst_x ? dst_x : none;
        r[k].dst_y = dst_y ? dst_y : none;
        r[k].pairs = d_sel;
        r[k].count = d_sel_count;
        r[k].n_max = cap;
        r[k].mirror = k == 0;
        r[k].p = d_p16 + 8 * k;
        r[k].info = d_info10 + STITCH_RANSAC_INFO * k;
    }
    r[0].inliers = d_inliers;  // of the forward map, or NULL
    return stitch_dev_ransac_many(r, 2, ransac, s);
}

// Read-back 3: the first `bytes` of the block (StepBlock::kBack at least) into `got`, decoded into *st; *ok = both maps are OK.
int chain_step_read(const StepBlock& B, size_t bytes, int src, int dst, hipStream_t s, unsigned char* got, stitch_panorama_step* st, bool* ok) {
    HIPCHK(hipMemcpyAsync(got, B.d, bytes, hipMemcpyDeviceToHost, s));
    int rc = pano_sync(s);
    if (rc) return rc;
    std::memset(st, 0, sizeof *st);
    st->src = src;
    st->dst = dst;
    std::memcpy(st->p_fwd, got, sizeof st->p_fwd);
    std::memcpy(st->p_bwd, got + sizeof st->p_fwd, sizeof st->p_bwd);
    std::memcpy(st->info, got + StepBlock::kMaps, sizeof st->info);
    *ok = st->info[0][0] == STITCH_RANSAC_OK && st->info[1][0] == STITCH_RANSAC_OK;
    return STITCH_OK;
}

}  // namespace
