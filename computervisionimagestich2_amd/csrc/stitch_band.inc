// stitch_band.inc -- ONE pair split into row bands over the GPUs of a node (BASELINE.json configs[4]: a 16384 x 16384 pair
// over 8 GPUs; SURVEY.md 8(e), option (ii)).  Included at the end of stitch_hip.hip (one translation unit: the kernels of
// stitch_kernels.hpp are used as they are).
//
// Rank r of N owns rows [r*h_l/N, (r+1)*h_l/N) of every SPLIT level l < Ls of the blend's pyramids (a contiguous row band,
// even row counts, so that the 2:1 decimation never straddles two ranks); the levels from Ls up are small and are
// replicated: every rank gathers level Ls and runs them through an ordinary plan.  What crosses ranks (the caller moves
// it: torch.distributed in pipeline.BandStitcher -- RCCL send/recv over xGMI on the GPUs, gloo in the CPU-staged test):
//   * causal y sweep of level l (CImg.h:34887-34932 along columns): three doubles per column and plane from the rank
//     above (k_vv_y_fwd `resume`), all seven planes in one launch and one message (a band's sweep is a chain of dependent
//     rows, as long for one plane as for seven: handing planes over one by one only adds stages to the chain of ranks);
//   * anticausal y sweep (+ fused decimation): the same from the rank below (k_vv_y_bwd_dec `resume`); the Triggs boundary
//     is taken by the last rank alone;
//   * level Ls: an all-gather of the bands (7 planes);
//   * collapse of level l: HALO rows of G_{l+1} (a, b) and E_{l+1} from either neighbour (the linear EXPAND reads source
//     rows iy, iy+1 with iy ~ y/2 - 1 .. y/2; CImg.h:29618-29690).
// The x sweeps, S1 (compose), the mask, the decimation and the collapse itself are local to a band.  The seam scan needs the
// canvas's middle row only and reads it straight from the input frames, which every rank holds, so every rank derives the
// same seam without communication.  Arithmetic: the kernels of the single-GPU path, sample for sample; the unfused
// sweeps are used (the fused band pipeline of k_vv_xbyf is the in-GPU form of the same hand-off).
// What a band holds and what every entry point launches is decided in stitch_call_form.h (BandShape, band_form); here are argument
// checks, the state of the zero-tile flags, and the kernels' arguments.
struct stitch_band : BandShape {
    int device = 0;
    stitch_blend_opts opts{};
    VVK vvk{};
    void* arena = nullptr;
    size_t arena_bytes = 0;
    float* T = nullptr;         // blur scratch, level-0 layout
    double* state_x = nullptr;  // [4][lines] of the x sweeps
    SeamDev *d_seam = nullptr, *h_seam = nullptr;
    stitch_plan* top = nullptr;  // ordinary plan of levels Ls.. (canvas = level Ls), level 0 handed in as planes
    float* gtop = nullptr;       // level Ls, all rows: 7 dense planes
    float* etop = nullptr;       // E of level Ls, all rows: 3 dense planes
    // the fused anticausal-x + causal-y sweep inside a band (stitch_band_reduce_xy_fwd): hand-off granules of the largest level,
    // band-queue head + abort word, the sticky count of timed-out waits and its host mirror
    u64* wf_yg = nullptr;
    unsigned* wf_ctrl = nullptr;  // [0]: queue head, [16]: abort, [32]: sticky
    unsigned* h_wf_sticky = nullptr;
    unsigned wf_sticky_seen = 0;
    bool wf_used = false;  // stitch_band_reduce_xy_fwd has run: status reads the sticky count back
    // Source-fused level 0 (as in a plan: the six level-0 planes and the mask plane are never stored).  compose leaves the index
    // plane of the warped frame in the slot of plane 0 (rows from the first halo row), the causal x sweep and the level-0 collapse
    // gather from the frames; the mosaic is a pure shift, so the band's first canvas row is folded into its row offset: pa?x counts
    // rows from the buffer's first halo row (x sweeps), pa?c from the band's first row (collapse).
    bool src_l0_next = true;  // stitch_band_set_level0's value: it reaches the shape with the next compose
    int px = 0;  // sizeof the pixel type of the last compose (1 / 4)
    PairArgs<uint8_t> pa8x{}, pa8c{};
    PairArgs<float> pafx{}, pafc{};
    float* mask_side = nullptr;  // [pitch]: the x-blurred row of the implicit level-0 mask
    uint8_t *zt = nullptr, *zi = nullptr;  // zero-tile flags of level 0: [7][NC][NR] of T, [NC][NR] of the index plane (see ZeroTiles)
    int zt_level = -1;  // the level whose fused reduce left flags for its anticausal sweep (-1: none): band_zt_after
    hipStream_t last_stream = nullptr;
    bool pending = false;
};
namespace {
template <typename PX>
PairArgs<PX>& band_pa(stitch_band* b, bool collapse);
template <>
PairArgs<uint8_t>& band_pa<uint8_t>(stitch_band* b, bool collapse) { return collapse ? b->pa8c : b->pa8x; }
template <>
PairArgs<float>& band_pa<float>(stitch_band* b, bool collapse) { return collapse ? b->pafc : b->pafx; }
// a flag record of the level where the form has flags, an empty one otherwise (one buffer, sized for level 0)
ZeroTiles band_tiles(const stitch_band* b, bool on, uint8_t* flags, int level, const BandForm& f) {
    return on ? ZeroTiles{flags, b->lv[level].rows, f.NR, f.NC} : ZeroTiles{};
}
MaskL0 band_mask(const stitch_band* b) { return MaskL0{b->d_seam, b->mask_side, b->lv[0].ph(), 1}; }
// (the defaults as they are: a plan's STITCH_XBYF_SPIN_LIMIT / STITCH_XBYF_EARLY and stitch_plan_set_handoff_spin_limit do not reach a band)
Handoff band_handoff(const stitch_band* b) { return Handoff{b->wf_yg, b->wf_ctrl, b->wf_ctrl + 16, b->wf_ctrl + 32, WF_SPIN_LIMIT, 1}; }

int band_check(stitch_band* b, int level, int max_level) {
    if (!b) return fail(STITCH_ERR_ARG, "null band");
    if (level < 0 || level > max_level) return fail(STITCH_ERR_ARG, "band: level %d outside 0..%d", level, max_level);
    int dev = -1;
    HIPCHK(hipGetDevice(&dev));
    if (dev != b->device) return fail(STITCH_ERR_ARG, "band belongs to device %d, current device is %d", b->device, dev);
    return STITCH_OK;
}

template <typename PX>
int band_compose(stitch_band* b, const PX* d_frame, int fw, int fh, const double pm[8], float offx, float offy, const PX* d_mosaic, int mw,
                 int mh, int ox, int oy, void* stream) {
    int rc = band_check(b, 0, 0);
    if (rc) return rc;
    if (!d_frame || !d_mosaic || !pm || fw <= 0 || fh <= 0 || mw <= 0 || mh <= 0) return fail(STITCH_ERR_ARG, "band_compose: bad argument");
    hipStream_t s = as_stream(stream);
    PairArgs<PX> pa{};
    pa.frame[0] = d_frame, pa.mosaic[0] = d_mosaic;
    std::memcpy(pa.map[0].p, pm, sizeof pa.map[0].p);
    pa.fw[0] = fw, pa.fh[0] = fh, pa.mw[0] = mw, pa.mh[0] = mh, pa.ox[0] = ox, pa.oy[0] = oy, pa.offx[0] = offx, pa.offy[0] = offy;
    set_index_owners(pa, 1, nullptr);  // a band computes its plane on every compose
    const BandLevel& a = b->lv[0];
    b->px = (int)sizeof(PX);
    band_set_src_l0(*b, b->src_l0_next);
    const BandForm f = band_form(*b, BO_COMPOSE, 0);
    if (f.src0) {
        if ((unsigned long long)fw * fh * sizeof(PX) >= 0xfffffff0ULL || (unsigned long long)mw * mh * sizeof(PX) >= 0xfffffff0ULL)
            return fail(STITCH_ERR_ARG, "band_compose: a channel plane of the inputs must stay below 4 GB for the source-fused level 0");
        const int ph = a.ph(), ybase = a.row0 - a.halo;
        PairArgs<PX>& px = band_pa<PX>(b, false);
        PairArgs<PX>& pc = band_pa<PX>(b, true);
        px = pa, pc = pa;
        px.oy[0] = oy + ybase, pc.oy[0] = oy + a.row0;
        // the index plane of the band's rows and its halo rows (a halo row outside the canvas maps wherever the map says: it is
        // swept along x like every halo row and never read)
        const ZeroTiles zi = band_tiles(b, f.zi, b->zi, 0, f);  // tiles of the index plane that lie outside the frame altogether
        if (zi.flags) k_fill_bytes<<<64, 256, 0, s>>>(zi.flags, (size_t)zi.NR * zi.NC, (uint8_t)1);
        k_src_index<PX><<<grid_xy(a.pitch, (ph + SI_ROWS - 1) / SI_ROWS, 1), 256, 0, s>>>(pa, a.g, a.w, ph, a.pitch, a.ps, zi, ybase);
        k_seam<PX><<<1, 256, 0, s>>>(nullptr, b->cw, b->ch, a.pitch, a.ps, b->opts.seam_rule, b->d_seam, pa, 1);
    } else {
        // S1 for this band's rows (canvas rows row0 ..): warp + move + value cast into the level-0 planes
        k_compose<PX><<<grid_xy(a.pitch, a.rows, 1), 256, 0, s>>>(pa, a.origin_g(), a.w, a.rows, a.pitch, a.ps, a.row0);
        // B1: the seam scan reads the canvas's middle row from the frames themselves (every rank: same inputs, same seam)
        k_seam<PX><<<1, 256, 0, s>>>(nullptr, b->cw, b->ch, a.pitch, a.ps, b->opts.seam_rule, b->d_seam, pa, 1);
        k_mask<<<grid_xy(a.pitch, a.rows, 1), 256, 0, s>>>(a.origin_g(), a.w, a.pitch, a.ps, b->d_seam);
    }
    HIPCHK(hipMemcpyAsync(b->h_seam, b->d_seam, sizeof(SeamDev), hipMemcpyDeviceToHost, s));
    b->last_stream = s, b->pending = true;
    return launch_check("band_compose");
}

template <typename OUT>
int band_collapse(stitch_band* b, int level, OUT* d_out, void* stream) {
    int rc = band_check(b, level, b->Ls - 1);
    if (rc) return rc;
    if (level == 0 && !d_out) return fail(STITCH_ERR_ARG, "band_collapse: level 0 needs the output band");
    hipStream_t s = as_stream(stream);
    const BandForm f = band_form(*b, BO_COLLAPSE, level);
    const BandLevel& a = b->lv[level];
    const BandLevel& nx = b->lv[level + 1];
    const float* gn = f.top_src ? b->gtop : nx.g;
    const float* en = f.top_src ? b->etop : nx.e;
    const int spitch = f.top_src ? nx.w : nx.pitch;
    const size_t sps = f.top_src ? (size_t)nx.w * nx.h_full : nx.ps;
    const CollapseKind kind{false, false, false, false, true};  // no lockstep, no block order, none of the plan's flags
    if (level == 0) {
        OutPtrs<OUT> outs{};
        outs.p[0] = d_out;
        if (b->src_l0 && b->px != (int)sizeof(OUT)) return fail(STITCH_ERR_ARG, "band_collapse: the output's pixel type differs from the composed inputs'");
        CollapseArgs<OUT, true> A{a.origin_g(), a.w, a.rows, a.pitch, a.ps, gn, en, nx.w, a.sh_eff, spitch, sps, {a.ix, a.ax, a.iy, a.ay}, outs,
                                  a.w, (size_t)a.w * a.rows, b->d_seam, b->src_l0 ? band_pa<OUT>(b, true) : PairArgs<OUT>{}, b->src_l0 ? 1 : 0, f.crows, f.xa, f.xb,
                                  1};  // u8_words: the aligned case only (the launcher's clamp)
        launch_collapse(A, kind, f.cols, f.strips, 1, MaskRowsArg{}, s);
    } else {
        OutPtrs<float> eo{};
        eo.p[0] = a.origin_e();
        CollapseArgs<float, false> A{a.origin_g(), a.w, a.rows, a.pitch, a.ps, gn, en, nx.w, a.sh_eff, spitch, sps, {a.ix, a.ax, a.iy, a.ay}, eo,
                                     a.pitch, a.ps, nullptr, NoPairArgs{}, 0, f.crows, f.xa, f.xb, 1};
        launch_collapse(A, kind, f.cols, f.strips, 1, MaskRowsArg{}, s);
    }
    b->last_stream = s, b->pending = true;
    return launch_check("band_collapse");
}

// The x sweeps of a level from its record: the causal one (at a source-fused level 0: frame channels through the index plane, the mosaic
// as a shift, the mask generated) and, bwd, the anticausal one behind it
int band_x_sweeps(stitch_band* b, int level, const BandForm& f, bool bwd, hipStream_t s) {
    const BandLevel& a = b->lv[level];
    const long lines = 7L * a.ph();
    const Bands bd = f.per_plane ? Bands{f.bands_nr, f.bands_h} : Bands{};
    const ZeroTiles zt = band_tiles(b, f.zt, b->zt, level, f), zi = band_tiles(b, f.zi, b->zi, level, f);
    const MaskL0 mk = f.src0 ? band_mask(b) : MaskL0{};
    if (f.src0 && b->px != 1 && b->px != 4) return fail(STITCH_ERR_ARG, "band: reduce before compose");
    if (f.src0 && b->px == 1)
        k_vv_x_fwd<uint8_t, true><<<f.nbx, 64, 0, s>>>(a.g, b->T, a.w, a.pitch, lines, b->vvk, b->state_x, mk, b->pa8x, zt, zi, nullptr, bd);
    else if (f.src0)
        k_vv_x_fwd<float, true><<<f.nbx, 64, 0, s>>>(a.g, b->T, a.w, a.pitch, lines, b->vvk, b->state_x, mk, b->pafx, zt, zi, nullptr, bd);
    else
        k_vv_x_fwd<float, false><<<f.nbx, 64, 0, s>>>(a.g, b->T, a.w, a.pitch, lines, b->vvk, b->state_x, mk, NoPairArgs{}, zt, ZeroTiles{}, nullptr, bd);
    if (bwd) k_vv_x_bwd<<<f.nbx, 64, 0, s>>>(b->T, a.w, a.pitch, lines, b->vvk, b->state_x, mk, bd);
    b->zt_level = f.zt_after;
    return STITCH_OK;
}

// The two y sweeps of a level, whole (x0 = 0, cols = the pitch) or over a column range
int band_y_fwd(stitch_band* b, int level, const BandForm& f, int plane, int x0, int cols, const double* d_resume, double* d_state_out, hipStream_t s) {
    const BandLevel& a = b->lv[level];
    float* t = b->T + (size_t)(plane < 0 ? 0 : plane) * a.ps + (size_t)a.halo * a.pitch;
    // source-fused level 0: the mask plane's input is one x-blurred row for every y (MaskL0::side), shifted to the band's first row
    const MaskL0 mk = f.src0 ? band_mask(b) : MaskL0{};
    const dim3 g((cols + YCOLS - 1) / YCOLS, f.np);
    if (f.xch)
        k_vv_y_fwd<true><<<g, 64, 0, s>>>(t, a.rows, a.pitch, a.ps, b->vvk, d_state_out, mk, d_resume, x0);
    else
        k_vv_y_fwd<<<g, 64, 0, s>>>(t, a.rows, a.pitch, a.ps, b->vvk, d_state_out, mk, d_resume);
    b->last_stream = s, b->pending = true;
    return STITCH_OK;
}
int band_y_bwd(stitch_band* b, int level, const BandForm& f, int plane, int x0, int cols, const double* d_fwd_state, const double* d_resume, double* d_state_out,
               hipStream_t s) {
    const BandLevel& a = b->lv[level];
    const BandLevel& d = b->lv[level + 1];
    float* t = b->T + (size_t)(plane < 0 ? 0 : plane) * a.ps + (size_t)a.halo * a.pitch;
    float* dst = d.origin_g() + (size_t)(plane < 0 ? 0 : plane) * d.ps;
    if (f.y_bwd == YB_DEC)  // (rowz: a chunk of rows may straddle two bands of tiles, per-row flag look-up)
        launch_y_bwd_dec(f.dec, f.np, s, DecPlanes{t, a.w, a.rows, a.pitch, a.ps, a.h_full}, DecPlanes{dst, d.w, d.rows, d.pitch, d.ps, d.h_full}, b->vvk, d_fwd_state,
                         band_tiles(b, f.zt, b->zt, level, f), d_resume, d_state_out, x0, cols, 0, ZeroTiles{}, ZeroTiles{});
    else {
        k_vv_y_bwd<<<dim3((cols + YCOLS - 1) / YCOLS, f.np), 64, 0, s>>>(t, a.rows, a.pitch, a.ps, b->vvk, d_fwd_state, d_resume, d_state_out);
        k_decimate<<<grid_xy(d.pitch, d.rows, f.np), 256, 0, s>>>(t, a.w, a.h_full, a.pitch, a.ps, dst, d.w, d.h_full, d.pitch, d.ps, d.row0, a.row0);
    }
    b->last_stream = s, b->pending = true;
    return STITCH_OK;
}
// columns [x0, x1) of a y sweep over a column range: multiples of YCOLS, x1 possibly the pitch
bool band_cols_ok(const BandLevel& a, int x0, int x1) { return x0 >= 0 && x1 > x0 && x0 % YCOLS == 0 && (x1 % YCOLS == 0 || x1 == a.pitch) && x1 <= a.pitch; }
}  // namespace

extern "C" {

int stitch_band_create(int cw, int ch, int rank, int nranks, int split_levels, const stitch_blend_opts* opts, stitch_band** out) {
    if (!out) return fail(STITCH_ERR_ARG, "band_create: null output");
    *out = nullptr;
    int rc = need_device();
    if (rc) return rc;
    stitch_blend_opts o;
    stitch_blend_opts_default(&o);
    if (opts) o = *opts;
    if (o.blur_kind != 0 || o.level_rule != 0 || o.seam_rule != 0 || !(o.sigma >= 0.5f))
        return fail(STITCH_ERR_ARG, "band_create: the band split implements the root variant (Van Vliet blur, sigma >= 0.5)");
    stitch_band* b = new stitch_band();
    // the band's switches, read ONCE here with the plan's semantics (Tuning::env_int: set and > 0; "=0" means off, as for a plan):
    // STITCH_BAND_PLANES=1: materialised level-0 planes and mask (rounds 1-2); STITCH_BAND_PLAIN=1: the two-kernel decimation (A/B)
    BandWhy y;
    const BandRefusal no = band_shape(*b, cw, ch, rank, nranks, split_levels, !(Tuning::env_int("STITCH_NO_ZERO_TILES") > 0), !(Tuning::env_int("STITCH_BAND_PLANES") > 0),
                                      Tuning::env_int("STITCH_BAND_PLAIN") > 0, &y);
    if (no != BAND_OK) delete b;
    switch (no) {
    case BAND_OK: break;
    case BAND_BAD_RANK: return fail(STITCH_ERR_ARG, "band_create: rank %d of %d", rank, nranks);
    case BAND_BAD_PYRAMID: return pyramid_levels(cw, ch, 0, nullptr, nullptr);
    case BAND_BAD_SPLIT: return fail(STITCH_ERR_ARG, "band_create: split_levels must be 1..%d for a %d-level pyramid", y.level - 1, y.level);
    case BAND_BAD_ROWS:
        return fail(STITCH_ERR_ARG, "band_create: level %d has %d rows, not divisible into %d bands of even height >= %d", y.level, y.row, nranks, 2 * BAND_HALO);
    case BAND_BAD_WIDTH: return fail(STITCH_ERR_ARG, "band_create: level %d is %d columns wide", y.level, y.src_a);
    case BAND_BAD_HALO:
        return fail(STITCH_ERR_ARG, "band_create: level %d row %d needs source row %d..%d, outside the band's halo", y.level, y.row, y.src_a, y.src_b);
    }
    const int Ls = b->Ls;
    b->opts = o, b->src_l0_next = b->src_l0;
    b->vvk = make_vvk(o.sigma);
    if (hipGetDevice(&b->device) != hipSuccess) {
        delete b;
        return fail(STITCH_ERR_HIP, "hipGetDevice failed");
    }
    size_t off = 0;
    auto take = [&](size_t bytes) {
        const size_t o2 = off;
        off += align256(bytes);
        return o2;
    };
    size_t g_off[32], e_off[32], ix_off[32], ax_off[32], iy_off[32], ay_off[32];
    for (int l = 0; l <= Ls; ++l) {
        const BandLevel& v = b->lv[l];
        g_off[l] = take(sizeof(float) * (v.ps * 7 + (size_t)v.pitch * 64));  // + slack rows for the x sweeps' last partial block
        e_off[l] = (l >= 1 && l < Ls) ? take(sizeof(float) * v.ps * 3) : 0;
        if (l < Ls) {
            ix_off[l] = take(sizeof(int32_t) * v.w);
            ax_off[l] = take(sizeof(double) * v.w);
            iy_off[l] = take(sizeof(int32_t) * v.rows);
            ay_off[l] = take(sizeof(double) * v.rows);
        }
    }
    const BandLevel &v0 = b->lv[0], &vt = b->lv[Ls];
    const size_t t_off = take(sizeof(float) * (v0.ps * 7 + (size_t)v0.pitch * 64));
    const size_t st_off = take(sizeof(double) * 4 * 7 * (size_t)(v0.rows + 2 * BAND_HALO + 64));
    const size_t seam_off = take(sizeof(SeamDev));
    const size_t side_off = take(sizeof(float) * v0.pitch);
    const size_t ntile0 = (size_t)tiles(v0.rows) * tiles(v0.w);
    const size_t zt_off = take(7 * ntile0), zi_off = take(ntile0);
    const size_t yg_off = take(sizeof(u64) * (7 * (size_t)(v0.pitch / TS) * WF_GRAN * WAVE + 1));
    const size_t wfc_off = take(sizeof(unsigned) * 64);
    const size_t gtop_off = take(sizeof(float) * 7 * (size_t)vt.w * vt.h_full);
    const size_t etop_off = take(sizeof(float) * 3 * (size_t)vt.w * vt.h_full);
    b->arena_bytes = off;
    if (hipMalloc(&b->arena, off) != hipSuccess || hipMemset(b->arena, 0, off) != hipSuccess ||
        hipHostMalloc((void**)&b->h_seam, sizeof(SeamDev)) != hipSuccess || hipHostMalloc((void**)&b->h_wf_sticky, sizeof(unsigned)) != hipSuccess) {
        (void)hipGetLastError();
        stitch_band_destroy(b);
        return fail(STITCH_ERR_HIP, "band_create: allocation of %zu bytes failed", off);
    }
    std::memset(b->h_seam, 0, sizeof(SeamDev));
    *b->h_wf_sticky = 0;
    char* base = static_cast<char*>(b->arena);
    b->mask_side = reinterpret_cast<float*>(base + side_off);
    b->zt = reinterpret_cast<uint8_t*>(base + zt_off);
    b->zi = reinterpret_cast<uint8_t*>(base + zi_off);
    b->wf_yg = reinterpret_cast<u64*>(base + yg_off);
    b->wf_ctrl = reinterpret_cast<unsigned*>(base + wfc_off);
    b->T = reinterpret_cast<float*>(base + t_off);
    b->state_x = reinterpret_cast<double*>(base + st_off);
    b->d_seam = reinterpret_cast<SeamDev*>(base + seam_off);
    b->gtop = reinterpret_cast<float*>(base + gtop_off);
    b->etop = reinterpret_cast<float*>(base + etop_off);
    for (int l = 0; l <= Ls; ++l) {
        BandLevel& v = b->lv[l];
        v.g = reinterpret_cast<float*>(base + g_off[l]);
        v.e = (l >= 1 && l < Ls) ? reinterpret_cast<float*>(base + e_off[l]) : nullptr;
        if (l >= Ls) continue;
        v.ix = reinterpret_cast<int32_t*>(base + ix_off[l]);
        v.ax = reinterpret_cast<double*>(base + ax_off[l]);
        v.iy = reinterpret_cast<int32_t*>(base + iy_off[l]);
        v.ay = reinterpret_cast<double*>(base + ay_off[l]);
        std::vector<int32_t> idx;
        std::vector<double> al;
        expand_table(b->lv[l + 1].w, v.w, idx, al);
        bool ok = hipMemcpy(v.ix, idx.data(), sizeof(int32_t) * v.w, hipMemcpyHostToDevice) == hipSuccess &&
                  hipMemcpy(v.ax, al.data(), sizeof(double) * v.w, hipMemcpyHostToDevice) == hipSuccess;
        band_row_table(*b, l, idx, al);
        ok = ok && hipMemcpy(v.iy, idx.data(), sizeof(int32_t) * v.rows, hipMemcpyHostToDevice) == hipSuccess &&
             hipMemcpy(v.ay, al.data(), sizeof(double) * v.rows, hipMemcpyHostToDevice) == hipSuccess;
        if (!ok) {
            stitch_band_destroy(b);
            return fail(STITCH_ERR_HIP, "band_create: table upload failed");
        }
    }
    // the replicated levels: an ordinary single-pair plan whose level 0 is level Ls, handed in as planes
    if ((rc = plan_create(vt.w, vt.h_full, &o, 1, true, &b->top))) {
        stitch_band_destroy(b);
        return rc;
    }
    if (b->top->L != b->L - Ls) {
        stitch_band_destroy(b);
        return fail(STITCH_ERR_PYRAMID, "band_create: the coarse plan has %d levels, expected %d", b->top->L, b->L - Ls);
    }
    *out = b;
    return STITCH_OK;
}

void stitch_band_destroy(stitch_band* b) {
    if (!b) return;
    if (b->pending) (void)hipStreamSynchronize(b->last_stream);
    if (b->top) stitch_plan_destroy(b->top);
    if (b->arena) (void)hipFree(b->arena);
    if (b->h_seam) (void)hipHostFree(b->h_seam);
    if (b->h_wf_sticky) (void)hipHostFree(b->h_wf_sticky);
    delete b;
}

// Level 0 of this band source-fused (1: the default -- index plane + gathers, implicit mask) or materialised (0: k_compose's six
// planes and k_mask's seventh, what reduce_y_fwd / reduce_y_bwd of ONE plane at a time need).  Takes effect with the next compose.
int stitch_band_set_level0(stitch_band* b, int source_fused) {
    if (!b) return fail(STITCH_ERR_ARG, "null band");
    b->src_l0_next = source_fused != 0;
    return STITCH_OK;
}

int stitch_band_geometry(const stitch_band* b, int level, int out[6]) {
    if (!b || !out || level < 0 || level > b->Ls) return fail(STITCH_ERR_ARG, "band_geometry: bad argument");
    const BandLevel& v = b->lv[level];
    out[0] = v.w, out[1] = v.rows, out[2] = v.row0, out[3] = v.pitch, out[4] = v.h_full, out[5] = v.halo;
    return STITCH_OK;
}
int stitch_band_levels(const stitch_band* b, int* total_levels) {
    if (!b) return fail(STITCH_ERR_ARG, "null band");
    if (total_levels) *total_levels = b->L;
    return b->Ls;
}

int stitch_band_compose_u8(stitch_band* b, const uint8_t* d_frame, int fw, int fh, const double p[8], float offx, float offy,
                           const uint8_t* d_mosaic, int mw, int mh, int ox, int oy, void* stream) {
    return band_compose<uint8_t>(b, d_frame, fw, fh, p, offx, offy, d_mosaic, mw, mh, ox, oy, stream);
}
int stitch_band_compose_f32(stitch_band* b, const float* d_frame, int fw, int fh, const double p[8], float offx, float offy,
                            const float* d_mosaic, int mw, int mh, int ox, int oy, void* stream) {
    return band_compose<float>(b, d_frame, fw, fh, p, offx, offy, d_mosaic, mw, mh, ox, oy, stream);
}

int stitch_band_reduce_x(stitch_band* b, int level, void* stream) {
    int rc = band_check(b, level, b ? b->Ls - 1 : 0);
    if (rc) return rc;
    hipStream_t s = as_stream(stream);
    if ((rc = band_x_sweeps(b, level, band_form(*b, BO_X, level, b->zt_level), true, s))) return rc;  // (the separate sweeps leave no flags)
    b->last_stream = s, b->pending = true;
    return launch_check("band_reduce_x");
}

// reduce_x and reduce_y_fwd(plane -1) in two launches instead of three: the causal x sweep, then the anticausal x sweep fused
// with the causal y sweep (k_vv_xbyf: the level is read and written once instead of twice).  The fused sweep starts from
// `resume` ([3][7][pitch] from the rank above; NULL exactly on rank 0) and leaves `state_out` ([4][7][pitch]) as reduce_y_fwd
// does.  A rank's launch cannot start before the rank above has finished its own, as with the separate causal y sweep.
int stitch_band_reduce_xy_fwd(stitch_band* b, int level, const double* d_resume, double* d_state_out, void* stream) {
    int rc = band_check(b, level, b ? b->Ls - 1 : 0);
    if (rc) return rc;
    if (!d_state_out || (b->rank > 0) != (d_resume != nullptr))
        return fail(STITCH_ERR_ARG, "band_reduce_xy_fwd: a state buffer, and a resume state exactly on ranks > 0");
    hipStream_t s = as_stream(stream);
    const BandLevel& a = b->lv[level];
    const BandForm f = band_form(*b, BO_XY_FWD, level, b->zt_level);
    if ((rc = band_x_sweeps(b, level, f, false, s))) return rc;
    Wavefront wf = wavefront_of(band_handoff(b), 7, f.NR, f.NC, band_tiles(b, f.zt, b->zt, level, f), s);
    wf.mask_l0 = f.src0 ? 1 : 0;  // the mask plane's rows below its first band are the row that travels with the y state
    wf.ph = a.ph();
    wf.y0 = a.halo;
    wf.resume = d_resume;
    k_clear_words<<<1, 64, 0, s>>>((u64*)b->wf_ctrl, 16);  // queue head and abort word; the sticky count stays
    launch_xbyf<float>(f.wgs, s, false, false, false, f.banded, b->T, a.w, a.rows, a.pitch, b->vvk, b->state_x, 7L * a.ph(), d_state_out, wf, Recompute{}, PairArgs<float>{});
    b->last_stream = s, b->pending = true, b->wf_used = true;
    return launch_check("band_reduce_xy_fwd");
}

// Causal y sweep of one plane of this band (plane 0..6; states [k][pitch]) or of all seven in one launch (plane -1; states
// [k][7][pitch]).  resume: k = 3 doubles per column left by the rank above (NULL on rank 0: the sweep starts at the image's
// first row); state_out: k = 4 -- (v1, v2, v3) for the rank below, and the sample of the band's last row (the last rank's
// Triggs boundary input).
int stitch_band_reduce_y_fwd(stitch_band* b, int level, int plane, const double* d_resume, double* d_state_out, void* stream) {
    int rc = band_check(b, level, b ? b->Ls - 1 : 0);
    if (rc) return rc;
    if (plane < -1 || plane >= 7 || !d_state_out || (b->rank > 0) != (d_resume != nullptr))
        return fail(STITCH_ERR_ARG, "band_reduce_y_fwd: plane -1 (all) or 0..6, a state buffer, and a resume state exactly on ranks > 0");
    const BandForm f = band_form(*b, BO_Y_FWD, level, b->zt_level, plane);
    if (!f.admitted) return fail(STITCH_ERR_ARG, "band_reduce_y_fwd: one plane at a time needs the materialised level 0 (STITCH_BAND_PLANES=1)");
    band_y_fwd(b, level, f, plane, 0, b->lv[level].pitch, d_resume, d_state_out, as_stream(stream));
    return launch_check("band_reduce_y_fwd");
}

// Anticausal y sweep + decimation of one plane into this rank's band of level+1.  d_fwd_state: what reduce_y_fwd left for
// this plane (read on the last rank only: Triggs boundary, CImg.h:34911-34922); resume: [3][pitch] from the rank below
// (NULL on the last rank); state_out: [3][pitch] for the rank above.
int stitch_band_reduce_y_bwd(stitch_band* b, int level, int plane, const double* d_fwd_state, const double* d_resume, double* d_state_out,
                             void* stream) {
    int rc = band_check(b, level, b ? b->Ls - 1 : 0);
    if (rc) return rc;
    if (plane < -1 || plane >= 7 || !d_fwd_state || !d_state_out || (b->rank < b->nranks - 1) != (d_resume != nullptr))
        return fail(STITCH_ERR_ARG, "band_reduce_y_bwd: plane -1 (all) or 0..6, state buffers, and a resume state exactly on ranks below the last");
    band_y_bwd(b, level, band_form(*b, BO_Y_BWD, level, b->zt_level, plane), plane, 0, b->lv[level].pitch, d_fwd_state, d_resume, d_state_out, as_stream(stream));
    return launch_check("band_reduce_y_bwd");
}

// The same two sweeps over a COLUMN RANGE [x0, x1) of all seven planes (multiples of 128; x1 may be the pitch), with the chunk's own
// state arrays: resume [3][7][x1-x0], state_out [4][7][x1-x0] (causal) / [3][7][x1-x0] (anticausal), fwd_state = the chunk's causal
// state_out.  Columns are independent in a y sweep, so a rank can hand the state of a chunk on as soon as that chunk is swept and
// the ranks below work on earlier chunks meanwhile: the hand-off chain of a level is N + C - 1 chunk-sweeps long instead of N
// whole sweeps (SURVEY.md 8(e)(ii): "pipeline it over column chunks").  Even level widths only (the odd-width decimation overlaps
// workgroups by two columns).
int stitch_band_reduce_y_fwd_cols(stitch_band* b, int level, int x0, int x1, const double* d_resume, double* d_state_out, void* stream) {
    int rc = band_check(b, level, b ? b->Ls - 1 : 0);
    if (rc) return rc;
    const BandLevel& a = b->lv[level];
    if (!band_cols_ok(a, x0, x1) || !d_state_out || (b->rank > 0) != (d_resume != nullptr))
        return fail(STITCH_ERR_ARG, "band_reduce_y_fwd_cols: columns [%d, %d) must be multiples of %d inside the pitch %d, with a state buffer and a resume state exactly on ranks > 0", x0, x1, YCOLS, a.pitch);
    band_y_fwd(b, level, band_form(*b, BO_Y_FWD_COLS, level, b->zt_level), -1, x0, x1 - x0, d_resume, d_state_out, as_stream(stream));
    return launch_check("band_reduce_y_fwd_cols");
}
int stitch_band_reduce_y_bwd_cols(stitch_band* b, int level, int x0, int x1, const double* d_fwd_state, const double* d_resume, double* d_state_out,
                                  void* stream) {
    int rc = band_check(b, level, b ? b->Ls - 1 : 0);
    if (rc) return rc;
    const BandLevel& a = b->lv[level];
    if (!band_cols_ok(a, x0, x1) || !d_fwd_state || !d_state_out || (b->rank < b->nranks - 1) != (d_resume != nullptr))
        return fail(STITCH_ERR_ARG, "band_reduce_y_bwd_cols: columns [%d, %d) must be multiples of %d inside the pitch %d, with state buffers and a resume state exactly on ranks below the last", x0, x1, YCOLS, a.pitch);
    const BandForm f = band_form(*b, BO_Y_BWD_COLS, level, b->zt_level);
    if (!f.admitted) return fail(STITCH_ERR_ARG, "band_reduce_y_bwd_cols: even level widths and the fused decimation only (level %d is %d wide)", level, a.w);
    band_y_bwd(b, level, f, -1, x0, x1 - x0, d_fwd_state, d_resume, d_state_out, as_stream(stream));
    return launch_check("band_reduce_y_bwd_cols");
}

// Rows of this rank's band <-> a dense buffer [planes][nrows][w] (what the caller sends to / receives from its neighbours).
// kind 0: G a, b (6 planes); 1: E (3 planes); 2: G with the mask (7 planes).  first_row is band-local and may reach into the
// halo: -HALO .. rows + HALO - 1.  to_buffer != 0 packs, 0 unpacks.
int stitch_band_rows(stitch_band* b, int level, int kind, int first_row, int nrows, float* d_buf, int to_buffer, void* stream) {
    int rc = band_check(b, level, b ? b->Ls : 0);
    if (rc) return rc;
    const BandLevel& v = b->lv[level];
    const int planes = kind == 0 ? 6 : kind == 1 ? 3 : kind == 2 ? 7 : 0;
    if (!planes || !d_buf || nrows < 1 || first_row < -v.halo || first_row + nrows > v.rows + v.halo || (kind == 1 && !v.e))
        return fail(STITCH_ERR_ARG, "band_rows: bad argument (level %d kind %d rows %d..%d)", level, kind, first_row, first_row + nrows - 1);
    hipStream_t s = as_stream(stream);
    float* base = kind == 1 ? v.e : v.g;
    for (int q = 0; q < planes; ++q) {
        float* band_rows = base + (size_t)q * v.ps + (size_t)(v.halo + first_row) * v.pitch;
        float* buf_rows = d_buf + (size_t)q * nrows * v.w;
        if (to_buffer)
            HIPCHK(hipMemcpy2DAsync(buf_rows, sizeof(float) * v.w, band_rows, sizeof(float) * v.pitch, sizeof(float) * v.w, nrows, hipMemcpyDeviceToDevice, s));
        else
            HIPCHK(hipMemcpy2DAsync(band_rows, sizeof(float) * v.pitch, buf_rows, sizeof(float) * v.w, sizeof(float) * v.w, nrows, hipMemcpyDeviceToDevice, s));
    }
    b->last_stream = s, b->pending = true;
    return STITCH_OK;
}

// The replicated levels.  d_g7: level Ls, ALL rows, 7 dense planes [a0 a1 a2 b0 b1 b2 m][h][w] (the all-gather of the bands).
// Runs REDUCE and the collapse of levels Ls.. on this rank and keeps G_Ls and E_Ls for the collapse of level Ls-1.
int stitch_band_top(stitch_band* b, const float* d_g7, void* stream) {
    int rc = band_check(b, 0, 0);
    if (rc) return rc;
    if (!d_g7) return fail(STITCH_ERR_ARG, "band_top: null planes");
    hipStream_t s = as_stream(stream);
    stitch_plan* p = b->top;
    const Level& a = p->lv[0];
    const size_t n = (size_t)a.w * a.h;
    HIPCHK(hipMemcpyAsync(b->gtop, d_g7, sizeof(float) * 7 * n, hipMemcpyDeviceToDevice, s));
    for (int q = 0; q < 7; ++q)
        HIPCHK(hipMemcpy2DAsync(a.g + (size_t)q * a.ps, sizeof(float) * a.pitch, b->gtop + (size_t)q * n, sizeof(float) * a.w, sizeof(float) * a.w, a.h,
                                hipMemcpyDeviceToDevice, s));
    const PairArgs<float> none{};
    const CallForm c = p->last_form = call_form(*p, 1, false, false);
    if ((rc = run_reduce<float>(p, c, s, none, ZeroTiles{}))) return rc;
    OutPtrs<float> outs{};
    outs.p[0] = b->etop;
    if ((rc = run_collapse<float>(p, c, outs, s, none))) return rc;
    p->last_stream = s, p->pending = true, p->last_n = 1;
    b->last_stream = s, b->pending = true;
    return STITCH_OK;
}

int stitch_band_collapse_u8(stitch_band* b, int level, uint8_t* d_out_band, void* stream) { return band_collapse<uint8_t>(b, level, d_out_band, stream); }
int stitch_band_collapse_f32(stitch_band* b, int level, float* d_out_band, void* stream) { return band_collapse<float>(b, level, d_out_band, stream); }

// Waits for the band's last call and reports the seam outcome like stitch_plan_status (plus a timed-out fused sweep of the
// coarse plan).
int stitch_band_status(stitch_band* b, stitch_seam* seam_out) {
    if (!b) return fail(STITCH_ERR_ARG, "null band");
    if (b->pending) {
        // the count of timed-out waits of the band's own fused sweep comes back on the stream of the last call (no device-wide
        // synchronisation: other bands of the same device keep running)
        if (b->wf_used) HIPCHK(hipMemcpyAsync(b->h_wf_sticky, b->wf_ctrl + 32, sizeof(unsigned), hipMemcpyDeviceToHost, b->last_stream));
        HIPCHK(hipStreamSynchronize(b->last_stream));
        b->pending = false;
    }
    if (b->top->h_wf_abort && *b->top->h_wf_abort != b->top->wf_abort_seen)
        return fail(STITCH_ERR_HIP, "band: a hand-off wait of the coarse levels' fused sweep timed out (results are invalid)");
    if (*b->h_wf_sticky != b->wf_sticky_seen) {
        b->wf_sticky_seen = *b->h_wf_sticky;
        return fail(STITCH_ERR_HIP, "band: a hand-off wait of the band's fused sweep timed out (results are invalid)");
    }
    const SeamDev& sd = *b->h_seam;
    seam_to_public(sd, seam_out);
    if (sd.status == -2) return fail(STITCH_ERR_EMPTY_MIDROW, "blend: channel 0 of a's middle row is empty");
    if (sd.status == -3) return fail(STITCH_ERR_ZERO_OVERLAP, "blend: a and b do not overlap on the middle row");
    return STITCH_OK;
}

}  // extern "C"
