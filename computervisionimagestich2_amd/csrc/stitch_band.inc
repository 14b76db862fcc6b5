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
namespace {
constexpr int BAND_HALO = 2;

struct BandLevel {
    int w = 0, h_full = 0, rows = 0, row0 = 0, pitch = 0;
    int halo = 0;        // halo rows either side: BAND_HALO on levels >= 1 (sources of an EXPAND) of a band with neighbours, else none
    size_t ps = 0;       // plane stride in floats: pitch * (rows + 2 * halo)
    float* g = nullptr;  // 7 planes (base = first halo row); origin = g + halo * pitch
    float* e = nullptr;  // 3 planes, levels 1..Ls-1
    int32_t *ix = nullptr, *iy = nullptr;  // resize tables level+1 -> level, rows in band-local source coordinates
    double *ax = nullptr, *ay = nullptr;
    int c4_xa = 0, c4_xb = 0, sh_eff = 0;
    float* origin_g() const { return g + (size_t)halo * pitch; }
    float* origin_e() const { return e + (size_t)halo * pitch; }
};
}  // namespace

struct stitch_band {
    int device = 0, cw = 0, ch = 0, rank = 0, nranks = 1, Ls = 0, L = 0;
    stitch_blend_opts opts{};
    VVK vvk{};
    BandLevel lv[32];  // 0..Ls (level Ls: this rank's band of the first replicated level, the decimation's output)
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
    bool src_l0 = true;
    int px = 0;  // sizeof the pixel type of the last compose (1 / 4)
    PairArgs<uint8_t> pa8x{}, pa8c{};
    PairArgs<float> pafx{}, pafc{};
    float* mask_side = nullptr;  // [pitch]: the x-blurred row of the implicit level-0 mask
    uint8_t *zt = nullptr, *zi = nullptr;  // zero-tile flags of level 0: [7][NC][NR] of T, [NC][NR] of the index plane (see ZeroTiles)
    int zt_level = -1;  // the level whose fused reduce left flags for its anticausal sweep (-1: none)
    bool zero_tiles = true;  // STITCH_NO_ZERO_TILES, read once at creation (a flag written must be a flag read)
    bool plain_dec = false;  // STITCH_BAND_PLAIN, read once at creation
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
ZeroTiles band_zero_tiles(const stitch_band* b, uint8_t* flags, int level = 0);
MaskL0 band_mask(const stitch_band* b) { return MaskL0{b->d_seam, b->mask_side, b->lv[0].rows + 2 * b->lv[0].halo, 1}; }
}  // namespace

namespace {
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
    const BandLevel& a = b->lv[0];
    b->px = (int)sizeof(PX);
    if (b->src_l0) {
        if ((unsigned long long)fw * fh * sizeof(PX) >= 0xfffffff0ULL || (unsigned long long)mw * mh * sizeof(PX) >= 0xfffffff0ULL)
            return fail(STITCH_ERR_ARG, "band_compose: a channel plane of the inputs must stay below 4 GB for the source-fused level 0");
        const int ph = a.rows + 2 * a.halo, ybase = a.row0 - a.halo;
        PairArgs<PX>& px = band_pa<PX>(b, false);
        PairArgs<PX>& pc = band_pa<PX>(b, true);
        px = pa, pc = pa;
        px.oy[0] = oy + ybase, pc.oy[0] = oy + a.row0;
        // the index plane of the band's rows and its halo rows (a halo row outside the canvas maps wherever the map says: it is
        // swept along x like every halo row and never read)
        const ZeroTiles zi = band_zero_tiles(b, b->zi);  // tiles of the index plane that lie outside the frame altogether
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
    const BandLevel& a = b->lv[level];
    const BandLevel& nx = b->lv[level + 1];
    const bool top_src = level + 1 == b->Ls;  // the source level is replicated: all rows, dense planes
    const float* gn = top_src ? b->gtop : nx.g;
    const float* en = top_src ? b->etop : nx.e;
    const int spitch = top_src ? nx.w : nx.pitch;
    const size_t sps = top_src ? (size_t)nx.w * nx.h_full : nx.ps;
    int xa = a.c4_xa, xb = a.c4_xb;
    const int crows = std::max(4, std::min(32, a.rows / 8));
    const int strips = (a.rows + crows - 1) / crows;
    if (level == 0) {
        if ((a.w % 4) != 0 || (reinterpret_cast<uintptr_t>(d_out) % (4 * sizeof(OUT))) != 0) xa = xb = 0;
        OutPtrs<OUT> outs{};
        outs.p[0] = d_out;
        if (b->src_l0 && b->px != (int)sizeof(OUT)) return fail(STITCH_ERR_ARG, "band_collapse: the output's pixel type differs from the composed inputs'");
        CollapseArgs<OUT, true> A{a.origin_g(), a.w, a.rows, a.pitch, a.ps, gn, en, nx.w, a.sh_eff, spitch, sps, {a.ix, a.ax, a.iy, a.ay}, outs,
                                  a.w, (size_t)a.w * a.rows, b->d_seam, b->src_l0 ? band_pa<OUT>(b, true) : PairArgs<OUT>{}, b->src_l0 ? 1 : 0, crows, xa, xb,
                                  1};  // u8_words: the aligned case only (checked above)
        const int rest = a.w - (xb - xa), nb4 = ((xb - xa) / 4 + WAVE - 1) / WAVE, ncb = (rest + C4_THREADS - 1) / C4_THREADS;
        if (xb > xa)
            k_collapse4<OUT, true><<<dim3(nb4 + ncb * C4_SUB, strips, 1), C4_THREADS, 0, s>>>(A, nb4, ncb);
        else
            k_collapse<OUT, true><<<grid_xy(a.w, strips, 1), 256, 0, s>>>(A);
    } else {
        OutPtrs<float> eo{};
        eo.p[0] = a.origin_e();
        CollapseArgs<float, false> A{a.origin_g(), a.w, a.rows, a.pitch, a.ps, gn, en, nx.w, a.sh_eff, spitch, sps, {a.ix, a.ax, a.iy, a.ay}, eo,
                                     a.pitch, a.ps, nullptr, NoPairArgs{}, 0, crows, xa, xb, 1};
        const int rest = a.pitch - (xb - xa), nb4 = ((xb - xa) / 4 + WAVE - 1) / WAVE, ncb = (rest + C4_THREADS - 1) / C4_THREADS;
        if (xb > xa)
            k_collapse4<float, false><<<dim3(nb4 + ncb * C4_SUB, strips, 1), C4_THREADS, 0, s>>>(A, nb4, ncb);
        else
            k_collapse<float, false><<<grid_xy(a.pitch, strips, 1), 256, 0, s>>>(A);
    }
    b->last_stream = s, b->pending = true;
    return launch_check("band_collapse");
}
}  // namespace

namespace {
Bands band_bands(const stitch_band* b) {
    const int ph = b->lv[0].rows + 2 * b->lv[0].halo;
    return Bands{(ph + TS - 1) / TS, ph};
}
// Zero-tile flags of level 0 (as in a plan, and under its conditions: every user of T is a fused form -- so only with
// reduce_xy_fwd --, an even width, at most 256 bands per plane); planes = 7 for T's flags, 1 for the index plane's.
ZeroTiles band_zero_tiles(const stitch_band* b, uint8_t* flags, int level) {
    const BandLevel& a = b->lv[level];
    ZeroTiles z{};
    const int NR = (a.rows + TS - 1) / TS;
    if ((level > 0 || b->src_l0) && (a.w & 1) == 0 && NR <= 256 && a.halo == 0 && b->zero_tiles && !b->plain_dec) {  // the two-kernel form reads every tile
        z.flags = flags;  // one buffer, sized for level 0: a level's flags live from its causal x sweep to its anticausal y sweep
        z.h = a.rows;
        z.NR = NR;
        z.NC = (a.w + TS - 1) / TS;
    }
    return z;
}
// the causal x sweep of a source-fused level 0: frame channels through the index plane, the mosaic as a shift, the mask generated
int band_x_fwd_src(stitch_band* b, hipStream_t s, bool flags) {
    const BandLevel& a = b->lv[0];
    const Bands bd = band_bands(b);
    const long lines = 7L * bd.h;
    const ZeroTiles zt = flags ? band_zero_tiles(b, b->zt) : ZeroTiles{}, zi = band_zero_tiles(b, b->zi);
    if (b->px == 1)
        k_vv_x_fwd<uint8_t, true><<<7 * bd.nr, 64, 0, s>>>(a.g, b->T, a.w, a.pitch, lines, b->vvk, b->state_x, band_mask(b), b->pa8x, zt, zi, nullptr, bd);
    else if (b->px == 4)
        k_vv_x_fwd<float, true><<<7 * bd.nr, 64, 0, s>>>(a.g, b->T, a.w, a.pitch, lines, b->vvk, b->state_x, band_mask(b), b->pafx, zt, zi, nullptr, bd);
    else
        return fail(STITCH_ERR_ARG, "band: reduce before compose");
    return STITCH_OK;
}
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
    if (nranks < 1 || rank < 0 || rank >= nranks) return fail(STITCH_ERR_ARG, "band_create: rank %d of %d", rank, nranks);
    int lw[32], lh[32];
    const int L = pyramid_levels(cw, ch, 0, lw, lh);
    if (L < 0) return L;
    const int Ls = split_levels;
    if (Ls < 1 || Ls > L - 1) return fail(STITCH_ERR_ARG, "band_create: split_levels must be 1..%d for a %d-level pyramid", L - 1, L);
    for (int l = 0; l <= Ls; ++l) {
        const int q = l < Ls ? 2 * nranks : nranks;  // split levels: even band heights (the 2:1 decimation stays inside a band)
        if (lh[l] % q != 0 || lh[l] / nranks < (l < Ls ? 2 * BAND_HALO : 1))
            return fail(STITCH_ERR_ARG, "band_create: level %d has %d rows, not divisible into %d bands of even height >= %d", l, lh[l], nranks,
                        2 * BAND_HALO);
        if (lw[l] < 2) return fail(STITCH_ERR_ARG, "band_create: level %d is %d columns wide", l, lw[l]);
    }
    stitch_band* b = new stitch_band();
    b->cw = cw, b->ch = ch, b->rank = rank, b->nranks = nranks, b->Ls = Ls, b->L = L, b->opts = o;
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
        BandLevel& v = b->lv[l];
        v.w = lw[l], v.h_full = lh[l], v.rows = lh[l] / nranks, v.row0 = rank * v.rows, v.pitch = round_up(v.w, 64);
        v.halo = l == 0 || nranks == 1 ? 0 : BAND_HALO;  // a band without neighbours has nobody's rows to hold
        v.ps = (size_t)v.pitch * (v.rows + 2 * v.halo);
        g_off[l] = take(sizeof(float) * (v.ps * 7 + (size_t)v.pitch * 64));  // + slack rows for the x sweeps' last partial block
        e_off[l] = (l >= 1 && l < Ls) ? take(sizeof(float) * v.ps * 3) : 0;
        if (l < Ls) {
            ix_off[l] = take(sizeof(int32_t) * v.w);
            ax_off[l] = take(sizeof(double) * v.w);
            iy_off[l] = take(sizeof(int32_t) * v.rows);
            ay_off[l] = take(sizeof(double) * v.rows);
        }
    }
    const BandLevel& v0 = b->lv[0];
    const size_t t_off = take(sizeof(float) * (v0.ps * 7 + (size_t)v0.pitch * 64));
    const size_t st_off = take(sizeof(double) * 4 * 7 * (size_t)(v0.rows + 2 * BAND_HALO + 64));
    const size_t seam_off = take(sizeof(SeamDev));
    const size_t side_off = take(sizeof(float) * v0.pitch);
    const size_t ntile0 = (size_t)((v0.rows + TS - 1) / TS) * ((v0.w + TS - 1) / TS);
    const size_t zt_off = take(7 * ntile0), zi_off = take(ntile0);
    const size_t yg_off = take(sizeof(u64) * (7 * (size_t)(v0.pitch / TS) * WF_GRAN * WAVE + 1));
    const size_t wfc_off = take(sizeof(unsigned) * 64);
    const size_t gtop_off = take(sizeof(float) * 7 * (size_t)lw[Ls] * lh[Ls]);
    const size_t etop_off = take(sizeof(float) * 3 * (size_t)lw[Ls] * lh[Ls]);
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
    // the band's switches, read ONCE here with the plan's semantics (Tuning::env_int: set and > 0; "=0" means off, as for a plan)
    b->zero_tiles = !(Tuning::env_int("STITCH_NO_ZERO_TILES") > 0);
    b->src_l0 = !(Tuning::env_int("STITCH_BAND_PLANES") > 0);  // STITCH_BAND_PLANES=1: materialised level-0 planes and mask (rounds 1-2)
    b->plain_dec = Tuning::env_int("STITCH_BAND_PLAIN") > 0;   // STITCH_BAND_PLAIN=1: anticausal y sweep and decimation as two kernels (A/B)
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
        // the reference's tables for the whole level (CImg.h:29625-29637); rows re-based to what this rank holds of level l+1:
        // its band with BAND_HALO rows either side (source row 0 of the buffer = row0_{l+1} - HALO), or all rows when l+1 is
        // the first replicated level
        std::vector<int32_t> idx;
        std::vector<double> al;
        expand_table(lw[l + 1], v.w, idx, al);
        regular_range(idx, v.w, lw[l + 1], lh[l + 1], &v.c4_xa, &v.c4_xb);
        bool ok = hipMemcpy(v.ix, idx.data(), sizeof(int32_t) * v.w, hipMemcpyHostToDevice) == hipSuccess &&
                  hipMemcpy(v.ax, al.data(), sizeof(double) * v.w, hipMemcpyHostToDevice) == hipSuccess;
        expand_table(lh[l + 1], lh[l], idx, al);
        const bool top_src = l + 1 == Ls;
        const int nh = b->lv[l + 1].halo;
        const int src_base = top_src ? 0 : b->lv[l + 1].row0 - nh, src_rows = top_src ? lh[l + 1] : b->lv[l + 1].rows + 2 * nh;
        std::vector<int32_t> iyl(v.rows);
        for (int y = 0; y < v.rows; ++y) {
            const int gi = idx[v.row0 + y], gi2 = gi < lh[l + 1] - 1 ? gi + 1 : gi;
            iyl[y] = gi - src_base;
            if (iyl[y] < 0 || gi2 - src_base >= src_rows) {
                stitch_band_destroy(b);
                return fail(STITCH_ERR_ARG, "band_create: level %d row %d needs source row %d..%d, outside the band's halo", l, v.row0 + y, gi, gi2);
            }
        }
        // `iy < sh - 1 ? iy + 1 : iy` of the kernels must clamp at the LEVEL's last row only
        v.sh_eff = top_src ? lh[l + 1] : (rank == nranks - 1 ? b->lv[l + 1].rows + nh : (1 << 30));
        ok = ok && hipMemcpy(v.iy, iyl.data(), sizeof(int32_t) * v.rows, hipMemcpyHostToDevice) == hipSuccess &&
             hipMemcpy(v.ay, al.data() + v.row0, sizeof(double) * v.rows, hipMemcpyHostToDevice) == hipSuccess;
        if (!ok) {
            stitch_band_destroy(b);
            return fail(STITCH_ERR_HIP, "band_create: table upload failed");
        }
    }
    // the replicated levels: an ordinary single-pair plan whose level 0 is level Ls, handed in as planes
    if ((rc = stitch_plan_create(lw[Ls], lh[Ls], &o, &b->top))) {
        stitch_band_destroy(b);
        return rc;
    }
    if (b->top->L != L - Ls) {
        stitch_band_destroy(b);
        return fail(STITCH_ERR_PYRAMID, "band_create: the coarse plan has %d levels, expected %d", b->top->L, L - Ls);
    }
    b->top->planes_in = true;
    b->top->mask_opt = false;
    b->top->src_fuse = false;
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
    b->src_l0 = source_fused != 0;
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
    const BandLevel& a = b->lv[level];
    const long lines = 7L * (a.rows + 2 * a.halo);  // halo rows are swept too (their contents are never used)
    if (b->zt_level == level) b->zt_level = -1;  // the separate sweeps leave no flags
    if (level == 0 && b->src_l0) {
        if ((rc = band_x_fwd_src(b, s, false))) return rc;
        const Bands bd = band_bands(b);
        k_vv_x_bwd<<<7 * bd.nr, 64, 0, s>>>(b->T, a.w, a.pitch, lines, b->vvk, b->state_x, band_mask(b), bd);
    } else {
        const int nb = (int)((lines + TS - 1) / TS);
        k_vv_x_fwd<float, false><<<nb, 64, 0, s>>>(a.g, b->T, a.w, a.pitch, lines, b->vvk, b->state_x, MaskL0{}, NoPairArgs{}, ZeroTiles{}, ZeroTiles{}, nullptr, Bands{});
        k_vv_x_bwd<<<nb, 64, 0, s>>>(b->T, a.w, a.pitch, lines, b->vvk, b->state_x, MaskL0{}, Bands{});
    }
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
    const int ph = a.rows + 2 * a.halo;
    const long lines = 7L * ph;  // halo rows are swept along x too (their contents are never used)
    const int nb = (int)((lines + TS - 1) / TS);
    const bool src = level == 0 && b->src_l0;
    const ZeroTiles zt = level < 2 ? band_zero_tiles(b, b->zt, level) : ZeroTiles{};
    b->zt_level = zt.flags ? level : (b->zt_level == level ? -1 : b->zt_level);
    if (src) {
        if ((rc = band_x_fwd_src(b, s, true))) return rc;
    } else if (zt.flags)  // per-plane bands: a block's flags belong to one plane
        k_vv_x_fwd<float, false><<<7 * zt.NR, 64, 0, s>>>(a.g, b->T, a.w, a.pitch, lines, b->vvk, b->state_x, MaskL0{}, NoPairArgs{}, zt, ZeroTiles{}, nullptr, Bands{zt.NR, a.rows});
    else
        k_vv_x_fwd<float, false><<<nb, 64, 0, s>>>(a.g, b->T, a.w, a.pitch, lines, b->vvk, b->state_x, MaskL0{}, NoPairArgs{}, ZeroTiles{}, ZeroTiles{}, nullptr, Bands{});
    Wavefront wf{};
    wf.mask_l0 = src ? 1 : 0;  // the mask plane's rows below its first band are the row that travels with the y state
    wf.zt = zt;
    wf.yg = b->wf_yg;
    wf.counter = b->wf_ctrl;
    wf.abort = b->wf_ctrl + 16;
    wf.sticky = b->wf_ctrl + 32;
    wf.spin_limit = 1u << 23;
    wf.NR = (a.rows + TS - 1) / TS;
    wf.NC = (a.w + TS - 1) / TS;
    wf.NP = 7;
    wf.epoch = 1;
    wf.early_read = 1;
    wf.ph = ph;
    wf.y0 = a.halo;
    wf.resume = d_resume;
    const size_t gran_words = (size_t)wf.NP * wf.NC * WF_GRAN * WAVE;
    k_clear_words<<<(int)std::min<size_t>((gran_words + 255) / 256, 2048), 256, 0, s>>>(b->wf_yg, gran_words);
    k_clear_words<<<1, 64, 0, s>>>((u64*)b->wf_ctrl, 16);  // queue head and abort word; the sticky count stays
    const long ntiles = (long)wf.NP * wf.NR;
    // a level without halo rows that starts at the image's first row is exactly a plan's launch: the plain instance (the BANDED
    // one carries more scalars through the tile loop and is a few per cent slower)
    if (a.halo == 0 && !d_resume)
        k_vv_xbyf<false><<<(int)std::min<long>(ntiles, 2304), 64, 0, s>>>(b->T, a.w, a.rows, a.pitch, b->vvk, b->state_x, lines, d_state_out, wf, Recompute{}, NoPairArgs{});
    else
        k_vv_xbyf<false, float, 0, true><<<(int)std::min<long>(ntiles, 2304), 64, 0, s>>>(b->T, a.w, a.rows, a.pitch, b->vvk, b->state_x, lines, d_state_out, wf,
                                                                                          Recompute{}, NoPairArgs{});
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
    hipStream_t s = as_stream(stream);
    const BandLevel& a = b->lv[level];
    const int np = plane < 0 ? 7 : 1;  // all planes in one launch: states are [k][7][pitch]
    float* t = b->T + (size_t)(plane < 0 ? 0 : plane) * a.ps + (size_t)a.halo * a.pitch;
    const bool src = level == 0 && b->src_l0;
    if (src && plane >= 0) return fail(STITCH_ERR_ARG, "band_reduce_y_fwd: one plane at a time needs the materialised level 0 (STITCH_BAND_PLANES=1)");
    // source-fused level 0: the mask plane's input is one x-blurred row for every y (MaskL0::side), shifted to the band's first row
    MaskL0 mk = src ? band_mask(b) : MaskL0{};
    k_vv_y_fwd<<<dim3((a.pitch + YCOLS - 1) / YCOLS, np), 64, 0, s>>>(t, a.rows, a.pitch, a.ps, b->vvk, d_state_out, mk, d_resume);
    b->last_stream = s, b->pending = true;
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
    hipStream_t s = as_stream(stream);
    const BandLevel& a = b->lv[level];
    const BandLevel& d = b->lv[level + 1];
    const int np = plane < 0 ? 7 : 1;
    float* t = b->T + (size_t)(plane < 0 ? 0 : plane) * a.ps + (size_t)a.halo * a.pitch;
    float* dst = d.origin_g() + (size_t)(plane < 0 ? 0 : plane) * d.ps;
    const dim3 g((a.pitch + YCOLS - 1) / YCOLS, np);
    const ZeroTiles zt = b->zt_level == level && plane < 0 ? band_zero_tiles(b, b->zt, level) : ZeroTiles{};
    if (zt.flags && (a.rows % YCH) != 0 && !b->plain_dec)  // a chunk of rows may straddle two bands: per-row flag look-up
        k_vv_y_bwd_dec<true><<<g, 128, 0, s>>>(t, a.w, a.rows, a.pitch, a.ps, b->vvk, d_fwd_state, dst, d.w, d.rows, d.pitch, d.ps, zt, d_resume, d_state_out,
                                               a.h_full, d.h_full);
    else if ((a.w & 1) == 0 && !b->plain_dec)
        k_vv_y_bwd_dec<<<g, 128, 0, s>>>(t, a.w, a.rows, a.pitch, a.ps, b->vvk, d_fwd_state, dst, d.w, d.rows, d.pitch, d.ps, zt, d_resume,
                                         d_state_out, a.h_full, d.h_full);
    else {
        k_vv_y_bwd<<<g, 64, 0, s>>>(t, a.rows, a.pitch, a.ps, b->vvk, d_fwd_state, d_resume, d_state_out);
        k_decimate<<<grid_xy(d.pitch, d.rows, np), 256, 0, s>>>(t, a.w, a.h_full, a.pitch, a.ps, dst, d.w, d.h_full, d.pitch, d.ps, d.row0, a.row0);
    }
    b->last_stream = s, b->pending = true;
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
    if (x0 < 0 || x1 <= x0 || x0 % YCOLS || (x1 % YCOLS && x1 != a.pitch) || x1 > a.pitch || !d_state_out || (b->rank > 0) != (d_resume != nullptr))
        return fail(STITCH_ERR_ARG, "band_reduce_y_fwd_cols: columns [%d, %d) must be multiples of %d inside the pitch %d, with a state buffer and a resume state exactly on ranks > 0", x0, x1, YCOLS, a.pitch);
    hipStream_t s = as_stream(stream);
    float* t = b->T + (size_t)a.halo * a.pitch;
    const bool src = level == 0 && b->src_l0;
    MaskL0 mk = src ? band_mask(b) : MaskL0{};
    k_vv_y_fwd<true><<<dim3((x1 - x0 + YCOLS - 1) / YCOLS, 7), 64, 0, s>>>(t, a.rows, a.pitch, a.ps, b->vvk, d_state_out, mk, d_resume, x0);
    b->last_stream = s, b->pending = true;
    return launch_check("band_reduce_y_fwd_cols");
}
int stitch_band_reduce_y_bwd_cols(stitch_band* b, int level, int x0, int x1, const double* d_fwd_state, const double* d_resume, double* d_state_out,
                                  void* stream) {
    int rc = band_check(b, level, b ? b->Ls - 1 : 0);
    if (rc) return rc;
    const BandLevel& a = b->lv[level];
    const BandLevel& d = b->lv[level + 1];
    if (x0 < 0 || x1 <= x0 || x0 % YCOLS || (x1 % YCOLS && x1 != a.pitch) || x1 > a.pitch || !d_fwd_state || !d_state_out ||
        (b->rank < b->nranks - 1) != (d_resume != nullptr))
        return fail(STITCH_ERR_ARG, "band_reduce_y_bwd_cols: columns [%d, %d) must be multiples of %d inside the pitch %d, with state buffers and a resume state exactly on ranks below the last", x0, x1, YCOLS, a.pitch);
    if ((a.w & 1) != 0 || b->plain_dec) return fail(STITCH_ERR_ARG, "band_reduce_y_bwd_cols: even level widths and the fused decimation only (level %d is %d wide)", level, a.w);
    hipStream_t s = as_stream(stream);
    float* t = b->T + (size_t)a.halo * a.pitch;
    float* dst = d.origin_g();
    const dim3 g((x1 - x0 + YCOLS - 1) / YCOLS, 7);
    const ZeroTiles zt = b->zt_level == level ? band_zero_tiles(b, b->zt, level) : ZeroTiles{};
    if (zt.flags && (a.rows % YCH) != 0)
        k_vv_y_bwd_dec<true, YST, true, false, true><<<g, 128, 0, s>>>(t, a.w, a.rows, a.pitch, a.ps, b->vvk, d_fwd_state, dst, d.w, d.rows, d.pitch, d.ps, zt, d_resume,
                                                                    d_state_out, a.h_full, d.h_full, x0);
    else
        k_vv_y_bwd_dec<false, YST, true, false, true><<<g, 128, 0, s>>>(t, a.w, a.rows, a.pitch, a.ps, b->vvk, d_fwd_state, dst, d.w, d.rows, d.pitch, d.ps, zt, d_resume,
                                                                     d_state_out, a.h_full, d.h_full, x0);
    b->last_stream = s, b->pending = true;
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
