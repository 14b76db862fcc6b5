// Part of stitch_kernels.hpp (included there, inside namespace sk): Van Vliet recursive Gaussian: causal / anticausal x and y sweeps, fused anticausal-y + decimation (B3, B4).
// ---- B3: Van Vliet recursive Gaussian, CImg.h:34887-34932 ---------------------------------------------------
// The recurrence is strictly sequential along a line (double accumulators that keep their unrounded value,
// every output stored to float), so the parallel axis is "lines": one line per work-item.
//
// x pass: a wavefront owns 64 consecutive rows.  Rows are moved between HBM and LDS as 64x64 tiles with
// 16-byte-per-lane accesses (a lane loads 4 consecutive samples of one row, 16 lanes cover a 256-byte row
// segment); in LDS a row is padded to 68 floats so that both the row-wise tile traffic and the per-lane
// ds_read_b128 of "my row" are bank-conflict free.  The next tile is prefetched into registers while the
// current one runs its 64 recurrence steps.  The forward kernel leaves (v1,v2,v3,iplus) of every line in
// `state`; the backward kernel starts from the Triggs boundary values computed from them.
constexpr int TP = 68;  // padded LDS row (floats)
static_assert(TP == TS + 4, "k_src_runs (k_compose.inc) records a patch's position in the padded tile");

__device__ __forceinline__ void tile_load(const float* __restrict__ base, int pitch, int c0, int lane, f4 pre[16]) {
    // lane -> (row group, 4-column group): rows lane/16 + 4*i, columns 4*(lane%16)..+3
    const float* p = base + (size_t)(lane >> 4) * pitch + c0 + ((lane & 15) << 2);
#pragma unroll
    for (int i = 0; i < 16; ++i) pre[i] = *reinterpret_cast<const f4*>(p + (size_t)(4 * i) * pitch);
}
__device__ __forceinline__ void tile_to_lds(float* tile, int lane, const f4 pre[16]) {
    float* t = tile + (lane >> 4) * TP + ((lane & 15) << 2);
#pragma unroll
    for (int i = 0; i < 16; ++i) *reinterpret_cast<f4*>(t + (4 * i) * TP) = pre[i];
}
__device__ __forceinline__ void tile_store(float* __restrict__ base, int pitch, int c0, int lane, const float* tile) {
    float* p = base + (size_t)(lane >> 4) * pitch + c0 + ((lane & 15) << 2);
    const float* t = tile + (lane >> 4) * TP + ((lane & 15) << 2);
#pragma unroll
    for (int i = 0; i < 16; ++i)
        __builtin_nontemporal_store(*reinterpret_cast<const f4*>(t + (4 * i) * TP), reinterpret_cast<f4*>(p + (size_t)(4 * i) * pitch));
}

// How the blocks of an x sweep map to lines.  nr == 0: `lines` = the rows of all planes stacked, block b owns lines
// 64b .. 64b+63 (a block may straddle two planes: fine when every line is treated alike).  nr > 0: block b owns band
// b % nr (64 rows, the last one of a plane possibly partial) of plane b / nr -- never more than one plane, which is what
// the implicit level-0 mask, the source-fused level 0 and the zero-tile flags need (their treatment of a block depends on
// its plane), at ANY plane height.
struct Bands {
    int nr, h;  // bands per plane (0 = stacked lines), rows per plane
};

// Level-0 mask without a level-0 mask plane.  The reference's mask[0] is a vertical step (ImageProcess.cpp:690-698):
// every row is the same function of x, so (with per-plane blocks, Bands) the x sweeps generate the step on the fly,
// compute only the first 64 of its identical rows,
// leave the x-blurred row in a small side buffer, and the causal y sweep reads that one row for every y.  The
// collapse kernel evaluates the step directly.  Saves one plane write and six plane reads/writes of level 0.
struct MaskL0 {
    const SeamDev* seam;  // per pair
    float* side;          // [pairs][pitch]: the x-blurred mask row
    int h;                // level height = lines per plane
    int enabled;
    const unsigned* keep; // any level: the slots' mask_todo words (k_mask_keys, mask_stands), or nullptr
};
// The mask pyramid of a slot stands (k_mask_keys, k_compose.inc): an earlier call of the same form and the same seam record wrote plane 6
// of every G_l >= 1 and its row-repeat flags, and this call leaves them as they are, bit for bit.  Every kernel between G_l and G_{l+1}
// drops the work of such a plane under the SAME word, which a kernel earlier in stream order wrote: the scratch of that plane (T, the sweep
// states, its T flags, the side row) is then neither written nor read by anyone.  todo == nullptr (a band, a call that does not take
// part): every plane is computed.
__device__ __forceinline__ bool mask_stands(const unsigned* __restrict__ todo, long plane) {
    return todo != nullptr && plane % 7 == 6 && todo[plane / 7] == 0u;
}
__device__ __forceinline__ float mask_step(const SeamDev& sd, int x) {
    return sd.branch == 0 ? ((double)x < sd.thr ? 1.f : 0.f) : (x >= sd.start ? 1.f : 0.f);
}

__device__ __forceinline__ void tile_store_rows(float* __restrict__ base, int pitch, int c0, int lane, const float* tile, int nrows) {
    float* p = base + (size_t)(lane >> 4) * pitch + c0 + ((lane & 15) << 2);
    const float* t = tile + (lane >> 4) * TP + ((lane & 15) << 2);
#pragma unroll
    for (int i = 0; i < 16; ++i)
        if ((lane >> 4) + 4 * i < nrows)
            __builtin_nontemporal_store(*reinterpret_cast<const f4*>(t + (4 * i) * TP), reinterpret_cast<f4*>(p + (size_t)(4 * i) * pitch));
}

// Source-fused level 0: plane byte offsets of one 64x64 tile in tile_load's element-to-lane layout (or "outside"),
// and the gather through them.  k_compose's two stores: the warped sample goes through the degenerate bilinear call,
// the moved one is a copy.
template <typename PX>
__device__ __forceinline__ void mosaic_indices(const XShift& ms, int c0, int lane, int y0, int w, f4 nidx[16]) {
    const int c = c0 + ((lane & 15) << 2);
    const unsigned c0i = mosaic_col<PX>(ms, c, w), c1i = mosaic_col<PX>(ms, c + 1, w), c2i = mosaic_col<PX>(ms, c + 2, w),
                   c3i = mosaic_col<PX>(ms, c + 3, w);
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        const unsigned row = mosaic_row<PX>(ms, y0 + (lane >> 4) + 4 * i);
        f4 v;
        v.x = __uint_as_float(mosaic_offset<PX>(row, c0i));
        v.y = __uint_as_float(mosaic_offset<PX>(row, c1i));
        v.z = __uint_as_float(mosaic_offset<PX>(row, c2i));
        v.w = __uint_as_float(mosaic_offset<PX>(row, c3i));
        nidx[i] = v;
    }
}
template <typename PX>
__device__ __forceinline__ float src_px(__amdgpu_buffer_rsrc_t rs, bool warped, unsigned byte_off) {
    const float v = buf_px<PX>(rs, byte_off);
    return warped ? warped_px<PX>(v) : v;
}
template <typename PX>
__device__ __forceinline__ void src_gather(__amdgpu_buffer_rsrc_t rs, const f4 nidx[16], f4 pre[16]) {  // raw bits
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        const f4 id = nidx[i];
        f4 v;
        v.x = buf_raw<PX>(rs, __float_as_uint(id.x));
        v.y = buf_raw<PX>(rs, __float_as_uint(id.y));
        v.z = buf_raw<PX>(rs, __float_as_uint(id.z));
        v.w = buf_raw<PX>(rs, __float_as_uint(id.w));
        pre[i] = v;
    }
}
// The same tile through the groups' bases (SrcRuns): 16 loads of 16 bytes.  A base is the offset of a group whose 16 bytes lie inside
// the plane, or SR_BASE_OUTSIDE, whose four words all lie beyond it and read as 0: no load straddles the plane's end.
__device__ __forceinline__ void src_gather_runs(__amdgpu_buffer_rsrc_t rs, const f4 nbase[4], f4 pre[16]) {  // raw bits
#pragma unroll
    for (int i = 0; i < 16; ++i)
        pre[i] = __builtin_bit_cast(f4, __builtin_amdgcn_raw_buffer_load_b128(rs, __float_as_uint(nbase[i >> 2][i & 3]), 0, 0));
}
template <typename PX>
__device__ __forceinline__ void src_finish(bool warped, f4 pre[16]) {  // raw bits -> the value k_compose would have stored
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        f4 v = pre[i];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float t = raw_to_px<PX>(v[j]);
            v[j] = warped ? warped_px<PX>(t) : t;
        }
        pre[i] = v;
    }
}

// `lines` = rows of all planes stacked (plane stride = pitch*h, so line L starts at L*pitch); the buffers are
// allocated with 64 spare rows so that a partial last block may touch rows >= lines without leaving them.
// Level 0 of a source-fused plan (use_src; needs mk.enabled and per-plane bands): the input
// tile is not read from `in` but evaluated from the pair's frames (PairSrc), so S1 never materialises.
// CKPT (a level whose anticausal sweep re-runs the causal one tile by tile, k_vv_xbyf MODE 1/2): the swept samples are not
// written at all; what is kept is the recurrence state in front of every tile (ckpt[3][tiles][lines], doubles), from which
// the consumer reproduces the tile's samples exactly -- 24 bytes per 64 samples instead of 256 written and read back.
template <typename PX, bool SRC, bool CKPT = false>
__global__ __launch_bounds__(64) void k_vv_x_fwd(const float* __restrict__ in, float* __restrict__ out, int w, int pitch,
                                                  long lines, VVK k, double* __restrict__ state, MaskL0 mk,
                                                  typename CollapseSrc<PX, SRC>::type pa, ZeroTiles zt, ZeroTiles zi,
                                                  double* __restrict__ ckpt, Bands bd, ZeroTiles mr = ZeroTiles{}, SrcRuns sr = SrcRuns{}) {
    __shared__ __attribute__((aligned(16))) float tile[TS * TP];
    const int lane = threadIdx.x;
    long blk = blockIdx.x;
    if (SRC && bd.nr > 0 && bd.nr % 8 == 0) {
        // Source-fused level 0: the three channel sweeps of a band read the same index tiles.  Workgroups go round-robin
        // over the 8 XCDs (each with its own L2), so the planes of a pair are interleaved in groups of 8 bands: the seven
        // blocks of one band are then 8 apart -- same XCD, dispatched together -- so that a re-read of an index tile can
        // be served on the chip.  (Plain order: plane-major, the channels of a band 64 blocks apart in time.)  Measured:
        // the kernel is 1.5 % faster, but FETCH_SIZE (traffic leaving the L2) is unchanged -- at 8 workgroups per CU a
        // 4 MB L2 does not keep a tile from one channel sweep to the next; what helps is the memory-side cache.
        const long nr = bd.nr, per_pair = 7 * nr, pr_ = blk / per_pair, r = blk % per_pair;
        const long band = (r / 56) * 8 + r % 8, q = (r / 8) % 7;
        blk = pr_ * per_pair + q * nr + band;
    }
    // wave-uniform: this block's plane, first row within it and number of rows (per-plane bands), or 64 stacked lines
    const long plane = bd.nr > 0 ? blk / bd.nr : 0;
    const int band_y0 = bd.nr > 0 ? (int)(blk % bd.nr) * TS : 0;
    const int nrows = bd.nr > 0 ? min(TS, bd.h - band_y0) : TS;
    const long line0 = bd.nr > 0 ? plane * bd.h + band_y0 : blk * TS, line = line0 + lane;
    const float* ib = in + (size_t)line0 * pitch;
    float* ob = out + (size_t)line0 * pitch;
    const int ntiles = (w + TS - 1) / TS;
    const bool live = lane < nrows && line < lines;
    // A block whose lines all belong to mask planes that stand has nothing to do (mask_stands): its plane with per-plane bands, every
    // line's plane with stacked lines -- one wave-uniform answer; a block that mixes planes runs as before
    if (mk.keep != nullptr && (bd.nr > 0 ? mask_stands(mk.keep, plane) : __all(line >= lines || mask_stands(mk.keep, line / mk.h)))) return;
    // Row-repeat flags of this level's mask plane (mask_rows; per-plane bands): a flagged tile of a band below the first was not stored
    // and its 64 rows are taken from row 0 of the plane -- an address select, the loads stay unconditional.  At a fused level (T flags:
    // k_vv_xbyf knows the flags too) a band whose tiles are ALL flagged has nothing to do here, like the level-0 step below its first band.
#if STITCH_MASK_ROWS_IGNORE & 1  // (hand-check libraries only: proves that the stale-data tests see a sweep that ignores the flags)
    const bool mr_on = false;
#else
    const bool mr_on = !SRC && !CKPT && mr.flags != nullptr && plane % 7 == 6 && band_y0 > 0;  // wave-uniform
#endif
    const float* row0 = in + (size_t)plane * bd.h * pitch;
    auto tile_row0 = [&](int t) -> bool { return mr_on && mr.flags[mr.index(plane / 7, band_y0 / TS, t)] != 0; };
    if (mr_on && zt.flags) {
        bool all = true;
        for (int t0 = 0; t0 < ntiles; t0 += WAVE) all = all && __all(t0 + lane >= ntiles || mr.flags[mr.index(plane / 7, band_y0 / TS, min(t0 + lane, ntiles - 1))] != 0);
        if (all) return;
    }
    bool gen_mask = false;  // wave-uniform: this block's 64 lines are rows of a level-0 mask plane
    SeamDev sd;
    int src_q = 0, src_y0 = 0, src_pr = 0;  // wave-uniform: plane, first row and pair of this block (use_src)
    if (mk.enabled) {  // the host launches per-plane bands (bd.nr > 0) whenever the mask is implicit
        if (plane % 7 == 6) {
            if (band_y0 >= TS) return;  // rows 64.. of the step are copies of rows 0..63 and are never read
            gen_mask = true;
            sd = mk.seam[plane / 7];
        }
        src_q = (int)(plane % 7);
        src_pr = (int)(plane / 7);
        src_y0 = band_y0;
    }
    // frame channels come through the index plane; the mosaic -- and canvas a of a dense pair -- are pure shifts
    const bool gen_frame = SRC && !gen_mask && src_q < 3 && !a_is_dense(pa), gen_mosaic = SRC && !gen_mask && !gen_frame;
    const __amdgpu_buffer_rsrc_t rs = x_rsrc<PX>(pa, src_pr, src_q);
    const XShift ms = x_shift<PX>(pa, src_pr, src_q);
    // rows src_y0.. of the pair's index plane (the slot of level-0 plane 0)
    const int idx_pr = index_owner(pa, src_pr);  // (an equal pair of the call may own the plane and its flags)
    const float* idx_rows = in + ((size_t)idx_pr * 7 * bd.h + src_y0) * pitch;
    // Element indices of the next tile, produced one tile ahead of the gather that consumes them: loaded from the index
    // plane (frame channels) or computed (the mosaic is a pure shift).
    f4 nidx[SRC ? 16 : 1];
    // index tile t of this block's band: from the index plane, or all "outside" when k_src_index left the tile's flag set
    // frame channels: tile t of this band lies outside the frame altogether (k_src_index's flag): its samples are +0
    auto tile_outside = [&](int t) -> bool {
        if constexpr (SRC) return gen_frame && zi.flags && zi.flags[zi.index(idx_pr, src_y0 >> 6, t)];
        // planes of G_1 / G_2: `zi` carries the level's G column flags (g_cols; per-plane bands) -- a flagged tile column was not stored
        return zi.flags && zi.flags[zi.index(plane, 0, t)];
    };
    // Frame channels of float frames with the plane's runs at hand (SrcRuns): a tile of class <= 64 is gathered through its 16 bases
    // (nidx[0..3]) and mended by at most one patch per lane (record in nidx[4]); class 255 goes through the index tile as before.
    // The class is wave-uniform: one scalar branch per tile.
    const bool runs_on = SRC && sizeof(PX) == 4 && gen_frame && sr.cls != nullptr;
    const size_t sr_band = runs_on ? sr.tile(idx_pr, src_y0 >> 6, 0) : 0;
    unsigned ncls = src_runs::SR_GENERAL;  // class of the tile whose indices `nidx` holds
    unsigned pcls = 0, ppos = 0;           // tile in `pre`: its patches (0: none to apply), this lane's patch position and raw value
    float pval = 0.f;
    auto index_tile = [&](int t) {
        if constexpr (SRC)
            if (!tile_outside(t)) {  // an outside tile is not gathered at all
                ncls = runs_on ? __builtin_amdgcn_readfirstlane((unsigned)sr.cls[sr_band + t]) : src_runs::SR_GENERAL;
                if (ncls != src_runs::SR_GENERAL) {
                    const f4* bp = reinterpret_cast<const f4*>(sr.bases) + (sr_band + t) * (4 * WAVE) + lane;
#pragma unroll
                    for (int q = 0; q < 4; ++q) nidx[q] = bp[q * WAVE];
                    if (ncls > 0) {
                        const uint2 r = sr.patches[(sr_band + t) * src_runs::SR_MAX_PATCHES + lane];
                        nidx[4].x = __uint_as_float(r.x), nidx[4].y = __uint_as_float(r.y);
                    }
                } else
                    tile_load(idx_rows, pitch, t * TS, lane, nidx);
            }
    };
    // tile T through what index_tile(T) left in `nidx`
    auto gather_tile = [&](f4 pre_[16]) {
        pcls = 0;
        if constexpr (SRC) {
            if (gen_frame && ncls != src_runs::SR_GENERAL) {
                src_gather_runs(rs, nidx, pre_);
                pcls = ncls;
                if (pcls > 0) {
                    ppos = __float_as_uint(nidx[4].x);
                    pval = buf_raw<PX>(rs, __float_as_uint(nidx[4].y));
                }
            } else
                src_gather<PX>(rs, nidx, pre_);
        }
    };
    // The mosaic planes of float frames (sr.mosaic16): a pure shift, so a tile whose 64 columns and 64 rows all lie inside the mosaic
    // is 16 loads of 16 bytes from one computed offset per group, and a tile wholly beside the mosaic is zeros without a load; only a
    // tile the mosaic's edge crosses (or a partial last band) needs mosaic_indices' 64 range-checked offsets.  Wave-uniform per tile.
    const bool mos16 = SRC && sizeof(PX) == 4 && gen_mosaic && sr.mosaic16 != 0;
    const long long my0 = (long long)src_y0 + ms.oy;  // mosaic row of the band's first row
    const bool rows_in = nrows == TS && my0 >= 0 && my0 + TS <= ms.mh, rows_out = my0 + TS <= 0 || my0 >= ms.mh;
    enum { MK_EDGE = 0, MK_IN = 1, MK_OUT = 2 };
    auto mosaic_kind = [&](int t) -> int {
        if (!mos16) return MK_EDGE;
        const long long mx0 = (long long)t * TS + ms.ox;
        if (rows_out || mx0 + TS <= 0 || mx0 >= ms.mw) return MK_OUT;
        return rows_in && mx0 >= 0 && mx0 + TS <= ms.mw && (t + 1) * TS <= w ? MK_IN : MK_EDGE;
    };
    auto mosaic_tile_in = [&](int t, f4 pre_[16]) {  // every offset lies inside the plane: (my0 + row) * mw + mx0 + column, in bytes
        const unsigned row_b = (unsigned)ms.mw * (unsigned)sizeof(PX);
        const unsigned o = ((unsigned)my0 + (unsigned)(lane >> 4)) * row_b + ((unsigned)(t * TS + ms.ox) + (unsigned)((lane & 15) << 2)) * (unsigned)sizeof(PX);
#pragma unroll
        for (int i = 0; i < 16; ++i) pre_[i] = __builtin_bit_cast(f4, __builtin_amdgcn_raw_buffer_load_b128(rs, o + (unsigned)(4 * i) * row_b, 0, 0));
    };
    auto gen_tile = [&](int c0, f4 pre[16]) {
        f4 v;
        const int c = c0 + ((lane & 15) << 2);
        v.x = mask_step(sd, c);
        v.y = mask_step(sd, c + 1);
        v.z = mask_step(sd, c + 2);
        v.w = mask_step(sd, c + 3);
#pragma unroll
        for (int i = 0; i < 16; ++i) pre[i] = v;
    };
    double iplus = 0.0;  // CImg.h:34906
    if (live)
        iplus = gen_mask     ? (double)mask_step(sd, w - 1)
                : gen_frame  ? (double)src_px<PX>(rs, true, reinterpret_cast<const unsigned*>(idx_rows)[(size_t)lane * pitch + (w - 1)])
                : gen_mosaic ? (double)src_px<PX>(rs, false, mosaic_offset<PX>(mosaic_row<PX>(ms, src_y0 + lane), mosaic_col<PX>(ms, w - 1, w)))
                : tile_outside(ntiles - 1) ? 0.0
                : tile_row0(ntiles - 1)    ? (double)row0[w - 1]
                             : (double)in[(size_t)line * pitch + (w - 1)];
    double v1 = 0, v2 = 0, v3 = 0;
    f4 pre[16];
// tile T into `pre`; a source-fused block gathers through the indices produced during the previous fetch, then produces the next
#define STITCH_X_FETCH(T)                                                      \
    do {                                                                       \
        if (gen_mask)                                                          \
            gen_tile((T) * TS, pre);                                           \
        else if constexpr (SRC) {                                              \
            if (tile_outside(T)) {                                             \
                pcls = 0;                                                      \
                _Pragma("unroll") for (int i_ = 0; i_ < 16; ++i_) pre[i_] = f4{0.f, 0.f, 0.f, 0.f}; \
            } else if (mosaic_kind(T) == MK_IN) {                              \
                pcls = 0;                                                      \
                mosaic_tile_in((T), pre);                                      \
            } else if (mosaic_kind(T) == MK_OUT) {                             \
                pcls = 0;                                                      \
                _Pragma("unroll") for (int i_ = 0; i_ < 16; ++i_) pre[i_] = f4{0.f, 0.f, 0.f, 0.f}; \
            } else                                                             \
                gather_tile(pre);                                              \
            if ((T) + 1 < ntiles) {                                            \
                if (gen_frame)                                                 \
                    index_tile((T) + 1);                                       \
                else if (mosaic_kind((T) + 1) == MK_EDGE)                      \
                    mosaic_indices<PX>(ms, ((T) + 1) * TS, lane, src_y0, w, nidx); \
            }                                                                  \
        } else if (tile_outside(T)) {                                          \
            _Pragma("unroll") for (int i_ = 0; i_ < 16; ++i_) pre[i_] = f4{0.f, 0.f, 0.f, 0.f}; \
        } else {                                                               \
            const bool r0_ = tile_row0(T);                                     \
            tile_load(r0_ ? row0 : ib, r0_ ? 0 : pitch, (T) * TS, lane, pre);  \
        }                                                                      \
    } while (0)
    if constexpr (SRC) {
        if (gen_frame)
            index_tile(0);
        else if (gen_mosaic && mosaic_kind(0) == MK_EDGE)
            mosaic_indices<PX>(ms, 0, lane, src_y0, w, nidx);
    }
    STITCH_X_FETCH(0);
    for (int t = 0; t < ntiles; ++t) {
        // Zeros in under a zero state: every product and sum of the recurrence is +0 again, the state stays as it is and the
        // tile would be recorded as all +0 -- recorded at once.  (In a stitch step the frame's canvas is empty left of the
        // frame: a third of the frame channels' tiles in config 2.)
        if (!CKPT && zt.flags && tile_outside(t) &&
            (t == 0 || __ballot(live && (__double_as_longlong(v1) | __double_as_longlong(v2) | __double_as_longlong(v3)) != 0) == 0)) {
            if (t + 1 < ntiles) STITCH_X_FETCH(t + 1);
            if (lane == 0) zt.flags[zt.index(plane, band_y0 / TS, t)] = 1;
            continue;
        }
        // a level without flags of T (level 2 of a batch), zeros in under a zero state: the tile of zeros is stored as it was
        // fetched (it was not loaded: G column flags), the sweep over it is skipped -- the state stays +0
        const bool zskip = !SRC && !CKPT && !zt.flags && tile_outside(t) &&
                           (t == 0 || __ballot(live && (__double_as_longlong(v1) | __double_as_longlong(v2) | __double_as_longlong(v3)) != 0) == 0);
        if constexpr (SRC)
            if (!gen_mask) src_finish<PX>(gen_frame, pre);
        tile_to_lds(tile, lane, pre);
        if constexpr (SRC) {
            if (pcls > 0) {  // the samples the bases did not deliver: the same element through the same conversion, over what the run left there
                __builtin_amdgcn_wave_barrier();
                if ((unsigned)lane < pcls && ppos < (unsigned)(TS * TP)) tile[ppos] = warped_px<PX>(raw_to_px<PX>(pval));
            }
        }
        if (t + 1 < ntiles) STITCH_X_FETCH(t + 1);
        __syncthreads();  // one wave per workgroup: orders the tile writes before the per-lane row reads
        float* row = tile + lane * TP;
        const int jmax = zskip ? 0 : min(TS, w - t * TS);
        if (t == 0) v1 = v2 = v3 = (double)row[0] / k.sumsq;  // CImg.h:34909
        if (CKPT && t > 0 && live) {
            double* c = ckpt + (size_t)(3 * t) * lines + line;
            c[0] = v1;
            c[lines] = v2;
            c[2 * lines] = v3;
        }
        const int jfull = jmax & ~15;
        unsigned nz = 0;  // OR of the bit patterns this lane stores: 0 <=> every sample is +0.0f
        for (int jb = 0; jb < jfull; jb += 16) {
            float xs[16];
#pragma unroll
            for (int q = 0; q < 4; ++q) *reinterpret_cast<f4*>(xs + 4 * q) = *reinterpret_cast<const f4*>(row + jb + 4 * q);
#pragma unroll
            for (int u = 0; u < 16; ++u) {
                double v0 = (double)xs[u];
                v0 += v1 * k.f1;
                v0 += v2 * k.f2;
                v0 += v3 * k.f3;
                xs[u] = (float)v0;
                nz |= __float_as_uint(xs[u]);
                v3 = v2;
                v2 = v1;
                v1 = v0;
            }
            if (!CKPT) {
#pragma unroll
                for (int q = 0; q < 4; ++q) *reinterpret_cast<f4*>(row + jb + 4 * q) = *reinterpret_cast<const f4*>(xs + 4 * q);
            }
        }
        for (int j = jfull; j < jmax; ++j) {  // ragged tail of the last tile, straight from LDS
            double v0 = (double)row[j];
            v0 += v1 * k.f1;
            v0 += v2 * k.f2;
            v0 += v3 * k.f3;
            const float f = (float)v0;
            if (!CKPT) row[j] = f;
            nz |= __float_as_uint(f);
            v3 = v2;
            v2 = v1;
            v1 = v0;
        }
        __syncthreads();
        if (zt.flags) {  // an all-(+0) tile is recorded instead of written: its consumers never read it (ZeroTiles)
            const bool zero = __ballot(live && nz != 0) == 0;  // rows past a partial last band hold whatever the fetch found: not asked
            if (lane == 0) zt.flags[zt.index(plane, band_y0 / TS, t)] = zero ? 1 : 0;
            if (zero) continue;
        }
        if (!CKPT) {
            if (nrows == TS)
                tile_store(ob, pitch, t * TS, lane, tile);
            else
                tile_store_rows(ob, pitch, t * TS, lane, tile, nrows);  // a partial last band must not touch the next plane's rows
        }
    }
    if (live) {
        state[line] = v1;
        state[lines + line] = v2;
        state[2 * lines + line] = v3;
        state[3 * lines + line] = iplus;
    }
}

#undef STITCH_X_FETCH

__device__ __forceinline__ void triggs(const VVK& k, double iplus, double& v1, double& v2, double& v3, float& first) {
    // CImg.h:34911-34922
    const double uplus = iplus / k.den, vplus = uplus / k.den, unp = v1 - uplus, unp1 = v2 - uplus, unp2 = v3 - uplus;
    const double n0 = (k.M[0] * unp + k.M[1] * unp1 + k.M[2] * unp2 + vplus) * k.sum;
    const double n1 = (k.M[3] * unp + k.M[4] * unp1 + k.M[5] * unp2 + vplus) * k.sum;
    const double n2 = (k.M[6] * unp + k.M[7] * unp1 + k.M[8] * unp2 + vplus) * k.sum;
    first = (float)n0;
    v3 = n2;
    v2 = n1;
    v1 = n0;
}

__global__ __launch_bounds__(64) void k_vv_x_bwd(float* __restrict__ data, int w, int pitch, long lines, VVK k,
                                                  const double* __restrict__ state, MaskL0 mk, Bands bd) {
    __shared__ __attribute__((aligned(16))) float tile[TS * TP];
    const int lane = threadIdx.x;
    const long blk = blockIdx.x, plane = bd.nr > 0 ? blk / bd.nr : 0;
    const int band_y0 = bd.nr > 0 ? (int)(blk % bd.nr) * TS : 0;
    const int nrows = bd.nr > 0 ? min(TS, bd.h - band_y0) : TS;
    const long line0 = bd.nr > 0 ? plane * bd.h + band_y0 : blk * TS, line = line0 + lane;
    float* side_row = nullptr;  // level-0 mask plane: row 0 of this block is also left in the side buffer
    // (as in k_vv_x_fwd: nothing to do where every line is a line of a mask plane that stands)
    if (mk.keep != nullptr && (bd.nr > 0 ? mask_stands(mk.keep, plane) : __all(line >= lines || mask_stands(mk.keep, line / mk.h)))) return;
    if (mk.enabled) {
        if (plane % 7 == 6) {
            if (band_y0 >= TS) return;
            side_row = mk.side + (size_t)(plane / 7) * pitch;
        }
    }
    float* base = data + (size_t)line0 * pitch;
    const int ntiles = (w + TS - 1) / TS;
    const bool live = lane < nrows && line < lines;
    double v1 = 0, v2 = 0, v3 = 0, iplus = 0;
    if (live) {
        v1 = state[line];
        v2 = state[lines + line];
        v3 = state[2 * lines + line];
        iplus = state[3 * lines + line];
    }
    float first;
    triggs(k, iplus, v1, v2, v3, first);
    f4 pre[16];
    tile_load(base, pitch, (ntiles - 1) * TS, lane, pre);
    for (int t = ntiles - 1; t >= 0; --t) {
        tile_to_lds(tile, lane, pre);
        if (t > 0) tile_load(base, pitch, (t - 1) * TS, lane, pre);
        __syncthreads();
        float* row = tile + lane * TP;
        int jtop = min(TS, w - t * TS);  // samples [0,jtop) of this tile, processed from jtop-1 down to 0
        if (t == ntiles - 1) {
            row[jtop - 1] = first;  // sample N-1 takes the boundary value (CImg.h:34920)
            --jtop;
        }
        // whole 16-sample groups below jtop, then the ragged top group first (descending order overall)
        const int jfull = jtop & ~15;
        if (jtop > jfull) {
            for (int j = jtop - 1; j >= jfull; --j) {
                double v0 = (double)row[j];
                v0 *= k.sum;
                v0 += v1 * k.f1;
                v0 += v2 * k.f2;
                v0 += v3 * k.f3;
                row[j] = (float)v0;
                v3 = v2;
                v2 = v1;
                v1 = v0;
            }
        }
        for (int jb = jfull - 16; jb >= 0; jb -= 16) {
            float xs[16];
#pragma unroll
            for (int q = 0; q < 4; ++q) *reinterpret_cast<f4*>(xs + 4 * q) = *reinterpret_cast<const f4*>(row + jb + 4 * q);
#pragma unroll
            for (int u = 15; u >= 0; --u) {
                double v0 = (double)xs[u];
                v0 *= k.sum;
                v0 += v1 * k.f1;
                v0 += v2 * k.f2;
                v0 += v3 * k.f3;
                xs[u] = (float)v0;
                v3 = v2;
                v2 = v1;
                v1 = v0;
            }
#pragma unroll
            for (int q = 0; q < 4; ++q) *reinterpret_cast<f4*>(row + jb + 4 * q) = *reinterpret_cast<const f4*>(xs + 4 * q);
        }
        __syncthreads();
        if (nrows == TS)
            tile_store(base, pitch, t * TS, lane, tile);
        else
            tile_store_rows(base, pitch, t * TS, lane, tile, nrows);
        if (side_row && lane < 16) *reinterpret_cast<f4*>(side_row + t * TS + (lane << 2)) = *reinterpret_cast<const f4*>(tile + (lane << 2));
    }
}

// overlap weights of the moving-average resize (used by the fused anticausal pass and by k_decimate)
struct Taps {  // up to 4 overlaps per output sample (3 when n_src = 2*n_dst+1, 2 when n_src = 2*n_dst)
    int s0, n;
    float d[4];
};
__device__ __forceinline__ Taps make_taps(int t, int n_src, int n_dst) {
    Taps r;
    const long long pos = (long long)t * n_src;
    int s = (int)(pos / n_dst);
    int c_left = (int)((long long)(s + 1) * n_dst - pos);
    int remaining = n_src;
    r.s0 = s;
    r.n = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int d = remaining < c_left ? remaining : c_left;
        r.d[i] = (float)(unsigned)d;
        if (d > 0) r.n = i + 1;
        remaining -= d;
        c_left = n_dst;
    }
    return r;
}

// y pass: two adjacent columns per work-item (8-byte accesses: a wavefront moves 512 contiguous bytes of one row
// per step, and the two independent recurrences interleave in the fp64 pipe).  The recurrence is cheap next to an
// HBM round trip, so rows are fetched far ahead of their use: YST stages of YCH rows rotate through registers
// (YCH*(YST-1) = 24 rows in flight per wavefront while one chunk computes).  In place.
// grid = (ceil(pitch/128), planes); pitch is a multiple of 64, a last half-empty block is masked off.
constexpr int YST = 4;

// Calls f(y, value) for rows y_begin, y_begin +/- 1, ... (count rows), loading each row's value long before.
typedef float f2 __attribute__((ext_vector_type(2)));
// One row of a plane through a raw buffer descriptor (wave-uniform, SGPRs): the lane's column as a 32-bit byte offset in a
// VGPR, the row's byte offset in an SGPR -- no vector address arithmetic per row.  Planes are below 4 GB.
__device__ __forceinline__ f2 ld_row2(__amdgpu_buffer_rsrc_t rs, unsigned xb, unsigned row_b) {
    return __builtin_bit_cast(f2, __builtin_amdgcn_raw_buffer_load_b64(rs, xb, row_b, 0));
}
__device__ __forceinline__ void st_row1(__amdgpu_buffer_rsrc_t rs, unsigned xb, unsigned row_b, float v) {
    __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(v), rs, xb, row_b, 0);
}
template <bool DOWN, typename V = f2, typename F>
__device__ __forceinline__ void stream_rows(const float* __restrict__ p, int pitch, int y_begin, int count, F&& f) {
    V buf[YST][YCH];
    // row index is clamped instead of predicated: the tail re-reads the last row, the loop body stays branch-free
    auto ld = [&](int i) {
        const int ic = i < count ? i : count - 1;
        return *reinterpret_cast<const V*>(p + (size_t)(DOWN ? y_begin + ic : y_begin - ic) * pitch);
    };
#pragma unroll
    for (int s = 0; s < YST - 1; ++s)
#pragma unroll
        for (int u = 0; u < YCH; ++u) buf[s][u] = ld(s * YCH + u);
    int c0 = 0;
    for (; c0 + YST * YCH <= count; c0 += YST * YCH) {  // whole groups: no predicates at all
#pragma unroll
        for (int s = 0; s < YST; ++s) {
#pragma unroll
            for (int u = 0; u < YCH; ++u) buf[(s + YST - 1) % YST][u] = ld(c0 + (s + YST - 1) * YCH + u);
#pragma unroll
            for (int u = 0; u < YCH; ++u) {
                const int i = c0 + s * YCH + u;
                f(DOWN ? y_begin + i : y_begin - i, buf[s][u]);
            }
        }
    }
    if (c0 < count) {  // ragged last group
#pragma unroll
        for (int s = 0; s < YST; ++s) {
#pragma unroll
            for (int u = 0; u < YCH; ++u) buf[(s + YST - 1) % YST][u] = ld(c0 + (s + YST - 1) * YCH + u);
#pragma unroll
            for (int u = 0; u < YCH; ++u) {
                const int i = c0 + s * YCH + u;
                if (i < count) f(DOWN ? y_begin + i : y_begin - i, buf[s][u]);
            }
        }
    }
}

// recurrence state of the two columns a work-item owns
struct Y2 {
    double a1, a2, a3, b1, b2, b3;
};
__device__ __forceinline__ f2 y2_step_fwd(Y2& s, const VVK& k, f2 x) {
    double a0 = (double)x.x, b0 = (double)x.y;
    a0 += s.a1 * k.f1;
    b0 += s.b1 * k.f1;
    a0 += s.a2 * k.f2;
    b0 += s.b2 * k.f2;
    a0 += s.a3 * k.f3;
    b0 += s.b3 * k.f3;
    s.a3 = s.a2;
    s.a2 = s.a1;
    s.a1 = a0;
    s.b3 = s.b2;
    s.b2 = s.b1;
    s.b1 = b0;
    f2 r;
    r.x = (float)a0;
    r.y = (float)b0;
    return r;
}
__device__ __forceinline__ f2 y2_step_bwd(Y2& s, const VVK& k, f2 x) {
    double a0 = (double)x.x, b0 = (double)x.y;
    a0 *= k.sum;
    b0 *= k.sum;
    a0 += s.a1 * k.f1;
    b0 += s.b1 * k.f1;
    a0 += s.a2 * k.f2;
    b0 += s.b2 * k.f2;
    a0 += s.a3 * k.f3;
    b0 += s.b3 * k.f3;
    s.a3 = s.a2;
    s.a2 = s.a1;
    s.a1 = a0;
    s.b3 = s.b2;
    s.b2 = s.b1;
    s.b1 = b0;
    f2 r;
    r.x = (float)a0;
    r.y = (float)b0;
    return r;
}
// state buffer: [4][planes][pitch] doubles -- v1, v2, v3, iplus of every column
__device__ __forceinline__ size_t ystate_index(int plane, int pitch, int x) { return (size_t)plane * pitch + x; }

// resume (one pair split into row bands over several GPUs): the rows above this band belong to another rank, which left its
// recurrence state (v1, v2, v3 per column, [3][planes][pitch]) behind: the sweep continues from it instead of starting at
// the image's first row.  The state this kernel leaves is exactly what the rank below resumes from.
// XCH (a row band of a split pair whose state crosses ranks in column chunks, stitch_band_reduce_y_fwd_cols): the launch covers
// columns x_base .. x_base + 128 * gridDim.x - 1, and `state` / `resume` are the CHUNK's own arrays, [k][planes][128 * gridDim.x].
template <bool XCH = false>
__global__ __launch_bounds__(64) void k_vv_y_fwd(float* __restrict__ data, int h, int pitch, size_t ps, VVK k,
                                                  double* __restrict__ state, MaskL0 mk, const double* __restrict__ resume, int x_base = 0) {
    const int xl = (blockIdx.x * WAVE + threadIdx.x) * 2, x = XCH ? xl + x_base : xl;
    if (x >= pitch || mask_stands(mk.keep, blockIdx.y)) return;  // (a mask plane that stands: nothing is touched)
    const int sp = XCH ? (int)gridDim.x * YCOLS : pitch, sx = XCH ? xl : x;  // the state arrays' pitch and this lane's place in them
    float* p = data + blockIdx.y * ps + x;
    // level-0 mask plane: every input row is the one x-blurred row kept in the side buffer (row stride 0)
    const bool side = mk.enabled && (blockIdx.y % 7 == 6);
    const float* src = side ? mk.side + (size_t)(blockIdx.y / 7) * pitch + x : p;
    const int spitch = side ? 0 : pitch;
    const f2 last = *reinterpret_cast<const f2*>(src + (size_t)(h - 1) * spitch);  // iplus, read before the sweep
    const f2 x0 = *reinterpret_cast<const f2*>(src);
    Y2 s;
    s.a1 = s.a2 = s.a3 = (double)x0.x / k.sumsq;
    s.b1 = s.b2 = s.b3 = (double)x0.y / k.sumsq;
    if (resume) {
        const size_t n = (size_t)gridDim.y * sp, i = ystate_index(blockIdx.y, sp, sx);
        s.a1 = resume[i], s.b1 = resume[i + 1];
        s.a2 = resume[n + i], s.b2 = resume[n + i + 1];
        s.a3 = resume[2 * n + i], s.b3 = resume[2 * n + i + 1];
    }
    stream_rows<true>(src, spitch, 0, h, [&](int y, f2 xv) {
        *reinterpret_cast<f2*>(p + (size_t)y * pitch) = y2_step_fwd(s, k, xv);
    });
    const size_t n = (size_t)gridDim.y * sp, i = ystate_index(blockIdx.y, sp, sx);
    state[i] = s.a1;
    state[i + 1] = s.b1;
    state[n + i] = s.a2;
    state[n + i + 1] = s.b2;
    state[2 * n + i] = s.a3;
    state[2 * n + i + 1] = s.b3;
    state[3 * n + i] = (double)last.x;
    state[3 * n + i + 1] = (double)last.y;
}

// The same sweep with ONE column per work-item, for launches that leave SIMDs idle (a single pair: 7 planes x 6144 columns are
// 336 wavefronts of two columns on 1024 SIMDs).  A wavefront alone on its SIMD issues one vector instruction every ~6 cycles
// (profiles/r03_experiments/valu_issue_rates.txt), so a row costs its instruction count: two interleaved columns are twice the
// instructions per row of one, and there are twice as many wavefronts to spread.
__global__ __launch_bounds__(64) void k_vv_y_fwd1(float* __restrict__ data, int h, int pitch, size_t ps, VVK k,
                                                   double* __restrict__ state, MaskL0 mk, const double* __restrict__ resume) {
    const int x = blockIdx.x * WAVE + threadIdx.x;  // pitch is a multiple of 64
    if (mask_stands(mk.keep, blockIdx.y)) return;  // (a mask plane that stands: nothing is touched)
    float* p = data + blockIdx.y * ps + x;
    const bool side = mk.enabled && (blockIdx.y % 7 == 6);
    const float* src = side ? mk.side + (size_t)(blockIdx.y / 7) * pitch + x : p;
    const int spitch = side ? 0 : pitch;
    const float last = src[(size_t)(h - 1) * spitch];
    const float x0 = src[0];
    double v1, v2, v3;
    v1 = v2 = v3 = (double)x0 / k.sumsq;
    const size_t n = (size_t)gridDim.y * pitch, i = ystate_index(blockIdx.y, pitch, x);
    if (resume) {
        v1 = resume[i];
        v2 = resume[n + i];
        v3 = resume[2 * n + i];
    }
    stream_rows<true, float>(src, spitch, 0, h, [&](int y, float xv) {
        double v0 = (double)xv;
        v0 += v1 * k.f1;
        v0 += v2 * k.f2;
        v0 += v3 * k.f3;
        v3 = v2;
        v2 = v1;
        v1 = v0;
        p[(size_t)y * pitch] = (float)v0;
    });
    state[i] = v1;
    state[n + i] = v2;
    state[2 * n + i] = v3;
    state[3 * n + i] = (double)last;
}

__device__ __forceinline__ void y2_triggs(const VVK& k, const double* __restrict__ state, size_t n, size_t i, Y2& s, f2& first) {
    float fa, fb;
    s.a1 = state[i];
    s.a2 = state[n + i];
    s.a3 = state[2 * n + i];
    triggs(k, state[3 * n + i], s.a1, s.a2, s.a3, fa);
    s.b1 = state[i + 1];
    s.b2 = state[n + i + 1];
    s.b3 = state[2 * n + i + 1];
    triggs(k, state[3 * n + i + 1], s.b1, s.b2, s.b3, fb);
    first.x = fa;
    first.y = fb;
}

// Anticausal y pass, stand-alone (odd source widths): stores the blurred rows in place.
// resume / state_out: as in k_vv_y_fwd, for the band BELOW (the anticausal sweep runs bottom-up): with `resume` the last row of
// this band is an ordinary step from the state the rank below left after its first row, not the Triggs boundary value.
__device__ __forceinline__ void y2_load(const double* __restrict__ st, size_t n, size_t i, Y2& s) {
    s.a1 = st[i], s.b1 = st[i + 1];
    s.a2 = st[n + i], s.b2 = st[n + i + 1];
    s.a3 = st[2 * n + i], s.b3 = st[2 * n + i + 1];
}
__device__ __forceinline__ void y2_store(double* __restrict__ st, size_t n, size_t i, const Y2& s) {
    st[i] = s.a1, st[i + 1] = s.b1;
    st[n + i] = s.a2, st[n + i + 1] = s.b2;
    st[2 * n + i] = s.a3, st[2 * n + i + 1] = s.b3;
}
__global__ __launch_bounds__(64) void k_vv_y_bwd(float* __restrict__ data, int h, int pitch, size_t ps, VVK k,
                                                  const double* __restrict__ state, const double* __restrict__ resume,
                                                  double* __restrict__ state_out) {
    const int x = (blockIdx.x * WAVE + threadIdx.x) * 2;
    if (x >= pitch) return;
    float* p = data + blockIdx.y * ps + x;
    const size_t n = (size_t)gridDim.y * pitch, i = ystate_index(blockIdx.y, pitch, x);
    Y2 s;
    if (resume) {
        y2_load(resume, n, i, s);
        stream_rows<false>(p, pitch, h - 1, h, [&](int y, f2 xv) {
            *reinterpret_cast<f2*>(p + (size_t)y * pitch) = y2_step_bwd(s, k, xv);
        });
    } else {
        f2 first;
        y2_triggs(k, state, n, i, s, first);
        *reinterpret_cast<f2*>(p + (size_t)(h - 1) * pitch) = first;
        stream_rows<false>(p, pitch, h - 2, h - 1, [&](int y, f2 xv) {
            *reinterpret_cast<f2*>(p + (size_t)y * pitch) = y2_step_bwd(s, k, xv);
        });
    }
    if (state_out) y2_store(state_out, n, i, s);
}

// Anticausal y pass fused with the decimation (even source width): the blurred level is never written.
// A lone wavefront is bound by its own instruction issue (recurrence + IEEE divides), so the work is split over
// the two wavefronts of a workgroup:
//   wave 0 (producer)  runs the recurrence for 128 columns (two per lane), rows bottom-up, and drops each blurred
//                      row into an LDS ring (two slots of YCH rows);
//   wave 1 (consumer)  owns one column PAIR per lane: x-decimates each row (columns 2t, 2t+1, both overlaps = w2,
//                      CImg.h:29542-29555: acc = 0; acc += s0*d; acc += s1*d; acc /= W), keeps the last two
//                      x-decimated rows, and for every output row y-decimates (CImg.h:29557-29575: accumulation in
//                      INCREASING source row although rows arrive bottom-up; overlaps {h2,h2} for even h,
//                      {h2-t, h2, t+1} for odd h) and stores 256 bytes of the next pyramid level.
// One workgroup barrier per YCH rows hands a slot over.  rc = h-1-y counts rows in processing order.
// ROWZ: the zero-tile flag is looked up per row instead of per chunk of YCH rows (heights that are not a multiple of YCH: a
// chunk, counted from the bottom row, then straddles 64-row bands).
// NST: stages of YCH rows rotating through the producer's registers, i.e. YCH * (NST - 1) rows in flight (24 with NST = YST).
// Measured with one pair in flight (a launch's time = the length of a wavefront's chain of rows): 56 rows in flight (NST = 8) change
// nothing -- 372 against 371 us at 6144 x 4096 -- and neither does a causal sweep that moves 64 x 64 tiles through LDS with
// 16-byte accesses instead of one load and one store per row (298 against 275 us): the y sweeps' 68-90 ns per row against the x
// sweeps' 41 ns per sample are not the memory round trip.
// ZT = false (launches without zero-tile flags): the producer's loads and the consumer's stores take a raw buffer descriptor over
// the plane, the lane's column as a 32-bit offset and the row's byte offset in an SGPR carried from row to row.  With the per-lane
// 64-bit address p + (flag ? h-1 : y) * pitch a row cost about ten scalar and four vector instructions of address arithmetic,
// and with one wavefront per SIMD (one pair in flight) every instruction is an issue slot of 4-5 cycles: 367 -> 315 us at
// 6144 x 4096, 29 -> 26 us at 540 x 263.  (The same change in the row-streaming causal sweeps k_vv_y_fwd / k_vv_y_fwd1 gained
// nothing below 3072 x 2048 and lost 20 % at 6144 x 4096, where that sweep is bound by the bytes it moves, not by issue: kept
// on flat addresses.)
// ODD (source width w = 2 * w2 + 1): output column t overlaps source columns 2t, 2t+1, 2t+2 with weights w2 - t, w2, t + 1
// (make_taps; CImg.h:29542-29555).  The third column is the next lane's first, so a workgroup advances by 63 output columns
// instead of 64 -- consecutive workgroups overlap by two source columns, whose recurrence both run -- and lane 63 only feeds
// its neighbour; its 128 columns then lie in up to three tiles of the zero-tile flags.
// XCH (even widths; stitch_band_reduce_y_bwd_cols): the launch covers source columns x_base .. x_base + 128 * gridDim.x - 1 and
// `state` / `resume` / `state_out` are the chunk's own arrays, [k][planes][128 * gridDim.x] (as k_vv_y_fwd<true>).
// fill_l0 (a plan's fused level 0 with the implicit mask; k_vv_xbyf, Wavefront::mask_l0 == 2): on the planes y % 7 == 6 a flagged tile was
// not all +0 but a repetition of the plane's row 0, which is always stored: the row a flagged lane re-reads IS that row, and the lane keeps
// what it read instead of taking zeros (no register holds the fill values: the ROWZ instances sit at 127 of 128 VGPRs for four wavefronts).
// The same holds for the mask plane of a fused level >= 1 that has row-repeat flags (mask_rows, k_compose.inc).
// mr (even widths and heights, whole-width launches with T flags): row-repeat flags of the mask plane of the level being PRODUCED, which
// the consumer wavefront of the mask planes' workgroups writes while it stores that plane lazily (see the consumer loop).
template <bool ROWZ = false, int NST = YST, bool ZT = true, bool ODD = false, bool XCH = false>
__global__ __launch_bounds__(128) void k_vv_y_bwd_dec(const float* __restrict__ data, int w, int h, int pitch, size_t ps,
                                                      VVK k, const double* __restrict__ state, float* __restrict__ dst,
                                                      int w2, int h2, int dpitch, size_t dps, ZeroTiles zt,
                                                      const double* __restrict__ resume, double* __restrict__ state_out, int wh, int wh2,
                                                      int x_base = 0, int fill_l0 = 0, ZeroTiles gz = ZeroTiles{}, ZeroTiles mr = ZeroTiles{},
                                                      const unsigned* __restrict__ keep = nullptr) {
    static_assert(!(XCH && ODD), "column chunks: even widths");
    // keep (mask_stands): the workgroups of a mask plane that stands return before they touch anything -- plane 6 of G_{l+1}, its `mr`
    // bytes and whatever the memory holds where they say "not stored" are an earlier call's, left bit for bit (a mask plane has neither
    // G column flags nor a state_out)
    if (mask_stands(keep, blockIdx.y)) return;
    // wh, wh2: the heights the decimation's overlap weights are taken from (CImg.h:29557-29575 weights by the LEVEL's
    // heights): h, h2 for a whole level; for a row band of a split pair the level's, not the band's (the quotient is the same
    // number, but (x*32 + y*32)/64 and (x*96 + y*96)/192 round differently)
    __shared__ __attribute__((aligned(16))) float ring[2][YCH][YCOLS];
    // the wave id is wave-uniform, but anything derived from threadIdx is a lane value to the compiler: readfirstlane
    // keeps the producer/consumer role branches scalar
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
    const int nchunks = (h + YCH - 1) / YCH;
    constexpr int ADV = ODD ? WAVE - 1 : WAVE;      // output columns a workgroup advances by
    const int xl = (blockIdx.x * ADV + lane) * 2, x = XCH ? xl + x_base : xl;  // first of this lane's two columns
    const bool col_live = x < pitch;
    const int sp = XCH ? (int)gridDim.x * YCOLS : pitch, sx = XCH ? xl : x;  // the state arrays' pitch and this lane's place in them
    const float* p = data + blockIdx.y * ps + (col_live ? x : 0);
    Y2 s{};
    f2 first{};
    f2 buf[NST][YCH];
    // zero-tile flags of this lane's 64-column tile, one bit per 64-row band, gathered once before the walk starts (the
    // host enables the flags only up to 256 bands); the row loop then only tests a bit
    unsigned long long zm[4] = {0, 0, 0, 0};
    const bool zt_on = ZT && zt.flags != nullptr;
    if (zt_on) {
        // a wavefront's 128 columns lie in two tiles (lanes 0..31 / 32..63) -- three when the workgroups advance by 126 columns
        // (ODD) --: lane i fetches the flag of band g*64+i of each of them (the bands of a tile column are contiguous bytes), a
        // ballot turns 64 flags into a mask, and every lane keeps the mask of the tile its two columns are in
        const int tA = ((XCH ? x_base : 0) + blockIdx.x * ADV * 2) >> 6, mine = (x >> 6) - tA;
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            if (g * 64 < zt.NR) {  // wave-uniform
                const int band = g * 64 + lane;
                const bool inb = band < zt.NR;
                const unsigned char fa = inb && tA < zt.NC ? zt.flags[zt.index(blockIdx.y, band, tA)] : 0;
                const unsigned char fb = inb && tA + 1 < zt.NC ? zt.flags[zt.index(blockIdx.y, band, tA + 1)] : 0;
                const unsigned long long mA = __ballot(fa != 0), mB = __ballot(fb != 0);
                unsigned long long m = mine == 0 ? mA : mB;
                if constexpr (ODD) {
                    const unsigned char fc = inb && tA + 2 < zt.NC ? zt.flags[zt.index(blockIdx.y, band, tA + 2)] : 0;
                    const unsigned long long mC = __ballot(fc != 0);
                    m = mine == 2 ? mC : m;
                }
                zm[g] = (x >> 6) < zt.NC ? m : 0ull;  // columns past the last tile (dead lanes of the last workgroup) read their own rows
            }
        }
    }
    // When the height is a multiple of YCH a chunk of YCH rows (counted from the bottom) never straddles a 64-row band, so the
    // flag is looked up once per chunk; otherwise per row (ROWZ).  The loads stay branch-free (the prefetch stream must remain
    // one straight run of loads): a lane whose tile is flagged re-reads one fixed row of its column -- a cache hit after the
    // first time, no HBM traffic -- and discards it.
    auto zero_at = [&](int rc) {
        if (!zt_on) return false;
        const int r = rc < h ? rc : h - 1, b = (h - 1 - r) >> 6, g = b >> 6;
        const unsigned long long m = g == 0 ? zm[0] : g == 1 ? zm[1] : g == 2 ? zm[2] : zm[3];
        return ((m >> (b & 63)) & 1) != 0;
    };
    auto chunk_zero = [&](int chunk) { return ROWZ ? false : zero_at(chunk * YCH); };
    // ZT = false: rows h-1, h-2, ... 0 are loaded strictly in this order (rc counts them); past row 0 the offset stays there
    const bool fill_on = ZT && zt_on && fill_l0 != 0 && blockIdx.y % 7 == 6;  // workgroup-uniform
    const int dummy = fill_on ? 0 : h - 1;  // the row a flagged lane re-reads: on a fill plane the very row it stands for
    const __amdgpu_buffer_rsrc_t rsp = plane_rsrc(data + blockIdx.y * ps, ps);
    const unsigned xo = (col_live ? (unsigned)x : 0u) * 4u, pitch_b = (unsigned)pitch * 4u;
    unsigned next = (unsigned)(h - 1) * pitch_b;  // byte offset of the next row to load
    int issued = 0;
    auto ld = [&](int rc, bool zero) {
        if constexpr (!ZT) {
            const f2 v = ld_row2(rsp, xo, next);
            if (++issued < h) next -= pitch_b;
            return v;
        } else {
            if (ROWZ) zero = zero_at(rc);
            const int r = rc < h ? rc : h - 1, y = h - 1 - r;
            const f2 v = *reinterpret_cast<const f2*>(p + (size_t)(zero ? dummy : y) * pitch);
            // (as a mask on the bits, not a select between two values: 131 -> 124 VGPRs, ROWZ 127 -> 118)
            const unsigned keep = (zero && !fill_on) ? 0u : ~0u;
            return f2{__uint_as_float(__float_as_uint(v.x) & keep), __uint_as_float(__float_as_uint(v.y) & keep)};
        }
    };
    if (wave == 0) {
        if (col_live) {
            if (resume)
                y2_load(resume, (size_t)gridDim.y * sp, ystate_index(blockIdx.y, sp, sx), s);
            else
                y2_triggs(k, state, (size_t)gridDim.y * sp, ystate_index(blockIdx.y, sp, sx), s, first);
        }
    }
    // A workgroup whose columns are flagged zero in EVERY band and whose sweep starts from a +0 state (the canvas left of the warped frame,
    // right of the mosaic: a third of six planes at config 2) has nothing to compute: every product and sum of the recurrence is +0 again
    // (+0 plus a zero of either sign is +0), every x- and y-decimated sum and quotient +0 -- it writes the zeros of the next level and ends.
    // (Until round 4 it ran the whole instruction stream on re-read zeros: this kernel is bound by instruction issue, not by bytes.)
    if (ZT && zt_on) {
        __shared__ int s_allz;
        bool mine_all = true;
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            if (g * 64 < zt.NR) {  // wave-uniform
                const int bits = min(64, zt.NR - g * 64);
                const unsigned long long full = bits == 64 ? ~0ull : ((1ull << bits) - 1ull);
                mine_all = mine_all && (zm[g] & full) == full;
            }
        }
        if (wave == 0) {
            const unsigned long long sb = (unsigned long long)__double_as_longlong(s.a1) | (unsigned long long)__double_as_longlong(s.a2) |
                                          (unsigned long long)__double_as_longlong(s.a3) | (unsigned long long)__double_as_longlong(s.b1) |
                                          (unsigned long long)__double_as_longlong(s.b2) | (unsigned long long)__double_as_longlong(s.b3) |
                                          (unsigned long long)(__float_as_uint(first.x) | __float_as_uint(first.y));
            const bool allz0 = __all(mine_all && sb == 0ull) && !fill_on;  // (on a fill plane a flag stands for row 0, not for zeros)
            if (lane == 0) s_allz = allz0 ? 1 : 0;
        }
        // G column flags of the level being produced (even, whole-width launches only: a workgroup's 64 output columns are then ONE
        // tile column, blockIdx.x): meanwhile the consumer wavefront asks the same question of the two neighbouring workgroups -- their
        // input tiles flagged in every band, their y state and Triggs value +0 -- since the zeros are left unstored only where both
        // neighbours are zero as well (see g_cols; the plane's edge counts as a zero neighbour, a fill plane never qualifies, and neither
        // does a workgroup whose second input tile lies past the level's last one: not here, tN + 1 < zt.NC, and not for itself, since
        // zm is 0 on those dead lanes).
        const bool gz_on = !ODD && !XCH && gz.flags != nullptr;  // workgroup-uniform
        __shared__ int s_nbz;
        if (gz_on && wave == 1) {
            bool ok = !fill_on && blockIdx.y % 7 != 6;  // (the mask plane has no flags: the collapse reads it as it stands)
            for (int side = -1; side <= 1; side += 2) {
                const int nb = (int)blockIdx.x + side, tN = 2 * nb;
                if (nb < 0 || nb >= gz.NC) continue;  // workgroup-uniform
                bool flagged = tN + 1 < zt.NC;
                for (int g = 0; g < 4 && flagged; ++g) {
                    if (g * 64 < zt.NR) {
                        const int band = g * 64 + lane;
                        const bool inb = band < zt.NR;
                        const unsigned char fa = inb ? zt.flags[zt.index(blockIdx.y, band, tN)] : 1;
                        const unsigned char fb = inb ? zt.flags[zt.index(blockIdx.y, band, tN + 1)] : 1;
                        flagged = __all(fa != 0 && fb != 0);
                    }
                }
                unsigned long long sn = 0ull;
                const int xn = (nb * WAVE + lane) * 2;
                if (flagged && xn < pitch) {
                    Y2 q;
                    f2 qf;
                    y2_triggs(k, state, (size_t)gridDim.y * sp, ystate_index(blockIdx.y, sp, xn), q, qf);
                    sn = (unsigned long long)__double_as_longlong(q.a1) | (unsigned long long)__double_as_longlong(q.a2) |
                         (unsigned long long)__double_as_longlong(q.a3) | (unsigned long long)__double_as_longlong(q.b1) |
                         (unsigned long long)__double_as_longlong(q.b2) | (unsigned long long)__double_as_longlong(q.b3) |
                         (unsigned long long)(__float_as_uint(qf.x) | __float_as_uint(qf.y));
                }
                ok = ok && flagged && __all(sn == 0ull);
            }
            if (lane == 0) s_nbz = ok ? 1 : 0;
        }
        __syncthreads();
        const bool g_skip = gz_on && s_allz != 0 && s_nbz != 0;  // workgroup-uniform
        if (gz_on && threadIdx.x == 0 && (int)blockIdx.x < gz.NC) gz.flags[gz.index(blockIdx.y, 0, blockIdx.x)] = g_skip ? 1 : 0;  // every byte, every call
        if (s_allz != 0) {  // workgroup-uniform
            if (wave == 1) {
                const int tx_ = blockIdx.x * ADV + lane + (XCH ? x_base / 2 : 0);
                if (!g_skip && tx_ < w2 && (!ODD || lane < WAVE - 1)) {
                    float* dc = dst + blockIdx.y * dps + tx_;
                    for (int t = 0; t < h2; ++t) dc[(size_t)t * dpitch] = 0.f;
                }
            } else if (state_out && col_live)
                y2_store(state_out, (size_t)gridDim.y * sp, ystate_index(blockIdx.y, sp, sx), s);
            return;
        }
    }
    if (wave == 0) {
#pragma unroll
        for (int st = 0; st < NST - 1; ++st) {
            const bool z = chunk_zero(st);
#pragma unroll
            for (int u = 0; u < YCH; ++u) buf[st][u] = ld(st * YCH + u, z);
        }
    }
    // consumer state: this lane's output column t_x = x/2
    const float fsx = (float)(unsigned)w2, fw = (float)(unsigned)w, fh = (float)(unsigned)wh, fsy = (float)(unsigned)wh2;
    const bool h_odd = (h & 1) != 0;
    const int tx = blockIdx.x * ADV + lane + (XCH ? x_base / 2 : 0);
    float* dcol = dst + blockIdx.y * dps + tx;
    const __amdgpu_buffer_rsrc_t rdst = plane_rsrc(dst + blockIdx.y * dps, dps);  // ZT = false: scalar row offset + this lane's column
    const bool dst_live = tx < w2 && (!ODD || lane < WAVE - 1);
    const float od0 = (float)(unsigned)(w2 - min(tx, w2)), od2 = (float)(unsigned)(tx + 1);  // ODD: the outer two overlap weights
    auto st_out = [&](int t, float v) {
        if constexpr (!ZT)
            st_row1(rdst, (unsigned)tx * 4u, (unsigned)t * (unsigned)dpitch * 4u, v);
        else
            dcol[(size_t)t * dpitch] = v;
    };
    float Xp1 = 0.f, Xp2 = 0.f;  // x-decimated rows y+1 and y+2 (previous two rows in processing order)

    // The two roles run separate loops (same trip count, one barrier per chunk each): in one loop body the producer's 64
    // registers of prefetched rows would stay allocated across the consumer's code.
    if (wave == 0) {
        for (int j0 = 0; j0 <= nchunks; j0 += NST) {
#pragma unroll
            for (int st = 0; st < NST; ++st) {
                const int j = j0 + st;
                const bool z = chunk_zero(j + NST - 1);
#pragma unroll
                for (int u = 0; u < YCH; ++u) buf[(st + NST - 1) % NST][u] = ld((j + NST - 1) * YCH + u, z);
                if (j < nchunks) {
                    const int live = min(YCH, h - j * YCH);  // rows of this chunk that exist (wave-uniform)
                    if (live == YCH) {
#pragma unroll
                        for (int u = 0; u < YCH; ++u) {
                            const int rc = j * YCH + u;
                            // sample h-1 takes the Triggs boundary value (CImg.h:34920)
                            const f2 o = (rc == 0 && !resume) ? first : y2_step_bwd(s, k, buf[st][u]);
                            *reinterpret_cast<f2*>(&ring[st & 1][u][2 * lane]) = o;
                        }
                    } else {
                        // the partial last chunk (heights that are not a multiple of YCH): rows past the image are NOT stepped -- the
                        // state this sweep leaves (state_out: the band above resumes from it) is the state after row 0; the ring's
                        // slots of those rows keep whatever they held (the consumer computes from them and never stores)
#pragma unroll
                        for (int u = 0; u < YCH; ++u) {
                            const int rc = j * YCH + u;
                            if (u < live) {
                                const f2 o = (rc == 0 && !resume) ? first : y2_step_bwd(s, k, buf[st][u]);
                                *reinterpret_cast<f2*>(&ring[st & 1][u][2 * lane]) = o;
                            }
                        }
                    }
                }
                __syncthreads();
            }
        }
    } else {
        // Row-repeat flags of the mask plane of the level being produced (mask_rows; even widths and heights, whole-width launches: a
        // workgroup's 64 output columns are ONE tile column).  The sweep walks bottom-up and cannot know row 0 in advance, so the consumer
        // stores lazily: it keeps the value of the current run of equal rows per lane and the run's top (first met) row; an output row
        // that equals the run in every live lane is not stored; a row that differs first stores the rows the run skipped, then starts a
        // new run.  Behind row 0 the last run is rows 0 .. run_top: band 0's rows are stored, a band the run covers whole is flagged,
        // a band it covers in part is stored as far as the run goes, and every byte is written.  Rows that never repeat are each
        // stored once, as without the flags.  Only the mask planes' workgroups take this form of the loop (workgroup-uniform).
#ifdef STITCH_NO_MASK_ROWS
        const bool mr_on = false;
#else
        const bool mr_on = ZT && !ODD && !XCH && mr.flags != nullptr && blockIdx.y % 7 == 6 && !h_odd;
#endif
        float runv = 0.f;
        int run_top = -1;
        auto consume = [&](auto MR) {
            for (int j0 = 0; j0 <= nchunks; j0 += NST) {
#pragma unroll
                for (int st = 0; st < NST; ++st) {
                    const int j = j0 + st;
                    if (j >= 1 && j - 1 < nchunks) {
                        // The rows of a chunk are independent until the y step, and a row is one dependent chain (LDS read, two
                        // multiply-adds, an IEEE divide): all YCH chains are laid side by side, free of branches, so that they overlap --
                        // row after row the consumer was the slower wavefront of the two (264 cycles per row against the producer's
                        // 173).  Rows past the image (last chunk) are computed from whatever the ring holds and never stored.
                        const int rc0 = (j - 1) * YCH;
                        float E[YCH + 2];  // x-decimated rows: E[0], E[1] = the two rows before this chunk, E[2 + u] = row rc0 + u
                        E[0] = Xp2;
                        E[1] = Xp1;
#pragma unroll
                        for (int u = 0; u < YCH; ++u) {
                            const f2 v = *reinterpret_cast<const f2*>(&ring[(st + 1) & 1][u][2 * lane]);
                            float X = 0.f;
                            if constexpr (ODD) {
                                const float v2 = ring[(st + 1) & 1][u][lane < WAVE - 1 ? 2 * lane + 2 : 2 * lane];  // the next lane's first column
                                X += v.x * od0;
                                X += v.y * fsx;
                                X += v2 * od2;
                            } else {
                                X += v.x * fsx;
                                X += v.y * fsx;
                            }
                            X /= fw;
                            E[2 + u] = X;
                            if (u == YCH / 2 - 1) __builtin_amdgcn_sched_barrier(0);  // two groups of four: eight divides side by side need 140 VGPRs
                        }
                        __builtin_amdgcn_sched_barrier(0);
                        // row y = 2t completes output row t; y = h-1-rc0-u and rc0 is a multiple of YCH (even): for an even height the
                        // odd u, for an odd height the even u
                        if (h_odd) {
#pragma unroll
                            for (int u = 0; u < YCH; u += 2) {
                                const int y = h - 1 - rc0 - u, t = y >> 1;
                                float a2 = 0.f;
                                a2 += E[2 + u] * (float)(unsigned)(h2 - t);
                                a2 += E[1 + u] * fsy;
                                a2 += E[u] * (float)(unsigned)(t + 1);
                                a2 /= fh;
                                if (y >= 0 && t < h2 && dst_live) st_out(t, a2);
                            }
                        } else {
#pragma unroll
                            for (int u = 1; u < YCH; u += 2) {
                                const int y = h - 1 - rc0 - u, t = y >> 1;
                                float a2 = 0.f;
                                a2 += E[2 + u] * fsy;
                                a2 += E[1 + u] * fsy;
                                a2 /= fh;
                                if constexpr (decltype(MR)::value) {
                                    if (y >= 0 && t < h2) {  // (workgroup-uniform)
                                        if (run_top < 0 || !__all(!dst_live || __float_as_uint(a2) == __float_as_uint(runv))) {
                                            if (dst_live)
                                                for (int tt = t + 1; tt <= run_top; ++tt) st_out(tt, runv);  // the run that ends here
                                            runv = a2;
                                            run_top = t;
                                        }
                                    }
                                } else if (y >= 0 && t < h2 && dst_live)
                                    st_out(t, a2);
                            }
                        }
                        Xp2 = E[YCH];
                        Xp1 = E[YCH + 1];
                    }
                    __syncthreads();
                }
            }
        };
        if (mr_on) {
            consume(std::true_type{});
            if (dst_live)
                for (int tt = 0; tt <= min(run_top, TS - 1); ++tt) st_out(tt, runv);
            for (int b = 1; b < mr.NR; ++b) {
                const int lo = b * TS, hi = min(lo + TS, h2) - 1;
                const bool whole = hi <= run_top;
                if (!whole && dst_live)
                    for (int tt = lo; tt <= run_top; ++tt) st_out(tt, runv);
                if (lane == 0 && (int)blockIdx.x < mr.NC) mr.flags[mr.index(blockIdx.y / 7, b, blockIdx.x)] = whole ? 1 : 0;
            }
            if (lane == 0 && (int)blockIdx.x < mr.NC) mr.flags[mr.index(blockIdx.y / 7, 0, blockIdx.x)] = 0;
        } else
            consume(std::false_type{});
    }
    if (state_out && wave == 0 && col_live) y2_store(state_out, (size_t)gridDim.y * sp, ystate_index(blockIdx.y, sp, sx), s);
}
