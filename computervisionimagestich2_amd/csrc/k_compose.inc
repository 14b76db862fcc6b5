// Part of stitch_kernels.hpp (included there, inside namespace sk): S1 -- the level-0 planes of a pair (k_compose), or their
// source index and the gathers through it (source-fused level 0) -- and the seam scan / mask (B1).
// The level-0 planes of one pair as a FUNCTION of the inputs -- exactly the values k_compose stores (planes 0..2 the
// warped frame, 3..5 the moved mosaic, 0 where the reference leaves its zeroed canvas untouched).  The consumers of
// level 0 (seam scan, causal x sweep, level-0 collapse) evaluate it in place when the plan runs "source-fused", so the
// six level-0 planes are never written to or read from HBM.  The double-precision map is evaluated once per canvas
// pixel by k_src_index, which leaves the byte offset of frame sample (nx, ny) within a channel plane (or "outside") in
// the slot of level-0 plane 0; the three channel sweeps and the collapse gather through that index.  use_src = 0: the planes are in memory (k_compose ran).
template <typename PX>
struct PairSrc {
    const PX* __restrict__ frame;
    const PX* __restrict__ mosaic;
    MapP map;
    int fw, fh, mw, mh, ox, oy;
    float offx, offy;
    size_t fpl, mpl;
    bool a_dense;  // PairArgs::a_dense: `frame` is canvas a itself (stitch_blend_*)
    __device__ __forceinline__ PairSrc(const PairArgs<PX>& pa, int pr)
        : frame(pa.frame[pr]), mosaic(pa.mosaic[pr]), map(pa.map[pr]), fw(pa.fw[pr]), fh(pa.fh[pr]), mw(pa.mw[pr]), mh(pa.mh[pr]),
          ox(pa.ox[pr]), oy(pa.oy[pr]), offx(pa.offx[pr]), offy(pa.offy[pr]), fpl((size_t)pa.fw[pr] * pa.fh[pr]),
          mpl((size_t)pa.mw[pr] * pa.mh[pr]), a_dense(pa.a_dense != 0) {}
    __device__ __forceinline__ bool frame_at(int x, int y, size_t& so) const {
        if (a_dense) {
            if (x >= fw || y >= fh) return false;
            so = (size_t)y * fw + x;
            return true;
        }
        int nx, ny;
        if (!map_to_src(map, (float)x + offx, (float)y + offy, fw, fh, nx, ny)) return false;
        so = (size_t)ny * fw + nx;
        return true;
    }
    __device__ __forceinline__ bool mosaic_at(int x, int y, size_t& so) const {
        const long long mx = (long long)x + ox, my = (long long)y + oy;
        if (mx < 0 || mx >= mw || my < 0 || my >= mh) return false;
        so = (size_t)my * mw + mx;
        return true;
    }
    __device__ __forceinline__ float frame_val(size_t so, int c) const {
        const float v = (float)frame[so + c * fpl];
        return a_dense ? v : warped_px<PX>(v);  // a dense canvas is value-cast (CImg<float>(a)), a warped sample went through the tap
    }
    __device__ __forceinline__ float mosaic_val(size_t so, int c) const { return (float)mosaic[so + c * mpl]; }
    // plane q (0..5) at canvas pixel (x, y), 0 <= x < cw
    __device__ __forceinline__ float plane(int q, int x, int y) const {
        size_t so;
        if (q < 3) return frame_at(x, y, so) ? frame_val(so, q) : 0.f;
        return mosaic_at(x, y, so) ? mosaic_val(so, q - 3) : 0.f;
    }
};

struct NoPairArgs {};  // levels >= 1 carry no pair description
// the slot whose index plane and `zi` bytes pair pr gathers through (PairArgs::idx_pr); wave-uniform wherever pr is
template <typename PX>
__device__ __forceinline__ int index_owner(const PairArgs<PX>& pa, int pr) {
    return pa.idx_pr[pr];
}
__device__ __forceinline__ int index_owner(const NoPairArgs&, int pr) { return pr; }
template <typename OUT, bool DENSE>
struct CollapseSrc {
    typedef NoPairArgs type;
};
template <typename OUT>
struct CollapseSrc<OUT, true> {
    typedef PairArgs<OUT> type;
};
// What one block of the causal x sweep needs of the pair when level 0 is source-fused: a range-checked descriptor of
// its channel plane of the frame (q < 3, gathered through the index plane) or of the mosaic (a pure shift).
struct XShift {
    int mw, mh, ox, oy;
};
template <typename PX>
__device__ __forceinline__ __amdgpu_buffer_rsrc_t x_rsrc(const PairArgs<PX>& pa, int pr, int q) {
    const bool fr = q < 3;
    const PX* base = fr ? pa.frame[pr] : pa.mosaic[pr];
    const size_t elems = fr ? (size_t)pa.fw[pr] * pa.fh[pr] : (size_t)pa.mw[pr] * pa.mh[pr];
    return plane_rsrc(base + (size_t)(fr ? q : (q < 6 ? q - 3 : 0)) * elems, elems);
}
template <typename PX>
__device__ __forceinline__ __amdgpu_buffer_rsrc_t x_rsrc(const NoPairArgs&, int, int) {
    return plane_rsrc<PX>(nullptr, 0);
}
// plane q of pair pr as a shifted dense image: the mosaic (q >= 3), or canvas a of a dense pair (q < 3, zero shift)
template <typename PX>
__device__ __forceinline__ XShift x_shift(const PairArgs<PX>& pa, int pr, int q) {
    if (q < 3 && pa.a_dense) return XShift{pa.fw[pr], pa.fh[pr], 0, 0};
    return XShift{pa.mw[pr], pa.mh[pr], pa.ox[pr], pa.oy[pr]};
}
template <typename PX>
__device__ __forceinline__ XShift x_shift(const NoPairArgs&, int, int) {
    return XShift{0, 0, 0, 0};
}
template <typename PX>
__device__ __forceinline__ bool a_is_dense(const PairArgs<PX>& pa) {
    return pa.a_dense != 0;
}
__device__ __forceinline__ bool a_is_dense(const NoPairArgs&) { return false; }
// mosaic byte offset of canvas (x, y) = row part + column part; either part 0xffffffff = outside (a valid part is
// below 0xfffffff0).  Branch-free.
template <typename PX>
__device__ __forceinline__ unsigned mosaic_col(const XShift& m, int x, int w) {
    const long long mx = (long long)x + m.ox;
    const bool ok = x < w && mx >= 0 && mx < m.mw;
    return ok ? (unsigned)mx * (unsigned)sizeof(PX) : 0xffffffffu;
}
template <typename PX>
__device__ __forceinline__ unsigned mosaic_row(const XShift& m, int y) {
    const long long my = (long long)y + m.oy;
    const bool ok = my >= 0 && my < m.mh;
    const unsigned r = (unsigned)my * (unsigned)m.mw * (unsigned)sizeof(PX);
    return ok ? r : 0xffffffffu;
}
template <typename PX>
__device__ __forceinline__ unsigned mosaic_offset(unsigned row, unsigned col) {
    // saturating add: an "outside" part (all ones) drags the sum to all ones; two valid parts never reach it (planes stay below
    // 0xfffffff0 bytes).  Masked down to the access size, all ones IS off_outside<PX>().  Two operations instead of five per
    // sample of the sweep's mosaic planes.
    return __builtin_elementwise_add_sat(row, col) & (0u - (unsigned)sizeof(PX));
}

// Sparse canvases.  A stitched canvas is mostly empty for either image (the reference blurs and decimates the zeros
// like everything else), and the recursive filters leave exact +0.0f wherever the input was zero and the state has
// died out (about 150 samples past the data; the tails of these images are non-negative).  For the levels the fused
// sweep covers (heights that are multiples of 64), a kernel that produces a 64x64 tile of the blur scratch T made of
// +0.0f only records one byte instead of storing the tile, and the next kernel takes the zeros from the flag instead
// of from HBM.  The arithmetic is unchanged (zeros are swept like any other sample); only stores and loads of
// zeros are skipped.  The test is on the bit pattern, so a -0.0f keeps its tile "non-zero".
struct ZeroTiles {
    uint8_t* flags;  // [planes][NC][NR] (bands of one tile column are contiguous), nullptr = feature off for this level
    int h, NR, NC;   // rows per plane, 64-row bands per plane, 64-column tiles per row
    __device__ __forceinline__ size_t index(long plane, int band, int tile) const { return ((size_t)plane * NC + tile) * NR + band; }
};

// G column flags: the same idea for the pyramid planes G_1 and G_2 of a batch, one byte per (plane, 64-column tile column), written
// by the decimating sweep that produces the level (k_vv_y_bwd_dec) on every call.  A set byte means: every sample of the tile column,
// in all rows, is +0.0f by bit pattern, BOTH neighbouring tile columns are +0.0f throughout as well (the plane's edge counts as
// one), and the column was NOT stored -- the memory holds whatever an earlier call left.  One exception: the producer's workgroup of
// tile column t reads the tile columns 2t and 2t + 1 of the level above, and where 2t + 1 lies past that level's last tile column (an
// odd count of them) it neither takes its all-zero path nor passes for a zero neighbour: t counts as zero, for itself and as a neighbour,
// only if 2t + 1 < ceil(w_{l-1} / 64).  Below such a level the last two tile columns are therefore never flagged, whatever they hold:
// they are stored and read like data (tests/g_flags_ref.py states the rule on the host).  The producer decides from what it READS, the
// zero-tile flags of the blurred tile columns 2t and 2t + 1 and a +0 sweep state, so the flag is sufficient for "+0 throughout", not
// necessary: where the blur's tail ends on an odd column, which the decimation drops, the tile column of G is +0 in every sample
// and still stored as data (tests/test_gpu_hard_content.py: a black band inside a frame).  Carried as a ZeroTiles with one "band":
// index(plane, 0, tile) = plane * NC + tile.  Readers (k_vv_x_fwd, the collapse kernels) take zeros instead of loading; a 16-byte
// load of the collapse that straddles two tile columns is zero when either column is flagged: a flagged column's neighbours are zero,
// and an unflagged DATA column never has a flagged neighbour.
__host__ __device__ inline ZeroTiles g_cols(uint8_t* flags, int w) { return ZeroTiles{flags, 0, 1, (w + 63) / 64}; }
__device__ __forceinline__ bool g_col_flag(const uint8_t* __restrict__ flags, int nc, int plane, int col) {
    return flags[(size_t)plane * nc + min(col >> 6, nc - 1)] != 0;
}

// Row-repeat flags of the MASK plane (slot 6 of a pair) of G_1 and G_2: one byte per (pair, 64-column tile column, 64-row band), written
// by the same producer on every call.  The blend's mask is a vertical step, and below a level of even height and width its blurred and
// decimated rows still repeat, bit for bit, down to the few rows at the bottom where the anticausal y sweep leaves its Triggs boundary.
// A set byte of band b >= 1 means: every existing row of that tile equals row 0 of the plane in its 64 columns, by bit pattern, and the
// tile was NOT stored -- the memory holds whatever an earlier call left.  Band 0 is always stored and never flagged.  No neighbour rule:
// the mask plane is read only at its own level, by the x sweep in whole tiles and by the collapse in aligned 16-byte loads.  A column of
// zeros is the case where row 0 is +0.  Carried as a ZeroTiles over PAIRS: index(pair, band, tile).  Readers take row 0 instead:
// k_vv_x_fwd (and skips a band whose tiles are all flagged), k_vv_xbyf (such a band is a constant band, as below the first band of the
// implicit level-0 mask), the collapse kernels (address select).  call_form (stitch_call_form.h) decides.
__host__ __device__ inline ZeroTiles mask_rows(uint8_t* flags, int w, int h) { return ZeroTiles{flags, h, (h + 63) / 64, (w + 63) / 64}; }
// the mask sample at (x, y) of pair pr is taken from row 0
__device__ __forceinline__ bool mask_row_flag(const uint8_t* __restrict__ flags, int nc, int nr, int pr, int x, int y) {
    return flags != nullptr && flags[((size_t)pr * nc + min(x >> 6, nc - 1)) * nr + (y >> 6)] != 0;
}

// What the index plane and the `zi` bytes in a plan's slot were computed from, kept on the device so that the decision to reuse
// them is taken in stream order (a captured sequence is replayed behind the host's back and decides again on every replay).
// The plane is a function of exactly these fields and the plan's canvas; doubles and floats are compared by bit pattern.
struct IndexKey {
    unsigned long long map[8];
    unsigned offx, offy;
    int fw, fh;
    unsigned px;     // sizeof(PX)
    unsigned valid;  // 0 at creation, after a launch that overwrote the slot (k_index_forget) and after stitch_plan_clear_fault
};
// In front of a source-fused call of n pairs, one wavefront: lane i compares pair i's descriptor with the record of slot i, leaves
// todo[i] = 1 where k_src_index has to run for the slot and takes the record over.  A pair whose owner is an earlier pair
// (PairArgs::idx_pr) reads that pair's plane: its own slot and record stay as they are.  counts (stitch_plan_index_counts): slots
// computed, slots reused from an earlier call, pairs that share another pair's plane.
template <typename PX>
__global__ __launch_bounds__(64) void k_index_keys(PairArgs<PX> pa, int n, IndexKey* __restrict__ keys, unsigned* __restrict__ todo,
                                                   unsigned* __restrict__ counts) {
    const int i = threadIdx.x;
    const bool in = i < n, owner = in && pa.idx_pr[min(i, MAXB - 1)] == i;
    bool same = false;
    if (owner) {
        IndexKey k;
        for (int j = 0; j < 8; ++j) k.map[j] = (unsigned long long)__double_as_longlong(pa.map[i].p[j]);
        k.offx = __float_as_uint(pa.offx[i]), k.offy = __float_as_uint(pa.offy[i]);
        k.fw = pa.fw[i], k.fh = pa.fh[i];
        k.px = (unsigned)sizeof(PX), k.valid = 1u;
#ifndef STITCH_NO_INDEX_REUSE  // (the A/B library: every plane on every call)
        const IndexKey r = keys[i];
        same = r.valid != 0 && r.offx == k.offx && r.offy == k.offy && r.fw == k.fw && r.fh == k.fh && r.px == k.px;
        for (int j = 0; j < 8; ++j) same = same && r.map[j] == k.map[j];
#endif
        if (!same) keys[i] = k;
    }
    if (i < MAXB) todo[i] = owner && !same ? 1u : 0u;
    const int computed = __popcll(__ballot(owner && !same)), reused = __popcll(__ballot(owner && same)), shared = __popcll(__ballot(in && !owner));
    if (i == 0) counts[0] = (unsigned)computed, counts[1] = (unsigned)reused, counts[2] = (unsigned)shared;
}
// Behind a launch that overwrote the level-0 slots of pairs 0 .. n-1 (k_compose, k_load_canvases): their records no longer hold
__global__ __launch_bounds__(64) void k_index_forget(IndexKey* __restrict__ keys, int n) {
    if ((int)threadIdx.x < n) keys[threadIdx.x].valid = 0u;
}
// What the mask pyramid in a plan's slot was computed from (include/stitch_mask_keep.h): the seam record's step and the call's form word
// (mask_keep_word, stitch_call_form.h).  The mask plane of every level is a function of exactly these and the plan; no pixel reaches
// it except through the seam scan's integers.  Kept on the device for the same reason as IndexKey.
constexpr int WF_STAND_WORD = 8;  // Wavefront::sticky[WF_STAND_WORD] (k_fused_sweep.inc): bit i set = the mask pyramid of slot i stands in this call; 0 in a band's block
struct MaskKey {
    unsigned long long thr;  // SeamDev::thr by bit pattern
    int branch, start;
    unsigned form;
    unsigned valid;  // 0 at creation and after stitch_plan_clear_fault
};
// Behind the launch that writes the call's seam records, one wavefront: lane i compares slot i's record with the call's SeamDev and form
// word, leaves todo[i] = 1 where the slot's mask planes have to be computed and 0 where they stand, and takes the record over.  A pyramid
// stands only under an identical word that has MK_KEEP_OK, and never where the scan failed (status != 0: the record is forgotten).
// A fused sweep that gave up on a hand-off leaves planes nobody may trust, and a healthy call may be queued right behind it: the count
// of timed-out waits (sticky[0], which only grows) is compared with the count this kernel saw last (counts[2]); where it has grown, no
// record of the plan holds, in this call or for the slots it does not use.
// sticky[WF_STAND_WORD]: the same answer as one word, bit i set = slot i stands, for k_vv_xbyf; counts: slots computed, slots that stood.
__global__ __launch_bounds__(64) void k_mask_keys(const SeamDev* __restrict__ seam, int n, int cap, unsigned form, MaskKey* __restrict__ keys,
                                                  unsigned* __restrict__ todo, unsigned* __restrict__ sticky, unsigned* __restrict__ counts) {
    const int i = threadIdx.x;
    const bool in = i < n;
    const unsigned timeouts = sticky ? sticky[0] : 0u;
    const bool trusted = timeouts == counts[2];
    bool same = false;
    if (in) {
        const SeamDev sd = seam[i];
        MaskKey k;
        k.thr = (unsigned long long)__double_as_longlong(sd.thr);
        k.branch = sd.branch, k.start = sd.start;
        k.form = form, k.valid = sd.status == 0 ? 1u : 0u;
        const MaskKey r = keys[i];
        same = trusted && (form & MK_KEEP_OK) != 0 && k.valid != 0 && r.valid != 0 && r.form == form && r.thr == k.thr && r.branch == k.branch && r.start == k.start;
        if (!same) keys[i] = k;
    } else if (!trusted && i < cap)
        keys[i].valid = 0u;
    if (i < MAXB) todo[i] = in && same ? 0u : 1u;
    const unsigned long long stood = __ballot(in && same);
    if (i == 0) {
        counts[0] = (unsigned)(n - __popcll(stood)), counts[1] = (unsigned)__popcll(stood), counts[2] = timeouts;
        if (sticky) sticky[WF_STAND_WORD] = (unsigned)stood;
    }
}
// the preset of the `zi` bytes ("outside" until k_src_index finds a sample) of the slots whose plane is computed in this call
__global__ __launch_bounds__(256) void k_zi_preset(uint8_t* __restrict__ flags, int per_slot, const unsigned* __restrict__ todo) {
    if (!todo[blockIdx.y]) return;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < per_slot; i += gridDim.x * blockDim.x) flags[(size_t)blockIdx.y * per_slot + i] = 1;
}

constexpr int SI_ROWS = 8;  // rows per workgroup of k_src_index (a one-row workgroup is launch-bound: 393k workgroups per batch)
// Workgroups per column block and pair in a plan's launch, each looping over the row groups.  A call whose planes all stand still
// launches the grid, and every workgroup returns at once: 12 288 of them per 16-pair sequence at 6144 x 4096 instead of 196 608.
constexpr int SI_WGY = 32;
// todo (a plan's call): the plane of slot pr is computed only where todo[pr] is set (k_index_keys); nullptr (a band): always
template <typename PX>
__global__ __launch_bounds__(256) void k_src_index(PairArgs<PX> pa, float* __restrict__ g0_all, int cw, int ch, int pitch, size_t ps,
                                                   ZeroTiles zi, int y_base = 0,  // y_base: canvas row of plane row 0 (a rank's band)
                                                   const unsigned* __restrict__ todo = nullptr) {
    const int x = blockIdx.x * blockDim.x + threadIdx.x, pr = blockIdx.z;
    if (todo && !todo[pr]) return;
    if (x >= pitch) return;
    const MapP m = pa.map[pr];
    const float offx = pa.offx[pr], offy = pa.offy[pr];
    const int fw = pa.fw[pr], fh = pa.fh[pr];
    unsigned* __restrict__ idx = reinterpret_cast<unsigned*>(g0_all + (size_t)pr * 7 * ps);
    // groups of SI_ROWS rows, gridDim.y apart (a plan's launch has at most SI_WGY workgroups per column block and pair)
    for (int y0 = blockIdx.y * SI_ROWS; y0 < ch; y0 += gridDim.y * SI_ROWS) {
        const int y1 = min(y0 + SI_ROWS, ch);
        for (int y = y0; y < y1; ++y) {
            unsigned v = off_outside<PX>();
            int nx, ny;
            if (x < cw && map_to_src(m, (float)x + offx, (float)(y + y_base) + offy, fw, fh, nx, ny))
                v = ((unsigned)ny * (unsigned)fw + (unsigned)nx) * (unsigned)sizeof(PX);  // the host checked that a plane fits 32 bits
            // a wavefront is 64 consecutive pixels of one row = one row of one 64x64 tile (the pitch is a multiple of 64): the
            // tile's "every pixel outside the frame" flag, preset to 1, is cleared by any row that holds a sample (same byte,
            // same value)
            if (zi.flags && __ballot(v != off_outside<PX>()) != 0 && (threadIdx.x & 63) == 0) zi.flags[zi.index(pr, y >> 6, x >> 6)] = 0;
            idx[(size_t)y * pitch + x] = v;
        }
    }
}

// The index plane of a slot in 16-byte runs (src_runs_rule.h; float frames).  A map that is close to a translation sends the four
// samples of an aligned group to four adjacent frame samples almost everywhere, so the causal x sweep of a frame channel can take a
// group with one 16-byte load from the group's base instead of four 4-byte gathers through four index words.  Per 64x64 tile, in
// tile_load's element-to-lane layout (lane -> rows lane/16 + 4i, columns 4(lane%16)..+3):
//   bases    [4][64 lanes][4] words: base of the lane's group i at [i / 4][lane][i % 4] -- four 16-byte loads per lane;
//   patches  64 records (position in the padded LDS tile, byte offset or off_outside): the samples a base does not deliver;
//   cls      the number of records, 0..64, or 255 = "general": gathered through the full index plane as before;
//   live     1 where any pixel of the tile has a sample (for the counts alone: the sweep knows outside tiles from `zi`).
// Plan-owned per slot with the lifecycle of the index plane and of `zi`: written -- every byte -- by k_src_runs behind k_src_index
// wherever a slot's todo word is set, kept while the slot's record stands, shared through index_owner.  flags-style null = absent.
struct SrcRuns {
    unsigned* bases;
    uint2* patches;
    uint8_t* cls;
    uint8_t* live;
    int NR, NC;    // 64-row bands per plane, 64-column tiles per row
    int mosaic16;  // the same sweep takes the mosaic's interior tiles in 16-byte loads too (k_vv_x_fwd; nothing of the arrays is involved)
    __device__ __forceinline__ size_t tile(int slot, int band, int t) const { return ((size_t)slot * NR + band) * NC + t; }
};
// One wavefront per tile of the planes k_src_index has just computed (rows >= ch of a partial last band count as outside); a workgroup
// loops over the bands gridDim.y apart, so that a call whose planes all stand launches few workgroups that return at once (SR_WGY).
constexpr int SR_WGY = 8;
template <typename PX>
__device__ __forceinline__ void src_runs_tile(const PairArgs<PX>& pa, const float* __restrict__ g0_all, int ch, int pitch, size_t ps, const SrcRuns& sr, int t,
                                              int band, int pr, int lane);
template <typename PX>
__global__ __launch_bounds__(64) void k_src_runs(PairArgs<PX> pa, const float* __restrict__ g0_all, int ch, int pitch, size_t ps, SrcRuns sr,
                                                 const unsigned* __restrict__ todo) {
    const int t = blockIdx.x, pr = blockIdx.z, lane = threadIdx.x;
    if (!todo[pr]) return;
    for (int band = blockIdx.y; band < sr.NR; band += gridDim.y) src_runs_tile<PX>(pa, g0_all, ch, pitch, ps, sr, t, band, pr, lane);
}
template <typename PX>
__device__ __forceinline__ void src_runs_tile(const PairArgs<PX>& pa, const float* __restrict__ g0_all, int ch, int pitch, size_t ps, const SrcRuns& sr, int t,
                                              int band, int pr, int lane) {
    constexpr unsigned OUT = off_outside<PX>(), px = (unsigned)sizeof(PX);
    const unsigned plane_bytes = (unsigned)pa.fw[pr] * (unsigned)pa.fh[pr] * px;
    const int r0 = lane >> 4, c = (lane & 15) << 2;
    const unsigned* __restrict__ idx = reinterpret_cast<const unsigned*>(g0_all + (size_t)pr * 7 * ps) + (size_t)band * TS * pitch + t * TS + c;
    u4 o[16];
    unsigned b[16];
    unsigned long long pm = 0;  // bit 4i + j: sample j of group i is a patch
    bool any = false;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        const int y = band * TS + r0 + 4 * i;
        o[i] = y < ch ? *reinterpret_cast<const u4*>(idx + (size_t)(r0 + 4 * i) * pitch) : u4{OUT, OUT, OUT, OUT};
        b[i] = src_runs::group_base(o[i][0], OUT, plane_bytes);
        any = any || o[i][0] != OUT || o[i][1] != OUT || o[i][2] != OUT || o[i][3] != OUT;
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (src_runs::is_patch(b[i], j, o[i][j], OUT, px)) pm |= 1ull << (4 * i + j);
    }
    unsigned incl = (unsigned)__popcll(pm);  // inclusive scan over the lanes
#pragma unroll
    for (int d = 1; d < WAVE; d <<= 1) {
        const unsigned up = __shfl_up(incl, d, WAVE);
        if (lane >= d) incl += up;
    }
    const unsigned total = __shfl(incl, WAVE - 1, WAVE), cls = src_runs::tile_class(total, px);
    const size_t ti = sr.tile(pr, band, t);
    u4* bo = reinterpret_cast<u4*>(sr.bases) + ti * 4 * WAVE + lane;
#pragma unroll
    for (int q = 0; q < 4; ++q) bo[q * WAVE] = u4{b[4 * q], b[4 * q + 1], b[4 * q + 2], b[4 * q + 3]};
    uint2* rec = sr.patches + ti * src_runs::SR_MAX_PATCHES;
    if (cls == src_runs::SR_GENERAL || (unsigned)lane >= total) rec[lane] = uint2{0u, OUT};  // the records nobody reads: defined all the same
    if (cls != src_runs::SR_GENERAL) {
        unsigned k = incl - (unsigned)__popcll(pm);
#pragma unroll
        for (int i = 0; i < 16; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if ((pm >> (4 * i + j)) & 1ull) {
                    if (k < src_runs::SR_MAX_PATCHES) rec[k] = uint2{(unsigned)((r0 + 4 * i) * (TS + 4) + c + j), o[i][j]};
                    ++k;
                }
    }
    const bool live = __ballot(any) != 0;
    if (lane == 0) sr.cls[ti] = (uint8_t)cls, sr.live[ti] = live ? 1 : 0;
}

// row0: canvas row of the planes' row 0 (0 for a whole canvas; the first row of a rank's band when one pair is split over GPUs)
template <typename PX>
__global__ __launch_bounds__(256) void k_compose(PairArgs<PX> pa, float* __restrict__ g0_all, int cw, int ch, int pitch,
                                                 size_t ps, int row0) {
    const int x = blockIdx.x * blockDim.x + threadIdx.x, yl = blockIdx.y, y = yl + row0, pr = blockIdx.z;
    if (x >= pitch) return;
    float* g0 = g0_all + (size_t)pr * 7 * ps;
    float a[3] = {0.f, 0.f, 0.f}, b[3] = {0.f, 0.f, 0.f};
    if (x < cw) {
        const PX* __restrict__ frame = pa.frame[pr];
        const PX* __restrict__ mosaic = pa.mosaic[pr];
        const int fw = pa.fw[pr], fh = pa.fh[pr], mw = pa.mw[pr], mh = pa.mh[pr];
        int nx, ny;
        if (map_to_src(pa.map[pr], (float)x + pa.offx[pr], (float)y + pa.offy[pr], fw, fh, nx, ny)) {
            const size_t spl = (size_t)fw * fh, so = (size_t)ny * fw + nx;
#pragma unroll
            for (int c = 0; c < 3; ++c) a[c] = warped_px<PX>((float)frame[so + c * spl]);
        }
        const long long mx = (long long)x + pa.ox[pr], my = (long long)y + pa.oy[pr];
        if (mx >= 0 && mx < mw && my >= 0 && my < mh) {
            const size_t spl = (size_t)mw * mh, so = (size_t)my * mw + mx;
#pragma unroll
            for (int c = 0; c < 3; ++c) b[c] = (float)mosaic[so + c * spl];
        }
    }
    const size_t o = (size_t)yl * pitch + x;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        g0[o + c * ps] = a[c];
        g0[o + (3 + c) * ps] = b[c];
    }
}

// dense canvases a, b (already warped / moved by the caller) -> level-0 planes (stitch_blend_*)
template <typename PX>
__global__ __launch_bounds__(256) void k_load_canvases(const PX* __restrict__ a, const PX* __restrict__ b,
                                                       float* __restrict__ g0, int cw, int ch, int pitch, size_t ps) {
    const int x = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y;
    if (x >= pitch) return;
    const size_t cpl = (size_t)cw * ch, co = (size_t)y * cw + x, o = (size_t)y * pitch + x;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        g0[o + c * ps] = x < cw ? (float)a[co + c * cpl] : 0.f;
        g0[o + (3 + c) * ps] = x < cw ? (float)b[co + c * cpl] : 0.f;
    }
}

// ---- B1: seam scan, ImageProcess.cpp:659-671,686-698 --------------------------------------------------------
// One workgroup walks the middle row of the level-0 planes; integer sums are reduced with wavefront shuffles
// and one LDS exchange.  Thread 0 derives ratio / ov / branch / start exactly as the reference does (seam_finish).
__device__ __forceinline__ int wave_sum(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    return v;
}

// The tail of the scan, ImageProcess.cpp:686-698: ratio / ov / branch / start from the four integers, exactly as the reference
// derives them (rule 0 in float, rule 1 in double).  Shared by k_seam, by the seams a caller states (k_seam_given, k_cover_seam:
// k_rig_seams.inc) and by the host's stitch_seam_from_sums, so a given seam is the record the scan would have written.
__host__ __device__ __forceinline__ SeamDev seam_finish(int s_a, int n_a, int s_o, int n_o, int seam_rule, int cw) {
    SeamDev s;
    s.sum_a_x = s_a;
    s.n_a = n_a;
    s.sum_ov_x = s_o;
    s.n_ov = n_o;
    s.ratio = s.ov = 0.f;
    s.branch = 1;
    s.start = cw;  // neutral mask (all zero) when the scan fails
    s.thr = 0.0;
    s.status = 0;
    s.pad = 0;
    if (n_a == 0)
        s.status = -2;
    else if (n_o == 0)
        s.status = -3;
    else if (seam_rule == 0) {
        const float ratio = (float)(1.0 * (double)s_a / (double)n_a);
        const float ov = (float)(1.0 * (double)s_o / (double)n_o);
        s.ratio = ratio;
        s.ov = ov;
        s.branch = (ratio < ov) ? 0 : 1;
        s.start = (int)(ov + 1.f);
        s.thr = (double)ov;
    } else {
        const double ratio = (double)s_a / (double)n_a, ov = (double)s_o / (double)n_o;
        s.ratio = (float)ratio;
        s.ov = (float)ov;
        s.branch = (ratio < ov) ? 0 : 1;
        s.start = (int)(ov + 1.0);
        s.thr = ov;
    }
    return s;
}

template <typename PX>
__global__ __launch_bounds__(1024) void k_seam(const float* __restrict__ g0_all, int cw, int ch, int pitch, size_t ps,
                                               int seam_rule, SeamDev* __restrict__ out_all, PairArgs<PX> pa, int use_src) {
    __shared__ int red[4][16];
    const int mid = ch / 2;
    const float* g0 = g0_all + (size_t)blockIdx.x * 7 * ps;  // one workgroup per pair
    SeamDev* out = out_all + blockIdx.x;
    const float* a0 = g0 + (size_t)mid * pitch;
    const float* b0 = a0 + 3 * ps;
    const PairSrc<PX> src(pa, blockIdx.x);
    int s_a = 0, n_a = 0, s_o = 0, n_o = 0;
    for (int x = threadIdx.x; x < cw; x += blockDim.x) {
        bool a_on, b_on;
        if (use_src) {  // source-fused plan: the middle row straight from the inputs
            size_t fo = 0, mo = 0;
            const bool fin = src.frame_at(x, mid, fo), min_ = src.mosaic_at(x, mid, mo);
            a_on = fin && src.frame_val(fo, 0) != 0.f;
            b_on = min_ && src.mosaic_val(mo, 0) != 0.f;
            if (seam_rule) {
                a_on = a_on && src.frame_val(fo, 1) != 0.f && src.frame_val(fo, 2) != 0.f;
                b_on = b_on && src.mosaic_val(mo, 1) != 0.f && src.mosaic_val(mo, 2) != 0.f;
            }
        } else {
            a_on = a0[x] != 0.f;
            b_on = b0[x] != 0.f;
            if (seam_rule) {
                a_on = a_on && a0[x + ps] != 0.f && a0[x + 2 * ps] != 0.f;
                b_on = b_on && b0[x + ps] != 0.f && b0[x + 2 * ps] != 0.f;
            }
        }
        if (a_on) {
            s_a += x;
            ++n_a;
            if (b_on) {
                s_o += x;
                ++n_o;
            }
        }
    }
    s_a = wave_sum(s_a);
    n_a = wave_sum(n_a);
    s_o = wave_sum(s_o);
    n_o = wave_sum(n_o);
    const int wid = threadIdx.x >> 6, lane = threadIdx.x & 63;
    if (lane == 0) {
        red[0][wid] = s_a;
        red[1][wid] = n_a;
        red[2][wid] = s_o;
        red[3][wid] = n_o;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        const int nw = blockDim.x >> 6;
        s_a = n_a = s_o = n_o = 0;
        for (int i = 0; i < nw; ++i) {
            s_a += red[0][i];
            n_a += red[1][i];
            s_o += red[2][i];
            n_o += red[3][i];
        }
        *out = seam_finish(s_a, n_a, s_o, n_o, seam_rule, cw);
    }
}

// mask level 0: a vertical step (ImageProcess.cpp:682,690-698), plane 6 of level 0
__global__ __launch_bounds__(256) void k_mask(float* __restrict__ g0_all, int cw, int pitch, size_t ps,
                                              const SeamDev* __restrict__ seam_all) {
    const int x = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y;
    if (x >= pitch) return;
    float* m0 = g0_all + ((size_t)blockIdx.z * 7 + 6) * ps;
    const SeamDev* seam = seam_all + blockIdx.z;
    float v = 0.f;
    if (x < cw) v = seam->branch == 0 ? ((double)x < seam->thr ? 1.f : 0.f) : (x >= seam->start ? 1.f : 0.f);
    m0[(size_t)y * pitch + x] = v;
}
