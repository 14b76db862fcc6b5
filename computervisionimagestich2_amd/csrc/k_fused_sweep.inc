// Part of stitch_kernels.hpp (included there, inside namespace sk): the fused anticausal-x + causal-y sweep: row bands as pipeline stages (k_vv_xbyf).
// ---- fused anticausal-x + causal-y sweep: row bands as pipeline stages ---------------------------------------
// The anticausal x sweep walks a row right-to-left, the causal y sweep walks a column top-down.  One wavefront owns
// a 64-row band of one plane and walks it right-to-left in 64x64 tiles: each tile is fetched to LDS, swept along x
// (lane = row; the x state never leaves the registers), then along y (lane = column) and written back once -- the
// level is read and written ONCE instead of twice.  The y sweep of tile (R,C) needs the y state of the 64 columns
// as band R-1 left it, so band R simply runs a constant lag (one y sweep + one hand-off) behind band R-1: all
// bands of all planes are in flight at once, a 64-deep software pipeline per plane.  The per-sample arithmetic and
// its order are those of k_vv_x_bwd / k_vv_y_fwd.
//
// Workgroups are persistent and claim bands in increasing R from one atomic counter, so the band a claimed band
// depends on has always been claimed earlier by a workgroup that is running (no residency assumption, no deadlock).
// The y state travels as 8-byte granules, a 16-bit tag above 48 bits of payload (the data is the flag; relaxed
// agent-scope atomics = sc1 write-through stores / L1-bypassing loads; guide 6, Guideline 16, form R2): four
// granules per lane for three doubles, a fifth on the planes that pass the level-0 mask row down.  tag = (epoch << 12)
// | (producer band + 1), so the slot of a column block is reused band after band within a launch; tag bit 15 marks a
// state that is +0 in every live column, which travels as the polled word alone (a third of the image planes at
// config 2: the canvas left of the warped frame, right of the mosaic).  Between launches the host clears the slots with k_clear_words and passes a constant epoch: a
// per-launch epoch would be frozen by a HIP-graph capture and stale tags of the previous replay would match at
// once.  Every spin is bounded; a timeout raises `abort` for all workgroups.
typedef unsigned long long u64;
typedef __attribute__((address_space(1))) u64 gu64;
typedef __attribute__((address_space(1))) unsigned gu32;

struct Wavefront {
    u64* yg;            // [planes][NC][WF_GRAN][64] granules: y state leaving band R towards band R+1
    int mask_l0;        // level-0 implicit mask (see MaskL0): planes p%7==6 carry their x-blurred row in the 5th granule.
                        // 2: the tiles of such a plane below its first band are recorded, not stored, where they repeat the
                        // plane's row 0 (the reader is k_vv_y_bwd_dec with fill_l0 set: a plan's batch launch only)
    unsigned* counter;  // band queue head (zeroed by the host before the launch)
    unsigned* abort;    // set when a spin timed out (cleared in front of every launch sequence)
    unsigned* sticky;   // count of timed-out waits since the plan was created: NEVER cleared by the launch sequence, so
                        // a bail-out in any earlier queued call is still visible to stitch_plan_status_at.  Behind it, as
                        // 64-bit words that only grow too: hand-offs published in full (sticky + 2) and as the zero marker
                        // (sticky + 4), added once per band by one lane (stitch_plan_handoff_counts)
    int NR, NC, NP;
    unsigned epoch;
    unsigned spin_limit;      // polls before a wait gives up (STITCH_XBYF_SPIN_LIMIT; tests force the bail-out path with 0)
    ZeroTiles zt;             // zero-tile flags of T at this level (see ZeroTiles)
    ZeroTiles mr;             // a level >= 1: row-repeat flags of the mask plane of G at this level (mask_rows), or none
    // read by the BANDED instance only (stitch_band: a row band of a pair split over several GPUs)
    int ph, y0;               // rows per plane in memory and the first swept row of a plane: the band sweeps rows y0 .. y0+h-1
    const double* resume;     // a band below the first: the y state the band above left, [3][planes][pitch] (as k_vv_y_fwd)
    int early_read;           // read the hand-off state ahead of the tile prefetch (granules_issue)
    unsigned long long* dbg;  // diagnostic build only: [workgroups][8] cycle sums per segment
};

#ifndef STITCH_XBYF_SLEEP
#define STITCH_XBYF_SLEEP 32  // s_sleep between the polls of a hand-off wait (A/B builds: 8 and 2 measured, scripts/experiments/r4_run28.sh)
#endif
constexpr int WF_GRAN = 5;  // slot stride in granules per lane: 3 doubles = 4 payloads of 48 bits, + the mask row's word (pass_row planes only)
constexpr int WF_POLL = 3;  // the polled word: granule WF_POLL of the last lane
constexpr unsigned WF_ZERO = 0x8000u;  // tag bit: every live column's state is +0 (and the row word 0); ONLY the polled word was stored
constexpr u64 WF_PAYLOAD = (1ull << 48) - 1;
// Publishes the y state of `live` columns under `tag`; returns true when it went out as the zero marker (one word instead of four
// or five per lane).  The test is on the bit pattern, as in y_idle and the zero-tile flags: a -0.0 is not zero here.
__device__ __forceinline__ bool granules_publish(u64* base, int lane, int live, unsigned tag, double a, double b, double c, unsigned extra, bool row) {
    const u64 wa = (u64)__double_as_longlong(a), wb = (u64)__double_as_longlong(b), wc = (u64)__double_as_longlong(c), t = (u64)tag << 48;
    if (__ballot(lane < live && ((wa | wb | wc) != 0 || (row && extra != 0))) == 0) {
        if (lane == WAVE - 1)
            __hip_atomic_store((gu64*)(base + WF_POLL * WAVE + lane), (u64)(tag | WF_ZERO) << 48, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        return true;
    }
    if (row) __hip_atomic_store((gu64*)(base + 4 * WAVE + lane), t | extra, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store((gu64*)(base + lane), t | (wa & WF_PAYLOAD), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store((gu64*)(base + WAVE + lane), t | (wa >> 48) | ((wb & 0xffffffffull) << 16), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store((gu64*)(base + 2 * WAVE + lane), t | (wb >> 32) | ((wc & 0xffffull) << 32), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store((gu64*)(base + 3 * WAVE + lane), t | (wc >> 16), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    return false;
}
// Wait for a state.  Pollers cost the streaming wavefronts bandwidth (guide, "polling-cost"), and most bands wait
// long for their first tile (band R starts R hand-offs after band 0), so the wait is two-phase: ONE lane re-reads
// ONE granule with a long sleep between polls; once its tag matches, the whole wavefront reads its four (five) granules,
// repeating that (rarely) until every tag matches -- the stores of one publish may become visible in any order.  A polled
// word that carries the zero marker IS the whole state: nothing else is read.
// Wave-uniform exit; false on timeout / abort.
// The same read, split in two so that it can be issued early: the loads go out BEFORE the next tile's prefetch
// (loads return in order, so a poll issued behind 16 tile loads would wait for all of them), the check happens after the
// x sweep.  In the steady state of the pipeline the band above is ahead and the early read already holds the state.  The
// polled word is the last lane's granule WF_POLL, so the early read holds the zero marker too: no second round trip.
// (A second tile of prefetch was tried and is slower: more bytes in flight lengthen every queue the hand-off sits in.)
// `row` (wave-uniform, constant over a band): the plane passes the mask row down, i.e. the fifth granule exists.
__device__ __forceinline__ void granules_issue(const u64* base, int lane, u64 g[WF_GRAN], bool row) {
#pragma unroll
    for (int i = 0; i < 4; ++i) g[i] = __hip_atomic_load((gu64*)(base + i * WAVE + lane), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    g[4] = 0;
    if (row) g[4] = __hip_atomic_load((gu64*)(base + 4 * WAVE + lane), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ bool granules_accept(const u64 g[WF_GRAN], unsigned tag, double& a, double& b, double& c, unsigned& extra, bool row) {
    const unsigned polled = (unsigned)__builtin_amdgcn_readlane((int)(g[WF_POLL] >> 48), WAVE - 1);
    if (polled == (tag | WF_ZERO)) {
        a = b = c = 0.0;
        extra = 0;
        return true;
    }
    bool ok = !row || (unsigned)(g[4] >> 48) == tag;
#pragma unroll
    for (int i = 0; i < 4; ++i) ok &= (unsigned)(g[i] >> 48) == tag;
    if (!__all(ok)) return false;
    extra = (unsigned)g[4];
    a = __longlong_as_double((long long)((g[0] & WF_PAYLOAD) | (g[1] << 48)));
    b = __longlong_as_double((long long)(((g[1] & WF_PAYLOAD) >> 16) | (g[2] << 32)));
    c = __longlong_as_double((long long)(((g[2] & WF_PAYLOAD) >> 32) | (g[3] << 16)));
    return true;
}
__device__ __forceinline__ bool granules_consume(const u64* base, int lane, unsigned tag, unsigned* abort, unsigned* sticky,
                                                 unsigned spin_limit, double& a, double& b, double& c, unsigned& extra, bool row, bool brisk = false) {
    // brisk (k_vv_xby_m's courier: a wavefront that does nothing else, few of them on the chip): short naps between polls
    for (unsigned spins = 0;; ++spins) {
        // two-phase poll: one lane watches the tag of one granule, the whole wavefront reads its granules only once it has
        // appeared (polling all of them, or sleeping less, measured within +-3 %)
        unsigned seen = 0;
        if (lane == 0)
            seen = (unsigned)(__hip_atomic_load((gu64*)(base + WF_POLL * WAVE + (WAVE - 1)), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) >> 48);
        seen = __shfl(seen, 0, 64);
        if (seen == (tag | WF_ZERO)) {  // the marker: nothing else was stored
            a = b = c = 0.0;
            extra = 0;
            return true;
        }
        if (seen == tag) {
            u64 g[WF_GRAN];
            granules_issue(base, lane, g, row);
            if (granules_accept(g, tag, a, b, c, extra, row)) return true;
        }
        {
            if ((spins & 31) == 31) {
                unsigned ab = 0;
                if (lane == 0) ab = __hip_atomic_load((gu32*)abort, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                ab = __shfl(ab, 0, 64);
                if (ab != 0 || spins > spin_limit) {
                    if (lane == 0) {
                        __hip_atomic_store((gu32*)abort, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                        atomicAdd(sticky, 1u);
                    }
                    return false;
                }
            }
            if (brisk)
                __builtin_amdgcn_s_sleep(2);
            else
                __builtin_amdgcn_s_sleep(STITCH_XBYF_SLEEP);
        }
    }
}

//
// MODE 0: the samples the causal x sweep left are read from `data` and swept in place.  MODE 1 / 2: the causal x sweep ran
// as k_vv_x_fwd<.., CKPT> and kept only its state in front of every tile; this kernel fetches the level's INPUT tile (MODE 1:
// the planes `in`; MODE 2, source-fused level 0: the pair's frames through the index plane, as k_vv_x_fwd<PX, true> does),
// re-runs the 64 causal steps from the checkpoint in LDS -- the same operations on the same operands, so the same bits --
// and carries on as MODE 0.  The level's x-swept samples never travel to HBM and back.
struct Recompute {
    const float* in;       // MODE 1: level input planes; MODE 2: the plan's level-0 planes (slot 0 of a pair = its index plane)
    const double* ckpt;    // [3][tiles][lines]
    const SeamDev* seam;   // implicit level-0 mask: band 0 of a mask plane generates the step
    ZeroTiles zi;          // MODE 2: index tiles that lie outside the frame
};
// BANDED (stitch_band: a row band of a pair split over several GPUs): rows y0 .. y0+h-1 of planes that are ph rows apart in
// memory, starting from the y state `resume` when the band is not the first.  A template parameter, not a run-time test: the
// extra scalars alone (11 more SGPR spills in a kernel that already spills) cost the batch sweep 9 % when they were arguments
// of the one instance.
// Three wavefronts per SIMD (168 VGPRs) are asked for where the instance fits them: left to itself the scheduler gives up that tier for a
// register or two at the tile store and then spreads to 190 (the re-run forms and the diagnostic build need two tiers anyway).
template <bool STAMP, typename PX = float, int MODE = 0, bool BANDED = false>
__global__ __launch_bounds__(64, (MODE == 0 && !STAMP) ? 3 : 2) void k_vv_xbyf(float* __restrict__ data, int w, int h, int pitch, VVK k,
                                                 const double* __restrict__ state_x, long lines, double* __restrict__ state_y,
                                                 Wavefront wf, Recompute rc, typename CollapseSrc<PX, MODE == 2>::type pa) {
    __shared__ __attribute__((aligned(16))) float tile[TS * TP];
    const int lane = threadIdx.x;
    const unsigned nbands = (unsigned)wf.NP * wf.NR;
    unsigned long long seg[8] = {0, 0, 0, 0, 0, 0, 0, 0}, t0 = 0, t1 = 0;
    auto stamp = [&](int i) {
        if (STAMP) {
            t1 = __builtin_amdgcn_s_memtime();
            seg[i] += t1 - t0;
            t0 = t1;
        }
    };
    if (STAMP) t0 = __builtin_amdgcn_s_memtime();
    bool dead = false;
    while (!dead) {
        unsigned q = 0;
        // A mask plane that stands (mask_stands, k_sweeps.inc): its bands are claimed and dropped, here in the claim itself.  The slots'
        // bits come through a pointer the kernel holds anyway (word WF_STAND_WORD behind the sticky count; one more scalar argument costs
        // this instance its tier).  Nobody waits for a dropped band: only band (R+1, p) polls the granules of band (R, p), it is dropped
        // under the same bit, and the bit was written by a kernel earlier in stream order (k_mask_keys) -- it cannot change while this
        // launch runs.
        for (;;) {
            if (lane == 0) q = atomicAdd(wf.counter, 1u);
            q = __builtin_amdgcn_readfirstlane(__shfl(q, 0, 64));  // provably wave-uniform: band, plane and every branch on them stay scalar
            if constexpr (MODE == 0 && !BANDED) {
                const unsigned pc = q % (unsigned)wf.NP;
                if (q < nbands && pc % 7u == 6u && ((__builtin_amdgcn_readfirstlane(wf.sticky[WF_STAND_WORD]) >> (pc / 7u)) & 1u) != 0) continue;
            }
            break;
        }
        if (q >= nbands) break;
        const int R = (int)(q / wf.NP), p = (int)(q % wf.NP);  // every plane's band R before any band R+1
        const int r0 = R * TS, nrows = min(TS, h - r0);
        const int ph = BANDED ? wf.ph : h, y0 = BANDED ? wf.y0 : 0;  // wave-uniform
        float* base = data + ((size_t)p * ph + y0 + r0) * pitch;
        // level-0 implicit mask plane below its first band: every row equals the x-blurred row that band 0 passes down
        // with the y state, so there is nothing to fetch and no x sweep to run (k_vv_x_fwd skipped these rows too)
        // A level >= 1 with row-repeat flags of its mask plane (mask_rows): the plane passes its x-blurred row 0 down in the same way,
        // and a band below the first whose tiles are ALL flagged repeats row 0 of G_l in every row -- the same constant band, with nothing
        // stored behind it (k_vv_x_fwd returned at once).  Any other band of the plane is fetched and swept like a plane of samples; it
        // receives and forwards the fifth granule.
        const bool rows_l = MODE == 0 && !BANDED && wf.mr.flags != nullptr;  // wave-uniform
        const bool pass_row = (wf.mask_l0 || rows_l) && (p % 7 == 6);
        bool const_rows = wf.mask_l0 && (p % 7 == 6) && R > 0;
#if !(STITCH_MASK_ROWS_IGNORE & 2)  // (hand-check libraries only: a sweep that fetches the unstored bands)
        if (rows_l && pass_row && R > 0) {
            bool all = true;
            for (int t0 = 0; t0 < wf.NC; t0 += WAVE) all = all && __all(t0 + lane >= wf.NC || wf.mr.flags[wf.mr.index(p / 7, R, min(t0 + lane, wf.NC - 1))] != 0);
            const_rows = all;
        }
#endif
        const bool fill_plane = !BANDED && pass_row && (wf.mask_l0 == 2 || rows_l);  // flags of T mean "repeats row 0" on this plane
        stamp(0);  // claim

        // x state of this band's rows: where the causal x sweep left it, through the Triggs boundary (CImg.h:34911-34922)
        double v1 = 0, v2 = 0, v3 = 0;
        float first;
        {
            const long line = (long)p * ph + y0 + r0 + lane;
            double iplus = 0;
            if (lane < nrows) {
                v1 = state_x[line];
                v2 = state_x[lines + line];
                v3 = state_x[2 * lines + line];
                iplus = state_x[3 * lines + line];
            }
            triggs(k, iplus, v1, v2, v3, first);
        }
        f4 pre[16];
        // MODE 1/2: where this band's input comes from (all wave-uniform)
        const int src_q = p % 7, src_pr = p / 7;
        const bool gen_mask = MODE != 0 && pass_row;  // band 0 of an implicit mask plane: the step itself
        const bool gen_frame = MODE == 2 && src_q < 3 && !a_is_dense(pa), gen_mosaic = MODE == 2 && src_q < 6 && !gen_frame;
        const float* in_base = MODE == 1 ? rc.in + ((size_t)p * h + r0) * pitch : nullptr;
        const int idx_pr = index_owner(pa, src_pr);
        const float* idx_rows = MODE == 2 ? rc.in + ((size_t)idx_pr * 7 * h + r0) * pitch : nullptr;  // rows r0.. of the index plane the pair reads
        const __amdgpu_buffer_rsrc_t rs = x_rsrc<PX>(pa, src_pr, src_q);
        const XShift ms = x_shift<PX>(pa, src_pr, src_q);
        SeamDev sd{};
        if (gen_mask) sd = rc.seam[src_pr];
        // checkpoint of tile C (the causal state in front of its first sample); tile 0 starts from the boundary value instead
        const long cline = (long)p * h + r0 + lane;
        double n1 = 0, n2 = 0, n3 = 0;
        auto fetch_ckpt = [&](int C) {
            if (MODE != 0 && C > 0 && lane < nrows) {
                const double* c = rc.ckpt + (size_t)(3 * C) * lines + cline;
                n1 = c[0];
                n2 = c[lines];
                n3 = c[2 * lines];
            }
        };
        // Tile C of this band into `pre`: from HBM, or zeros when the causal x sweep recorded it as all +0.  MODE 2 fetches in
        // two steps through the SAME registers: fetch_tile puts the tile's element indices into `pre` (index plane, frame
        // channels), gather_tile -- issued one sweep later -- replaces them by the samples (a second register tile for the
        // indices would halve the wavefronts per SIMD).
        auto fetch_tile = [&](int C) {  // true: the tile is all +0
            const bool zero = wf.zt.flags && wf.zt.flags[wf.zt.index(p, R, C)];
            if (zero) {
#pragma unroll
                for (int i = 0; i < 16; ++i) pre[i] = f4{0.f, 0.f, 0.f, 0.f};
            } else if (MODE == 0)
                tile_load(base, pitch, C * TS, lane, pre);
            else if (gen_mask) {
                f4 v;
                const int c = C * TS + ((lane & 15) << 2);
                v.x = mask_step(sd, c);
                v.y = mask_step(sd, c + 1);
                v.z = mask_step(sd, c + 2);
                v.w = mask_step(sd, c + 3);
#pragma unroll
                for (int i = 0; i < 16; ++i) pre[i] = v;
            } else if (MODE == 1)
                tile_load(in_base, pitch, C * TS, lane, pre);
            else if (gen_frame) {
                if (rc.zi.flags && rc.zi.flags[rc.zi.index(idx_pr, R, C)]) {
                    const float o = __uint_as_float(off_outside<PX>());
#pragma unroll
                    for (int i = 0; i < 16; ++i) pre[i] = f4{o, o, o, o};
                } else
                    tile_load(idx_rows, pitch, C * TS, lane, pre);
            }
            if (MODE != 0 && !zero) fetch_ckpt(C);
            return zero;
        };
        auto gather_tile = [&](int C, bool zero) {
            if constexpr (MODE == 2) {
                if (zero || gen_mask) return;
                if (gen_mosaic) mosaic_indices<PX>(ms, C * TS, lane, r0, w, pre);
                src_gather<PX>(rs, pre, pre);
            }
        };
        bool next_zero = false, spec = true;
        unsigned sent = 0;  // hand-offs of this band: full ones in the low half, zero markers in the high half (NC < 65536)
        // Level-0 mask blur, recorded instead of stored.  Below the first band every input of a column is the one constant rowv, and
        // the causal sweep started at that constant's fixed point (u = rowv / sumsq): in float the outputs repeat the first one (row
        // 0 of the plane, which band 0 always stores) although the double state may cycle in its last bit -- so the equality is
        // tested, tile by tile, on the outputs themselves.  The flag of such a tile then means "every sample equals row 0 of its
        // column"; +0 everywhere is the case rowv = +0.  k_vv_y_bwd_dec substitutes the row-0 value.
        const bool fill_rows = fill_plane && const_rows;
        unsigned recorded = 0;
        if (!const_rows) {
            next_zero = fetch_tile(wf.NC - 1);
            gather_tile(wf.NC - 1, next_zero);
        }
        for (int C = wf.NC - 1; C >= 0; --C) {
            const int c0 = C * TS, ncols = min(TS, w - c0);
            const bool tile_zero = next_zero;  // the tile now going to LDS holds +0 only
            u64* slot = wf.yg + ((size_t)p * wf.NC + C) * WF_GRAN * WAVE;
            u64 early[WF_GRAN];
            // speculation is dropped while it fails (the band above is not ahead: the loads would only be repeated
            // by the poll) and probed again every fourth tile
            const bool early_on = R > 0 && wf.early_read && (spec || (C & 3) == 0);
            if (early_on) granules_issue(slot, lane, early, pass_row);  // ahead of the prefetch below (in-order return)
            double f1 = n1, f2 = n2, f3 = n3;  // this tile's checkpoint (MODE 1/2)
            if (!const_rows) {
                if constexpr (MODE == 2)
                    if (!tile_zero && !gen_mask) src_finish<PX>(gen_frame, pre);
                tile_to_lds(tile, lane, pre);
                if (C > 0) next_zero = fetch_tile(C - 1);  // next tile of the band, in flight during both sweeps
            }
            __syncthreads();
            stamp(1);  // tile fetch
            // ---- MODE 1/2: the causal x sweep of this tile again, lane = row r0+lane (k_vv_x_fwd's loop) -------------
            if (MODE != 0 && !const_rows && !tile_zero) {
                float* row = tile + lane * TP;
                if (C == 0) f1 = f2 = f3 = (double)row[0] / k.sumsq;  // CImg.h:34909
                const int jfull = ncols & ~15;
                for (int jb = 0; jb < jfull; jb += 16) {
                    float xs[16];
#pragma unroll
                    for (int qq = 0; qq < 4; ++qq) *reinterpret_cast<f4*>(xs + 4 * qq) = *reinterpret_cast<const f4*>(row + jb + 4 * qq);
#pragma unroll
                    for (int u = 0; u < 16; ++u) {
                        double v0 = (double)xs[u];
                        v0 += f1 * k.f1;
                        v0 += f2 * k.f2;
                        v0 += f3 * k.f3;
                        xs[u] = (float)v0;
                        f3 = f2;
                        f2 = f1;
                        f1 = v0;
                    }
#pragma unroll
                    for (int qq = 0; qq < 4; ++qq) *reinterpret_cast<f4*>(row + jb + 4 * qq) = *reinterpret_cast<const f4*>(xs + 4 * qq);
                }
                for (int j = jfull; j < ncols; ++j) {
                    double v0 = (double)row[j];
                    v0 += f1 * k.f1;
                    v0 += f2 * k.f2;
                    v0 += f3 * k.f3;
                    row[j] = (float)v0;
                    f3 = f2;
                    f2 = f1;
                    f1 = v0;
                }
            }
            if (!const_rows && C > 0) gather_tile(C - 1, next_zero);  // MODE 2: the indices have arrived during the causal sweep
            // ---- anticausal x sweep, lane = row r0+lane ---------------------------------------------------------
            // Zeros in, zero state: every product and sum of the recurrence is +0 again (x*sum = +0, and +0 plus a zero of
            // either sign is +0), so the sweep would rewrite the zeros it found and leave the state as it is: skipped.
            const bool x_idle = tile_zero && !const_rows && C != wf.NC - 1 &&
                                __ballot((__double_as_longlong(v1) | __double_as_longlong(v2) | __double_as_longlong(v3)) != 0) == 0;
            if (!const_rows && !x_idle) {
                float* row = tile + lane * TP;
                int jtop = ncols;
                if (C == wf.NC - 1) {
                    row[jtop - 1] = first;  // sample w-1 takes the boundary value (CImg.h:34920)
                    --jtop;
                }
                const int jfull = jtop & ~15;
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
                for (int jb = jfull - 16; jb >= 0; jb -= 16) {
                    float xs[16];
#pragma unroll
                    for (int qq = 0; qq < 4; ++qq) *reinterpret_cast<f4*>(xs + 4 * qq) = *reinterpret_cast<const f4*>(row + jb + 4 * qq);
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
                    for (int qq = 0; qq < 4; ++qq) *reinterpret_cast<f4*>(row + jb + 4 * qq) = *reinterpret_cast<const f4*>(xs + 4 * qq);
                }
            }
            __syncthreads();
            stamp(2);  // x sweep
            // ---- causal y sweep, lane = column c0+lane -----------------------------------------------------------
            float* colp = tile + lane;
            double u1, u2, u3;
            unsigned rowbits = 0;
            if (BANDED && R == 0 && wf.resume) {  // the sweep continues from the state another GPU's band left
                const size_t n = (size_t)wf.NP * pitch, i = (size_t)p * pitch + c0 + lane;
                u1 = wf.resume[i], u2 = wf.resume[n + i], u3 = wf.resume[2 * n + i];
                rowbits = __float_as_uint(colp[0]);  // implicit mask plane: the x-blurred row, as below
            } else if (R == 0) {
                u1 = u2 = u3 = (double)colp[0] / k.sumsq;  // CImg.h:34909
                rowbits = __float_as_uint(colp[0]);     // the x-blurred row (mask plane: identical for every y)
            } else {
                const bool hit = early_on && granules_accept(early, (wf.epoch << 12) | (unsigned)R, u1, u2, u3, rowbits, pass_row);
                if (early_on) spec = hit;
                if (!hit && !granules_consume(slot, lane, (wf.epoch << 12) | (unsigned)R, wf.abort, wf.sticky, wf.spin_limit, u1, u2, u3, rowbits, pass_row)) {
                    dead = true;
                    break;
                }
            }
            stamp(3);  // y state wait
            const float rowv = __uint_as_float(rowbits);
            unsigned fillbits = 0;  // what the outputs are compared with: +0, or (fill_rows) the first causal output for rowv
            if (fill_rows) {  // the operations band 0 performs for its row 0
                const double u = (double)rowv / k.sumsq;
                double v0 = (double)rowv;
                v0 += u * k.f1;
                v0 += u * k.f2;
                v0 += u * k.f3;
                fillbits = __float_as_uint((float)v0);
            }
            // rows that are all the passed-down row: below the first band of an implicit mask plane -- and, in a BANDED launch, in
            // the first band too: it starts y0 rows into the plane, so its last rows lie beyond the 64 rows the x sweeps generate
            const bool y_const = const_rows || (BANDED && pass_row);
            unsigned ynz = 0;  // OR of the bit patterns of this lane's column after the sweep, each XOR fillbits
            const double iplus_y = y_const ? (double)rowv : (double)colp[(nrows - 1) * TP];  // last band only (CImg.h:34906)
            // the same for the y sweep: a tile of +0 under a +0 state stays +0 (only the columns that exist are asked)
            const bool y_idle = x_idle && __ballot(lane < ncols && (__double_as_longlong(u1) | __double_as_longlong(u2) |
                                                                   __double_as_longlong(u3)) != 0) == 0;
            for (int j0 = 0; j0 < (y_idle ? 0 : nrows); j0 += 16) {
                if (j0 + 16 <= nrows) {
                    // all 16 column samples are read before the chain starts and written after it ends: a read placed
                    // between the writes would be kept in program order (the compiler cannot tell the rows apart) and
                    // put one LDS round trip per sample on the critical path
                    float ys[16];
                    if (y_const) {
#pragma unroll
                        for (int u = 0; u < 16; ++u) ys[u] = rowv;
                    } else {
#pragma unroll
                        for (int u = 0; u < 16; ++u) ys[u] = colp[(j0 + u) * TP];
                    }
#pragma unroll
                    for (int u = 0; u < 16; ++u) {
                        double v0 = (double)ys[u];
                        v0 += u1 * k.f1;
                        v0 += u2 * k.f2;
                        v0 += u3 * k.f3;
                        ys[u] = (float)v0;
                        ynz |= __float_as_uint(ys[u]) ^ fillbits;
                        u3 = u2;
                        u2 = u1;
                        u1 = v0;
                    }
#pragma unroll
                    for (int u = 0; u < 16; ++u) colp[(j0 + u) * TP] = ys[u];
                } else {
                    for (int j = j0; j < nrows; ++j) {
                        double v0 = y_const ? (double)rowv : (double)colp[j * TP];
                        v0 += u1 * k.f1;
                        v0 += u2 * k.f2;
                        v0 += u3 * k.f3;
                        colp[j * TP] = (float)v0;
                        ynz |= __float_as_uint(colp[j * TP]) ^ fillbits;
                        u3 = u2;
                        u2 = u1;
                        u1 = v0;
                    }
                }
            }
            if (R < wf.NR - 1)
                sent += granules_publish(slot, lane, ncols, (wf.epoch << 12) | (unsigned)(R + 1), u1, u2, u3, rowbits, pass_row) ? 0x10000u : 1u;
            else {  // last band: the state the anticausal y sweep starts from ([4][planes][pitch], as k_vv_y_fwd leaves it)
                const size_t n = (size_t)wf.NP * pitch, i = (size_t)p * pitch + c0 + lane;
                state_y[i] = u1;
                state_y[n + i] = u2;
                state_y[2 * n + i] = u3;
                state_y[3 * n + i] = iplus_y;
            }
            __syncthreads();
            stamp(4);  // y sweep + publish
            bool out_zero = false;
            if (wf.zt.flags) {  // the y sweep ran over every column of the tile; columns >= w hold whatever the fetch left: not counted
                out_zero = __ballot(lane < ncols && ynz != 0) == 0;
                // a band of samples of a plane whose flags mean "repeats row 0" is always stored: band 0 holds that row, and an all-(+0)
                // tile of a swept band of a level >= 1 would be read back as row 0
                if (fill_plane && !const_rows) out_zero = false;
                if (lane == 0) wf.zt.flags[wf.zt.index(p, R, C)] = out_zero ? 1 : 0;
                if (fill_rows && out_zero) ++recorded;
            }
            if (!out_zero) tile_store_rows(base, pitch, c0, lane, tile, nrows);  // a partial last band must not touch the next plane's rows
            __syncthreads();  // the tile buffer is refilled next
            stamp(5);  // store
        }
        if (lane == 0 && sent != 0) {
            atomicAdd((u64*)(wf.sticky + 2), (u64)(sent & 0xffffu));
            atomicAdd((u64*)(wf.sticky + 4), (u64)(sent >> 16));
        }
        if (lane == 0 && recorded != 0) atomicAdd((u64*)(wf.sticky + 6), (u64)recorded);
    }
    if (STAMP && lane == 0)
        for (int i = 0; i < 8; ++i) wf.dbg[(size_t)blockIdx.x * 8 + i] = seg[i];
}
