// Part of stitch_kernels.hpp (included there, inside namespace sk): the sweeps of the recursive Gaussian (B3) and the fused
// decimation (B4) for launches that leave SIMDs idle -- ONE pair in flight, the form every call of the reference's sequential
// matching() takes through the drop-in.  Same arithmetic, same order per sample as k_sweeps.inc's kernels.
//
// What bounds such a launch is not bytes but one wavefront's chain: the critical path of a pyramid level is 2 w + 2 h dependent
// recurrence steps (causal x, anticausal x, causal y, anticausal y; a level starts from the LAST rows the level above emits --
// its anticausal y sweep runs bottom-up, the next level's causal one top-down -- so levels do not overlap either).  A step is
// four dependent double-precision operations, 34 cycles = 14.3 ns (scripts/experiments/chain_rate.hip); everything else the
// wavefront issues around them -- loads, stores, LDS transposes, barriers, address arithmetic, the decimation's IEEE divides --
// is time added to every step, because a wavefront that has a SIMD to itself issues one instruction at a time.  Round 3's
// kernels ran at 31 (x), 45 (causal y) and 75 ns (anticausal y + decimation) per step.  What this file does about it:
//   * k_vv_y_fwd1s       rows through a raw buffer descriptor with the row offset carried in an SGPR (one scalar add and clamp
//                        per row instead of a 64-bit row * pitch product per load and per store): 45 -> 39 ns;
//   * k_vv_x_m, k_vv_y_m the recurrence ALONE on one wavefront (the chain), on LDS-resident tiles / rows with compile-time bounds
//                        and its LDS reads one group ahead; a loader and a storer wavefront of the same workgroup (other SIMDs
//                        of the CU) stream the data between HBM and LDS two steps ahead and one step behind; k_vv_x_m's loader also
//                        does the gathers of a source-fused level 0, so that a lone pair skips k_compose too: 31 -> 21 ns (x),
//                        39 -> 30 ns (y);
//   * k_vv_y_bwd_dec7    loader, two chains and four consumers as a free-running pipeline through an LDS ring with progress counters
//                        instead of barriers; the divides by a level's width / height in a five-instruction form (fastdiv) that is
//                        bit-identical to the IEEE sequence wherever that sequence does not rescale: 75 -> 59 ns.
// One rule all loaders obey: NOTHING that issues a global load is conditional on the loop step (clamped re-reads instead).  A load
// that only some paths through a loop issue makes the compiler's wait-count insertion assume the fewest possible younger loads at
// every later wait -- vmcnt(0..3) for registers filled iterations earlier -- and a prefetch distance of several steps silently
// collapses to one (this is why more tiles / rows in flight never changed anything in rounds 2 and 3).
// Planes must stay below 2 GB where a row offset is clamped with a signed compare; the host checks.
__device__ __forceinline__ float ld_row1(__amdgpu_buffer_rsrc_t rs, unsigned xb, unsigned row_b) {
    return __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(rs, xb, row_b, 0));
}

// Causal y sweep, one column per lane, in place.  Arguments and the state it leaves: k_vv_y_fwd1.  NST stages of YCH rows rotate
// through the registers: YCH * (NST - 1) rows in flight.
template <int NST>
__global__ __launch_bounds__(64) void k_vv_y_fwd1s(float* __restrict__ data, int h, int pitch, size_t ps, VVK k,
                                                    double* __restrict__ state, MaskL0 mk, const double* __restrict__ resume) {
    const int x = blockIdx.x * WAVE + threadIdx.x;  // pitch is a multiple of 64
    if (mask_stands(mk.keep, blockIdx.y)) return;  // (a mask plane that stands: nothing is touched)
    // level-0 mask plane: every input row is the one x-blurred row kept in the side buffer (row step 0)
    const bool side = mk.enabled && (blockIdx.y % 7 == 6);
    const float* sp = side ? mk.side + (size_t)(blockIdx.y / 7) * pitch : data + blockIdx.y * ps;
    const __amdgpu_buffer_rsrc_t rsrc = plane_rsrc(sp, side ? (size_t)pitch : ps), rdst = plane_rsrc(data + blockIdx.y * ps, ps);
    const unsigned xo = (unsigned)x * 4u, pitch_b = (unsigned)pitch * 4u, sstep = side ? 0u : pitch_b, last_off = (unsigned)(h - 1) * sstep;
    const float last = ld_row1(rsrc, xo, last_off);  // iplus, read before the sweep overwrites it
    const float x0 = ld_row1(rsrc, xo, 0);
    double v1, v2, v3;
    v1 = v2 = v3 = (double)x0 / k.sumsq;
    const size_t n = (size_t)gridDim.y * pitch, i = ystate_index(blockIdx.y, pitch, x);
    if (resume) {
        v1 = resume[i];
        v2 = resume[n + i];
        v3 = resume[2 * n + i];
    }
    unsigned lo = 0, so = 0;  // byte offsets of the next row to load / to store (wave-uniform: SGPRs)
    auto ld = [&]() {
        const float v = ld_row1(rsrc, xo, lo);
        lo = min(lo + sstep, last_off);  // past the last row the stream re-reads it (never used): the loop body stays branch-free
        return v;
    };
    auto step = [&](float xv) {
        double v0 = (double)xv;
        v0 += v1 * k.f1;
        v0 += v2 * k.f2;
        v0 += v3 * k.f3;
        v3 = v2;
        v2 = v1;
        v1 = v0;
        st_row1(rdst, xo, so, (float)v0);
        so += pitch_b;
    };
    float buf[NST][YCH];
#pragma unroll
    for (int s = 0; s < NST - 1; ++s)
#pragma unroll
        for (int u = 0; u < YCH; ++u) buf[s][u] = ld();
    int c0 = 0;
    for (; c0 + NST * YCH <= h; c0 += NST * YCH) {
#pragma unroll
        for (int s = 0; s < NST; ++s) {
#pragma unroll
            for (int u = 0; u < YCH; ++u) buf[(s + NST - 1) % NST][u] = ld();
#pragma unroll
            for (int u = 0; u < YCH; ++u) step(buf[s][u]);
        }
    }
    if (c0 < h) {  // ragged last group
#pragma unroll
        for (int s = 0; s < NST; ++s) {
#pragma unroll
            for (int u = 0; u < YCH; ++u) buf[(s + NST - 1) % NST][u] = ld();
#pragma unroll
            for (int u = 0; u < YCH; ++u)
                if (c0 + s * YCH + u < h) step(buf[s][u]);
        }
    }
    state[i] = v1;
    state[n + i] = v2;
    state[2 * n + i] = v3;
    state[3 * n + i] = (double)last;
}

// ---- chain + mover: the sweeps of a lone pair with the memory traffic on a second wavefront -------------------------------
// Measured (scripts/experiments/chain_rate.hip): the inner loop of k_vv_x_fwd alone -- 64 samples per lane from an LDS tile, 8
// double-precision operations per sample, results back into the tile -- runs at 14.4 ns per sample on a wavefront that has a
// SIMD to itself: the latency of the four dependent operations.  The kernel takes 30-31 ns per sample, with one tile in flight or
// three (more tiles in flight change nothing: it is not the HBM round trip).  The other half is what the SAME wavefront does
// around the loop to move a tile: 16 global loads, 16 + 16 LDS transposing accesses, 16 global stores, two barriers -- every one of
// them an issue slot of the one wavefront the SIMD has.  The y sweeps pay the same way: a load and a store per row next to
// eight arithmetic instructions, 39 ns per row.
// So the work is split: wavefront 0 (the chain) only runs the recurrence on LDS-resident data, wavefront 1 (the mover, on another
// SIMD of the CU) streams tiles / rows between HBM and LDS one step ahead and one step behind.  One workgroup barrier per step.
// The arithmetic and its order per sample are those of k_vv_x_fwd / k_vv_x_bwd / k_vv_y_fwd / k_vv_y_bwd.
// A whole tile is swept with compile-time bounds and the LDS reads of the next 16 samples issued ahead of the current 16's
// arithmetic: with run-time bounds every group starts with its four ds_read_b128 and waits for them -- 20.0 against 14.3 ns per
// sample for the same arithmetic (scripts/experiments/chain_rate.hip, D against A).
__device__ __forceinline__ float x_step_fwd(float x, const VVK& k, double& v1, double& v2, double& v3) {
    double v0 = (double)x;
    v0 += v1 * k.f1;
    v0 += v2 * k.f2;
    v0 += v3 * k.f3;
    v3 = v2;
    v2 = v1;
    v1 = v0;
    return (float)v0;
}
__device__ __forceinline__ float x_step_bwd(float x, const VVK& k, double& v1, double& v2, double& v3) {
    double v0 = (double)x;
    v0 *= k.sum;
    v0 += v1 * k.f1;
    v0 += v2 * k.f2;
    v0 += v3 * k.f3;
    v3 = v2;
    v2 = v1;
    v1 = v0;
    return (float)v0;
}
__device__ __forceinline__ void x_chain_fwd(float* row, int jmax, bool first_tile, const VVK& k, double& v1, double& v2, double& v3) {
    if (first_tile) v1 = v2 = v3 = (double)row[0] / k.sumsq;  // CImg.h:34909
    if (jmax == TS) {
        f4 cur[4], nxt[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) cur[q] = *reinterpret_cast<const f4*>(row + 4 * q);
#pragma unroll
        for (int g = 0; g < TS / 16; ++g) {
            if (g + 1 < TS / 16) {
#pragma unroll
                for (int q = 0; q < 4; ++q) nxt[q] = *reinterpret_cast<const f4*>(row + 16 * (g + 1) + 4 * q);
            }
#pragma unroll
            for (int q = 0; q < 4; ++q)
#pragma unroll
                for (int e = 0; e < 4; ++e) cur[q][e] = x_step_fwd(cur[q][e], k, v1, v2, v3);
#pragma unroll
            for (int q = 0; q < 4; ++q) *reinterpret_cast<f4*>(row + 16 * g + 4 * q) = cur[q];
#pragma unroll
            for (int q = 0; q < 4; ++q) cur[q] = nxt[q];
        }
        return;
    }
    for (int j = 0; j < jmax; ++j) row[j] = x_step_fwd(row[j], k, v1, v2, v3);  // the ragged last tile
}
// samples [0, jtop) of a tile from jtop-1 down to 0; last_tile: sample N-1 takes the Triggs boundary value (CImg.h:34920)
__device__ __forceinline__ void x_chain_bwd(float* row, int jtop, bool last_tile, float first, const VVK& k, double& v1, double& v2, double& v3) {
    if (jtop == TS && !last_tile) {
        f4 cur[4], nxt[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) cur[q] = *reinterpret_cast<const f4*>(row + TS - 16 + 4 * q);
#pragma unroll
        for (int g = TS / 16 - 1; g >= 0; --g) {
            if (g > 0) {
#pragma unroll
                for (int q = 0; q < 4; ++q) nxt[q] = *reinterpret_cast<const f4*>(row + 16 * (g - 1) + 4 * q);
            }
#pragma unroll
            for (int q = 3; q >= 0; --q)
#pragma unroll
                for (int e = 3; e >= 0; --e) cur[q][e] = x_step_bwd(cur[q][e], k, v1, v2, v3);
#pragma unroll
            for (int q = 0; q < 4; ++q) *reinterpret_cast<f4*>(row + 16 * g + 4 * q) = cur[q];
#pragma unroll
            for (int q = 0; q < 4; ++q) cur[q] = nxt[q];
        }
        return;
    }
    if (last_tile) {
        row[jtop - 1] = first;
        --jtop;
    }
    for (int j = jtop - 1; j >= 0; --j) row[j] = x_step_bwd(row[j], k, v1, v2, v3);
}

// x sweep, causal (FWD: in -> out, leaves v1, v2, v3, iplus of every line in `state`) or anticausal (in place, starts from the
// Triggs boundary values computed from `state`).  One workgroup = 64 lines: step s sweeps tile tt(s) (left to right / right to
// left) in LDS buffer s % 3 while the mover stores tile tt(s-1) from buffer (s-1) % 3, drops tile tt(s+1) -- fetched one step
// earlier -- into buffer (s+1) % 3 and sends the loads of tile tt(s+2).  Blocks, bands, the implicit level-0 mask: k_vv_x_fwd.
// SRC (FWD only; needs the implicit mask and per-plane bands, as k_vv_x_fwd<PX, true>): level 0 is not read from `in` but evaluated
// from the pair's frames -- the warped frame through the index plane k_src_index left in the slot of plane 0, the mosaic as a
// pure shift.  The gathers (64 four-byte loads per lane and tile) are the LOADER's: on the one wavefront of k_vv_x_fwd they sit
// on the recurrence's issue stream (460 against 250 us at 6144 x 4096, DESIGN.md round 3), here they run beside it, so a lone
// pair's level 0 is source-fused too: k_compose (a write and a re-read of six planes) never runs.
constexpr int XM_BUFS = 3;
template <bool FWD, typename PX = float, bool SRC = false>
__global__ __launch_bounds__(192) void k_vv_x_m(const float* __restrict__ in, float* __restrict__ out, int w, int pitch, long lines, VVK k,
                                               double* __restrict__ state, MaskL0 mk, Bands bd, typename CollapseSrc<PX, SRC>::type pa) {
    static_assert(FWD || !SRC, "only the causal sweep reads level 0");
    __shared__ __attribute__((aligned(16))) float tiles[XM_BUFS][TS * TP];
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
    const long blk = blockIdx.x, plane = bd.nr > 0 ? blk / bd.nr : 0;
    const int band_y0 = bd.nr > 0 ? (int)(blk % bd.nr) * TS : 0;
    const int nrows = bd.nr > 0 ? min(TS, bd.h - band_y0) : TS;
    const long line0 = bd.nr > 0 ? plane * bd.h + band_y0 : blk * TS, line = line0 + lane;
    bool gen_mask = false;       // FWD: this block's lines are rows of a level-0 mask plane, generated instead of loaded
    float* side_row = nullptr;  // !FWD: row 0 of the mask plane's first band is also left in the side buffer (see MaskL0)
    SeamDev sd;
    // (as in k_vv_x_fwd: nothing to do where every line is a line of a mask plane that stands; the whole workgroup, before any barrier)
    if (mk.keep != nullptr && (bd.nr > 0 ? mask_stands(mk.keep, plane) : __all(line >= lines || mask_stands(mk.keep, line / mk.h)))) return;
    if (mk.enabled && plane % 7 == 6) {
        if (band_y0 >= TS) return;  // rows 64.. of the step are copies of rows 0..63 and are never read (whole workgroup)
        if (FWD) {
            gen_mask = true;
            sd = mk.seam[plane / 7];
        } else
            side_row = mk.side + (size_t)(plane / 7) * pitch;
    }
    // SRC: plane, pair and first row of this block; frame channels come through the index plane, the mosaic -- and canvas a of a
    // dense pair -- are pure shifts
    const int src_q = (int)(plane % 7), src_pr = (int)(plane / 7);
    const bool gen_frame = SRC && !gen_mask && src_q < 3 && !a_is_dense(pa), gen_mosaic = SRC && !gen_mask && !gen_frame;
    const __amdgpu_buffer_rsrc_t rs = x_rsrc<PX>(pa, src_pr, src_q);
    const XShift ms = x_shift<PX>(pa, src_pr, src_q);
    const float* idx_rows = in + ((size_t)index_owner(pa, src_pr) * 7 * bd.h + band_y0) * pitch;  // rows band_y0.. of the index plane the pair reads
    const float* ib = in + (size_t)line0 * pitch;
    float* ob = out + (size_t)line0 * pitch;
    const int ntiles = (w + TS - 1) / TS;
    auto tt = [&](int s) { return FWD ? s : ntiles - 1 - s; };
    // every wavefront runs the same padded number of steps (even, and covering the storer's last tile), so that the loader's loop
    // body has no branch around its loads
    const int nsteps = (ntiles + 2) & ~1;
    if (wave == 1) {
        // The loader: two tiles travel in registers -- tile tt(s+3) is requested during step s, tile tt(s+1) dropped into its LDS
        // buffer.  SRC: the element indices of tile tt(s+4) are requested FIRST (loaded from the index plane, or computed for a
        // shift), then tile tt(s+3) is gathered through the indices requested a step earlier: loads return in order, so the wait
        // for a step's indices never stands behind the gathers issued after them.
        // NOTHING that issues a global load is conditional on the step: a load that only SOME paths through the loop issue makes
        // the compiler's wait-count insertion assume the fewest possible younger loads at every later wait, i.e. vmcnt(0..3) for
        // registers filled steps earlier, and the prefetch distance collapses to nothing.  Steps past the end fetch the last tile
        // again (never used).
        // (the mask plane's block, whose tiles are generated, runs its own copy of the loop for the same reason)
        auto loader = [&](auto GM) {
            constexpr bool GEN = decltype(GM)::value;
            f4 pre[2][16];
            f4 nidx[2][SRC && !GEN ? 16 : 1];
            auto indices = [&](int s_, f4 ni[]) {
                if constexpr (SRC && !GEN) {
                    const int s = min(s_, ntiles - 1);
                    if (gen_frame)
                        tile_load(idx_rows, pitch, s * TS, lane, ni);
                    else
                        mosaic_indices<PX>(ms, s * TS, lane, band_y0, w, ni);
                }
            };
            auto fetch = [&](int s_, const f4 ni[], f4 dst[16]) {
                const int s = min(s_, ntiles - 1);
                if constexpr (GEN) {
                    const int c = tt(s) * TS + ((lane & 15) << 2);
                    const f4 v = {mask_step(sd, c), mask_step(sd, c + 1), mask_step(sd, c + 2), mask_step(sd, c + 3)};
#pragma unroll
                    for (int i = 0; i < 16; ++i) dst[i] = v;
                } else if constexpr (SRC)
                    src_gather<PX>(rs, ni, dst);
                else
                    tile_load(ib, pitch, tt(s) * TS, lane, dst);
            };
            auto drop = [&](float* tile, f4 v[16]) {  // a fetched tile into LDS (SRC: raw bits -> the value k_compose would have stored)
                if constexpr (SRC && !GEN) src_finish<PX>(gen_frame, v);
                tile_to_lds(tile, lane, v);
            };
            indices(0, nidx[0]);
            indices(1, nidx[1]);
            fetch(0, nidx[0], pre[0]);
            fetch(1, nidx[1], pre[1]);
            indices(2, nidx[0]);
            drop(tiles[0], pre[0]);
            fetch(2, nidx[0], pre[0]);
            indices(3, nidx[1]);
            __syncthreads();
            for (int s0 = 0; s0 < nsteps; s0 += 2) {
#pragma unroll
                for (int b = 0; b < 2; ++b) {  // step s = s0 + b: tile s+1 waits in pre[1 - b], the indices of tile s+3 in nidx[1 - b]
                    const int s = s0 + b;
                    drop(tiles[(s + 1) % XM_BUFS], pre[1 - b]);  // (past the end: a copy of the last tile into a buffer the storer has emptied)
                    indices(s + 4, nidx[b]);
                    fetch(s + 3, nidx[1 - b], pre[1 - b]);
                    __syncthreads();
                }
            }
        };
        if (gen_mask)
            loader(std::true_type{});
        else
            loader(std::false_type{});
    } else if (wave == 2) {
        // the storer: tile tt(s-1) leaves its buffer during step s
        auto store = [&](int s) {
            const float* tile = tiles[s % XM_BUFS];
            const int t = tt(s);
            if (nrows == TS)
                tile_store(ob, pitch, t * TS, lane, tile);
            else
                tile_store_rows(ob, pitch, t * TS, lane, tile, nrows);  // a partial last band must not touch the next plane's rows
            if (!FWD && side_row && lane < 16) *reinterpret_cast<f4*>(side_row + t * TS + (lane << 2)) = *reinterpret_cast<const f4*>(tile + (lane << 2));
        };
        __syncthreads();
        for (int s = 0; s < nsteps; ++s) {
            if (s >= 1 && s <= ntiles) store(s - 1);
            __syncthreads();
        }
    } else {
        const bool live = lane < nrows && line < lines;
        double v1 = 0, v2 = 0, v3 = 0, iplus = 0;
        float first = 0.f;
        if (FWD) {
            if (live) {  // CImg.h:34906
                if (gen_mask)
                    iplus = (double)mask_step(sd, w - 1);
                else if (gen_frame)
                    iplus = (double)src_px<PX>(rs, true, reinterpret_cast<const unsigned*>(idx_rows)[(size_t)lane * pitch + (w - 1)]);
                else if (gen_mosaic)
                    iplus = (double)src_px<PX>(rs, false, mosaic_offset<PX>(mosaic_row<PX>(ms, band_y0 + lane), mosaic_col<PX>(ms, w - 1, w)));
                else
                    iplus = (double)in[(size_t)line * pitch + (w - 1)];
            }
        } else {
            if (live) {
                v1 = state[line];
                v2 = state[lines + line];
                v3 = state[2 * lines + line];
                iplus = state[3 * lines + line];
            }
            triggs(k, iplus, v1, v2, v3, first);
        }
        __syncthreads();
        for (int s = 0; s < nsteps; ++s) {
            if (s >= ntiles) {  // padding steps
                __syncthreads();
                continue;
            }
            float* row = tiles[s % XM_BUFS] + lane * TP;
            const int t = tt(s), n = min(TS, w - t * TS);
            if (FWD)
                x_chain_fwd(row, n, s == 0, k, v1, v2, v3);
            else
                x_chain_bwd(row, n, s == 0, first, k, v1, v2, v3);
            __syncthreads();
        }
        if (FWD && live) {
            state[line] = v1;
            state[lines + line] = v2;
            state[2 * lines + line] = v3;
            state[3 * lines + line] = iplus;
        }
    }
}

// y sweep, causal (FWD; leaves v1, v2, v3, iplus of every column in `state`, [4][planes][pitch]) or anticausal (starts from the
// Triggs boundary values computed from `state`), in place, 64 columns per workgroup.  Rows move in chunks of YM_ROWS in
// processing order (top-down / bottom-up) through a ring of four LDS slots.  Step s: the chain (lane = column) first reads chunk
// s+1 out of its slot into registers, then sweeps chunk s -- read one step earlier, so the LDS round trip is off the recurrence --
// and writes the results back to slot s % 4; the mover stores chunk s-1, drops chunk s+2 into its slot and sends the loads of
// chunk s+6 (a lane of the mover owns four columns of four rows per access: 16 bytes per lane, a row of the block = 256 contiguous
// bytes; four chunks = 64 rows in flight).  The four slots in use at step s are s-1 (being stored), s (results), s+1 (being read)
// and s+2 (being filled).
constexpr int YM_ROWS = 16, YM_SLOTS = 4;
template <bool FWD>
__global__ __launch_bounds__(192) void k_vv_y_m(float* __restrict__ data, int h, int pitch, size_t ps, VVK k, double* __restrict__ state, MaskL0 mk) {
    __shared__ __attribute__((aligned(16))) float ring[YM_SLOTS][YM_ROWS][WAVE];
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
    const int x0 = blockIdx.x * WAVE;  // pitch is a multiple of 64
    if (mask_stands(mk.keep, blockIdx.y)) return;  // (a mask plane that stands: nothing is touched; the whole workgroup, before any barrier)
    float* p = data + blockIdx.y * ps + x0;
    // level-0 mask plane, causal sweep: every input row is the one x-blurred row kept in the side buffer (row stride 0)
    const bool side = FWD && mk.enabled && (blockIdx.y % 7 == 6);
    const float* src = side ? mk.side + (size_t)(blockIdx.y / 7) * pitch + x0 : p;
    const int spitch = side ? 0 : pitch;
    const int nchunks = (h + YM_ROWS - 1) / YM_ROWS;
    // every wavefront runs the same padded number of steps (a multiple of YM_SLOTS that covers the storer's last chunk), so that the
    // loader's loop body has no branch around its loads (see k_vv_x_m's loader); past the end its rows are clamped re-reads
    const int nsteps = (nchunks + 1 + YM_SLOTS - 1) / YM_SLOTS * YM_SLOTS;
    auto yrow = [&](int i) { return FWD ? i : h - 1 - i; };  // memory row of the i-th row in processing order
    const int r4 = lane >> 4, c4 = (lane & 15) << 2;  // loader / storer: this lane's row within a group of four and its four columns
    if (wave == 1) {  // the loader
        f4 q[YM_SLOTS][YM_ROWS / 4];
        auto load = [&](int j, f4 dst[YM_ROWS / 4]) {  // rows past the end re-read the last one (never used)
#pragma unroll
            for (int m = 0; m < YM_ROWS / 4; ++m) {
                const int i = min(j * YM_ROWS + 4 * m + r4, h - 1);
                dst[m] = *reinterpret_cast<const f4*>(src + (size_t)yrow(i) * spitch + c4);
            }
        };
        auto to_ring = [&](int sl, const f4 v[YM_ROWS / 4]) {
#pragma unroll
            for (int m = 0; m < YM_ROWS / 4; ++m) *reinterpret_cast<f4*>(&ring[sl][4 * m + r4][c4]) = v[m];
        };
#pragma unroll
        for (int j = 0; j < YM_SLOTS; ++j) load(j, q[j]);
        to_ring(0, q[0]);
        to_ring(1, q[1]);
        load(YM_SLOTS, q[0]);
        load(YM_SLOTS + 1, q[1]);
        __syncthreads();
        for (int s0 = 0; s0 < nsteps; s0 += YM_SLOTS) {
#pragma unroll
            for (int b = 0; b < YM_SLOTS; ++b) {  // step s = s0 + b: chunk s+2 waits in q[(b + 2) % 4] and goes to slot (b + 2) % 4
                to_ring((b + 2) % YM_SLOTS, q[(b + 2) % YM_SLOTS]);  // (past the end: into a slot the storer emptied a step ago)
                load(s0 + b + 2 + YM_SLOTS, q[(b + 2) % YM_SLOTS]);
                __syncthreads();
            }
        }
    } else if (wave == 2) {  // the storer: chunk s-1 leaves its slot during step s
        auto store = [&](int j) {
            const int sl = j % YM_SLOTS;
            if ((j + 1) * YM_ROWS <= h) {
#pragma unroll
                for (int m = 0; m < YM_ROWS / 4; ++m)
                    *reinterpret_cast<f4*>(p + (size_t)yrow(j * YM_ROWS + 4 * m + r4) * pitch + c4) = *reinterpret_cast<const f4*>(&ring[sl][4 * m + r4][c4]);
            } else {
#pragma unroll
                for (int m = 0; m < YM_ROWS / 4; ++m) {
                    const int i = j * YM_ROWS + 4 * m + r4;
                    if (i < h) *reinterpret_cast<f4*>(p + (size_t)yrow(i) * pitch + c4) = *reinterpret_cast<const f4*>(&ring[sl][4 * m + r4][c4]);
                }
            }
        };
        __syncthreads();
        for (int s = 0; s < nsteps; ++s) {
            if (s >= 1 && s <= nchunks) store(s - 1);
            __syncthreads();
        }
    } else {
        const size_t n = (size_t)gridDim.y * pitch, si = ystate_index(blockIdx.y, pitch, x0 + lane);
        double v1 = 0, v2 = 0, v3 = 0;
        float first = 0.f, last = 0.f;
        if (FWD)
            last = src[(size_t)(h - 1) * spitch + lane];  // iplus, read before the sweep overwrites the row
        else {
            v1 = state[si];
            v2 = state[n + si];
            v3 = state[2 * n + si];
            triggs(k, state[3 * n + si], v1, v2, v3, first);
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // `last` has arrived before the mover may store anything
        __syncthreads();
        float cur[YM_ROWS], nxt[YM_ROWS];
#pragma unroll
        for (int u = 0; u < YM_ROWS; ++u) cur[u] = ring[0][u][lane], nxt[u] = 0.f;
        for (int s = 0; s < nsteps; ++s) {
            if (s >= nchunks) {  // padding steps
                __syncthreads();
                continue;
            }
            if (s + 1 < nchunks) {
                const float* c1 = &ring[(s + 1) % YM_SLOTS][0][lane];
#pragma unroll
                for (int u = 0; u < YM_ROWS; ++u) nxt[u] = c1[u * WAVE];
            }
            const int live = min(YM_ROWS, h - s * YM_ROWS);
            if (s == 0) {  // the first row in processing order starts the recurrence
                if (FWD)
                    v1 = v2 = v3 = (double)cur[0] / k.sumsq;  // CImg.h:34909; the row is then an ordinary step
                else
                    cur[0] = first;  // sample h-1 takes the Triggs boundary value and leaves the state as triggs() set it (CImg.h:34920)
#pragma unroll
                for (int u = 0; u < YM_ROWS; ++u)
                    if (u < live && (FWD || u > 0)) cur[u] = FWD ? x_step_fwd(cur[u], k, v1, v2, v3) : x_step_bwd(cur[u], k, v1, v2, v3);
            } else if (live == YM_ROWS) {
#pragma unroll
                for (int u = 0; u < YM_ROWS; ++u) cur[u] = FWD ? x_step_fwd(cur[u], k, v1, v2, v3) : x_step_bwd(cur[u], k, v1, v2, v3);
            } else {
#pragma unroll
                for (int u = 0; u < YM_ROWS; ++u)
                    if (u < live) cur[u] = FWD ? x_step_fwd(cur[u], k, v1, v2, v3) : x_step_bwd(cur[u], k, v1, v2, v3);
            }
            float* c0 = &ring[s % YM_SLOTS][0][lane];
#pragma unroll
            for (int u = 0; u < YM_ROWS; ++u) c0[u * WAVE] = cur[u];
            __syncthreads();
#pragma unroll
            for (int u = 0; u < YM_ROWS; ++u) cur[u] = nxt[u];
        }
        if (FWD) {
            state[si] = v1;
            state[n + si] = v2;
            state[2 * n + si] = v3;
            state[3 * n + si] = (double)last;
        }
    }
}

// ---- the decimation's divides by a constant ---------------------------------------------------------------------------------
// acc / W (CImg.h:29555, 29575: W = the level's width or height as a float, 2 <= W < 2^24) is an IEEE divide: on gfx950 eleven
// dependent instructions -- v_div_scale (x2), v_rcp, five multiply-adds, v_div_fmas, v_div_fixup -- of which v_div_scale writes
// and v_div_fmas reads VCC, so the twelve divides of a chunk cannot overlap where it matters and a consumer wavefront runs at the
// LATENCY of one divide after the other.  For a denominator in that range and a numerator that is +0 or has 2^-100 <= |a| <= 2^90
// the sequence never scales anything (V_DIV_SCALE returns its operand, VCC = 0, V_DIV_FMAS is a plain multiply-add, V_DIV_FIXUP
// returns the quotient with the sign it already has), and the reciprocal's refinement depends on W alone: what is left per
// divide is one multiply and four multiply-adds on values that are bit for bit those of the full sequence.  fastdiv() is that;
// div_exp() is the numerator's exponent for the range test: the smallest exponent and the largest magnitude of a chunk's
// numerators are accumulated and tested once -- a chunk with
// a numerator outside the range (denormal tails, overflow) is redone with the IEEE divide.  Compared with `/` over ALL 2^32
// numerators for a set of denominators by tests/test_gpu_parity.py::test_fastdiv_equals_ieee_divide (stitch_dev_check_fastdiv).
struct FastDiv {
    float b, r;
};
__device__ __forceinline__ FastDiv fastdiv_make(float b) {
    const float r0 = __builtin_amdgcn_rcpf(b);
    const float e = __builtin_fmaf(-b, r0, 1.0f);
    return FastDiv{b, __builtin_fmaf(e, r0, r0)};
}
__device__ __forceinline__ float fastdiv(float a, const FastDiv& d) {
    const float q = a * d.r;
    const float e1 = __builtin_fmaf(-d.b, q, a);
    const float q1 = __builtin_fmaf(e1, d.r, q);
    const float e2 = __builtin_fmaf(-d.b, q1, a);
    return __builtin_fmaf(e2, d.r, q1);
}
constexpr int FASTDIV_EMIN = -99;       // frexp exponent of 2^-100 (+0 has exponent 0, a denormal its true exponent)
constexpr float FASTDIV_AMAX = 0x1p90f;  // largest |numerator| of the short form
__device__ __forceinline__ int div_exp(float a) { return __builtin_amdgcn_frexp_expf(a); }
// The range test of one numerator.  -0 and NaN are outside by definition: the decimation's numerators are sums that start from
// +0 (never -0), and a NaN numerator means the frames held non-finite samples (the quotient is then some NaN in either form).
__device__ __forceinline__ bool fastdiv_ok(float a) { return div_exp(a) >= FASTDIV_EMIN && fabsf(a) <= FASTDIV_AMAX && __float_as_uint(a) != 0x80000000u; }
// every numerator x of 2^32 bit patterns (grid-stride), denominator w: counts where fastdiv differs from x / w although the range test passed
__global__ void k_check_fastdiv(float w, unsigned long long* __restrict__ bad, unsigned long long* __restrict__ tested) {
    const FastDiv d = fastdiv_make(w);
    unsigned long long nb = 0, nt = 0;
    for (unsigned long long i = blockIdx.x * (unsigned long long)blockDim.x + threadIdx.x; i < (1ull << 32); i += (unsigned long long)gridDim.x * blockDim.x) {
        const float a = __uint_as_float((unsigned)i);
        if (!fastdiv_ok(a)) continue;
        ++nt;
        const float q = fastdiv(a, d), ref = a / w;
        if (__float_as_uint(q) != __float_as_uint(ref)) ++nb;
    }
    if (nb) atomicAdd(bad, nb);
    atomicAdd(tested, nt);
}

// ---- anticausal y sweep + decimation as a pipeline of seven wavefronts ------------------------------------------------------
// k_vv_y_bwd_dec runs the recurrence of two columns per lane AND the row loads on one wavefront and all twelve IEEE divides of a chunk
// on a second one, one barrier per chunk: 75 ns per row with a pair alone on the chip.  Here the stages are spread over seven
// wavefronts that run free of each other: chunks of YCH rows travel through a ring of D7_SLOTS LDS slots and counters in LDS say
// how far each stage has come (release stores / acquire loads at workgroup scope, on LDS addresses: through a generic pointer
// they would also wait for every global load in flight; a stage announces a chunk one iteration after writing it, when the
// release has nothing left to wait for; all wavefronts of a
// workgroup are resident together, so every wait ends):
//   wavefront 0      the loader: rows bottom-up from HBM into a slot, 16 bytes per lane (two rows of 128 columns per access),
//                    D7_AHEAD chunks of loads in flight;
//   wavefronts 1, 2  the chains: the recurrence of 64 columns each, one per lane, in place in the slot (k_vv_y_bwd's arithmetic);
//   wavefronts 3-6   the consumers: consumer c takes chunks c, c+4, ... WHOLE -- the eight x-decimations and four y-decimations of
//                    a chunk are independent chains laid side by side -- and stores rows of the next level (k_vv_y_bwd_dec's
//                    arithmetic, CImg.h:29542-29575).  Odd heights: an output row also takes the x-decimated rows 6 and 7 of the
//                    chunk before, which the consumer recomputes from that chunk's slot (two divides more per chunk) instead of
//                    waiting for another consumer.
// Slot j % D7_SLOTS is loaded again only when chunks j - D7_SLOTS and j - D7_SLOTS + 1 have been consumed.
// ODD (source width 2 * w2 + 1): as k_vv_y_bwd_dec.
#ifndef STITCH_D7_SLOTS
#define STITCH_D7_SLOTS 8
#endif
#ifndef STITCH_D7_AHEAD
#define STITCH_D7_AHEAD 5
#endif
constexpr int D7_SLOTS = STITCH_D7_SLOTS, D7_AHEAD = STITCH_D7_AHEAD, D7_CONS = 4, D7_THREADS = (3 + D7_CONS) * WAVE;
typedef float f4a4 __attribute__((ext_vector_type(4), aligned(4)));  // 16 bytes at 4-byte alignment (ODD: a workgroup starts on an even column)
template <bool ODD>
__global__ __launch_bounds__(D7_THREADS) void k_vv_y_bwd_dec7(const float* __restrict__ data, int w, int h, int pitch, size_t ps, VVK k,
                                                             const double* __restrict__ state, float* __restrict__ dst, int w2, int h2,
                                                             int dpitch, size_t dps, unsigned long long* dbg = nullptr, int dbg_mode = 0,
                                                             const unsigned* __restrict__ keep = nullptr) {
    __shared__ __attribute__((aligned(16))) float ring[D7_SLOTS][YCH][YCOLS];
    __shared__ int cnt_loaded, cnt_chain[2], cnt_cons[D7_CONS];
    if (mask_stands(keep, blockIdx.y)) return;  // (as k_vv_y_bwd_dec: plane 6 of G_{l+1} stays as an earlier call wrote it)
    // Which wavefront plays which stage: the wavefronts of a workgroup go to the CU's four SIMDs in rotation (0, 2, 1, 3, 0, ...
    // from some start: scripts/experiments/simd_place.hip), so hardware wavefronts i and i + 4 share a SIMD and number 3 has one to
    // itself.  A chain issues one dependent instruction at a time; next to a consumer -- a wavefront full of independent vector
    // instructions -- every one of them waits for its turn at the SIMD's vector ALU (124 cycles per row against 36 alone, round 4's
    // stamps).  So: chain 0 shares with the loader (few instructions), chain 1 is alone, the consumers share two SIMDs in pairs.
    // Measured against the identity placement (-DSTITCH_D7_PLACE=0, scripts/experiments/r4_run19.sh): one pair 2.428 / 1.266 / 0.349 ms
    // against 2.436 / 1.269 / 0.350 at 6144x4096 / 4421x2315 / 1081x527 -- within the noise; kept because it costs nothing.
#ifndef STITCH_D7_PLACE
#define STITCH_D7_PLACE 1  // 0: hardware wavefront i plays stage i (A/B build)
#endif
    constexpr int stage_of[3 + D7_CONS] = {STITCH_D7_PLACE ? 1 : 0, STITCH_D7_PLACE ? 3 : 1, STITCH_D7_PLACE ? 4 : 2, STITCH_D7_PLACE ? 2 : 3,
                                           STITCH_D7_PLACE ? 0 : 4, 5, 6};
    const int wave = stage_of[__builtin_amdgcn_readfirstlane(threadIdx.x >> 6)], lane = threadIdx.x & 63;
    if (threadIdx.x == 0) {
        cnt_loaded = 0, cnt_chain[0] = cnt_chain[1] = 0;
        for (int c = 0; c < D7_CONS; ++c) cnt_cons[c] = 0;
    }
    __syncthreads();
    const int nchunks = (h + YCH - 1) / YCH;
    // diagnostics (STITCH_D7_STAMP=<level>): the middle workgroup of plane 0 records when each wavefront left each chunk
    const bool track = dbg != nullptr && blockIdx.x == gridDim.x / 2 && blockIdx.y == 0;
    auto stamp = [&](int j) {
        if (track) dbg[(size_t)wave * nchunks + j] = __builtin_amdgcn_s_memtime();
    };
    constexpr int ADV = ODD ? WAVE - 1 : WAVE;  // output columns a workgroup advances by
    const int xw = blockIdx.x * ADV * 2;        // first source column of the workgroup
    // the counters are addressed as LDS (address space 3): through a generic pointer an acquire / release would also have to
    // wait for every global load in flight (vmcnt(0)) -- on the loader that is its whole prefetch stream, once per chunk
    typedef __attribute__((address_space(3))) int lds_int;
    auto rd = [](int* p) { return __hip_atomic_load((lds_int*)p, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_WORKGROUP); };
    auto wr = [](int* p, int v) { __hip_atomic_store((lds_int*)p, v, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP); };
    if (wave == 0) {
        // lane -> row (lane >> 5) of a pair of rows, columns 4 * (lane & 31) .. +3 of the 128
        const int r2 = lane >> 5, c4 = (lane & 31) << 2;
        // a group of four columns that starts past the pitch (last workgroup) re-reads the row's last four (never used); one that
        // STRADDLES the pitch (ODD: a workgroup starts on an even column, not on a multiple of four) keeps its place -- its first
        // columns are the level's last ones -- and reads on into the next row's first floats (allocated: rows are contiguous, the
        // scratch ends in 64 slack rows), which nothing uses
        const int xc = xw + c4 < pitch ? xw + c4 : pitch - 4;
        const float* p = data + blockIdx.y * ps + xc;
        f4 q[D7_AHEAD][YCH / 2];
        int consumed = 0;  // chunks 0 .. consumed-1 are known to have been consumed
        auto load = [&](int j, f4 dst_[YCH / 2]) {
#pragma unroll
            for (int m = 0; m < YCH / 2; ++m) {
                const int i = min(j * YCH + 2 * m + r2, h - 1);  // rows past the end re-read row 0 (never used)
                dst_[m] = *reinterpret_cast<const f4a4*>(p + (size_t)(h - 1 - i) * pitch);
            }
        };
#pragma unroll
        for (int a = 0; a < D7_AHEAD; ++a) load(a, q[a]);
        for (int j0 = 0; j0 < nchunks; j0 += D7_AHEAD) {
#pragma unroll
            for (int a = 0; a < D7_AHEAD; ++a) {
                const int j = j0 + a;
                if (j < nchunks) {
                    // the slot is free when every chunk up to j - D7_SLOTS + 1 has been consumed; the counters are read only when what
                    // is known of them does not answer the question (a poll is four LDS round trips on the loader's one instruction stream)
                    while (consumed < j - D7_SLOTS + 2) {
                        const int c0 = rd(&cnt_cons[0]), c1 = rd(&cnt_cons[1]), c2 = rd(&cnt_cons[2]), c3 = rd(&cnt_cons[3]);
                        consumed = min(min(0 + D7_CONS * c0, 1 + D7_CONS * c1), min(2 + D7_CONS * c2, 3 + D7_CONS * c3));  // chunks 0 .. consumed-1 are done
                        if (consumed < j - D7_SLOTS + 2) __builtin_amdgcn_s_sleep(2);
                    }
                    // chunk j-1 is announced now, an iteration after its LDS writes went out: the release has nothing left to wait for
                    if (j >= 1) wr(&cnt_loaded, j);
                    float* sl = &ring[j % D7_SLOTS][r2][c4];
#pragma unroll
                    for (int m = 0; m < YCH / 2; ++m) *reinterpret_cast<f4*>(sl + (2 * m) * YCOLS) = q[a][m];
                    stamp(j);
                }
                // unconditional: a load that only some paths through the loop issue makes the compiler wait for everything at every
                // later use of a prefetched register (see k_vv_x_m's loader); past the end the rows are clamped re-reads
                load(j + D7_AHEAD, q[a]);
            }
        }
        wr(&cnt_loaded, nchunks);
    } else if (wave <= 2) {
        const int cw = wave - 1, x = xw + cw * WAVE + lane;
        const int xs = min(x, pitch - 1);
        double v1, v2, v3;
        float first;
        {
            const size_t n = (size_t)gridDim.y * pitch, i = ystate_index(blockIdx.y, pitch, xs);
            v1 = state[i];
            v2 = state[n + i];
            v3 = state[2 * n + i];
            triggs(k, state[3 * n + i], v1, v2, v3, first);
        }
        int loaded = 0;  // chunks 0 .. loaded-1 are known to be in their slots
        typedef __attribute__((address_space(3))) int lds_int;
        auto wait_loaded = [&](int j) {
            while (loaded < j + 1) {
                loaded = rd(&cnt_loaded);
                if (loaded < j + 1) __builtin_amdgcn_s_sleep(1);
            }
        };
        float xv[YCH], nx[YCH];
        wait_loaded(0);
#pragma unroll
        for (int u = 0; u < YCH; ++u) xv[u] = ring[0][u][cw * WAVE + lane], nx[u] = 0.f;
        // Nothing in the loop waits for an LDS round trip it has just started: the loader's progress is read (relaxed) at the top of
        // an iteration and looked at at its end; chunk j+1 leaves LDS before chunk j's arithmetic when it is known to be there;
        // chunk j-1 is announced in the MIDDLE of chunk j's rows, when its writes (and this iteration's reads) are long done, so
        // that the release finds nothing outstanding.  (LDS serves a wavefront's accesses in order, and the loader wrote its rows
        // before its counter: rows read after the counter was seen are the loader's.)
        // diagnostics (STITCH_D7_STAMP_MODE & 2): where chain 0 of the tracked workgroup spends a chunk -- sums of s_memtime differences
        const bool fine = track && (dbg_mode & 2) && cw == 0;
        unsigned long long seg[6] = {0, 0, 0, 0, 0, 0}, t_prev = 0;
        auto tick = [&](int i) {
            if (fine) {
                const unsigned long long t = __builtin_amdgcn_s_memtime();
                seg[i] += t - t_prev;
                t_prev = t;
            }
        };
        if (fine) t_prev = __builtin_amdgcn_s_memtime();
        for (int j = 0; j < nchunks; ++j) {
            tick(5);  // loop back edge + whatever the last iteration's tail left
            const int seen = __hip_atomic_load((lds_int*)&cnt_loaded, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            const bool early = j + 1 < nchunks && loaded >= j + 2;
            asm volatile("" ::: "memory");
            if (early) {
                const float* c1 = &ring[(j + 1) % D7_SLOTS][0][cw * WAVE + lane];
#pragma unroll
                for (int u = 0; u < YCH; ++u) nx[u] = c1[u * YCOLS];
            }
            const int live = min(YCH, h - j * YCH);
            auto rows = [&](int ua, int ub) {
                if (live == YCH && j > 0) {
#pragma unroll
                    for (int u = ua; u < ub; ++u) xv[u] = x_step_bwd(xv[u], k, v1, v2, v3);
                } else {
#pragma unroll
                    for (int u = ua; u < ub; ++u) {
                        if (j == 0 && u == 0)
                            xv[0] = first;  // sample h-1 takes the Triggs boundary value and leaves the state as triggs() set it (CImg.h:34920)
                        else if (u < live)
                            xv[u] = x_step_bwd(xv[u], k, v1, v2, v3);
                    }
                }
            };
            tick(0);  // counter read + the next chunk's reads issued
            rows(0, YCH / 2);
            tick(1);
            if (j >= 1) wr(&cnt_chain[cw], j);
            tick(2);
            rows(YCH / 2, YCH);
            tick(3);
            float* col = &ring[j % D7_SLOTS][0][cw * WAVE + lane];
#pragma unroll
            for (int u = 0; u < YCH; ++u) col[u * YCOLS] = xv[u];
            loaded = max(loaded, seen);
            tick(4);
            if (j + 1 < nchunks && !early) {
                wait_loaded(j + 1);
                const float* c1 = &ring[(j + 1) % D7_SLOTS][0][cw * WAVE + lane];
#pragma unroll
                for (int u = 0; u < YCH; ++u) nx[u] = c1[u * YCOLS];
            }
#pragma unroll
            for (int u = 0; u < YCH; ++u) xv[u] = nx[u];
            stamp(j);
        }
        if (fine)
            for (int i = 0; i < 6; ++i) dbg[(size_t)7 * nchunks + i] = seg[i];
        wr(&cnt_chain[cw], nchunks);
    } else {
        const int c = wave - 3;
        const float fsx = (float)(unsigned)w2, fw = (float)(unsigned)w, fh = (float)(unsigned)h, fsy = (float)(unsigned)h2;
        const bool h_odd = (h & 1) != 0;
        const int tx = blockIdx.x * ADV + lane;
        const __amdgpu_buffer_rsrc_t rdst = plane_rsrc(dst + blockIdx.y * dps, dps);
        const bool dst_live = tx < w2 && (!ODD || lane < WAVE - 1);
        const unsigned txo = dst_live ? (unsigned)tx * 4u : 0xfffffff0u;  // a dead lane's store is out of range: dropped by the descriptor
        const unsigned dpitch_b = (unsigned)dpitch * 4u;
        const float od0 = (float)(unsigned)(w2 - min(tx, w2)), od2 = (float)(unsigned)(tx + 1);  // ODD: the outer two overlap weights
        const FastDiv dw = fastdiv_make(fw), dh = fastdiv_make(fh);
        // one row of a slot -> the numerator of its x-decimated sample for this lane's output column
        auto xnum = [&](const float* r) {
            const f2 v = *reinterpret_cast<const f2*>(r + 2 * lane);
            float X = 0.f;
            if constexpr (ODD) {
                const float vn = r[lane < WAVE - 1 ? 2 * lane + 2 : 2 * lane];  // the next lane's first column
                X += v.x * od0;
                X += v.y * fsx;
                X += vn * od2;
            } else {
                X += v.x * fsx;
                X += v.y * fsx;
            }
            return X;
        };
        // output row t from the chunk's row u (source row y = 2t) and the one / two rows before it in processing order: the numerator
        auto ynum = [&](const float* E, int u, int t) {
            float a2 = 0.f;
            if (h_odd) {
                a2 += E[2 + u] * (float)(unsigned)(h2 - t);
                a2 += E[1 + u] * fsy;
                a2 += E[u] * (float)(unsigned)(t + 1);
            } else {
                a2 += E[2 + u] * fsy;
                a2 += E[1 + u] * fsy;
            }
            return a2;
        };
        int blurred = 0;  // chunks 0 .. blurred-1 are known to have left both chains
        for (int j = c; j < nchunks; j += D7_CONS) {
            while (blurred < j + 1) {
                blurred = min(rd(&cnt_chain[0]), rd(&cnt_chain[1]));
                if (blurred < j + 1) __builtin_amdgcn_s_sleep(1);
            }
            if (dbg_mode & 1) {  // diagnostics only (wrong results): the consumers do nothing but count
                wr(&cnt_cons[c], j / D7_CONS + 1);
                stamp(j);
                continue;
            }
            const float* sl = &ring[j % D7_SLOTS][0][0];
            const float* pv = &ring[(j + D7_SLOTS - 1) % D7_SLOTS][0][0];  // the chunk before (odd heights, j > 0: rows 6, 7)
            const bool prev = h_odd && j > 0;
            float N[YCH + 2], E[YCH + 2], A[YCH / 2], R[YCH / 2];
            // E[0], E[1]: x-decimated rows 6, 7 of the chunk before (odd heights); E[2 + u]: row u of this chunk
            N[0] = prev ? xnum(pv + 6 * YCOLS) : 0.f;
            N[1] = prev ? xnum(pv + 7 * YCOLS) : 0.f;
#pragma unroll
            for (int u = 0; u < YCH; ++u) N[2 + u] = xnum(sl + u * YCOLS);
            int emin = 0;
            float amax = 0.f;
#pragma unroll
            for (int u = 0; u < YCH + 2; ++u) {
                emin = min(emin, div_exp(N[u]));
                amax = fmaxf(amax, fabsf(N[u]));
                E[u] = fastdiv(N[u], dw);
            }
            const int u0 = h_odd ? 0 : 1;  // the chunk's rows that complete an output row: even u for an odd height, odd u for an even one
#pragma unroll
            for (int i = 0; i < YCH / 2; ++i) {
                const int u = u0 + 2 * i, t = (h - 1 - j * YCH - u) >> 1;
                A[i] = ynum(E, u, t);
                emin = min(emin, div_exp(A[i]));
                amax = fmaxf(amax, fabsf(A[i]));
                R[i] = fastdiv(A[i], dh);
            }
            // a numerator outside the range of the short form: the whole chunk again with the IEEE divide (wave-uniform; denormal
            // tails at the edges of the data, otherwise never)
            const bool redo = emin < FASTDIV_EMIN || !(amax <= FASTDIV_AMAX);
            if (__any(redo)) {
#pragma unroll
                for (int u = 0; u < YCH + 2; ++u) E[u] = N[u] / fw;
#pragma unroll
                for (int i = 0; i < YCH / 2; ++i) {
                    const int u = u0 + 2 * i, t = (h - 1 - j * YCH - u) >> 1;
                    R[i] = ynum(E, u, t) / fh;
                }
            }
#pragma unroll
            for (int i = 0; i < YCH / 2; ++i) {
                const int u = u0 + 2 * i, y = h - 1 - j * YCH - u, t = y >> 1;
                if (y >= 0 && t < h2) st_row1(rdst, txo, (unsigned)t * dpitch_b, R[i]);
            }
            wr(&cnt_cons[c], j / D7_CONS + 1);
            stamp(j);
        }
    }
}
