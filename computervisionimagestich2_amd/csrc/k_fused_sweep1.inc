// Part of stitch_kernels.hpp (included there, inside namespace sk): the fused anticausal-x + causal-y sweep for ONE pair in flight (k_vv_xby_m).
// ---- fused anticausal x + causal y sweep of a lone pair: five wavefronts per 64-row band ------------------------------------------
// k_vv_xbyf (k_fused_sweep.inc) reads and writes a level once instead of twice, but ONE wavefront per band fetches, sweeps along x,
// waits for the band above, sweeps along y, publishes and stores: with a pair alone on the chip a tile costs that whole sequence
// (3.4 against 3.0 ms per pair at 6144 x 4096 in round 2), so a lone pair ran the two sweeps as separate launches -- 251 + 274 us at
// 6144 x 4096, both bound by their 1.4 GB.  Here the band's stages are five wavefronts that run free of each other on tiles in a
// ring of XY_BUFS LDS buffers, progress counters in LDS between them (the idiom of k_vv_y_bwd_dec7):
//   wavefront 0  the x chain: anticausal sweep of tile j, lane = row (x_chain_bwd: k_vv_x_bwd's arithmetic);
//   wavefront 1  the y chain: causal sweep of tile j, lane = column, from the state the band above left (k_vv_y_fwd's arithmetic);
//   wavefront 2  the loader: tiles right to left from HBM, two in flight in registers;
//   wavefront 3  the storer: as soon as the y chain has left tile j, publishes the band's y state of those 64 columns for the band
//                below (k_vv_xbyf's granules: the data is the flag) -- or, for the last band, leaves it where the anticausal y sweep
//                looks for it -- and then stores the tile;
//   wavefront 4  the courier: polls the granules of the band above for the tiles to come and keeps up to XY_IN states waiting in LDS.
// Neither chain touches global memory: a wait for its own stores' acknowledgements (loads and stores share one counter, and
// write-through stores take a microsecond) or a poll behind its own loads would sit on the recurrence.  Bands are claimed in
// increasing R from one counter by persistent workgroups (no residency assumption: the band a band waits for was claimed earlier
// by a workgroup that is running); every wait on another band is bounded and raises the launch's abort flag.
// Row bands of a plane follow each other at the y chain's time for one tile plus the hand-off: the launch takes about
// (NR - 1) * (0.9 us + hand-off) + NC * step.  Level-0 implicit mask, partial last band / tile: as k_vv_xbyf.
#ifndef STITCH_XY_BUFS
#define STITCH_XY_BUFS 4  // tile buffers of a band's ring (A/B builds: 2 lets three workgroups share a CU's LDS instead of two)
#endif
#ifndef STITCH_XY_WGS
#define STITCH_XY_WGS 512  // persistent workgroups of a launch: two per CU with four buffers
#endif
constexpr int XY_BUFS = STITCH_XY_BUFS, XY_IN = 2, XY_THREADS = 5 * WAVE, XY_WGS = STITCH_XY_WGS;
struct XYState {  // one tile's y state in LDS: three doubles, iplus (last band) and the passed-down mask row per column
    double u[4][WAVE];
    unsigned extra[WAVE];
};
__global__ __launch_bounds__(XY_THREADS, 3) void k_vv_xby_m(float* __restrict__ data, int w, int h, int pitch, VVK k, const double* __restrict__ state_x,
                                                        long lines, double* __restrict__ state_y, Wavefront wf, const float* __restrict__ zero_page) {
    // Zero-tile flags (wf.zt.flags != nullptr; a pair so large that its x sweeps run one wavefront per band anyway: config 5): a tile of T
    // the causal x sweep recorded as all +0.0f is not fetched -- the loader's loads go to 256 bytes of zeros instead, so that no load is
    // conditional --, and a FULL tile that is all +0.0f after both sweeps is recorded instead of stored (partial tiles are always stored).
    // The band's flags are read into LDS when the band is claimed (at most XY_MAXNC tile columns; the host checks).
    __shared__ __attribute__((aligned(16))) float tiles[XY_BUFS][TS * TP];
    __shared__ uint8_t s_zf[XY_MAXNC];
    __shared__ XYState st_in[XY_IN], st_out[2];
    __shared__ int c_loaded, c_x, c_y, c_stored, c_in, s_dead;
    __shared__ unsigned s_q;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
    const unsigned nbands = (unsigned)wf.NP * wf.NR;
    typedef __attribute__((address_space(3))) int lds_int;
    auto rd = [](int* p) { return __hip_atomic_load((lds_int*)p, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_WORKGROUP); };
    auto wr = [](int* p, int v) { __hip_atomic_store((lds_int*)p, v, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP); };
    // every wait on another wavefront of the band is bounded too: a stage that stops (a lost hand-off further up the plane) must not
    // leave the others spinning; once s_dead is set every wait falls through and the band runs out on whatever it finds
    auto wait_ge = [&](int* cnt, int& known, int need) {
        for (unsigned spins = 0; known < need; ++spins) {
            known = rd(cnt);
            if (known < need) {
                if ((spins & 63u) == 63u) {  // (not in every round: a second LDS round trip per poll doubles the time to notice)
                    if (rd(&s_dead) != 0) break;
                    if (spins > (1u << 22)) {
                        wr(&s_dead, 1);
                        break;
                    }
                }
                __builtin_amdgcn_s_sleep(1);
            }
        }
    };
    if (threadIdx.x == 0) s_dead = 0;
    for (;;) {
        if (threadIdx.x == 0) {
            s_q = atomicAdd(wf.counter, 1u);
            c_loaded = c_x = c_y = c_stored = c_in = 0;
        }
        __syncthreads();
        const unsigned q = __builtin_amdgcn_readfirstlane(s_q);
        const bool dead = __builtin_amdgcn_readfirstlane(s_dead) != 0;
        if (q >= nbands || dead) break;
        const int R = (int)(q / wf.NP), p = (int)(q % wf.NP);  // every plane's band R before any band R+1
        const int r0 = R * TS, nrows = min(TS, h - r0), NC = wf.NC;
        float* base = data + ((size_t)p * h + r0) * pitch;
        // level-0 implicit mask plane below its first band: every row equals the x-blurred row band 0 passes down with the y state
        const bool pass_row = wf.mask_l0 && (p % 7 == 6), const_rows = pass_row && R > 0;
        const unsigned tag_in = (wf.epoch << 12) | (unsigned)R, tag_out = (wf.epoch << 12) | (unsigned)(R + 1);
        // diagnostics (STITCH_XBYM_STAMP=1): the middle band of plane 0 records when each of its wavefronts left each tile
        const bool track = wf.dbg != nullptr && R == wf.NR / 2 && p == 0;
        auto stamp = [&](int j) {
            if (track) wf.dbg[(size_t)wave * NC + j] = __builtin_amdgcn_s_memtime();
        };
        auto slot_of = [&](int j) { return wf.yg + ((size_t)p * NC + (NC - 1 - j)) * WF_GRAN * WAVE; };
        const bool use_zt = wf.zt.flags != nullptr;  // wave-uniform
        if (use_zt) {
            if (!const_rows)
                for (int c = threadIdx.x; c < NC; c += XY_THREADS) s_zf[c] = wf.zt.flags[wf.zt.index(p, R, c)];
            __syncthreads();
        }
        if (wave == 0) {
            // ---- the x chain ---------------------------------------------------------------------------------------------
            if (!const_rows) {
                double v1 = 0, v2 = 0, v3 = 0;
                float first;
                {
                    const long line = (long)p * h + r0 + lane;
                    double iplus = 0;
                    if (lane < nrows) {
                        v1 = state_x[line];
                        v2 = state_x[lines + line];
                        v3 = state_x[2 * lines + line];
                        iplus = state_x[3 * lines + line];
                    }
                    triggs(k, iplus, v1, v2, v3, first);
                }
                int loaded = 0;
                for (int j = 0; j < NC; ++j) {
                    wait_ge(&c_loaded, loaded, j + 1);
                    float* row = tiles[j % XY_BUFS] + lane * TP;
                    const int c0 = (NC - 1 - j) * TS;
                    x_chain_bwd(row, min(TS, w - c0), j == 0, first, k, v1, v2, v3);
                    wr(&c_x, j + 1);
                    stamp(j);
                }
            }
        } else if (wave == 1) {
            // ---- the y chain (a band of constant rows runs its own copy of the loop: no per-sample choice of operand) ------------------
            const bool last_band = R == wf.NR - 1;
            auto ychain = [&](auto CR) {
                constexpr bool CONST = decltype(CR)::value;
                int xdone = 0, indone = 0, stored = 0;
                for (int j = 0; j < NC; ++j) {
                    float* colp = tiles[j % XY_BUFS] + lane;
                    if constexpr (!CONST)
                        wait_ge(&c_x, xdone, j + 1);
                    else
                        wait_ge(&c_stored, stored, j - XY_BUFS + 1);  // nobody else guards the buffer of a band that fetches nothing
                    double u1, u2, u3;
                    unsigned rowbits;
                    if (R == 0) {
                        const float x0 = colp[0];
                        u1 = u2 = u3 = (double)x0 / k.sumsq;  // CImg.h:34909
                        rowbits = __float_as_uint(x0);        // the x-blurred row (mask plane: identical for every y)
                    } else {
                        wait_ge(&c_in, indone, j + 1);
                        const XYState& si = st_in[j % XY_IN];
                        u1 = si.u[0][lane], u2 = si.u[1][lane], u3 = si.u[2][lane];
                        rowbits = si.extra[lane];
                    }
                    const float rowv = __uint_as_float(rowbits);
                    double iplus_y = (double)rowv;  // last band only (CImg.h:34906)
                    if constexpr (!CONST) iplus_y = (double)colp[(nrows - 1) * TP];
                    if (nrows == TS) {
                        float cur[16], nxt[16];
#pragma unroll
                        for (int u = 0; u < 16; ++u) cur[u] = CONST ? rowv : colp[u * TP], nxt[u] = rowv;
#pragma unroll
                        for (int g = 0; g < TS / 16; ++g) {
                            if constexpr (!CONST) {
                                if (g + 1 < TS / 16) {
#pragma unroll
                                    for (int u = 0; u < 16; ++u) nxt[u] = colp[(16 * (g + 1) + u) * TP];
                                }
                            }
#pragma unroll
                            for (int u = 0; u < 16; ++u) cur[u] = x_step_fwd(cur[u], k, u1, u2, u3);
#pragma unroll
                            for (int u = 0; u < 16; ++u) colp[(16 * g + u) * TP] = cur[u];
#pragma unroll
                            for (int u = 0; u < 16; ++u) cur[u] = nxt[u];
                        }
                    } else {
                        for (int r = 0; r < nrows; ++r) colp[r * TP] = x_step_fwd(CONST ? rowv : colp[r * TP], k, u1, u2, u3);
                    }
                    wait_ge(&c_stored, stored, j - 1);  // the storer has taken the state of tile j-2 out of this slot
                    XYState& so = st_out[j & 1];
                    so.u[0][lane] = u1, so.u[1][lane] = u2, so.u[2][lane] = u3;
                    if (last_band) so.u[3][lane] = iplus_y;
                    so.extra[lane] = pass_row ? rowbits : 0u;
                    wr(&c_y, j + 1);
                    stamp(j);
                }
            };
            if (const_rows)
                ychain(std::true_type{});
            else
                ychain(std::false_type{});
        } else if (wave == 2) {
            // ---- the loader: NOTHING that issues a global load is conditional on the step (see k_vv_x_m) ---------------------------
            if (!const_rows) {
                f4 pre[2][16];
                auto fetch = [&](int j_, f4 dst[16]) {
                    const int C = NC - 1 - min(j_, NC - 1);
                    const bool z = use_zt && s_zf[C] != 0;
                    tile_load(z ? zero_page : base, z ? 0 : pitch, z ? 0 : C * TS, lane, dst);
                };
                fetch(0, pre[0]);
                fetch(1, pre[1]);
                int stored = 0;
                for (int j0 = 0; j0 < NC; j0 += 2) {
#pragma unroll
                    for (int b = 0; b < 2; ++b) {
                        const int j = j0 + b;
                        if (j < NC) {
                            wait_ge(&c_stored, stored, j - XY_BUFS + 1);
                            tile_to_lds(tiles[j % XY_BUFS], lane, pre[b]);
                            wr(&c_loaded, j + 1);
                            stamp(j);
                        }
                        fetch(j + 2, pre[b]);
                    }
                }
            }
        } else if (wave == 3) {
            // ---- the storer ------------------------------------------------------------------------------------------------
            int ydone = 0;
            unsigned sent = 0;  // hand-offs of this band: full ones in the low half, zero markers in the high half (as k_vv_xbyf)
            const bool last_band = R == wf.NR - 1;
            for (int j = 0; j < NC; ++j) {
                wait_ge(&c_y, ydone, j + 1);
                const XYState& so = st_out[j & 1];
                const int c0 = (NC - 1 - j) * TS;
                if (!last_band)
                    sent += granules_publish(slot_of(j), lane, min(TS, w - c0), tag_out, so.u[0][lane], so.u[1][lane], so.u[2][lane], so.extra[lane], pass_row) ? 0x10000u : 1u;
                else {  // the state the anticausal y sweep starts from ([4][planes][pitch], as k_vv_y_fwd leaves it)
                    const size_t n = (size_t)wf.NP * pitch, i = (size_t)p * pitch + c0 + lane;
                    state_y[i] = so.u[0][lane];
                    state_y[n + i] = so.u[1][lane];
                    state_y[2 * n + i] = so.u[2][lane];
                    state_y[3 * n + i] = so.u[3][lane];
                }
                bool out_zero = false;
                if (use_zt) {
                    if (nrows == TS && c0 + TS <= w) {  // a full tile: every sample is one the level owns
                        const float* t = tiles[j % XY_BUFS] + (lane >> 4) * TP + ((lane & 15) << 2);
                        unsigned nz = 0;
#pragma unroll
                        for (int i = 0; i < 16; ++i) {
                            const f4 v = *reinterpret_cast<const f4*>(t + (4 * i) * TP);
                            nz |= __float_as_uint(v.x) | __float_as_uint(v.y) | __float_as_uint(v.z) | __float_as_uint(v.w);
                        }
                        out_zero = __ballot(nz != 0) == 0;
                    }
                    if (lane == 0) wf.zt.flags[wf.zt.index(p, R, NC - 1 - j)] = out_zero ? 1 : 0;
                }
                if (out_zero) {
                } else if (nrows == TS)
                    tile_store(base, pitch, c0, lane, tiles[j % XY_BUFS]);
                else
                    tile_store_rows(base, pitch, c0, lane, tiles[j % XY_BUFS], nrows);  // a partial last band must not touch the next plane's rows
                wr(&c_stored, j + 1);
                stamp(j);
            }
            if (lane == 0 && sent != 0) {
                atomicAdd((u64*)(wf.sticky + 2), (u64)(sent & 0xffffu));
                atomicAdd((u64*)(wf.sticky + 4), (u64)(sent >> 16));
            }
        } else if (R > 0) {
            // ---- the courier: the y state of the band above, one tile ahead of the poll it is needed by ------------------------------
            // (a plane that passes the mask row down runs its own copy of the loop: the fifth granule's load is not conditional in either)
            auto courier = [&](auto ROW) {
                constexpr bool row = decltype(ROW)::value;
                int ydone = 0;
                u64 g[2][WF_GRAN];
                granules_issue(slot_of(0), lane, g[0], row);
                bool alive = true;
                for (int j0 = 0; j0 < NC; j0 += 2) {
#pragma unroll
                    for (int b = 0; b < 2; ++b) {
                        const int j = j0 + b;
                        granules_issue(slot_of(min(j + 1, NC - 1)), lane, g[1 - b], row);  // unconditional (past the end: read again, never used)
                        if (j < NC) {
                            double a = 0, bb = 0, c = 0;
                            unsigned extra = 0;
                            if (alive && !granules_accept(g[b], tag_in, a, bb, c, extra, row)) {
                                alive = granules_consume(slot_of(j), lane, tag_in, wf.abort, wf.sticky, wf.spin_limit, a, bb, c, extra, row, true);
                                if (!alive) wr(&s_dead, 1);  // the band runs out on zeros, the workgroup ends after it
                            }
                            wait_ge(&c_y, ydone, j - XY_IN + 1);  // the y chain has left tile j - XY_IN: its slot is free
                            XYState& si = st_in[j % XY_IN];
                            si.u[0][lane] = a, si.u[1][lane] = bb, si.u[2][lane] = c;
                            si.extra[lane] = extra;
                            wr(&c_in, j + 1);
                            stamp(j);
                        }
                    }
                }
            };
            if (pass_row)
                courier(std::true_type{});
            else
                courier(std::false_type{});
        }
        __syncthreads();  // the band is done: counters and s_q are written again
    }
}
