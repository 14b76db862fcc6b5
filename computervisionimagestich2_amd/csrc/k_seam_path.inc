// Part of stitch_kernels.hpp (included there, inside namespace sk): path seams (include/stitch_seam_path.h, which states the
// definitions) -- the level-0 mask plane from one column per row, and the finder: a fully parallel cost pass, then one workgroup
// per pair for the dynamic programme and the walk back.  Integers only.  Wave64, plain C++, ordinary vector loads and stores.

constexpr int SP_MAXW = 8192;     // STITCH_SEAM_PATH_MAX_WIDTH: two rows of 64-bit states for SP_MAXW + 1 columns are 131 KB of LDS
constexpr int SP_MAXK = 8;        // STITCH_SEAM_PATH_MAX_STEP
constexpr int SP_MAXM = 64;       // STITCH_SEAM_PATH_MAX_MARGIN
constexpr int SP_CT = 256;        // work-items of the cost pass: a workgroup owns one row of one pair
constexpr int SP_CPER = SP_MAXW / SP_CT;  // columns per work-item of the cost pass, at most (a 32-bit mask of flags)
constexpr int SP_DT = 1024;       // work-items of the dynamic programme
constexpr int SP_DPER = (SP_MAXW + 1 + SP_DT - 1) / SP_DT;  // states per work-item, at most
constexpr unsigned SP_WRONG = 4096;  // the weight of a pixel on the wrong side: above the largest crossing cost, 2 * 1020

// ---- the mask plane of level 0 from paths -----------------------------------------------------------------------------------------
struct PathArgs {  // up to MAXB pairs travel as a kernel argument, the way PairArgs does
    const int32_t* path[MAXB];
    int branch[MAXB];
};

// Plane 6 of level 0 of pair blockIdx.z, the full pitch (zeros beyond cw, as k_mask writes them): four columns per work-item, one
// 16-byte store.  pitch is a multiple of 64 floats and the planes start 256-byte aligned, so every store is aligned.
__global__ __launch_bounds__(256) void k_mask_path(float* __restrict__ g0_all, int cw, int pitch, size_t ps, PathArgs pa) {
    const int x = 4 * (blockIdx.x * blockDim.x + threadIdx.x), y = blockIdx.y;
    if (x >= pitch) return;
    float* m0 = g0_all + ((size_t)blockIdx.z * 7 + 6) * ps;
    const int s = pa.path[blockIdx.z][y], branch = pa.branch[blockIdx.z];
    f4 v;
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] = x + j < cw && (branch == 0 ? x + j < s : x + j >= s) ? 1.f : 0.f;
    *reinterpret_cast<f4*>(m0 + (size_t)y * pitch + x) = v;
}

// the seam records of a pathed call: zero but for the branch (stitch_plan_status_at hands them out)
__global__ void k_seam_pathed(PathArgs pa, int n, SeamDev* __restrict__ out) {
    const int i = threadIdx.x;
    if (i >= n) return;
    SeamDev s;
    s.sum_a_x = s.n_a = s.sum_ov_x = s.n_ov = 0;
    s.ratio = s.ov = 0.f;
    s.branch = pa.branch[i];
    s.start = 0;
    s.thr = 0.0;
    s.status = 0;
    s.pad = 0;
    out[i] = s;
}

// ---- the finder ------------------------------------------------------------------------------------------------------------------
struct SeamPathPair {
    const uint8_t* frame;   // fw x fh, three planes: what the warp samples
    const uint8_t* mosaic;  // mw x mh, three planes: what the move copies
    const void* cov_a;      // where a can have data: cw * ch bytes, or a bit plane (cover_bit)
    const void* cov_b;      // the same for b
    MapP map;
    float offx, offy;
    int fw, fh, mw, mh, ox, oy, branch;
};

// Coverage is a policy of this one function: bytes for the stand-alone call, a rig's bit planes otherwise.
template <bool BYTES>
__device__ __forceinline__ bool sp_covered(const void* plane, int cw, int wpr, int x, int y) {
    return BYTES ? static_cast<const uint8_t*>(plane)[(size_t)y * cw + x] != 0 : cover_bit(static_cast<const unsigned long long*>(plane), wpr, x, y);
}

// The exclusive prefix of v over the SP_CT work-items of the workgroup (in work-item order) and, in *total, the sum over all of them.
// red: 2 * (SP_CT / WAVE) words of LDS, free on entry; every work-item calls it.
__device__ __forceinline__ unsigned sp_block_scan(unsigned v, unsigned* red, unsigned* total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    unsigned inc = v;
#pragma unroll
    for (int o = 1; o < WAVE; o <<= 1) {
        const unsigned up = __shfl_up(inc, o, WAVE);
        if (lane >= o) inc += up;
    }
    if (lane == WAVE - 1) red[wave] = inc;
    __syncthreads();
    unsigned before = 0, all = 0;
#pragma unroll
    for (int w = 0; w < SP_CT / WAVE; ++w) {
        const unsigned t = red[w];
        if (w < wave) before += t;
        all += t;
    }
    __syncthreads();  // red may be written again
    *total = all;
    return before + inc - v;
}

// The costs c(y, s), s = 0 .. cw, of row blockIdx.x of pair blockIdx.y as 32-bit words: cost[(pair * ch + y) * (cw + 1) + s].
// Work-item t owns the `per` columns from t * per.  Two prefix sums over the row give the eroded masks (a window holds no
// uncovered pixel), two more the counts of L and R in front of every s; g_a comes through the warp's own map_to_src, 0 where it
// reports "outside", which is the zero-initialised canvas.
struct SeamPathLds {
    unsigned short pa_[SP_MAXW + 2], pb_[SP_MAXW + 2], dd[SP_MAXW + 2];  // prefix counts at s = 0 .. cw; d at columns -1 .. cw
    unsigned red[2 * (SP_CT / WAVE)];
};
template <bool BYTES>
__device__ __forceinline__ void seam_path_cost(const SeamPathPair& P, int cw, int ch, int wpr, int margin, unsigned* __restrict__ cost, SeamPathLds& lds) {
    unsigned short *pa_ = lds.pa_, *pb_ = lds.pb_, *dd = lds.dd;
    unsigned* red = lds.red;
    const int y = blockIdx.x, t = threadIdx.x;
    const int per = (cw + SP_CT - 1) / SP_CT, x0 = min(t * per, cw), x1 = min(x0 + per, cw);
    const size_t fpl = (size_t)P.fw * P.fh, mpl = (size_t)P.mw * P.mh;
    // ---- coverage flags of the work-item's columns, d where both cover ----
    unsigned abits = 0, bbits = 0, na = 0, nb = 0;
    if (t == 0) dd[0] = dd[cw + 1] = 0;
    for (int x = x0; x < x1; ++x) {
        const bool a = sp_covered<BYTES>(P.cov_a, cw, wpr, x, y), b = sp_covered<BYTES>(P.cov_b, cw, wpr, x, y);
        abits |= (unsigned)a << (x - x0);
        bbits |= (unsigned)b << (x - x0);
        na += !a;
        nb += !b;
        int d = 0;
        if (a && b) {
            int ga = 0, gb = 0, nx, ny;
            if (map_to_src(P.map, (float)x + P.offx, (float)y + P.offy, P.fw, P.fh, nx, ny)) {
                const size_t o = (size_t)ny * P.fw + nx;
                ga = (int)P.frame[o] + 2 * (int)P.frame[o + fpl] + (int)P.frame[o + 2 * fpl];
            }
            const long long mx = (long long)x + P.ox, my = (long long)y + P.oy;
            if (mx >= 0 && mx < P.mw && my >= 0 && my < P.mh) {
                const size_t o = (size_t)my * P.mw + (size_t)mx;
                gb = (int)P.mosaic[o] + 2 * (int)P.mosaic[o + mpl] + (int)P.mosaic[o + 2 * mpl];
            }
            d = ga > gb ? ga - gb : gb - ga;
        }
        dd[x + 1] = (unsigned short)d;
    }
    // ---- uncovered pixels in front of every column: pa_[s] = #{x < s : !A}, pb_ likewise ----
    unsigned tot;
    unsigned ea = sp_block_scan(na, red, &tot), eb = sp_block_scan(nb, red, &tot);
    if (t == 0) pa_[0] = pb_[0] = 0;
    for (int x = x0; x < x1; ++x) {
        ea += !((abits >> (x - x0)) & 1);
        eb += !((bbits >> (x - x0)) & 1);
        pa_[x + 1] = (unsigned short)ea;
        pb_[x + 1] = (unsigned short)eb;
    }
    __syncthreads();
    // ---- L and R of the work-item's columns ----
    const int branch = P.branch;
    unsigned lbits = 0, rbits = 0, nl = 0, nr = 0;
    for (int x = x0; x < x1; ++x) {
        const int lo = max(x - margin, 0), hi = min(x + margin, cw - 1) + 1;
        const bool a = (abits >> (x - x0)) & 1, b = (bbits >> (x - x0)) & 1;
        const bool ae = pa_[hi] == pa_[lo], be = pb_[hi] == pb_[lo];  // A', B': no uncovered pixel in the window
        const bool only_b = b && !ae, only_a = a && !be;
        const bool l = branch == 0 ? only_b : only_a, r = branch == 0 ? only_a : only_b;
        lbits |= (unsigned)l << (x - x0);
        rbits |= (unsigned)r << (x - x0);
        nl += l;
        nr += r;
    }
    __syncthreads();  // every window has been read: the two arrays take the counts of L and R
    unsigned tot_l, tot_r;
    unsigned el = sp_block_scan(nl, red, &tot_l), er = sp_block_scan(nr, red, &tot_r);
    for (int x = x0; x < x1; ++x) {
        el += (lbits >> (x - x0)) & 1;
        er += (rbits >> (x - x0)) & 1;
        pa_[x + 1] = (unsigned short)el;
        pb_[x + 1] = (unsigned short)er;
    }
    __syncthreads();
    // ---- c(y, s) = 4096 * (#{x < s in L} + #{x >= s in R}) + d[s - 1] + d[s] ----
    unsigned* row = cost + ((size_t)blockIdx.y * ch + y) * (size_t)(cw + 1);
    for (int s = t; s <= cw; s += SP_CT) row[s] = SP_WRONG * ((unsigned)pa_[s] + tot_r - (unsigned)pb_[s]) + (unsigned)dd[s] + (unsigned)dd[s + 1];
}

// the pairs of a device table (the stand-alone call: any number of pairs, byte masks), grid (rows, pairs)
__global__ __launch_bounds__(SP_CT) void k_seam_path_cost(const SeamPathPair* __restrict__ tab, int cw, int ch, int margin, unsigned* __restrict__ cost) {
    __shared__ SeamPathLds lds;
    seam_path_cost<true>(tab[blockIdx.y], cw, ch, 0, margin, cost, lds);
}
// the pairs of a rig's step: the m <= MAXB sets in flight, their descriptors in the kernel argument, the step's coverage as bit planes
struct SeamPathArgs {
    SeamPathPair p[MAXB];
};
__global__ __launch_bounds__(SP_CT) void k_seam_path_cost_step(SeamPathArgs a, int cw, int ch, int wpr, int margin, unsigned* __restrict__ cost) {
    __shared__ SeamPathLds lds;
    seam_path_cost<false>(a.p[blockIdx.y], cw, ch, wpr, margin, cost, lds);
}

// The temporal term of an anchored finder (include/stitch_seam_anchor.h): c_t(y, s) = c(y, s) + weight * min(|s - r[y]|, cap).
struct SeamAnchor {
    const int32_t* const* tab;  // a device table of one anchor per pair (a null entry: that pair is unanchored); or, where tab is null,
    const int32_t* base;        // ... pair i anchors on base + i * stride (null: no pair is anchored)
    size_t stride;
    unsigned weight, cap;
    unsigned long long* moved;  // pair i's `moved` goes to moved[i * moved_stride]
    size_t moved_stride;
};
// An anchor's columns as the global memory they are: a pointer that was read from a table is a flat one to the compiler, and a flat load
// waits for every LDS and memory operation in flight -- the next row's costs among them.
typedef const int32_t __attribute__((address_space(1))) * SpAnchorCols;
// r[y] folded into [-cap, cw + cap], once per row (it is uniform over the workgroup): min(|s - r|, cap) is the same for every
// s in 0 .. cw, whatever 32-bit value r has, and the per-state term stays in 32 bits.
__device__ __forceinline__ int sp_anchor_fold(int r, int cw, unsigned cap) {
    const long long lo = -(long long)cap, hi = (long long)cw + (long long)cap, v = r;  // (cap <= INT32_MAX: lo fits an int; where hi does not, no v exceeds it)
    return (int)(v < lo ? lo : v > hi ? hi : v);
}
// weight * min(|s - folded|, cap): the distance is below 2^32 (s <= 8192, folded >= -INT32_MAX), so unsigned arithmetic states it
__device__ __forceinline__ unsigned sp_anchor_term(int s, int folded, unsigned weight, unsigned cap) {
    const unsigned d = s >= folded ? (unsigned)s - (unsigned)folded : (unsigned)folded - (unsigned)s;
    return weight * min(d, cap);
}

// One workgroup per pair walks the rows.  The states D(y, .) of two rows live in LDS (dynamic: 2 * (cw + 1) 64-bit words); work-item
// t owns the states s = t, t + SP_DT, ...  Per row: the minimum of the previous row over [s - K, s + K], candidates taken in the
// order t = s, s - 1, s + 1, s - 2, ... under a strict comparison -- ties to the smallest |t - s|, then to the smaller t -- one
// byte t - s + K per state, one barrier (the row written is the one read two rows ago).  The next row's costs are loaded before
// the minimum of this one.  Then the least final state (ties to the smallest s: a 64-bit minimum over D * 2^14 + s) and the walk
// back along the bytes, by work-item 0.  Pair i's path goes to paths + i * path_stride, its cost to costs[i * cost_stride].
// With one more argument, a SeamAnchor, the anchored form: every row's cost takes the pair's temporal term, its anchor column loaded
// a row ahead like the costs, and work-item 0 sums `moved` along the walk back; a pair without an anchor runs with weight 0.  With
// no such argument the kernel is the finder as it was, instruction for instruction.
__device__ __forceinline__ SeamAnchor sp_anchor_of() { return SeamAnchor{}; }
__device__ __forceinline__ const SeamAnchor& sp_anchor_of(const SeamAnchor& a) { return a; }
template <typename... AN>
__global__ __launch_bounds__(SP_DT) void k_seam_path_dp(const unsigned* __restrict__ cost, int cw, int ch, int K, uint8_t* pred, int32_t* __restrict__ paths,
                                                        size_t path_stride, unsigned long long* __restrict__ costs, size_t cost_stride, AN... anchor) {
    constexpr bool ANCH = sizeof...(AN) != 0;
    const SeamAnchor an = sp_anchor_of(anchor...);
    extern __shared__ unsigned long long sp_state[];
    __shared__ unsigned long long best;
    const int t = threadIdx.x, ns = cw + 1;
    const size_t pair = blockIdx.x;
    const unsigned* c = cost + pair * ch * (size_t)ns;
    uint8_t* pr = pred + pair * ch * (size_t)ns;
    unsigned long long *prev = sp_state, *cur = sp_state + ns;
    SpAnchorCols r = nullptr;
    unsigned aw = 0;
    int r0 = 0, rn = 0;  // rn: the next row's column as loaded, folded where the row uses it
    if constexpr (ANCH) {
        r = (SpAnchorCols)(an.tab ? an.tab[pair] : an.base ? an.base + pair * an.stride : nullptr);
        aw = r ? an.weight : 0;
        r0 = r ? sp_anchor_fold(r[0], cw, an.cap) : 0;
        rn = r && ch > 1 ? r[1] : 0;
    }
    unsigned cn[SP_DPER];
#pragma unroll
    for (int i = 0; i < SP_DPER; ++i) {
        const int s = t + i * SP_DT;
        if (s < ns) {
            if constexpr (ANCH)
                prev[s] = c[s] + sp_anchor_term(s, r0, aw, an.cap);
            else
                prev[s] = c[s];
        }
        cn[i] = s < ns && ch > 1 ? c[(size_t)ns + s] : 0;
    }
    if (t == 0) best = ~0ull;
    __syncthreads();
    for (int y = 1; y < ch; ++y) {
        unsigned cy[SP_DPER];
#pragma unroll
        for (int i = 0; i < SP_DPER; ++i) {
            const int s = t + i * SP_DT;
            cy[i] = cn[i];
            cn[i] = s < ns && y + 1 < ch ? c[(size_t)(y + 1) * ns + s] : 0;
        }
        const int ry = rn;
        if constexpr (ANCH) rn = r && y + 1 < ch ? r[y + 1] : 0;
#pragma unroll
        for (int i = 0; i < SP_DPER; ++i) {
            const int s = t + i * SP_DT;
            if (s < ns) {
                unsigned long long m = prev[s];
                int at = 0;
                for (int k = 1; k <= K; ++k) {
                    if (s - k >= 0) {
                        const unsigned long long v = prev[s - k];
                        if (v < m) m = v, at = -k;
                    }
                    if (s + k < ns) {
                        const unsigned long long v = prev[s + k];
                        if (v < m) m = v, at = k;
                    }
                }
                if constexpr (ANCH)
                    cur[s] = m + cy[i] + sp_anchor_term(s, sp_anchor_fold(ry, cw, an.cap), aw, an.cap);
                else
                    cur[s] = m + cy[i];
                pr[(size_t)y * ns + s] = (uint8_t)(at + K);
            }
        }
        __syncthreads();
        unsigned long long* sw = prev;
        prev = cur;
        cur = sw;
    }
    unsigned long long mine = ~0ull;
#pragma unroll
    for (int i = 0; i < SP_DPER; ++i) {
        const int s = t + i * SP_DT;
        if (s < ns) mine = min(mine, (prev[s] << 14) | (unsigned long long)s);
    }
    if (mine != ~0ull) atomicMin(&best, mine);
    __syncthreads();  // the bytes of every row are written, and visible to the workgroup
    if (t == 0) {
        int s = (int)(best & 0x3fffull);
        costs[pair * cost_stride] = best >> 14;
        int32_t* path = paths + pair * path_stride;
        path[ch - 1] = s;
        if constexpr (ANCH) {
            if (r) {  // the row above's anchor column is loaded beside the byte that leads there: one wait per row, as without
                unsigned long long mv = 0;
                int ra = r[ch - 1];
                for (int y = ch - 1; y >= 1; --y) {
                    const int rb = r[y - 1];
                    const int up = (int)pr[(size_t)y * ns + s] - K;
                    mv += sp_anchor_term(s, sp_anchor_fold(ra, cw, an.cap), 1, an.cap);
                    s += up;
                    path[y - 1] = s;
                    ra = rb;
                }
                an.moved[pair * an.moved_stride] = mv + sp_anchor_term(s, sp_anchor_fold(ra, cw, an.cap), 1, an.cap);
                return;
            }
            an.moved[pair * an.moved_stride] = 0;
        }
        for (int y = ch - 1; y >= 1; --y) {
            s += (int)pr[(size_t)y * ns + s] - K;
            path[y - 1] = s;
        }
    }
}
