// Part of stitch_kernels.hpp (included there, inside namespace sk): a rig's alignment monitor (include/stitch_rig_monitor.h, which
// states the record) -- the domain of a step from its coverage bit planes, and the residuals of many pairs over every integer
// shift within a radius.  Integers only: a record is the same bits whatever order its parts arrive in.  Wave64, plain C++,
// ordinary vector stores and vector atomics.

constexpr int RES_MAXR = 8;                      // STITCH_RESIDUAL_MAX_RADIUS
constexpr int RES_TW = 64, RES_TH = 32;          // a workgroup's tile of the bounding box: a wavefront is a row, a lane owns RES_PX rows
constexpr int RES_PX = RES_TH / 4;               // pixels per lane: 8 * 1 040 400 per-lane, 2048 * 1 040 400 per-tile sums fit 32 bits
constexpr int RES_PITCH = RES_TW + 2 * RES_MAXR, RES_ROWS = RES_TH + 2 * RES_MAXR;
constexpr int RES_MAXWORDS = 2 + 3 * (2 * RES_MAXR + 1) * (2 * RES_MAXR + 1);

// ---- D_k = B & erode(A, the (2r+1)^2 box), and its bounding box ------------------------------------------------------------------
// One work-item per 64-bit word of the plane.  A position outside the canvas does not constrain the erosion, so the bits past the
// width and the words past the row read as ones; B's padding bits are 0, and so are D's.  box (zeroed by the caller) takes, by
// atomicMax, {cw - min x, ch - min y, max x + 1, max y + 1} of the set bits: all zero = an empty domain.
__device__ __forceinline__ unsigned long long cover_word_ones(const unsigned long long* __restrict__ row, int wx, int wpr, int cw) {
    const unsigned long long ones = ~0ull;
    const int tail = cw & 63;
    unsigned long long cur = row[wx];
    if (wx == wpr - 1 && tail) cur |= ones << tail;
    return cur;
}
__global__ __launch_bounds__(256) void k_residual_domain(const unsigned long long* __restrict__ A, const unsigned long long* __restrict__ B, int cw, int ch,
                                                         int wpr, int r, unsigned long long* __restrict__ D, unsigned* __restrict__ box) {
    const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (size_t)wpr * ch) return;
    const int y = (int)(idx / wpr), wx = (int)(idx % wpr);
    unsigned long long e = ~0ull;
    for (int dy = -r; dy <= r; ++dy) {
        const int yy = y + dy;
        if (yy < 0 || yy >= ch) continue;
        const unsigned long long* row = A + (size_t)yy * wpr;
        const unsigned long long cur = cover_word_ones(row, wx, wpr, cw);
        const unsigned long long prev = wx > 0 ? cover_word_ones(row, wx - 1, wpr, cw) : ~0ull;
        const unsigned long long next = wx + 1 < wpr ? cover_word_ones(row, wx + 1, wpr, cw) : ~0ull;
        e &= cur;
        for (int dx = 1; dx <= r; ++dx) {
            e &= (cur >> dx) | (next << (64 - dx));  // bit x takes A[x + dx]
            e &= (cur << dx) | (prev >> (64 - dx));  // bit x takes A[x - dx]
        }
    }
    const unsigned long long d = e & B[idx];
    D[idx] = d;
    if (d) {
        const int lo = wx * 64 + __builtin_ctzll(d), hi = wx * 64 + 63 - __builtin_clzll(d);
        atomicMax(&box[0], (unsigned)(cw - lo));
        atomicMax(&box[1], (unsigned)(ch - y));
        atomicMax(&box[2], (unsigned)(hi + 1));
        atomicMax(&box[3], (unsigned)(y + 1));
    }
}

// ---- the residuals of many pairs ---------------------------------------------------------------------------------------------------
struct ResPair {
    const uint8_t* frame;     // fw x fh, three planes: what the warp samples
    const uint8_t* mosaic;    // mw x mh, three planes: what the move copies
    const void* domain;       // a bit plane (cover_bit) or cw * ch bytes
    unsigned long long* rec;  // the pair's record, zeroed before the launch
    MapP map;
    float offx, offy;
    int fw, fh, mw, mh, ox, oy;
    int x0, y0, x1, y1;  // the part of the canvas the tiles cover: the domain's bounding box inside the margin r, or that margin
};
struct ResArgs {  // up to MAXB pairs travel as a kernel argument, the way PairArgs does
    ResPair p[MAXB];
};

// The sum over a full wavefront, in lane 63: an inclusive scan by data-parallel moves inside the vector unit -- row_shr 1, 2, 4, 8
// within each row of 16 lanes, then lane 15 of every even row into the odd row above it (row_bcast:15, rows 1 and 3) and lane 31 into
// the upper half (row_bcast:31, rows 2 and 3).  A lane without a source adds 0.  Six dependent adds, no trip through the LDS crossbar:
// the shift loop runs three of these per shift, and its time was theirs while they were shuffles.  All 64 lanes must be active.
__device__ __forceinline__ unsigned res_wave_sum(unsigned v) {
    int x = (int)v;
    x += __builtin_amdgcn_update_dpp(0, x, 0x111, 0xf, 0xf, false);
    x += __builtin_amdgcn_update_dpp(0, x, 0x112, 0xf, 0xf, false);
    x += __builtin_amdgcn_update_dpp(0, x, 0x114, 0xf, 0xf, false);
    x += __builtin_amdgcn_update_dpp(0, x, 0x118, 0xf, 0xf, false);
    x += __builtin_amdgcn_update_dpp(0, x, 0x142, 0xa, 0xf, false);
    x += __builtin_amdgcn_update_dpp(0, x, 0x143, 0xc, 0xf, false);
    return (unsigned)x;
}

// A workgroup owns one RES_TW x RES_TH tile of pair blockIdx.z's box; lane l of wavefront w owns column l of rows w, w + 4, ...
// g_b and the domain bit of a lane's pixels stay in registers (g_b is 0 outside the domain, and so is the mask that g_a is ANDed
// with: such a pixel adds 0 to every sum); g_a over tile + halo r is staged in LDS as 16-bit values, one map_to_src per staged
// pixel -- the warp's own function -- and 0 where it reports "outside", which is the zero-initialised canvas.  Per shift a lane sums
// its RES_PX pixels in 32 bits, the wavefront reduces, and the four wavefronts meet in LDS; the tile's sums (below 2^32, see RES_PX)
// are added into the record by 64-bit global atomics, whose order cannot change an integer sum.
template <bool BYTES>
__device__ __forceinline__ void pairs_residual(const ResPair& P, int cw, int ch, int wpr, int r, unsigned short* ga, unsigned* red, int* any) {
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int tx0 = P.x0 + (int)blockIdx.x * RES_TW, ty0 = P.y0 + (int)blockIdx.y * RES_TH;
    if (tx0 >= P.x1 || ty0 >= P.y1) return;
    const int x = tx0 + lane;
    // ---- the domain bits of the lane's pixels; a tile without one is done ----
    unsigned bits = 0;
#pragma unroll
    for (int k = 0; k < RES_PX; ++k) {
        const int y = ty0 + wave + 4 * k;
        bool in = x < P.x1 && y < P.y1 && x >= r && x < cw - r && y >= r && y < ch - r;
        if (in) in = BYTES ? static_cast<const uint8_t*>(P.domain)[(size_t)y * cw + x] != 0 : cover_bit(static_cast<const unsigned long long*>(P.domain), wpr, x, y);
        bits |= (unsigned)in << k;
    }
    if (t == 0) *any = 0;
    __syncthreads();
    if (bits) *any = 1;
    __syncthreads();
    if (!*any) return;
    // ---- g_b of the lane's pixels ----
    int gb[RES_PX], msk[RES_PX];
    unsigned n_l = 0, sb_l = 0;
    const size_t mpl = (size_t)P.mw * P.mh;
#pragma unroll
    for (int k = 0; k < RES_PX; ++k) {
        gb[k] = 0;
        msk[k] = (bits >> k) & 1 ? 0xffff : 0;
        if (msk[k]) {
            const long long mx = (long long)x + P.ox, my = (long long)(ty0 + wave + 4 * k) + P.oy;
            if (mx >= 0 && mx < P.mw && my >= 0 && my < P.mh) {
                const size_t o = (size_t)my * P.mw + (size_t)mx;
                gb[k] = (int)P.mosaic[o] + 2 * (int)P.mosaic[o + mpl] + (int)P.mosaic[o + 2 * mpl];
            }
            ++n_l;
            sb_l += (unsigned)gb[k];
        }
    }
    // ---- g_a over the tile and its halo ----
    const int cols = RES_TW + 2 * r, rows = RES_TH + 2 * r;
    const size_t fpl = (size_t)P.fw * P.fh;
    for (int i = t; i < cols * rows; i += 256) {
        const int sy = i / cols, sx = i - sy * cols;
        const int cx = tx0 - r + sx, cy = ty0 - r + sy;
        int v = 0, nx, ny;
        if (cx >= 0 && cx < cw && cy >= 0 && cy < ch && map_to_src(P.map, (float)cx + P.offx, (float)cy + P.offy, P.fw, P.fh, nx, ny)) {
            const size_t o = (size_t)ny * P.fw + nx;
            v = (int)P.frame[o] + 2 * (int)P.frame[o + fpl] + (int)P.frame[o + 2 * fpl];
        }
        ga[sy * RES_PITCH + sx] = (unsigned short)v;
    }
    __syncthreads();
    // ---- n, sum_b, then every shift ----
    unsigned* my_red = red + wave * RES_MAXWORDS;
    n_l = res_wave_sum(n_l);
    sb_l = res_wave_sum(sb_l);
    if (lane == 63) {
        my_red[0] = n_l;
        my_red[1] = sb_l;
    }
    const unsigned short* base = ga + (wave + r) * RES_PITCH + lane + r;
    int j = 0;
    for (int dy = -r; dy <= r; ++dy)
        for (int dx = -r; dx <= r; ++dx, ++j) {
            const unsigned short* at = base + dy * RES_PITCH + dx;
            unsigned sa = 0, sd = 0, sq = 0;
#pragma unroll
            for (int k = 0; k < RES_PX; ++k) {
                const int a = (int)at[4 * k * RES_PITCH] & msk[k];
                const int d = a - gb[k];
                const unsigned ad = (unsigned)(d < 0 ? -d : d);
                sa += (unsigned)a;
                sd += ad;
                sq += ad * ad;
            }
            sa = res_wave_sum(sa);
            sd = res_wave_sum(sd);
            sq = res_wave_sum(sq);
            if (lane == 63) {
                my_red[2 + 3 * j] = sa;
                my_red[3 + 3 * j] = sd;
                my_red[4 + 3 * j] = sq;
            }
        }
    __syncthreads();
    const int words = 2 + 3 * (2 * r + 1) * (2 * r + 1);
    for (int i = t; i < words; i += 256) {
        const unsigned long long v = (unsigned long long)red[i] + red[RES_MAXWORDS + i] + red[2 * RES_MAXWORDS + i] + red[3 * RES_MAXWORDS + i];
        if (v) atomicAdd(P.rec + i, v);
    }
}

// the pairs of a device table (the stand-alone call: any number of pairs, byte masks), grid (tiles x, tiles y, pairs)
template <bool BYTES>
__global__ __launch_bounds__(256) void k_pairs_residual(const ResPair* __restrict__ tab, int cw, int ch, int wpr, int r) {
    __shared__ unsigned short ga[RES_ROWS * RES_PITCH];
    __shared__ unsigned red[4 * RES_MAXWORDS];
    __shared__ int any;
    pairs_residual<BYTES>(tab[blockIdx.z], cw, ch, wpr, r, ga, red, &any);
}
// the pairs of a rig's step: the m <= MAXB sets in flight, their descriptors in the kernel argument, the step's D_k as bits
__global__ __launch_bounds__(256) void k_pairs_residual_step(ResArgs a, int cw, int ch, int wpr, int r) {
    __shared__ unsigned short ga[RES_ROWS * RES_PITCH];
    __shared__ unsigned red[4 * RES_MAXWORDS];
    __shared__ int any;
    pairs_residual<false>(a.p[blockIdx.z], cw, ch, wpr, r, ga, red, &any);
}
