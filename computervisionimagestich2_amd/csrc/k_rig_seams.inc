// Part of stitch_kernels.hpp (included there, inside namespace sk): fixed seams for a rig (include/stitch_rig_seams.h) -- the seam
// records of a launch sequence from integers the caller states, and coverage: where an image CAN have data, kept as bit planes.
//
// All of it is set-up work, bound by launch latency, that runs once per fix.  Wave64, plain C++, ordinary vector stores.

// ---- given seams: the records of n <= MAXB pairs from their four integers -------------------------------------------------------
struct SeamInts {  // travels as a kernel argument, the way PairArgs does
    int v[MAXB][4];  // sum_a_x, n_a, sum_ov_x, n_ov
};
// One work-item per pair writes what k_seam's last work-item would have written for these sums; k_mask, the level-0 collapse and
// the fused sweep's mask flag read the record as they read a scanned one.
__global__ __launch_bounds__(64) void k_seam_given(SeamInts g, int n, int cw, int seam_rule, SeamDev* __restrict__ out_all) {
    const int i = threadIdx.x;
    if (i < n) out_all[i] = seam_finish(g.v[i][0], g.v[i][1], g.v[i][2], g.v[i][3], seam_rule, cw);
}

// ---- coverage as bit planes -----------------------------------------------------------------------------------------------------
// One bit per pixel, rows padded to 64-bit words (`wpr` words per row): bit (x & 63) of word [y * wpr + (x >> 6)].  A wavefront
// covers 64 consecutive columns of one row, so its word is one __ballot, stored by one lane; the bits past the width are 0.
// Launch shape of the plane kernels: 256 work-items = four words of one row per workgroup, grid (ceil(wpr / 4), rows).
__device__ __forceinline__ bool cover_bit(const unsigned long long* __restrict__ plane, int wpr, int x, int y) {
    return (plane[(size_t)y * wpr + (x >> 6)] >> (x & 63)) & 1ull;
}

// C_proj: the projection's own inside test (project_untiled, k_geometry.inc: the same float expressions in the same order).
__global__ __launch_bounds__(256) void k_cover_proj(unsigned long long* __restrict__ plane, int wpr, int w, int h, int flag, int width, int height,
                                                    float r) {
    const int x = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y;
    if ((x >> 6) >= wpr) return;  // whole wavefronts
    const float dst_x = (float)((flag ? y : x) - width / 2);
    const float dst_y = (float)((flag ? x : y) - height / 2);
    const double rd = (double)r, dx = (double)dst_x;
    const float k = (float)(rd / sqrt(rd * rd + dx * dx));
    const float src_x = dst_x / k, src_y = dst_y / k;
    const float u = src_x + (float)(width / 2);
    const float v = src_y + (float)(height / 2);
    const bool in = x < w && u >= 0 && u < (float)width && v >= 0 && v < (float)height;
    const unsigned long long word = __ballot(in);
    if ((threadIdx.x & 63) == 0) plane[(size_t)y * wpr + (x >> 6)] = word;
}

// One step: A = the warp's footprint (the map of k_compose / k_warp, then the frame's own coverage at the sample), B = the moved
// mosaic's coverage, U = A | B.  Per lane one map_to_src and two word loads with a shift.
struct CoverStep {
    MapP map;
    float offx, offy;
    int fw, fh, fwpr;  // the warped frame and its C_proj plane
    int mw, mh, mwpr;  // the mosaic before the step and its coverage plane
    int ox, oy;
    int cw, ch, wpr;   // the canvas and its three planes
};
__global__ __launch_bounds__(256) void k_cover_step(CoverStep c, const unsigned long long* __restrict__ f_cov, const unsigned long long* __restrict__ m_cov,
                                                    unsigned long long* __restrict__ A, unsigned long long* __restrict__ B, unsigned long long* __restrict__ U) {
    const int x = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y;
    if ((x >> 6) >= c.wpr) return;  // whole wavefronts
    bool a = false, b = false;
    if (x < c.cw) {
        int nx, ny;
        if (map_to_src(c.map, (float)x + c.offx, (float)y + c.offy, c.fw, c.fh, nx, ny)) a = cover_bit(f_cov, c.fwpr, nx, ny);
        const long long mx = (long long)x + c.ox, my = (long long)y + c.oy;
        if (mx >= 0 && mx < c.mw && my >= 0 && my < c.mh) b = cover_bit(m_cov, c.mwpr, (int)mx, (int)my);
    }
    const unsigned long long wa = __ballot(a), wb = __ballot(b);
    if ((threadIdx.x & 63) == 0) {
        const size_t o = (size_t)y * c.wpr + (x >> 6);
        A[o] = wa;
        B[o] = wb;
        U[o] = wa | wb;
    }
}

// The reference's scan (k_seam) of the middle row over coverage: one workgroup, one column per work-item and round.
__global__ __launch_bounds__(256) void k_cover_seam(const unsigned long long* __restrict__ A, const unsigned long long* __restrict__ B, int cw, int ch,
                                                    int wpr, int seam_rule, SeamDev* __restrict__ out) {
    __shared__ int red[4][4];
    const unsigned long long* a_row = A + (size_t)(ch / 2) * wpr;
    const unsigned long long* b_row = B + (size_t)(ch / 2) * wpr;
    int s_a = 0, n_a = 0, s_o = 0, n_o = 0;
    for (int x = threadIdx.x; x < cw; x += blockDim.x) {
        const bool a_on = (a_row[x >> 6] >> (x & 63)) & 1ull, b_on = (b_row[x >> 6] >> (x & 63)) & 1ull;
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
        s_a = n_a = s_o = n_o = 0;
        for (int i = 0; i < 4; ++i) {
            s_a += red[0][i];
            n_a += red[1][i];
            s_o += red[2][i];
            n_o += red[3][i];
        }
        *out = seam_finish(s_a, n_a, s_o, n_o, seam_rule, cw);
    }
}

// A plane as bytes, 0 or 255, dense w x h (stitch_dev_rig_coverage_u8).
__global__ __launch_bounds__(256) void k_cover_bytes(const unsigned long long* __restrict__ plane, int wpr, int w, int h, uint8_t* __restrict__ out) {
    const int x = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y;
    if (x >= w) return;
    out[(size_t)y * w + x] = cover_bit(plane, wpr, x, y) ? 255 : 0;
}
