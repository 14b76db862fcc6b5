// k_calibrate.inc -- the small kernels that pool the feature stages over several captures of one rig (include/stitch_calibrate.h;
// host side in stitch_calibrate.inc).  gfx950, wave64; plain loads and stores, LDS for at most 64 values per workgroup, no
// atomics.  All three are latency-bound: a launch moves a few kilobytes at the most.
//   k_pool_counts   pooled[i][j] = the sum over captures of count_k[i][j]
//   k_pool_select   the longer-list rule of ImageProcess.cpp:185-198 on the POOLED totals, and the pooled list itself: the
//                   captures' accepted lists one behind the other, each capture's rows moved by its bases
//   k_step_support  per capture: entries of the winning inlier list that fall into the capture's segment of the pooled list

constexpr int CAL_MAXSETS = 64;  // captures per call (the LDS arrays below)

// counts: n_sets matrices of nn = n * n int32, capture-major; pooled: nn int32.  A matcher count is at most its query frame's row
// count, and the host bounds the sum of those over the captures below 2^31.
__global__ __launch_bounds__(256) void k_pool_counts(const int32_t* __restrict__ counts, int n_sets, int nn, int32_t* __restrict__ pooled) {
    const int gid = (int)(blockIdx.x * blockDim.x + threadIdx.x), stride = (int)(gridDim.x * blockDim.x);
    for (int c = gid; c < nn; c += stride) {
        int32_t sum = 0;
        for (int k = 0; k < n_sets; ++k) sum += counts[(size_t)k * nn + c];
        pooled[c] = sum;
    }
}

// One capture's share of a step (src, dst): sd = getImgPair(src, dst) of that capture, (src row, dst row) per accepted dst query;
// ds = getImgPair(dst, src).  cap_sd / cap_ds are the lists' capacities (the capture's dst / src rows); base_src / base_dst are
// where the capture's rows start in the pooled coordinate arrays of the two cameras.
struct PoolSeg {
    const int32_t *sd, *count_sd, *ds, *count_ds;
    int32_t cap_sd, cap_ds, base_src, base_dst;
};

// k_pair_select for n_sets captures at once, with its output contract: out[2m], out[2m+1] = (src row, dst row) of pooled pair m in
// the pooled arrays, zeros from the pooled count up to `cap`, *out_count the pooled count; no list entry at or beyond its list's
// count is read.  The rule is decided once, on the totals: every capture's sd list on a strict >, else the mirror of every
// capture's ds list.  Every workgroup forms the totals and the prefix of the chosen counts itself (at most 64 values, one lane;
// a second launch would cost more than the 64 additions).  seg_off (n_sets + 1 int32) receives that prefix for k_step_support.
__global__ __launch_bounds__(256) void k_pool_select(const PoolSeg* __restrict__ seg, int n_sets, int cap, int32_t* __restrict__ out,
                                                     int32_t* __restrict__ out_count, int32_t* __restrict__ seg_off) {
    __shared__ int32_t c_sd[CAL_MAXSETS], c_ds[CAL_MAXSETS], off[CAL_MAXSETS + 1];
    __shared__ int32_t use_sd_s;
    const int tid = (int)threadIdx.x;
    if (tid < n_sets) {
        c_sd[tid] = min(max(*seg[tid].count_sd, 0), seg[tid].cap_sd);
        c_ds[tid] = min(max(*seg[tid].count_ds, 0), seg[tid].cap_ds);
    }
    __syncthreads();
    if (tid == 0) {
        int t_sd = 0, t_ds = 0;
        for (int k = 0; k < n_sets; ++k) {
            t_sd += c_sd[k];
            t_ds += c_ds[k];
        }
        const bool u = t_sd > t_ds;
        int at = 0;
        off[0] = 0;
        for (int k = 0; k < n_sets; ++k) {
            at = min(at + (u ? c_sd[k] : c_ds[k]), cap);
            off[k + 1] = at;
        }
        use_sd_s = u;
    }
    __syncthreads();
    const bool use_sd = use_sd_s != 0;
    const int cnt = off[n_sets];
    const int gid = (int)(blockIdx.x * blockDim.x + threadIdx.x), stride = (int)(gridDim.x * blockDim.x);
    for (int m = gid; m < cap; m += stride) {
        int a = 0, b = 0;
        if (m < cnt) {
            int lo = 0, hi = n_sets - 1;  // the capture k with off[k] <= m < off[k + 1]: the last k with off[k] <= m
            while (lo < hi) {
                const int mid = (lo + hi + 1) >> 1;
                if (off[mid] <= m)
                    lo = mid;
                else
                    hi = mid - 1;
            }
            const PoolSeg& g = seg[lo];
            const int r = m - off[lo];
            if (use_sd) {
                a = g.sd[2 * r] + g.base_src;
                b = g.sd[2 * r + 1] + g.base_dst;
            } else {
                a = g.ds[2 * r + 1] + g.base_src;
                b = g.ds[2 * r] + g.base_dst;
            }
        }
        out[2 * m] = a;
        out[2 * m + 1] = b;
    }
    if (gid == 0) *out_count = cnt;
    if (blockIdx.x == 0 && tid <= n_sets) seg_off[tid] = off[tid];
}

// inliers: the output of stitch_dev_ransac_many for the forward map -- positions in the pooled list in increasing order, then -1;
// info: that list's info row (status, n, winning round, winning count, draws).  support: per capture {pairs the capture put into
// the pooled list, entries of the winning list inside its segment}.  The list is sorted, so a capture's entries are those between
// the lower bounds of its segment's two ends: one lane per capture, two binary searches.  One workgroup of 64.
__global__ __launch_bounds__(WAVE) void k_step_support(const int32_t* __restrict__ inliers, int n_max, const int32_t* __restrict__ info,
                                                       const int32_t* __restrict__ seg_off, int n_sets, int32_t* __restrict__ support) {
    const int k = (int)threadIdx.x;
    if (k >= n_sets) return;
    const int n_win = info[0] == RANSAC_OK ? min(max(info[3], 0), n_max) : 0;
    const int from = seg_off[k], to = seg_off[k + 1];
    int pos[2];
    for (int e = 0; e < 2; ++e) {  // the number of entries below `from` / below `to`
        const int v = e ? to : from;
        int lo = 0, hi = n_win;
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (inliers[mid] < v)
                lo = mid + 1;
            else
                hi = mid;
        }
        pos[e] = lo;
    }
    support[2 * k] = to - from;
    support[2 * k + 1] = pos[1] - pos[0];
}
