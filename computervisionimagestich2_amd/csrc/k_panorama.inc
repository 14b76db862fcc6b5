// k_panorama.inc -- the small kernels that join the feature stages on the device (include/stitch_panorama.h; host side in
// stitch_panorama.inc).  gfx950, wave64; plain loads and stores, no atomics, nothing shared between work-items.
//   k_feat_gather   a frame's feature rows in the std::map's order: descriptors and the x / y of each row's key point
//   k_pair_select   the longer-list rule of ImageProcess.cpp:185-198 on the matcher's two device lists
//   k_map_points    updateFeaturesByHomography (:622-631) on device arrays
//   k_shift_points  updateFeaturesByOffset (:633-640) on device arrays

constexpr int PANO_MAXFRAMES = 16;  // frames per launch of k_feat_gather (blockIdx.y), as the k_sift_* kernels take them
constexpr int PANO_GATHER_T = 256;  // four wavefronts = four output rows per workgroup

struct FeatGatherFrame {
    const float* desc;        // feat_desc of the SIFT call: rows in insertion order
    const int32_t* fkp;       // feat_kp: key point of each row
    const SiftKeypoint* kp;   // the key-point records
    const int32_t* index;     // map order: output row -> input row (stitch_feature_order)
    float *out_desc, *out_x, *out_y;
    int32_t n, n_rows, n_kp;  // output rows; input rows and key points written by the SIFT call
};
struct FeatGatherArgs {
    FeatGatherFrame f[PANO_MAXFRAMES];
};

// One wavefront per output row: lanes 0..31 move the 512-byte descriptor row as 16-byte loads and stores (rows start 512 bytes
// apart in buffers aligned to 256), lane 32 writes the key point's x and y.  Rows are independent.
__global__ __launch_bounds__(PANO_GATHER_T) void k_feat_gather(const FeatGatherArgs a) {
    const FeatGatherFrame& f = a.f[blockIdx.y];
    const int lane = threadIdx.x & (WAVE - 1);
    const int row = (int)blockIdx.x * (PANO_GATHER_T / WAVE) + (int)(threadIdx.x / WAVE);
    if (row >= f.n) return;
    const int src = f.index[row];
    // the index comes from the host: one outside the SIFT call's rows (or a row whose key point is outside the records) is never
    // followed.  Its output row gets a fill nobody can take for a feature -- zeros and NaN coordinates -- instead of staying as the
    // allocator left it, so that an ordering fault upstream shows in every later stage (RANSAC reports NO_CONSENSUS on NaN).
    const bool ok = src >= 0 && src < f.n_rows;
    if (lane < SIFT_DESC / 4) {
        f4 v = {0.f, 0.f, 0.f, 0.f};
        if (ok) v = reinterpret_cast<const f4*>(f.desc + (size_t)src * SIFT_DESC)[lane];
        reinterpret_cast<f4*>(f.out_desc + (size_t)row * SIFT_DESC)[lane] = v;
    } else if (lane == SIFT_DESC / 4) {
        const int k = ok ? f.fkp[src] : -1;
        const bool kp_ok = k >= 0 && k < f.n_kp;
        f.out_x[row] = kp_ok ? f.kp[k].x : __builtin_nanf("");
        f.out_y[row] = kp_ok ? f.kp[k].y : __builtin_nanf("");
    }
}

// srcToDstPair of ImageProcess.cpp:177-198 as (row of a src key point, row of a dst key point + dst_base): sd is
// getImgPair(src, dst) -- (src row, dst row) per accepted dst query -- and ds is getImgPair(dst, src) -- (dst row, src row).  sd
// itself when it is the longer list (strictly), else the mirror of ds; dstToSrcPair is the mirror of the result either way,
// which is what stitch_ransac_desc.mirror gives.  dst_base is the number of src rows where both frames' coordinates lie in one
// array and 0 where the estimation addresses the two frames' arrays separately.  Entries from the count up to `cap` are
// zeroed; no list entry at or beyond its list's count is read.
__global__ __launch_bounds__(256) void k_pair_select(const int32_t* __restrict__ sd, const int32_t* __restrict__ count_sd, int cap_sd,
                                                     const int32_t* __restrict__ ds, const int32_t* __restrict__ count_ds, int cap_ds,
                                                     int dst_base, int cap, int32_t* __restrict__ out, int32_t* __restrict__ out_count) {
    const int c_sd = min(max(*count_sd, 0), cap_sd), c_ds = min(max(*count_ds, 0), cap_ds);
    const bool use_sd = c_sd > c_ds;
    const int cnt = min(use_sd ? c_sd : c_ds, cap);
    const int gid = (int)(blockIdx.x * blockDim.x + threadIdx.x), stride = (int)(gridDim.x * blockDim.x);
    for (int m = gid; m < cap; m += stride) {
        int a = 0, b = 0;
        if (m < cnt) {
            if (use_sd) {
                a = sd[2 * m];
                b = sd[2 * m + 1] + dst_base;
            } else {
                a = ds[2 * m + 1];
                b = ds[2 * m] + dst_base;
            }
        }
        out[2 * m] = a;
        out[2 * m + 1] = b;
    }
    if (gid == 0) *out_count = cnt;
}

// `int = float` as the reference's host compiles it (cvttss2si): a value that does not fit, or NaN, gives INT_MIN
__device__ __forceinline__ int32_t point_trunc(float v) { return (v > -2147483648.0f && v < 2147483648.0f) ? (int32_t)v : INT32_MIN; }

// x' = (float)(p0 x + p1 y + p2 x y + p3) - offx, y' likewise: the map in double, rounded to float, then a float subtraction --
// the expression of map_to_src (k_geometry.inc) and of the host's stitch_map_points, term for term.
__global__ __launch_bounds__(256) void k_map_points(float* __restrict__ x, float* __restrict__ y, int32_t* __restrict__ ix,
                                                    int32_t* __restrict__ iy, int n, const MapP m, float offx, float offy) {
    const int i = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (i >= n) return;
    const double dx = (double)x[i], dy = (double)y[i];
    const float X = (float)(m.p[0] * dx + m.p[1] * dy + m.p[2] * dx * dy + m.p[3]);
    const float Y = (float)(m.p[4] * dx + m.p[5] * dy + m.p[6] * dx * dy + m.p[7]);
    const float nx = X - offx, ny = Y - offy;
    x[i] = nx;
    y[i] = ny;
    if (ix) ix[i] = point_trunc(nx);
    if (iy) iy[i] = point_trunc(ny);
}

__global__ __launch_bounds__(256) void k_shift_points(float* __restrict__ x, float* __restrict__ y, int32_t* __restrict__ ix,
                                                      int32_t* __restrict__ iy, int n, int ox, int oy) {
    const int i = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (i >= n) return;
    const float nx = x[i] - (float)ox, ny = y[i] - (float)oy;
    x[i] = nx;
    y[i] = ny;
    if (ix) ix[i] = point_trunc(nx);
    if (iy) iy[i] = point_trunc(ny);
}
