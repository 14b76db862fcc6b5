// Part of stitch_kernels.hpp (included there, inside namespace sk): the crop of a rig's output (include/stitch_rig_crop.h) -- the
// largest axis-aligned rectangle inside a coverage mask, and the copy of a rectangle out of many full-canvas mosaics.
//
// The search is the histogram method, one bottom row at a time: up[y][x] is the run of covered pixels that ends at (x, y) going
// up, and the best rectangle standing on row y at column x spans the columns between x's nearest STRICTLY smaller neighbours.
// Every rectangle of maximal area cannot be extended, so it is one of these candidates, and the order below (area, then the
// smallest y0, the smallest x0, the widest) picks one winner whatever the order of evaluation.  Integers only; wave64, plain C++.

// ---- the two sources of a mask ----------------------------------------------------------------------------------------------------
struct CropBytes {  // dense w x h bytes, non-zero = covered
    const uint8_t* p;
    int w;
    __device__ __forceinline__ bool at(int x, int y) const { return p[(size_t)y * w + x] != 0; }
};
struct CropBits {  // a coverage bit plane of k_rig_seams.inc, read in place
    const unsigned long long* p;
    int wpr;
    __device__ __forceinline__ bool at(int x, int y) const { return cover_bit(p, wpr, x, y); }
};

// ---- up-heights: one column per lane, rows in turn; T holds the mask's height -----------------------------------------------------
template <typename SRC, typename T>
__global__ __launch_bounds__(64) void k_crop_up(SRC src, int w, int h, T* __restrict__ up) {
    const unsigned ux = blockIdx.x * blockDim.x + threadIdx.x;
    if (ux >= (unsigned)w) return;
    const int x = (int)ux;
    unsigned run = 0;
#pragma unroll 8
    for (int y = 0; y < h; ++y) {
        run = src.at(x, y) ? run + 1u : 0u;
        up[(size_t)y * w + x] = (T)run;
    }
}

// ---- the four-key order -----------------------------------------------------------------------------------------------------------
struct CropRec {  // a rectangle as the order reads it; the height is area / rw.  area = 0: none
    int area, y0, x0, rw;
};
__device__ __forceinline__ bool crop_better(const CropRec& a, const CropRec& b) {  // a before b
    if (a.area != b.area) return a.area > b.area;
    if (a.y0 != b.y0) return a.y0 < b.y0;
    if (a.x0 != b.x0) return a.x0 < b.x0;
    return a.rw > b.rw;
}
__device__ __forceinline__ CropRec crop_wave_best(CropRec r) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const CropRec t{__shfl_xor(r.area, o, 64), __shfl_xor(r.y0, o, 64), __shfl_xor(r.x0, o, 64), __shfl_xor(r.rw, o, 64)};
        if (crop_better(t, r)) r = t;
    }
    return r;
}
// the best of a 256-lane workgroup, valid in work-item 0
__device__ __forceinline__ CropRec crop_block_best(CropRec r, CropRec* red) {
    r = crop_wave_best(r);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = r;
    __syncthreads();
    if (threadIdx.x == 0)
        for (int i = 1; i < 4; ++i)
            if (crop_better(red[i], r)) r = red[i];
    return r;
}

// ---- the per-row search -----------------------------------------------------------------------------------------------------------
// A row's heights with a hierarchy of block minima over them, four children per entry: level 0 is the row, level k + 1 holds the
// minimum of every aligned group of four of level k.  Every level is padded to a multiple of four with the largest value of T,
// which is never STRICTLY smaller than a height, so a descent needs no bounds.  off[k]: where level k starts; pad[k]: its padded
// length; about 4/3 w entries in all.
constexpr int CROP_MAXLEV = 17;  // 4^16 > 2^31 columns
struct CropLevels {
    int n;  // levels, the last one a single group of four
    unsigned long long off[CROP_MAXLEV];
    unsigned pad[CROP_MAXLEV];
};

// The nearest column left of x whose height is < v, or -1: up through the left siblings of every level until a group's minimum is
// smaller, then down to its rightmost such child.  At most three reads per level each way, whatever the row holds.
template <typename T>
__device__ __forceinline__ long long crop_left(const T* hier, const unsigned long long* off, int levels, unsigned x, unsigned v) {
    unsigned i = x;
    int lev = 0;
    for (;;) {
        bool hit = false;
        while ((i & 3u) != 0u) {
            --i;
            if (hier[off[lev] + i] < v) {
                hit = true;
                break;
            }
        }
        if (hit) break;
        if (i == 0u || lev + 1 >= levels) return -1;  // (the last level is one group, so i is 0 there: the level count only bounds the loop)
        i >>= 2;
        ++lev;
    }
    while (lev > 0) {
        --lev;
        i = i * 4u + 3u;
        while (!(hier[off[lev] + i] < v)) --i;  // the parent's minimum is < v: one of the four is
    }
    return (long long)i;
}
// The nearest column right of x whose height is < v, or w.
template <typename T>
__device__ __forceinline__ long long crop_right(const T* hier, const unsigned long long* off, const unsigned* pad, int levels, unsigned x, unsigned v,
                                                int w) {
    unsigned i = x;
    int lev = 0;
    for (;;) {
        bool hit = false;
        while ((i & 3u) != 3u) {
            ++i;
            if (hier[off[lev] + i] < v) {
                hit = true;
                break;
            }
        }
        if (hit) break;
        if (i + 1u >= pad[lev] || lev + 1 >= levels) return w;  // (likewise: i is the last entry of the last level)
        i >>= 2;
        ++lev;
    }
    while (lev > 0) {
        --lev;
        i = i * 4u;
        while (!(hier[off[lev] + i] < v)) ++i;
    }
    return (long long)i;
}

// One workgroup per bottom row (rows in turn where the grid is smaller than the mask): the row's hierarchy in LDS (IN_LDS) or, for a
// row too wide for 64 KB, in the workgroup's slice of `g_hier`; one candidate per column; the workgroup's best of all its rows goes
// to rec[blockIdx.x].
template <typename T, bool IN_LDS>
__global__ __launch_bounds__(256) void k_crop_rows(const T* __restrict__ up, int w, int h, CropLevels lv, T* __restrict__ g_hier, unsigned long long hier_len,
                                                   CropRec* __restrict__ rec) {
    extern __shared__ __attribute__((aligned(16))) unsigned char crop_smem[];
    __shared__ unsigned long long s_off[CROP_MAXLEV];
    __shared__ unsigned s_pad[CROP_MAXLEV];
    __shared__ CropRec red[4];
    T* hier;
    if constexpr (IN_LDS)
        hier = reinterpret_cast<T*>(crop_smem);
    else
        hier = g_hier + (size_t)blockIdx.x * hier_len;
    if (threadIdx.x < CROP_MAXLEV) {
        s_off[threadIdx.x] = lv.off[threadIdx.x];
        s_pad[threadIdx.x] = lv.pad[threadIdx.x];
    }
    constexpr T INF = (T)~(T)0;
    CropRec best{0, 0, 0, 0};
    for (long long yy = blockIdx.x; yy < h; yy += gridDim.x) {
        const int y = (int)yy;
        __syncthreads();  // the last row's searches are over (and the tables are there)
        const T* row = up + (size_t)y * w;
        for (unsigned i = threadIdx.x; i < lv.pad[0]; i += blockDim.x) hier[i] = i < (unsigned)w ? row[i] : INF;
        for (int k = 1; k < lv.n; ++k) {
            __syncthreads();
            const T* lo = hier + lv.off[k - 1];
            T* hi = hier + lv.off[k];
            const unsigned n = lv.pad[k - 1] / 4u;
            for (unsigned i = threadIdx.x; i < lv.pad[k]; i += blockDim.x) {
                T m = INF;
                if (i < n) {
                    const T a = lo[4u * i], b = lo[4u * i + 1u], c = lo[4u * i + 2u], d = lo[4u * i + 3u];
                    const T ab = a < b ? a : b, cd = c < d ? c : d;
                    m = ab < cd ? ab : cd;
                }
                hi[i] = m;
            }
        }
        __syncthreads();
        for (unsigned x = threadIdx.x; x < (unsigned)w; x += blockDim.x) {
            const unsigned v = hier[x];
            if (v == 0u) continue;
            const long long l = crop_left(hier, s_off, lv.n, x, v), r = crop_right(hier, s_off, s_pad, lv.n, x, v, w);
            const int rw = (int)(r - l - 1);
            const CropRec c{(int)((long long)v * rw), y - (int)v + 1, (int)(l + 1), rw};  // v <= h and rw <= w: the product fits
            if (crop_better(c, best)) best = c;
        }
    }
    __syncthreads();
    best = crop_block_best(best, red);
    if (threadIdx.x == 0) rec[blockIdx.x] = best;
}

// The best of n records, as x0, y0, w, h (all zero where nothing is covered).
__global__ __launch_bounds__(256) void k_crop_pick(const CropRec* __restrict__ rec, int n, int32_t* __restrict__ out) {
    __shared__ CropRec red[4];
    CropRec best{0, 0, 0, 0};
    for (int i = threadIdx.x; i < n; i += blockDim.x)
        if (crop_better(rec[i], best)) best = rec[i];
    best = crop_block_best(best, red);
    if (threadIdx.x == 0) {
        out[0] = best.area ? best.x0 : 0;
        out[1] = best.area ? best.y0 : 0;
        out[2] = best.area ? best.rw : 0;
        out[3] = best.area ? best.area / best.rw : 0;
    }
}

// ---- the copy: rectangle (x0, y0, rw, rh) of a W x H planar mosaic (src) to a dense rw x rh one (dst), many images per launch -------
// blockIdx.z = image, blockIdx.y = channel * rh + row (in turn where the grid is smaller).  A row whose source and destination share
// their offset within 16 bytes moves as bytes up to the boundary, 16 bytes per lane between, bytes after; any other row moves as bytes.
__global__ __launch_bounds__(256) void k_crop_many(const RigImage* __restrict__ img, int W, int H, int x0, int y0, int rw, int rh) {
    const RigImage e = img[blockIdx.z];
    for (int j = blockIdx.y; j < 3 * rh; j += gridDim.y) {
        const int c = j / rh, row = j - c * rh;
        const uint8_t* s = e.src + ((size_t)c * H + (size_t)(y0 + row)) * W + x0;
        uint8_t* d = e.dst + (size_t)j * rw;
        const unsigned sa = (unsigned)(reinterpret_cast<uintptr_t>(s) & 15u), da = (unsigned)(reinterpret_cast<uintptr_t>(d) & 15u);
        int head = rw, body = 0;  // bytes before the first boundary, 16-byte runs behind them
        if (sa == da) {
            head = min(rw, (int)((16u - sa) & 15u));
            body = (rw - head) / 16;
        }
        const int tail_at = head + 16 * body;
        for (int i = threadIdx.x; i < head; i += blockDim.x) d[i] = s[i];
        const uint4* s4 = reinterpret_cast<const uint4*>(s + head);
        uint4* d4 = reinterpret_cast<uint4*>(d + head);
        for (int i = threadIdx.x; i < body; i += blockDim.x) d4[i] = s4[i];
        for (int i = tail_at + threadIdx.x; i < rw; i += blockDim.x) d[i] = s[i];
    }
}
