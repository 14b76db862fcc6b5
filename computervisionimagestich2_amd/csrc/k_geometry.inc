// Part of stitch_kernels.hpp (included there, inside namespace sk): cylindrical projection, the bilinear map, stand-alone warp and move (P1, P2, W1-W3).
// ---- P1: cylindrical projection, Projection.cpp:20-73 ------------------------------------------------------
// One output pixel (three channels) per work-item; r is computed on the host (tan).  Writes 0 where the
// source coordinate falls outside, so no memset pass is needed.
// (The body is a device function so that k_project_many, k_rig.inc, runs it per image of a batch: blockIdx.x / .y address the pixel.)
template <typename PX>
__device__ __forceinline__ void project_untiled(const PX* __restrict__ src, PX* __restrict__ dst, int w, int h, int flag, int width, int height,
                                                float r, uint8_t* __restrict__ gray, float* __restrict__ gray_f32) {
    const int x = blockIdx.x * blockDim.x + threadIdx.x;
    const int y = blockIdx.y;
    if (x >= w) return;
    const float dst_x = (float)((flag ? y : x) - width / 2);
    const float dst_y = (float)((flag ? x : y) - height / 2);
    const double rd = (double)r, dx = (double)dst_x;
    const float k = (float)(rd / sqrt(rd * rd + dx * dx));
    const float src_x = dst_x / k, src_y = dst_y / k;
    const float u = src_x + (float)(width / 2);
    const float v = src_y + (float)(height / 2);
    PX o[3] = {PX(0), PX(0), PX(0)};
    if (u >= 0 && u < (float)width && v >= 0 && v < (float)height) {
        if (flag)
            bilinear3<PX>(src, w, h, v, u, o);
        else
            bilinear3<PX>(src, w, h, u, v, o);
    }
    const size_t pl = (size_t)w * h, off = (size_t)y * w + x;
    dst[off] = o[0];
    dst[off + pl] = o[1];
    dst[off + 2 * pl] = o[2];
    if (sizeof(PX) == 1 && (gray || gray_f32)) {  // readFile's next step on the same pixel (ImageProcess.cpp:20)
        const uint8_t v = gray_ref((uint8_t)o[0], (uint8_t)o[1], (uint8_t)o[2]);
        if (gray) gray[off] = v;
        if (gray_f32) gray_f32[off] = (float)v;
    }
}
template <typename PX>
__global__ __launch_bounds__(256) void k_project(const PX* __restrict__ src, PX* __restrict__ dst, int w, int h,
                                                 int flag, int width, int height, float r, uint8_t* __restrict__ gray,
                                                 float* __restrict__ gray_f32) {
    project_untiled<PX>(src, dst, w, h, flag, width, height, r, gray, gray_f32);
}

// ---- W1: the bilinear map, ImageProcess.cpp:465-471 --------------------------------------------------------
// double: ((p0*x + p1*y) + (p2*x)*y) + p3, rounded to float; then `int newX = float` truncation.  Values that
// do not fit an int (x86 gives INT_MIN, which fails the range test) and NaN are reported as "outside".
__device__ __forceinline__ bool map_to_src(const MapP& m, float fx, float fy, int sw, int sh, int& nx, int& ny) {
    const double dx = (double)fx, dy = (double)fy;
    const float X = (float)(m.p[0] * dx + m.p[1] * dy + m.p[2] * dx * dy + m.p[3]);
    const float Y = (float)(m.p[4] * dx + m.p[5] * dy + m.p[6] * dx * dy + m.p[7]);
    if (!(X > -2147483648.0f && X < 2147483648.0f) || !(Y > -2147483648.0f && Y < 2147483648.0f)) return false;
    nx = (int)X;
    ny = (int)Y;
    return nx >= 0 && nx < sw && ny >= 0 && ny < sh;
}

// The degenerate bilinear call of the warp (ImageProcess.cpp:602): a = b = 0, so the value is
// ((1*1)*ld + (0*1)*rd + (0*0)*rt + (1*0)*lt) = ld*1 + rd*0 + rt*0 + lt*0 with all four taps = ld.
// For every float that expression equals 0*ld + ld rounded once: a finite ld gives 1*ld = ld and 0*ld = a zero of ld's sign,
// and ld plus zeros of its own sign is ld (-0 included); an infinite or NaN ld gives NaN either way.  One v_fma_f32 instead
// of seven operations -- the causal x sweep and the collapse of a source-fused level 0 evaluate it for every sample, and the
// sweep is bound by instruction issue.
__device__ __forceinline__ float warp_tap(float ld) { return __builtin_fmaf(0.f, ld, ld); }
// px_store<PX>(warp_tap(t)) as a float, t a sample of a PX frame: a byte value comes through both steps unchanged
template <typename PX>
__device__ __forceinline__ float warped_px(float t);
template <>
__device__ __forceinline__ float warped_px<float>(float t) {
    return warp_tap(t);
}
template <>
__device__ __forceinline__ float warped_px<uint8_t>(float t) {
    return t;
}

// ---- W2 / W3 stand-alone (read-modify-write canvases of the C++ seam) ---------------------------------------
template <typename PX>
__global__ __launch_bounds__(256) void k_warp(const PX* __restrict__ src, int sw, int sh, MapP m, float offx,
                                              float offy, PX* __restrict__ canvas, int cw, int ch) {
    const int x = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y;
    if (x >= cw) return;
    int nx, ny;
    if (!map_to_src(m, (float)x + offx, (float)y + offy, sw, sh, nx, ny)) return;
    const size_t spl = (size_t)sw * sh, so = (size_t)ny * sw + nx, cpl = (size_t)cw * ch, co = (size_t)y * cw + x;
#pragma unroll
    for (int c = 0; c < 3; ++c) canvas[co + c * cpl] = px_store<PX>(warp_tap((float)src[so + c * spl]));
}

template <typename PX>
__global__ __launch_bounds__(256) void k_move(const PX* __restrict__ src, int sw, int sh, int ox, int oy,
                                              PX* __restrict__ canvas, int cw, int ch) {
    const int x = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y;
    if (x >= cw) return;
    const long long nx = (long long)x + ox, ny = (long long)y + oy;
    if (nx < 0 || nx >= sw || ny < 0 || ny >= sh) return;
    const size_t spl = (size_t)sw * sh, so = (size_t)ny * sw + nx, cpl = (size_t)cw * ch, co = (size_t)y * cw + x;
#pragma unroll
    for (int c = 0; c < 3; ++c) canvas[co + c * cpl] = src[so + c * spl];
}
