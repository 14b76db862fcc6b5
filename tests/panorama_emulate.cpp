// Host emulation of the kernels of csrc/k_panorama.inc for tests/test_panorama_host.py: the kernel source itself is compiled for
// the CPU (no FMA contraction) as a shared library and its work-items run one after the other -- none of the kernels has a
// barrier or shares anything between work-items -- so that what they compute can be compared with the Python chain and the
// library's host functions on a machine without a GPU.
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstring>
#define __device__
#define __host__
#define __global__
#define __forceinline__ inline
#define __restrict__
#define __launch_bounds__(x)
struct Dim3 {
    unsigned x, y, z;
};
static Dim3 threadIdx{0, 0, 0}, blockIdx{0, 0, 0}, blockDim{1, 1, 1}, gridDim{1, 1, 1};
using std::max;
using std::min;
constexpr int WAVE = 64;
constexpr int SIFT_DESC = 128;
struct f4 {  // the device's native 16-byte vector: the kernels only move it
    float v[4];
};
struct MapP {
    double p[8];
};
struct SiftKeypoint {  // k_sift.inc
    int32_t o, ix, iy, is;
    float x, y, s, sigma;
};
#include "k_panorama.inc"

template <typename F>
static void run_grid(unsigned gx, unsigned gy, unsigned threads, F kernel) {
    gridDim = {gx, gy, 1};
    blockDim = {threads, 1, 1};
    for (unsigned by = 0; by < gy; ++by)
        for (unsigned bx = 0; bx < gx; ++bx)
            for (unsigned t = 0; t < threads; ++t) {
                blockIdx = {bx, by, 0};
                threadIdx = {t, 0, 0};
                kernel();
            }
}

extern "C" {

// the launch of pano_select_and_fit (stitch_panorama.inc), with dst_base left to the caller
void emu_pair_select(const int32_t* sd, const int32_t* count_sd, int cap_sd, const int32_t* ds, const int32_t* count_ds, int cap_ds, int dst_base,
                     int cap, int32_t* out, int32_t* out_count) {
    run_grid((unsigned)std::min((cap + 255) / 256, 64), 1, 256, [&] { k_pair_select(sd, count_sd, cap_sd, ds, count_ds, cap_ds, dst_base, cap, out, out_count); });
}

void emu_map_points(float* x, float* y, int32_t* ix, int32_t* iy, int n, const double* p, float offx, float offy) {
    MapP m;
    std::memcpy(m.p, p, sizeof m.p);
    run_grid((unsigned)((n + 255) / 256), 1, 256, [&] { k_map_points(x, y, ix, iy, n, m, offx, offy); });
}

void emu_shift_points(float* x, float* y, int32_t* ix, int32_t* iy, int n, int ox, int oy) {
    run_grid((unsigned)((n + 255) / 256), 1, 256, [&] { k_shift_points(x, y, ix, iy, n, ox, oy); });
}

// `frames` frames with the same inputs apart from their index arrays (index + k * n per frame k), as one launch over blockIdx.y
void emu_feat_gather(const float* desc, const int32_t* fkp, const void* kp, const int32_t* index, float* out_desc, float* out_x, float* out_y, int n,
                     int n_rows, int n_kp, int frames) {
    FeatGatherArgs a;
    std::memset(&a, 0, sizeof a);
    for (int k = 0; k < frames; ++k)
        a.f[k] = FeatGatherFrame{desc, fkp, static_cast<const SiftKeypoint*>(kp), index + (size_t)k * n, out_desc + (size_t)k * n * SIFT_DESC,
                                 out_x + (size_t)k * n, out_y + (size_t)k * n, n, n_rows, n_kp};
    run_grid((unsigned)((n + PANO_GATHER_T / WAVE - 1) / (PANO_GATHER_T / WAVE)), (unsigned)frames, PANO_GATHER_T, [&] { k_feat_gather(a); });
}

int emu_max_frames(void) { return PANO_MAXFRAMES; }

// What this file declares by hand in place of stitch_kernels.hpp and k_sift.inc, for the test to hold against the real sources.
void emu_layout(int out[8]) {
    out[0] = (int)sizeof(SiftKeypoint);
    out[1] = (int)offsetof(SiftKeypoint, x);
    out[2] = (int)offsetof(SiftKeypoint, y);
    out[3] = WAVE;
    out[4] = SIFT_DESC;
    out[5] = (int)sizeof(f4);
    out[6] = (int)sizeof(MapP);
    out[7] = (int)offsetof(SiftKeypoint, sigma);
}

}  // extern "C"
