// Part of stitch_kernels.hpp (included there, inside namespace sk): the two per-image stages of a rig's replay (include/stitch_rig.h)
// for MANY same-size images per launch.  The image is one more grid dimension; per image the work is the single-image kernel's own
// device function (k_geometry.inc, k_project_lds.inc, k_equalize.inc), so arithmetic, tiling and launch arithmetic per image are
// the single-image ones and the bytes equal stitch_dev_project_u8 / stitch_dev_finish_u8.
struct RigImage {  // one entry of the device table of a many-image launch
    const uint8_t* src;
    uint8_t* dst;
};

// ---- projection: blockIdx.z = image ---------------------------------------------------------------------------------------------
template <int TW, int TH>
__global__ __launch_bounds__(256) void k_project_lds_many(const RigImage* __restrict__ img, int w, int h, float r, int lds_bytes) {
    const RigImage e = img[blockIdx.z];
    project_lds_tile<uint8_t, TW, TH>(e.src, e.dst, w, h, r, nullptr, nullptr, lds_bytes);
}
template <int TW, int TH>
__global__ __launch_bounds__(256) void k_project_lds_t_many(const RigImage* __restrict__ img, int w, int h, float r, int lds_bytes) {
    const RigImage e = img[blockIdx.z];
    project_lds_tile_t<uint8_t, TW, TH>(e.src, e.dst, w, h, r, nullptr, nullptr, lds_bytes);
}
__global__ __launch_bounds__(256) void k_project_many(const RigImage* __restrict__ img, int w, int h, int flag, int width, int height, float r) {
    const RigImage e = img[blockIdx.z];
    project_untiled<uint8_t>(e.src, e.dst, w, h, flag, width, height, r, nullptr, nullptr);
}

// ---- finish: blockIdx.y = mosaic; scratch holds 256 bins and 256 LUT entries per mosaic (bins zeroed by the host) ----------------
constexpr int RIG_EQ_WORDS = 512;
template <bool WORDS>
__global__ __launch_bounds__(HIST_WAVES * 64) void k_hist_many(const RigImage* __restrict__ img, size_t n, int32_t* __restrict__ scratch) {
    const uint8_t* p = img[blockIdx.y].dst;
    int32_t* hist = scratch + (size_t)blockIdx.y * RIG_EQ_WORDS;
    if constexpr (WORDS)
        hist_words(p, n, hist);
    else
        hist_bytes(p, n, hist);
}
__global__ __launch_bounds__(256) void k_lut_many(int32_t* __restrict__ scratch, int w, int h) {
    int32_t* hist = scratch + (size_t)blockIdx.x * RIG_EQ_WORDS;
    lut_of_hist(hist, w, h, hist + 256);
}
template <bool WORDS>
__global__ __launch_bounds__(256) void k_finish_apply_many(const RigImage* __restrict__ img, size_t n, const int32_t* __restrict__ scratch, MixK mk) {
    uint8_t* p = img[blockIdx.y].dst;
    const int32_t* lut = scratch + (size_t)blockIdx.y * RIG_EQ_WORDS + 256;
    if constexpr (WORDS)
        equalize_apply_words<true>(p, n, lut, mk);
    else
        equalize_apply_bytes<true>(p, n, lut, mk);
}
