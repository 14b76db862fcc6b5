// Part of stitch_kernels.hpp (included there, inside namespace sk, after k_exposure.inc and k_rig.inc): the six kernels of the
// colour transfer for MANY images per launch (include/stitch_rig_exposure.h, DESIGN.md 15), and behind them the two kernels of
// include/stitch_rig_exposure_temporal.h (DESIGN.md 24).  k_exposure.inc's kernels take up to
// six planes by value in an ExArgs; these read a device table instead, and the plane (or the image) is one more grid dimension.
// Per plane and per image the work is the single-image kernel's own device function (tr_to_lab_image, tr_stats_chain,
// ex_span_sum_plane, ex_span_map_plane, ex_walk_plane, ex_apply_image), so no arithmetic is stated here and the bytes, the
// statistics' bits and the counters equal stitch_dev_transfer_form_u8's per image.  No workgroup waits for another.
struct ExPlane {  // one float plane and where its two statistics go
    const float* p;
    unsigned long long n;
    float* mean;  // one float each; pass 2 reads what pass 1 wrote
    float* sd;
    float cnt;
    uint32_t pad;
};
struct ExImage {  // one image of a transfer: a source (out and stats set) or a template (both null)
    const uint8_t* src;
    float* lab;  // 3 * n floats
    uint8_t* out;
    const float* stats;  // the twelve statistics of this source and its template
    unsigned long long n;
};

// blockIdx.y = image; the x dimension is sized for the largest image, and a smaller image's surplus workgroups find i >= n at once
__global__ __launch_bounds__(256) void k_tr_to_lab_many(const ExImage* __restrict__ img, TrK k) {
    const ExImage e = img[blockIdx.y];
    tr_to_lab_image(e.src, (size_t)e.n, k, e.lab);
}

// blockIdx.x = plane
__global__ __launch_bounds__(64) void k_ex_stats_serial_many(const ExPlane* __restrict__ planes) {
    __shared__ __attribute__((aligned(16))) float buf[2][256];
    const ExPlane e = planes[blockIdx.x];
    tr_stats_chain(e.p, (size_t)e.n, e.cnt, e.mean, e.sd, buf);
}

// blockIdx.y = plane, blockIdx.x = span: the grid is sized by the longest plane, a shorter plane's surplus workgroups return at
// once (b >= n in the device functions).  sums[plane * max_spans + span], table likewise.
__global__ __launch_bounds__(EX_T) void k_ex_span_sums_many(const ExPlane* __restrict__ planes, int pass, int max_spans, double* __restrict__ sums) {
    __shared__ ExShared sh;
    const ExPlane e = planes[blockIdx.y];
    ex_span_sum_plane(sh, e.p, (size_t)e.n, e.mean, pass, (int)blockIdx.x, sums + (size_t)blockIdx.y * max_spans);
}
__global__ __launch_bounds__(EX_T) void k_ex_span_maps_many(const ExPlane* __restrict__ planes, int pass, int max_spans, const double* __restrict__ sums,
                                                            ExSpanEntry* __restrict__ table) {
    __shared__ ExShared sh;
    const ExPlane e = planes[blockIdx.y];
    ex_span_map_plane(sh, e.p, (size_t)e.n, e.mean, pass, (int)blockIdx.x, sums + (size_t)blockIdx.y * max_spans, table + (size_t)blockIdx.y * max_spans);
}

// blockIdx.x = plane.  table == nullptr: form 1, both passes in this launch.
__global__ __launch_bounds__(EX_T) void k_ex_walk_many(const ExPlane* __restrict__ planes, int pass, int max_spans, const ExSpanEntry* __restrict__ table,
                                                       uint32_t* __restrict__ diag_out) {
    __shared__ ExShared sh;
    const ExPlane e = planes[blockIdx.x];
    ex_walk_plane(sh, e.p, (size_t)e.n, e.cnt, e.mean, e.sd, pass, table ? table + (size_t)blockIdx.x * max_spans : nullptr,
                  diag_out ? diag_out + (size_t)blockIdx.x * EX_DIAG_N : nullptr);
}

// blockIdx.y = source image: entry blockIdx.y * every of the table (sources and templates alternate in it, every = 2)
__global__ __launch_bounds__(256) void k_ex_apply_many(const ExImage* __restrict__ img, int every, TrK k, int keep_black) {
    const ExImage e = img[(size_t)blockIdx.y * every];
    ex_apply_image(e.lab, (size_t)e.n, e.stats, k, keep_black ? e.src : nullptr, e.out);
}

// ---- include/stitch_rig_exposure_temporal.h (DESIGN.md 24) ----------------------------------------------------------------------
// The apply with GIVEN statistics: source bytes in, recoloured bytes out, no lab plane in between.  One pixel is tr_rgb_to_lab, the
// line of ex_apply_image and tr_lab_to_rgb -- the values tr_to_lab_image would have stored as floats are floats in registers here,
// so the bytes are k_ex_apply_many's on k_tr_to_lab_many's planes.
struct ExGiven {  // one image of an apply with given statistics
    const uint8_t* src;
    uint8_t* out;  // may be src: a work-item reads its pixels before it writes them, and no other work-item touches them
};
__device__ __forceinline__ void ex_given_pixel(const TrK& k, const float (&st)[12], int keep_black, uint32_t r, uint32_t g, uint32_t b, uint32_t& ro, uint32_t& go,
                                               uint32_t& bo) {
    float x[3], v[3], R, G, B;
    tr_rgb_to_lab(k, (float)r, (float)g, (float)b, x[0], x[1], x[2]);
#pragma unroll
    for (int c = 0; c < 3; ++c) v[c] = (x[c] - st[c]) * st[9 + c] / st[3 + c] + st[6 + c];  // transfer.cpp:168-170, as ex_apply_image
    tr_lab_to_rgb(k, v[0], v[1], v[2], R, G, B);
    const bool black = keep_black && (r | g | b) == 0;
    ro = black ? 0u : (uint32_t)px_store<uint8_t>(R);
    go = black ? 0u : (uint32_t)px_store<uint8_t>(G);
    bo = black ? 0u : (uint32_t)px_store<uint8_t>(B);
}
// blockIdx.y = image, every image of n pixels.  Where n is a multiple of 4 and both bases are 4-byte aligned (so every plane is), a
// work-item takes four consecutive pixels with one dword load and one dword store per plane; otherwise a pixel at a time.  The
// choice is per image and uniform over the workgroup.  Image i is recoloured with the twelve statistics at stats + i * stats_stride
// (stride 0: one record for all).  wave64, no LDS.
__global__ __launch_bounds__(256) void k_ex_transfer_given_many(const ExGiven* __restrict__ img, unsigned long long n, const float* __restrict__ stats,
                                                                int stats_stride, TrK k, int keep_black) {
    const ExGiven e = img[blockIdx.y];
    float st[12];
#pragma unroll
    for (int i = 0; i < 12; ++i) st[i] = stats[(size_t)blockIdx.y * stats_stride + i];
    const size_t stride = (size_t)gridDim.x * blockDim.x, first = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if ((((uintptr_t)e.src | (uintptr_t)e.out | (uintptr_t)n) & 3u) == 0) {
        const size_t nq = (size_t)n / 4;
        const uint32_t* s4 = reinterpret_cast<const uint32_t*>(e.src);
        uint32_t* o4 = reinterpret_cast<uint32_t*>(e.out);
        for (size_t q = first; q < nq; q += stride) {
            const uint32_t r4 = s4[q], g4 = s4[q + nq], b4 = s4[q + 2 * nq];
            uint32_t ro4 = 0, go4 = 0, bo4 = 0;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                uint32_t ro, go, bo;
                ex_given_pixel(k, st, keep_black, (r4 >> (8 * j)) & 255u, (g4 >> (8 * j)) & 255u, (b4 >> (8 * j)) & 255u, ro, go, bo);
                ro4 |= ro << (8 * j);
                go4 |= go << (8 * j);
                bo4 |= bo << (8 * j);
            }
            o4[q] = ro4;
            o4[q + nq] = go4;
            o4[q + 2 * nq] = bo4;
        }
    } else {
        for (size_t i = first; i < n; i += stride) {
            uint32_t ro, go, bo;
            ex_given_pixel(k, st, keep_black, e.src[i], e.src[i + n], e.src[i + 2 * n], ro, go, bo);
            e.out[i] = (uint8_t)ro;
            e.out[i + n] = (uint8_t)go;
            e.out[i + 2 * n] = (uint8_t)bo;
        }
    }
}

// The filter of the statistics of `count` sets, in order: ONE wavefront, lanes 0 .. 11 each carry one of the twelve values.  Record
// i is read at m + i * m_stride and its filtered twin written at u + i * u_stride (a rig's records are 16 floats apart, dense ones
// 12).  A record is valid when every lane's value is finite and the sds' (lanes 3 .. 5, 9 .. 11) are > 0: a wave vote.  The state
// stays in a register across the loop and is written back once, with the flag.
// A rig's replay (failed != NULL): failed[i] says whether record i's set was refused by the seam scan of an earlier step of this
// sequence -- `prev` holds the scans of the step before (NULL at step 0, which clears the flags; NULL too where no scan can refuse).
// What such a set measures from then on means nothing: its record passes through unfiltered and never enters the state.
__global__ __launch_bounds__(64) void k_ex_stats_filter(const float* m, size_t m_stride, float* u, size_t u_stride, int count, float kf, float* __restrict__ state12,
                                                        int32_t* __restrict__ has_io, int32_t* failed, const SeamDev* prev, int first_step) {
    const int lane = threadIdx.x;
    const bool active = lane < 12, is_sd = active && (lane % 6) >= 3;
    bool has = *has_io != 0;
    float p = active && has ? state12[lane] : 0.0f;
    for (int i = 0; i < count; ++i) {
        bool out = false;  // wave-uniform
        if (failed) {
            out = !first_step && (failed[i] != 0 || (prev && prev[i].status != 0));
            if (lane == 0) failed[i] = out ? 1 : 0;
        }
        const float v = active ? m[(size_t)i * m_stride + lane] : 1.0f;
        const bool bad = active && (!(fabsf(v) <= 3.402823466e38f) || (is_sd && !(v > 0.0f)));
        float w = v;
        if (!out && !__any(bad)) {
            if (has) w = v + kf * (p - v);
            p = w;
            has = true;
        }
        if (active) u[(size_t)i * u_stride + lane] = w;
    }
    if (active && has) state12[lane] = p;
    if (lane == 0) *has_io = has ? 1 : 0;
}
