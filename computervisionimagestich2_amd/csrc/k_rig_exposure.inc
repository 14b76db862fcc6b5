// Part of stitch_kernels.hpp (included there, inside namespace sk, after k_exposure.inc and k_rig.inc): the six kernels of the
// colour transfer for MANY images per launch (include/stitch_rig_exposure.h, DESIGN.md 15).  k_exposure.inc's kernels take up to
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
