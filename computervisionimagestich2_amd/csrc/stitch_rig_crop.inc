// stitch_rig_crop.inc -- the crop of a rig's output (include/stitch_rig_crop.h; kernels in k_rig_crop.inc, DESIGN.md 18).  Included
// at the end of stitch_hip.hip (one translation unit), behind stitch_rig_seams.inc.  The replay itself is rig_stitch of
// stitch_rig.inc, which sends the last step of a cropped rig to the rig's own full-canvas buffers and calls rig_crop_copy.
namespace {

constexpr size_t kCropLdsBytes = 64 * 1024 - 1024;       // a row's hierarchy in LDS, without the opt-in for more than 64 KB
constexpr size_t kCropGlobalBytes = (size_t)64 << 20;    // rows too wide for it: the hierarchies of all workgroups in flight
constexpr int kCropMaxBlocks = 2048;

// The levels over a row of w heights: every level padded to a multiple of four, the last one a single group.
CropLevels crop_levels(int w, unsigned long long* total) {
    CropLevels lv;
    std::memset(&lv, 0, sizeof lv);
    unsigned long long at = 0;
    unsigned long long n = (unsigned long long)w;
    for (;;) {
        const unsigned long long pad = (n + 3) / 4 * 4;
        lv.off[lv.n] = at;
        lv.pad[lv.n] = (unsigned)pad;
        ++lv.n;
        at += pad;
        if (pad <= 4) break;
        n = pad / 4;
    }
    *total = at;
    return lv;
}

// The search over one source, heights held in T.  The four integers come back to the host: waits for `s`.
template <typename SRC, typename T>
int crop_search_as(SRC src, int w, int h, stitch_rect* out, hipStream_t s) {
    unsigned long long hier_len = 0;
    const CropLevels lv = crop_levels(w, &hier_len);
    const size_t hier_bytes = (size_t)hier_len * sizeof(T);
    const bool in_lds = hier_bytes <= kCropLdsBytes;
    int blocks = std::min(h, kCropMaxBlocks);
    if (!in_lds) blocks = (int)std::max<size_t>(1, std::min<size_t>((size_t)blocks, kCropGlobalBytes / hier_bytes));
    PanoArena A(s);
    T *up = nullptr, *g_hier = nullptr;
    CropRec* rec = nullptr;
    int32_t* d_out = nullptr;
    int rc;
    if ((rc = A.take(&up, sizeof(T) * (size_t)w * h)) || (rc = A.take(&rec, sizeof(CropRec) * blocks)) || (rc = A.take(&d_out, sizeof(int32_t) * 4))) return rc;
    if (!in_lds && (rc = A.take(&g_hier, hier_bytes * blocks))) return rc;
    PanoWait wait{s};  // what the arena frees is idle on every return path
    k_crop_up<SRC, T><<<(unsigned)(((size_t)w + 63) / 64), 64, 0, s>>>(src, w, h, up);
    if ((rc = launch_check("k_crop_up"))) return rc;
    if (in_lds)
        k_crop_rows<T, true><<<(unsigned)blocks, 256, hier_bytes, s>>>(up, w, h, lv, nullptr, hier_len, rec);
    else
        k_crop_rows<T, false><<<(unsigned)blocks, 256, 0, s>>>(up, w, h, lv, g_hier, hier_len, rec);
    if ((rc = launch_check("k_crop_rows"))) return rc;
    k_crop_pick<<<1, 256, 0, s>>>(rec, blocks, d_out);
    if ((rc = launch_check("k_crop_pick"))) return rc;
    int32_t got[4] = {0, 0, 0, 0};
    HIPCHK(hipMemcpyAsync(got, d_out, sizeof got, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    *out = stitch_rect{got[0], got[1], got[2], got[3]};
    return STITCH_OK;
}

// Heights in the narrowest type the mask's height fits: a column of h covered rows reaches h.
template <typename SRC>
int crop_search(SRC src, int w, int h, stitch_rect* out, hipStream_t s) {
    return h <= 0xffff ? crop_search_as<SRC, uint16_t>(src, w, h, out, s) : crop_search_as<SRC, uint32_t>(src, w, h, out, s);
}

int crop_check_size(int w, int h, const char* who) {
    if (w < 1 || h < 1) return fail(STITCH_ERR_ARG, "%s: bad size %d x %d", who, w, h);
    if ((long long)w * h > 0x7fffffffLL) return fail(STITCH_ERR_ARG, "%s: w*h overflows int", who);
    return STITCH_OK;
}

// ---- the rig's side (declared in stitch_rig.inc) ---------------------------------------------------------------------------
// max_sets full canvases, `crop_full_bytes` apart, on the device of the rig's workspaces.
int rig_crop_workspace(stitch_rig* R) {
    R->crop_full_bytes = align256((size_t)3 * R->out_w * R->out_h);
    if (!R->crop_full) HIPCHK(hipMalloc((void**)&R->crop_full, (size_t)R->max_sets * R->crop_full_bytes));
    return STITCH_OK;
}

// The rectangle of m full canvases (the src entries of the table) to the dst entries, in one launch.
int rig_crop_copy(const stitch_rig* R, const RigImage* d_tab, int m, hipStream_t s) {
    const stitch_rect& c = R->crop;
    k_crop_many<<<dim3(1u, (unsigned)std::min(3 * (long long)c.h, 65535LL), (unsigned)m), 256, 0, s>>>(d_tab, R->out_w, R->out_h, c.x0, c.y0, c.w, c.h);
    return launch_check("k_crop_many");
}

}  // namespace

extern "C" {

int stitch_dev_largest_rect_u8(const uint8_t* d_mask, int w, int h, stitch_rect* out, void* stream) {
    if (!d_mask || !out) return fail(STITCH_ERR_ARG, "largest_rect: null mask or output");
    int rc = crop_check_size(w, h, "largest_rect");
    if (rc) return rc;
    if ((rc = need_device())) return rc;
    return crop_search(CropBytes{d_mask, w}, w, h, out, as_stream(stream));
}

int stitch_dev_rig_inscribed_rect(stitch_rig* rig, int step, stitch_rect* out, void* stream) {
    if (!rig || !out) return fail(STITCH_ERR_ARG, "rig_inscribed_rect: null handle or output");
    const int ns = (int)rig->steps.size();
    if (step < -1 || step >= ns) return fail(STITCH_ERR_ARG, "rig_inscribed_rect: step %d outside -1 .. %d", step, ns - 1);
    int rc = need_device();
    if (rc) return rc;
    hipStream_t s = as_stream(stream);
    if ((rc = rig_cover(rig, s))) return rc;
    const int k = step < 0 ? ns - 1 : step;
    const int w = ns ? rig->steps[k].geom.cw : rig->fw[rig->start], h = ns ? rig->steps[k].geom.ch : rig->fh[rig->start], wpr = cover_wpr(w);
    if ((rc = crop_check_size(w, h, "rig_inscribed_rect"))) return rc;
    const unsigned long long* plane = ns ? rig->cover + rig->cover_step[k] + (size_t)2 * wpr * h : rig->cover + rig->cover_proj[rig->start];
    return crop_search(CropBits{plane, wpr}, w, h, out, s);
}

int stitch_rig_set_crop(stitch_rig* rig, const stitch_rect* rect, int mode) {
    if (!rig || !rect) return fail(STITCH_ERR_ARG, "rig_set_crop: null handle or rectangle");
    if (mode < STITCH_CROP_AFTER_FINISH || mode > STITCH_CROP_BEFORE_FINISH) return fail(STITCH_ERR_ARG, "rig_set_crop: mode %d outside 1 .. 2", mode);
    const stitch_rect& c = *rect;
    if (c.w < 1 || c.h < 1 || c.x0 < 0 || c.y0 < 0 || (long long)c.x0 + c.w > rig->out_w || (long long)c.y0 + c.h > rig->out_h)
        return fail(STITCH_ERR_ARG, "rig_set_crop: the rectangle %d x %d at (%d, %d) is empty or not inside the %d x %d canvas", c.w, c.h, c.x0, c.y0, rig->out_w,
                    rig->out_h);
    rig->crop = c;
    rig->crop_mode = mode;
    return STITCH_OK;
}

int stitch_rig_clear_crop(stitch_rig* rig) {
    if (!rig) return fail(STITCH_ERR_ARG, "rig_clear_crop: null handle");
    rig->crop_mode = 0;
    return STITCH_OK;
}

int stitch_rig_crop(const stitch_rig* rig, stitch_rect* rect_out, int* mode_out) {
    if (!rig) return fail(STITCH_ERR_ARG, "rig_crop: null handle");
    if (rect_out) *rect_out = rig->crop_mode ? rig->crop : stitch_rect{0, 0, rig->out_w, rig->out_h};
    if (mode_out) *mode_out = rig->crop_mode;
    return STITCH_OK;
}

int stitch_rig_output_size(const stitch_rig* rig, int* width, int* height) {
    if (!rig) return fail(STITCH_ERR_ARG, "rig_output_size: null handle");
    // (include/stitch_rig_scale.h: a rig with an output scale writes that size)
    if (width) *width = rig->scale_w ? rig->scale_w : rig->crop_mode ? rig->crop.w : rig->out_w;
    if (height) *height = rig->scale_h ? rig->scale_h : rig->crop_mode ? rig->crop.h : rig->out_h;
    return STITCH_OK;
}

}  // extern "C"
