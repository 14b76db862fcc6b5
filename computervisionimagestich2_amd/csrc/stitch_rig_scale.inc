// stitch_rig_scale.inc -- a rig's output at the size its consumer wants (include/stitch_rig_scale.h; kernel in k_rig_scale.inc,
// DESIGN.md 25).  Included at the end of stitch_hip.hip (one translation unit), behind stitch_rig_seam_paths.inc.  The replay itself
// is rig_stitch of stitch_rig.inc: with a scale set it takes the path of a formatted output for every call, and rig_fmt_finish_pack of
// stitch_rig_formats.inc ends in rig_scale_pack below instead of the k_pack_many launch.
namespace {

// the header's size rule
bool scale_rule(long long w, long long h, long long ow, long long oh) {
    return ow >= 1 && ow <= w && w <= STITCH_SCALE_MAX_FACTOR * ow && oh >= 1 && oh <= h && h <= STITCH_SCALE_MAX_FACTOR * oh;
}

int scale_gcd(int a, int b) {
    while (b) {
        const int t = a % b;
        a = b;
        b = t;
    }
    return a;
}

ScaleK scale_k(int w, int h, int ow, int oh) {
    const int gx = scale_gcd(w, ow), gy = scale_gcd(h, oh);
    const int strips = (ow + SC_STRIP - 1) / SC_STRIP, sw = ((ow + strips - 1) / strips + 3) / 4 * 4;  // the fewest strips, equally wide: sw <= SC_STRIP
    return ScaleK{ow, oh, sw, (unsigned)(w / gx), (unsigned)(ow / gx), (unsigned)(h / gy), (unsigned)(oh / gy)};
}

// rc: the source rectangle of the planar sides, scaled to ow x oh (the rule holds, and rc.w * rc.h <= 2^31 - 1)
template <bool FINISH>
int scale_launch_as(int fmt, int matrix, const FmtImage* d_tab, int count, const FmtRect& rc, int ow, int oh, const int32_t* d_eq, const MixK& mk, hipStream_t s) {
    const ScaleK sk = scale_k(rc.w, rc.h, ow, oh);
    const dim3 g((unsigned)((ow + sk.sw - 1) / sk.sw), (unsigned)std::min((oh + SC_BAND - 1) / SC_BAND, 65535), (unsigned)count);
    const Nv12K k = kNv12[matrix];
    switch (fmt) {
        case STITCH_PIX_PLANAR: k_pack_scaled_many<PIX_PLANAR, FINISH><<<g, SC_STRIP, 0, s>>>(d_tab, rc, sk, d_eq, mk, k); break;
        case STITCH_PIX_RGB24: k_pack_scaled_many<PIX_RGB24, FINISH><<<g, SC_STRIP, 0, s>>>(d_tab, rc, sk, d_eq, mk, k); break;
        case STITCH_PIX_BGR24: k_pack_scaled_many<PIX_BGR24, FINISH><<<g, SC_STRIP, 0, s>>>(d_tab, rc, sk, d_eq, mk, k); break;
        case STITCH_PIX_RGBX32: k_pack_scaled_many<PIX_RGBX32, FINISH><<<g, SC_STRIP, 0, s>>>(d_tab, rc, sk, d_eq, mk, k); break;
        case STITCH_PIX_BGRX32: k_pack_scaled_many<PIX_BGRX32, FINISH><<<g, SC_STRIP, 0, s>>>(d_tab, rc, sk, d_eq, mk, k); break;
        case STITCH_PIX_NV12: k_pack_scaled_many<PIX_NV12, FINISH><<<g, SC_STRIP, 0, s>>>(d_tab, rc, sk, d_eq, mk, k); break;
        case STITCH_PIX_YUYV: k_pack_scaled_many<PIX_YUYV, FINISH><<<g, SC_STRIP, 0, s>>>(d_tab, rc, sk, d_eq, mk, k); break;
        case STITCH_PIX_UYVY: k_pack_scaled_many<PIX_UYVY, FINISH><<<g, SC_STRIP, 0, s>>>(d_tab, rc, sk, d_eq, mk, k); break;
        case STITCH_PIX_NV21: k_pack_scaled_many<PIX_NV21, FINISH><<<g, SC_STRIP, 0, s>>>(d_tab, rc, sk, d_eq, mk, k); break;
        case STITCH_PIX_NV16: k_pack_scaled_many<PIX_NV16, FINISH><<<g, SC_STRIP, 0, s>>>(d_tab, rc, sk, d_eq, mk, k); break;
        default: return fail(STITCH_ERR_ARG, "scale_pack_many: format %d", fmt);
    }
    return launch_check("k_pack_scaled_many");
}

// ---- the rig's side (declared in stitch_rig.inc) ---------------------------------------------------------------------------
// what the rig writes per set without the scale
void rig_scale_source(const stitch_rig* R, int* w, int* h) {
    *w = R->crop_mode ? R->crop.w : R->out_w;
    *h = R->crop_mode ? R->crop.h : R->out_h;
}

int rig_scale_check(const stitch_rig* R, const char* who) {
    int w, h;
    rig_scale_source(R, &w, &h);
    if (!scale_rule(w, h, R->scale_w, R->scale_h))
        return fail(STITCH_ERR_ARG, "%s: the rig's output scale %d x %d is outside 1 <= ow <= w <= 8 ow, 1 <= oh <= h <= 8 oh for its %d x %d source (include/stitch_rig_scale.h)",
                    who, R->scale_w, R->scale_h, w, h);
    return STITCH_OK;
}

// the one launch that ends a sequence of a rig with a scale: m images' rectangle rc, finished where d_eq holds their LUTs
int rig_scale_pack(const stitch_rig* R, const FmtImage* d_fmt, int m, const FmtRect& rc, const int32_t* d_eq, const MixK& mk, hipStream_t s) {
    return d_eq ? scale_launch_as<true>(R->out_fmt, R->matrix, d_fmt, m, rc, R->scale_w, R->scale_h, d_eq, mk, s)
                : scale_launch_as<false>(R->out_fmt, R->matrix, d_fmt, m, rc, R->scale_w, R->scale_h, nullptr, mk, s);
}

}  // namespace

extern "C" {

int stitch_dev_scale_pack_many_u8(int fmt, int matrix, const uint8_t* const* d_planar, int src_w, int src_h, const stitch_rect* rect, const stitch_image* dst,
                                  int count, void* stream) {
    const char* who = "scale_pack_many";
    if (!fmt_ok(fmt)) return fail(STITCH_ERR_ARG, "%s: format %d is not one of 0 .. 5, 16 .. 19", who, fmt);
    if (matrix < 0 || matrix > 2) return fail(STITCH_ERR_ARG, "%s: matrix %d outside 0 .. 2", who, matrix);
    if (!d_planar || !dst || count < 1 || count > kRigMaxImages) return fail(STITCH_ERR_ARG, "%s: null table or %d images (1 .. %d)", who, count, kRigMaxImages);
    if (src_w < 1 || src_h < 1 || (long long)src_w * src_h > 0x7fffffffLL / 3) return fail(STITCH_ERR_ARG, "%s: bad size %d x %d", who, src_w, src_h);
    const stitch_rect c = rect ? *rect : stitch_rect{0, 0, src_w, src_h};
    if (c.w < 1 || c.h < 1 || c.x0 < 0 || c.y0 < 0 || (long long)c.x0 + c.w > src_w || (long long)c.y0 + c.h > src_h)
        return fail(STITCH_ERR_ARG, "%s: the rectangle %d x %d at (%d, %d) is empty or not inside the %d x %d image", who, c.w, c.h, c.x0, c.y0, src_w, src_h);
    const int ow = dst[0].width, oh = dst[0].height;
    if (!scale_rule(c.w, c.h, ow, oh))
        return fail(STITCH_ERR_ARG, "%s: the target %d x %d is outside 1 <= ow <= w <= 8 ow, 1 <= oh <= h <= 8 oh for a %d x %d source", who, ow, oh, c.w, c.h);
    std::vector<FmtImage> tab;
    for (int i = 0; i < count; ++i) {
        const int rc = fmt_check_image(fmt, dst[i], ow, oh, who, "image", i);
        if (rc) return rc;
        if (!d_planar[i]) return fail(STITCH_ERR_ARG, "%s: image %d has no planar buffer", who, i);
        tab.push_back(FmtImage{dst[i].data, dst[i].data2, const_cast<uint8_t*>(d_planar[i]), dst[i].pitch, dst[i].pitch2});
    }
    int rc = need_device();
    if (rc) return rc;
    hipStream_t s = as_stream(stream);
    PanoArena A(s);
    FmtImage* d_tab = nullptr;
    if ((rc = A.take(&d_tab, sizeof(FmtImage) * count))) return rc;
    PanoWait wait{s};  // `tab` is read by its upload
    HIPCHK(hipMemcpyAsync(d_tab, tab.data(), sizeof(FmtImage) * count, hipMemcpyHostToDevice, s));
    return scale_launch_as<false>(fmt, matrix, d_tab, count, FmtRect{src_w, src_h, c.x0, c.y0, c.w, c.h}, ow, oh, nullptr, MixK{0.0, 1.0, 0.0}, s);
}

int stitch_rig_set_output_scale(stitch_rig* rig, int ow, int oh) {
    if (!rig) return fail(STITCH_ERR_ARG, "rig_set_output_scale: null handle");
    int w, h;
    rig_scale_source(rig, &w, &h);
    if (!scale_rule(w, h, ow, oh))
        return fail(STITCH_ERR_ARG, "rig_set_output_scale: %d x %d is outside 1 <= ow <= w <= 8 ow, 1 <= oh <= h <= 8 oh for the rig's %d x %d output", ow, oh, w, h);
    rig->scale_w = ow;
    rig->scale_h = oh;
    return STITCH_OK;
}

int stitch_rig_clear_output_scale(stitch_rig* rig) {
    if (!rig) return fail(STITCH_ERR_ARG, "rig_clear_output_scale: null handle");
    rig->scale_w = rig->scale_h = 0;
    return STITCH_OK;
}

int stitch_rig_output_scale(const stitch_rig* rig, int* ow, int* oh) {
    if (!rig) return fail(STITCH_ERR_ARG, "rig_output_scale: null handle");
    if (ow) *ow = rig->scale_w;
    if (oh) *oh = rig->scale_h;
    return STITCH_OK;
}

}  // extern "C"
