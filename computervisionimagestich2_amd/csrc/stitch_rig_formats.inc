// stitch_rig_formats.inc -- a rig's frames and mosaics in camera layouts (include/stitch_rig_formats.h and, for the 4:2:2 layouts
// and NV21, include/stitch_rig_formats_yuv.h; kernels in k_rig_formats.inc, DESIGN.md 19 and 23).  Included at the end of
// stitch_hip.hip (one translation unit), behind stitch_rig_crop.inc.  The replay itself is rig_stitch of stitch_rig.inc, which calls
// the rig_fmt_* functions below for a call with images.
namespace {

// include/stitch_rig_formats.h's two tables, one row per matrix
const Nv12K kNv12[3] = {
    {16, 76309, 104597, 25675, 53279, 132201, 16829, 33039, 6416, 9714, 19070, 28784, 28784, 24103, 4681},
    {16, 76309, 117489, 13975, 34925, 138438, 11966, 40254, 4064, 6596, 22188, 28784, 28784, 26145, 2639},
    {0, 65536, 91881, 22553, 46802, 116130, 19595, 38470, 7471, 11058, 21710, 32768, 32768, 27439, 5329},
};

bool fmt_ok(int fmt) { return (fmt >= STITCH_PIX_PLANAR && fmt <= STITCH_PIX_NV12) || (fmt >= STITCH_PIX_YUYV && fmt <= STITCH_PIX_NV16); }
bool fmt_two_planes(int fmt) { return fmt == STITCH_PIX_NV12 || fmt == STITCH_PIX_NV21 || fmt == STITCH_PIX_NV16; }
bool fmt_420(int fmt) { return fmt == STITCH_PIX_NV12 || fmt == STITCH_PIX_NV21; }
// the pixel bytes of a row of plane 0
long long fmt_row_bytes(int fmt, long long w) {
    if (fmt == STITCH_PIX_YUYV || fmt == STITCH_PIX_UYVY) return 4 * ((w + 1) / 2);
    return (fmt == STITCH_PIX_RGB24 || fmt == STITCH_PIX_BGR24 ? 3 : fmt_two_planes(fmt) ? 1 : 4) * w;
}

// The extents of an image's planes, or false for a bad format, size or pitch.
bool fmt_extents(int fmt, long long w, long long h, long long pitch, long long pitch2, size_t* b1, size_t* b2) {
    if (!fmt_ok(fmt) || w < 1 || h < 1) return false;
    size_t e1 = 0, e2 = 0;
    if (fmt == STITCH_PIX_PLANAR) {
        e1 = (size_t)3 * (size_t)w * (size_t)h;
    } else {
        const long long row = fmt_row_bytes(fmt, w);
        if (pitch < row) return false;
        e1 = (size_t)((h - 1) * pitch + row);
        if (fmt_two_planes(fmt)) {
            const long long row2 = 2 * ((w + 1) / 2), rows2 = fmt_420(fmt) ? (h + 1) / 2 : h;
            if (pitch2 < row2) return false;
            e2 = (size_t)((rows2 - 1) * pitch2 + row2);
        }
    }
    if (b1) *b1 = e1;
    if (b2) *b2 = e2;
    return true;
}

// One image of a call: its size against (w, h), its pointers, its pitches.
int fmt_check_image(int fmt, const stitch_image& im, int w, int h, const char* who, const char* what, int index) {
    if (im.width != w || im.height != h) return fail(STITCH_ERR_ARG, "%s: %s %d is %d x %d, expected %d x %d", who, what, index, im.width, im.height, w, h);
    if (!im.data || (fmt_two_planes(fmt) && !im.data2)) return fail(STITCH_ERR_ARG, "%s: %s %d has a null plane", who, what, index);
    if (!fmt_extents(fmt, w, h, im.pitch, im.pitch2, nullptr, nullptr))
        return fail(STITCH_ERR_ARG, "%s: %s %d has a pitch (%d, %d) below its %d x %d rows", who, what, index, im.pitch, im.pitch2, w, h);
    return STITCH_OK;
}

bool fmt_images_overlap(int fa, const stitch_image& a, int fb, const stitch_image& b) {
    size_t a1 = 0, a2 = 0, b1 = 0, b2 = 0;
    fmt_extents(fa, a.width, a.height, a.pitch, a.pitch2, &a1, &a2);
    fmt_extents(fb, b.width, b.height, b.pitch, b.pitch2, &b1, &b2);
    return ranges_overlap(a.data, a1, b.data, b1) || (a2 && ranges_overlap(a.data2, a2, b.data, b1)) || (b2 && ranges_overlap(a.data, a1, b.data2, b2)) ||
           (a2 && b2 && ranges_overlap(a.data2, a2, b.data2, b2));
}

dim3 fmt_grid(int w, int rows, int count) { return dim3((unsigned)(((w + 3) / 4 + 255) / 256), (unsigned)std::min(rows, 65535), (unsigned)count); }

int fmt_launch_unpack(int fmt, int matrix, const FmtImage* d_tab, int count, int w, int h, hipStream_t s) {
    const dim3 g = fmt_grid(w, h, count);
    const Nv12K k = kNv12[matrix];
    switch (fmt) {
        case STITCH_PIX_RGB24: k_unpack_many<PIX_RGB24><<<g, 256, 0, s>>>(d_tab, w, h, k); break;
        case STITCH_PIX_BGR24: k_unpack_many<PIX_BGR24><<<g, 256, 0, s>>>(d_tab, w, h, k); break;
        case STITCH_PIX_RGBX32: k_unpack_many<PIX_RGBX32><<<g, 256, 0, s>>>(d_tab, w, h, k); break;
        case STITCH_PIX_BGRX32: k_unpack_many<PIX_BGRX32><<<g, 256, 0, s>>>(d_tab, w, h, k); break;
        case STITCH_PIX_NV12: k_unpack_many<PIX_NV12><<<g, 256, 0, s>>>(d_tab, w, h, k); break;
        case STITCH_PIX_YUYV: k_unpack_many<PIX_YUYV><<<g, 256, 0, s>>>(d_tab, w, h, k); break;
        case STITCH_PIX_UYVY: k_unpack_many<PIX_UYVY><<<g, 256, 0, s>>>(d_tab, w, h, k); break;
        case STITCH_PIX_NV21: k_unpack_many<PIX_NV21><<<g, 256, 0, s>>>(d_tab, w, h, k); break;
        case STITCH_PIX_NV16: k_unpack_many<PIX_NV16><<<g, 256, 0, s>>>(d_tab, w, h, k); break;
        default: return fail(STITCH_ERR_ARG, "unpack_many: format %d", fmt);
    }
    return launch_check("k_unpack_many");
}

template <bool FINISH>
int fmt_launch_pack_as(int fmt, int matrix, const FmtImage* d_tab, int count, const FmtRect& rc, const int32_t* d_eq, const MixK& mk, hipStream_t s) {
    const dim3 g = fmt_grid(rc.w, fmt_420(fmt) ? (rc.h + 1) / 2 : rc.h, count);  // row pairs for 4:2:0; rows for 4:2:2 and the rest
    const Nv12K k = kNv12[matrix];
    switch (fmt) {
        case STITCH_PIX_RGB24: k_pack_many<PIX_RGB24, FINISH><<<g, 256, 0, s>>>(d_tab, rc, d_eq, mk, k); break;
        case STITCH_PIX_BGR24: k_pack_many<PIX_BGR24, FINISH><<<g, 256, 0, s>>>(d_tab, rc, d_eq, mk, k); break;
        case STITCH_PIX_RGBX32: k_pack_many<PIX_RGBX32, FINISH><<<g, 256, 0, s>>>(d_tab, rc, d_eq, mk, k); break;
        case STITCH_PIX_BGRX32: k_pack_many<PIX_BGRX32, FINISH><<<g, 256, 0, s>>>(d_tab, rc, d_eq, mk, k); break;
        case STITCH_PIX_NV12: k_pack_many<PIX_NV12, FINISH><<<g, 256, 0, s>>>(d_tab, rc, d_eq, mk, k); break;
        case STITCH_PIX_YUYV: k_pack_many<PIX_YUYV, FINISH><<<g, 256, 0, s>>>(d_tab, rc, d_eq, mk, k); break;
        case STITCH_PIX_UYVY: k_pack_many<PIX_UYVY, FINISH><<<g, 256, 0, s>>>(d_tab, rc, d_eq, mk, k); break;
        case STITCH_PIX_NV21: k_pack_many<PIX_NV21, FINISH><<<g, 256, 0, s>>>(d_tab, rc, d_eq, mk, k); break;
        case STITCH_PIX_NV16: k_pack_many<PIX_NV16, FINISH><<<g, 256, 0, s>>>(d_tab, rc, d_eq, mk, k); break;
        default: return fail(STITCH_ERR_ARG, "pack_many: format %d", fmt);
    }
    return launch_check("k_pack_many");
}

int fmt_many_args(int fmt, int matrix, const void* a, const void* b, int count, const char* who) {
    if (!fmt_ok(fmt) || fmt == STITCH_PIX_PLANAR) return fail(STITCH_ERR_ARG, "%s: format %d is not one of the packed formats 1 .. 5, 16 .. 19", who, fmt);
    if (matrix < 0 || matrix > 2) return fail(STITCH_ERR_ARG, "%s: matrix %d outside 0 .. 2", who, matrix);
    if (!a || !b || count < 1 || count > kRigMaxImages) return fail(STITCH_ERR_ARG, "%s: null table or %d images (1 .. %d)", who, count, kRigMaxImages);
    return STITCH_OK;
}

// the table of a stand-alone conversion, checked: every image of images[0]'s size, the planar side dense
int fmt_many_table(int fmt, const stitch_image* images, const uint8_t* const* planar, int count, const char* who, std::vector<FmtImage>* tab) {
    const int w = images[0].width, h = images[0].height;
    if (w < 1 || h < 1 || (long long)w * h > 0x7fffffffLL / 3) return fail(STITCH_ERR_ARG, "%s: bad size %d x %d", who, w, h);
    for (int i = 0; i < count; ++i) {
        const int rc = fmt_check_image(fmt, images[i], w, h, who, "image", i);
        if (rc) return rc;
        if (!planar[i]) return fail(STITCH_ERR_ARG, "%s: image %d has no planar buffer", who, i);
        tab->push_back(FmtImage{images[i].data, images[i].data2, const_cast<uint8_t*>(planar[i]), images[i].pitch, images[i].pitch2});
    }
    return STITCH_OK;
}

// ---- the rig's side (declared in stitch_rig.inc) ---------------------------------------------------------------------------
// The form of frame index f's projection in this call.  Fused -- the tiled projection stages the packed frames itself -- where the
// planar frame would take the tiled form (project_lds_bytes: a width that is a multiple of 4, a box within the LDS budget) and every
// set's planes and pitches are multiples of four, which the staging's dword loads ask.  Otherwise the stated fallback: k_unpack_many
// into the rig's planar scratch, then the planar projection in whatever form it takes.
bool rig_fmt_fused(const stitch_rig* R, const RigFmtCall& fc, int f, int n_sets) {
    const ProjParams pp = proj_params(R->fw[f], R->fh[f], R->fov_deg);
    if (!project_lds_bytes<uint8_t>(R->fw[f], R->fh[f], pp, true)) return false;
    for (int i = 0; i < n_sets; ++i) {
        const stitch_image& im = fc.frames[(size_t)i * R->n + f];
        uintptr_t bits = reinterpret_cast<uintptr_t>(im.data) | (uintptr_t)im.pitch;
        if (fmt_two_planes(R->in_fmt)) bits |= reinterpret_cast<uintptr_t>(im.data2) | (uintptr_t)im.pitch2;
        if (bits & 3u) return false;
    }
    return true;
}

// Whether the one pack reads the rectangle out of the full canvases (no crop copy): mode 1, and mode 2 without a finish pass.
bool rig_fmt_pack_from_full(const stitch_rig* R) { return R->crop_mode == 1 || (R->crop_mode == 2 && !R->finish); }

int rig_fmt_workspace(stitch_rig* R, RigFmtCall* fc, int n_sets) {
    fc->fused.assign((size_t)R->n, 0);
    if (R->in_fmt) {
        if (R->fmt_in.empty()) R->fmt_in.assign((size_t)R->n, nullptr);
        for (int f : R->needed) {
            fc->fused[f] = rig_fmt_fused(R, *fc, f, n_sets);
            if (!fc->fused[f] && !R->fmt_in[f]) HIPCHK(hipMalloc((void**)&R->fmt_in[f], (size_t)R->max_sets * 3 * R->fw[f] * R->fh[f]));
        }
    }
    if ((R->out_fmt || R->scale_w) && !rig_fmt_pack_from_full(R)) {  // (else nothing reads them.)  Of the canvas's size: a crop is inside it
        R->fmt_out_bytes = align256((size_t)3 * R->out_w * R->out_h);
        if (!R->fmt_out) HIPCHK(hipMalloc((void**)&R->fmt_out, (size_t)R->max_sets * R->fmt_out_bytes));
    }
    return STITCH_OK;
}

// h_tab: rig_stitch's pointer table -- per sequence m entries per projected frame, whose dst is where the projection writes, then
// the outputs' entries (two slices for a cropped rig).
void rig_fmt_tables(const stitch_rig* R, RigFmtCall* fc, const RigImage* h_tab, int n_sets) {
    fc->tab.clear();
    int set0 = 0;
    size_t at = 0;
    for (int m : rig_sequences(n_sets, R->max_sets)) {
        for (int f : R->needed)
            for (int i = 0; i < m; ++i, ++at) {
                if (!R->in_fmt) continue;
                const stitch_image& im = fc->frames[(size_t)(set0 + i) * R->n + f];
                // the planar side: the projection's destination (fused), or the scratch the planar projection reads
                uint8_t* planar = fc->fused[f] ? h_tab[at].dst : R->fmt_in[f] + (size_t)i * 3 * R->fw[f] * R->fh[f];
                fc->tab.push_back(FmtImage{im.data, im.data2, planar, im.pitch, im.pitch2});
            }
        at += (size_t)m * (R->crop_mode ? 2 : 1);
        if (R->out_fmt || R->scale_w)  // (include/stitch_rig_scale.h: a scaled planar output is an image of the table as well)
            for (int i = 0; i < m; ++i) {
                const stitch_image& im = fc->out[set0 + i];
                uint8_t* planar = rig_fmt_pack_from_full(R) ? R->crop_full + (size_t)i * R->crop_full_bytes : R->fmt_out + (size_t)i * R->fmt_out_bytes;
                fc->tab.push_back(FmtImage{im.data, im.data2, planar, im.pitch, im.pitch2});
            }
        set0 += m;
    }
}

int rig_fmt_unpack(const stitch_rig* R, const FmtImage* d_tab, int m, int w, int h, hipStream_t s) { return fmt_launch_unpack(R->in_fmt, R->matrix, d_tab, m, w, h, s); }

template <int FMT>
void rig_fmt_project_as(const FmtImage* d_tab, int m, int w, int h, const ProjParams& pp, size_t lds, const Nv12K& k, hipStream_t s) {
    constexpr int TW = PJ_TW_U8, TH = PJ_TH_U8;
    const dim3 g((w + TW - 1) / TW, (h + TH - 1) / TH, (unsigned)m);
    if (!pp.flag)
        k_project_fmt_lds_many<FMT, TW, TH><<<g, 256, lds, s>>>(d_tab, w, h, pp.r, (int)lds, k);
    else
        k_project_fmt_lds_t_many<FMT, TW, TH><<<g, 256, lds, s>>>(d_tab, w, h, pp.r, (int)lds, k);
}
// m frames of one index through the fused projection: rig_project_many's tiled forms with the staging of k_rig_formats.inc
int rig_fmt_project(const stitch_rig* R, const FmtImage* d_tab, int m, int w, int h, hipStream_t s) {
    const ProjParams pp = proj_params(w, h, R->fov_deg);
    const size_t lds = project_lds_bytes<uint8_t>(w, h, pp, true);  // > 0: rig_fmt_fused
    const Nv12K k = kNv12[R->matrix];
    switch (R->in_fmt) {
        case STITCH_PIX_RGB24: rig_fmt_project_as<PIX_RGB24>(d_tab, m, w, h, pp, lds, k, s); break;
        case STITCH_PIX_BGR24: rig_fmt_project_as<PIX_BGR24>(d_tab, m, w, h, pp, lds, k, s); break;
        case STITCH_PIX_RGBX32: rig_fmt_project_as<PIX_RGBX32>(d_tab, m, w, h, pp, lds, k, s); break;
        case STITCH_PIX_BGRX32: rig_fmt_project_as<PIX_BGRX32>(d_tab, m, w, h, pp, lds, k, s); break;
        case STITCH_PIX_YUYV: rig_fmt_project_as<PIX_YUYV>(d_tab, m, w, h, pp, lds, k, s); break;
        case STITCH_PIX_UYVY: rig_fmt_project_as<PIX_UYVY>(d_tab, m, w, h, pp, lds, k, s); break;
        case STITCH_PIX_NV21: rig_fmt_project_as<PIX_NV21>(d_tab, m, w, h, pp, lds, k, s); break;
        case STITCH_PIX_NV16: rig_fmt_project_as<PIX_NV16>(d_tab, m, w, h, pp, lds, k, s); break;
        default: rig_fmt_project_as<PIX_NV12>(d_tab, m, w, h, pp, lds, k, s); break;
    }
    return launch_check("k_project_fmt_lds_many");
}

// histogram and LUT of m planar images by the finish pass's own launches (rig_hist_lut_many of stitch_rig.inc)
int fmt_hist_lut(const RigImage* h_tab, const RigImage* d_tab, int32_t* d_eq, int m, int w, int h, hipStream_t s) {
    (void)rig_hist_lut_many(h_tab, d_tab, d_eq, m, w, h, s);
    return launch_check("hist_lut_many");
}

// h_tab / d_tab: the sequence's output entries {full canvas or NULL, the rig's planar output}, and for a cropped rig m entries
// {NULL, full canvas} behind them (rig_stitch's table).
int rig_fmt_finish_pack(const stitch_rig* R, const RigImage* h_tab, const RigImage* d_tab, const FmtImage* d_fmt, int32_t* d_eq, int m, hipStream_t s) {
    int rc;
    const stitch_rect& c = R->crop;
    FmtRect r{R->out_w, R->out_h, 0, 0, R->out_w, R->out_h};
    if (R->crop_mode && rig_fmt_pack_from_full(R)) {
        // the LUT is the full canvas's, the pack reads the rectangle out of it
        if (R->finish && (rc = fmt_hist_lut(h_tab + m, d_tab + m, d_eq, m, R->out_w, R->out_h, s))) return rc;
        r = FmtRect{R->out_w, R->out_h, c.x0, c.y0, c.w, c.h};
    } else if (R->crop_mode) {
        // mode 2 with the finish pass: the rectangle is an image of its own, with a LUT of its own
        if ((rc = rig_crop_copy(R, d_tab, m, s)) || (rc = fmt_hist_lut(h_tab, d_tab, d_eq, m, c.w, c.h, s))) return rc;
        r = FmtRect{c.w, c.h, 0, 0, c.w, c.h};
    } else if (R->finish && (rc = fmt_hist_lut(h_tab, d_tab, d_eq, m, R->out_w, R->out_h, s))) {
        return rc;
    }
    const MixK mk = mix_params(R->num, R->den);
    if (R->scale_w) return rig_scale_pack(R, d_fmt, m, r, R->finish ? d_eq : nullptr, mk, s);  // include/stitch_rig_scale.h: in place of the pack
    return R->finish ? fmt_launch_pack_as<true>(R->out_fmt, R->matrix, d_fmt, m, r, d_eq, mk, s) : fmt_launch_pack_as<false>(R->out_fmt, R->matrix, d_fmt, m, r, nullptr, mk, s);
}

}  // namespace

extern "C" {

int stitch_image_bytes(int fmt, int w, int h, int pitch, int pitch2, size_t* bytes, size_t* bytes2) {
    if (!fmt_extents(fmt, w, h, pitch, pitch2, bytes, bytes2))
        return fail(STITCH_ERR_ARG, "image_bytes: format %d (0 .. 5, 16 .. 19), size %d x %d or pitches (%d, %d) below a row", fmt, w, h, pitch, pitch2);
    return STITCH_OK;
}

int stitch_dev_unpack_many_u8(int fmt, int matrix, const stitch_image* src, uint8_t* const* d_planar, int count, void* stream) {
    int rc = fmt_many_args(fmt, matrix, src, d_planar, count, "unpack_many");
    if (rc) return rc;
    std::vector<FmtImage> tab;
    if ((rc = fmt_many_table(fmt, src, d_planar, count, "unpack_many", &tab))) return rc;
    if ((rc = need_device())) return rc;
    hipStream_t s = as_stream(stream);
    PanoArena A(s);
    FmtImage* d_tab = nullptr;
    if ((rc = A.take(&d_tab, sizeof(FmtImage) * count))) return rc;
    PanoWait wait{s};  // `tab` is read by its upload
    HIPCHK(hipMemcpyAsync(d_tab, tab.data(), sizeof(FmtImage) * count, hipMemcpyHostToDevice, s));
    return fmt_launch_unpack(fmt, matrix, d_tab, count, src[0].width, src[0].height, s);
}

int stitch_dev_pack_many_u8(int fmt, int matrix, const uint8_t* const* d_planar, const stitch_image* dst, int count, void* stream) {
    int rc = fmt_many_args(fmt, matrix, d_planar, dst, count, "pack_many");
    if (rc) return rc;
    std::vector<FmtImage> tab;
    if ((rc = fmt_many_table(fmt, dst, d_planar, count, "pack_many", &tab))) return rc;
    if ((rc = need_device())) return rc;
    hipStream_t s = as_stream(stream);
    PanoArena A(s);
    FmtImage* d_tab = nullptr;
    if ((rc = A.take(&d_tab, sizeof(FmtImage) * count))) return rc;
    PanoWait wait{s};  // `tab` is read by its upload
    HIPCHK(hipMemcpyAsync(d_tab, tab.data(), sizeof(FmtImage) * count, hipMemcpyHostToDevice, s));
    const int w = dst[0].width, h = dst[0].height;
    return fmt_launch_pack_as<false>(fmt, matrix, d_tab, count, FmtRect{w, h, 0, 0, w, h}, nullptr, MixK{0.0, 1.0, 0.0}, s);
}

int stitch_rig_set_formats(stitch_rig* rig, int in_fmt, int out_fmt, int matrix) {
    if (!rig) return fail(STITCH_ERR_ARG, "rig_set_formats: null handle");
    if (!fmt_ok(in_fmt) || !fmt_ok(out_fmt)) return fail(STITCH_ERR_ARG, "rig_set_formats: formats (%d, %d) outside 0 .. 5, 16 .. 19", in_fmt, out_fmt);
    if (matrix < 0 || matrix > 2) return fail(STITCH_ERR_ARG, "rig_set_formats: matrix %d outside 0 .. 2", matrix);
    rig->in_fmt = in_fmt;
    rig->out_fmt = out_fmt;
    rig->matrix = matrix;
    return STITCH_OK;
}

int stitch_rig_formats(const stitch_rig* rig, int* in_fmt, int* out_fmt, int* matrix) {
    if (!rig) return fail(STITCH_ERR_ARG, "rig_formats: null handle");
    if (in_fmt) *in_fmt = rig->in_fmt;
    if (out_fmt) *out_fmt = rig->out_fmt;
    if (matrix) *matrix = rig->matrix;
    return STITCH_OK;
}

int stitch_rig_input_form(const stitch_rig* rig, int frame, int* form) {
    if (!rig || !form) return fail(STITCH_ERR_ARG, "rig_input_form: null argument");
    if (frame < 0 || frame >= rig->n) return fail(STITCH_ERR_ARG, "rig_input_form: frame %d outside 0 .. %d", frame, rig->n - 1);
    *form = rig->fmt_form.empty() ? STITCH_RIG_INPUT_NONE : rig->fmt_form[(size_t)frame];
    return STITCH_OK;
}

int stitch_rig_clear_formats(stitch_rig* rig) {
    if (!rig) return fail(STITCH_ERR_ARG, "rig_clear_formats: null handle");
    rig->in_fmt = rig->out_fmt = STITCH_PIX_PLANAR;
    rig->matrix = 0;
    return STITCH_OK;
}

int stitch_dev_rig_stitch_fmt_u8(stitch_rig* rig, const stitch_image* frames, int n_sets, const stitch_image* out, int32_t* set_status, stitch_seam* seams,
                                 float* stats, void* stream) {
    const char* who = "rig_stitch_fmt";
    if (!rig || !frames || !out || !set_status || n_sets < 1) return fail(STITCH_ERR_ARG, "%s: null argument or %d sets", who, n_sets);
    if (stats && !rig->ex.mode) return fail(STITCH_ERR_ARG, "%s: statistics asked of a rig made without a transfer (mode 0)", who);
    const stitch_rig* R = rig;
    int rc;
    if (R->scale_w && (rc = rig_scale_check(R, who))) return rc;  // include/stitch_rig_scale.h: the outputs have the scaled size
    const int n = R->n, ow = R->scale_w ? R->scale_w : R->crop_mode ? R->crop.w : R->out_w, oh = R->scale_w ? R->scale_h : R->crop_mode ? R->crop.h : R->out_h;
    for (int i = 0; i < n_sets; ++i) {
        if ((rc = fmt_check_image(R->out_fmt, out[i], ow, oh, who, "the output of set", i))) return rc;
        for (int f = 0; f < n; ++f) {
            const stitch_image& fr = frames[(size_t)i * n + f];
            if (fr.width != R->fw[f] || fr.height != R->fh[f])
                return fail(STITCH_ERR_ARG, "%s: set %d frame %d is %d x %d, the rig was made for %d x %d", who, i, f, fr.width, fr.height, R->fw[f], R->fh[f]);
        }
        for (int f : R->needed)
            if ((rc = fmt_check_image(R->in_fmt, frames[(size_t)i * n + f], R->fw[f], R->fh[f], who, "a frame of set", i))) return rc;
    }
    for (int i = 0; i < n_sets; ++i) {
        for (int f : R->needed)
            for (int j = 0; j < n_sets; ++j)
                if (fmt_images_overlap(R->out_fmt, out[j], R->in_fmt, frames[(size_t)i * n + f]))
                    return fail(STITCH_ERR_ARG, "%s: the output of set %d overlaps frame %d of set %d", who, j, f, i);
        for (int j = 0; j < i; ++j)
            if (fmt_images_overlap(R->out_fmt, out[j], R->out_fmt, out[i])) return fail(STITCH_ERR_ARG, "%s: the outputs of sets %d and %d overlap", who, j, i);
    }
    // the planar call's arguments: read for a planar side only
    std::vector<stitch_frame_u8> pf((size_t)n_sets * n);
    std::vector<uint8_t*> po((size_t)n_sets);
    for (size_t i = 0; i < pf.size(); ++i) pf[i] = stitch_frame_u8{frames[i].data, frames[i].width, frames[i].height};
    for (int i = 0; i < n_sets; ++i) po[i] = out[i].data;
    RigFmtCall fc{frames, out, {}, {}, nullptr};
    return rig_stitch(rig, pf.data(), n_sets, po.data(), set_status, seams, stats, stream, &fc);
}

}  // extern "C"
