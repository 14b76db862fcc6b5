// Part of stitch_kernels.hpp (included there, inside namespace sk): a rig's frames and mosaics in camera layouts
// (include/stitch_rig_formats.h and include/stitch_rig_formats_yuv.h, which state every rule restated here) -- packed RGB / BGR with or
// without a fourth byte, NV12 and NV21 (4:2:0), YUYV, UYVY and NV16 (4:2:2) -- to and from the dense planar layout of every other
// kernel, many same-size images per launch.
//
// blockIdx.z = image, blockIdx.y = row (NV12 / NV21 pack: row PAIR; in turn where the grid is smaller), and a work-item owns four
// pixels of the row (NV12 / NV21 pack: two 2 x 2 blocks; 4:2:2 pack: two 2 x 1 pairs -- the chroma average needs no second pass).
// A row whose addresses on both sides are multiples of four moves its full groups as dwords (a row of four-byte pixels on a 16-byte
// boundary as one 16-byte access per group); the pixels behind the last full group, and every row of any other alignment, move as
// bytes.  Both forms run the same per-pixel functions, so they give the same bytes.  Integers only; wave64, plain C++.
constexpr int PIX_PLANAR = 0, PIX_RGB24 = 1, PIX_BGR24 = 2, PIX_RGBX32 = 3, PIX_BGRX32 = 4, PIX_NV12 = 5;
constexpr int PIX_YUYV = 16, PIX_UYVY = 17, PIX_NV21 = 18, PIX_NV16 = 19;

struct FmtImage {  // one entry of the device table: the packed image and the dense planar one
    uint8_t* data;
    uint8_t* data2;
    uint8_t* planar;
    int pitch, pitch2;
};
struct FmtRect {  // the planar side of a pack: the rectangle (x0, y0, w, h) of a (3, H, W) image
    int W, H, x0, y0, w, h;
};
struct Nv12K {  // the 16.16 coefficients of one matrix, both directions
    int yoff, ky, krv, kgu, kgv, kbu;
    int yr, yg, yb, ur, ug, ub, vr, vg, vb;
};

template <int FMT>
struct FmtTraits {
    static constexpr bool yuv = FMT == PIX_NV12 || FMT >= PIX_YUYV;                 // Y Cb Cr through one of the matrices
    static constexpr bool two_planes = FMT == PIX_NV12 || FMT == PIX_NV21 || FMT == PIX_NV16;
    static constexpr bool c422 = FMT == PIX_YUYV || FMT == PIX_UYVY || FMT == PIX_NV16;  // a chroma pair per 2 x 1 pixels (else, yuv: per 2 x 2)
    // bytes from one pixel of plane 0 to the next (YUYV, UYVY: from one Y to the next)
    static constexpr int bpp = FMT == PIX_RGB24 || FMT == PIX_BGR24 ? 3 : two_planes ? 1 : FMT == PIX_YUYV || FMT == PIX_UYVY ? 2 : 4;
    static constexpr int ro = FMT == PIX_BGR24 || FMT == PIX_BGRX32 ? 2 : 0;  // the byte of a pixel that holds R; G is byte 1, B is 2 - ro
    // yuv: a chroma pair's place is cstep bytes after the one before it; Cb and Cr are its bytes cbo and cro.  In YUYV and UYVY that
    // place is the 4-byte group itself, and pixel 2i's Y is byte yo of the group, pixel 2i+1's is byte yo + 2.
    static constexpr int cstep = two_planes ? 2 : 4;
    static constexpr int yo = FMT == PIX_UYVY ? 1 : 0;
    static constexpr int cbo = FMT == PIX_YUYV || FMT == PIX_NV21 ? 1 : 0;
    static constexpr int cro = FMT == PIX_YUYV ? 3 : FMT == PIX_UYVY ? 2 : FMT == PIX_NV21 ? 0 : 1;
};
// the chroma row of row y (srow: its row of plane 0): the second plane's, or for one plane the row itself
template <int FMT, typename P>
__device__ __forceinline__ P* fmt_crow(const FmtImage& e, int y, P* srow) {
    if constexpr (FmtTraits<FMT>::two_planes)
        return e.data2 + (size_t)(FmtTraits<FMT>::c422 ? y : y / 2) * e.pitch2;
    else
        return srow;
}

__device__ __forceinline__ unsigned fmt_clip(int v) { return (unsigned)max(0, min(v, 255)); }
__device__ __forceinline__ void nv12_decode(const Nv12K& k, int Y, int Cb, int Cr, unsigned& r, unsigned& g, unsigned& b) {
    const int c = k.ky * (Y - k.yoff), d = Cb - 128, e = Cr - 128;
    r = fmt_clip((c + k.krv * e + 32768) >> 16);
    g = fmt_clip((c - k.kgu * d - k.kgv * e + 32768) >> 16);
    b = fmt_clip((c + k.kbu * d + 32768) >> 16);
}
__device__ __forceinline__ void nv12_encode(const Nv12K& k, int r, int g, int b, unsigned& Y, unsigned& Cb, unsigned& Cr) {
    Y = fmt_clip(((k.yr * r + k.yg * g + k.yb * b + 32768) >> 16) + k.yoff);
    Cb = fmt_clip(((-k.ur * r - k.ug * g + k.ub * b + 32768) >> 16) + 128);
    Cr = fmt_clip(((k.vr * r - k.vg * g - k.vb * b + 32768) >> 16) + 128);
}
__device__ __forceinline__ unsigned fmt_byte(unsigned v, int k) { return (v >> (8 * k)) & 255u; }
// Four values 0 .. 255 as the bytes of one dword, by v_perm_b32.  Not a | (b << 8) | ...: of clip(x >> 16) | clip(y >> 16) << 8 the
// compiler makes one v_ashr_pk_u8_i32 and takes bits 16 .. 31 of its result for zero, which they were not on the MI355X -- the
// decoded pixels 2 and 3 of every group came out OR-ed with them (tests/test_gpu_pixfmt.py at 64 x 48).
__device__ __forceinline__ unsigned fmt_pack4(unsigned a, unsigned b, unsigned c, unsigned d) {
    return __builtin_amdgcn_perm(__builtin_amdgcn_perm(d, c, 0x0c0c0400u), __builtin_amdgcn_perm(b, a, 0x0c0c0400u), 0x05040100u);
}
__device__ __forceinline__ bool fmt_aligned(const void* a, const void* b, const void* c, const void* d, unsigned mask) {
    return ((reinterpret_cast<uintptr_t>(a) | reinterpret_cast<uintptr_t>(b) | reinterpret_cast<uintptr_t>(c) | reinterpret_cast<uintptr_t>(d)) & mask) == 0;
}

// ---- to planar -----------------------------------------------------------------------------------------------------------------
// One pixel of a packed row (p = its first byte), or of a Y Cb Cr row (p = its Y byte, q = the place of its chroma pair).
template <int FMT>
__device__ __forceinline__ void fmt_load_px(const uint8_t* p, const uint8_t* q, const Nv12K& k, unsigned& r, unsigned& g, unsigned& b) {
    if constexpr (FmtTraits<FMT>::yuv)
        nv12_decode(k, p[FmtTraits<FMT>::yo], q[FmtTraits<FMT>::cbo], q[FmtTraits<FMT>::cro], r, g, b);
    else
        r = p[FmtTraits<FMT>::ro], g = p[1], b = p[2 - FmtTraits<FMT>::ro];
}
// The Y of four pixels and their two chroma pairs from a 4-byte-aligned row: one dword of Y and one of chroma (two planes), or the
// two dwords of two groups (YUYV, UYVY).  p, q as above, of the four's first pixel.
template <int FMT>
__device__ __forceinline__ void fmt_yuv_4(const uint8_t* p, const uint8_t* q, int Y[4], int Cb[2], int Cr[2]) {
    using T = FmtTraits<FMT>;
    if constexpr (T::two_planes) {
        const unsigned y4 = *reinterpret_cast<const unsigned*>(p), uv = *reinterpret_cast<const unsigned*>(q);
#pragma unroll
        for (int i = 0; i < 4; ++i) Y[i] = (int)fmt_byte(y4, i);
#pragma unroll
        for (int j = 0; j < 2; ++j) Cb[j] = (int)fmt_byte(uv, 2 * j + T::cbo), Cr[j] = (int)fmt_byte(uv, 2 * j + T::cro);
    } else {
        const unsigned* s = reinterpret_cast<const unsigned*>(p);
        const unsigned v[2] = {s[0], s[1]};
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            Y[2 * j] = (int)fmt_byte(v[j], T::yo), Y[2 * j + 1] = (int)fmt_byte(v[j], T::yo + 2);
            Cb[j] = (int)fmt_byte(v[j], T::cbo), Cr[j] = (int)fmt_byte(v[j], T::cro);
        }
    }
}
// Four pixels of an aligned row as one dword per plane (byte i = pixel i).  p, q as above, of the group's first pixel.
template <int FMT>
__device__ __forceinline__ void fmt_load_4(const uint8_t* p, const uint8_t* q, bool by16, const Nv12K& k, unsigned& R, unsigned& G, unsigned& B) {
    unsigned c[3] = {0u, 0u, 0u};
    if constexpr (FmtTraits<FMT>::yuv) {
        int Y[4], Cb[2], Cr[2];
        fmt_yuv_4<FMT>(p, q, Y, Cb, Cr);
        unsigned r[4], g[4], b[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) nv12_decode(k, Y[i], Cb[i / 2], Cr[i / 2], r[i], g[i], b[i]);
        c[0] = fmt_pack4(r[0], r[1], r[2], r[3]), c[1] = fmt_pack4(g[0], g[1], g[2], g[3]), c[2] = fmt_pack4(b[0], b[1], b[2], b[3]);
    } else if constexpr (FmtTraits<FMT>::bpp == 4) {
        uint4 v;
        if (by16) {
            v = *reinterpret_cast<const uint4*>(p);
        } else {
            const unsigned* s = reinterpret_cast<const unsigned*>(p);
            v = uint4{s[0], s[1], s[2], s[3]};
        }
        const unsigned px[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) c[ch] |= fmt_byte(px[i], ch) << (8 * i);
    } else {
        const unsigned* s = reinterpret_cast<const unsigned*>(p);
        const unsigned v[3] = {s[0], s[1], s[2]};  // twelve bytes: pixel i's channel ch is byte 3 i + ch
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) c[ch] |= fmt_byte(v[(3 * i + ch) / 4], (3 * i + ch) % 4) << (8 * i);
    }
    if constexpr (FmtTraits<FMT>::yuv) {
        R = c[0], G = c[1], B = c[2];
    } else {
        R = c[FmtTraits<FMT>::ro], G = c[1], B = c[2 - FmtTraits<FMT>::ro];
    }
}

template <int FMT>
__global__ __launch_bounds__(256) void k_unpack_many(const FmtImage* __restrict__ img, int w, int h, Nv12K k) {
    const FmtImage e = img[blockIdx.z];
    constexpr int bpp = FmtTraits<FMT>::bpp;
    const size_t pl = (size_t)w * h;
    const int groups = (w + 3) / 4;
    for (int y = blockIdx.y; y < h; y += gridDim.y) {
        const uint8_t* srow = e.data + (size_t)y * e.pitch;
        const uint8_t* crow = fmt_crow<FMT>(e, y, srow);
        uint8_t* d0 = e.planar + (size_t)y * w;
        const bool wide = fmt_aligned(srow, crow, d0, d0 + pl, 3u) && fmt_aligned(d0 + 2 * pl, nullptr, nullptr, nullptr, 3u);  // block-uniform
        const bool by16 = bpp == 4 && (reinterpret_cast<uintptr_t>(srow) & 15u) == 0;
        for (int gi = blockIdx.x * blockDim.x + threadIdx.x; gi < groups; gi += gridDim.x * blockDim.x) {
            const int x = 4 * gi, npx = min(4, w - x);
            if (wide && npx == 4) {
                unsigned R, G, B;
                fmt_load_4<FMT>(srow + (size_t)x * bpp, crow + x, by16, k, R, G, B);  // (two planes: pair x / 2 is at byte x, x a multiple of 4)
                *reinterpret_cast<unsigned*>(d0 + x) = R;
                *reinterpret_cast<unsigned*>(d0 + pl + x) = G;
                *reinterpret_cast<unsigned*>(d0 + 2 * pl + x) = B;
            } else {
                for (int i = 0; i < npx; ++i) {
                    unsigned r, g, b;
                    fmt_load_px<FMT>(srow + (size_t)(x + i) * bpp, crow + FmtTraits<FMT>::cstep * ((x + i) / 2), k, r, g, b);
                    d0[x + i] = (uint8_t)r;
                    d0[pl + x + i] = (uint8_t)g;
                    d0[2 * pl + x + i] = (uint8_t)b;
                }
            }
        }
    }
}

// ---- from planar ---------------------------------------------------------------------------------------------------------------
// The finish pass's per-pixel function (equalize_apply_bytes<true> of k_equalize.inc, by its own device functions): the pixel
// equalised through the LUT, then the luminance mix of the two.
__device__ __forceinline__ void fmt_finish_px(unsigned& r, unsigned& g, unsigned& b, const int* slut, const MixK& mk) {
    unsigned yq, cbq, crq, er, eg, eb;
    rgb_to_ycc_bins(r, g, b, yq, cbq, crq);
    ycc_bins_to_rgb((unsigned)slut[yq] & 255u, cbq, crq, er, eg, eb);
    float Y, Cb, Cr, Ye, Cbe, Cre;
    rgb_to_ycc(r, g, b, Y, Cb, Cr);
    rgb_to_ycc(er, eg, eb, Ye, Cbe, Cre);
    const float Ym = mix_y(Y, Ye, mk);
    uint8_t o0, o1, o2;
    ycc_to_rgb_u8(Ym, Cb, Cr, o0, o1, o2);
    r = o0, g = o1, b = o2;
}
template <bool FINISH>
__device__ __forceinline__ void fmt_src_px(const uint8_t* s, size_t pl, const int* slut, const MixK& mk, unsigned& r, unsigned& g, unsigned& b) {
    r = s[0], g = s[pl], b = s[2 * pl];
    if constexpr (FINISH) fmt_finish_px(r, g, b, slut, mk);
}
// four pixels from an aligned planar row, finished: one dword per channel in, r / g / b per pixel out
template <bool FINISH>
__device__ __forceinline__ void fmt_src_4(const uint8_t* s, size_t pl, const int* slut, const MixK& mk, unsigned r[4], unsigned g[4], unsigned b[4]) {
    const unsigned R = *reinterpret_cast<const unsigned*>(s), G = *reinterpret_cast<const unsigned*>(s + pl), B = *reinterpret_cast<const unsigned*>(s + 2 * pl);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        r[i] = fmt_byte(R, i), g[i] = fmt_byte(G, i), b[i] = fmt_byte(B, i);
        if constexpr (FINISH) fmt_finish_px(r[i], g[i], b[i], slut, mk);
    }
}
template <int FMT>
__device__ __forceinline__ void fmt_store_px(uint8_t* p, unsigned r, unsigned g, unsigned b) {
    p[FmtTraits<FMT>::ro] = (uint8_t)r;
    p[1] = (uint8_t)g;
    p[2 - FmtTraits<FMT>::ro] = (uint8_t)b;
    if constexpr (FmtTraits<FMT>::bpp == 4) p[3] = 255;
}
template <int FMT>
__device__ __forceinline__ void fmt_store_4(uint8_t* p, bool by16, const unsigned r[4], const unsigned g[4], const unsigned b[4]) {
    constexpr int ro = FmtTraits<FMT>::ro;
    if constexpr (FmtTraits<FMT>::bpp == 4) {
        unsigned px[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) px[i] = ((ro ? b[i] : r[i])) | (g[i] << 8) | ((ro ? r[i] : b[i]) << 16) | 0xff000000u;
        if (by16) {
            *reinterpret_cast<uint4*>(p) = uint4{px[0], px[1], px[2], px[3]};
        } else {
            unsigned* d = reinterpret_cast<unsigned*>(p);
            d[0] = px[0], d[1] = px[1], d[2] = px[2], d[3] = px[3];
        }
    } else {
        unsigned v[3] = {0u, 0u, 0u};
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const unsigned ch[3] = {ro ? b[i] : r[i], g[i], ro ? r[i] : b[i]};
#pragma unroll
            for (int c = 0; c < 3; ++c) v[(3 * i + c) / 4] |= ch[c] << (8 * ((3 * i + c) % 4));
        }
        unsigned* d = reinterpret_cast<unsigned*>(p);
        d[0] = v[0], d[1] = v[1], d[2] = v[2];
    }
}

// scratch: RIG_EQ_WORDS int32 per image as k_hist_many / k_lut_many leave them (FINISH only; the LUT is the second half)
template <int FMT, bool FINISH>
__global__ __launch_bounds__(256) void k_pack_many(const FmtImage* __restrict__ img, FmtRect rc, const int32_t* __restrict__ scratch, MixK mk, Nv12K k) {
    __shared__ int slut[256];
    if constexpr (FINISH) {
        const int32_t* lut = scratch + (size_t)blockIdx.z * RIG_EQ_WORDS + 256;
        for (int i = threadIdx.x; i < 256; i += blockDim.x) slut[i] = lut[i];
        __syncthreads();
    }
    const FmtImage e = img[blockIdx.z];
    const size_t pl = (size_t)rc.W * rc.H;
    const int w = rc.w, h = rc.h, groups = (w + 3) / 4;
    if constexpr (!FmtTraits<FMT>::yuv) {
        constexpr int bpp = FmtTraits<FMT>::bpp;
        for (int y = blockIdx.y; y < h; y += gridDim.y) {
            const uint8_t* s0 = e.planar + (size_t)(rc.y0 + y) * rc.W + rc.x0;
            uint8_t* drow = e.data + (size_t)y * e.pitch;
            const bool wide = fmt_aligned(s0, s0 + pl, s0 + 2 * pl, drow, 3u);  // block-uniform
            const bool by16 = bpp == 4 && (reinterpret_cast<uintptr_t>(drow) & 15u) == 0;
            for (int gi = blockIdx.x * blockDim.x + threadIdx.x; gi < groups; gi += gridDim.x * blockDim.x) {
                const int x = 4 * gi, npx = min(4, w - x);
                if (wide && npx == 4) {
                    unsigned r[4], g[4], b[4];
                    fmt_src_4<FINISH>(s0 + x, pl, slut, mk, r, g, b);
                    fmt_store_4<FMT>(drow + (size_t)x * bpp, by16, r, g, b);
                } else {
                    for (int i = 0; i < npx; ++i) {
                        unsigned r, g, b;
                        fmt_src_px<FINISH>(s0 + x + i, pl, slut, mk, r, g, b);
                        fmt_store_px<FMT>(drow + (size_t)(x + i) * bpp, r, g, b);
                    }
                }
            }
        }
    } else if constexpr (FmtTraits<FMT>::c422) {
        using T = FmtTraits<FMT>;
        for (int y = blockIdx.y; y < h; y += gridDim.y) {
            const uint8_t* s0 = e.planar + (size_t)(rc.y0 + y) * rc.W + rc.x0;
            uint8_t* drow = e.data + (size_t)y * e.pitch;
            uint8_t* crow = fmt_crow<FMT>(e, y, drow);
            const bool wide = fmt_aligned(s0, s0 + pl, s0 + 2 * pl, drow, 3u) && fmt_aligned(crow, nullptr, nullptr, nullptr, 3u);  // block-uniform
            for (int gi = blockIdx.x * blockDim.x + threadIdx.x; gi < groups; gi += gridDim.x * blockDim.x) {
                const int x = 4 * gi, npx = min(4, w - x);
                if (wide && npx == 4) {
                    unsigned r[4], g[4], b[4], Y[4], cb[4], cr[4];
                    fmt_src_4<FINISH>(s0 + x, pl, slut, mk, r, g, b);
#pragma unroll
                    for (int i = 0; i < 4; ++i) nv12_encode(k, (int)r[i], (int)g[i], (int)b[i], Y[i], cb[i], cr[i]);
                    const unsigned u0 = (cb[0] + cb[1] + 1u) >> 1, v0 = (cr[0] + cr[1] + 1u) >> 1, u1 = (cb[2] + cb[3] + 1u) >> 1, v1 = (cr[2] + cr[3] + 1u) >> 1;
                    if constexpr (T::two_planes) {
                        *reinterpret_cast<unsigned*>(drow + x) = fmt_pack4(Y[0], Y[1], Y[2], Y[3]);
                        *reinterpret_cast<unsigned*>(crow + x) = fmt_pack4(u0, v0, u1, v1);
                    } else {
                        unsigned* d = reinterpret_cast<unsigned*>(drow + 2 * (size_t)x);  // two groups: byte 2 x of the row on
                        d[0] = FMT == PIX_YUYV ? fmt_pack4(Y[0], u0, Y[1], v0) : fmt_pack4(u0, Y[0], v0, Y[1]);
                        d[1] = FMT == PIX_YUYV ? fmt_pack4(Y[2], u1, Y[3], v1) : fmt_pack4(u1, Y[2], v1, Y[3]);
                    }
                } else {
                    for (int i0 = 0; i0 < npx; i0 += 2) {  // one 2 x 1 pair: columns xa, xb (xb == xa on the clamped last column of an odd width)
                        const int xa = x + i0, xb = min(xa + 1, w - 1);
                        unsigned r, g, b, Ya, Yb, ua, ub, va, vb;
                        fmt_src_px<FINISH>(s0 + xa, pl, slut, mk, r, g, b);
                        nv12_encode(k, (int)r, (int)g, (int)b, Ya, ua, va);
                        fmt_src_px<FINISH>(s0 + xb, pl, slut, mk, r, g, b);
                        nv12_encode(k, (int)r, (int)g, (int)b, Yb, ub, vb);
                        uint8_t* c = crow + T::cstep * (xa / 2);  // the pair's place; one plane: the group, whose Y1 byte is a pixel byte
                        if constexpr (T::two_planes) {
                            drow[xa] = (uint8_t)Ya;
                            drow[xb] = (uint8_t)Yb;  // a clamped coordinate writes its own pixel's value again
                        } else {
                            c[T::yo] = (uint8_t)Ya;
                            c[T::yo + 2] = (uint8_t)Yb;  // ... and here the luma of pixel w - 1 into the last group's Y1
                        }
                        c[T::cbo] = (uint8_t)((ua + ub + 1u) >> 1);
                        c[T::cro] = (uint8_t)((va + vb + 1u) >> 1);
                    }
                }
            }
        }
    } else {
        const int hp = (h + 1) / 2;
        for (int j = blockIdx.y; j < hp; j += gridDim.y) {
            const int ya = 2 * j, yb = min(2 * j + 1, h - 1);  // the pair's rows; yb == ya on the clamped last row of an odd height
            const uint8_t* sa = e.planar + (size_t)(rc.y0 + ya) * rc.W + rc.x0;
            const uint8_t* sb = e.planar + (size_t)(rc.y0 + yb) * rc.W + rc.x0;
            uint8_t* da = e.data + (size_t)ya * e.pitch;
            uint8_t* db = e.data + (size_t)yb * e.pitch;
            uint8_t* dc = e.data2 + (size_t)j * e.pitch2;
            const bool wide = yb != ya && fmt_aligned(sa, sa + pl, sa + 2 * pl, sb, 3u) && fmt_aligned(sb + pl, sb + 2 * pl, da, db, 3u) &&
                              fmt_aligned(dc, nullptr, nullptr, nullptr, 3u);  // block-uniform
            for (int gi = blockIdx.x * blockDim.x + threadIdx.x; gi < groups; gi += gridDim.x * blockDim.x) {
                const int x = 4 * gi, npx = min(4, w - x);
                if (wide && npx == 4) {
                    unsigned r[4], g[4], b[4], ya4 = 0u, yb4 = 0u, cb[4], cr[4];
                    fmt_src_4<FINISH>(sa + x, pl, slut, mk, r, g, b);
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        unsigned Y;
                        nv12_encode(k, (int)r[i], (int)g[i], (int)b[i], Y, cb[i], cr[i]);
                        ya4 |= Y << (8 * i);
                    }
                    fmt_src_4<FINISH>(sb + x, pl, slut, mk, r, g, b);
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        unsigned Y, u, v;
                        nv12_encode(k, (int)r[i], (int)g[i], (int)b[i], Y, u, v);
                        yb4 |= Y << (8 * i);
                        cb[i] += u, cr[i] += v;
                    }
                    *reinterpret_cast<unsigned*>(da + x) = ya4;
                    *reinterpret_cast<unsigned*>(db + x) = yb4;
                    if constexpr (FMT == PIX_NV21)  // every pair Cr Cb
                        *reinterpret_cast<unsigned*>(dc + x) =
                            fmt_pack4((cr[0] + cr[1] + 2u) >> 2, (cb[0] + cb[1] + 2u) >> 2, (cr[2] + cr[3] + 2u) >> 2, (cb[2] + cb[3] + 2u) >> 2);
                    else
                        *reinterpret_cast<unsigned*>(dc + x) = ((cb[0] + cb[1] + 2u) >> 2) | (((cr[0] + cr[1] + 2u) >> 2) << 8) | (((cb[2] + cb[3] + 2u) >> 2) << 16) |
                                                               (((cr[2] + cr[3] + 2u) >> 2) << 24);
                } else {
                    for (int i0 = 0; i0 < npx; i0 += 2) {  // one 2 x 2 block: columns xa, xb (xb == xa on the clamped last column of an odd width)
                        const int xa = x + i0, xb = min(xa + 1, w - 1);
                        unsigned su = 0u, sv = 0u;
#pragma unroll
                        for (int q = 0; q < 4; ++q) {
                            const int xx = (q & 1) ? xb : xa;
                            const bool second_row = (q & 2) != 0;
                            unsigned r, g, b, Y, u, v;
                            fmt_src_px<FINISH>((second_row ? sb : sa) + xx, pl, slut, mk, r, g, b);
                            nv12_encode(k, (int)r, (int)g, (int)b, Y, u, v);
                            su += u, sv += v;
                            (second_row ? db : da)[xx] = (uint8_t)Y;  // a clamped coordinate writes its own pixel's value again
                        }
                        dc[2 * (xa / 2) + FmtTraits<FMT>::cbo] = (uint8_t)((su + 2u) >> 2);
                        dc[2 * (xa / 2) + FmtTraits<FMT>::cro] = (uint8_t)((sv + 2u) >> 2);
                    }
                }
            }
        }
    }
}

// ---- the projection that stages a packed source itself -----------------------------------------------------------------------------
// Four pixels of a 4-byte-aligned row as the LDS dwords pj_stage_rgbx builds (R | G << 8 | B << 16; pj_bilinear2 never reads bits
// 24 .. 31, which hold X or a neighbour's byte here): no perm for RGBX32, one per pixel for BGRX32 and the three-byte formats, the
// decode for the Y Cb Cr formats (fmt_yuv_4's dwords: a width that is a multiple of 4 keeps every 4:2:2 group whole).  p, q as for
// fmt_load_4.
template <int FMT>
__device__ __forceinline__ uint4 fmt_lds_4(const uint8_t* p, const uint8_t* q, const Nv12K& k) {
    const unsigned* s = reinterpret_cast<const unsigned*>(p);
    if constexpr (FmtTraits<FMT>::yuv) {
        int Y[4], Cb[2], Cr[2];
        fmt_yuv_4<FMT>(p, q, Y, Cb, Cr);
        unsigned px[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            unsigned r, g, b;
            nv12_decode(k, Y[i], Cb[i / 2], Cr[i / 2], r, g, b);
            px[i] = fmt_pack4(r, g, b, 0u);
        }
        return uint4{px[0], px[1], px[2], px[3]};
    } else if constexpr (FMT == PIX_RGBX32) {
        return uint4{s[0], s[1], s[2], s[3]};
    } else if constexpr (FMT == PIX_BGRX32) {
        return uint4{__builtin_amdgcn_perm(0u, s[0], 0x0c000102u), __builtin_amdgcn_perm(0u, s[1], 0x0c000102u), __builtin_amdgcn_perm(0u, s[2], 0x0c000102u),
                     __builtin_amdgcn_perm(0u, s[3], 0x0c000102u)};
    } else if constexpr (FMT == PIX_RGB24) {  // bytes 3 i .. 3 i + 2 of the twelve
        const unsigned v0 = s[0], v1 = s[1], v2 = s[2];
        return uint4{v0, __builtin_amdgcn_perm(v1, v0, 0x0c050403u), __builtin_amdgcn_perm(v2, v1, 0x0c040302u), v2 >> 8};
    } else {  // BGR24: the same bytes, ends swapped
        const unsigned v0 = s[0], v1 = s[1], v2 = s[2];
        return uint4{__builtin_amdgcn_perm(0u, v0, 0x0c000102u), __builtin_amdgcn_perm(v1, v0, 0x0c030405u), __builtin_amdgcn_perm(v2, v1, 0x0c020304u),
                     __builtin_amdgcn_perm(0u, v2, 0x0c010203u)};
    }
}
// The staging policy (k_project_lds.inc): the box's rows r0 .. r0 + nrow - 1, columns c0a .. c0a + ncol - 1 (both multiples of 16) into
// one dword per pixel.  64 lanes across a row's groups of four pixels, 4 rows per pass.  The frame's width is a multiple of four (the
// tiled form asks that), so a group lies inside the row or behind it: those behind are zero and never sampled.  Rows are 4-byte
// aligned: the host sends any other frame through k_unpack_many.  Only pixel bytes are read, never padding.
template <int FMT>
struct PjStageFmt {
    static constexpr bool kPlanarSource = false;
    FmtImage e;
    Nv12K k;
    __device__ __forceinline__ void operator()(const uint8_t*, size_t, int w, int r0, int nrow, int c0a, int ncol, uint8_t* smem) const {
        constexpr int bpp = FmtTraits<FMT>::bpp;
        const int gpr = ncol >> 2, lc = threadIdx.x & 63, lr = threadIdx.x >> 6;
        for (int rr = lr; rr < nrow; rr += 4) {
            const int y = r0 + rr;
            const uint8_t* srow = e.data + (size_t)y * e.pitch;
            const uint8_t* crow = fmt_crow<FMT>(e, y, srow);
            for (int g = lc; g < gpr; g += 64) {
                const int x = c0a + 4 * g;
                uint4 v = uint4{0u, 0u, 0u, 0u};
                if (x + 3 < w) v = fmt_lds_4<FMT>(srow + (size_t)x * bpp, crow + x, k);
                *reinterpret_cast<uint4*>(smem + ((size_t)rr * ncol + 4 * g) * 4) = v;
            }
        }
    }
};
// blockIdx.z = image; the entry's planar image is the projection's destination
template <int FMT, int TW, int TH>
__global__ __launch_bounds__(256) void k_project_fmt_lds_many(const FmtImage* __restrict__ img, int w, int h, float r, int lds_bytes, Nv12K k) {
    const FmtImage e = img[blockIdx.z];
    project_lds_tile<uint8_t, TW, TH, PjStageFmt<FMT>>(nullptr, e.planar, w, h, r, nullptr, nullptr, lds_bytes, PjStageFmt<FMT>{e, k});
}
template <int FMT, int TW, int TH>
__global__ __launch_bounds__(256) void k_project_fmt_lds_t_many(const FmtImage* __restrict__ img, int w, int h, float r, int lds_bytes, Nv12K k) {
    const FmtImage e = img[blockIdx.z];
    project_lds_tile_t<uint8_t, TW, TH, PjStageFmt<FMT>>(nullptr, e.planar, w, h, r, nullptr, nullptr, lds_bytes, PjStageFmt<FMT>{e, k});
}
