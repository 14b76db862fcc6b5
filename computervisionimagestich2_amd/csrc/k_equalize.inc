// Part of stitch_kernels.hpp (included there, inside namespace sk): equalisation and luminance mix (E1-E3, M1).
// ---- E1-E3 / M1: equalisation and luminance mix --------------------------------------------------------------
__device__ __forceinline__ float clamp256(float v) { return v > 0 ? (v < 256 ? v : 255.f) : 0.f; }
// (unsigned char)(int)clamp256(v) in two instructions: the median of (v, 0, 255.5) truncates to the same byte -- v <= 0 -> 0,
// 0 < v < 255.5 -> v itself, 255.5 <= v < 256 -> 255.5 -> 255 (clamp256 keeps v, which truncates to 255 too), v >= 256 -> 255;
// a NaN gives 0 either way (v_med3_f32 returns the minimum of the other two).
__device__ __forceinline__ uint8_t clamp256_u8(float v) { return (uint8_t)(int)__builtin_amdgcn_fmed3f(v, 0.f, 255.5f); }
// ---- the colour transforms on BYTE inputs, in integers -------------------------------------------------------------------
// equalization.cpp:78-80 / ImageProcess.cpp:242-244 evaluate   Y  = 0.299 R + 0.857 G + 0.114 B   (0.857 sic)
//                                                              Cb = 128 - 0.168736 R - 0.331264 G + 0.5 B
//                                                              Cr = 128 + 0.5 R - 0.418688 G - 0.081312 B
// in double, store to float and clamp in float.  R, G, B are bytes, so the exact values are t / 1000 and t / 10^6 with integer
// t (ycc_terms); the double evaluation is within 1e-13 of them, and no t / 10^k comes within 7e-9 of a point where the float
// rounding could go either way -- so   (float)((double)t * 1e-k)   IS the reference's float, and its truncation (the
// CImg<unsigned char> store of equalization.cpp:83-85) is the integer quotient t / 10^k (Cb and Cr lie in 0.5 .. 255.5 and all
// their t are multiples of 32, never just below an integer).  Likewise the way back from BYTE Y, Cb, Cr (equalization.cpp:93-98):
// Y + 1.402 (Cr-128) etc. are t / 1000 and t / 10^5, the clamp and the truncation are max(0, min(255, t / 10^k)).
// tests/test_oracle_golden.py::test_integer_colour_transforms_are_exact checks every one of the 2^24 inputs of either direction
// against the double / float expressions; the GPU kernels are compared with the oracle on an image that holds every colour.
// A pixel costs a few integer multiply-adds instead of ~25 double-precision operations and their conversions.
struct YccTerms {
    unsigned ty, tcb, tcr;  // 1000 Y, 10^6 Cb, 10^6 Cr
};
__device__ __forceinline__ YccTerms ycc_terms(unsigned r, unsigned g, unsigned b) {
    YccTerms t;
    t.ty = 299u * r + 857u * g + 114u * b;
    t.tcb = 128000000u - 168736u * r - 331264u * g + 500000u * b;  // 0.5e6 .. 255.5e6
    t.tcr = 128000000u + 500000u * r - 418688u * g - 81312u * b;
    return t;
}
// the float Y, Cb, Cr the reference holds (ImageProcess.cpp:242-244: not truncated there)
__device__ __forceinline__ void rgb_to_ycc(unsigned r, unsigned g, unsigned b, float& Y, float& Cb, float& Cr) {
    const YccTerms t = ycc_terms(r, g, b);
    const float y = (float)((double)t.ty * 0.001);
    Y = y < 256.f ? y : 255.f;            // clamp256: y >= 0 always, and 0 maps to 0 either way
    Cb = (float)((double)t.tcb * 1e-6);  // 0.5 .. 255.5: clamp256 is the identity there
    Cr = (float)((double)t.tcr * 1e-6);
}
// the bytes equalization.cpp:83-85 stores
__device__ __forceinline__ void rgb_to_ycc_bins(unsigned r, unsigned g, unsigned b, unsigned& yq, unsigned& cbq, unsigned& crq) {
    const YccTerms t = ycc_terms(r, g, b);
    const unsigned q = t.ty / 1000u;
    yq = q < 255u ? q : 255u;
    cbq = t.tcb / 1000000u;
    crq = t.tcr / 1000000u;
}
// max(0, min(255, t / d)) for d > 0, branch-free: clamp the dividend (one v_med3_i32), then one unsigned division by a constant
__device__ __forceinline__ unsigned clamp_quot(int t, int d) { return (unsigned)max(0, min(t, 256 * d - 1)) / (unsigned)d; }
// equalization.cpp:93-98 on byte Y, Cb, Cr
__device__ __forceinline__ void ycc_bins_to_rgb(unsigned y, unsigned cb, unsigned cr, unsigned& r, unsigned& g, unsigned& b) {
    const int Y = (int)y, cbd = (int)cb - 128, crd = (int)cr - 128;
    r = clamp_quot(1000 * Y + 1402 * crd, 1000);
    g = clamp_quot(100000 * Y - 34414 * cbd - 71414 * crd, 100000);
    b = clamp_quot(1000 * Y + 1772 * cbd, 1000);
}
// ImageProcess.cpp:261: Y = Y*num/den + Yeq/den in double, stored to float.  The two IEEE divides are a third of the mix's
// double-precision work.  With rden = RN(1/den) the quotient a/den can be had as q = a*rden, r = fma(-q, den, a), q + r*rden
// (three operations), which is the correctly rounded quotient for almost every a -- "almost" is not good enough here, so the
// HOST decides per (num, den): Y and Yeq can only be one of the 323 851 floats (float)(t/1000), t = 0 .. 323 850 (ycc_terms),
// so it evaluates both forms for every one of them (mix_fastdiv_ok in stitch_hip.hip, cached per pair of parameters) and passes
// rden only if they agree on all; otherwise rden = 0 and the kernels divide.
struct MixK {
    double num, den, rden;  // rden = 0: use the IEEE divide
};
__device__ __forceinline__ double mix_quot(double a, const MixK& k) {
    if (k.rden == 0.0) return a / k.den;  // wave-uniform
    const double q = a * k.rden;
    const double r = __builtin_fma(-q, k.den, a);
    return __builtin_fma(r, k.rden, q);
}
__device__ __forceinline__ float mix_y(float Y, float Ye, const MixK& k) {
    return (float)(mix_quot((double)Y * k.num, k) + mix_quot((double)Ye, k));
}
// equalization.cpp:93-98 / ImageProcess.cpp:262-267 on float inputs (the luminance mix)
__device__ __forceinline__ void ycc_to_rgb_u8(float Y, float Cb, float Cr, uint8_t& r, uint8_t& g, uint8_t& b) {
    const float R = (float)((double)Y + 1.402 * ((double)Cr - 128.0));
    const float G = (float)((double)Y - 0.34414 * ((double)Cb - 128.0) - 0.71414 * ((double)Cr - 128.0));
    const float B = (float)((double)Y + 1.772 * ((double)Cb - 128.0));
    r = clamp256_u8(R);
    g = clamp256_u8(G);
    b = clamp256_u8(B);
}

// The histogram bin of a pixel in integers.  The reference evaluates Y = 0.299 R + 0.857 G + 0.114 B in double, rounds to
// float, clamps and truncates (equalization.cpp:78, :83-85, then `hist[Y]`).  R, G, B are integers 0..255, so the exact sum
// is t / 1000 with t = 299 R + 857 G + 114 B: either an integer or at least 0.001 away from one, while the double and float
// roundings move the value by less than 2e-5 -- the truncation therefore equals floor(t / 1000), capped at 255 by the clamp.
// tests/test_oracle_golden.py::test_integer_luma_bin_is_exact checks all 2^24 colours against the oracle.
__device__ __forceinline__ unsigned luma_bin(unsigned r, unsigned g, unsigned b) {
    const unsigned q = (299u * r + 857u * g + 114u * b) / 1000u;
    return q < 255u ? q : 255u;
}

// Y histogram (equalization.cpp:104-107): each wavefront owns a private 256-bin LDS histogram (no cross-wave
// contention), the workgroup's wavefronts are summed through LDS, and each bin is flushed with one global
// atomic per workgroup.  Four pixels per work-item per step (uchar4 loads when the plane size allows).
// (The bodies of these kernels are device functions so that the many-mosaic forms of k_rig.inc run them per mosaic of a batch:
// blockIdx.x / gridDim.x address the samples.)
constexpr int HIST_WAVES = 4;
__device__ __forceinline__ void hist_bytes(const uint8_t* __restrict__ img, size_t n, int32_t* __restrict__ hist) {
    __shared__ int lh[HIST_WAVES][256];
    const int wid = threadIdx.x >> 6;
    for (int i = threadIdx.x; i < HIST_WAVES * 256; i += blockDim.x) (&lh[0][0])[i] = 0;
    __syncthreads();
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        atomicAdd(&lh[wid][luma_bin(img[i], img[i + n], img[i + 2 * n])], 1);
    }
    __syncthreads();
    for (int b = threadIdx.x; b < 256; b += blockDim.x) {
        int s = 0;
#pragma unroll
        for (int k2 = 0; k2 < HIST_WAVES; ++k2) s += lh[k2][b];
        if (s) atomicAdd(&hist[b], s);
    }
}
__global__ __launch_bounds__(HIST_WAVES * 64) void k_hist(const uint8_t* __restrict__ img, size_t n, int32_t* __restrict__ hist) {
    hist_bytes(img, n, hist);
}

// CDF and LUT (equalization.cpp:110-124): p_i = hist_i / total for all bins side by side (the divisions are independent),
// then the running sum as 256 sequential double additions on one lane -- its order is the reference's, so the sum is
// bit-identical -- then lut_i = round(255 cdf_i) side by side again; round() is half-away-from-zero.  (All on one lane this took
// 20 us -- a sixth of an equalisation of 25 MPix: every iteration waited for a double-precision divide.)
__device__ __forceinline__ void lut_of_hist(const int32_t* __restrict__ hist, int w, int h, int32_t* __restrict__ lut) {
    __shared__ double pc[256];
    const double total = (double)(w * h);
    const int i = threadIdx.x;
    pc[i] = (double)hist[i] / total;
    __syncthreads();
    if (i == 0) {
        double cdf = pc[0];
        for (int j = 1; j < 256; ++j) {
            cdf = cdf + pc[j];
            pc[j] = cdf;
        }
    }
    __syncthreads();
    lut[i] = (int32_t)round(255.0 * pc[i]);
}
__global__ __launch_bounds__(256) void k_lut(const int32_t* __restrict__ hist, int w, int h, int32_t* __restrict__ lut) {
    lut_of_hist(hist, w, h, lut);
}

// apply (equalization.cpp:127-130 + :92-99), in place; FUSE_MIX additionally performs M1 so that the equalised
// copy never exists in memory (stitch_dev_finish_u8).
template <bool FUSE_MIX>
__device__ __forceinline__ void equalize_apply_bytes(uint8_t* __restrict__ img, size_t n, const int32_t* __restrict__ lut, const MixK& mk) {
    __shared__ int slut[256];
    for (int i = threadIdx.x; i < 256; i += blockDim.x) slut[i] = lut[i];
    __syncthreads();
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const unsigned r = img[i], g = img[i + n], b = img[i + 2 * n];
        unsigned yq, cbq, crq, er, eg, eb;
        rgb_to_ycc_bins(r, g, b, yq, cbq, crq);  // CImg<uchar> store
        ycc_bins_to_rgb((unsigned)slut[yq] & 255u, cbq, crq, er, eg, eb);
        uint8_t o0 = (uint8_t)er, o1 = (uint8_t)eg, o2 = (uint8_t)eb;
        if (FUSE_MIX) {
            float Y, Cb, Cr, Ye, Cbe, Cre;
            rgb_to_ycc(r, g, b, Y, Cb, Cr);
            rgb_to_ycc(er, eg, eb, Ye, Cbe, Cre);
            const float Ym = mix_y(Y, Ye, mk);  // ImageProcess.cpp:261
            ycc_to_rgb_u8(Ym, Cb, Cr, o0, o1, o2);
        }
        img[i] = o0;
        img[i + n] = o1;
        img[i + 2 * n] = o2;
    }
}
template <bool FUSE_MIX>
__global__ __launch_bounds__(256) void k_equalize_apply(uint8_t* __restrict__ img, size_t n, const int32_t* __restrict__ lut, MixK mk) {
    equalize_apply_bytes<FUSE_MIX>(img, n, lut, mk);
}

// M1 stand-alone, ImageProcess.cpp:240-268
__global__ __launch_bounds__(256) void k_lummix(uint8_t* __restrict__ res, const uint8_t* __restrict__ eq, size_t n, MixK mk) {
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        float Y, Cb, Cr, Ye, Cbe, Cre;
        rgb_to_ycc(res[i], res[i + n], res[i + 2 * n], Y, Cb, Cr);
        rgb_to_ycc(eq[i], eq[i + n], eq[i + 2 * n], Ye, Cbe, Cre);
        const float Ym = mix_y(Y, Ye, mk);
        uint8_t r, g, b;
        ycc_to_rgb_u8(Ym, Cb, Cr, r, g, b);
        res[i] = r;
        res[i + n] = g;
        res[i + 2 * n] = b;
    }
}

// ---- histogram and apply, four pixels per work-item and step (planes of n % 4 == 0 bytes at 4-byte aligned bases) ----
// Every plane is moved as 32-bit words (4 pixels) instead of bytes; the arithmetic per pixel is unchanged (these kernels
// are bound by their double-precision conversions, so the gain is modest: equalise 0.167 -> 0.150 ms, finish 0.234 -> 0.203
// at 6144 x 4096; the luminance mix alone is no faster this way, 0.108 against 0.100, and stays a byte kernel).  The histogram keeps HIST_COPIES copies per wavefront (lane & 7 picks one; rows padded to 257 words so
// that equal bins of different copies fall into different banks): images saturate (the 0.857 coefficient pushes bright
// pixels to Y = 255) and neighbouring pixels share bins, and LDS atomics on one address serialise.
constexpr int HIST_COPIES = 8, HIST_PITCH = 257;
typedef unsigned u4a __attribute__((ext_vector_type(4), aligned(4)));  // 16-byte access at 4-byte alignment
__device__ __forceinline__ void unpack4(unsigned w, float v[4]) {
    v[0] = (float)(w & 255u), v[1] = (float)((w >> 8) & 255u), v[2] = (float)((w >> 16) & 255u), v[3] = (float)(w >> 24);
}
__device__ __forceinline__ void hist_words(const uint8_t* __restrict__ img, size_t n, int32_t* __restrict__ hist) {
    __shared__ int lh[HIST_WAVES * HIST_COPIES * HIST_PITCH];
    for (int i = threadIdx.x; i < HIST_WAVES * HIST_COPIES * HIST_PITCH; i += blockDim.x) lh[i] = 0;
    __syncthreads();
    int* mine = lh + ((threadIdx.x >> 6) * HIST_COPIES + (threadIdx.x & (HIST_COPIES - 1))) * HIST_PITCH;
    const unsigned* __restrict__ pr = reinterpret_cast<const unsigned*>(img);
    const unsigned* __restrict__ pg = reinterpret_cast<const unsigned*>(img + n);
    const unsigned* __restrict__ pb = reinterpret_cast<const unsigned*>(img + 2 * n);
    const size_t n4 = n / 4, n16 = n4 / 4, stride = (size_t)gridDim.x * blockDim.x;
    // sixteen pixels per step (dword-aligned 16-byte loads): with 512 workgroups a work-item walks dozens of steps, and a step
    // is load -> wait -> atomics; four words per load keep four times the bytes in flight (29 -> 17 us at 25 MPix)
    const u4a* __restrict__ qr = reinterpret_cast<const u4a*>(pr);
    const u4a* __restrict__ qg = reinterpret_cast<const u4a*>(pg);
    const u4a* __restrict__ qb = reinterpret_cast<const u4a*>(pb);
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n16; i += stride) {
        const u4a r4 = qr[i], g4 = qg[i], b4 = qb[i];
#pragma unroll
        for (int k2 = 0; k2 < 4; ++k2) {
            const unsigned r = r4[k2], g = g4[k2], b = b4[k2];
#pragma unroll
            for (int j = 0; j < 4; ++j) atomicAdd(&mine[luma_bin((r >> (8 * j)) & 255u, (g >> (8 * j)) & 255u, (b >> (8 * j)) & 255u)], 1);
        }
    }
    for (size_t i = n16 * 4 + (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += stride) {  // up to three words left over
        const unsigned r = pr[i], g = pg[i], b = pb[i];
#pragma unroll
        for (int j = 0; j < 4; ++j) atomicAdd(&mine[luma_bin((r >> (8 * j)) & 255u, (g >> (8 * j)) & 255u, (b >> (8 * j)) & 255u)], 1);
    }
    __syncthreads();
    for (int bin = threadIdx.x; bin < 256; bin += blockDim.x) {
        int s_ = 0;
#pragma unroll
        for (int k2 = 0; k2 < HIST_WAVES * HIST_COPIES; ++k2) s_ += lh[k2 * HIST_PITCH + bin];
        if (s_) atomicAdd(&hist[bin], s_);
    }
}
__global__ __launch_bounds__(HIST_WAVES * 64) void k_hist4(const uint8_t* __restrict__ img, size_t n, int32_t* __restrict__ hist) {
    hist_words(img, n, hist);
}

template <bool FUSE_MIX>
__device__ __forceinline__ void equalize_apply_words(uint8_t* __restrict__ img, size_t n, const int32_t* __restrict__ lut, const MixK& mk) {
    __shared__ int slut[256];
    for (int i = threadIdx.x; i < 256; i += blockDim.x) slut[i] = lut[i];
    __syncthreads();
    unsigned* __restrict__ pr = reinterpret_cast<unsigned*>(img);
    unsigned* __restrict__ pg = reinterpret_cast<unsigned*>(img + n);
    unsigned* __restrict__ pb = reinterpret_cast<unsigned*>(img + 2 * n);
    const size_t n4 = n / 4, n16 = n4 / 4, stride = (size_t)gridDim.x * blockDim.x;
    auto word = [&](unsigned wr, unsigned wg, unsigned wb, unsigned& o_r, unsigned& o_g, unsigned& o_b) {
        o_r = o_g = o_b = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const unsigned r = (wr >> (8 * j)) & 255u, g = (wg >> (8 * j)) & 255u, b = (wb >> (8 * j)) & 255u;
            unsigned yq, cbq, crq, er, eg, eb;
            rgb_to_ycc_bins(r, g, b, yq, cbq, crq);  // CImg<uchar> store
            ycc_bins_to_rgb((unsigned)slut[yq] & 255u, cbq, crq, er, eg, eb);
            if (FUSE_MIX) {
                float Y, Cb, Cr, Ye, Cbe, Cre;
                rgb_to_ycc(r, g, b, Y, Cb, Cr);
                rgb_to_ycc(er, eg, eb, Ye, Cbe, Cre);
                const float Ym = mix_y(Y, Ye, mk);  // ImageProcess.cpp:261
                uint8_t m0, m1, m2;
                ycc_to_rgb_u8(Ym, Cb, Cr, m0, m1, m2);
                er = m0, eg = m1, eb = m2;
            }
            o_r |= er << (8 * j);
            o_g |= eg << (8 * j);
            o_b |= eb << (8 * j);
        }
    };
    // sixteen pixels per step (dword-aligned 16-byte accesses), then the up to three words left over
    u4a* __restrict__ qr = reinterpret_cast<u4a*>(pr);
    u4a* __restrict__ qg = reinterpret_cast<u4a*>(pg);
    u4a* __restrict__ qb = reinterpret_cast<u4a*>(pb);
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n16; i += stride) {
        const u4a r4 = qr[i], g4 = qg[i], b4 = qb[i];
        u4a o_r, o_g, o_b;
#pragma unroll
        for (int k2 = 0; k2 < 4; ++k2) {
            unsigned a, b, c;
            word(r4[k2], g4[k2], b4[k2], a, b, c);
            o_r[k2] = a, o_g[k2] = b, o_b[k2] = c;
        }
        qr[i] = o_r;
        qg[i] = o_g;
        qb[i] = o_b;
    }
    for (size_t i = n16 * 4 + (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += stride) {
        unsigned a, b, c;
        word(pr[i], pg[i], pb[i], a, b, c);
        pr[i] = a;
        pg[i] = b;
        pb[i] = c;
    }
}
template <bool FUSE_MIX>
__global__ __launch_bounds__(256) void k_equalize_apply4(uint8_t* __restrict__ img, size_t n, const int32_t* __restrict__ lut, MixK mk) {
    equalize_apply_words<FUSE_MIX>(img, n, lut, mk);
}
