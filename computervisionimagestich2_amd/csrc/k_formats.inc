// Part of stitch_kernels.hpp (included there, inside namespace sk): gray + SIFT staging, BMP decode/encode, colour transfer (SURVEY.md 8(f)).
// ---- gray conversion + SIFT input staging (SURVEY.md 8(f) row 1) ---------------------------------------------
// ImageProcess::toGrayScale, ImageProcess.cpp:27-40: gray = 0.299*R + 0.587*G + 0.114*B evaluated in double on
// float-cast pixels, stored to unsigned char by truncation; siftAlgorithm stages it as float (:47-51).
__device__ __forceinline__ uint8_t gray_ref(uint8_t r, uint8_t g, uint8_t b) {
    return (uint8_t)(int)(0.299 * (double)(float)r + 0.587 * (double)(float)g + 0.114 * (double)(float)b);
}
__global__ __launch_bounds__(256) void k_gray(const uint8_t* __restrict__ rgb, size_t n, uint8_t* __restrict__ gray,
                                              float* __restrict__ gray_f32) {
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const uint8_t v = gray_ref(rgb[i], rgb[i + n], rgb[i + 2 * n]);
        if (gray) gray[i] = v;
        if (gray_f32) gray_f32[i] = (float)v;
    }
}

// ---- BMP <-> planar RGB (CImg.h:48395-48566 _load_bmp, :52614-52700 _save_bmp) ------------------------------
// The on-disk format either side of the path: rows bottom-up (or top-down when the header height is negative), bytes
// B G R [X], rows padded to 4 bytes.  One workgroup moves 1024 pixels of one file row; the file side is accessed in
// A-byte units (A = the alignment the file position allows, usually 2 because pixel data starts at byte 54), staged
// through LDS so that both the interleaved file bytes and the three planar rows are moved by coalesced accesses.
struct BmpGeom {
    int w, h, bp, top_down;  // bp = bytes per pixel in the file (3 or 4)
    unsigned long long data_pos, stride, data_bytes;
    int planar_vec;  // planar rows start 4-byte aligned (w % 4 == 0 and an aligned base): uchar4 accesses
};
constexpr int BMP_SEG = 1024;  // pixels per workgroup
template <int A>
struct BmpUnit;
template <>
struct BmpUnit<1> { typedef uint8_t type; };
template <>
struct BmpUnit<2> { typedef uint16_t type; };
template <>
struct BmpUnit<4> { typedef uint32_t type; };

template <int A>
__global__ __launch_bounds__(256) void k_bmp_decode(const uint8_t* __restrict__ file, BmpGeom g, uint8_t* __restrict__ planar) {
    typedef typename BmpUnit<A>::type U;
    __shared__ __attribute__((aligned(16))) uint8_t seg[BMP_SEG * 4];
    const int x0 = blockIdx.x * BMP_SEG, r = blockIdx.y;  // r = row in file order
    const int npx = min(BMP_SEG, g.w - x0), nbytes = npx * g.bp;
    const unsigned long long row_off = (unsigned long long)r * g.stride + (unsigned long long)x0 * g.bp;  // within the pixel data
    const uint8_t* src = file + g.data_pos + row_off;
    for (int u = threadIdx.x; u * A < nbytes; u += 256) {
        const unsigned long long o = row_off + (unsigned long long)u * A;
        U v = 0;
        if (o + A <= g.data_bytes)
            v = reinterpret_cast<const U*>(src)[u];
        else  // a file that ends early: the reference's zero-filled buffer (CImg.h:48445)
            for (int k = 0; k < A; ++k)
                if (o + k < g.data_bytes) v |= (U)((U)src[(size_t)u * A + k] << (8 * k));
        reinterpret_cast<U*>(seg)[u] = v;
    }
    __syncthreads();
    const int x = 4 * threadIdx.x;
    if (x >= npx) return;
    const int y = g.top_down ? r : g.h - 1 - r;  // CImg.h:48536 (rows arrive last-first), :48563 (mirror when dy < 0)
    const size_t pl = (size_t)g.w * g.h, o = (size_t)y * g.w + x0 + x;
    const uint8_t* p = seg + x * g.bp;
#pragma unroll
    for (int c = 0; c < 3; ++c) {  // channel c = byte 2 - c of the pixel (CImg.h:48540-48542)
        if (g.planar_vec) {
            uchar4 v;
            v.x = p[2 - c];
            v.y = p[g.bp + 2 - c];
            v.z = p[2 * g.bp + 2 - c];
            v.w = p[3 * g.bp + 2 - c];
            *reinterpret_cast<uchar4*>(planar + c * pl + o) = v;
        } else
            for (int j = 0; j < 4 && x + j < npx; ++j) planar[c * pl + o + j] = p[j * g.bp + 2 - c];
    }
}

struct BmpHeader {
    uint8_t b[56];
};
template <int A>
__global__ __launch_bounds__(256) void k_bmp_encode(const uint8_t* __restrict__ planar, BmpGeom g, BmpHeader hdr, uint8_t* __restrict__ file) {
    typedef typename BmpUnit<A>::type U;
    __shared__ __attribute__((aligned(16))) uint8_t seg[BMP_SEG * 3 + 16];
    const int x0 = blockIdx.x * BMP_SEG, r = blockIdx.y;
    if (blockIdx.x == 0 && r == 0 && threadIdx.x < 54) file[threadIdx.x] = hdr.b[threadIdx.x];
    const int y = g.h - 1 - r;  // bottom-up (CImg.h:52672-52674, :52698)
    const size_t pl = (size_t)g.w * g.h;
    {
        const int x = x0 + 4 * threadIdx.x;
        uint8_t px[3][4] = {{0, 0, 0, 0}, {0, 0, 0, 0}, {0, 0, 0, 0}};  // pixels beyond the row stay 0 = the row padding
        const size_t o = (size_t)y * g.w + x;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            if (g.planar_vec && x + 3 < g.w) {
                const uchar4 v = *reinterpret_cast<const uchar4*>(planar + c * pl + o);
                px[c][0] = v.x;
                px[c][1] = v.y;
                px[c][2] = v.z;
                px[c][3] = v.w;
            } else
                for (int j = 0; j < 4; ++j)
                    if (x + j < g.w) px[c][j] = planar[c * pl + o + j];
        }
        uint8_t* p = seg + 12 * threadIdx.x;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            p[3 * j] = px[2][j];
            p[3 * j + 1] = px[1][j];
            p[3 * j + 2] = px[0][j];
        }
    }
    __syncthreads();
    // bytes of this row segment in the file: up to the end of the row including its padding
    const unsigned long long seg_off = (unsigned long long)x0 * 3;
    const int nbytes = (int)min((unsigned long long)BMP_SEG * 3, g.stride - seg_off);
    uint8_t* dst = file + 54 + (unsigned long long)r * g.stride + seg_off;
    for (int u = threadIdx.x; u * A < nbytes; u += 256) reinterpret_cast<U*>(dst)[u] = reinterpret_cast<const U*>(seg)[u];
}

// ---- l-alpha-beta colour transfer, transfer.cpp:3-13,125-225 (SURVEY.md 8(f) row 4; dead code in the reference) --
// The per-pixel arithmetic with every float/double promotion where the C++ puts it; std::log(float) and
// std::pow(10, float) are the specified functions of include/stitch_elem.h (see there).  Constants that the reference
// obtains from sqrt() are evaluated on the host.
struct TrK {
    float a1, b1, c1;  // 1/sqrt(3), 1/sqrt(6), 1/sqrt(2) as float (transfer.cpp:193-195)
    float a2, b2, c2;  // sqrt(3)/3, sqrt(6)/6, sqrt(2)/2 as float (transfer.cpp:204-206)
    double ln10;       // log(10)
};
__device__ __forceinline__ void tr_rgb_to_lab(const TrK& k, float R, float G, float B, float& L, float& a, float& b) {
    float l = (float)(0.3811 * (double)R + 0.5783 * (double)G + 0.0402 * (double)B);
    float m = (float)(0.1967 * (double)R + 0.7244 * (double)G + 0.0782 * (double)B);
    float s = (float)(0.0241 * (double)R + 0.1288 * (double)G + 0.8444 * (double)B);
    if (l == 0) l = 1;
    if (m == 0) m = 1;
    if (s == 0) s = 1;
    l = (float)((double)stitch_elem_logf(l) / k.ln10);
    m = (float)((double)stitch_elem_logf(m) / k.ln10);
    s = (float)((double)stitch_elem_logf(s) / k.ln10);
    L = k.a1 * ((l + m) + s);
    a = (float)((double)(k.b1 * l + k.b1 * m) - (2.0 * (double)k.b1) * (double)s);
    b = k.c1 * l - k.c1 * m;
}
__device__ __forceinline__ void tr_lab_to_rgb(const TrK& k, float L, float a, float b, float& R, float& G, float& B) {
    float l = (k.a2 * L + k.b2 * a) + k.c2 * b;
    float m = (k.a2 * L + k.b2 * a) - k.c2 * b;
    float s = (float)((double)(k.a2 * L) - (2.0 * (double)k.b2) * (double)a);
    l = (float)stitch_elem_pow10((double)l);
    m = (float)stitch_elem_pow10((double)m);
    s = (float)stitch_elem_pow10((double)s);
    const float r = (float)((4.4679 * (double)l - 3.5873 * (double)m) + 0.1193 * (double)s);
    const float g = (float)(((-1.2186) * (double)l + 2.3809 * (double)m) - 0.1624 * (double)s);
    const float bb = (float)((0.0497 * (double)l - 0.2439 * (double)m) + 1.2045 * (double)s);
    R = r > 0.0f ? (r < 255.0f ? r : 255.0f) : 0.0f;
    G = g > 0.0f ? (g < 255.0f ? g : 255.0f) : 0.0f;
    B = bb > 0.0f ? (bb < 255.0f ? bb : 255.0f) : 0.0f;
}
// One image's pixels, strided over the x dimension of the grid (k_rig_exposure.inc runs the same per image of a many-image launch).
__device__ __forceinline__ void tr_to_lab_image(const uint8_t* __restrict__ rgb, size_t n, const TrK& k, float* __restrict__ lab) {
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        float L, a, b;
        tr_rgb_to_lab(k, (float)rgb[i], (float)rgb[i + n], (float)rgb[i + 2 * n], L, a, b);
        lab[i] = L;
        lab[i + n] = a;
        lab[i + 2 * n] = b;
    }
}
__global__ __launch_bounds__(256) void k_tr_to_lab(const uint8_t* __restrict__ rgb, size_t n, TrK k, float* __restrict__ lab) {
    tr_to_lab_image(rgb, n, k, lab);
}
// transfer.cpp:128-164: mean and standard deviation with FLOAT accumulators in raster order.  A float running sum is
// not associative, so the order is kept: one wavefront per (image, channel) chain walks its plane serially; the 64
// lanes only fetch (256 samples ahead, double-buffered in LDS) and square, every lane then adds the same samples in
// the same order.  Six chains run side by side.  stats = [mean_src[3], sd_src[3], mean_tem[3], sd_tem[3]].
// One chain: the wavefront's walk over plane p of n samples (csrc/k_exposure.inc runs the same walk as its form 0).
__device__ __forceinline__ void tr_stats_chain(const float* __restrict__ p, size_t n, float cnt, float* __restrict__ mean_out, float* __restrict__ sd_out,
                                               float (*buf)[256]) {
    const int lane = threadIdx.x;
    const size_t nblk = (n + 255) / 256;
    float mean = 0.f;
    for (int pass = 0; pass < 2; ++pass) {
        // out-of-range slots add exactly nothing: 0 in the sum pass, (mean - mean)^2 = 0 in the squares pass
        const float pad = pass ? mean : 0.f;
        float r[4];
        auto fetch = [&](size_t b) {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const size_t i = b * 256 + (size_t)j * 64 + lane;
                r[j] = i < n ? p[i] : pad;
            }
        };
        auto stash = [&](int which) {
#pragma unroll
            for (int j = 0; j < 4; ++j) buf[which][j * 64 + lane] = pass ? (r[j] - mean) * (r[j] - mean) : r[j];
        };
        fetch(0);
        stash(0);
        __syncthreads();
        float acc = 0.f;
        for (size_t b = 0; b < nblk; ++b) {
            if (b + 1 < nblk) fetch(b + 1);
            // the add chain is the critical path (one dependent v_add_f32 per sample): LDS reads run one 16-sample
            // group ahead of it, in registers
            const f4* q = reinterpret_cast<const f4*>(buf[b & 1]);
            f4 cur[4], nxt[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) cur[j] = q[j];
#pragma unroll
            for (int g = 0; g < 16; ++g) {
                if (g + 1 < 16) {
#pragma unroll
                    for (int j = 0; j < 4; ++j) nxt[j] = q[4 * (g + 1) + j];
                }
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    acc += cur[j].x;
                    acc += cur[j].y;
                    acc += cur[j].z;
                    acc += cur[j].w;
                }
#pragma unroll
                for (int j = 0; j < 4; ++j) cur[j] = nxt[j];
            }
            if (b + 1 < nblk) stash((int)((b + 1) & 1));
            __syncthreads();
        }
        if (pass == 0)
            mean = acc / cnt;
        else if (lane == 0) {
            *mean_out = mean;
            *sd_out = sqrtf(acc / cnt);
        }
    }
}
__global__ __launch_bounds__(64) void k_tr_stats(const float* __restrict__ lab_s, size_t ns, float cnt_s, const float* __restrict__ lab_t,
                                                 size_t nt, float cnt_t, float* __restrict__ stats) {
    __shared__ __attribute__((aligned(16))) float buf[2][256];
    const int chain = blockIdx.x, c = chain % 3;
    const bool is_t = chain >= 3;
    const size_t n = is_t ? nt : ns;
    tr_stats_chain((is_t ? lab_t : lab_s) + (size_t)c * n, n, is_t ? cnt_t : cnt_s, stats + (is_t ? 6 : 0) + c, stats + (is_t ? 9 : 3) + c, buf);
}
__global__ __launch_bounds__(256) void k_tr_apply(const float* __restrict__ lab, size_t n, const float* __restrict__ stats, TrK k,
                                                  uint8_t* __restrict__ out) {
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    float st[12];
#pragma unroll
    for (int i = 0; i < 12; ++i) st[i] = stats[i];
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        float v[3], R, G, B;
#pragma unroll
        for (int c = 0; c < 3; ++c) v[c] = (lab[i + (size_t)c * n] - st[c]) * st[9 + c] / st[3 + c] + st[6 + c];  // transfer.cpp:168-170
        tr_lab_to_rgb(k, v[0], v[1], v[2], R, G, B);
        out[i] = px_store<uint8_t>(R);  // the CImg<float> -> CImg<unsigned char> assignment of transfer.cpp:12
        out[i + n] = px_store<uint8_t>(G);
        out[i + 2 * n] = px_store<uint8_t>(B);
    }
}
