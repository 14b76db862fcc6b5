// Part of stitch_kernels.hpp (included there, inside namespace sk): exact L1 two-nearest-neighbour search with the ratio test of
// ImageProcess::getImgPair (ImageProcess.cpp:273-351).
//
// The reference builds a one-tree vl_kdforest over A's descriptors (L1 norm, exact search) and queries it with every descriptor of
// B for two neighbours.  Each distance is VLFeat's plain C _vl_distance_l1_f (vl/mathop.c:307-318): acc = 0.0f, then for
// k = 0..127 in order acc += |q[k] - x[k]| (VL_MAX(d, -d) differs from |d| only in the sign of a zero, which cannot change a sum
// that starts at +0).  On descriptors in [0, 1) -- all that VLFeat's SIFT produces -- the forest's answer is the exact top two by
// that distance, so a brute-force search that keeps the same 128-add chain reproduces it bit for bit.  (Outside [0, 1) the
// forest's squared split-distance bound can prune true neighbours; this search stays exact.)
//
// Three launches per call, every set of a batch in each (blockIdx.z / blockIdx.x = set):
//   k_match_partial  one lane = one query (128 floats in VGPRs); the data rows are wave-uniform and come in through scalar loads.
//                    The data set is cut into slabs across workgroups (blockIdx.y); each writes its slab's top-2 per query.
//   k_match_merge    slabs in index order -> d0, d1, index of d0 (equal distances: the lower index wins), ratio test.
//   k_match_compact  accepted (data index, query index) pairs in query order, and their count.
constexpr int MATCH_DIM = 128;      // DESCRIPTOR_SUM, ImageProcess.h:20
constexpr int MATCH_QB = 256;       // queries per workgroup of k_match_partial / k_match_merge
constexpr int MATCH_UNROLL = 4;     // data rows per iteration: four independent add chains
constexpr int MATCH_KCHUNK = 16;    // dimensions per batch of scalar loads
constexpr int MATCH_MAXSETS = 16;   // (data, query) sets per launch
constexpr int MATCH_COMPACT_T = 1024;

struct MatchSet {
    const float* db;     // n_db x 128
    const float* query;  // n_query x 128
    int32_t* nn;         // per query: index of d0, -1 without data (may be null)
    float* dist2;        // per query: d0, d1 (may be null)
    int32_t* pairs;      // 2 per accepted query: data index, query index
    int32_t* count;      // number of accepted queries
    float* part_d;       // scratch: nslabs x n_query x {d0, d1}
    int32_t* part_i;     // scratch: nslabs x n_query
    int32_t* acc;        // scratch: per query, the data index if accepted, else -1
    int n_db, n_query, slab;
};
struct MatchArgs {
    MatchSet s[MATCH_MAXSETS];
    int nslabs;
    double ratio;
};

__device__ __forceinline__ void match_top2(float d, int j, float& b0, float& b1, int& i0) {
    if (d < b0) {  // strict: an equal distance later in index order never displaces the nearest
        b1 = b0;
        b0 = d;
        i0 = j;
    } else if (d < b1) {
        b1 = d;
    }
}

__global__ void __launch_bounds__(MATCH_QB) k_match_partial(MatchArgs A) {
    const MatchSet& S = A.s[blockIdx.z];
    const int nq = S.n_query;
    if ((int)blockIdx.x * MATCH_QB >= nq) return;
    const int q = blockIdx.x * MATCH_QB + threadIdx.x;
    const int j0 = min((int)blockIdx.y * S.slab, S.n_db), j1 = min(j0 + S.slab, S.n_db);

    float qv[MATCH_DIM];
    {
        const f4* src = reinterpret_cast<const f4*>(S.query + (size_t)min(q, nq - 1) * MATCH_DIM);
#pragma unroll
        for (int k = 0; k < MATCH_DIM / 4; ++k) {
            const f4 v = src[k];
            qv[4 * k] = v.x;
            qv[4 * k + 1] = v.y;
            qv[4 * k + 2] = v.z;
            qv[4 * k + 3] = v.w;
        }
    }
    float b0 = __builtin_inff(), b1 = __builtin_inff();
    int i0 = -1;
    int j = j0;
    for (; j + MATCH_UNROLL <= j1; j += MATCH_UNROLL) {
        const float* x = S.db + (size_t)j * MATCH_DIM;  // wave-uniform
        float a[MATCH_UNROLL];
#pragma unroll
        for (int u = 0; u < MATCH_UNROLL; ++u) a[u] = 0.0f;
        // 16 dimensions of the four rows at a time (64 SGPRs).  Left alone, the compiler hoists all 512 scalar loads of an
        // iteration to its top and spills SGPRs into VGPR lanes.  The empty asm makes each chunk's offset depend on the
        // previous chunk's sums, so its loads issue only after those adds.  (Scalar loads return out of order -- a wave waits
        // for all of its outstanding ones at once -- so nothing is lost: the other waves of the SIMD cover the latency.)
        int kc = 0;  // == k0; an SGPR the asm "changes"
#pragma unroll
        for (int k0 = 0; k0 < MATCH_DIM; k0 += MATCH_KCHUNK) {
            float xs[MATCH_UNROLL][MATCH_KCHUNK];
#pragma unroll
            for (int u = 0; u < MATCH_UNROLL; ++u)
#pragma unroll
                for (int k = 0; k < MATCH_KCHUNK; ++k) xs[u][k] = x[u * MATCH_DIM + kc + k];
#pragma unroll
            for (int k = 0; k < MATCH_KCHUNK; ++k) {
#pragma unroll
                for (int u = 0; u < MATCH_UNROLL; ++u) a[u] += fabsf(qv[k0 + k] - xs[u][k]);
            }
            kc += MATCH_KCHUNK;
            asm("" : "+s"(kc) : "v"(a[0]), "v"(a[1]), "v"(a[2]), "v"(a[3]));
        }
#pragma unroll
        for (int u = 0; u < MATCH_UNROLL; ++u) match_top2(a[u], j + u, b0, b1, i0);
    }
    for (; j < j1; ++j) {
        const float* x = S.db + (size_t)j * MATCH_DIM;
        float a = 0.0f;
        int kc = 0;
#pragma unroll
        for (int k0 = 0; k0 < MATCH_DIM; k0 += MATCH_KCHUNK) {
            float xs[MATCH_KCHUNK];
#pragma unroll
            for (int k = 0; k < MATCH_KCHUNK; ++k) xs[k] = x[kc + k];
#pragma unroll
            for (int k = 0; k < MATCH_KCHUNK; ++k) a += fabsf(qv[k0 + k] - xs[k]);
            kc += MATCH_KCHUNK;
            asm("" : "+s"(kc) : "v"(a));
        }
        match_top2(a, j, b0, b1, i0);
    }
    if (q < nq) {
        const size_t o = (size_t)blockIdx.y * nq + q;
        S.part_d[2 * o] = b0;
        S.part_d[2 * o + 1] = b1;
        S.part_i[o] = i0;
    }
}

__global__ void __launch_bounds__(MATCH_QB) k_match_merge(MatchArgs A) {
    const MatchSet& S = A.s[blockIdx.z];
    const int nq = S.n_query;
    const int q = blockIdx.x * MATCH_QB + threadIdx.x;
    if (q >= nq) return;
    float d0 = __builtin_inff(), d1 = __builtin_inff();
    int i0 = -1;
    for (int s = 0; s < A.nslabs; ++s) {  // slabs cover increasing index ranges: on a tie the earlier slab keeps the index
        const size_t o = (size_t)s * nq + q;
        const float e0 = S.part_d[2 * o], e1 = S.part_d[2 * o + 1];
        if (e0 < d0) {
            d1 = fminf(d0, e1);
            d0 = e0;
            i0 = S.part_i[o];
        } else {
            d1 = fminf(d1, e0);
        }
    }
    // ImageProcess.cpp:334-336: float ratio = d0 / d1 (double quotient rounded to float = the fp32 quotient); accepted if < ratio.
    // 0/0 (tied at zero) is NaN and d0 == d1 gives 1: both rejected.  Fewer than two data rows: d1 is NaN, rejected.
    const bool have1 = d1 < __builtin_inff();
    const bool ok = i0 >= 0 && have1 && (double)(d0 / d1) < A.ratio;
    if (S.nn) S.nn[q] = i0;
    if (S.dist2) {
        S.dist2[2 * q] = i0 >= 0 ? d0 : __builtin_nanf("");
        S.dist2[2 * q + 1] = have1 ? d1 : __builtin_nanf("");
    }
    S.acc[q] = ok ? i0 : -1;
}

__global__ void __launch_bounds__(MATCH_COMPACT_T) k_match_compact(MatchArgs A) {
    const MatchSet& S = A.s[blockIdx.x];
    const int nq = S.n_query;
    __shared__ int wave_n[MATCH_COMPACT_T / WAVE];
    const int lane = threadIdx.x % WAVE, wave = threadIdx.x / WAVE;
    int base = 0;
    for (int c0 = 0; c0 < nq; c0 += MATCH_COMPACT_T) {
        const int q = c0 + threadIdx.x;
        const int v = q < nq ? S.acc[q] : -1;
        const unsigned long long m = __ballot(v >= 0);
        if (lane == 0) wave_n[wave] = __popcll(m);
        __syncthreads();
        int pos = base + __popcll(m & ((1ull << lane) - 1)), total = 0;
        for (int w = 0; w < MATCH_COMPACT_T / WAVE; ++w) {
            const int n = wave_n[w];
            pos += w < wave ? n : 0;
            total += n;
        }
        if (v >= 0) {
            S.pairs[2 * pos] = v;
            S.pairs[2 * pos + 1] = q;
        }
        base += total;
        __syncthreads();  // wave_n is rewritten by the next chunk
    }
    if (threadIdx.x == 0) *S.count = base;
}
