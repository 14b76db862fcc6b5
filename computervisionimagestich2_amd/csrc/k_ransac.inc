// Part of stitch_kernels.hpp (included there, inside namespace sk): ImageProcess::RANSAC (ImageProcess.cpp:395-529) on lists of
// matched keypoints, bit for bit.
//
// What is reproduced, and why each piece is exact:
//   * rand() after srand(seed): glibc's TYPE_3 additive-feedback generator (random_r.c), restated in 32-bit integer arithmetic --
//     31 words seeded by the 16807 Lehmer step (Schrage form), 310 discarded outputs, o = r[i-31] + r[i-3], result o >> 1.
//   * the index walk of :409-418: `rand() % n`, redrawn while the index repeats within the round; sequential per list.
//   * getHomographyMat (:439-462): CImg's _LU + _solve (CImg.h:25911-25953, 25401-25420) on the 4 sampled rows in draw order, in
//     double, same operation order, `>=` pivot choice, 1e-20 pivot substitution, the `ii` skip of leading zeros.
//   * getInlinerIndex (:473-497): the map in double from float coordinates, left to right, rounded to float; float differences,
//     squares and sum.  The reference then tests sqrtf(s) < threshold.  IEEE sqrt is correctly rounded and therefore monotone, so
//     {s >= 0 : sqrtf(s) < t} is a prefix [0, s*) of the floats: the host finds s* -- the smallest float whose sqrtf is >= t --
//     by bisection over the bit patterns with the same correctly rounded sqrtf, and the kernels test s < s*.  NaN fails both forms.
//   * getInlinerHomography (:500-529): LU again for exactly 4 rows, otherwise CImg's SVD (CImg.h:25755-25895), the decreasing sort
//     of the singular values with its column permutation, the pseudo-inverse's tolerance and V * U^T * b.  Every sum over rows is
//     added serially in row order (the terms are formed in parallel: a product rounds the same whoever forms it, and the build
//     contracts nothing into FMAs); everything that is independent per row runs one row per lane.
//
// Launches per batch of up to RANSAC_MAXLISTS lists (blockIdx.y or .x = list):
//   k_ransac_prepare  resolves (pairs, count, mirror) into four dense coordinate arrays, clears the per-round counts
//   k_ransac_sample   one lane per list: generator + index walk -> rounds x 4 indices, draws consumed, status
//   k_ransac_hyp      one lane per (list, round): 4 x 4 LU and two solves -> 8 doubles
//   k_ransac_count    one lane per round, its map in VGPRs; the points of a slab are wave-uniform (scalar loads); point slabs
//                     across workgroups, integer partial counts merged by integer atomics (exact, order-free)
//   k_ransac_select   lowest round among the maximal counts; the winner's inliers in index order (ballot prefix); info
//   k_ransac_fit      one workgroup per list: LU or SVD + pseudo-inverse solve -> p
constexpr int RANSAC_MAXLISTS = 16;  // lists per launch sequence
constexpr int RANSAC_PREP_T = 256;
constexpr int RANSAC_ROUND_T = 64;   // rounds per workgroup of k_ransac_hyp / k_ransac_count
constexpr int RANSAC_SELECT_T = 256;
constexpr int RANSAC_FIT_T = 256;
constexpr int RANSAC_FIT_TILE = 512;  // terms of a serial sum staged in LDS at a time
constexpr int RANSAC_FIT_SUMS = 8;    // serial sums running side by side at most (4 parameters x 2 right-hand sides)

// per-list status, info[0] (include/stitch.h: STITCH_RANSAC_*)
constexpr int RANSAC_OK = 0, RANSAC_TOO_FEW = 1, RANSAC_NO_CONSENSUS = 2, RANSAC_DRAW_CAP = 3;

struct RansacList {
    const float *src_x, *src_y, *dst_x, *dst_y;
    const int32_t* pairs;  // may be null: row i with row i
    const int32_t* count;  // may be null: n_max pairs
    double* p;             // out: 8
    int32_t* inliers;      // out: n_max (never null here: the host substitutes scratch)
    int32_t* info;         // out: 5
    // scratch
    double* hyp;    // rounds x 8
    double* U;      // 4 columns of n_max rows
    float* pts;     // 4 arrays of n_max: ImgPair.src x, y, ImgPair.dst x, y
    int32_t* idx;   // rounds x 4
    int32_t* cnt;   // rounds
    int32_t* hdr;   // n, status, draws, winning round, winning count
    int n_max, mirror;
};
struct RansacArgs {
    RansacList l[RANSAC_MAXLISTS];
    int rounds, nslabs, slab, draw_cap;
    uint32_t seed;
    float s_star;  // smallest float whose sqrtf is >= threshold (0 when nothing can pass)
};

__device__ __forceinline__ int ransac_n(const RansacList& L) {
    return L.count ? max(0, min(*L.count, L.n_max)) : L.n_max;
}

__global__ void __launch_bounds__(RANSAC_PREP_T) k_ransac_prepare(RansacArgs A) {
    const RansacList& L = A.l[blockIdx.y];
    const int n = ransac_n(L);
    const int t = blockIdx.x * RANSAC_PREP_T + threadIdx.x, stride = gridDim.x * RANSAC_PREP_T;
    for (int r = t; r < A.rounds; r += stride) L.cnt[r] = 0;
    if (t == 0) L.hdr[0] = n;
    for (int i = t; i < n; i += stride) {
        const int a = L.pairs ? L.pairs[2 * i] : i, b = L.pairs ? L.pairs[2 * i + 1] : i;
        const float ax = L.src_x[a], ay = L.src_y[a], bx = L.dst_x[b], by = L.dst_y[b];
        const size_t m = (size_t)L.n_max;
        L.pts[i] = L.mirror ? bx : ax;
        L.pts[m + i] = L.mirror ? by : ay;
        L.pts[2 * m + i] = L.mirror ? ax : bx;
        L.pts[3 * m + i] = L.mirror ? ay : by;
    }
}

// glibc random_r.c, TYPE_3 (x**31 + x**3 + 1); on the device the state is in LDS and one lane walks it.  The same code serves
// the host hook stitch_ransac_rand.
struct RansacRand {
    int32_t* r;  // 31 words
    int f, b;    // front / rear positions
    __host__ __device__ void seed(uint32_t s) {
        int32_t word = s ? (int32_t)s : 1;
        r[0] = word;
        for (int i = 1; i < 31; ++i) {  // word = 16807 * word % 2147483647 without overflow
            const int32_t hi = word / 127773, lo = word % 127773;
            word = 16807 * lo - 2836 * hi;
            if (word < 0) word += 2147483647;
            r[i] = word;
        }
        f = 3;
        b = 0;
        for (int i = 0; i < 310; ++i) (void)next();
    }
    __host__ __device__ int32_t next() {
        const uint32_t v = (uint32_t)r[f] + (uint32_t)r[b];
        r[f] = (int32_t)v;
        f = f == 30 ? 0 : f + 1;
        b = b == 30 ? 0 : b + 1;
        return (int32_t)(v >> 1);
    }
};

__global__ void __launch_bounds__(WAVE) k_ransac_sample(RansacArgs A) {
    const RansacList& L = A.l[blockIdx.x];
    __shared__ int32_t state[31];
    if (threadIdx.x != 0) return;
    const int n = ransac_n(L);
    int status = RANSAC_OK, draws = 0;
    if (n < 4) {
        status = RANSAC_TOO_FEW;  // the reference's redraw loop never finds a fourth distinct index
    } else {
        RansacRand g{state, 0, 0};
        g.seed(A.seed);
        for (int r = 0; r < A.rounds && status == RANSAC_OK; ++r) {
            int c0 = -1, c1 = -1, c2 = -1;
            for (int i = 0; i < 4; ++i) {
                int index = 0;
                do {
                    if (draws >= A.draw_cap) {
                        status = RANSAC_DRAW_CAP;
                        break;
                    }
                    index = (int)((uint32_t)g.next() % (uint32_t)n);
                    ++draws;
                } while (index == c0 || index == c1 || index == c2);
                if (status != RANSAC_OK) break;
                L.idx[4 * r + i] = index;
                if (i == 0) c0 = index;
                if (i == 1) c1 = index;
                if (i == 2) c2 = index;
            }
        }
    }
    L.hdr[1] = status;
    L.hdr[2] = draws;
}

// CImg::_LU + _solve on a 4 x 4 system (lu[row][col]) for two right-hand sides, CImg.h:25911-25953, 25401-25420.  Everything is
// unrolled with the dynamic row choices turned into selects, so the matrix stays in registers.  A row of the design matrix ends in
// 1, so the "row of zeros" exit of _LU (:25923) cannot be taken.
__device__ __forceinline__ void ransac_lu_solve4(double (&lu)[4][4], double (&x1)[4], double (&x2)[4]) {
    double vv[4];
    int indx[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        double vmax = 0.0;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const double t = fabs(lu[i][j]);
            if (t > vmax) vmax = t;
        }
        vv[i] = 1 / vmax;
    }
    int imax = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
#pragma unroll
        for (int i = 0; i < j; ++i) {
            double s = lu[i][j];
#pragma unroll
            for (int k = 0; k < i; ++k) s -= lu[i][k] * lu[k][j];
            lu[i][j] = s;
        }
        double vmax = 0.0;
#pragma unroll
        for (int i = j; i < 4; ++i) {
            double s = lu[i][j];
#pragma unroll
            for (int k = 0; k < j; ++k) s -= lu[i][k] * lu[k][j];
            lu[i][j] = s;
            const double t = vv[i] * fabs(s);
            if (t >= vmax) {
                vmax = t;
                imax = i;
            }
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            if (r != j && r == imax) {
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const double t = lu[r][k];
                    lu[r][k] = lu[j][k];
                    lu[j][k] = t;
                }
                vv[r] = vv[j];
            }
        }
        indx[j] = imax;
        if (lu[j][j] == 0) lu[j][j] = 1e-20;
        const double t = 1 / lu[j][j];
#pragma unroll
        for (int i = j + 1; i < 4; ++i) lu[i][j] = lu[i][j] * t;
    }
#pragma unroll
    for (int rhs = 0; rhs < 2; ++rhs) {
        double(&x)[4] = rhs ? x2 : x1;
        int ii = -1;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int ip = indx[i];
            double s = x[0];
#pragma unroll
            for (int r = 1; r < 4; ++r) s = ip == r ? x[r] : s;
            const double xi = x[i];
#pragma unroll
            for (int r = 0; r < 4; ++r) x[r] = ip == r ? xi : x[r];
            if (ii >= 0) {
#pragma unroll
                for (int j = 0; j < i; ++j)
                    if (j >= ii) s -= lu[i][j] * x[j];
            } else if (s != 0) {
                ii = i;
            }
            x[i] = s;
        }
#pragma unroll
        for (int i = 3; i >= 0; --i) {
            double s = x[i];
#pragma unroll
            for (int j = i + 1; j < 4; ++j) s -= lu[i][j] * x[j];
            x[i] = s / lu[i][i];
        }
    }
}

// rows k = 0..3 of the system from points i[k]: A = (x, y, x*y, 1) in double, b = dst x / dst y
__device__ __forceinline__ void ransac_fit4(const RansacList& L, const int (&i)[4], double (&p)[8]) {
    const size_t m = (size_t)L.n_max;
    double lu[4][4], x1[4], x2[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const double x = (double)L.pts[i[k]], y = (double)L.pts[m + i[k]];
        lu[k][0] = x;
        lu[k][1] = y;
        lu[k][2] = x * y;
        lu[k][3] = 1.0;
        x1[k] = (double)L.pts[2 * m + i[k]];
        x2[k] = (double)L.pts[3 * m + i[k]];
    }
    ransac_lu_solve4(lu, x1, x2);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        p[k] = x1[k];
        p[4 + k] = x2[k];
    }
}

__global__ void __launch_bounds__(RANSAC_ROUND_T) k_ransac_hyp(RansacArgs A) {
    const RansacList& L = A.l[blockIdx.y];
    if (L.hdr[1] != RANSAC_OK) return;
    const int r = blockIdx.x * RANSAC_ROUND_T + threadIdx.x;
    if (r >= A.rounds) return;
    const int i[4] = {L.idx[4 * r], L.idx[4 * r + 1], L.idx[4 * r + 2], L.idx[4 * r + 3]};
    double p[8];
    ransac_fit4(L, i, p);
#pragma unroll
    for (int k = 0; k < 8; ++k) L.hyp[8 * (size_t)r + k] = p[k];
}

// getInlinerIndex's test for one point (ImageProcess.cpp:466, :470, :482-491); s_star replaces sqrtf(s) < threshold (see the top)
__device__ __forceinline__ bool ransac_inlier(const double (&p)[8], float sx, float sy, float dx, float dy, float s_star) {
    const double x = (double)sx, y = (double)sy;
    const float X = (float)(p[0] * x + p[1] * y + p[2] * x * y + p[3]);
    const float Y = (float)(p[4] * x + p[5] * y + p[6] * x * y + p[7]);
    const float ex = X - dx, ey = Y - dy;
    const float s = ex * ex + ey * ey;
    return s < s_star;
}

__global__ void __launch_bounds__(RANSAC_ROUND_T) k_ransac_count(RansacArgs A) {
    const RansacList& L = A.l[blockIdx.z];
    if (L.hdr[1] != RANSAC_OK) return;
    const int n = L.hdr[0];
    const int j0 = min((int)blockIdx.y * A.slab, n), j1 = min(j0 + A.slab, n);
    if (j0 >= j1) return;
    const int r = blockIdx.x * RANSAC_ROUND_T + threadIdx.x;
    const int rr = min(r, A.rounds - 1);
    double p[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) p[k] = L.hyp[8 * (size_t)rr + k];
    const size_t m = (size_t)L.n_max;
    const float *px = L.pts, *py = L.pts + m, *qx = L.pts + 2 * m, *qy = L.pts + 3 * m;
    int c = 0;
    for (int j = j0; j < j1; ++j)  // wave-uniform addresses
        c += ransac_inlier(p, px[j], py[j], qx[j], qy[j], A.s_star) ? 1 : 0;
    if (r < A.rounds && c) atomicAdd(&L.cnt[r], c);
}

__global__ void __launch_bounds__(RANSAC_SELECT_T) k_ransac_select(RansacArgs A) {
    const RansacList& L = A.l[blockIdx.x];
    __shared__ unsigned long long best[RANSAC_SELECT_T];
    __shared__ int wave_n[RANSAC_SELECT_T / WAVE];
    const int tid = threadIdx.x, lane = tid % WAVE, wave = tid / WAVE;
    const int n = L.hdr[0];
    int status = L.hdr[1];
    int win = -1, wcount = 0;
    if (status == RANSAC_OK) {
        // largest count, lowest round: a later round replaces the best only on a strictly larger count (:427)
        unsigned long long key = 0;
        for (int r = tid; r < A.rounds; r += RANSAC_SELECT_T)
            key = max(key, ((unsigned long long)(unsigned)L.cnt[r] << 32) | (unsigned)(0x7fffffff - r));
        best[tid] = key;
        __syncthreads();
        for (int s = RANSAC_SELECT_T / 2; s > 0; s >>= 1) {
            if (tid < s) best[tid] = max(best[tid], best[tid + s]);
            __syncthreads();
        }
        key = best[0];
        wcount = (int)(key >> 32);
        win = 0x7fffffff - (int)(unsigned)(key & 0xffffffffu);
        if (wcount == 0) {
            status = RANSAC_NO_CONSENSUS;  // the reference solves an empty system here and terminates
            win = -1;
        }
    }
    int base = 0;
    if (status == RANSAC_OK) {
        double p[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) p[k] = L.hyp[8 * (size_t)win + k];
        const size_t m = (size_t)L.n_max;
        for (int c0 = 0; c0 < n; c0 += RANSAC_SELECT_T) {
            const int i = c0 + tid;
            const bool in = i < n && ransac_inlier(p, L.pts[i], L.pts[m + i], L.pts[2 * m + i], L.pts[3 * m + i], A.s_star);
            const unsigned long long mask = __ballot(in);
            if (lane == 0) wave_n[wave] = __popcll(mask);
            __syncthreads();
            int pos = base + __popcll(mask & ((1ull << lane) - 1)), total = 0;
            for (int w = 0; w < RANSAC_SELECT_T / WAVE; ++w) {
                const int c = wave_n[w];
                pos += w < wave ? c : 0;
                total += c;
            }
            if (in) L.inliers[pos] = i;
            base += total;
            __syncthreads();
        }
    }
    for (int i = base + tid; i < L.n_max; i += RANSAC_SELECT_T) L.inliers[i] = -1;
    if (status != RANSAC_OK && tid < 8) L.p[tid] = __builtin_nan("");
    if (tid == 0) {
        L.hdr[1] = status;
        L.hdr[3] = win;
        L.hdr[4] = base;
        L.info[0] = status;
        L.info[1] = n;
        L.info[2] = win;
        L.info[3] = base;  // == the round's count: the same arithmetic decided both
        L.info[4] = L.hdr[2];
    }
}

// std::max: the first argument unless it is smaller (NaN in either place keeps the first)
template <typename T>
__device__ __forceinline__ T ransac_max(T a, T b) {
    return a < b ? b : a;
}

// cimg::_hypot, CImg.h:5845-5850
__device__ __forceinline__ double ransac_hypot(double x, double y) {
    double nx = fabs(x), ny = fabs(y), t;
    if (nx < ny) {
        t = nx;
        nx = ny;
    } else {
        t = ny;
    }
    if (nx > 0) {
        t /= nx;
        return nx * sqrt(1 + t * t);
    }
    return 0.0;
}

// NS sums over k = k0 .. k1-1, each added serially in index order starting from +0 by one lane; term(k, v) forms the NS terms of
// row k (any lane).  Called by the whole workgroup; every thread gets every sum.
template <int NS, typename F>
__device__ __forceinline__ void ransac_serial_sums(int k0, int k1, double* tile, double* res, F term, double (&out)[NS]) {
    const int tid = threadIdx.x;
    double acc = 0.0;
    for (int c0 = k0; c0 < k1; c0 += RANSAC_FIT_TILE) {
        const int m = min(RANSAC_FIT_TILE, k1 - c0);
        for (int t = tid; t < m; t += RANSAC_FIT_T) {
            double v[NS];
            term(c0 + t, v);
#pragma unroll
            for (int s = 0; s < NS; ++s) tile[s * RANSAC_FIT_TILE + t] = v[s];
        }
        __syncthreads();
        if (tid < NS)
            for (int t = 0; t < m; ++t) acc += tile[tid * RANSAC_FIT_TILE + t];
        __syncthreads();
    }
    if (tid < NS) res[tid] = acc;
    __syncthreads();
#pragma unroll
    for (int s = 0; s < NS; ++s) out[s] = res[s];
    __syncthreads();
}

// getInlinerHomography (ImageProcess.cpp:500-529).  Scalars of the SVD (S, rv1, V, the rotation coefficients) are held by every
// thread and computed by every thread from the same broadcast sums, so all branches are uniform over the workgroup.  U lives in
// global scratch, column-major.  In a per-row step that starts at row `first` (i, l or 0, depending on the phase) thread t works on
// rows first + t, first + t + RANSAC_FIT_T, ...: a row's owner is (row - first) mod RANSAC_FIT_T and changes from phase to phase.
// What makes that safe is a __syncthreads between the last write under one owner and the first access under the next; within the
// diagonalisation every loop starts at row 0, so there a row keeps one owner throughout.
__global__ void __launch_bounds__(RANSAC_FIT_T) k_ransac_fit(RansacArgs A) {
    const RansacList& L = A.l[blockIdx.x];
    if (L.hdr[1] != RANSAC_OK) return;
    const int H = L.hdr[4], W = 4, tid = threadIdx.x, T = RANSAC_FIT_T;
    const size_t m = (size_t)L.n_max;
    const int32_t* inl = L.inliers;
    if (H == 4) {  // square system: the LU path of CImg::solve
        if (tid == 0) {
            const int i[4] = {inl[0], inl[1], inl[2], inl[3]};
            double p[8];
            ransac_fit4(L, i, p);
#pragma unroll
            for (int k = 0; k < 8; ++k) L.p[k] = p[k];
        }
        return;
    }
    __shared__ double tile[RANSAC_FIT_SUMS * RANSAC_FIT_TILE];
    __shared__ double res[RANSAC_FIT_SUMS];
    double* Ug = L.U;
    const size_t ld = m;
#define UU(k, c) Ug[(size_t)(c) * ld + (size_t)(k)]
    for (int k = tid; k < H; k += T) {
        const double x = (double)L.pts[inl[k]], y = (double)L.pts[m + inl[k]];
        UU(k, 0) = x;
        UU(k, 1) = y;
        UU(k, 2) = x * y;
        UU(k, 3) = 1.0;
    }
    __syncthreads();

    // ---- CImg::SVD (CImg.h:25755-25895), sorting = true, max_iteration = 40 ----
    double S[4] = {0, 0, 0, 0}, rv1[4] = {0, 0, 0, 0}, V[4][4];  // V[row][col]
    for (int a = 0; a < 4; ++a)
        for (int b = 0; b < 4; ++b) V[a][b] = 0.0;
    double anorm = 0, c = 0, f = 0, g = 0, h = 0, s = 0, scale = 0;
    int l = 0, nm = 0;
    for (int i = 0; i < W; ++i) {  // Householder reduction to bidiagonal form
        l = i + 1;
        rv1[i] = scale * g;
        g = s = scale = 0;
        if (i < H) {
            double o1[1];
            ransac_serial_sums<1>(i, H, tile, res, [&](int k, double(&v)[1]) { v[0] = fabs(UU(k, i)); }, o1);
            scale = o1[0];
            if (scale) {
                for (int k = i + tid; k < H; k += T) UU(k, i) /= scale;
                __syncthreads();
                ransac_serial_sums<1>(i, H, tile, res, [&](int k, double(&v)[1]) { v[0] = UU(k, i) * UU(k, i); }, o1);
                s = o1[0];
                f = UU(i, i);
                g = (f >= 0 ? -1 : 1) * sqrt(s);
                h = f * g - s;
                __syncthreads();  // every thread has read U(i,i)
                if (tid == 0) UU(i, i) = f - g;
                __syncthreads();
                double o3[3];
                ransac_serial_sums<3>(i, H, tile, res, [&](int k, double(&v)[3]) {
                    const double u = UU(k, i);
#pragma unroll
                    for (int q = 0; q < 3; ++q) v[q] = l + q < W ? u * UU(k, l + q) : 0.0;
                }, o3);
                for (int q = 0; q < 3; ++q) {
                    const int j = l + q;
                    if (j >= W) break;
                    f = o3[q] / h;
                    for (int k = i + tid; k < H; k += T) UU(k, j) += f * UU(k, i);
                }
                for (int k = i + tid; k < H; k += T) UU(k, i) *= scale;  // rows owned by this thread: ordered after its own reads
                __syncthreads();
            }
        }
        S[i] = scale * g;
        g = s = scale = 0;
        if (i < H && i != W - 1) {
            double row[4] = {0, 0, 0, 0};  // row i, columns l..: every thread computes it, thread 0 stores it
            for (int k = l; k < W; ++k) row[k] = UU(i, k);
            for (int k = l; k < W; ++k) scale += fabs(row[k]);
            __syncthreads();  // row i read by everyone before anyone stores into it
            if (scale) {
                for (int k = l; k < W; ++k) {
                    row[k] /= scale;
                    s += row[k] * row[k];
                }
                f = row[l];
                g = (f >= 0 ? -1 : 1) * sqrt(s);
                h = f * g - s;
                row[l] = f - g;
                for (int k = l; k < W; ++k) rv1[k] = row[k] / h;
                for (int j = l + tid; j < H; j += T) {
                    double sj = 0;
                    for (int k = l; k < W; ++k) sj += UU(j, k) * row[k];
                    for (int k = l; k < W; ++k) UU(j, k) += sj * rv1[k];
                }
                if (tid == 0)
                    for (int k = l; k < W; ++k) UU(i, k) = row[k] * scale;
                __syncthreads();
            }
        }
        anorm = (double)ransac_max((float)anorm, (float)(fabs(S[i]) + fabs(rv1[i])));
    }
    for (int i = W - 1; i >= 0; --i) {  // accumulation of the right-hand transformations (row i of U only: no stores)
        if (i < W - 1) {
            if (g) {
                for (int j = l; j < W; ++j) V[j][i] = (UU(i, j) / UU(i, l)) / g;
                for (int j = l; j < W; ++j) {
                    s = 0;
                    for (int k = l; k < W; ++k) s += UU(i, k) * V[k][j];
                    for (int k = l; k < W; ++k) V[k][j] += s * V[k][i];
                }
            }
            for (int j = l; j < W; ++j) V[i][j] = V[j][i] = 0.0;
        }
        V[i][i] = 1.0;
        g = rv1[i];
        l = i;
    }
    for (int i = min(W, H) - 1; i >= 0; --i) {  // accumulation of the left-hand transformations
        l = i + 1;
        g = S[i];
        __syncthreads();
        if (tid == 0)
            for (int j = l; j < W; ++j) UU(i, j) = 0.0;
        __syncthreads();
        if (g) {
            g = 1 / g;
            double o3[3];
            ransac_serial_sums<3>(l, H, tile, res, [&](int k, double(&v)[3]) {
                const double u = UU(k, i);
#pragma unroll
                for (int q = 0; q < 3; ++q) v[q] = l + q < W ? u * UU(k, l + q) : 0.0;
            }, o3);
            const double uii = UU(i, i);
            for (int q = 0; q < 3; ++q) {
                const int j = l + q;
                if (j >= W) break;
                f = (o3[q] / uii) * g;
                for (int k = i + tid; k < H; k += T) UU(k, j) += f * UU(k, i);
            }
            __syncthreads();  // U(i,i) read by everyone before its owner scales it
            for (int j = i + tid; j < H; j += T) UU(j, i) *= g;
        } else {
            for (int j = i + tid; j < H; j += T) UU(j, i) = 0.0;
        }
        __syncthreads();
        if (tid == 0) UU(i, i) += 1;
        __syncthreads();
    }
    // diagonalisation of the bidiagonal form: every U operation below is local to a row and every row loop starts at row 0, so a
    // row keeps the owner tid = row mod RANSAC_FIT_T from here to the end of the sweeps -> no barriers
    for (int k = W - 1; k >= 0; --k) {
        for (int its = 0; its < 40; ++its) {
            bool flag = true;
            for (l = k; l >= 1; --l) {
                nm = l - 1;
                if ((fabs(rv1[l]) + anorm) == anorm) {
                    flag = false;
                    break;
                }
                if ((fabs(S[nm]) + anorm) == anorm) break;
            }
            if (flag) {
                c = 0;
                s = 1;
                for (int i = l; i <= k; ++i) {
                    f = s * rv1[i];
                    rv1[i] = c * rv1[i];
                    if ((fabs(f) + anorm) == anorm) break;
                    g = S[i];
                    h = ransac_hypot(f, g);
                    S[i] = h;
                    h = 1 / h;
                    c = g * h;
                    s = -f * h;
                    for (int j = tid; j < H; j += T) {
                        const double y = UU(j, nm), z = UU(j, i);
                        UU(j, nm) = y * c + z * s;
                        UU(j, i) = z * c - y * s;
                    }
                }
            }
            const double z = S[k];
            if (l == k) {
                if (z < 0) {
                    S[k] = -z;
                    for (int j = 0; j < W; ++j) V[j][k] = -V[j][k];
                }
                break;
            }
            nm = k - 1;
            double x = S[l], y = S[nm];
            g = rv1[nm];
            h = rv1[k];
            f = ((y - z) * (y + z) + (g - h) * (g + h)) / ransac_max(1e-25, 2 * h * y);
            g = ransac_hypot(f, 1.0);
            f = ((x - z) * (x + z) + h * ((y / (f + (f >= 0 ? g : -g))) - h)) / ransac_max(1e-25, x);
            c = s = 1;
            for (int j = l; j <= nm; ++j) {
                const int i = j + 1;
                g = rv1[i];
                h = s * g;
                g = c * g;
                y = S[i];
                double zz = ransac_hypot(f, h);
                rv1[j] = zz;
                c = f / ransac_max(1e-25, zz);
                s = h / ransac_max(1e-25, zz);
                f = x * c + g * s;
                g = g * c - x * s;
                h = y * s;
                y *= c;
                for (int jj = 0; jj < W; ++jj) {
                    const double xx = V[jj][j], vz = V[jj][i];
                    V[jj][j] = xx * c + vz * s;
                    V[jj][i] = vz * c - xx * s;
                }
                zz = ransac_hypot(f, h);
                S[j] = zz;
                if (zz) {
                    zz = 1 / ransac_max(1e-25, zz);
                    c = f * zz;
                    s = h * zz;
                }
                f = c * g + s * y;
                x = c * y - s * g;
                for (int jj = tid; jj < H; jj += T) {
                    const double yy = UU(jj, j), uz = UU(jj, i);
                    UU(jj, j) = yy * c + uz * s;
                    UU(jj, i) = uz * c - yy * s;
                }
            }
            rv1[l] = 0;
            rv1[k] = f;
            S[k] = x;
        }
    }
    // S.sort(permutations, false) (CImg.h:25607-25612, _quicksort 25676-25731): decreasing, columns of U and V follow
    int perm[4] = {0, 1, 2, 3};
    {
        int stack[16], sp = 0;
        stack[sp++] = 0;
        stack[sp++] = W - 1;
        auto sw = [&](int a, int b) {
            const double t = S[a];
            S[a] = S[b];
            S[b] = t;
            const int u = perm[a];
            perm[a] = perm[b];
            perm[b] = u;
        };
        while (sp > 0) {
            const int hi = stack[--sp], lo = stack[--sp];
            if (lo >= hi) continue;
            const int mid = (lo + hi) / 2;
            if (S[lo] < S[mid]) sw(lo, mid);
            if (S[mid] < S[hi]) sw(hi, mid);
            if (S[lo] < S[mid]) sw(lo, mid);
            if (hi - lo >= 3) {
                const double piv = S[mid];
                int i = lo, j = hi;
                do {
                    while (S[i] > piv) ++i;
                    while (S[j] < piv) --j;
                    if (i <= j) {
                        sw(i, j);
                        ++i;
                        --j;
                    }
                } while (i <= j);
                if (lo < j && sp + 2 <= 16) {
                    stack[sp++] = lo;
                    stack[sp++] = j;
                }
                if (i < hi && sp + 2 <= 16) {
                    stack[sp++] = i;
                    stack[sp++] = hi;
                }
            }
        }
    }
    // get_pseudoinvert (CImg.h:25293-25302) and its product with b (operator*, 12244-12264)
    double smax = S[0];
    for (int x = 1; x < W; ++x)
        if (S[x] > smax) smax = S[x];
    const double tol = (double)(1.11e-16f * (float)max(W, H)) * smax;
    double Vs[4][4];  // sorted columns, scaled by the inverted singular values
    for (int x = 0; x < W; ++x) {
        const double sv = S[x], invs = sv > tol ? 1 / sv : 0.0;
        for (int y = 0; y < W; ++y) Vs[y][x] = V[y][perm[x]] * invs;
    }
    __syncthreads();  // the last rotations of U
    double o8[8];
    ransac_serial_sums<8>(0, H, tile, res, [&](int i, double(&v)[8]) {
        const double u0 = UU(i, perm[0]), u1 = UU(i, perm[1]), u2 = UU(i, perm[2]), u3 = UU(i, perm[3]);
        const double bx = (double)L.pts[2 * m + inl[i]], by = (double)L.pts[3 * m + inl[i]];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            double pv = 0.0;  // (V * U^T)(i, j): value = 0, then += V(k, j) * U(k, i) for k = 0..3
            pv += Vs[j][0] * u0;
            pv += Vs[j][1] * u1;
            pv += Vs[j][2] * u2;
            pv += Vs[j][3] * u3;
            v[j] = pv * bx;
            v[4 + j] = pv * by;
        }
    }, o8);
    (void)o8;
    if (tid < 8) L.p[tid] = res[tid];  // still holds the eight sums
#undef UU
}
