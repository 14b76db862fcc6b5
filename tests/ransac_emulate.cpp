// Host emulation of the kernels of csrc/k_ransac.inc for tests/test_ransac_host.py: the kernel source itself is compiled for the
// CPU (no FMA contraction) and run on one list, so that its arithmetic can be compared with the reference's recorded maps on a
// machine without a GPU.  k_ransac_prepare / _sample / _hyp / _count have no barriers: their threads run one after the other.
// k_ransac_fit runs as RANSAC_FIT_T host threads with a barrier for __syncthreads.  k_ransac_select is wave-level code (ballot
// prefix); its outcome -- lowest round among the largest counts, the winner's inliers in index order -- is restated here.
//   ransac_emulate <list file: int32 n, then 4 x n float32 (src x, src y, dst x, dst y)> [rounds]
//   -> status n round count draws p0 .. p7 (hex floats)
#include <pthread.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <thread>
#include <vector>
#define __device__
#define __host__
#define __global__
#define __forceinline__ inline
#define __shared__ static
#define __launch_bounds__(x)
struct Dim3 {
    unsigned x, y, z;
};
static thread_local Dim3 threadIdx{0, 0, 0};
static Dim3 blockIdx{0, 0, 0}, gridDim{1, 1, 1};
static pthread_barrier_t g_barrier;
static bool g_threads = false;
static void __syncthreads() {
    if (g_threads) pthread_barrier_wait(&g_barrier);
}
using std::max;
using std::min;
static unsigned long long __ballot(bool b) { return b ? 1 : 0; }  // (k_ransac_select is compiled, not run)
static int __popcll(unsigned long long v) { return __builtin_popcountll(v); }
static int atomicAdd(int* p, int v) {
    const int o = *p;
    *p += v;
    return o;
}
constexpr int WAVE = 64;
#include "k_ransac.inc"

static float s_star(float t) {  // stitch_ransac.inc: ransac_s_star
    if (!(t > 0)) return 0.0f;
    uint32_t lo = 0, hi = 0x7f800000u;
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo) / 2;
        float s;
        memcpy(&s, &mid, 4);
        if (std::sqrt(s) >= t)
            hi = mid;
        else
            lo = mid + 1;
    }
    float s;
    memcpy(&s, &lo, 4);
    return s;
}

template <typename K>
static void run_block(K kernel, const RansacArgs& A, unsigned threads) {
    for (unsigned t = 0; t < threads; ++t) {
        threadIdx = {t, 0, 0};
        kernel(A);
    }
    threadIdx = {0, 0, 0};
}

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 2;
    int n = 0;
    const int K = argc > 2 ? atoi(argv[2]) : 72;
    if (fread(&n, 4, 1, f) != 1 || n < 0) return 2;
    std::vector<float> xy(4 * (size_t)n + 4);
    if (fread(xy.data(), 4, 4 * (size_t)n, f) != 4 * (size_t)n) return 2;
    fclose(f);
    RansacArgs A;
    memset(&A, 0, sizeof A);
    RansacList& L = A.l[0];
    std::vector<double> hyp(8 * (size_t)K), U(4 * (size_t)n + 4);
    std::vector<float> pts(4 * (size_t)n + 4);
    std::vector<int32_t> idx(4 * (size_t)K), cnt(K), hdr(8), inl(n + 1), info(5);
    double p[8];
    L.src_x = xy.data();
    L.src_y = xy.data() + n;
    L.dst_x = xy.data() + 2 * (size_t)n;
    L.dst_y = xy.data() + 3 * (size_t)n;
    L.p = p;
    L.inliers = inl.data();
    L.info = info.data();
    L.hyp = hyp.data();
    L.U = U.data();
    L.pts = pts.data();
    L.idx = idx.data();
    L.cnt = cnt.data();
    L.hdr = hdr.data();
    L.n_max = n;
    A.rounds = K;
    A.nslabs = 3;  // uneven slabs on purpose
    A.slab = std::max(1, (n + 2) / 3);
    A.draw_cap = 32 * K + 4096;
    A.seed = 666666;
    A.s_star = s_star(4.0f);
    const unsigned kblocks = (unsigned)((K + RANSAC_ROUND_T - 1) / RANSAC_ROUND_T);
    gridDim = {(unsigned)((std::max(n, K) + RANSAC_PREP_T - 1) / RANSAC_PREP_T), 1, 1};
    for (unsigned b = 0; b < gridDim.x; ++b) {
        blockIdx = {b, 0, 0};
        run_block(k_ransac_prepare, A, RANSAC_PREP_T);
    }
    blockIdx = {0, 0, 0};
    run_block(k_ransac_sample, A, 1);
    for (unsigned b = 0; b < kblocks; ++b) {
        blockIdx = {b, 0, 0};
        run_block(k_ransac_hyp, A, RANSAC_ROUND_T);
    }
    for (unsigned b = 0; b < kblocks; ++b)
        for (unsigned s = 0; s < (unsigned)A.nslabs; ++s) {
            blockIdx = {b, s, 0};
            run_block(k_ransac_count, A, RANSAC_ROUND_T);
        }
    blockIdx = {0, 0, 0};
    int status = hdr[1], win = -1, M = 0;
    if (status == RANSAC_OK) {
        int best = 0;
        for (int r = 0; r < K; ++r)
            if (cnt[r] > best) {
                best = cnt[r];
                win = r;
            }
        if (best == 0) {
            status = RANSAC_NO_CONSENSUS;
        } else {
            double q[8];
            for (int k = 0; k < 8; ++k) q[k] = hyp[8 * (size_t)win + k];
            for (int i = 0; i < n; ++i)
                if (ransac_inlier(q, pts[i], pts[n + i], pts[2 * (size_t)n + i], pts[3 * (size_t)n + i], A.s_star)) inl[M++] = i;
            if (M != best) return 3;
        }
    }
    hdr[1] = status;
    hdr[3] = win;
    hdr[4] = M;
    for (int k = 0; k < 8; ++k) p[k] = NAN;
    pthread_barrier_init(&g_barrier, nullptr, RANSAC_FIT_T);
    g_threads = true;
    {
        std::vector<std::thread> th;
        for (unsigned t = 0; t < (unsigned)RANSAC_FIT_T; ++t)
            th.emplace_back([&A, t] {
                threadIdx = {t, 0, 0};
                k_ransac_fit(A);
            });
        for (auto& t : th) t.join();
    }
    printf("%d %d %d %d %d", status, hdr[0], win, M, hdr[2]);
    for (int k = 0; k < 8; ++k) printf(" %a", p[k]);
    printf("\n");
    return 0;
}
