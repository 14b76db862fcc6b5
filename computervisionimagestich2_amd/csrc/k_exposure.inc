// k_exposure.inc -- exact float running sums by scan (DESIGN.md 14): the statistics of the colour transfer, transfer.cpp:128-164,
// bit for bit what the serial walk of k_tr_stats (k_formats.inc) gives, without its one dependent add per sample.
//
// The state.  A running sum s that is a normal, non-zero float lies in a binade [2^e, 2^(e+1)); with u = 2^(e-23) it is
// S = |s| / u, an integer in [2^23, 2^24).  For an addend x let v = sign(s) * x / u (exact in double), q = floor(v), r = v - q.
// While the exact sum stays in the binade, fl(s + x) is S' = S + q + d with d = 1 for r > 1/2, d = (S + q) & 1 for r == 1/2 (ties
// to even), d = 0 otherwise: a step is S -> S + a[S & 1] with two integers that do not depend on S.  Such maps compose,
// c[p] = a[p] + b[(p + a[p]) & 1], associatively, so a run of samples reduces to two integers by a parallel scan that needs only
// the sign and e of s.  Validity travels with the offsets: per entry parity the minimum over the run of S_prev + q -- the FLOOR of
// the exact sum, not the rounded S': below 2^23 the spacing halves, and an exact sum of 2^23 - 0.3 rounds to 2^23 - 1/2 in float
// but to 2^23 by the integer rule -- and the maximum of S', both relative to the entry S.  A run is valid for S iff
// S + lo[p] >= 2^23 and S + hi[p] < 2^24.  Everything else -- a state that is zero, subnormal, infinite or NaN, an element that
// is not finite or too large, the first element that would leave the binade -- is ONE plain float add, after which sign and e
// are taken anew.
//
// The workgroup functions below (ex_tile_maps, ex_redo, ex_span_map, ex_walk_spans) are written once for the device and for
// tests/exposure_emulate.cpp: code inside EX_THREADS(t) is what thread t does between two barriers, code outside it is uniform
// over the workgroup.  On the device EX_THREADS runs its body once, for threadIdx.x; the emulation loops over all threads.
#ifndef EX_HOST
#define EX_THREADS(t) for (int t = (int)threadIdx.x, t##_once = 1; t##_once; t##_once = 0)
#define EX_PER_THREAD(type, name) type name[1]
#define EX_MINE(name, t) name[0]
#define EX_SYNC() __syncthreads()
#define EX_ATOMIC_MIN(p, v) atomicMin(p, v)
#define EX_DEV __device__ __forceinline__
#endif

constexpr int EX_T = 256;                         // threads of a workgroup
constexpr int EX_K = 8;                           // consecutive samples a thread composes serially
constexpr int EX_TILE = EX_T * EX_K;              // samples per scan
constexpr int EX_SPAN_TILES = 4;
constexpr int EX_SPAN = EX_TILE * EX_SPAN_TILES;  // samples per entry of the span table
constexpr int EX_MAX_RESTARTS = EX_TILE / 8;      // a tile that restarts more often finishes serially (DESIGN.md 14: why an eighth)
constexpr int EX_WALK_CHUNK = 256;                // span-table entries staged in LDS at a time
constexpr int32_t EX_S_MIN = 1 << 23, EX_S_END = 1 << 24;
constexpr int32_t EX_DEAD = 1 << 30;
constexpr uint32_t EX_NO_GUESS = 0xffffffffu;
enum { EX_DIAG_PLAIN = 0, EX_DIAG_SPANS_O1 = 1, EX_DIAG_SPANS_REDONE = 2, EX_DIAG_TILES_SERIAL = 3, EX_DIAG_N = 4 };

// Offsets are int32: a usable map has |c|, |lo|, |hi| <= 2^23, because S + lo >= 2^23 and S + hi < 2^24 cannot hold for any S
// of [2^23, 2^24) beyond that.  A map that leaves this range for an entry parity is marked unusable for it (c = 0,
// lo = -2^30, hi = 2^30: invalid for every S, and it stays so under composition), so no sum of two fields overflows whatever
// the span length.
struct ExMap {
    int32_t c[2], lo[2], hi[2];
};
struct ExSpanEntry {  // one span under its guess
    ExMap m;
    uint32_t key;  // sign and exponent field of the guessed entry state (float bits >> 23), EX_NO_GUESS: redo the span
    uint32_t pad;
};
struct ExShared {
    float x[EX_TILE];  // the tile's addends (squares of the deviations in the second pass)
    ExMap wave[EX_T / 64];
    ExSpanEntry spans[EX_WALK_CHUNK];
    double red[EX_T / 64];
    int32_t first, s_at;
};
struct ExArgs {  // up to six planes per launch, as k_tr_stats takes them
    const float* p[6];
    unsigned long long n[6];
    float cnt[6];
    float* mean[6];  // one float each; pass 2 reads what pass 1 wrote
    float* sd[6];
};

EX_DEV uint32_t ex_bits(float f) {
    uint32_t u;
    __builtin_memcpy(&u, &f, 4);
    return u;
}
EX_DEV float ex_float(uint32_t u) {
    float f;
    __builtin_memcpy(&f, &u, 4);
    return f;
}
EX_DEV bool ex_key_normal(uint32_t key) { return (key & 0xff) != 0 && (key & 0xff) != 0xff; }
// sign(s) / u as a double: +-2^(150 - exponent field)
EX_DEV double ex_scale(uint32_t key) {
    const unsigned long long b = ((unsigned long long)(key >> 8) << 63) | ((unsigned long long)(1023 + 150 - (int)(key & 0xff)) << 52);
    double d;
    __builtin_memcpy(&d, &b, 8);
    return d;
}
EX_DEV int32_t ex_pick(int32_t v0, int32_t v1, int p) { return p ? v1 : v0; }  // a select on values: no indexed register array
EX_DEV ExMap ex_identity() { return ExMap{{0, 0}, {0, 0}, {0, 0}}; }
EX_DEV void ex_kill(ExMap& m, int p) {
    m.c[p] = 0;
    m.lo[p] = -EX_DEAD;
    m.hi[p] = EX_DEAD;
}
// q and the two roundings of one element; false: not finite or out of every state's reach
EX_DEV bool ex_elem_q(float x, double scale, int32_t& q, int32_t& d0, int32_t& d1) {
    const double v = (double)x * scale;
    if (!(__builtin_fabs(v) < 8388608.0)) return false;
    const double qf = __builtin_floor(v), r = v - qf;
    q = (int32_t)qf;
    d0 = r > 0.5 ? 1 : r == 0.5 ? (q & 1) : 0;
    d1 = r > 0.5 ? 1 : r == 0.5 ? ((q + 1) & 1) : 0;
    return true;
}
EX_DEV ExMap ex_elem_map(float x, double scale) {
    ExMap m;
    int32_t q, d0, d1;
    if (!ex_elem_q(x, scale, q, d0, d1)) {
        ex_kill(m, 0);
        ex_kill(m, 1);
        return m;
    }
    m.c[0] = m.hi[0] = q + d0;
    m.c[1] = m.hi[1] = q + d1;
    m.lo[0] = m.lo[1] = q;
    return m;
}
// f first, then g
EX_DEV ExMap ex_compose(const ExMap& f, const ExMap& g) {
    ExMap h;
#pragma unroll
    for (int p = 0; p < 2; ++p) {
        const int32_t a = f.c[p];
        const int pp = (p + a) & 1;
        h.c[p] = a + ex_pick(g.c[0], g.c[1], pp);
        const int32_t lo = a + ex_pick(g.lo[0], g.lo[1], pp), hi = a + ex_pick(g.hi[0], g.hi[1], pp);
        h.lo[p] = f.lo[p] < lo ? f.lo[p] : lo;
        h.hi[p] = f.hi[p] > hi ? f.hi[p] : hi;
        if (h.lo[p] < -EX_S_MIN || h.hi[p] > EX_S_MIN) ex_kill(h, p);
    }
    return h;
}
EX_DEV bool ex_valid(const ExMap& m, int32_t S) {
    const int p = S & 1;
    return S + ex_pick(m.lo[0], m.lo[1], p) >= EX_S_MIN && S + ex_pick(m.hi[0], m.hi[1], p) < EX_S_END;
}
EX_DEV float ex_addend(float x, int pass, float mean) { return pass ? (x - mean) * (x - mean) : x; }

#ifndef EX_HOST
// Exclusive prefix of the workgroup's maps in thread order (in place) and their total: a wavefront scan, then LDS across the
// four wavefronts.
__device__ __forceinline__ ExMap ex_shfl_up(const ExMap& m, int d) {
    ExMap o;
#pragma unroll
    for (int p = 0; p < 2; ++p) {
        o.c[p] = __shfl_up(m.c[p], d);
        o.lo[p] = __shfl_up(m.lo[p], d);
        o.hi[p] = __shfl_up(m.hi[p], d);
    }
    return o;
}
__device__ __forceinline__ void ex_block_scan(ExShared& sh, ExMap* mine, ExMap& total) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    ExMap inc = mine[0];
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const ExMap o = ex_shfl_up(inc, d);
        if (lane >= d) inc = ex_compose(o, inc);
    }
    if (lane == 63) sh.wave[w] = inc;
    ExMap ex = ex_shfl_up(inc, 1);
    if (lane == 0) ex = ex_identity();
    __syncthreads();
    ExMap pre = ex_identity();
    total = ex_identity();
#pragma unroll
    for (int k = 0; k < EX_T / 64; ++k) {
        if (k < w) pre = ex_compose(pre, sh.wave[k]);
        total = ex_compose(total, sh.wave[k]);
    }
    mine[0] = ex_compose(pre, ex);
    __syncthreads();
}
#else
// the emulation's scan: the same prefixes, one thread after the other
static inline void ex_block_scan(ExShared&, ExMap* maps, ExMap& total) {
    ExMap run = ex_identity();
    for (int t = 0; t < EX_T; ++t) {
        const ExMap mine = maps[t];
        maps[t] = run;
        run = ex_compose(run, mine);
    }
    total = run;
}
#endif

// The tile's addends into LDS.  Slots past `len` hold 0 and are never composed.
EX_DEV void ex_load_tile(ExShared& sh, const float* p, size_t pos, int len, int pass, float mean) {
    EX_THREADS(t) {
#pragma unroll
        for (int j = 0; j < EX_K; ++j) {
            const int i = j * EX_T + t;
            sh.x[i] = i < len ? ex_addend(p[pos + i], pass, mean) : 0.f;
        }
    }
    EX_SYNC();
}
// Every thread's K consecutive samples of [off, len) composed under `key`; then the exclusive prefixes and the total.
EX_DEV void ex_tile_maps(ExShared& sh, int off, int len, uint32_t key, ExMap* maps, ExMap& total) {
    const double scale = ex_scale(key);
    EX_THREADS(t) {
        ExMap m = ex_identity();
#pragma unroll
        for (int j = 0; j < EX_K; ++j) {
            const int i = t * EX_K + j;
            if (i >= off && i < len) m = ex_compose(m, ex_elem_map(sh.x[i], scale));
        }
        EX_MINE(maps, t) = m;
    }
    ex_block_scan(sh, maps, total);
}

// Samples [b, e) of plane p added to acc in order, exactly as a float loop adds them.  Tile by tile: scan under the state's sign
// and binade, accept up to the last sample before the first violation, add the next one with a plain float add, continue
// behind it.
EX_DEV float ex_redo(ExShared& sh, const float* p, size_t b, size_t e, float acc, int pass, float mean, uint32_t* diag) {
    EX_PER_THREAD(ExMap, maps);
    for (size_t pos = b; pos < e; pos += EX_TILE) {
        const int len = (int)(e - pos < (size_t)EX_TILE ? e - pos : (size_t)EX_TILE);
        ex_load_tile(sh, p, pos, len, pass, mean);
        int off = 0, restarts = 0;
        while (off < len) {
            const uint32_t bits = ex_bits(acc), key = bits >> 23;
            if (bits == 0) {  // +0 + x = x, and +0 for either zero: go to the first sample that is not a zero
                EX_THREADS(t) {
                    if (t == 0) sh.first = len;
                }
                EX_SYNC();
                EX_THREADS(t) {
                    int i = t * EX_K < off ? off : t * EX_K;
                    const int end = (t + 1) * EX_K < len ? (t + 1) * EX_K : len;
                    while (i < end && sh.x[i] == 0.f) ++i;
                    if (i < end) EX_ATOMIC_MIN(&sh.first, i);
                }
                EX_SYNC();
                const int m = sh.first;
                EX_SYNC();
                if (m < len) {
                    acc = acc + sh.x[m];
                    ++diag[EX_DIAG_PLAIN];
                }
                off = m < len ? m + 1 : len;
                continue;
            }
            if (restarts >= EX_MAX_RESTARTS) {  // as k_tr_stats walks
                for (int i = off; i < len; ++i) acc = acc + sh.x[i];
                diag[EX_DIAG_PLAIN] += (uint32_t)(len - off);
                ++diag[EX_DIAG_TILES_SERIAL];
                break;
            }
            if (!ex_key_normal(key)) {  // subnormal, -0, infinite, NaN
                acc = acc + sh.x[off++];
                ++diag[EX_DIAG_PLAIN];
                ++restarts;
                continue;
            }
            const int32_t S = (int32_t)((bits & 0x7fffffu) | 0x800000u);
            ExMap total;
            ex_tile_maps(sh, off, len, key, maps, total);
            // the one thread whose entry state is valid and whose samples hold the first violation reports it; without a
            // violation the last thread reports the state behind the tile
            const double scale = ex_scale(key);
            EX_THREADS(t) {
                if (t == 0) sh.first = len;
            }
            EX_SYNC();
            EX_THREADS(t) {
                const ExMap& pre = EX_MINE(maps, t);
                if (ex_valid(pre, S)) {
                    int32_t St = S + ex_pick(pre.c[0], pre.c[1], S & 1);
                    int hit = -1;
                    for (int j = 0; j < EX_K && hit < 0; ++j) {
                        const int i = t * EX_K + j;
                        if (i < off || i >= len) continue;
                        int32_t q, d0, d1;
                        if (!ex_elem_q(sh.x[i], scale, q, d0, d1)) {
                            hit = i;
                            break;
                        }
                        const int32_t nx = St + q + ((St & 1) ? d1 : d0);
                        if (St + q < EX_S_MIN || nx >= EX_S_END)
                            hit = i;
                        else
                            St = nx;
                    }
                    if (hit >= 0) sh.first = hit;
                    if (hit >= 0 || t == EX_T - 1) sh.s_at = St;
                }
            }
            EX_SYNC();
            const int m = sh.first;
            acc = ex_float((key << 23) | ((uint32_t)sh.s_at & 0x7fffffu));
            EX_SYNC();
            if (m < len) {
                acc = acc + sh.x[m];
                ++diag[EX_DIAG_PLAIN];
                ++restarts;
            }
            off = m < len ? m + 1 : len;
        }
        EX_SYNC();  // the next tile overwrites sh.x
    }
    return acc;
}

// Samples [b, e) -- one span -- reduced under the guess `key` (a normal state's sign and exponent field).
EX_DEV ExMap ex_span_map(ExShared& sh, const float* p, size_t b, size_t e, int pass, float mean, uint32_t key) {
    EX_PER_THREAD(ExMap, maps);
    ExMap run = ex_identity();
    for (size_t pos = b; pos < e; pos += EX_TILE) {
        const int len = (int)(e - pos < (size_t)EX_TILE ? e - pos : (size_t)EX_TILE);
        ex_load_tile(sh, p, pos, len, pass, mean);
        ExMap total;
        ex_tile_maps(sh, 0, len, key, maps, total);
        run = ex_compose(run, total);
    }
    return run;
}

// One span of the walk with the true state: O(1) where the state's sign and binade are the span's guess and the bounds hold.
EX_DEV float ex_walk_span(ExShared& sh, const ExSpanEntry& en, const float* p, size_t b, size_t e, float acc, int pass, float mean, uint32_t* diag) {
    const uint32_t bits = ex_bits(acc), key = bits >> 23;
    const int32_t S = (int32_t)((bits & 0x7fffffu) | 0x800000u);
    if (en.key == key && ex_key_normal(key) && ex_valid(en.m, S)) {
        ++diag[EX_DIAG_SPANS_O1];
        return ex_float((key << 23) | ((uint32_t)(S + ex_pick(en.m.c[0], en.m.c[1], S & 1)) & 0x7fffffu));
    }
    ++diag[EX_DIAG_SPANS_REDONE];
    return ex_redo(sh, p, b, e, acc, pass, mean, diag);
}

#ifndef EX_HOST
__device__ __forceinline__ double ex_block_sum(ExShared& sh, double v) {
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) v += __shfl_down(v, d);
    if ((threadIdx.x & 63) == 0) sh.red[threadIdx.x >> 6] = v;
    __syncthreads();
    double s = 0.0;
#pragma unroll
    for (int k = 0; k < EX_T / 64; ++k) s += sh.red[k];
    __syncthreads();
    return s;
}

// The kernels' bodies, per plane or per image: the kernels below run them on the planes an ExArgs holds by value, the many-plane
// forms of k_rig_exposure.inc on the records of a device table.  `sums`, `table` and `diag_out` are the plane's own rows.

// Form 2, first launch of a pass: one span's sum in double.
__device__ __forceinline__ void ex_span_sum_plane(ExShared& sh, const float* __restrict__ p, size_t n, const float* mean_at, int pass, int span,
                                                  double* __restrict__ sums) {
    const size_t b = (size_t)span * EX_SPAN;
    if (b >= n) return;
    const size_t e = b + EX_SPAN < n ? b + EX_SPAN : n;
    const float mean = pass ? *mean_at : 0.f;
    double v = 0.0;
    for (size_t i = b + threadIdx.x; i < e; i += EX_T) v += (double)ex_addend(p[i], pass, mean);
    v = ex_block_sum(sh, v);
    if (threadIdx.x == 0) sums[span] = v;
}

// Form 2, second launch: the guess of the state at the span's entry (the double prefix of the spans before it, rounded to
// float), then the span reduced under that guess.
__device__ __forceinline__ void ex_span_map_plane(ExShared& sh, const float* __restrict__ p, size_t n, const float* mean_at, int pass, int span,
                                                  const double* __restrict__ sums, ExSpanEntry* __restrict__ table) {
    const size_t b = (size_t)span * EX_SPAN;
    if (b >= n) return;
    const size_t e = b + EX_SPAN < n ? b + EX_SPAN : n;
    double v = 0.0;
    for (int k = threadIdx.x; k < span; k += EX_T) v += sums[k];
    const uint32_t key = ex_bits((float)ex_block_sum(sh, v)) >> 23;
    ExSpanEntry en;
    en.pad = 0;
    if (ex_key_normal(key)) {
        en.key = key;
        en.m = ex_span_map(sh, p, b, e, pass, pass ? *mean_at : 0.f, key);
    } else {
        en.key = EX_NO_GUESS;
        en.m = ex_identity();
    }
    if (threadIdx.x == 0) table[span] = en;
}

// One workgroup goes over the plane in order with the true state.  table == nullptr: the single-workgroup form, both passes in
// this launch.  With a table: one pass, the spans in order.
__device__ __forceinline__ void ex_walk_plane(ExShared& sh, const float* __restrict__ p, size_t n, float cnt, float* mean_at, float* sd_at, int pass,
                                              const ExSpanEntry* __restrict__ table, uint32_t* __restrict__ diag_out) {
    uint32_t diag[EX_DIAG_N] = {0, 0, 0, 0};
    float mean = 0.f, acc = 0.f;
    if (!table) {
        acc = ex_redo(sh, p, 0, n, 0.f, 0, 0.f, diag);
        mean = acc / cnt;
        acc = ex_redo(sh, p, 0, n, 0.f, 1, mean, diag);
    } else {
        mean = pass ? *mean_at : 0.f;
        const size_t spans = (n + EX_SPAN - 1) / EX_SPAN;
        for (size_t s0 = 0; s0 < spans; s0 += EX_WALK_CHUNK) {
            const int m = (int)(spans - s0 < (size_t)EX_WALK_CHUNK ? spans - s0 : (size_t)EX_WALK_CHUNK);
            if ((int)threadIdx.x < m) sh.spans[threadIdx.x] = table[s0 + threadIdx.x];
            __syncthreads();
            for (int k = 0; k < m; ++k) {
                const size_t b = (s0 + k) * EX_SPAN;
                acc = ex_walk_span(sh, sh.spans[k], p, b, b + EX_SPAN < n ? b + EX_SPAN : n, acc, pass, mean, diag);
            }
            __syncthreads();
        }
    }
    if (threadIdx.x == 0) {
        if (table && pass == 0)
            *mean_at = acc / cnt;
        else {
            *mean_at = mean;
            *sd_at = sqrtf(acc / cnt);
        }
        if (diag_out)
            for (int k = 0; k < EX_DIAG_N; ++k) diag_out[k] += diag[k];
    }
}

// k_tr_apply with keep_black: where src is given, a source pixel that is (0,0,0) stays (0,0,0).  out may be src.  One image's
// pixels, strided over the x dimension of the grid.
__device__ __forceinline__ void ex_apply_image(const float* __restrict__ lab, size_t n, const float* __restrict__ stats, const TrK& k, const uint8_t* src,
                                               uint8_t* out) {
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    float st[12];
#pragma unroll
    for (int i = 0; i < 12; ++i) st[i] = stats[i];
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const bool black = src && (src[i] | src[i + n] | src[i + 2 * n]) == 0;
        float v[3], R, G, B;
#pragma unroll
        for (int c = 0; c < 3; ++c) v[c] = (lab[i + (size_t)c * n] - st[c]) * st[9 + c] / st[3 + c] + st[6 + c];  // transfer.cpp:168-170
        tr_lab_to_rgb(k, v[0], v[1], v[2], R, G, B);
        out[i] = black ? (uint8_t)0 : px_store<uint8_t>(R);
        out[i + n] = black ? (uint8_t)0 : px_store<uint8_t>(G);
        out[i + 2 * n] = black ? (uint8_t)0 : px_store<uint8_t>(B);
    }
}

// Form 0: the serial walk of k_tr_stats, one wavefront per plane.
__global__ __launch_bounds__(64) void k_ex_stats_serial(ExArgs a) {
    __shared__ __attribute__((aligned(16))) float buf[2][256];
    const int pl = blockIdx.x;
    tr_stats_chain(a.p[pl], (size_t)a.n[pl], a.cnt[pl], a.mean[pl], a.sd[pl], buf);
}

// sums[plane * max_spans + span], table[plane * max_spans + span], diag_out[plane * EX_DIAG_N + counter]
__global__ __launch_bounds__(EX_T) void k_ex_span_sums(ExArgs a, int pass, int max_spans, double* __restrict__ sums) {
    __shared__ ExShared sh;
    const int pl = blockIdx.y;
    ex_span_sum_plane(sh, a.p[pl], (size_t)a.n[pl], a.mean[pl], pass, (int)blockIdx.x, sums + (size_t)pl * max_spans);
}

__global__ __launch_bounds__(EX_T) void k_ex_span_maps(ExArgs a, int pass, int max_spans, const double* __restrict__ sums, ExSpanEntry* __restrict__ table) {
    __shared__ ExShared sh;
    const int pl = blockIdx.y;
    ex_span_map_plane(sh, a.p[pl], (size_t)a.n[pl], a.mean[pl], pass, (int)blockIdx.x, sums + (size_t)pl * max_spans, table + (size_t)pl * max_spans);
}

__global__ __launch_bounds__(EX_T) void k_ex_walk(ExArgs a, int pass, int max_spans, const ExSpanEntry* __restrict__ table, uint32_t* __restrict__ diag_out) {
    __shared__ ExShared sh;
    const int pl = blockIdx.x;
    ex_walk_plane(sh, a.p[pl], (size_t)a.n[pl], a.cnt[pl], a.mean[pl], a.sd[pl], pass, table ? table + (size_t)pl * max_spans : nullptr,
                  diag_out ? diag_out + pl * EX_DIAG_N : nullptr);
}

__global__ __launch_bounds__(256) void k_ex_apply(const float* __restrict__ lab, size_t n, const float* __restrict__ stats, TrK k, const uint8_t* src,
                                                  uint8_t* out) {
    ex_apply_image(lab, n, stats, k, src, out);
}
#endif
