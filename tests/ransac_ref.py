"""Restatement of ImageProcess::RANSAC (ImageProcess.cpp:395-529) with CImg 2.4.0's solve / _LU / _solve / SVD / get_pseudoinvert
in Python doubles and numpy float32 / float64 elementwise operations (no FMA anywhere), the operation order of the cited lines.
tests/test_ransac_host.py checks it against the reference's recorded maps bit for bit; the GPU tests then use it where the
reference is not available.

Everything per-row is a numpy elementwise operation; every sum over rows is a sequential running sum (np.cumsum is a plain
left-to-right loop, np.sum is pairwise and is not used)."""
import math

import numpy as np

f32 = np.float32
OK, TOO_FEW, NO_CONSENSUS, DRAW_CAP = 0, 1, 2, 3
ROUNDS = math.ceil(math.log(1 - 0.99) / math.log(1 - 0.5 ** 4))  # 72, ImageProcess.cpp:398


def rand_stream(seed=666666):
    """glibc's rand() after srand(seed): random_r.c TYPE_3.  A generator of ints."""
    seed &= 0xFFFFFFFF
    word = seed - (1 << 32) if seed >= 1 << 31 else seed
    if word == 0:
        word = 1
    r = [word]
    for _ in range(1, 31):
        hi, lo = int(word / 127773), int(math.fmod(word, 127773))  # C division truncates
        word = 16807 * lo - 2836 * hi
        if word < 0:
            word += 2147483647
        r.append(word)
    r = [v & 0xFFFFFFFF for v in r]
    f, b, k = 3, 0, -310
    while True:
        v = (r[f] + r[b]) & 0xFFFFFFFF
        r[f] = v
        f = 0 if f == 30 else f + 1
        b = 0 if b == 30 else b + 1
        if k >= 0:
            yield v >> 1
        k += 1


def lu_solve4(A, bs):
    """A[row][col] 4x4 doubles; bs: right-hand sides.  CImg _LU (CImg.h:25911-25953) + _solve (25401-25420)."""
    N = 4
    lu = [list(map(float, row)) for row in A]
    vv = [0.0] * N
    indx = [0] * N
    for i in range(N):
        vmax = 0.0
        for j in range(N):
            t = abs(lu[i][j])
            if t > vmax:
                vmax = t
        assert vmax != 0  # a row of the design matrix ends in 1
        vv[i] = 1 / vmax
    imax = 0
    for j in range(N):
        for i in range(j):
            s = lu[i][j]
            for k in range(i):
                s -= lu[i][k] * lu[k][j]
            lu[i][j] = s
        vmax = 0.0
        for i in range(j, N):
            s = lu[i][j]
            for k in range(j):
                s -= lu[i][k] * lu[k][j]
            lu[i][j] = s
            t = vv[i] * abs(s)
            if t >= vmax:
                vmax, imax = t, i
        if j != imax:
            lu[imax], lu[j] = lu[j], lu[imax]
            vv[imax] = vv[j]
        indx[j] = imax
        if lu[j][j] == 0:
            lu[j][j] = 1e-20
        t = _div(1.0, lu[j][j])
        for i in range(j + 1, N):
            lu[i][j] = lu[i][j] * t
    outs = []
    for b in bs:
        x = list(map(float, b))
        ii = -1
        for i in range(N):
            ip = indx[i]
            s = x[ip]
            x[ip] = x[i]
            if ii >= 0:
                for j in range(ii, i):
                    s -= lu[i][j] * x[j]
            elif s != 0:
                ii = i
            x[i] = s
        for i in range(N - 1, -1, -1):
            s = x[i]
            for j in range(i + 1, N):
                s -= lu[i][j] * x[j]
            x[i] = _div(s, lu[i][i])
        outs.append(x)
    return outs


def _div(a, b):
    """IEEE double division (Python raises on a zero divisor)."""
    with np.errstate(all="ignore"):
        return float(np.float64(a) / np.float64(b))


def _sqrt(a):
    with np.errstate(all="ignore"):
        return float(np.sqrt(np.float64(a)))


def _hypot(x, y):
    nx, ny = abs(x), abs(y)
    if nx < ny:
        t, nx = nx, ny
    else:
        t = ny
    if nx > 0:
        t = _div(t, nx)
        return nx * _sqrt(1 + t * t)
    return 0.0


def _ssum(terms):
    """value = 0; value += t for t in terms, in order."""
    if len(terms) == 0:
        return 0.0
    with np.errstate(all="ignore"):
        return float(np.cumsum(np.concatenate([[0.0], terms]))[-1])


def svd(A, max_iteration=40):
    """CImg::SVD (CImg.h:25755-25895), sorting=true.  A (H, 4) float64 -> U (H, 4), S [4], V (4, 4), all [row][col]."""
    with np.errstate(all="ignore"):
        return _svd(np.array(A, np.float64), max_iteration)


def _svd(U, max_iteration):
    H, W = U.shape
    S = [0.0] * W
    V = [[0.0] * W for _ in range(W)]
    rv1 = [0.0] * W
    anorm = c = f = g = h = s = scale = 0.0
    l = nm = 0
    for i in range(W):
        l = i + 1
        rv1[i] = scale * g
        g = s = scale = 0.0
        if i < H:
            scale = _ssum(np.abs(U[i:, i]))
            if scale:
                U[i:, i] /= scale
                s = _ssum(U[i:, i] * U[i:, i])
                f = float(U[i, i])
                g = (-1 if f >= 0 else 1) * _sqrt(s)
                h = f * g - s
                U[i, i] = f - g
                for j in range(l, W):
                    s = _ssum(U[i:, i] * U[i:, j])
                    f = _div(s, h)
                    U[i:, j] += f * U[i:, i]
                U[i:, i] *= scale
        S[i] = scale * g
        g = s = scale = 0.0
        if i < H and i != W - 1:
            for k in range(l, W):
                scale += abs(float(U[i, k]))
            if scale:
                for k in range(l, W):
                    U[i, k] /= scale
                    s += float(U[i, k]) * float(U[i, k])
                f = float(U[i, l])
                g = (-1 if f >= 0 else 1) * _sqrt(s)
                h = f * g - s
                U[i, l] = f - g
                for k in range(l, W):
                    rv1[k] = _div(float(U[i, k]), h)
                if l < H:
                    sj = np.zeros(H - l)
                    for k in range(l, W):
                        sj = sj + U[l:, k] * U[i, k]
                    for k in range(l, W):
                        U[l:, k] += sj * rv1[k]
                for k in range(l, W):
                    U[i, k] *= scale
        anorm = float(max(f32(anorm), f32(abs(S[i]) + abs(rv1[i]))))
    for i in range(W - 1, -1, -1):
        if i < W - 1:
            if g:
                for j in range(l, W):
                    V[j][i] = _div(_div(float(U[i, j]), float(U[i, l])), g)
                for j in range(l, W):
                    s = 0.0
                    for k in range(l, W):
                        s += float(U[i, k]) * V[k][j]
                    for k in range(l, W):
                        V[k][j] += s * V[k][i]
            for j in range(l, W):
                V[i][j] = V[j][i] = 0.0
        V[i][i] = 1.0
        g = rv1[i]
        l = i
    for i in range(min(W, H) - 1, -1, -1):
        l = i + 1
        g = S[i]
        U[i, l:] = 0.0
        if g:
            g = _div(1.0, g)
            for j in range(l, W):
                s = _ssum(U[l:, i] * U[l:, j])
                f = _div(s, float(U[i, i])) * g
                U[i:, j] += f * U[i:, i]
            U[i:, i] *= g
        else:
            U[i:, i] = 0.0
        U[i, i] += 1
    for k in range(W - 1, -1, -1):
        for _its in range(max_iteration):
            flag = True
            l = k
            while l >= 1:
                nm = l - 1
                if (abs(rv1[l]) + anorm) == anorm:
                    flag = False
                    break
                if (abs(S[nm]) + anorm) == anorm:
                    break
                l -= 1
            if flag:
                c, s = 0.0, 1.0
                for i in range(l, k + 1):
                    f = s * rv1[i]
                    rv1[i] = c * rv1[i]
                    if (abs(f) + anorm) == anorm:
                        break
                    g = S[i]
                    h = _hypot(f, g)
                    S[i] = h
                    h = _div(1.0, h)
                    c = g * h
                    s = -f * h
                    y, z = U[:, nm].copy(), U[:, i].copy()
                    U[:, nm] = y * c + z * s
                    U[:, i] = z * c - y * s
            z = S[k]
            if l == k:
                if z < 0:
                    S[k] = -z
                    for j in range(W):
                        V[j][k] = -V[j][k]
                break
            nm = k - 1
            x, y = S[l], S[nm]
            g, h = rv1[nm], rv1[k]
            f = _div((y - z) * (y + z) + (g - h) * (g + h), max(1e-25, 2 * h * y))
            g = _hypot(f, 1.0)
            f = _div((x - z) * (x + z) + h * (_div(y, f + (g if f >= 0 else -g)) - h), max(1e-25, x))
            c = s = 1.0
            for j in range(l, nm + 1):
                i = j + 1
                g = rv1[i]
                h = s * g
                g = c * g
                y = S[i]
                z = _hypot(f, h)
                rv1[j] = z
                c = _div(f, max(1e-25, z))
                s = _div(h, max(1e-25, z))
                f = x * c + g * s
                g = g * c - x * s
                h = y * s
                y *= c
                for jj in range(W):
                    xx, zz = V[jj][j], V[jj][i]
                    V[jj][j] = xx * c + zz * s
                    V[jj][i] = zz * c - xx * s
                z = _hypot(f, h)
                S[j] = z
                if z:
                    z = _div(1.0, max(1e-25, z))
                    c = f * z
                    s = h * z
                f = c * g + s * y
                x = c * y - s * g
                yy, zz = U[:, j].copy(), U[:, i].copy()
                U[:, j] = yy * c + zz * s
                U[:, i] = zz * c - yy * s
            rv1[l] = 0.0
            rv1[k] = f
            S[k] = x
    perm = list(range(W))
    _quicksort_dec(S, perm, 0, W - 1)
    return U[:, perm], S, [[row[p] for p in perm] for row in V]


def _quicksort_dec(a, p, m, M):
    """CImg::_quicksort, decreasing, with its permutation (CImg.h:25676-25731)."""
    if m < M:
        mid = (m + M) // 2

        def sw(i, j):
            a[i], a[j] = a[j], a[i]
            p[i], p[j] = p[j], p[i]
        if a[m] < a[mid]:
            sw(m, mid)
        if a[mid] < a[M]:
            sw(M, mid)
        if a[m] < a[mid]:
            sw(m, mid)
        if M - m >= 3:
            piv = a[mid]
            i, j = m, M
            while True:
                while a[i] > piv:
                    i += 1
                while a[j] < piv:
                    j -= 1
                if i <= j:
                    sw(i, j)
                    i += 1
                    j -= 1
                if not i <= j:
                    break
            if m < j:
                _quicksort_dec(a, p, m, j)
            if i < M:
                _quicksort_dec(a, p, i, M)


def lstsq(A, bs):
    """A.get_pseudoinvert() * b (CImg.h:25293-25302, 12244-12264)."""
    A = np.asarray(A, np.float64)
    H, W = A.shape
    U, S, V = svd(A)
    smax = S[0]
    for v in S[1:]:
        if v > smax:
            smax = v
    tol = float(f32(1.11e-16) * f32(max(W, H))) * smax
    for x in range(W):
        s = S[x]
        invs = _div(1.0, s) if s > tol else 0.0
        for y in range(W):
            V[y][x] *= invs
    outs = [[] for _ in bs]
    with np.errstate(all="ignore"):
        for j in range(W):
            pv = np.zeros(H)
            for k in range(W):
                pv = pv + V[j][k] * U[:, k]
            for o, b in zip(outs, bs):
                o.append(_ssum(pv * np.asarray(b, np.float64)))
    return outs


def fit(sx, sy, dx, dy, idx):
    """getHomographyMat / getInlinerHomography (ImageProcess.cpp:439-462, 500-529) over the rows idx, in that order -> 8 doubles."""
    idx = np.asarray(idx, np.int64)
    x, y = sx[idx].astype(np.float64), sy[idx].astype(np.float64)
    A = np.stack([x, y, x * y, np.ones(len(idx))], 1)
    bs = [dx[idx].astype(np.float64), dy[idx].astype(np.float64)]
    x1, x2 = lu_solve4(A.tolist(), [b.tolist() for b in bs]) if len(idx) == 4 else lstsq(A, bs)
    return list(x1) + list(x2)


def inlier_mask(sx, sy, dx, dy, P, thr=4.0):
    """getInlinerIndex's test (ImageProcess.cpp:466, 470, 482-491) for hypotheses P (k, 8) over all points -> (k, n) bool."""
    P = np.asarray(P, np.float64).reshape(-1, 8)[:, :, None]
    x, y = sx.astype(np.float64)[None, :], sy.astype(np.float64)[None, :]
    with np.errstate(all="ignore"):
        X = (((P[:, 0] * x + P[:, 1] * y) + (P[:, 2] * x) * y) + P[:, 3]).astype(f32)
        Y = (((P[:, 4] * x + P[:, 5] * y) + (P[:, 6] * x) * y) + P[:, 7]).astype(f32)
        ex, ey = X - dx[None, :], Y - dy[None, :]
        d = np.sqrt(ex * ex + ey * ey)
        assert d.dtype == f32
        return d < f32(thr)


def ransac(sx, sy, dx, dy, rounds=0, threshold=4.0, seed=666666, max_draws=0, chunk=128):
    """-> (p [8 floats], inlier index list, info [status, n, winning round, winning count, rand() values consumed])."""
    sx, sy, dx, dy = (np.ascontiguousarray(v, f32) for v in (sx, sy, dx, dy))
    n = len(sx)
    k = rounds or ROUNDS
    cap = max_draws or 32 * k + 4096
    nan8 = [float("nan")] * 8
    if n < 4:
        return nan8, [], [TOO_FEW, n, -1, 0, 0]
    rs = rand_stream(seed)
    used = 0
    samples = []
    for _ in range(k):
        chosen = []
        for _i in range(4):
            while True:
                if used >= cap:
                    return nan8, [], [DRAW_CAP, n, -1, 0, used]
                index = next(rs) % n
                used += 1
                if index not in chosen:
                    break
            chosen.append(index)
        samples.append(chosen)
    best_count, best_round, best_p = 0, -1, None
    for r0 in range(0, k, chunk):
        P = [fit(sx, sy, dx, dy, c) for c in samples[r0:r0 + chunk]]
        counts = inlier_mask(sx, sy, dx, dy, P, threshold).sum(1)
        for j, cnt in enumerate(counts):
            if cnt > best_count:
                best_count, best_round, best_p = int(cnt), r0 + j, P[j]
    if best_count == 0:
        return nan8, [], [NO_CONSENSUS, n, -1, 0, used]
    best = np.nonzero(inlier_mask(sx, sy, dx, dy, [best_p], threshold)[0])[0].tolist()
    return fit(sx, sy, dx, dy, best), best, [OK, n, best_round, best_count, used]


def same_p(a, b):
    """All 64 bits of all 8 doubles equal; where a component is not finite, the same class (NaN, +inf, -inf) suffices."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    if a.shape != b.shape:
        return False
    fin = np.isfinite(a)
    if not np.array_equal(fin, np.isfinite(b)):
        return False
    if not np.array_equal(a[fin].view(np.uint64), b[fin].view(np.uint64)):
        return False
    return np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(a[~fin & ~np.isnan(a)], b[~fin & ~np.isnan(b)])


def stitch_lists(frames, pairs, src, dst):
    """The two lists matching() hands to RANSAC for src -> dst (ImageProcess.cpp:177-202) from per-frame (x, y) arrays in map
    order and the accepted (data, query) lists pairs[(i, j)] = getImgPair(imgs[i], imgs[j]).  Returns (dst_to_src, src_to_dst),
    each (sx, sy, dx, dy): RANSAC of the first is forward_H, of the second backward_H."""
    (xs, ys), (xd, yd) = frames[src], frames[dst]
    p_sd, p_ds = np.asarray(pairs[(src, dst)]).reshape(-1, 2), np.asarray(pairs[(dst, src)]).reshape(-1, 2)
    if len(p_sd) > len(p_ds):
        s2d = (xs[p_sd[:, 0]], ys[p_sd[:, 0]], xd[p_sd[:, 1]], yd[p_sd[:, 1]])
        d2s = (s2d[2], s2d[3], s2d[0], s2d[1])
    else:
        d2s = (xd[p_ds[:, 0]], yd[p_ds[:, 0]], xs[p_ds[:, 1]], ys[p_ds[:, 1]])
        s2d = (d2s[2], d2s[3], d2s[0], d2s[1])
    return d2s, s2d
