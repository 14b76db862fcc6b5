"""numpy statements of include/stitch_seam_path.h: the cost of a path, the dynamic programme and its walk back (seam_path);
the level-0 mask of a path (mask_from_path); and the blend with any level-0 mask (blend_with_mask), which restates blend_core of
oracle/stitch_oracle.c through the oracle's own blur, decimation and expansion (tests/oracle_lib.py)."""
import itertools

import numpy as np

WRONG = 4096


def gray(img):
    """R + 2 G + B of a (3, H, W) uint8 image, as int64."""
    i = img.astype(np.int64)
    return i[0] + 2 * i[1] + i[2]


def erode_x(mask, m):
    """A'[y][x]: mask holds on every x' in [x - m, x + m] inside the canvas."""
    mask = np.asarray(mask, bool)
    h, w = mask.shape
    bad = np.concatenate([np.zeros((h, 1), np.int64), np.cumsum(~mask, axis=1)], axis=1)  # bad[s] = #{x < s : not mask}
    x = np.arange(w)
    lo, hi = np.maximum(x - m, 0), np.minimum(x + m, w - 1) + 1
    return bad[:, hi] == bad[:, lo]


def cost(a, b, cov_a, cov_b, branch, margin):
    """c(y, s) for s = 0 .. cw as an (ch, cw + 1) int64 array.  a, b: the (3, ch, cw) uint8 canvases; cov_*: (ch, cw), non-zero = covered."""
    A, B = np.asarray(cov_a) != 0, np.asarray(cov_b) != 0
    h, w = A.shape
    Ae, Be = erode_x(A, margin), erode_x(B, margin)
    d = np.where(A & B, np.abs(gray(a) - gray(b)), 0)
    dp = np.zeros((h, w + 2), np.int64)  # columns -1 .. cw
    dp[:, 1:w + 1] = d
    only_b, only_a = B & ~Ae, A & ~Be
    Lm, Rm = (only_b, only_a) if branch == 0 else (only_a, only_b)
    z = np.zeros((h, 1), np.int64)
    left = np.concatenate([z, np.cumsum(Lm, axis=1)], axis=1)        # #{x < s in L}
    right = Rm.sum(axis=1, keepdims=True) - np.concatenate([z, np.cumsum(Rm, axis=1)], axis=1)  # #{x >= s in R}
    return WRONG * (left + right) + dp[:, 0:w + 1] + dp[:, 1:w + 2]


def dp_path(c, K):
    """The least-cost path through c (ch, cw + 1) with |s[y] - s[y-1]| <= K -> (path int32 (ch,), total cost).  Predecessor ties:
    the smallest |t - s|, then the smaller t; the end: the smallest s."""
    c = np.asarray(c, np.int64)
    h, ns = c.shape
    big = np.int64(1) << 62
    D = c[0].copy()
    pred = np.zeros((h, ns), np.int64)
    order = [0] + [v for k in range(1, K + 1) for v in (-k, k)]
    for y in range(1, h):
        pad = np.full(ns + 2 * K, big, np.int64)
        pad[K:K + ns] = D
        best, at = pad[K:K + ns].copy(), np.zeros(ns, np.int64)
        for o in order[1:]:
            v = pad[K + o:K + o + ns]
            take = v < best
            best = np.where(take, v, best)
            at = np.where(take, o, at)
        pred[y] = at
        D = best + c[y]
    s = int(np.argmin(D))  # the first minimum
    total = int(D[s])
    path = np.zeros(h, np.int32)
    path[h - 1] = s
    for y in range(h - 1, 0, -1):
        s += int(pred[y][s])
        path[y - 1] = s
    return path, total


def seam_path(a, b, cov_a, cov_b, branch, K, margin):
    return dp_path(cost(a, b, cov_a, cov_b, branch, margin), K)


def path_cost(c, path):
    return int(sum(int(c[y][int(s)]) for y, s in enumerate(path)))


def brute_force(c, K):
    """The least total over every path with steps within K, by enumeration (small canvases only)."""
    h, ns = np.asarray(c).shape
    best = None
    for p in itertools.product(range(ns), repeat=h):
        if all(abs(p[y] - p[y - 1]) <= K for y in range(1, h)):
            t = path_cost(c, p)
            best = t if best is None or t < best else best
    return best


def mask_from_path(path, branch, cw):
    """M[y][x] = 1 where x < s[y] (branch 0) or x >= s[y] (branch 1), as float32 (ch, cw)."""
    x = np.arange(cw)[None, :]
    s = np.asarray(path, np.int64)[:, None]
    return (x < s if branch == 0 else x >= s).astype(np.float32)


def constant_path(seam, seam_rule, ch):
    """The path of a Seam's vertical step: ceil(thr) for branch 0 (thr = ov, rule 0 in float, rule 1 in double), start for branch 1."""
    if seam.branch == 0:
        thr = float(np.float32(np.float64(seam.sum_ov_x) / np.float64(seam.n_ov))) if seam_rule == 0 else seam.sum_ov_x / seam.n_ov
        return np.full(ch, int(np.ceil(thr)), np.int32)
    return np.full(ch, int(seam.start), np.int32)


def opts_for(O, cw, ch, blur_kind, seam_rule, sigma=2.0):
    """Blend options of a blur kind and a seam rule for a cw x ch canvas: the root variant's level rule (the longer side) where
    the canvas has such a pyramid, the other (the shorter side) where a level of the first would have no rows."""
    level_rule = 0 if O.pyramid_levels(cw, ch, 0)[0] > 0 else 1
    return dict(sigma=sigma, blur_kind=blur_kind, level_rule=level_rule, seam_rule=seam_rule)


def blend_with_mask(O, a, b, mask, opts):
    """blend_core of oracle/stitch_oracle.c with `mask` (ch, cw) as the level-0 mask: the collapsed float32 image (3, ch, cw), before
    the final cast.  O: tests/oracle_lib.Oracle; a, b: (3, ch, cw) uint8 or float32 canvases."""
    _, h, w = a.shape
    L, lw, lh = O.pyramid_levels(w, h, opts["level_rule"])
    assert L >= 1
    A, B, M = [a.astype(np.float32)], [b.astype(np.float32)], [np.asarray(mask, np.float32).reshape(1, h, w)]
    for i in range(1, L):  # REDUCE
        for P in (A, B, M):
            P.append(O.decimate(O.blur(P[i - 1], opts["sigma"], opts["blur_kind"]), lw[i], lh[i]))
    for i in range(L - 1):  # Laplacian, finest first
        A[i] = A[i] - O.expand(A[i + 1], lw[i], lh[i])
        B[i] = B[i] - O.expand(B[i + 1], lw[i], lh[i])
    for i in range(L):  # a * m is a float product; b * (1.0 - m) and the sum are double; stored float
        m = M[i][0]
        am = A[i] * m[None]
        A[i] = (am.astype(np.float64) + B[i].astype(np.float64) * (1.0 - m.astype(np.float64))[None]).astype(np.float32)
    E = A[L - 1]
    for i in range(L - 2, -1, -1):  # collapse
        v = A[i] + O.expand(E, lw[i], lh[i])
        E = np.where(v > 255, np.float32(255), np.where(v < 0, np.float32(0), v)).astype(np.float32)
    return E


def blend_with_mask_as(O, a, b, mask, opts):
    """blend_with_mask in the pixel type of a: the truncating cast for uint8, the float image as it stands."""
    e = blend_with_mask(O, a, b, mask, opts)
    return e.astype(np.uint8) if a.dtype == np.uint8 else e
