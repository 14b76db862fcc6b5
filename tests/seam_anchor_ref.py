"""numpy statements of include/stitch_seam_anchor.h, on tests/seam_path_ref.py's cost and dynamic programme: the temporal term of a
row (penalty), and the anchored finder (anchored_path) with its path, its total D and `moved`."""
import itertools

import numpy as np

import seam_path_ref as sp

ANCHOR_MAX = 2055
INT32_MIN, INT32_MAX = -2 ** 31, 2 ** 31 - 1


def penalty(ns, r, w, T):
    """w * min(|s - r[y]|, T) for s = 0 .. ns - 1 as a (ch, ns) int64 array; the difference in Python integers, so any int32 r is exact."""
    s = np.arange(ns, dtype=np.int64)[None, :]
    r = np.asarray([int(v) for v in r], dtype=np.int64)[:, None]  # |s - r| < 2^32: exact in int64
    return np.int64(w) * np.minimum(np.abs(s - r), np.int64(T))


def moved_of(path, r, T):
    return int(sum(min(abs(int(s) - int(v)), int(T)) for s, v in zip(path, r)))


def anchored_path(c, K, r, w, T):
    """-> (path, D, moved) of the cost table c (ch, cw + 1) under the anchor r (ch integers, or None: unanchored, moved = 0)."""
    c = np.asarray(c, np.int64)
    if r is None:
        path, total = sp.dp_path(c, K)
        return path, total, 0
    assert 0 <= w and 1 <= T and w * T <= ANCHOR_MAX and len(r) == c.shape[0]
    path, total = sp.dp_path(c + penalty(c.shape[1], r, w, T), K)
    return path, total, moved_of(path, r, T)


def brute_force(c, K, r, w, T):
    """The least c_t total over every path with steps within K, by enumeration (small tables only)."""
    ct = np.asarray(c, np.int64) + penalty(np.asarray(c).shape[1], r, w, T)
    h, ns = ct.shape
    best = None
    for p in itertools.product(range(ns), repeat=h):
        if all(abs(p[y] - p[y - 1]) <= K for y in range(1, h)):
            t = sp.path_cost(ct, p)
            best = t if best is None or t < best else best
    return best
