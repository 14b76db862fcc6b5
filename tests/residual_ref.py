"""The numpy statement of include/stitch_rig_monitor.h: the record of a pair over a domain, the rig's domain of a step from its
coverage masks, and the shift a record favours, the last in Python integers.  Nothing here imports the product."""
import numpy as np


def words(r):
    return 2 + 3 * (2 * r + 1) ** 2


def gray(img):
    """(3, H, W) uint8 -> (H, W) int64 of R + 2 G + B."""
    img = np.asarray(img).astype(np.int64)
    return img[0] + 2 * img[1] + img[2]


def records(a, b, domain, r):
    """a, b: the dense (3, ch, cw) uint8 canvases of the warp and of the move; domain: (ch, cw), non-zero = inside.  -> the record as
    int64: n, sum_b, then sum_a, sad, ssd per shift, dy-major."""
    ga, gb = gray(a), gray(b)
    ch, cw = gb.shape
    out = np.zeros(words(r), np.int64)
    d = np.asarray(domain) != 0
    keep = np.zeros_like(d)
    if cw > 2 * r and ch > 2 * r:
        keep[r:ch - r, r:cw - r] = d[r:ch - r, r:cw - r]
    ys, xs = np.nonzero(keep)
    out[0] = len(ys)
    out[1] = gb[ys, xs].sum()
    j = 0
    for dy in range(-r, r + 1):
        for dx in range(-r, r + 1):
            diff = ga[ys + dy, xs + dx] - gb[ys, xs]
            out[2 + 3 * j:5 + 3 * j] = ga[ys + dy, xs + dx].sum(), np.abs(diff).sum(), (diff * diff).sum()
            j += 1
    return out


def rig_domain(A, B, r):
    """A, B: a step's coverage masks as bytes.  -> D as 0 / 255 bytes: B, and A at every shifted position that lies inside the canvas."""
    A, B = np.asarray(A) != 0, np.asarray(B) != 0
    ch, cw = A.shape
    pad = np.ones((ch + 2 * r, cw + 2 * r), bool)  # outside the canvas nothing is asked
    pad[r:r + ch, r:r + cw] = A
    e = np.ones((ch, cw), bool)
    for dy in range(2 * r + 1):
        for dx in range(2 * r + 1):
            e &= pad[dy:dy + ch, dx:dx + cw]
    return (e & B).astype(np.uint8) * 255


def best_shift(record, r, zero_mean=False):
    """-> (dx, dy), or None for n == 0.  Python integers throughout."""
    rec = [int(v) for v in record]
    n, sum_b = rec[0], rec[1]
    if n == 0:
        return None
    keys = []
    j = 0
    for dy in range(-r, r + 1):
        for dx in range(-r, r + 1):
            sum_a, ssd = rec[2 + 3 * j], rec[4 + 3 * j]
            score = n * ssd - (sum_a - sum_b) ** 2 if zero_mean else ssd
            keys.append((score, dx * dx + dy * dy, dy, dx))
            j += 1
    _, _, dy, dx = min(keys)
    return dx, dy
