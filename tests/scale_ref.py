"""The numpy statement of include/stitch_rig_scale.h: the exact area-average downscale in int64, and pack(fmt) of the scaled image on top
of tests/pixfmt_ref.py / tests/pixfmt_yuv_ref.py.  TEST INFRASTRUCTURE ONLY, shared by tests/test_rig_scale_host.py and
tests/test_gpu_rig_scale.py."""
import numpy as np

import pixfmt_yuv_ref as pyr

MAX_FACTOR = 8


def rule(w, h, ow, oh):
    """The header's size rule."""
    return 1 <= ow <= w <= MAX_FACTOR * ow and 1 <= oh <= h <= MAX_FACTOR * oh


def weights(n, on):
    """(on, n) int64: w(X, x) = max(0, min((X + 1) n, (x + 1) on) - max(X n, x on)); every row sums to n."""
    X, x = np.arange(on, dtype=np.int64)[:, None], np.arange(n, dtype=np.int64)[None, :]
    return np.maximum(0, np.minimum((X + 1) * n, (x + 1) * on) - np.maximum(X * n, x * on))


def apply(A, W):
    """A @ W.T in int64 for a weight matrix of weights(): (..., n) x (on, n) -> (..., on).  A row of W is a run of at most 9 non-zero
    entries, so the product gathers that run instead of multiplying by the zeros around it (numpy's int64 matmul has no fast path)."""
    on, n = W.shape
    first = (W != 0).argmax(1)
    at = first[:, None] + np.arange(int((W != 0).sum(1).max()))[None, :]  # (on, k): the run's columns, some behind the row's end
    idx = np.minimum(at, n - 1)
    wts = np.where(at < n, W[np.arange(on)[:, None], idx], 0)
    return (A.astype(np.int64)[..., idx] * wts).sum(-1)


def sums(planar, ow, oh):
    """S = Wy @ P @ Wx.T per channel, int64 (S <= 255 w h < 2^39): the horizontal sums, then the vertical ones."""
    _, h, w = planar.shape
    H = apply(planar, weights(w, ow))                                # (3, h, ow)
    return apply(H.transpose(0, 2, 1), weights(h, oh)).transpose(0, 2, 1)  # (3, oh, ow)


def scale(planar, ow, oh):
    """(3, h, w) uint8 -> (3, oh, ow) uint8: the sums, then one division, rounded half up."""
    _, h, w = planar.shape
    assert rule(w, h, ow, oh) and w * h <= 2 ** 31 - 1
    D = w * h
    return ((2 * sums(planar, ow, oh) + D) // (2 * D)).astype(np.uint8)


def scale_pack(fmt, planar, ow, oh, matrix=0, rect=None, pitch=None, pitch2=None, fill=0xEE):
    """pack(fmt)(scale(planar[rect])): the image dict of pixfmt_yuv_ref.pack (data, data2, pitch, pitch2; padding bytes are `fill`)."""
    if rect is not None:
        x0, y0, w, h = rect
        planar = planar[:, y0:y0 + h, x0:x0 + w]
    return pyr.pack(scale(np.ascontiguousarray(planar), ow, oh), fmt, matrix, pitch, pitch2, fill)
