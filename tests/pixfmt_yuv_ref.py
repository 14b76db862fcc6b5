"""The numpy statement of include/stitch_rig_formats_yuv.h: YUYV, UYVY and NV16 (4:2:2) and NV21, on the matrices, the decode, the
per-pixel encode and the 2 x 2 rule of tests/pixfmt_ref.py.  TEST INFRASTRUCTURE ONLY, shared by tests/test_pixfmt_yuv_host.py,
tests/test_gpu_pixfmt_yuv.py and tests/test_gpu_rig_formats_yuv.py.  Written from the header's rules, in int64 throughout.

Images are pixfmt_ref's dicts.  tight, image_bytes, unpack and pack take the codes 16 .. 19 and pass 0 .. 5 through to pixfmt_ref."""
import numpy as np

import pixfmt_ref as pf
from pixfmt_ref import BGR24, BGRX32, NV12, PLANAR, RGB24, RGBX32  # noqa: F401  (one module names every code)

YUYV, UYVY, NV21, NV16 = range(16, 20)
NEW = (YUYV, UYVY, NV21, NV16)
ALL = tuple(range(6)) + NEW
ONE_PLANE_422 = (YUYV, UYVY)
# YUYV, UYVY: the bytes of a group that hold Y0, Cb, Y1, Cr.  NV21, NV16: the bytes of a chroma pair that hold Cb, Cr.
GROUP = {YUYV: (0, 1, 2, 3), UYVY: (1, 0, 3, 2)}
PAIR = {NV21: (1, 0), NV16: (0, 1)}


def tight(fmt, w):
    if fmt not in NEW:
        return pf.tight(fmt, w)
    return (4 * ((w + 1) // 2), 0) if fmt in ONE_PLANE_422 else (w, 2 * ((w + 1) // 2))


def _chroma_rows(fmt, h):
    return (h + 1) // 2 if fmt == NV21 else h


def image_bytes(fmt, w, h, pitch=None, pitch2=None):
    """(bytes, bytes2): each plane from its first byte to the last pixel byte of its last row; None for a bad format, size or pitch."""
    if fmt not in NEW:
        return pf.image_bytes(fmt, w, h, pitch, pitch2)
    if w < 1 or h < 1:
        return None
    t = tight(fmt, w)
    pitch, pitch2 = t[0] if pitch is None else pitch, t[1] if pitch2 is None else pitch2
    if pitch < t[0] or (fmt not in ONE_PLANE_422 and pitch2 < t[1]):
        return None
    return (h - 1) * pitch + t[0], (0 if fmt in ONE_PLANE_422 else (_chroma_rows(fmt, h) - 1) * pitch2 + t[1])


def chroma_down_422(c):
    """(h, w) per-pixel 8-bit values -> (h, ceil(w/2)): (s + 1) >> 1 over each 2 x 1 pair, the column clamped to the image."""
    w = c.shape[1]
    c = c.astype(np.int64)[:, np.minimum(np.arange(2 * ((w + 1) // 2)), w - 1)]
    return ((c[:, 0::2] + c[:, 1::2] + 1) >> 1).astype(np.uint8)


def unpack(im, matrix=0):
    fmt, w, h = im["fmt"], im["w"], im["h"]
    if fmt not in NEW:
        return pf.unpack(im, matrix)
    wp, xx = (w + 1) // 2, np.arange(w)[None, :] // 2
    if fmt in ONE_PLANE_422:
        y0, cb, y1, cr = GROUP[fmt]
        g = pf._rows(im["data"], h, im["pitch"], 4 * wp).reshape(h, wp, 4)
        Y = np.stack([g[:, :, y0], g[:, :, y1]], axis=2).reshape(h, 2 * wp)[:, :w]  # (the Y1 of an odd width's last group is dropped)
        yy = np.arange(h)[:, None]
        return np.ascontiguousarray(np.stack(pf.decode(Y, g[yy, xx, cb], g[yy, xx, cr], matrix)))
    Y = pf._rows(im["data"], h, im["pitch"], w)
    hp = _chroma_rows(fmt, h)
    uv = pf._rows(im["data2"], hp, im["pitch2"], 2 * wp).reshape(hp, wp, 2)
    yy = np.arange(h)[:, None] // (2 if fmt == NV21 else 1)  # replication: pixel (x, y) takes the pair (x / 2, y) of 4:2:2
    return np.ascontiguousarray(np.stack(pf.decode(Y, uv[yy, xx, PAIR[fmt][0]], uv[yy, xx, PAIR[fmt][1]], matrix)))


def pack(planar, fmt, matrix=0, pitch=None, pitch2=None, fill=0xEE):
    if fmt not in NEW:
        return pf.pack(planar, fmt, matrix, pitch, pitch2, fill)
    _, h, w = planar.shape
    t = tight(fmt, w)
    pitch, pitch2 = t[0] if pitch is None else pitch, t[1] if pitch2 is None else pitch2
    b1, b2 = image_bytes(fmt, w, h, pitch, pitch2)
    data, data2 = np.full(b1, fill, np.uint8), (np.full(b2, fill, np.uint8) if b2 else None)
    Y, u, v = pf.encode(planar[0], planar[1], planar[2], matrix)
    wp = (w + 1) // 2
    if fmt in ONE_PLANE_422:
        y0, cb, y1, cr = GROUP[fmt]
        Yc = Y[:, np.minimum(np.arange(2 * wp), w - 1)]  # an odd width: the last group's Y1 is the luma of pixel w - 1
        g = np.zeros((h, wp, 4), np.uint8)
        g[:, :, y0], g[:, :, y1], g[:, :, cb], g[:, :, cr] = Yc[:, 0::2], Yc[:, 1::2], chroma_down_422(u), chroma_down_422(v)
        rows = g.reshape(h, -1)
    else:
        rows = Y
        down = chroma_down_422 if fmt == NV16 else pf.chroma_down
        uv = np.zeros((_chroma_rows(fmt, h), wp, 2), np.uint8)
        uv[:, :, PAIR[fmt][0]], uv[:, :, PAIR[fmt][1]] = down(u), down(v)
        uv = uv.reshape(uv.shape[0], -1)
        for j in range(uv.shape[0]):
            data2[j * pitch2:j * pitch2 + uv.shape[1]] = uv[j]
    for y in range(h):
        data[y * pitch:y * pitch + rows.shape[1]] = rows[y]
    return dict(fmt=fmt, w=w, h=h, data=data, data2=data2, pitch=pitch, pitch2=pitch2)
