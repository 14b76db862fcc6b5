"""The numpy statement of include/stitch_rig_formats.h: the five camera layouts, the three NV12 matrices in 16.16 fixed point, the
chroma rules.  TEST INFRASTRUCTURE ONLY, shared by tests/test_pixfmt_host.py, tests/test_gpu_pixfmt.py and
tests/test_gpu_rig_formats.py.  Written from the header's rules, in int64 throughout (the `track` hooks report the extremes of every
intermediate, so a test can hold them to int32).

An image is a dict(fmt, w, h, data, data2, pitch, pitch2): `data` / `data2` are 1-D uint8 arrays that start at the plane's first byte.
unpack(image, matrix) -> planar (3, h, w) uint8.   pack(planar, fmt, matrix, pitch, pitch2, fill) -> image (padding = fill)."""
import numpy as np

PLANAR, RGB24, BGR24, RGBX32, BGRX32, NV12 = range(6)
PACKED = (RGB24, BGR24, RGBX32, BGRX32)
BPP = {RGB24: 3, BGR24: 3, RGBX32: 4, BGRX32: 4, NV12: 1}
R_AT = {RGB24: 0, BGR24: 2, RGBX32: 0, BGRX32: 2}  # the byte of a pixel that holds R; G is byte 1, B the other end

# matrix: yoff, ky, krv, kgu, kgv, kbu
DECODE = {0: (16, 76309, 104597, 25675, 53279, 132201), 1: (16, 76309, 117489, 13975, 34925, 138438), 2: (0, 65536, 91881, 22553, 46802, 116130)}
# matrix: yr, yg, yb, ur, ug, ub, vr, vg, vb (yoff is DECODE's)
ENCODE = {0: (16829, 33039, 6416, 9714, 19070, 28784, 28784, 24103, 4681), 1: (11966, 40254, 4064, 6596, 22188, 28784, 28784, 26145, 2639),
          2: (19595, 38470, 7471, 11058, 21710, 32768, 32768, 27439, 5329)}


def tight(fmt, w):
    return (0, 0) if fmt == PLANAR else (BPP[fmt] * w, 2 * ((w + 1) // 2) if fmt == NV12 else 0)


def image_bytes(fmt, w, h, pitch=None, pitch2=None):
    """(bytes, bytes2): each plane from its first byte to the last pixel byte of its last row; None for a bad format, size or pitch."""
    if fmt not in range(6) or w < 1 or h < 1:
        return None
    if fmt == PLANAR:
        return 3 * w * h, 0
    t = tight(fmt, w)
    pitch, pitch2 = t[0] if pitch is None else pitch, t[1] if pitch2 is None else pitch2
    if pitch < t[0] or (fmt == NV12 and pitch2 < t[1]):
        return None
    return (h - 1) * pitch + t[0], ((((h + 1) // 2) - 1) * pitch2 + t[1] if fmt == NV12 else 0)


def _note(track, *values):
    if track is not None:
        for v in values:
            track[0], track[1] = min(track[0], int(np.min(v))), max(track[1], int(np.max(v)))


def decode(Y, Cb, Cr, matrix, track=None):
    """Arrays of Y, Cb, Cr (any integer type, 0 .. 255) -> R, G, B uint8."""
    yoff, ky, krv, kgu, kgv, kbu = DECODE[matrix]
    c, d, e = Y.astype(np.int64) - yoff, Cb.astype(np.int64) - 128, Cr.astype(np.int64) - 128
    r, g, b = ky * c + krv * e + 32768, ky * c - kgu * d - kgv * e + 32768, ky * c + kbu * d + 32768
    _note(track, ky * c, krv * e, kgu * d, kgv * e, kbu * d, ky * c - kgu * d, r, g, b)
    return tuple(np.clip(v >> 16, 0, 255).astype(np.uint8) for v in (r, g, b))  # >> on int64 is arithmetic: floor


def encode(R, G, B, matrix, track=None):
    """Arrays of R, G, B -> per-pixel Y, Cb, Cr uint8 (before any chroma averaging)."""
    yr, yg, yb, ur, ug, ub, vr, vg, vb = ENCODE[matrix]
    yoff = DECODE[matrix][0]
    R, G, B = (v.astype(np.int64) for v in (R, G, B))
    y, u, v = yr * R + yg * G + yb * B + 32768, -ur * R - ug * G + ub * B + 32768, vr * R - vg * G - vb * B + 32768
    _note(track, yr * R, yr * R + yg * G, -ur * R, -ur * R - ug * G, vr * R, vr * R - vg * G, y, u, v, (y >> 16) + yoff, (u >> 16) + 128, (v >> 16) + 128)
    return (np.clip((y >> 16) + yoff, 0, 255).astype(np.uint8), np.clip((u >> 16) + 128, 0, 255).astype(np.uint8),
            np.clip((v >> 16) + 128, 0, 255).astype(np.uint8))


def _rows(plane, h, pitch, row_bytes):
    """The pixel bytes of a pitched plane as an (h, row_bytes) array (a copy)."""
    return np.stack([plane[y * pitch:y * pitch + row_bytes] for y in range(h)])


def unpack(im, matrix=0):
    fmt, w, h = im["fmt"], im["w"], im["h"]
    if fmt == PLANAR:
        return np.ascontiguousarray(np.asarray(im["data"]).reshape(3, h, w))
    if fmt in PACKED:
        px = _rows(im["data"], h, im["pitch"], BPP[fmt] * w).reshape(h, w, BPP[fmt])
        return np.ascontiguousarray(np.stack([px[:, :, R_AT[fmt]], px[:, :, 1], px[:, :, 2 - R_AT[fmt]]]))
    Y = _rows(im["data"], h, im["pitch"], w)
    wp, hp = (w + 1) // 2, (h + 1) // 2
    uv = _rows(im["data2"], hp, im["pitch2"], 2 * wp).reshape(hp, wp, 2)
    yy, xx = np.arange(h)[:, None] // 2, np.arange(w)[None, :] // 2  # replication: pixel (x, y) takes the pair (x / 2, y / 2)
    return np.ascontiguousarray(np.stack(decode(Y, uv[yy, xx, 0], uv[yy, xx, 1], matrix)))


def chroma_down(c):
    """(h, w) per-pixel 8-bit values -> (ceil(h/2), ceil(w/2)): (s + 2) >> 2 over each 2 x 2 block, coordinates clamped to the image."""
    h, w = c.shape
    ys, xs = np.minimum(np.arange(2 * ((h + 1) // 2)), h - 1), np.minimum(np.arange(2 * ((w + 1) // 2)), w - 1)
    c = c.astype(np.int64)[ys][:, xs]
    return ((c[0::2, 0::2] + c[0::2, 1::2] + c[1::2, 0::2] + c[1::2, 1::2] + 2) >> 2).astype(np.uint8)


def pack(planar, fmt, matrix=0, pitch=None, pitch2=None, fill=0xEE):
    _, h, w = planar.shape
    if fmt == PLANAR:
        return dict(fmt=fmt, w=w, h=h, data=np.ascontiguousarray(planar).reshape(-1).copy(), data2=None, pitch=0, pitch2=0)
    t = tight(fmt, w)
    pitch, pitch2 = t[0] if pitch is None else pitch, t[1] if pitch2 is None else pitch2
    b1, b2 = image_bytes(fmt, w, h, pitch, pitch2)
    data, data2 = np.full(b1, fill, np.uint8), (np.full(b2, fill, np.uint8) if b2 else None)
    if fmt in PACKED:
        px = np.full((h, w, BPP[fmt]), 255, np.uint8)  # X is 255
        px[:, :, R_AT[fmt]], px[:, :, 1], px[:, :, 2 - R_AT[fmt]] = planar[0], planar[1], planar[2]
        rows = px.reshape(h, -1)
    else:
        Y, u, v = encode(planar[0], planar[1], planar[2], matrix)
        rows = Y
        uv = np.stack([chroma_down(u), chroma_down(v)], axis=2).reshape((h + 1) // 2, -1)
        for j in range(uv.shape[0]):
            data2[j * pitch2:j * pitch2 + uv.shape[1]] = uv[j]
    for y in range(h):
        data[y * pitch:y * pitch + rows.shape[1]] = rows[y]
    return dict(fmt=fmt, w=w, h=h, data=data, data2=data2, pitch=pitch, pitch2=pitch2)
