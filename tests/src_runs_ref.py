"""The rule of csrc/src_runs_rule.h restated in numpy (include/stitch_src_runs.h): from a pair's map to the byte offsets k_src_index
leaves in the index plane (map_to_src of csrc/k_geometry.inc), and from those to the class of every 64 x 64 tile."""
import numpy as np

TS = 64
GENERAL = 255
MAX_PATCHES = 64
BASE_OUTSIDE = 0xFFFFFFF0


def offsets(p, offx, offy, fw, fh, cw, ch, px=4):
    """-> (ch, cw) uint32: byte offset of the frame sample of every canvas pixel within a channel plane, or `outside` = 2^32 - px."""
    p = [float(v) for v in p]
    x = (np.arange(cw, dtype=np.float32) + np.float32(offx)).astype(np.float64)[None, :]
    y = (np.arange(ch, dtype=np.float32) + np.float32(offy)).astype(np.float64)[:, None]
    with np.errstate(all="ignore"):
        X = (((p[0] * x + p[1] * y) + (p[2] * x) * y) + p[3]).astype(np.float32)
        Y = (((p[4] * x + p[5] * y) + (p[6] * x) * y) + p[7]).astype(np.float32)
        lim = np.float32(2147483648.0)
        ok = (X > -lim) & (X < lim) & (Y > -lim) & (Y < lim)
        nx = np.trunc(np.where(ok, X, 0)).astype(np.int64)
        ny = np.trunc(np.where(ok, Y, 0)).astype(np.int64)
    ok &= (nx >= 0) & (nx < fw) & (ny >= 0) & (ny < fh)
    out = np.uint32(2 ** 32 - px)
    return np.where(ok, ((ny * fw + nx) * px) & 0xFFFFFFFF, out).astype(np.uint32)


def patch_counts(off, fw, fh, px=4):
    """-> ((bands, tiles) patches per tile, (bands, tiles) bool: some pixel of the tile has a sample)."""
    ch, cw = off.shape
    NR, NC = (ch + TS - 1) // TS, (cw + TS - 1) // TS
    out = 2 ** 32 - px
    o = np.full((NR * TS, NC * TS), out, dtype=np.int64)
    o[:ch, :cw] = off
    g = o.reshape(NR * TS, NC * TS // 4, 4)
    plane = fw * fh * px
    usable = (g[:, :, 0] != out) & (plane >= 16) & (g[:, :, 0] <= plane - 16)
    base = np.where(usable, g[:, :, 0], BASE_OUTSIDE)
    run = base[:, :, None] + np.arange(4)[None, None, :] * px
    patch = np.where(usable[:, :, None], g != run, g != out).reshape(NR * TS, NC * TS)
    tiles = lambda a: a.reshape(NR, TS, NC, TS).sum(axis=(1, 3))
    return tiles(patch.astype(np.int64)), tiles((o != out).astype(np.int64)) > 0


def classes(p, offx, offy, fw, fh, cw, ch, px=4):
    """-> ((outside, no patch, 1..64, general), (bands, tiles) uint8 classes) -- what stitch_src_run_classes reports."""
    n, live = patch_counts(offsets(p, offx, offy, fw, fh, cw, ch, px), fw, fh, px)
    cls = np.where((n > MAX_PATCHES) | (px != 4), GENERAL, n).astype(np.uint8)
    counts = (int((~live).sum()), int((live & (cls == 0)).sum()), int((live & (cls > 0) & (cls != GENERAL)).sum()), int((live & (cls == GENERAL)).sum()))
    return counts, cls
