"""numpy restatement of ImageProcess::getImgPair (ImageProcess.cpp:273-351) as an exact search: the L1 distance of VLFeat's
plain C _vl_distance_l1_f (vl/mathop.c:307-318) -- acc = 0.0f; for k = 0..127: acc += |q[k] - x[k]| in float32, in that
order -- for every (query, data) pair, the two smallest distances, the lowest index among equal nearest distances, and the
ratio test `(float)(d0 / d1) < ratio` (RATIO_THRESHOLD 0.5, ImageProcess.h:22).  Vectorised over pairs, sequential over k.
"""
import numpy as np

DIM = 128


def l1_distances(query, db, block=1 << 22):
    """(n_query, n_db) float32 distances, each the sequential fp32 sum over k = 0..127."""
    q = np.ascontiguousarray(query, np.float32)
    x = np.ascontiguousarray(db, np.float32)
    out = np.empty((len(q), len(x)), np.float32)
    rows = max(1, block // max(len(x), 1))
    for r0 in range(0, len(q), rows):
        qq = q[r0:r0 + rows]
        acc = np.zeros((len(qq), len(x)), np.float32)
        for k in range(DIM):
            acc += np.abs(qq[:, None, k] - x[None, :, k])
        out[r0:r0 + rows] = acc
    return out


def match(db, query, ratio=0.5):
    """(pairs, nn, d0, d1) as capi.match returns them."""
    db = np.asarray(db, np.float32).reshape(-1, DIM)
    query = np.asarray(query, np.float32).reshape(-1, DIM)
    nq, nd = len(query), len(db)
    nn = np.full(nq, -1, np.int32)
    d0 = np.full(nq, np.nan, np.float32)
    d1 = np.full(nq, np.nan, np.float32)
    if nq and nd:
        D = l1_distances(query, db)
        nn[:] = np.argmin(D, axis=1)  # first occurrence: the lowest index among equal distances
        d0[:] = D[np.arange(nq), nn]
        if nd > 1:
            d1[:] = np.partition(D, 1, axis=1)[:, 1]
    with np.errstate(divide="ignore", invalid="ignore"):
        r = d0 / d1  # float32 quotient (the double quotient rounded to float is the same value)
        ok = r.astype(np.float64) < ratio
    q_idx = np.nonzero(ok)[0].astype(np.int32)
    pairs = np.stack([nn[q_idx], q_idx], axis=1).astype(np.int32).reshape(-1, 2)
    return pairs, nn, d0, d1
