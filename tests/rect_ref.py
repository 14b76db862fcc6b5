"""The CPU statement of the largest inscribed rectangle (include/stitch_rig_crop.h).  TEST INFRASTRUCTURE ONLY, shared by
tests/test_rect_host.py, tests/test_gpu_largest_rect.py and tests/test_gpu_rig_crop.py.

THE RULE, on a boolean mask (h, w): among the rectangles (x0, y0, w, h) whose pixels are all covered, the largest area; then the
smallest y0; then the smallest x0; then the largest w.  Nothing covered: (0, 0, 0, 0).

brute   every (y0, y1) pair of rows with a running AND of the rows between them, and every maximal run of the AND.  A rectangle of
        maximal area cannot be widened, so it is a maximal run of its rows' AND.  O(h^2 w): small masks only.
stack   per bottom row the up-heights and the linear stack algorithm; every popped bar is a candidate.  O(h w).
The two share the key and nothing else; tests/test_rect_host.py holds them to each other, and to hand answers.
"""
import numpy as np


def key(r):
    """Smaller is better: r = (x0, y0, w, h)."""
    x0, y0, w, h = r
    return (-w * h, y0, x0, -w)


def _runs(row):
    """The maximal runs of True in a 1-d bool array -> (start, length) pairs."""
    d = np.diff(np.concatenate(([0], row.astype(np.int8), [0])))
    starts, ends = np.flatnonzero(d == 1), np.flatnonzero(d == -1)
    return zip(starts.tolist(), (ends - starts).tolist())


def brute(mask):
    m = np.asarray(mask) != 0
    h, w = m.shape
    best = None
    for y0 in range(h):
        acc = np.ones(w, bool)
        for y1 in range(y0, h):
            acc &= m[y1]
            if not acc.any():
                break
            for x0, n in _runs(acc):
                r = (x0, y0, n, y1 - y0 + 1)
                if best is None or key(r) < key(best):
                    best = r
    return best or (0, 0, 0, 0)


def stack(mask):
    m = np.asarray(mask) != 0
    h, w = m.shape
    up = np.zeros(w, np.int64)
    best = None
    for y in range(h):
        up = np.where(m[y], up + 1, 0)
        if not up.any():
            continue
        st = []  # (start column, height), heights strictly ascending
        for x, v in enumerate(up.tolist() + [0]):
            start = x
            while st and st[-1][1] >= v:
                start, hv = st.pop()
                if hv > 0:
                    r = (start, y - hv + 1, x - start, hv)
                    if best is None or key(r) < key(best):
                        best = r
            st.append((start, v))
    return best or (0, 0, 0, 0)


# ---- the masks the tests share ----------------------------------------------------------------------------------------------------
def staircase(width, peak):
    """Heights 1, 2, .., k, .., 2, 1 over `width` columns, clipped at `peak` rows: column x is covered on its bottom min(x + 1,
    width - x, peak) rows."""
    hts = np.minimum(np.minimum(np.arange(width) + 1, width - np.arange(width)), peak)
    rows = int(hts.max())
    return (np.arange(rows)[::-1, None] < hts[None, :]).astype(np.uint8) * 255


def ascending(width, peak):
    """Heights strictly ascending up to `peak` rows, then level: column x is covered on its bottom min(x + 1, peak) rows."""
    hts = np.minimum(np.arange(width) + 1, peak)
    rows = int(hts.max())
    return (np.arange(rows)[::-1, None] < hts[None, :]).astype(np.uint8) * 255


def small_masks():
    """name -> (mask uint8 (h, w), the hand answer or None).  Small enough for brute."""
    out = {}
    out["ones"] = (np.full((7, 9), 255, np.uint8), (0, 0, 9, 7))
    out["zeros"] = (np.zeros((5, 6), np.uint8), (0, 0, 0, 0))
    for name, (y, x) in {"corner_tl": (0, 0), "corner_br": (4, 6)}.items():
        m = np.zeros((5, 7), np.uint8)
        m[y, x] = 255
        out[name] = (m, (x, y, 1, 1))
    out["1x1"] = (np.full((1, 1), 255, np.uint8), (0, 0, 1, 1))
    out["1x1_zero"] = (np.zeros((1, 1), np.uint8), (0, 0, 0, 0))
    m = np.full((1, 300), 255, np.uint8)
    m[0, 100] = 0
    out["row_300"] = (m, (101, 0, 199, 1))
    m = np.full((300, 1), 255, np.uint8)
    m[220, 0] = 0
    out["column_300"] = (m, (0, 0, 1, 220))
    m = np.zeros((6, 8), np.uint8)
    m[1:4, 2:7] = 1
    m[2, 3] = 128
    out["values_1_and_128"] = (m, (2, 1, 5, 3))
    # ties by y0: two 3 x 2 rectangles, the second one row lower and further left
    m = np.zeros((6, 12), np.uint8)
    m[1:3, 7:10] = 255
    m[2:4, 1:4] = 255
    out["tie_y0"] = (m, (7, 1, 3, 2))
    # ties by x0: the same rows
    m = np.zeros((5, 12), np.uint8)
    m[1:3, 7:10] = 255
    m[1:3, 2:5] = 255
    out["tie_x0"] = (m, (2, 1, 3, 2))
    # one top-left corner: a 6 x 2 and a 3 x 4 block, area 12 each; the wider wins
    m = np.zeros((7, 9), np.uint8)
    m[1:3, 2:8] = 255
    m[1:5, 2:5] = 255
    out["tie_corner"] = (m, (2, 1, 6, 2))
    out["staircase_9"] = (staircase(9, 5), None)
    out["staircase_67"] = (staircase(67, 34), None)
    out["ascending_20"] = (ascending(20, 20), None)
    return out


def random_masks():
    """(w, h, density, seed) -> mask, for the sizes, densities and seeds the GPU test uses; every answer has area >= 2 (asserted by
    the tests that use them)."""
    out = {}
    for w, h in ((67, 45), (130, 70), (257, 33), (1030, 9)):
        for density in (0.9, 0.99):
            for seed in (1, 2, 3):
                rng = np.random.default_rng([w, h, int(density * 100), seed])
                out[(w, h, density, seed)] = (rng.random((h, w)) < density).astype(np.uint8) * 255
    return out
