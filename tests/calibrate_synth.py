"""Synthetic feature sets for the calibration from several captures (include/stitch_calibrate.h): descriptors and key points
whose match counts are known by construction, so that a test can choose the branch of csrc/k_calibrate.inc and
csrc/stitch_calibrate.inc it reaches.  TEST INFRASTRUCTURE ONLY, shared by tests/test_calibrate_synth_host.py (which proves every
claim below on the CPU) and tests/test_gpu_calibrate_synth.py.  Arrays are generated, never committed.

The recipe, for one capture and one pair of neighbouring cameras A (the lower index) and B that share `m` world points:
  * a world descriptor is rng.integers(1, 8, 128) / 8 with about 80 % of its components set to 0; the world rows are sorted
    lexicographically, so world point r is the r-th of them in either camera;
  * A holds the world rows with components 0 and 1 raised by 0.01 and, for the FIRST `ta` world points, a near-twin (components
    0, 1 and 2 raised by 0.01, coordinates + 0.25); B holds the world rows unchanged and, for the LAST `tb` world points, a
    near-twin (component 3 raised by 0.01, coordinates + 0.25); a camera also holds `extras` unrelated rows;
  * a twin on the data side makes d0 / d1 = 0.02 / 0.03, which the ratio test (0.5) rejects; a twin on the query side is one more
    accepted query.  So getImgPair(A, B) accepts m - ta + tb queries and getImgPair(B, A) accepts m + ta - tb
    (expected_counts); with m == ta and tb == 0 these are 0 and 2 m.  A camera that is searched needs two rows at least (with
    one row there is no second neighbour and nothing is accepted);
  * the rows of a camera are sorted lexicographically together with x and y: the std::map order, pipeline.feature_order is the
    identity on them;
  * A's points are uniform in A's frame, B's points are the fixed projective map chain_map(A's index) of them.  A share
    `outliers` of the world points gets unrelated B coordinates (edges="in": never the first or last world point, edges="out":
    always both).  In a `moved` capture B's points follow another map;
  * three or more cameras are a chain 0 - 1 - 2 (- 3): each neighbouring pair shares world points of its own, other cameras share
    none, so their counts are 0.
The formula was observed, not proven for every draw: tests/test_calibrate_synth_host.py is its proof for every case here."""
import numpy as np

DIM = 128
F = np.float32
EPS = F(0.01)
TWIN_SHIFT = F(0.25)


def pair(m, ta=0, tb=0, outliers=0.0, moved=False, edges=None):
    return dict(m=m, ta=ta, tb=tb, outliers=outliers, moved=moved, edges=edges)


def cap(pairs, extras):
    """One capture: the spec of every neighbouring pair (c, c + 1) and the unrelated rows per camera."""
    assert len(extras) == len(pairs) + 1
    return dict(pairs=list(pairs), extras=list(extras))


def _sixty_four():
    return [cap([pair(20 + 7 * k % 11, k % 3, k // 3 % 3, 0.1), pair(20 + (5 * k + 3) % 11, k // 2 % 3, k // 5 % 3, 0.1)], [k % 4, k // 4 % 3, (k + 1) % 5])
            for k in range(64)]


_FULL = [cap([pair(4096)], [0, 0]) for _ in range(16)]

# name -> seed, frame sizes (width, height) per camera, captures.  With 2 cameras the order is [(1, 0)]: the step's sd list is
# getImgPair(1, 0) = m + ta - tb, its ds list getImgPair(0, 1) = m - ta + tb.  With 3 it is [(1, 2), (1, 0)], with 4
# [(2, 3), (2, 1), (1, 0)].  "claims" is what the host test asserts of the CPU reference's result.
CASES = {
    # step (1, 2): pooled sd 76 > ds 68, capture 0 alone 18 < 26.  Step (1, 0): pooled sd 63 < ds 73, capture 0 alone 25 > 15.
    # Rows per camera and capture: 28 48 26 / 27 55 33 / 23 57 32, all different, so every base differs from every other.
    "rule_flips": dict(seed=101, sizes=[(160, 120), (144, 128), (168, 112)], captures=[
        cap([pair(20, 5, 0, 0.15), pair(22, 4, 0, 0.15)], [3, 2, 4]),
        cap([pair(25, 0, 4, 0.15), pair(26, 0, 5, 0.15)], [2, 0, 2]),
        cap([pair(23, 0, 6, 0.15), pair(24, 0, 3, 0.15)], [0, 4, 5])],
        claims=dict(steps=2, rows_differ=True, rule={0: ("sd", 0, "ds"), 1: ("ds", 0, "sd")})),
    # sd = 36 + 26 + 22 = 84 = 24 + 30 + 30 = ds: the else of the strict >, and no capture is tied
    "tie_on_totals": dict(seed=102, sizes=[(160, 120), (160, 120)], captures=[
        cap([pair(30, 6, 0, 0.1)], [2, 1]), cap([pair(28, 0, 2, 0.1)], [0, 3]), cap([pair(26, 0, 4, 0.1)], [4, 2])],
        claims=dict(steps=1, tie=[0])),
    # the chosen list is ds (127 > 97) with 0 pairs in captures 0, 2 and 4: captures 0 and 4 are m == ta (ds 0, sd 2 m), capture 2
    # has no shared point and camera 0 no row at all
    "empty_segments": dict(seed=103, sizes=[(160, 120), (152, 120)], captures=[
        cap([pair(8, 8, 0)], [2, 3]), cap([pair(50, 0, 15, 0.1)], [1, 2]), cap([pair(0)], [0, 4]), cap([pair(48, 0, 14, 0.1)], [3, 0]),
        cap([pair(6, 6, 0)], [2, 2])],
        claims=dict(steps=1, rule={0: ("ds", 0, "sd")}, empty={0: [0, 2, 4]}, other_direction={0: [0, 4]}, no_rows=[(2, 0)])),
    # capture 2's camera 1 follows another map: 28 pairs, no support.  sd (126 > 122) lists camera 0's queries in world order, so
    # capture 0's first and last pair are inliers and capture 1's are outliers
    "moved_capture": dict(seed=104, sizes=[(160, 120), (160, 120)], captures=[
        cap([pair(30, 0, 0, 0.2, edges="in")], [2, 3]), cap([pair(32, 0, 0, 0.2, edges="out")], [1, 0]), cap([pair(28, moved=True)], [0, 2]),
        cap([pair(34, 2, 0, 0.15)], [3, 1])],
        claims=dict(steps=1, rule={0: ("sd", None, None)}, moved=2, edges_in=0, edges_out=1)),
    # STITCH_CALIBRATE_MAX_SETS captures: the LDS arrays, the tid <= n_sets store, all 64 lanes of k_step_support
    "sixty_four_captures": dict(seed=105, sizes=[(160, 120), (144, 128), (168, 112)], captures=_sixty_four(), claims=dict(steps=2)),
    # three steps: the bases and the shift of the camera warped before are followed to step (1, 0), whose src was step 2's dst
    "four_camera_chain": dict(seed=106, sizes=[(160, 120), (144, 128), (168, 112), (152, 120)], captures=[
        cap([pair(22, 3, 0, 0.1), pair(24, 0, 4, 0.1), pair(21, 2, 0, 0.1)], [2, 1, 0, 3]),
        cap([pair(25, 0, 2, 0.1), pair(20, 5, 0, 0.1), pair(26, 0, 3, 0.1)], [0, 3, 2, 1]),
        cap([pair(23, 1, 0, 0.1), pair(27, 0, 1, 0.1), pair(24, 0, 5, 0.1)], [4, 0, 1, 2])],
        claims=dict(steps=3, rows_differ=True)),
    # a pooled list of exactly STITCH_CALIBRATE_MAX_PAIRS = 16 * 4096 pairs, and one pair more (the 17th capture's cameras hold
    # three unrelated rows each: a search among fewer than two rows accepts nothing).  Device only: see the GPU test.
    "capacity_exact": dict(seed=107, sizes=[(640, 480), (640, 480)], captures=_FULL, claims=None),
    "capacity_exceeded": dict(seed=107, sizes=[(640, 480), (640, 480)], captures=_FULL + [cap([pair(1)], [3, 3])], claims=None),
}
SMALL = [name for name, c in CASES.items() if c["claims"] is not None]


def chain_map(c, moved=False):
    """The projective map from camera c's frame to camera c + 1's: (a, b, tx, d, e, ty, g, h),
    x' = (a x + b y + tx) / (1 + g x + h y), y' = (d x + e y + ty) / (1 + g x + h y).  Mild: within a frame it stays well inside
    RANSAC's 4 pixels of the bilinear model that is estimated."""
    a, b, tx, d, e, ty = 1.02 - 0.01 * c, 0.03, -70.0 - 5 * c, -0.02, 0.98 + 0.01 * c, -14.0 + 12 * c
    if moved:
        a, e, tx, ty = a * 0.9, e * 1.1, tx + 40, ty - 30
    return a, b, tx, d, e, ty, 2e-5, -1e-5


def apply_map(M, x, y):
    a, b, tx, d, e, ty, g, h = M
    x, y = x.astype(np.float64), y.astype(np.float64)
    w = 1 + g * x + h * y
    return ((a * x + b * y + tx) / w).astype(F), ((d * x + e * y + ty) / w).astype(F)


def _rows(rng, m):
    w = (rng.integers(1, 8, (m, DIM)) / 8).astype(F)
    w[rng.random((m, DIM)) < 0.8] = 0
    return w[np.lexsort(w.T[::-1])] if m else w


def _capture(rng, sizes, spec):
    n = len(sizes)
    desc, xs, ys = [[] for _ in range(n)], [[] for _ in range(n)], [[] for _ in range(n)]

    def put(c, d, x, y):
        desc[c].append(d)
        xs[c].append(x)
        ys[c].append(y)

    for c, p in enumerate(spec["pairs"]):
        m, ta, tb = p["m"], p["ta"], p["tb"]
        assert ta + tb <= m
        w = _rows(rng, m)
        xa, ya = (rng.random(m) * sizes[c][0]).astype(F), (rng.random(m) * sizes[c][1]).astype(F)
        xb, yb = apply_map(chain_map(c, p["moved"]), xa, ya)
        n_out = int(round(p["outliers"] * m))
        if n_out:
            inner = rng.permutation(np.arange(1, m - 1))
            out = np.concatenate([[0, m - 1], inner[:n_out - 2]]) if p["edges"] == "out" else inner[:n_out] if p["edges"] == "in" else rng.permutation(m)[:n_out]
            xb[out], yb[out] = (rng.random(len(out)) * sizes[c + 1][0]).astype(F), (rng.random(len(out)) * sizes[c + 1][1]).astype(F)
        a = w.copy()
        a[:, :2] += EPS
        put(c, a, xa, ya)
        t = w[:ta].copy()
        t[:, :3] += EPS
        put(c, t, xa[:ta] + TWIN_SHIFT, ya[:ta] + TWIN_SHIFT)
        put(c + 1, w, xb, yb)
        t = w[m - tb:].copy()
        t[:, 3] += EPS
        put(c + 1, t, xb[m - tb:] + TWIN_SHIFT, yb[m - tb:] + TWIN_SHIFT)
    for c, e in enumerate(spec["extras"]):
        put(c, _rows(rng, e), (rng.random(e) * sizes[c][0]).astype(F), (rng.random(e) * sizes[c][1]).astype(F))
    feats = []
    for c in range(n):
        d, x, y = np.concatenate(desc[c]), np.concatenate(xs[c]), np.concatenate(ys[c])
        o = np.lexsort(d.T[::-1])
        f = tuple(np.ascontiguousarray(v[o], F) for v in (d, x, y))
        for v in f:
            v.setflags(write=False)
        feats.append(f)
    return feats


_cache = {}


def features(name):
    """(frame sizes, [[(descriptors (rows, 128), x, y) per camera] per capture]) of a case: float32, read-only, cached.  Capture k
    is drawn from default_rng([seed, k]) alone, so the two capacity cases share their first 16 captures."""
    case = CASES[name]
    feats = []
    for k, spec in enumerate(case["captures"]):
        key = (case["seed"], k, repr(spec), tuple(case["sizes"]))
        if key not in _cache:
            _cache[key] = _capture(np.random.default_rng([case["seed"], k]), case["sizes"], spec)
        feats.append(_cache[key])
    return list(case["sizes"]), feats


def expected_counts(name):
    """(n_sets, n, n) int32: the formula of the recipe."""
    case = CASES[name]
    n = len(case["sizes"])
    out = np.zeros((len(case["captures"]), n, n), np.int32)
    for k, spec in enumerate(case["captures"]):
        for c, p in enumerate(spec["pairs"]):
            out[k, c, c + 1] = p["m"] - p["ta"] + p["tb"]
            out[k, c + 1, c] = p["m"] + p["ta"] - p["tb"]
    return out


def expected_rows(name):
    """(n_sets, n): the rows per capture and camera."""
    case = CASES[name]
    out = np.array([spec["extras"] for spec in case["captures"]], np.int64)
    for k, spec in enumerate(case["captures"]):
        for c, p in enumerate(spec["pairs"]):
            out[k, c] += p["m"] + p["ta"]
            out[k, c + 1] += p["m"] + p["tb"]
    return out
