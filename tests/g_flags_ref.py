"""The rule of the G column flags (csrc/k_compose.inc, g_cols), restated on the host, and the inputs the G-flag tests share: narrow
images at one edge of a canvas, whose planes are +0 over the rest of every level.  A plain module: tests/test_gpu_g_flags.py and
tests/test_gpu_g_flags_readers.py evaluate the rule on the oracle's planes, tests/test_g_flags_rule_host.py on hand-made ones."""
import numpy as np

TS = 64
# the pyramid's depth from the SHORTER side: under the root rule canvases this flat have no valid pyramid, and the oracle refuses them
OPTS = dict(sigma=2.0, blur_kind=0, level_rule=1, seam_rule=0)
WARP = [1.0, 0.002, 1e-6, 0.0, -0.001, 1.0, 5e-7, 1.5]


def shift(x0, P=None):
    """Canvas -> frame map of a frame whose left edge lies at canvas column x0 (P: a slightly projective map instead of the shift)."""
    P = list(P) if P else [1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0]
    P[3] = -float(x0)
    return P


def cases(cw):
    """name -> (frame width, map, mosaic width, mosaic ox, seam branch).  A narrow image at one edge of the canvas: its three planes
    are +0 over the rest of every level -- further in than the blur's tails reach -- while the other image covers nearly everything."""
    return {
        "frame_right": (64, shift(cw - 64, WARP), cw - 34, 0, 1),
        "frame_left": (64, shift(0), cw - 40, -40, 0),
        "mosaic_left": (cw - 40, shift(40), 60, 0, 1),
        "mosaic_right": (cw - 40, shift(0), 60, -(cw - 60), 0),
    }


# the second batch has every zero region where the first had data: a tile column stored by call 1 is flagged -- and stale -- in call 2
BATCHES = [("frame_right", "mosaic_left"), ("frame_left", "mosaic_right")]
# the two ways level 2 reaches the sweep that reads the flags: as a third fused level (with flags of the blur scratch), and unfused
# behind two fused levels as in a large batch (a batch this small would otherwise take the three-wavefront x sweep, which has no flags)
FORMS = {"fused3": {"STITCH_WAVEFRONT": "3"}, "fused2": {"STITCH_WAVEFRONT": "2", "STITCH_MOVER": "0"}}


def tile_columns(w):
    return (w + TS - 1) // TS


def flagged_in_level(g, parent_w, ragged_exception=True, parent_blurred=None):
    """Flagged tile columns of the planes g (planes, rows, columns; float32) of a level produced from a level parent_w wide.
    A 64-column tile column counts when it is +0 by bit pattern in every row and so are both neighbouring tile columns; the plane's
    edge counts as a zero neighbour.  A level produced from an odd width has no flags.
    ragged_exception: the producer's workgroup of tile column t reads the parent's tile columns 2t and 2t + 1, and where the second
    lies past the parent's last tile column (an odd count of them) it neither takes its all-zero path nor is it taken for a zero
    neighbour: t can count as zero, for itself and as a neighbour, only if 2t + 1 < ceil(parent_w / 64).  So the last tile column of
    such a level and the one before it are never flagged.  False: the rule without that exception.
    parent_blurred: the blurred planes of the level above, before the decimation.  The producer takes its all-zero path from what it
    READS -- the blurred tile columns 2t and 2t + 1 of the level above, +0 throughout -- not from what it writes: where the blur's
    tail ends on an odd column, which the decimation drops, the tile column of G is +0 in every sample and still stored as data.
    Given the planes, t counts as zero only if those 128 columns are +0 as well."""
    g = np.ascontiguousarray(g, dtype=np.float32)
    if parent_w & 1:
        return 0
    nc = tile_columns(g.shape[2])
    zero = np.array([[not g[q, :, t * TS:(t + 1) * TS].view(np.uint32).any() for t in range(nc)] for q in range(g.shape[0])]).reshape(g.shape[0], nc)
    if parent_blurred is not None:
        pb = np.ascontiguousarray(parent_blurred, dtype=np.float32)
        zero &= np.array([[not pb[q, :, 2 * t * TS:(2 * t + 2) * TS].view(np.uint32).any() for t in range(nc)] for q in range(g.shape[0])]).reshape(g.shape[0], nc)
    if ragged_exception:
        zero &= (2 * np.arange(nc) + 1 < tile_columns(parent_w))[None, :]
    pad = np.pad(zero, ((0, 0), (1, 1)), constant_values=True)
    return int((pad[:, :-2] & pad[:, 1:-1] & pad[:, 2:]).sum())


def flagged_columns(oracle, a, b, levels=2, ragged_exception=True):
    """[count at level 1, count at level 2] under the rule (flagged_in_level, with the blurred planes of the level above: what the
    producer reads), from the oracle's planes of the canvases a and b."""
    g = np.concatenate([a, b]).astype(np.float32)
    _, lw, lh = oracle.pyramid_levels(g.shape[2], g.shape[1], OPTS["level_rule"])
    counts = []
    for lv in range(1, levels + 1):
        parent_w = g.shape[2]
        blurred = oracle.blur(g)
        g = oracle.decimate(blurred, lw[lv], lh[lv])
        counts.append(flagged_in_level(g, parent_w, ragged_exception, blurred))
    return counts
