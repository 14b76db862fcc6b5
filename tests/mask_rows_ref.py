"""The rule of the row-repeat flags of the mask plane (csrc/k_compose.inc, mask_rows; include/stitch_mask_rows.h), restated on the
host.  A plain module: tests/test_gpu_mask_rows.py evaluates the rule on the mask the oracle's seam gives, blurred and decimated by
the oracle; tests/test_mask_rows_rule_host.py evaluates it on hand-made planes."""
import numpy as np

TS = 64


def step_row(seam, cw):
    """Row of the blend's level-0 mask under seam_rule 0 (ImageProcess.cpp:690-698): every row of the mask is this row."""
    x = np.arange(cw)
    if seam.branch == 0:
        return (x.astype(np.float64) < float(seam.ov)).astype(np.float32)
    return (x >= seam.start).astype(np.float32)


def repeat_prefix(tile):
    """Rows of `tile` (rows, columns; float32) in the longest prefix of rows that equal row 0 by bit pattern."""
    bits = np.ascontiguousarray(tile, dtype=np.float32).view(np.uint32)
    differs = np.flatnonzero((bits != bits[0]).any(axis=1))
    return int(differs[0]) if differs.size else bits.shape[0]


def flagged_in_plane(m, parent_w, parent_h):
    """Flagged (tile column, band) entries of the mask plane m (rows, columns; float32) of a level produced from a level of
    parent_w x parent_h.  Per 64-column tile column the longest prefix of rows equal to row 0 is taken; a 64-row band b >= 1 counts
    when all its existing rows lie in that prefix.  Band 0 never counts.  A level below an odd height or width counts nothing."""
    if (parent_w & 1) or (parent_h & 1):
        return 0
    m = np.ascontiguousarray(m, dtype=np.float32)
    h, w = m.shape
    count = 0
    for t in range((w + TS - 1) // TS):
        prefix = repeat_prefix(m[:, t * TS:(t + 1) * TS])
        count += sum(1 for b in range(1, (h + TS - 1) // TS) if min((b + 1) * TS, h) <= prefix)
    return count


def flagged_entries(oracle, seam, cw, ch, level_rule, levels=2):
    """[count at level 1, count at level 2] under the rule, from the step of the oracle's seam blurred and decimated by the oracle.
    A level below a level of odd width or height counts nothing, and neither does any level below that one: its producer reads the
    blur of a mask plane whose tiles are all stored, and records nothing."""
    g = np.ascontiguousarray(np.broadcast_to(step_row(seam, cw), (1, ch, cw)), dtype=np.float32)
    _, lw, lh = oracle.pyramid_levels(cw, ch, level_rule)
    counts, even = [], True
    for lv in range(1, levels + 1):
        pw, ph = g.shape[2], g.shape[1]
        even = even and not (pw & 1) and not (ph & 1)
        g = oracle.decimate(oracle.blur(g), lw[lv], lh[lv])
        counts.append(flagged_in_plane(g[0], pw, ph) if even else 0)
    return counts
