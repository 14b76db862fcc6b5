"""Shared by tests/test_collapse_sides_host.py and tests/test_gpu_collapse_sides.py: the rule by which a 256-column block of the level-0
collapse reads one image or both (csrc/stitch_call_form.h, c4_block_side), restated in Python, and the four integers of a seam whose
step lies at a wanted column.  TEST INFRASTRUCTURE ONLY.  A plain module."""
import numpy as np

import rig_seams_ref as ref


def step_at(branch, start, thr, x):
    """mask_step: branch 0: 1 where (double)x < thr, branch 1: 1 where x >= start."""
    return int(float(x) < thr) if branch == 0 else int(x >= start)


def side_counts(branch, start, thr, xa, xb, sides=True):
    """(a-only, b-only, both) blocks of columns [xa, xb), block b = columns xa + 256 b .. min(that + 255, xb - 1)."""
    n = [0, 0, 0]
    for xf in range(xa, xb, 256):
        first, last = step_at(branch, start, thr, xf), step_at(branch, start, thr, min(xf + 255, xb - 1))
        n[2 if (first != last or not sides) else (0 if first else 1)] += 1
    return tuple(n)


def seam_for(branch, t, cw):
    """Four integers (stitch_dev_pairs_seamed_*) of a seam under rule 0 whose mask is 1 on columns x < t (branch 0, 1 <= t <= cw - 1)
    or on columns x >= t (branch 1, 1 <= t <= cw): the overlap is the one column c with ov = c; a's middle row is columns {0, c}
    (ratio = c / 2 < ov) for branch 0 and the same one column (ratio = ov) for branch 1.  No four integers give a step at column 0:
    ov >= 0 makes ratio < ov impossible there, and branch 1 starts at int(ov + 1) >= 1."""
    if branch == 0:
        assert 1 <= t <= cw - 1
        four = (t, 2, t, 1)
    else:
        assert 1 <= t <= cw
        four = (t - 1, 1, t - 1, 1)
    b, start, thr = ref.derive(four, 0)
    assert b == branch and (thr == float(t) if branch == 0 else start == t), (branch, t, four, b, start, thr)
    return four


def counts_of(four, seam_rule, xa, xb):
    """The rule on the oracle's record of the four integers."""
    branch, start, thr = ref.derive(four, seam_rule)
    return side_counts(branch, start, thr, xa, xb)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint8)
