"""The rule of the row-repeat flags of the mask plane (tests/mask_rows_ref.py) on hand-made planes: no GPU, no oracle."""
import numpy as np

from mask_rows_ref import TS, flagged_in_plane, repeat_prefix


def plane(h, w, seed=0):
    """Every row the same random row."""
    row = np.random.default_rng(seed).random(w, dtype=np.float32)
    return np.ascontiguousarray(np.broadcast_to(row, (h, w)))


def test_a_plane_of_equal_rows_is_flagged_below_its_first_band():
    assert flagged_in_plane(plane(256, 192), 384, 512) == 3 * 3  # three tile columns, bands 1..3


def test_a_deviation_in_the_last_row_costs_its_band_only():
    m = plane(256, 192)
    m[255, 70] += 1.0  # tile column 1, band 3
    assert repeat_prefix(m[:, 64:128]) == 255
    assert flagged_in_plane(m, 384, 512) == 9 - 1


def test_a_deviation_in_the_middle_of_a_band_costs_that_band_and_those_below():
    m = plane(256, 192)
    m[100, 130] += 1.0  # tile column 2, band 1: bands 1, 2, 3 of that column go
    assert flagged_in_plane(m, 384, 512) == 9 - 3
    n = plane(256, 192)
    n[64 + 127, 5] += 1.0  # the last row of band 2 in tile column 0: bands 2 and 3 go, band 1 stays
    assert flagged_in_plane(n, 384, 512) == 9 - 2


def test_a_deviation_in_row_1_leaves_nothing_of_its_column():
    m = plane(256, 192)
    m[1, 0] += 1.0
    assert repeat_prefix(m[:, :64]) == 1
    assert flagged_in_plane(m, 384, 512) == 9 - 3


def test_rows_that_agree_again_further_down_do_not_count():
    m = plane(256, 64)
    m[70] += 1.0  # rows 71.. equal row 0 again, but they are not in the prefix
    assert flagged_in_plane(m, 128, 512) == 0


def test_the_comparison_is_on_the_bit_pattern():
    m = np.zeros((128, 64), np.float32)
    assert flagged_in_plane(m, 128, 256) == 1
    m[127, 3] = -0.0
    assert flagged_in_plane(m, 128, 256) == 0


def test_a_zero_column_is_a_row_repeat_like_any_other():
    m = plane(192, 128)
    m[:, 64:] = 0.0
    assert flagged_in_plane(m, 256, 384) == 2 * 2


def test_a_ragged_last_band_counts_by_its_existing_rows():
    m = plane(98, 272)  # five tile columns, the last of 16 columns; band 1 has rows 64..97
    assert flagged_in_plane(m, 544, 196) == 5
    m[97, 271] += 1.0
    assert flagged_in_plane(m, 544, 196) == 4
    assert flagged_in_plane(plane(TS, 272), 544, 128) == 0  # one band: band 0 is never flagged


def test_below_an_odd_height_or_width_nothing_counts():
    m = plane(256, 192)
    assert flagged_in_plane(m, 384, 513) == 0
    assert flagged_in_plane(m, 385, 512) == 0
