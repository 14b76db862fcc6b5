"""The host restatement of the G column flag rule (tests/g_flags_ref.py, flagged_in_level) on hand-made planes: what the GPU tests
compare Plan.g_flag_counts() with must itself be right."""
import numpy as np

from g_flags_ref import TS, flagged_in_level, tile_columns


def planes(n, h, w, data_tiles=()):
    """n planes of +0 with a non-zero sample in each of the given (plane, tile column)s."""
    g = np.zeros((n, h, w), np.float32)
    for q, t in data_tiles:
        g[q, h // 2, min(t * TS + 5, w - 1)] = 1.0
    return g


def test_neighbour_rule_and_the_edge_as_a_neighbour():
    # 8 tile columns from a parent of 16: data in column 3 takes columns 2, 3 and 4 away; 0, 1 and 5, 6, 7 stay, both edge columns included
    g = planes(1, 8, 512, [(0, 3)])
    for exc in (True, False):
        assert flagged_in_level(g, 1024, exc) == 5
    # data in the edge column takes its one neighbour with it
    assert flagged_in_level(planes(1, 8, 512, [(0, 0)]), 1024) == 6
    assert flagged_in_level(planes(1, 8, 512, [(0, 7)]), 1024) == 6
    # planes are counted one by one: a zero plane beside a full one
    assert flagged_in_level(planes(2, 8, 512, [(1, t) for t in range(8)]), 1024) == 8
    # two data columns two apart leave nothing between them
    assert flagged_in_level(planes(1, 8, 512, [(0, 2), (0, 4)]), 1024) == 8 - 5
    # a single tile column has two edges for neighbours
    assert flagged_in_level(planes(1, 4, 64), 128) == 1
    assert flagged_in_level(planes(1, 4, 64, [(0, 0)]), 128) == 0


def test_a_sample_in_any_row_counts():
    g = planes(1, 70, 256)
    g[0, 69, 64] = 3.0  # last row, first column of tile column 1
    assert flagged_in_level(g, 512) == 1  # column 3 alone
    g = planes(1, 70, 256)
    g[0, 0, 127] = 3.0  # first row, last column of tile column 1
    assert flagged_in_level(g, 512) == 1


def test_negative_zero_keeps_its_column_unflagged():
    g = planes(1, 8, 512)
    assert flagged_in_level(g, 1024) == 8
    g[0, 3, 200] = -0.0  # tile column 3: equal to zero as a number, not by bit pattern
    assert g[0, 3, 200] == 0.0
    assert flagged_in_level(g, 1024) == 5


def test_partial_last_tile():
    # 300 columns: 5 tile columns, the last of 44 columns; its parent (600 columns) has 10, so the exception plays no part
    assert tile_columns(300) == 5 and tile_columns(600) == 10
    for exc in (True, False):
        assert flagged_in_level(planes(1, 8, 300), 600, exc) == 5
        assert flagged_in_level(planes(1, 8, 300, [(0, 4)]), 600, exc) == 3  # a sample in the partial tile: columns 3 and 4 go
        g = planes(1, 8, 300)
        g[0, 0, 299] = 1.0  # the plane's very last sample
        assert flagged_in_level(g, 600, exc) == 3
        assert flagged_in_level(planes(1, 8, 300, [(0, 2)]), 600, exc) == 2  # columns 0 and 4


def test_odd_parent_width_gives_no_flags():
    for exc in (True, False):
        assert flagged_in_level(planes(6, 8, 255), 511, exc) == 0
        assert flagged_in_level(planes(6, 8, 256), 511, exc) == 0
        assert flagged_in_level(planes(6, 8, 256), 512, exc) == 24


def test_both_variants_on_a_nine_tile_parent():
    # parent 576 columns = 9 tile columns; the level has 288 = 5 (4.5).  The producer of tile column 4 reads the parent's columns 8 and 9,
    # and 9 does not exist: with the exception column 4 is neither flagged nor a zero neighbour, so column 3 goes as well
    assert tile_columns(576) == 9 and tile_columns(288) == 5
    z = planes(1, 8, 288)
    assert flagged_in_level(z, 576, False) == 5
    assert flagged_in_level(z, 576, True) == 3
    d = planes(1, 8, 288, [(0, 0)])  # data at the left edge: columns 0 and 1 go under either rule
    assert flagged_in_level(d, 576, False) == 3
    assert flagged_in_level(d, 576, True) == 1
    d = planes(1, 8, 288, [(0, 4)])  # data in the last column: the same columns go under either rule
    assert flagged_in_level(d, 576, False) == 3
    assert flagged_in_level(d, 576, True) == 3
    # a parent of 10 tile columns (640 wide, level of 320 = 5): no exception
    assert flagged_in_level(planes(1, 8, 320), 640, True) == 5
    # the 1088-wide canvas of the GPU test: 17 tile columns, level 1 has 9 (8.5): 7 of 9 per zero plane
    assert flagged_in_level(planes(2, 8, 544), 1088, True) == 14
    assert flagged_in_level(planes(2, 8, 544), 1088, False) == 18
