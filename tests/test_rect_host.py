"""CPU: the two statements of the largest inscribed rectangle in tests/rect_ref.py -- the brute force over row pairs and the stack
algorithm per bottom row -- agree on every small mask the GPU tests use, on exhaustive tiny masks, and give the hand answers."""
import itertools

import numpy as np
import pytest

import rect_ref as ref


@pytest.mark.parametrize("name", sorted(ref.small_masks()))
def test_small_masks(name):
    mask, want = ref.small_masks()[name]
    b, s = ref.brute(mask), ref.stack(mask)
    assert b == s
    if want is not None:
        assert b == want
    x0, y0, w, h = b
    if w:
        assert (mask[y0:y0 + h, x0:x0 + w] != 0).all()


def test_every_3x4_mask():
    for bits in itertools.product((0, 1), repeat=12):
        m = np.array(bits, np.uint8).reshape(3, 4)
        assert ref.brute(m) == ref.stack(m), m


def test_random_masks_agree_and_are_not_degenerate():
    for k, m in ref.random_masks().items():
        if m.shape[0] * m.shape[0] * m.shape[1] > 1_000_000:  # the brute force on the smaller ones
            continue
        b = ref.brute(m)
        assert b == ref.stack(m), k
        assert b[2] * b[3] >= 2, k


def test_staircases_have_the_expected_areas():
    # heights 1 .. k .. 1 over 2k - 1 columns: a rectangle of height v spans 2k - 1 - 2(v - 1) columns
    m = ref.staircase(67, 34)
    best = max(v * (67 - 2 * (v - 1)) for v in range(1, 35))
    r = ref.stack(m)
    assert r[2] * r[3] == best and r == ref.brute(m)
    m = ref.ascending(20, 20)
    r = ref.stack(m)
    assert r[2] * r[3] == max(v * (20 - v + 1) for v in range(1, 21)) and r == ref.brute(m)
    assert ref.staircase(4099, 5).shape == (5, 4099) and ref.stack(ref.staircase(4099, 5)) == (4, 0, 4091, 5)
