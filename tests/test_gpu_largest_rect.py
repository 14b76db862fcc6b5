"""GPU: stitch_dev_largest_rect_u8 (include/stitch_rig_crop.h, csrc/k_rig_crop.inc) against tests/rect_ref.py -- the four integers
equal.  The brute force where it is quick, the stack form (held to it by tests/test_rect_host.py) elsewhere.

The shapes are the smallest at which the search can go wrong: widths around the hierarchy's groups of 4, the 64 lanes of a
wavefront and the 256 of a workgroup; staircases, on which a search that walks outward is quadratic; a column taller than 65 535
(heights in 32 bits); and a row of 30 011 columns, too wide for the 64 KB of LDS a row's hierarchy may take with 16-bit heights, so
it runs on the hierarchy in device memory.  (That form with 32-bit heights needs a mask of 12 000 x 65 536 and has no case here:
it is the same kernel template with the other pointer.)"""
import numpy as np
import pytest

import rect_ref as ref
from computervisionimagestich2_amd import capi

pytestmark = pytest.mark.gpu

_want = {}


def _reference(name, mask, brute=False):
    """Computed once per mask and left unchanged."""
    if name not in _want:
        _want[name] = ref.brute(mask) if brute else ref.stack(mask)
    return _want[name]


def _search(gpu, mask):
    import torch
    return capi.dev_largest_rect(torch.from_numpy(np.ascontiguousarray(mask)).to(gpu))


@pytest.mark.parametrize("name", sorted(ref.small_masks()))
def test_small_masks(st, gpu, name):
    """All ones, all zero, one covered pixel in a corner, 1 x 1, 1 x 300, 300 x 1, covered bytes of 1 and 128, and the three ties."""
    mask, want = ref.small_masks()[name]
    if want is None:
        want = _reference(name, mask, brute=True)
    assert _search(gpu, mask) == want
    if name == "zeros":
        assert want == (0, 0, 0, 0)


def test_tie_masks_do_have_ties(st):
    """Each tie mask holds two rectangles of the winning area, and the answer is the one the order names."""
    M = ref.small_masks()
    for name, other in (("tie_y0", (1, 2, 3, 2)), ("tie_x0", (7, 1, 3, 2)), ("tie_corner", (2, 1, 3, 4))):
        mask, want = M[name]
        x0, y0, w, h = other
        assert (mask[y0:y0 + h, x0:x0 + w] != 0).all() and w * h == want[2] * want[3] and ref.key(want) < ref.key(other)


STAIRS = [(67, 34), (257, 129), (1030, 515), (4099, 5)]


@pytest.mark.parametrize("shape", ["staircase", "ascending"])
@pytest.mark.parametrize("width,peak", STAIRS)
def test_staircases(st, gpu, shape, width, peak):
    """Heights 1, 2 .. k .. 2, 1 and heights strictly ascending: every lane's span ends at another distance."""
    if shape == "ascending" and peak != 5:
        peak = width
    mask = getattr(ref, shape)(width, peak)
    assert mask.shape == (peak, width)
    assert _search(gpu, mask) == _reference((shape, width), mask)


@pytest.mark.parametrize("zero_row", [None, 65536])
def test_a_column_taller_than_16_bits(st, gpu, zero_row):
    """3 x 70000, all covered: heights reach 70 000 and must not wrap; with a zero row at 65 536 the part above it wins."""
    mask = np.full((70000, 3), 255, np.uint8)
    if zero_row is not None:
        mask[zero_row] = 0
    want = (0, 0, 3, 70000 if zero_row is None else zero_row)
    assert _reference(("column", zero_row), mask) == want
    assert _search(gpu, mask) == want


def test_a_row_too_wide_for_lds(st, gpu):
    """30 011 columns of 16-bit heights: the hierarchy of a row is 80 KB and lives in device memory.  Heights 1 .. 3 in runs that
    cross every group boundary, with holes."""
    w, h = 30011, 3
    rng = np.random.default_rng(7)
    hts = np.repeat(rng.integers(1, h + 1, w // 37 + 1), 37)[:w]
    mask = (np.arange(h)[::-1, None] < hts[None, :]).astype(np.uint8) * 255
    mask[:, rng.integers(0, w, 40)] = 0
    want = _reference("wide", mask)
    assert want[2] * want[3] >= 2
    assert _search(gpu, mask) == want


@pytest.mark.parametrize("key", sorted(ref.random_masks()), ids=lambda k: f"{k[0]}x{k[1]}_d{int(k[2] * 100)}_s{k[3]}")
def test_random_masks(st, gpu, key):
    mask = ref.random_masks()[key]
    want = _reference(key, mask)
    assert want[2] * want[3] >= 2, "a degenerate draw"
    assert _search(gpu, mask) == want


def test_the_mask_is_only_read_and_the_call_waits(st, gpu):
    """The call returns host integers, so it has waited for its stream: a mask changed right after it does not change the answer."""
    import torch
    mask = torch.full((33, 130), 255, dtype=torch.uint8, device=gpu)
    mask[:, 100] = 0
    before = mask.clone()
    mine = torch.cuda.Stream()
    mine.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(mine):
        got = capi.dev_largest_rect(mask)
        assert bool((mask == before).all())
        mask.zero_()
        assert capi.dev_largest_rect(mask) == (0, 0, 0, 0)
    assert got == (0, 0, 100, 33)
    with pytest.raises(ValueError):
        capi.dev_largest_rect(before[:, ::2])
