"""Hand-made rigs whose canvases sit at the edges of the 64-bit words of the coverage bit planes, and the table of option combinations of
the rig replay.  TEST INFRASTRUCTURE ONLY, host only: nothing here needs a device.  Shared by tests/test_rig_edges_host.py,
tests/test_gpu_rig_word_edges.py and tests/test_gpu_rig_lattice.py.

RIGS      name -> (the size of each of the three frames, the moves as (frame, shift(...) arguments), the canvases the steps must get).
          The bit planes' readers index 64-bit words (wpr per row, tail = cw & 63 bits in the last one):
          w64_65     wpr == 1 with tail == 0 (no neighbour word on either side), then a last word of ONE bit
          w63_64     a last word of 63 bits, then a full one
          w64_twice  both steps on one 64 x 33 canvas: one workspace, one set of planes' sizes
          w128_129   two full words, then a third of one bit; the (72, 64) frames' own planes have an 8-bit tail
          w128_192   three full words; step 1's residual domain at radius 8 is ONE pixel
          odd_h      frames of odd height and a width that is a multiple of 4: NV12 with a clamped last chroma row.  At tight pitches
                     and aligned bases (the fixed row of tests/test_gpu_rig_lattice.py) the projection stages such frames itself; the
                     `nv12_mixed` level of the table below takes the unpack fallback
          w65_left_cut  w64_65 whose last step samples three columns further left than its canvas was made for (a third entry of the
                     move: the shift of the BACKWARD map), so the canvas's left border cuts the footprint.  The projection leaves
                     column 0 of a frame uncovered but for one pixel, so in every other rig no pixel of a domain lies within the radius
                     of the left border, and what the erosion takes the missing word before word 0 for decides nothing; here it does.
          w65_right_cut, w63_right_cut  likewise on the right, where the mosaic reaches the border too: the domains have pixels within
                     the radius of a right border that lies in a last word of 1 bit and of 63 bits, so the ones that the erosion reads
                     behind the width decide pixels.  (In the rigs above only the bottom border does.)
covering_rows  a deterministic greedy covering array over the option levels below: every pair (strength 2) or triple (strength 3) of
          levels of different factors occurs in some row.
"""
import itertools

import numpy as np

import pixfmt_ref as pf
import rig_seams_ref as ref

RIGS = {
    "w64_65": ((40, 32), [(1, (24.0, 1.25)), (2, (-1.0, -0.5))], [(64, 33), (65, 34)]),
    "w63_64": ((40, 32), [(1, (23.0, 1.25)), (2, (-1.0, -0.5))], [(63, 33), (64, 34)]),
    "w64_twice": ((40, 32), [(1, (24.0, 1.25)), (2, (12.0, 0.5, 2e-5, 1e-5))], [(64, 33), (64, 33)]),
    "w128_129": ((72, 64), [(1, (56.0, 1.25)), (2, (-1.0, -0.5))], [(128, 65), (129, 66)]),
    "w128_192": ((72, 64), [(1, (56.0, 1.25)), (2, (-64.0, -0.5))], [(128, 65), (192, 66)]),
    "odd_h": ((64, 37), [(1, (31.5, 1.25)), (2, (-29.75, -0.5))], [(95, 38), (125, 39)]),
    "w65_left_cut": ((40, 32), [(1, (24.0, 1.25)), (2, (-1.0, -0.5), (-4.0, -0.5))], [(64, 33), (65, 34)]),
    "w65_right_cut": ((40, 32), [(1, (24.0, 1.25)), (2, (-1.0, -0.5), (27.0, -0.5))], [(64, 33), (65, 34)]),
    "w63_right_cut": ((40, 32), [(1, (23.0, 1.25)), (2, (12.0, 0.5, 2e-5, 1e-5), (26.0, 0.5, 2e-5, 1e-5))], [(63, 33), (63, 33)]),
}
# name -> the side on which the last step's domains have pixels within the radius of the canvas border
CUT = {"w65_left_cut": "left", "w65_right_cut": "right", "w63_right_cut": "right"}
RADII = (0, 1, 8)


def sizes(name):
    return [RIGS[name][0]] * 3


def steps(capi, name):
    """The step dicts of a rig (capi.step_geometry: host arithmetic), each with the frame it is stitched to as "mosaic_src"."""
    moves = [(m[0], ref.shift(*m[1])[0], ref.shift(*m[-1])[1]) for m in RIGS[name][1]]  # (frame, forward map, backward map)
    st = ref.hand_steps(capi, sizes(name), moves)
    return [dict(s, mosaic_src=(st[k - 1]["src"] if k else s["start"])) for k, s in enumerate(st)]


def sums_of_a_row(four, cw):
    """Whether the four integers can be those of a middle row of cw columns (the rule stitch_seam_from_sums states)."""
    s_a, n_a, s_o, n_o = four
    ok = 1 <= n_o <= n_a <= cw and s_o <= s_a
    return ok and all(n * (n - 1) // 2 <= s <= n * cw - n * (n + 1) // 2 for s, n in ((s_a, n_a), (s_o, n_o)))


def given_seams(geometric, steps):
    """The `given` level of the seams factor: the geometric records with the footprint and the overlap both moved three columns to the
    right -- or to the left where the footprint touches the right border -- so the seam they state lies three columns from the
    geometric one, on the same branch."""
    out = []
    for s, st in zip(geometric, steps):
        s_a, n_a, s_o, n_o = (int(v) for v in s[:4])
        moved = [(s_a + d * n_a, n_a, s_o + d * n_o, n_o) for d in (3, -3)]
        out.append(next(m for m in moved if sums_of_a_row(m, st["cw"])))
    return out


def odd_rect(cw, ch):
    """The rectangle of crop mode 2: x0 odd, a width that is no multiple of 4, the right edge beyond x = 64 where the canvas has one."""
    x0, y0 = 27, 3
    w = min(38, cw - x0)
    w -= 1 if w % 4 == 0 else 0
    h = min(23, ch - y0 - 2)
    assert x0 % 2 == 1 and w % 4 and w >= 1 and h >= 1 and x0 + w <= cw and y0 + h <= ch
    return (x0, y0, w, h)


def repitched(im, pitch, pitch2, fill=0xEE):
    """An image (pixfmt_ref's dict) at other pitches: the same pixel bytes, every byte of padding = fill."""
    fmt, w, h = im["fmt"], im["w"], im["h"]
    t = pf.tight(fmt, w)
    b1, b2 = pf.image_bytes(fmt, w, h, pitch, pitch2 or None)
    data, data2 = np.full(b1, fill, np.uint8), (np.full(b2, fill, np.uint8) if b2 else None)
    for y in range(h):
        data[y * pitch:y * pitch + t[0]] = im["data"][y * im["pitch"]:y * im["pitch"] + t[0]]
    if b2:
        for y in range((h + 1) // 2):
            data2[y * pitch2:y * pitch2 + t[1]] = im["data2"][y * im["pitch2"]:y * im["pitch2"] + t[1]]
    return dict(fmt=fmt, w=w, h=h, data=data, data2=data2, pitch=pitch, pitch2=pitch2 if b2 else 0)


# ---- the option table ---------------------------------------------------------------------------------------------------------------------
FACTORS = ("exposure", "seams", "crop", "input", "output", "finish", "monitor", "sets")
VALUES = {
    "exposure": (0, 1, 2),
    "seams": ("content", "given", "geometric"),
    "crop": (0, 1, 2),  # none; mode 1 with the inscribed rectangle; mode 2 with odd_rect
    # planar; BGR24 at a tight pitch and an aligned base (the projection may stage it); NV12 at pitches of tight + 5 in every set
    # and the LAST set's planes one byte off as well.  Every set of that level is ineligible for staging by its pitch alone, so the call
    # takes the unpack fallback with rows of every alignment; it is NOT a call whose sets differ in eligibility -- the fixed rows of
    # tests/test_gpu_rig_lattice.py hold those (BGR24 with only the last set's base off) and NV12 that IS staged (tight, aligned)
    "input": ("planar", "bgr24", "nv12_mixed"),
    "output": ("planar", "nv12_padded", "rgbx32"),  # NV12 at pitches of tight + 5 in buffers of 0xEE; RGBX32 tight
    "finish": (True, False),
    "monitor": (None, 1, 8),
    "sets": ((2, 16), (3, 2)),  # (n_sets, max_sets): one launch sequence; two (2 + 1)
}
LEVELS = tuple(len(VALUES[f]) for f in FACTORS)
MATRIX = 1  # the NV12 matrix of every formatted row


def covering_rows(levels, strength):
    """Rows (tuples of level indices, one per factor) such that every `strength` factors take every combination of their levels in
    some row.  Greedy and deterministic: each step takes the row of the full product, in itertools.product's order, that covers the
    most combinations not yet covered; among equals the first."""
    rows = np.array(list(itertools.product(*[range(n) for n in levels])), np.int64)
    ids, base = [], 0
    for combo in itertools.combinations(range(len(levels)), strength):
        code = np.zeros(len(rows), np.int64)
        for f in combo:
            code = code * levels[f] + rows[:, f]
        ids.append(base + code)
        base += int(np.prod([levels[f] for f in combo]))
    ids = np.stack(ids, axis=1)  # (rows, combos): the combination each row gives each choice of factors
    open_ = np.ones(base, bool)
    out = []
    while open_.any():
        gain = open_[ids].sum(axis=1)
        best = int(np.argmax(gain))  # the first of the largest
        out.append(tuple(int(v) for v in rows[best]))
        open_[ids[best]] = False
    return out


def options(row):
    """A row of covering_rows(LEVELS, ...) as a dict factor -> value."""
    return {f: VALUES[f][i] for f, i in zip(FACTORS, row)}


def creation_key(opt):
    """What a handle is created with: rows that share it run on one handle."""
    return (opt["exposure"], opt["finish"], opt["sets"])


def groups(rows):
    """creation_key -> the rows' options in table order; the keys in order of first appearance."""
    out = {}
    for row in rows:
        opt = options(row)
        out.setdefault(creation_key(opt), []).append(opt)
    return out
