"""No GPU: tests/band_hard.py held to the oracle before any GPU run.

a  the table states the oracle's answer for every item tests/test_gpu_band_hard.py runs (the whole Oracle.pair and the seam scan of the
   middle row agree), the three refusal placements answer -3, -2 and -3 on every canvas, and derive_tables() gives PHASE and REFUSED;
b  emptiness is real: the bands EMPTY states hold only zeros on the oracle's canvases, the blurred plane is not +0 in the row where a
   state enters them, on every canvas some band next to an empty one holds a sample within two rows of the shared edge, and the
   directions the band path distinguishes (a band empty BELOW data: the causal state enters it; ABOVE data: the anticausal state)
   occur on every canvas that can have them;
c  the class rule covers: every class meets every form and every placement, every saturating and every holed class every canvas;
d  the content does what it is there for, counted on the oracle's output."""
import collections

import numpy as np
import pytest

import band_hard as BH
import hard_inputs as H


@pytest.fixture(scope="module")
def answers():
    """key -> (rc of Oracle.pair, rc of the seam scan, share of output samples equal to 255) of every item, computed once."""
    out = {}
    for c, placement, form, dtype, variant in BH.items():
        r = BH.item(c, placement, form, dtype, variant)
        rc, ref, _ = H.pair_oracle(r)
        out[r["key"]] = (rc, BH.seam_of(r)[0], float((ref == 255).mean()), r["frame"], r["mosaic"])
    return out


# ---- a ---------------------------------------------------------------------------------------------------------------------------
def test_the_table_states_the_oracles_answer(answers):
    assert len(answers) == len(set(BH.items())) == 2 * 2 * len(BH.PLACEMENTS) * (len(BH.FORM_NAMES) + 3 * 2)
    for key, (rc, seam_rc, _, _, _) in answers.items():
        want = BH.REFUSED.get(key, 0)
        assert rc == want and seam_rc == want, (key, rc, seam_rc, want)
    assert set(BH.REFUSED) <= set(answers) and set(BH.PHASE) <= set(answers) and not set(BH.REFUSED) & set(BH.PHASE)
    assert all(rc in (-2, -3) for rc in BH.REFUSED.values()) and all(ph in (1, 2, 3) for ph in BH.PHASE.values())
    assert set(BH.RUN_ORDER) == set(BH.PLACEMENTS)


def test_the_tables_are_what_the_search_gives():
    phases, refused = BH.derive_tables()
    assert phases == BH.PHASE and refused == BH.REFUSED
    assert BH.derive_refused() == BH.REFUSED


def test_the_refusal_placements_are_refused():
    for c in range(len(BH.CANVASES)):
        for dtype in BH.DTYPES:
            for name, want in BH.REFUSAL_PLACEMENTS.items():
                r = BH.refusal_pair(c, name, dtype)
                assert H.pair_oracle(r)[0] == want and BH.seam_of(r)[0] == want, (c, name, np.dtype(dtype).name)
    assert [BH.REFUSAL_PLACEMENTS[n] for n in ("mosaic_above_mid", "fold", "miss")] == [-3, -2, -3]


def test_phases_of_a_checkerboard_pair_on_frame_mid():
    """Where the phase matters: a checkerboard frame over a checkerboard mosaic on frame_mid at 768 x 384 is accepted at the phases 0
    and 3 and has no overlap at 1 and 2 -- the search's method on the one pair that needs it (the class rule never pairs two)."""
    cw, ch, x0, mw = BH.CANVASES[BH.MAIN][:4]
    f0, f1, m0, m1 = BH.rows("frame_mid", ch)
    got = []
    for phase in range(4):
        r = BH.placed(BH.MAIN, "frame_mid", "aligned", H.checker(cw - x0, f1 - f0, np.uint8, phase=phase >> 1), H.checker(mw, m1 - m0, np.uint8, phase=phase & 1))
        got.append(H.pair_oracle(r)[0])
    assert got == [0, -3, -3, 0]


# ---- b ---------------------------------------------------------------------------------------------------------------------------
def canvases_of(oracle, c, placement, variant):
    r = BH.synth_pair(c, placement, variant, np.uint8)
    return r, oracle.warp(r["F"], r["p"], 0.0, 0.0, r["cw"], r["ch"]), oracle.move(r["M"], r["ox"], r["oy"], r["cw"], r["ch"])


def test_the_placements_give_the_stated_rows(oracle):
    for c, (cw, ch, x0, mw, _, _) in enumerate(BH.CANVASES):
        for placement in BH.PLACEMENTS + ("mosaic_above_mid",):
            f0, f1, m0, m1 = BH.rows(placement, ch)
            assert 0 <= f0 < f1 <= ch and 0 <= m0 < m1 <= ch
            r, a, b = canvases_of(oracle, c, placement, "aligned")
            want = np.zeros_like(b)
            want[:, m0:m1, :mw] = r["M"]  # Oracle.move puts mosaic row r at canvas row r - oy
            assert np.array_equal(b, want), (c, placement)
            want = np.zeros_like(a)
            want[:, f0:f1, x0:] = r["F"]  # the exact shift
            assert np.array_equal(a, want), (c, placement)
            _, a, _ = canvases_of(oracle, c, placement, "tilted")  # an edge moves by up to two rows
            rows_hit = np.flatnonzero(a.any(axis=(0, 2)))
            assert max(f0 - 2, 0) <= rows_hit.min() <= f0 and max(f1 - 2, 0) <= rows_hit.max() + 1 <= f1, (c, placement, rows_hit.min(), rows_hit.max())
            if placement in BH.PLACEMENTS:
                assert f0 <= ch // 2 < f1 - 2 and m0 <= ch // 2 < m1  # both hold the middle row


# Where a placement's image ends at a band's edge (the *_mid placements on 128-, 132- and 64-row bands, frame_low at an even band count)
# the band beside an empty one holds a sample within two rows of the shared edge; elsewhere it ends up to 64 rows short of it.  What
# matters is that the state crossing the edge is not zero: the blur's tail stays non-zero for some 150 rows, and the blurred plane is
# held non-zero in the empty band's edge row in EVERY case; the cases within two rows are counted per canvas.


def test_emptiness_is_real(oracle):
    assert BH.derive_empty() == BH.EMPTY and set(BH.EMPTY) == {(c, q) for c in range(len(BH.CANVASES)) for q in BH.PLACEMENTS}
    below, above, neither = collections.defaultdict(list), collections.defaultdict(list), []
    for (c, placement), stated in BH.EMPTY.items():
        bands = BH.band_rows(c)
        assert bands[0][0] == 0 and bands[-1][1] == BH.CANVASES[c][1] and len({r1 - r0 for r0, r1 in bands}) == 1
        _, a, b = canvases_of(oracle, c, placement, "aligned")
        for what, img, empty in (("frame", a, stated[0]), ("mosaic", b, stated[1])):
            hit = img.any(axis=(0, 2))  # per canvas row
            blurred = oracle.blur(img.astype(np.float32)).view(np.uint32).any(axis=(0, 2)) if empty else None  # G_0's rows, bit patterns
            for k, (r0, r1) in enumerate(bands):
                assert hit[r0:r1].any() != (k in empty), (c, placement, what, k)
            for k in empty:
                r0, r1 = bands[k]
                if k > 0 and k - 1 not in empty:  # data above: the band is empty BELOW data, the causal state enters it
                    assert blurred[r0], (c, placement, what, k)  # the blur's tail is not +0 in the empty band's first row
                    below[c].append((placement, what, k, bool(hit[r0 - 2:r0].any())))
                if k + 1 < len(bands) and k + 1 not in empty:  # data below: empty ABOVE data, the anticausal state enters it
                    assert blurred[r1 - 1], (c, placement, what, k)
                    above[c].append((placement, what, k, bool(hit[r1:r1 + 2].any())))
        neither += [(c, placement, k) for k in stated[0] if k in stated[1]]
    print("empty below data:", dict(below))
    print("empty above data:", dict(above))
    print("reached by neither image:", neither)
    for c, canvas in enumerate(BH.CANVASES):
        assert any(e[3] for e in above[c]), c  # empty above data, and the data within two rows of the edge
        # with two bands the second begins with the middle row, which both images of an accepted pair hold: none can be empty below data
        assert bool(below[c]) == any(e[3] for e in below[c]) == (canvas[4] > 2), c
    assert neither == [(1, "both_mid", 0), (1, "both_mid", 5)]
    # consecutive runs of the GPU test leave their zero tiles elsewhere
    for c in range(len(BH.CANVASES)):
        if BH.CANVASES[c][4] > 2:
            for q0, q1 in zip(BH.RUN_ORDER, BH.RUN_ORDER[1:]):
                assert BH.EMPTY[(c, q0)] != BH.EMPTY[(c, q1)], (c, q0, q1)


# ---- c ---------------------------------------------------------------------------------------------------------------------------
def test_the_class_rule_covers():
    for dtype in BH.DTYPES:
        with_form, with_place, on_canvas = collections.defaultdict(set), collections.defaultdict(set), collections.defaultdict(set)
        for c, placement, form, dt, variant in BH.items():
            if dt is dtype and BH.stated_rc(c, placement, form, dt, variant) == 0:
                for cls in BH.item_classes(c, placement, form, dt):
                    with_form[cls].add(form)
                    with_place[cls].add(placement)
                    on_canvas[cls].add(c)
        classes = H.classes_of(dtype)
        assert set(with_form) == set(classes)
        for cls in classes:
            assert with_form[cls] == set(BH.FORM_NAMES), (cls, with_form[cls])
            assert with_place[cls] == set(BH.PLACEMENTS), (cls, with_place[cls])
            if cls in H.SATURATING + H.HOLED:
                assert on_canvas[cls] == set(range(len(BH.CANVASES))), (cls, on_canvas[cls])
    for classes in (H.U8_CLASSES, H.F32_CLASSES):  # the frame and the mosaic of an item never share a class: at most one checkerboard
        assert all(classes[i] != classes[(i + 3) % len(classes)] for i in range(len(classes)))
    seeds = [BH.item_seed(c, q) for c in range(len(BH.CANVASES)) for q in BH.PLACEMENTS]
    assert len(set(seeds)) == len(seeds)


# ---- d ---------------------------------------------------------------------------------------------------------------------------
def test_the_content_reaches_the_upper_clamp(oracle, answers):
    r = BH.full_height_pair(BH.MAIN, np.uint8)
    rc, ref, _ = H.pair_oracle(r)
    assert rc == 0 and (ref == 255).mean() < 1e-3  # the synthetic pair hardly saturates
    best = collections.defaultdict(float)
    for key, (rc, _, share, fc, mc) in answers.items():
        if rc == 0:
            for cls in (fc, mc):
                best[cls] = max(best[cls], share)
    print({k: round(v, 4) for k, v in sorted(best.items())})
    for cls in H.SATURATING:
        assert best[cls] >= 0.01, (cls, best[cls])


def test_tiny_puts_negative_zero_and_subnormals_beside_an_empty_band(oracle):
    """Every item with a `tiny` image that leaves a band empty: the band that borders the empty one holds -0.0f and subnormals of that
    image -- what the zero-tile flags must not take for +0, and what crosses to the neighbour in states and halo rows."""
    seen = collections.Counter()
    for c, placement, form, dtype, variant in BH.items():
        if dtype is not np.float32 or "tiny" not in BH.item_classes(c, placement, form, dtype):
            continue
        which = BH.item_classes(c, placement, form, dtype).index("tiny")
        empty = BH.EMPTY[(c, placement)][which]
        if not empty:
            continue
        r = BH.item(c, placement, form, dtype, variant)
        img = oracle.warp(r["F"], r["p"], 0.0, 0.0, r["cw"], r["ch"]) if which == 0 else oracle.move(r["M"], r["ox"], r["oy"], r["cw"], r["ch"])
        bits = img.view(np.uint32)
        bands = BH.band_rows(c)
        for k in empty:
            for nb in (k - 1, k + 1):
                if 0 <= nb < len(bands) and nb not in empty:
                    r0, r1 = bands[nb]
                    part = bits[:, r0:r1]
                    assert (part == 0x80000000).any(), (r["key"], nb)
                    assert ((part & 0x7F800000 == 0) & (part & 0x007FFFFF != 0)).any(), (r["key"], nb)
                    seen[c] += 1
    print(dict(seen))
    assert all(seen[c] > 0 for c in range(len(BH.CANVASES))), seen
