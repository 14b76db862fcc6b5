"""CPU: tests/rig_edges.py itself -- the covering arrays cover what they claim, and every hand-made rig is the rig its table row
states: the canvases (capi.step_geometry, host arithmetic), a pyramid under both level rules, a geometric seam at every step, a
residual domain at radii 0, 1 and 8, an inscribed rectangle, footprints that touch the canvas borders, and a `given` seam level that
is not the geometric seam.  The GPU files lean on these facts; here they are established on the CPU oracle alone."""
import itertools

import numpy as np
import pytest

import rect_ref
import residual_ref as rr
import rig_edges as re_
import rig_seams_ref as ref

_cache = {}


def _coverage(capi, oracle, name):
    if name not in _cache:
        st = re_.steps(capi, name)
        _cache[name] = (st, ref.coverage_chain(oracle, re_.sizes(name), 0, st)[0])
    return _cache[name]


# ---- the covering arrays --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("strength", [2, 3])
def test_covering_rows_cover_every_combination(strength):
    rows = re_.covering_rows(re_.LEVELS, strength)
    assert rows == re_.covering_rows(re_.LEVELS, strength)  # no randomness
    assert len(set(rows)) == len(rows) and all(len(r) == len(re_.LEVELS) and all(0 <= v < n for v, n in zip(r, re_.LEVELS)) for r in rows)
    n_product = int(np.prod(re_.LEVELS))
    assert len(rows) < n_product // 10
    for combo in itertools.combinations(range(len(re_.LEVELS)), strength):  # exhaustive
        seen = {tuple(r[f] for f in combo) for r in rows}
        assert seen == set(itertools.product(*[range(re_.LEVELS[f]) for f in combo])), combo
    # every row decodes, and the handle groups hold every row once, in table order
    grouped = re_.groups(rows)
    assert sum(len(g) for g in grouped.values()) == len(rows)
    for key, g in grouped.items():
        assert g == [re_.options(r) for r in rows if re_.creation_key(re_.options(r)) == key]


def test_covering_rows_of_a_small_product_by_hand():
    """Two factors of two levels at strength 2 need the whole product, in whatever order the gains give."""
    assert re_.covering_rows((2, 2), 2) == [(0, 0), (0, 1), (1, 0), (1, 1)]
    assert re_.covering_rows((2, 1, 2), 2) == [(0, 0, 0), (1, 0, 1), (0, 0, 1), (1, 0, 0)]  # the second row covers three new pairs, (0, 0, 1) two
    assert re_.covering_rows((2, 2, 2), 2) == [(0, 0, 0), (0, 1, 1), (1, 0, 1), (1, 1, 0)]  # ties go to the first row in product order


# ---- the rigs ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(re_.RIGS))
def test_every_rig_is_what_its_row_states(st, oracle, name):
    capi = st.capi
    steps, cov = _coverage(capi, oracle, name)
    frame, _, canvases = re_.RIGS[name]
    assert frame[0] % 4 == 0  # both forms of the format projection are eligible
    assert [(s["cw"], s["ch"]) for s in steps] == canvases and all(s["start"] == 0 for s in steps)
    for cw, ch in canvases:
        for rule in (0, 1):
            n, lw, lh = capi.pyramid_levels(cw, ch, rule)
            assert n >= 1 and min(lw) >= 1 and min(lh) >= 1
    for k, c in enumerate(cov):
        cw, ch = canvases[k]
        assert c["rc"] == 0 and c["A"].shape == (ch, cw), f"step {k}"
        for r in re_.RADII:
            assert rr.rig_domain(c["A"], c["B"], r).any(), (k, r)
        rect = rect_ref.stack(c["U"])
        assert rect[2] * rect[3] >= 2 and not c["U"].all()
        # positions outside the canvas do not constrain the erosion: the rule is live where A touches a border
        borders = dict(left=c["A"][:, 0].any(), right=c["A"][:, -1].any(), top=c["A"][0].any(), bottom=c["A"][-1].any())
        assert any(borders.values()), f"step {k}"
        if k == 0:
            assert borders["right"] and borders["bottom"]
        elif name in re_.CUT:
            assert borders[re_.CUT[name]]
        elif name != "w64_twice":  # (whose second frame lies inside the mosaic)
            assert borders["left"]
        # and at step 0 it decides pixels: the radius-8 domain keeps pixels within 8 of a border, which an erosion that took the
        # outside for uncovered would drop
        if k == 0:
            d8 = rr.rig_domain(c["A"], c["B"], 8) != 0
            assert d8[-8:].any() or d8[:, -8:].any()
    # the left and right borders decide pixels in the rigs made for it, and in no other
    near = {"left": lambda d, r: d[:, :r], "right": lambda d, r: d[:, d.shape[1] - r:]}
    for side in ("left", "right"):
        hits = [(near[side](rr.rig_domain(c["A"], c["B"], r), r) != 0).any() for c in cov for r in (2, 7, 8)]
        if re_.CUT.get(name) == side:
            assert all(hits[3:]) and canvases[1][0] % 64  # at the last step; the border lies inside a word
        else:
            assert not any(hits), side


@pytest.mark.parametrize("name", sorted(re_.RIGS))
def test_synthetic_frames_give_content_seams(st, oracle, name):
    """Oracle.synth frames 3 i + f, the sets the GPU tests replay: no step of sets 0 .. 2 fails for its pixels."""
    steps = re_.steps(st.capi, name)
    w, h = re_.RIGS[name][0]
    for i in range(3):
        proj = [oracle.project(oracle.synth(w, h, 3 * i + f)) for f in range(3)]
        mosaic = proj[0]
        for k, s in enumerate(steps):
            rc, mosaic = oracle.pair(proj[s["src"]], s["p"], s["offx"], s["offy"], mosaic, s["ox"], s["oy"], s["cw"], s["ch"])
            assert rc == 0, (i, k)


def _inside(domain, r):
    ch, cw = domain.shape
    return int((domain[r:ch - r, r:cw - r] != 0).sum()) if cw > 2 * r and ch > 2 * r else 0


def test_the_facts_the_gpu_tests_lean_on(st, oracle):
    capi = st.capi
    _, cov = _coverage(capi, oracle, "w64_65")
    doms = [rr.rig_domain(cov[0]["A"], cov[0]["B"], r) for r in re_.RADII]
    assert [int((d != 0).sum()) for d in doms] == [408, 364, 126]
    assert _inside(doms[2], 8) == 84  # the margin trims the radius-8 domain: n of the record is smaller than the domain
    _, cov = _coverage(capi, oracle, "w128_192")
    doms = [rr.rig_domain(cov[1]["A"], cov[1]["B"], r) for r in re_.RADII]
    assert [int((d != 0).sum()) for d in doms] == [475, 408, 1] and _inside(doms[2], 8) == 1
    for name, four in (("w64_65", (1691, 38, 455, 14)), ("w63_64", (1653, 38, 480, 15)), ("w128_129", (6475, 70, 903, 14))):
        assert tuple(_coverage(capi, oracle, name)[1][0]["seam"][:4]) == four, name


@pytest.mark.parametrize("name", sorted(re_.RIGS))
def test_the_given_seams_are_not_the_geometric_ones(st, oracle, name):
    capi = st.capi
    steps, cov = _coverage(capi, oracle, name)
    geometric = [c["seam"] for c in cov]
    given = re_.given_seams(geometric, steps)
    for k, (g, v) in enumerate(zip(geometric, given)):
        for rule in (0, 1):
            bg, sg, _ = ref.derive(g, rule)
            bv, sv, _ = ref.derive(v, rule)
            assert (bg, sg) != (bv, sv) and 0 < sv < steps[k]["cw"], (k, rule)
            got = capi.seam_from_sums(*v, rule, steps[k]["cw"])  # the library takes the record and derives the same seam
            assert (got.branch, got.start) == (bv, sv)


def test_the_crop_rectangles_and_the_repitch():
    import pixfmt_ref as pf
    for name in ("w64_65", "odd_h"):
        cw, ch = re_.RIGS[name][2][-1]
        x0, y0, w, h = re_.odd_rect(cw, ch)
        assert x0 % 2 == 1 and w % 4 and x0 < 64 < x0 + w and y0 + h <= ch
    rng = np.random.default_rng(5)
    planar = rng.integers(0, 256, (3, 7, 10), dtype=np.uint8)
    for fmt in (pf.NV12, pf.RGBX32, pf.BGR24):
        t = pf.tight(fmt, 10)
        wide = re_.repitched(pf.pack(planar, fmt, 1), t[0] + 5, t[1] + 5 if t[1] else 0)
        want = pf.pack(planar, fmt, 1, t[0] + 5, t[1] + 5 if t[1] else None, fill=0xEE)
        assert all(np.array_equal(wide[k], want[k]) for k in ("data", "data2") if want[k] is not None) and wide["pitch"] == want["pitch"]
        assert wide["pitch2"] == want["pitch2"]
