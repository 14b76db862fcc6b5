"""CPU: tests/rig_lattice2.py and tests/rig_chain_ref.py themselves, on the CPU oracle alone.  The table is deterministic and covers
every pair of levels; every (rig, crop, scale) satisfies the scale's size rule; every given seam is a row's sums; margin 1 leaves every
step's eroded coverage non-empty; with every new option off the CPU statement is rig_seams_ref.chain_given byte for byte; no level is
vacuous -- for every new level some row of the table changes when that level alone is switched off, and the facts the GPU file leans
on hold on the synthetic sets (a found path that is no vertical line, an anchor that moves a path, the two anchor policies apart, the
filter at work, fixed paths that are not the found ones); and three deliberate mis-statements each change some row."""
import itertools

import numpy as np
import pytest

import rig_chain_ref as rc
import rig_edges as re_
import rig_lattice2 as l2
import rig_seams_ref as ref
import scale_ref as sr
import seam_path_ref as sp

_ctx = {}
STREAM = ((3, 2), 2)


def _context(st, oracle, name):
    if name not in _ctx:
        _ctx[name] = l2.Ctx(st.capi, oracle, name)
    return _ctx[name]


# ---- the table ----------------------------------------------------------------------------------------------------------------------------
def test_the_table_is_deterministic_and_covers_every_pair():
    rows = l2.rows()
    assert rows == l2.rows() == re_.covering_rows((7, 6, 3, 3, 5, 5, 2, 2, 3), 2) and l2.LEVELS == (7, 6, 3, 3, 5, 5, 2, 2, 3)
    assert len(rows) == 48 and len(set(rows)) == 48
    for combo in itertools.combinations(range(len(l2.LEVELS)), 2):
        assert {tuple(r[f] for f in combo) for r in rows} == set(itertools.product(*[range(l2.LEVELS[f]) for f in combo])), combo
    tab = l2.table()
    grouped = l2.groups(tab)
    assert len(grouped) == 14 and sum(len(g) for g in grouped.values()) == 48
    assert len({l2.key_id(k) for k in grouped}) == 14
    for key, g in grouped.items():
        assert g == [o for o in tab if l2.creation_key(o) == key]
    assert all(o["exposure"][0] in (1, 2) for o in tab if o["exposure"][1] is not None)  # no temporal statistics without a mode
    assert re_.LEVELS == (3, 3, 3, 3, 3, 2, 3, 2)  # the first table stays what it was


def test_the_padded_pitches_and_the_scales():
    for t in range(1, 300):
        assert l2.padded(t) > t and l2.padded(t) % 4
    assert l2.scale_of("eighth", 65, 34) == (9, 5) and l2.scale_of("eighth", 64, 33) == (8, 5) and l2.scale_of(None, 65, 34) is None
    for w, h in ((65, 34), (125, 39), (38, 23), (63, 30)):
        ow, oh = l2.scale_of("coprime", w, h)
        assert np.gcd(ow, w) == 1 and np.gcd(oh, h) == 1 and 5 * ow >= 3 * w and 7 * oh >= 4 * h
        assert all(np.gcd(v, w) != 1 for v in range(-(-3 * w // 5), ow)) and all(np.gcd(v, h) != 1 for v in range(-(-4 * h // 7), oh))


@pytest.mark.parametrize("name", l2.RIG_NAMES + ("odd_w", "w64_twice"))
def test_the_rigs_admit_every_level(st, oracle, name):
    ctx = _context(st, oracle, name)
    assert ctx.cw <= 129 and ctx.ch <= 66
    x0, y0, w, h = ctx.inscribed
    assert w * h >= 2 and ctx.geo["cov"][-1]["U"][y0:y0 + h, x0:x0 + w].all()
    for opt in l2.table():
        w, h = ctx.source_size(opt)
        ow, oh = ctx.out_size(opt)
        assert sr.rule(w, h, ow, oh), (opt["crop"], opt["scale"])
    for four, s in zip(ctx.given, ctx.steps):
        assert re_.sums_of_a_row(four, s["cw"])
    assert [tuple(g) for g in ctx.given] != [g[:4] for g in ctx.geo["geometric"]]
    for k, c in enumerate(ctx.geo["cov"]):  # margin 1: the finder still has columns where neither side is wrong
        assert sp.erode_x(c["A"], l2.MARGIN).any() and sp.erode_x(c["B"], l2.MARGIN).any(), k
        assert (sp.erode_x(c["A"], l2.MARGIN) & sp.erode_x(c["B"], l2.MARGIN)).any(), k
    if name == "odd_w":
        assert all(w % 2 == 1 for w, _ in ctx.sizes) and [(s["cw"], s["ch"]) for s in ctx.steps] == [(65, 34), (66, 35)]
    if name == "w64_twice":
        assert len({(s["cw"], s["ch"]) for s in ctx.steps}) == 1  # one masked workspace serves both steps
    if name == "w64_65":
        assert ctx.cw == 65 and l2.pyr.tight(l2.pyr.YUYV, l2.scale_of("eighth", 65, 34)[0])[0] == 20  # 9 columns: five groups, the last of one pixel


# ---- the statement with every new option off -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", l2.RIG_NAMES)
def test_with_every_new_option_off_it_is_chain_given(st, oracle, name):
    ctx = _context(st, oracle, name)
    opt = dict(l2.NONE, calls=((3,), 2), index=0)
    (results, state), = ctx.run(opt)
    assert state["anchor"] is None and state["smooth"] == [None, None]
    for i, r in enumerate(results):
        assert r["status"] == 0 and r["paths"] == [] and r["records"] is None
        want = ref.chain_given(oracle, ctx.planar(i), ctx.steps, r["seams"])
        assert r["out"].tobytes() == want.tobytes() and r["out"].shape == want.shape, i
    given = ctx.run(dict(opt, seams="given"))[0][0]
    for i, r in enumerate(given):
        assert r["seams"] == [tuple(g) for g in ctx.given]
        assert r["out"].tobytes() == ref.chain_given(oracle, ctx.planar(i), ctx.steps, ctx.given).tobytes(), i
    unfinished = ctx.run(dict(opt, finish=False))[0][0]
    assert unfinished[0]["out"].tobytes() == ref.chain_given(oracle, ctx.planar(0), ctx.steps, results[0]["seams"], finish=False).tobytes()


# ---- no level is vacuous ----------------------------------------------------------------------------------------------------------------
def _signature(run):
    """Everything a row's CPU statement says, comparable."""
    sig = []
    for results, state in run:
        for r in results:
            out = r["out"]
            sig.append((out.tobytes(), out.shape) if isinstance(out, np.ndarray) else (out["data"].tobytes(), None if out["data2"] is None else out["data2"].tobytes(),
                                                                                      out["pitch"], out["pitch2"], out["fmt"], out["w"], out["h"]))
            sig.append(tuple(p.tobytes() for p in r["paths"]))
    return sig


OFF = dict(seams="content", crop=0, scale=None, input="planar", output="planar")
NEW_LEVELS = [("exposure", v, (v[0], None)) for v in l2.VALUES["exposure"] if v[1] is not None] + \
    [(f, v, OFF[f]) for f in ("seams", "scale", "input", "output") for v in l2.VALUES[f] if v != OFF[f] and v != "given"] + \
    [("seams", "paths_set", "paths"), ("seams", "paths_call", "paths"), ("seams", "paths_fixed", "paths")]


@pytest.mark.parametrize("name", l2.RIG_NAMES)
def test_no_new_level_is_vacuous(st, oracle, name):
    """For every new level some row of the table differs, in output bytes or paths, from the same row with that level switched off
    (an anchored or fixed-path level also from the same row with plain found paths)."""
    ctx = _context(st, oracle, name)
    tab = l2.table()
    for factor, level, off in NEW_LEVELS:
        rows = [o for o in tab if o[factor] == level]
        assert rows, (factor, level)
        assert any(_signature(ctx.run(o)) != _signature(ctx.run(dict(o, **{factor: off}))) for o in rows), (name, factor, level)


@pytest.mark.parametrize("name", l2.RIG_NAMES + ("w64_twice",))
def test_the_facts_the_gpu_rows_lean_on(st, oracle, name):
    ctx = _context(st, oracle, name)
    base = dict(l2.NONE, calls=STREAM, index=0)
    free = ctx.run(dict(base, seams="paths"))
    paths = [p for results, _ in free for r in results for p in r["paths"]]
    assert any(len(set(p.tolist())) > 1 for p in paths), "some found path is no vertical line"
    assert all(r["moved"] == [0, 0] for results, _ in free for r in results) and free[-1][1]["anchor"] is None
    per_set, per_call = ctx.run(dict(base, seams="paths_set")), ctx.run(dict(base, seams="paths_call"))
    moved = [(i, k) for i, r in enumerate(r for results, _ in per_set for r in results) for k in range(2)
             if r["moved"][k] > 0 and r["paths"][k].tolist() != [r2 for results, _ in free for r2 in results][i]["paths"][k].tolist()]
    assert moved, "some anchored path differs from the unanchored one with moved > 0"
    assert _signature(per_set) != _signature(per_call), 'policy "set" differs from policy "call" in the 3 + 2 stream'
    # the first set of a stream is unanchored under either policy; the second call's first set anchors on set 2 under both
    assert _signature(per_set)[:2] == _signature(per_call)[:2] == _signature(free)[:2]
    assert all(p.tolist() == q.tolist() for p, q in zip(per_set[0][1]["anchor"], per_set[0][0][-1]["paths"]))
    fixed = ctx.run(dict(base, seams="paths_fixed"))
    assert all(a.tolist() != b.tolist() and np.abs(a - b).max() == 1 for a, b in zip(fixed[0][0][0]["paths"], free[0][0][0]["paths"]))
    assert fixed[0][0][0]["out"].tobytes() != free[0][0][0]["out"].tobytes() and fixed[0][0][0]["costs"] == [0, 0]
    for mode in (1, 2):
        smooth, plain = ctx.run(dict(base, exposure=(mode, ("keep", 192)))), ctx.run(dict(base, exposure=(mode, ("keep", 0))))
        unsmoothed = ctx.run(dict(base, exposure=(mode, None)))
        assert _signature(plain) == _signature(unsmoothed), "keep 0 is the rig without the option"
        assert _signature(smooth) != _signature(plain), "keep 192 differs from keep 0"
        assert _signature(smooth)[0] == _signature(plain)[0]  # the first set has no state to lean on
        assert np.array_equal(smooth[1][1]["smooth"][0], smooth[1][0][-1]["used"][0])  # the state is the last used record
        given = ctx.run(dict(base, exposure=(mode, "fixed")))
        assert _signature(given)[0] != _signature(unsmoothed)[0] and smooth[0][1]["smooth"][0] is not None and given[0][1]["smooth"] == [None, None]
        assert rc.et.valid(given[0][0][0]["used"][0]) and np.array_equal(given[0][0][0]["used"], given[1][0][1]["measured"])


# ---- the statement is sensitive where a rig could go wrong ------------------------------------------------------------------------------
@pytest.mark.parametrize("name", l2.RIG_NAMES)
def test_three_mis_statements_each_change_some_row(st, oracle, name):
    ctx = _context(st, oracle, name)
    tab = l2.table()

    def changed(rows, **wrong):
        assert rows
        return any(_signature(ctx.run(o)) != _signature(ctx.run(o, chain=dict(ctx.chain_options(o), **wrong))) for o in rows)

    assert changed([o for o in tab if o["crop"] == 2 and o["finish"] and o["scale"]], wrong_scale_first=True), "the scale before a mode-2 finish pass"
    assert changed([o for o in tab if o["seams"] in ("paths_set", "paths_call") and o["calls"][1] == 2], wrong_anchor_cut=2), "the anchor dropped between sequences"
    assert changed([o for o in tab if o["exposure"][1] not in (None, "fixed") and len(o["calls"][0]) == 2], wrong_smoothing_cut=True), "the state dropped between calls"
