"""CPU: tests/rig_hard.py itself, held to the CPU statement of the replay (tests/rig_chain_ref.py) before any GPU run.  The class rule
is deterministic and, over the two rigs, brings every (factor level, class) pair into some row's stream; the statement refuses exactly
rig_hard.REFUSED; the classes reach what they are there for (NON-VACUITY, on the reference alone); some row's result differs from the
same row on synthetic frames in the thing its class is there for (SENSITIVITY); the contrast set's step-0 cost holds the d term's
ceiling, 2040.

Where the measured facts are narrower than "every set", the assertion says what holds and why the rest cannot:
  * samples equal to 255 in the unfinished mosaic.  A synthetic set holds at most 6 of them (below 0.1 % of its samples: the collapse's
    overshoot).  Every accepted `binary` and `white` set under exposure modes 0 and 1 holds them, and every accepted planar `checker`
    set under mode 1; each class reaches at least 1 % in some set (measured: white up to 29 %, binary 6.6 %, checker 5.9 %).  A one-pixel
    checkerboard through a 4:2:x layout has its chroma averaged to grey and hardly saturates (no such sample in 23 of 24 sets), and mode 2's transfer
    towards the running mosaic takes most of the saturation away (white: 0 .. 0.9 %).
  * all-zero pixels inside a step's coverage: every `band` set, and every `holes` set at the planar and the 4:2:2 levels.  NV21's
    2 x 2 chroma average leaves a lone black pixel its neighbours' chroma: such a `holes` set has none (measured: none in 7 of 8 sets)."""
import numpy as np
import pytest

import pixfmt_yuv_ref as pyr
import rig_hard as rh
import rig_lattice2 as l2

TABLE = l2.table()
PLAIN = dict(crop=None, scale=None, out_fmt=0, out_pitch=None, finish=False, monitor=None)  # the unfinished mosaic as it stands
_ctx, _runs = {}, {}


def _context(st, oracle, name, hard=True):
    if (name, hard) not in _ctx:
        _ctx[(name, hard)] = (rh.Ctx if hard else l2.Ctx)(st.capi, oracle, name)
    return _ctx[(name, hard)]


def _run(st, oracle, name, opt, hard=True, plain=False):
    """The CPU statement of a row, flat per set -> [one_set's dict]; once per (rig, row, frames, output)."""
    key = (name, opt["index"], hard, plain)
    if key not in _runs:
        ctx = _context(st, oracle, name, hard)
        chain = ctx.chain_options(opt)
        _runs[key] = [r for results, _ in ctx.run(opt, chain=dict(chain, **PLAIN) if plain else chain) for r in results]
    return _runs[key]


def _sets(st, oracle, name, opt):
    """Per set of a row's stream (set number, class, the frames' reference images)."""
    ctx = _context(st, oracle, name)
    flat = [[im for im, _ in fs] for sets in ctx.host(opt) for fs in sets]
    return [(i, rh.class_of(name, opt["index"], i), fs) for i, fs in enumerate(flat)]


# ---- the rule ---------------------------------------------------------------------------------------------------------------------------
def test_the_assignment_is_deterministic_and_covers_every_level_with_every_class(st, oracle):
    assert rh.CLASSES == ("checker", "holes", "fullrange", "binary", "band", "white", "raw") and rh.RIG_NUMBER == {"odd_h": 0, "w64_65": 1} and rh.OFFSET == 3
    everything = {(f, v, c) for f in l2.FACTORS for v in l2.VALUES[f] for c in rh.CLASSES}

    def seen(names):
        return {(f, opt[f], rh.class_of(n, opt["index"], i)) for n in names for opt in TABLE for i in range(sum(opt["calls"][0])) for f in l2.FACTORS}

    assert seen(l2.RIG_NAMES) == everything
    # one rig alone leaves two pairs out; the second rig's offset closes them
    assert everything - seen(("odd_h",)) == {("exposure", (1, ("keep", 192)), "holes"), ("output", "uyvy_tight", "checker")}
    for opt in TABLE:  # the class changes inside every stream
        n = sum(opt["calls"][0])
        assert all(rh.class_of(name, opt["index"], i) != rh.class_of(name, opt["index"], i + 1) for name in l2.RIG_NAMES for i in range(n - 1))
    a, b = rh.Ctx(st.capi, oracle, "w64_65"), _context(st, oracle, "w64_65")
    for opt in (TABLE[3], TABLE[5], TABLE[10]):  # the same bytes from another context
        for x, y in zip((im for sets in a.host(opt) for fs in sets for im, _ in fs), (im for sets in b.host(opt) for fs in sets for im, _ in fs)):
            assert l2.same(x, y)


def test_raw_is_no_pack_of_anything(st, oracle):
    """A raw image of a formatted level: every byte -- padding too -- is random, and packing its unpacked frame again does not give it
    back.  For the planar level raw is fullrange, and the classes do not depend on the level."""
    ctx = _context(st, oracle, "w64_65")
    opt = next(o for o in TABLE if o["input"] == "nv16_padded" and any(c == "raw" for _, c, _ in _sets(st, oracle, "w64_65", o)))
    i, _, frames = next(s for s in _sets(st, oracle, "w64_65", opt) if s[1] == "raw")
    im = frames[0]
    assert im["pitch"] > pyr.tight(im["fmt"], im["w"])[0] and len(np.unique(im["data"])) > 200 and len(np.unique(im["data2"])) > 200
    again = pyr.pack(pyr.unpack(im, ctx.matrix_of(opt)), im["fmt"], ctx.matrix_of(opt), im["pitch"], im["pitch2"])
    assert not np.array_equal(again["data"], im["data"])
    planar = dict(opt, input="planar")
    assert all(np.array_equal(p, rh.content("fullrange", p.shape[2], p.shape[1], 3 * i + f, f)) for f, p in enumerate(ctx.planar(i, opt["index"])))
    assert [c for _, c, _ in _sets(st, oracle, "w64_65", planar)] == [c for _, c, _ in _sets(st, oracle, "w64_65", opt)]
    for cls in ("raw", "edges"):
        for fmt in rh.ALL_INPUTS:
            e = rh.image_of(cls, fmt, 40, 32, 7)
            assert (e["pitch"], e["pitch2"]) == pyr.tight(fmt, 40) and (len(e["data"]), 0 if e["data2"] is None else len(e["data2"])) == pyr.image_bytes(fmt, 40, 32)
            assert cls == "raw" or (np.isin(e["data"], rh.EDGE_BYTES).all() and set(np.unique(e["data"])) == set(rh.EDGE_BYTES.tolist()))


# ---- refusals -----------------------------------------------------------------------------------------------------------------------------
def test_the_statement_refuses_exactly_the_stated_sets(st, oracle):
    got, total = {}, 0
    for name in l2.RIG_NAMES:
        for opt in TABLE:
            res = _run(st, oracle, name, opt)
            total += len(res)
            got.update({(name, opt["index"], i): r["status"] for i, r in enumerate(res) if r["status"]})
            assert not all(r["status"] for r in res), (name, opt["index"])  # no row is refused in every set
            assert opt["seams"] == "content" or not any(r["status"] for r in res), (name, opt["index"])  # paths and given seams refuse nothing
    assert got == rh.REFUSED == rh.derive_refused({n: _context(st, oracle, n) for n in l2.RIG_NAMES})
    assert total == 250 and 20 * len(got) <= total  # at most 5 % (here 4 of 250)
    for (name, row, i), code in rh.REFUSED.items():
        assert TABLE[row]["seams"] == "content" and code in (-2, -3) and rh.class_of(name, row, i) in ("checker", "white")


# ---- non-vacuity ----------------------------------------------------------------------------------------------------------------------------
def test_raw_bytes_leave_the_gamut(st, oracle):
    n = 0
    for name in l2.RIG_NAMES:
        for opt in TABLE:
            if l2.IN_FMT[opt["input"]][0] in rh.YUV:
                for i, cls, frames in _sets(st, oracle, name, opt):
                    if cls == "raw":
                        assert all(rh.decode_clipped(im, opt["index"] % 3) >= 0.5 for im in frames), (name, opt["index"], i)
                        n += 1
    assert n >= 20
    synthetic = pyr.pack(oracle.synth(40, 32, 0), pyr.YUYV, 0)
    assert rh.decode_clipped(synthetic, 0) < 0.01


def test_binary_costs_approach_the_ceiling(st, oracle):
    ctx, n = _context(st, oracle, "w64_65"), 0
    for opt in TABLE:
        for i, cls, frames in _sets(st, oracle, "w64_65", opt):
            if cls == "binary":
                assert rh.d_term(ctx, frames, l2.IN_FMT[opt["input"]][0], opt["index"] % 3).max() >= 1024, (opt["index"], i)
                n += 1
    assert n >= 15
    for name in l2.RIG_NAMES:
        syn = _context(st, oracle, name, hard=False)
        assert all(rh.d_term(syn, syn.planar(i)).max() < 1024 for i in range(5)), name


def test_saturating_classes_saturate_the_unfinished_mosaic(st, oracle):
    best = dict.fromkeys(rh.SATURATING, 0.0)
    for name in l2.RIG_NAMES:
        for opt in TABLE:
            hard, syn = _run(st, oracle, name, opt, plain=True), _run(st, oracle, name, opt, hard=False, plain=True)
            assert all(s["status"] == 0 and (s["out"] == 255).mean() < 0.001 for s in syn), (name, opt["index"])
            for i, r in enumerate(hard):
                cls = rh.class_of(name, opt["index"], i)
                if cls not in rh.SATURATING or r["status"]:
                    continue
                share = float((r["out"] == 255).mean())
                best[cls] = max(best[cls], share)
                if opt["exposure"][0] != 2 and (cls != "checker" or opt["input"] == "planar"):
                    assert share > 0, (name, opt["index"], i, cls)
    assert all(v >= 0.01 for v in best.values()), best


def test_holed_classes_put_black_pixels_inside_the_coverage(st, oracle):
    n = 0
    for name in l2.RIG_NAMES:
        ctx = _context(st, oracle, name)
        for opt in TABLE:
            fmt, m = l2.IN_FMT[opt["input"]][0], opt["index"] % 3
            for i, cls, frames in _sets(st, oracle, name, opt):
                if cls in rh.HOLED and not (cls == "holes" and fmt == pyr.NV21):
                    black = sum(int(((rh.warped(ctx, frames, k, fmt, m) == 0).all(axis=0) & ctx.geo["cov"][k]["A"]).sum()) for k in range(len(ctx.steps)))
                    assert black > 0, (name, opt["index"], i, cls)
                    n += 1
    assert n >= 50
    syn = _context(st, oracle, "w64_65", hard=False)
    assert not any(((rh.warped(syn, syn.planar(0), k) == 0).all(axis=0) & syn.geo["cov"][k]["A"]).any() for k in range(2))


# ---- sensitivity ------------------------------------------------------------------------------------------------------------------------------
def test_some_row_differs_from_its_synthetic_twin_where_its_class_matters(st, oracle):
    def paths(res):
        return [p.tolist() for r in res for p in r["paths"]]

    found = [o for o in TABLE if o["seams"] in ("paths", "paths_set", "paths_call")]
    assert any(paths(_run(st, oracle, n, o)) != paths(_run(st, oracle, n, o, hard=False)) for n in l2.RIG_NAMES for o in found), "a found path"

    def without_keep_black(name, opt):
        ctx = _context(st, oracle, name)
        off = [r for results, _ in ctx.run(opt, chain=dict(ctx.chain_options(opt), keep_black=False)) for r in results]
        return any(a["status"] == 0 and b["status"] == 0 and rh.class_of(name, opt["index"], i) in rh.HOLED and not l2.same(a["out"], b["out"])
                   for i, (a, b) in enumerate(zip(_run(st, oracle, name, opt), off)))

    # (no twin here: a projected frame is black outside its footprint, so the rule meets zeros on synthetic frames too -- at the
    # footprint's edge, never inside it.  The holed sets are those of test_holed_classes_put_black_pixels_inside_the_coverage.)
    moded = [o for o in TABLE if o["exposure"][0]]
    assert any(without_keep_black("w64_65", o) for o in moded[:6]), "the keep-black rule on a holed set"

    def at_the_bounds(res):  # output bytes at the ends of the encode's clips (the 0xEE padding is neither)
        return sum(int(np.isin(r["out"][p], (0, 255)).sum()) for r in res if r["status"] == 0 for p in ("data", "data2") if r["out"][p] is not None)

    full = [o for o in TABLE if o["output"] != "planar" and o["index"] % 3 == 2]  # the full-range matrix: 0 and 255 are its clips' ends
    assert any(at_the_bounds(_run(st, oracle, n, o)) > 0 and at_the_bounds(_run(st, oracle, n, o, hard=False)) == 0 for n in l2.RIG_NAMES for o in full), "the pack"


# ---- the contrast set ---------------------------------------------------------------------------------------------------------------------------
def test_the_contrast_set_reaches_the_cost_ceiling(st, oracle):
    ctx = _context(st, oracle, "w64_65")
    calls = rh.contrast_frames(ctx.sizes)
    assert [len(c) for c in calls] == [3, 2] and all((fs[0] == 255).all() and (fs[2] == 255).all() and set(np.unique(fs[1])) == {0, 255} for c in calls for fs in c)
    assert max(int(rh.d_term(ctx, fs).max()) for c in calls for fs in c) == 2040 == 2 * 4 * 255
    for mode in (0, 2):
        run = rh.rc.stream(oracle, ctx.geo, ctx.steps, calls, ctx.chain_options(rh.contrast_row(mode)))
        assert all(r["status"] == 0 for results, _ in run for r in results) and run[1][1]["anchor"] is not None
        assert any(m > 0 for r in run[1][0] for m in r["moved"]) or any(len(set(p.tolist())) > 1 for r in run[1][0] for p in r["paths"])
