"""GPU: temporally anchored path seams (include/stitch_seam_anchor.h; csrc/k_seam_path.inc, stitch_seam_path.inc,
stitch_rig_seam_paths.inc).  Everything is exact: paths, D, `moved` and bytes.  The anchored finder against tests/seam_anchor_ref.py
on the five pairs of tests/test_gpu_seam_path.py's _finder_case; the rig on the recorded run "4" against the loop of
pipeline.stitch_chain calls that passes each set's found paths on as the next set's anchors."""
import ctypes as C

import numpy as np
import pytest

import seam_anchor_ref as sa
import seam_path_ref as sp
from computervisionimagestich2_amd import capi, pipeline
from test_gpu_seam_path import _dev, _finder_case, _frames, _geometry, _geometry_of, _item, _out, _rig, _run4_sets, _run4_steps, _same, plans  # noqa: F401

pytestmark = pytest.mark.gpu

_cache = {}
OPTIONS = [(0, 1), (1, 2055), (32, 64), (2055, 1)]
MARGIN = 3


# ---- the finder against numpy ------------------------------------------------------------------------------------------------------------
def _anchor_kinds(cw, ch, K, T, free):
    """name -> five anchors (one per pair of _finder_case), each ch integers."""
    y = np.arange(ch)
    rng = np.random.default_rng(1000 * cw + ch)
    ends = np.where(y % 2 == 0, sa.INT32_MIN, sa.INT32_MAX)
    return {
        "own": [f.copy() for f in free],                                                  # the pair's own unanchored path
        "far": [np.full(ch, cw + T + 5)] * 5,                                             # at least T from every column
        "zigzag": [cw // 3 + i + (y % 2) * (K + 5) for i in range(5)],                    # steps larger than K
        "walk": [cw // 2 + np.cumsum(rng.integers(-3, 4, ch)) for _ in range(5)],         # a seeded random walk
        "outside": [np.where((y + i) % 2 == 0, -5, cw + 7) for i in range(5)],
        "ends": [ends if i % 2 == 0 else np.where(y % 2 == 0, sa.INT32_MAX, sa.INT32_MIN) for i in range(5)],
    }


def _find(gpu, dev, cases, cw, ch, K, anchors=None, w=None, T=None):
    pairs = [(d["f"], c["g"]["p"], c["g"]["offx"], c["g"]["offy"], d["m"], c["g"]["ox"], c["g"]["oy"]) for c, d in zip(cases, dev)]
    extra = {} if anchors is None else dict(anchors=[None if a is None else _dev(gpu, np.asarray(a, np.int64).astype(np.int32)) for a in anchors], weight=w, cap=T)
    got = capi.dev_pairs_seam_path(pairs, cw, ch, [d["A"] for d in dev], [d["B"] for d in dev], [c["branch"] for c in cases], max_step=K, margin=MARGIN, **extra)
    return [t.cpu().numpy() for t in got]


@pytest.mark.parametrize("cw", [63, 64, 1024, 1025])
def test_anchored_finder_against_numpy(st, gpu, oracle, cw):
    for ch in (1, 2, 37):
        cases = _finder_case(oracle, cw, ch)
        dev = [{k: _dev(gpu, c[k]) for k in ("f", "m", "A", "B")} for c in cases]
        costs = [sp.cost(c["a"], c["b"], c["A"], c["B"], c["branch"], MARGIN) for c in cases]
        for K in (1, 8):
            free = [sp.dp_path(c, K) for c in costs]
            paths, D = _find(gpu, dev, cases, cw, ch, K)
            assert [p.tolist() for p in paths] == [f[0].tolist() for f in free] and D.tolist() == [f[1] for f in free]
            for w, T in OPTIONS:
                kinds = _anchor_kinds(cw, ch, K, T, [f[0] for f in free])
                kinds["mixed"] = [kinds["own"][0], None, kinds["zigzag"][2], None, kinds["walk"][4]]  # null entries beside anchored pairs
                for name, anchors in kinds.items():
                    paths, D, moved = _find(gpu, dev, cases, cw, ch, K, anchors, w, T)
                    assert paths.shape == (5, ch) and paths.dtype == np.int32 and D.shape == moved.shape == (5,)
                    for i, r in enumerate(anchors):
                        want = sa.anchored_path(costs[i], K, r, w, T)
                        at = (ch, K, w, T, name, i)
                        assert (int(D[i]), int(moved[i])) == want[1:], (at, int(D[i]), int(moved[i]), want[1:])
                        assert paths[i].tolist() == want[0].tolist(), at
                        assert int(D[i]) == sp.path_cost(costs[i], paths[i]) + w * int(moved[i]), at
                        if name == "own" or r is None:  # the path, the cost and moved = 0 come back
                            assert (paths[i].tolist(), int(D[i]), int(moved[i])) == (free[i][0].tolist(), free[i][1], 0), at
                        elif name in ("far", "ends"):  # property (c)
                            assert (paths[i].tolist(), int(D[i]), int(moved[i])) == (free[i][0].tolist(), free[i][1] + ch * w * T, ch * T), at
                        else:  # property (d)
                            assert int(moved[i]) <= sa.moved_of(free[i][0], r, T), at
                    if name != "mixed":  # flat frames under full masks: c is zero everywhere, the temporal term alone decides
                        assert not costs[3].any() and int(D[3]) == w * int(moved[3])
                        assert all(abs(int(paths[3][j]) - int(paths[3][j - 1])) <= K for j in range(1, ch))
                        if name == "walk" and w > 0 and K == 8 and cw >= 1024:  # steps of at most 3 inside the canvas: the path is the anchor
                            assert (paths[3].tolist(), int(D[3]), int(moved[3])) == (np.asarray(anchors[3]).tolist(), 0, 0)
                        if name == "zigzag" and w > 0 and ch > 1:  # steps of K + 5: the path cannot follow, and pays
                            assert int(moved[3]) > 0


def test_anchored_finder_at_the_widest_canvas(st, gpu, oracle):
    cw, ch = 8192, 4
    g = _geometry(cw, ch)
    f, m = _frames(oracle, g, 0, np.dtype("uint8"))
    a, b = oracle.warp(f, g["p"], 0.0, 0.0, cw, ch), oracle.move(m, 0, 0, cw, ch)
    A = (oracle.warp(np.full_like(f, 255), g["p"], 0.0, 0.0, cw, ch)[0] != 0).astype(np.uint8)
    B = (oracle.move(np.full_like(m, 255), 0, 0, cw, ch)[0] != 0).astype(np.uint8)
    case = dict(g=g, branch=0)
    dev = [dict(f=_dev(gpu, f), m=_dev(gpu, m), A=_dev(gpu, A), B=_dev(gpu, B))]
    cost = sp.cost(a, b, A, B, 0, MARGIN)
    for K, w, T, r in ((8, 1, 2055, [sa.INT32_MAX] * 4), (1, 32, 64, [8192, 0, 4000, sa.INT32_MIN])):
        paths, D, moved = _find(gpu, dev, [case], cw, ch, K, [r], w, T)
        want = sa.anchored_path(cost, K, r, w, T)
        assert (paths[0].tolist(), int(D[0]), int(moved[0])) == (want[0].tolist(), want[1], want[2])
    free = sp.dp_path(cost, 8)
    paths, D, moved = _find(gpu, dev, [case], cw, ch, 8, [[sa.INT32_MAX] * 4], 1, 2055)
    assert (paths[0].tolist(), int(D[0]), int(moved[0])) == (free[0].tolist(), free[1] + 4 * 2055, 4 * 2055)


def test_anchored_paths_blend(st, gpu, oracle):
    """The anchored finder's output is the pathed blend's input, device to device: the mosaic along it is blend_with_mask's."""
    cw, ch = 300, 70
    opts = sp.opts_for(oracle, cw, ch, 0, 0)
    c = _finder_case(oracle, cw, ch)[0]
    r = cw // 2 + (np.arange(ch) % 2) * 9
    pair = [(_dev(gpu, c["f"]), c["g"]["p"], 0.0, 0.0, _dev(gpu, c["m"]), 0, 0)]
    paths, costs, moved = capi.dev_pairs_seam_path(pair, cw, ch, [_dev(gpu, c["A"])], [_dev(gpu, c["B"])], [c["branch"]], max_step=2, margin=3,
                                                   anchors=[_dev(gpu, r.astype(np.int32))], weight=32, cap=64)
    want = sa.anchored_path(sp.cost(c["a"], c["b"], c["A"], c["B"], c["branch"], 3), 2, r, 32, 64)
    assert (paths[0].cpu().numpy().tolist(), int(costs[0]), int(moved[0])) == (want[0].tolist(), want[1], want[2])
    plan = capi.Plan(cw, ch, opts, masked=True)
    try:
        f = _dev(gpu, c["f"])
        got = plan.pairs([_item(c["g"], f, _dev(gpu, c["m"]), _out(gpu, c["g"], f))], paths=[paths[0]], branches=[c["branch"]])[0]
        ref = sp.blend_with_mask_as(oracle, c["a"], c["b"], sp.mask_from_path(paths[0].cpu().numpy(), c["branch"], cw), opts)
        assert _same(got.cpu().numpy(), ref)
    finally:
        plan.close()


def test_weight_zero_takes_any_cap(st, gpu, oracle):
    """w = 0 admits every cap up to INT32_MAX: `moved` is then the whole distance, up to 2^31 + cw per row, and the path the unanchored one."""
    cw, ch = 64, 2
    cases = _finder_case(oracle, cw, ch)
    dev = [{k: _dev(gpu, c[k]) for k in ("f", "m", "A", "B")} for c in cases]
    anchors = [[sa.INT32_MIN, sa.INT32_MAX], [sa.INT32_MAX, sa.INT32_MIN], [-7, cw + 9], [sa.INT32_MIN, sa.INT32_MIN], [sa.INT32_MAX, 3]]
    paths, D, moved = _find(gpu, dev, cases, cw, ch, 2, anchors, 0, sa.INT32_MAX)
    for i, c in enumerate(cases):
        want = sa.anchored_path(sp.cost(c["a"], c["b"], c["A"], c["B"], c["branch"], MARGIN), 2, anchors[i], 0, sa.INT32_MAX)
        assert (paths[i].tolist(), int(D[i]), int(moved[i])) == (want[0].tolist(), want[1], want[2]), i


def test_finder_argument_errors(st, gpu, oracle):
    cw, ch = 64, 2
    c = _finder_case(oracle, cw, ch)[0]
    args = ([(_dev(gpu, c["f"]), c["g"]["p"], 0.0, 0.0, _dev(gpu, c["m"]), 0, 0)], cw, ch, [_dev(gpu, c["A"])], [_dev(gpu, c["B"])], [c["branch"]])
    r = _dev(gpu, np.zeros(ch, np.int32))
    for w, T in ((1, 2056), (8, 257), (4, 0), (-1, 4)):
        with pytest.raises(capi.StitchError) as e:
            capi.dev_pairs_seam_path(*args, anchors=[r], weight=w, cap=T)
        assert e.value.code == capi.ERR_ARG, (w, T)
    with pytest.raises(ValueError):
        capi.dev_pairs_seam_path(*args, anchors=[r])  # anchors come with a weight and a cap
    with pytest.raises(ValueError):
        capi.dev_pairs_seam_path(*args, anchors=[r[:1]], weight=1, cap=1)  # the wrong height


# ---- the rig on the recorded run "4" ----------------------------------------------------------------------------------------------------
K, M, W, T = 3, 4, 32, 64


def _chain(rig, frames, steps, plans, anchors, w=W, cap=T, **kw):
    cover, branches, _ = _geometry_of(rig)
    return pipeline.stitch_chain(frames, steps, plans=plans, seam_paths=dict(coverage=cover, branches=branches, max_step=K, margin=M, anchors=anchors, weight=w, cap=cap),
                                 **kw)


def _loop(rig, sets, steps, plans, key=None, anchors=None, carry=True, **kw):
    """The reference: the sets through the single-set chain one after another -- carry: each on the paths the set before it found (a
    rig that anchors per set); otherwise each on `anchors`.  -> per set the chain's return value.  Kept under `key` for the module."""
    if key is not None and key in _cache:
        return _cache[key]
    res, anchors = [], anchors if anchors is not None else [None] * len(steps)
    for frames in sets:
        res.append(_chain(rig, frames, steps, plans, anchors, **kw))
        if carry:
            anchors = [f[0] for f in res[-1][-1]]
    if key is not None:
        _cache[key] = res
    return res


def _same_found(rig, i, found):
    for k, (path, cost, moved) in enumerate(found):
        got, got_cost = rig.last_seam_paths(i, k)
        if got.tolist() != path.cpu().numpy().tolist() or got_cost != cost or rig.last_seam_moved(i, k) != moved:
            return False
    return True


def _equal(rig, got, want, i, j):
    """set i of the replay `got` is the chain result want[j]: bytes, paths, costs and moved."""
    return bool((got[0][i] == want[j][0]).all()) and _same_found(rig, i, want[j][-1])


def test_per_set_does_not_depend_on_how_the_stream_is_cut(st, gpu, plans):
    steps, sets = _run4_steps(), _run4_sets(gpu)
    rig = _rig(gpu, steps, sets).set_seam_paths(K, M)
    cut = _rig(gpu, steps, sets, max_sets=2).set_seam_paths(K, M).set_seam_anchor(W, T, "set")
    try:
        plain = rig.stitch(sets)
        free = [[rig.last_seam_paths(i, k) for k in range(3)] for i in range(3)]
        assert rig.set_seam_anchor(W, T, "set").seam_anchor() == ((W, T, "set"), False)
        want = _loop(rig, sets, steps, plans, key="per_set")
        got = rig.stitch(sets)  # one call of three sets
        assert got[1] == [0, 0, 0] and rig.seam_anchor()[1] is True
        assert all(_equal(rig, got, want, i, i) for i in range(3))
        # the first set had no anchor: it is the unanchored rig's; a later one paid for moving and differs from it somewhere
        assert bool((got[0][0] == plain[0][0]).all()) and all(rig.last_seam_moved(0, k) == 0 for k in range(3))
        assert all(rig.last_seam_paths(0, k)[0].tolist() == free[0][k][0].tolist() and rig.last_seam_paths(0, k)[1] == free[0][k][1] for k in range(3))
        assert any(rig.last_seam_paths(i, k)[0].tolist() != free[i][k][0].tolist() for i in (1, 2) for k in range(3))
        assert any(rig.last_seam_moved(i, k) > 0 for i in (1, 2) for k in range(3))
        for i in (1, 2):  # D = the path's cost under c + w * moved is at least the unanchored optimum
            assert all(rig.last_seam_paths(i, k)[1] >= free[i][k][1] for k in range(3))
        rig.reset_seam_anchor()
        for i, frames in enumerate(sets):  # three calls of one set
            one = rig.stitch([frames])
            assert one[1] == [0] and _equal(rig, one, want, 0, i), f"set {i}, fed alone"
        two = cut.stitch(sets)  # sequences of 2 + 1
        assert two[1] == [0, 0, 0] and all(_equal(cut, two, want, i, i) for i in range(3))
        again = cut.stitch(sets[:1])  # the stream goes on across calls: set 0 now anchors on set 2
        after = _chain(rig, sets[0], steps, plans, [f[0] for f in want[2][-1]])
        assert _equal(cut, again, [after], 0, 0)
    finally:
        rig.close()
        cut.close()


def test_per_call_anchors_every_set_on_the_previous_call(st, gpu, plans):
    steps, sets = _run4_steps(), _run4_sets(gpu)
    rig = _rig(gpu, steps, sets).set_seam_paths(K, M).set_seam_anchor(W, T, "call")
    cut = _rig(gpu, steps, sets, max_sets=2).set_seam_paths(K, M).set_seam_anchor(W, T, "call")
    try:
        per_set = _loop(rig, sets, steps, plans, key="per_set")
        first = [f[0] for f in per_set[0][-1]]  # set 0, unanchored
        want = _loop(rig, sets, steps, plans, anchors=first, carry=False)  # three stand-alone chains, each on set 0's paths
        for r in (rig, cut):
            one = r.stitch(sets[:1])
            assert _equal(r, one, per_set, 0, 0) and r.seam_anchor() == ((W, T, "call"), True)
            got = r.stitch(sets)  # a call of three sets after a call of one
            assert got[1] == [0, 0, 0] and all(_equal(r, got, want, i, i) for i in range(3))
        # with one set per call the two policies coincide; and so does the first set of a longer call
        rig.reset_seam_anchor()
        for i, frames in enumerate(sets):
            one = rig.stitch([frames])
            assert _equal(rig, one, per_set, 0, i), f"set {i}, fed alone"
        rig.reset_seam_anchor().stitch(sets[:1])
        got = rig.stitch(sets[1:])  # a call of two sets after a call of one: both anchor on set 0
        assert _equal(rig, got, per_set, 0, 1) and _equal(rig, got, want, 1, 2)
        last = _chain(rig, sets[0], steps, plans, [f[0] for f in want[2][-1]])  # then the anchor is the call's last set
        assert _equal(rig, rig.stitch(sets[:1]), [last], 0, 0)
    finally:
        rig.close()
        cut.close()


def test_anchor_handling(st, gpu, plans):
    steps, sets = _run4_steps(), _run4_sets(gpu)
    rig = _rig(gpu, steps, sets)
    try:
        before = rig.stitch(sets)
        plain = rig.set_seam_paths(K, M).stitch(sets)
        free = [[rig.last_seam_paths(i, k) for k in range(3)] for i in range(3)]
        # weight 0 is mode 1 without an anchor: bytes, paths and costs
        zero = rig.set_seam_anchor(0, 2 ** 31 - 1, "set").stitch(sets)
        assert all(bool((a == b).all()) for a, b in zip(zero[0], plain[0])) and zero[1:] == plain[1:]
        for i in range(3):
            for k in range(3):
                path, cost = rig.last_seam_paths(i, k)
                assert path.tolist() == free[i][k][0].tolist() and cost == free[i][k][1]
        # after a reset the next first set is the unanchored rig's
        rig.set_seam_anchor(W, T, "set").stitch(sets)
        assert rig.seam_anchor() == ((W, T, "set"), True) and rig.reset_seam_anchor().seam_anchor() == ((W, T, "set"), False)
        one = rig.stitch(sets[:1])
        assert bool((one[0][0] == plain[0][0]).all()) and all(rig.last_seam_paths(0, k)[0].tolist() == free[0][k][0].tolist() for k in range(3))
        assert all(rig.last_seam_moved(0, k) == 0 and rig.last_seam_paths(0, k)[1] == free[0][k][1] for k in range(3))
        # primed with set 0's own unanchored paths, set 0 returns them with moved = 0
        rig.reset_seam_anchor().prime_seam_anchor([free[0][k][0] for k in range(3)])
        assert rig.seam_anchor()[1] is True
        one = rig.stitch(sets[:1])
        assert bool((one[0][0] == plain[0][0]).all())
        assert all(rig.last_seam_paths(0, k)[0].tolist() == free[0][k][0].tolist() and rig.last_seam_paths(0, k)[1] == free[0][k][1] and rig.last_seam_moved(0, k) == 0
                   for k in range(3))
        # primed with a far anchor every path pays the full cap on every row
        far = [np.full(s["ch"], s["cw"] + T + 5, np.int32) for s in steps]
        rig.set_seam_anchor(W, T, "call").prime_seam_anchor(far)
        got = rig.stitch(sets)
        assert all(bool((a == b).all()) for a, b in zip(got[0], plain[0]))
        for i in range(3):
            for k, s in enumerate(steps):
                assert rig.last_seam_moved(i, k) == s["ch"] * T and rig.last_seam_paths(i, k)[1] == free[i][k][1] + s["ch"] * W * T
        # after clear_seam_anchor every byte equals mode 1 before, after clear_seam_paths the rig before any mode
        after = rig.clear_seam_anchor().stitch(sets)
        assert rig.seam_anchor() == (None, False) and all(bool((a == b).all()) for a, b in zip(after[0], plain[0])) and after[1:] == plain[1:]
        assert all(rig.last_seam_paths(i, k)[0].tolist() == free[i][k][0].tolist() and rig.last_seam_moved(i, k) == 0 for i in range(3) for k in range(3))
        rig.set_seam_anchor(W, T, "set").stitch(sets)
        assert rig.seam_anchor()[1] is True and rig.clear_seam_paths().seam_anchor() == ((W, T, "set"), False)
        after = rig.stitch(sets)
        assert all(bool((a == b).all()) for a, b in zip(after[0], before[0])) and after[1:] == before[1:]
        # fixed paths (mode 2) ignore the options
        fixed = rig.fix_seam_paths([free[0][k][0] for k in range(3)]).stitch(sets)
        assert bool((fixed[0][0] == plain[0][0]).all()) and rig.seam_anchor() == ((W, T, "set"), False) and rig.last_seam_moved(2, 1) == 0
    finally:
        rig.close()


def test_anchored_with_an_exposure_template(st, gpu, plans):
    steps, sets = _run4_steps(), _run4_sets(gpu)[:2]
    rig = _rig(gpu, steps, sets, exposure=1).set_seam_paths(K, M).set_seam_anchor(W, T, "set")
    try:
        got = rig.stitch(sets, return_stats=True)
        want = _loop(rig, sets, steps, plans, exposure=1)
        assert got[1] == [0, 0] and all(_equal(rig, got, want, i, i) for i in range(2))
    finally:
        rig.close()


def test_anchored_with_formats(st, gpu, plans):
    import pixfmt_ref as pf
    from test_gpu_pixfmt import from_dev, same_image, to_dev
    steps, sets = _run4_steps(), _run4_sets(gpu)[:2]
    rig = _rig(gpu, steps, sets).set_formats(pf.BGR24, pf.NV12, 1).set_seam_paths(K, M).set_seam_anchor(W, T, "set")
    try:
        packed = [[to_dev(pf.pack(f.cpu().numpy(), pf.BGR24, 1), gpu) for f in frames] for frames in sets]
        got = rig.stitch(packed)
        want = _loop(rig, packed, steps, plans, formats=(pf.BGR24, pf.NV12, 1))
        assert got[1] == [0, 0]
        for i in range(2):
            assert same_image(from_dev(want[i][0]), from_dev(got[0][i])) and _same_found(rig, i, want[i][-1]), f"set {i}"
    finally:
        rig.close()


def test_anchored_with_a_crop_and_a_monitor(st, gpu, plans):
    steps, sets = _run4_steps(), _run4_sets(gpu)[:2]
    rig = _rig(gpu, steps, sets).set_crop(mode=2).set_monitor(2).set_seam_paths(K, M).set_seam_anchor(W, T, "call")
    try:
        rig.prime_seam_anchor([np.full(s["ch"], s["cw"] // 2, np.int32) for s in steps])
        got = rig.stitch(sets)
        res = rig.residuals()
        assert got[1] == [0, 0] and res.shape[:2] == (2, 3)
        domains = [rig.residual_domain(k) for k in range(3)]
        want = _loop(rig, sets, steps, plans, anchors=[np.full(s["ch"], s["cw"] // 2, np.int32) for s in steps], carry=False, crop=rig.crop,
                     residuals=dict(radius=2, domains=domains))
        for i in range(2):
            assert _equal(rig, got, want, i, i), f"set {i}"
            assert np.array_equal(want[i][1].cpu().numpy().astype(np.int64), res[i].astype(np.int64))
    finally:
        rig.close()


def test_a_failed_replay_leaves_no_anchor(st, gpu):
    import torch
    import rig_seams_ref as ref
    sizes, steps, want = ref.failure_cases(capi)["no_overlap"]
    sets = [[capi.dev_synth(w, h, 3 * i + f, torch.uint8, gpu) for f, (w, h) in enumerate(sizes)] for i in range(2)]
    rig = capi.Rig.from_steps(sizes, 0, steps)
    try:
        rig.set_seam_paths(2, 8).set_seam_anchor(4, 16, "set").prime_seam_anchor([np.full(s["ch"], s["cw"] // 2, np.int32) for s in steps])
        assert rig.seam_anchor() == ((4, 16, "set"), True)
        rig.stitch(sets)
        assert rig.last_rc == want and b"step 1" in capi.lib().stitch_last_error()
        assert rig.seam_anchor() == ((4, 16, "set"), False)  # a half-written chain must not steer the next call
        with pytest.raises(capi.StitchError):
            rig.last_seam_moved(0, 0)
    finally:
        rig.close()


def test_rig_argument_errors(st, gpu):
    steps, sets = _run4_steps(), _run4_sets(gpu)
    rig = _rig(gpu, steps, sets).set_seam_paths(K, M)
    L = capi.lib()
    try:
        for w, cap in ((1, 2056), (8, 257), (4, 0), (-1, 4)):
            with pytest.raises(capi.StitchError) as e:
                rig.set_seam_anchor(w, cap)
            assert e.value.code == capi.ERR_ARG and rig.seam_anchor() == (None, False)
        for policy in (0, 3):
            with pytest.raises(capi.StitchError) as e:
                rig.set_seam_anchor(1, 1, policy)
            assert e.value.code == capi.ERR_ARG and rig.seam_anchor() == (None, False)
        with pytest.raises(capi.StitchError):
            rig.prime_seam_anchor([np.zeros(s["ch"], np.int32) for s in steps[:2]])  # two paths for three steps
        with pytest.raises(ValueError):
            rig.prime_seam_anchor([np.zeros(5, np.int32)] * 3)  # the wrong height
        assert L.stitch_rig_prime_seam_anchor(rig._h, (C.c_void_p * 3)(0x1000, None, 0x1000), 3) == L.stitch_rig_prime_seam_anchor(rig._h, None, 3) == capi.ERR_ARG
        o, moved = capi.SeamAnchorOpts(1, 1, 1), C.c_uint64()
        assert L.stitch_rig_set_seam_anchor(None, C.byref(o)) == L.stitch_rig_set_seam_anchor(rig._h, None) == L.stitch_rig_prime_seam_anchor(None, None, 0) \
            == L.stitch_rig_reset_seam_anchor(None) == L.stitch_rig_clear_seam_anchor(None) == L.stitch_rig_seam_anchor(None, None, None) \
            == L.stitch_rig_last_seam_moved(None, 0, 0, C.byref(moved)) == capi.ERR_ARG
        assert L.stitch_rig_last_seam_moved(rig._h, 0, 0, C.byref(moved)) == capi.ERR_ARG and rig.seam_anchor() == (None, False)  # no replay yet
        rig.stitch(sets[:1])
        assert rig.last_seam_moved(0, 2) == 0 and L.stitch_rig_last_seam_moved(rig._h, 1, 0, C.byref(moved)) == L.stitch_rig_last_seam_moved(rig._h, 0, 3, C.byref(moved)) \
            == L.stitch_rig_last_seam_moved(rig._h, 0, 0, None) == capi.ERR_ARG
    finally:
        rig.close()
