"""GPU: path seams for pairs and rigs (include/stitch_seam_path.h, csrc/stitch_seam_path.inc, stitch_rig_seam_paths.inc,
k_seam_path.inc).  Everything is exact, bytes and integers.  The yardsticks: a path whose columns are all equal is the vertical
seam, so its blend is stitch_dev_pairs_seamed_*'s, byte for byte; any other path against tests/seam_path_ref.py's blend_with_mask on
the CPU oracle (pinned to Oracle.blend by tests/test_seam_path_host.py); the finder against the same module's cost and dynamic
programme; the rig on the recorded run "4" against pipeline.stitch_chain(seam_paths=...) set by set, bytes, paths and costs."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import seam_path_ref as sp
from computervisionimagestich2_amd import bmp, capi, pipeline

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
_cache = {}


def _same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and bool((a == b).all())


def _bits(t):
    a = t.cpu().numpy()
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _geometry(cw, ch, k=0):
    """Pair k on a cw x ch canvas: the frame (two thirds of the canvas wide) is warped to the canvas's right part by a map that bends
    a little more with k, the mosaic (as wide) lies at the left edge -- the middle third is the overlap."""
    fw = mw = max(2, (2 * cw + 2) // 3)
    p = [1.0, 0.002 * (k + 1), 1e-6 * k, -float(cw - fw), -0.001 * k, 1.0, 5e-7 * k, 0.25 * k]
    return dict(fw=fw, fh=ch, mw=mw, mh=ch, p=p, offx=0.0, offy=0.0, ox=0, oy=0, cw=cw, ch=ch)


def _frames(oracle, g, k, dtype):
    """numpy frame and mosaic of pair k, no sample 0 (the scan of the ordinary calls finds a seam at any size)."""
    f, m = oracle.synth(g["fw"], g["fh"], 2 * k + 1, dtype), oracle.synth(g["mw"], g["mh"], 2 * k, dtype)
    return np.maximum(f, 1).astype(dtype), np.maximum(m, 1).astype(dtype)


def _item(g, frame, mosaic, out):
    return (frame, g["p"], g["offx"], g["offy"], mosaic, g["ox"], g["oy"], out)


def _dev(gpu, a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(gpu)


def _out(gpu, g, like, fill=0):
    import torch
    return torch.full((3, g["ch"], g["cw"]), fill, dtype=like.dtype, device=gpu)


def _status(plan, i):
    s = capi.Seam()
    return capi.lib().stitch_plan_status_at(plan._h, i, C.byref(s)), s


# ---- constant paths: the vertical seam, byte for byte --------------------------------------------------------------------------------
CONSTANT = [(3, 2, 1), (97, 61, 1), (300, 70, 1), (301, 71, 1), (520, 130, 1), (1024, 1024, 2), (1088, 1030, 2)]


@pytest.mark.parametrize("dtype", ["uint8", "float32"])
@pytest.mark.parametrize("cw,ch,n", CONSTANT, ids=[f"{c[0]}x{c[1]}" for c in CONSTANT])
def test_constant_paths_are_the_vertical_seam(st, gpu, oracle, cw, ch, n, dtype):
    npd = np.dtype(dtype)
    blur_kinds = (0, 1) if cw < 1000 else (0,)
    for blur_kind in blur_kinds:
        for seam_rule in (0, 1):
            opts = sp.opts_for(oracle, cw, ch, blur_kind, seam_rule)
            geo = [_geometry(cw, ch, k) for k in range(n)]
            ins = [tuple(_dev(gpu, a) for a in _frames(oracle, geo[k], k, npd)) for k in range(n)]
            if n == 2:  # another content seam for the second pair: dark columns of channel 0 in its overlap
                ins[1][0][0, :, : cw // 20] = 0
            plain = capi.Plan(cw, ch, opts, max_pairs=n)
            masked = capi.Plan(cw, ch, opts, max_pairs=n, masked=True)
            try:
                assert capi.lib().stitch_plan_is_masked(masked._h) == 1 and capi.lib().stitch_plan_is_masked(plain._h) == 0
                assert not {"implicit_mask", "source_fused"} & masked.fast_paths
                assert plain.levels == masked.levels and (plain.level_w, plain.level_h) == (masked.level_w, masked.level_h)
                if cw >= 1024:  # the fused sweep is reached, with the mask plane as a plane like the others
                    assert masked.fused_sweep_levels >= 1 and "fused_sweep" in masked.call_forms(2)
                if (cw, ch) == (3, 2):
                    assert masked.levels == 1
                plain.pairs([_item(g, f, m, _out(gpu, g, f)) for g, (f, m) in zip(geo, ins)])
                recs = [_status(plain, i) for i in range(n)]
                assert all(rc == 0 for rc, _ in recs)
                seams = [s.as_tuple() for _, s in recs]
                want = plain.pairs([_item(g, f, m, _out(gpu, g, f, 7)) for g, (f, m) in zip(geo, ins)], seams=seams)
                assert all(_status(plain, i)[0] == 0 for i in range(n))
                # an unmasked plan refuses paths
                paths = [_dev(gpu, sp.constant_path(s, seam_rule, ch)) for _, s in recs]
                branches = [s.branch for _, s in recs]
                with pytest.raises(capi.StitchError) as e:
                    plain.pairs([_item(g, f, m, _out(gpu, g, f)) for g, (f, m) in zip(geo, ins)], paths=paths, branches=branches)
                assert e.value.code == capi.ERR_ARG
                for kw in (dict(), dict(seams=seams)):  # ... and a masked plan the calls without them
                    with pytest.raises(capi.StitchError) as e:
                        masked.pairs([_item(g, f, m, _out(gpu, g, f)) for g, (f, m) in zip(geo, ins)], **kw)
                    assert e.value.code == capi.ERR_ARG
                canvas = _out(gpu, geo[0], ins[0][0], 1)
                with pytest.raises(capi.StitchError) as e:
                    masked.blend(canvas, canvas)
                assert e.value.code == capi.ERR_ARG
                got = masked.pairs([_item(g, f, m, _out(gpu, g, f, 9)) for g, (f, m) in zip(geo, ins)], paths=paths, branches=branches)
                for i in range(n):  # STITCH_OK and a zeroed record that carries the branch
                    rc, s = _status(masked, i)
                    assert rc == 0 and s.as_tuple() == (0, 0, 0, 0, branches[i], 0) and s.ratio == 0 and s.ov == 0
                for i in range(n):
                    assert _same(_bits(got[i]), _bits(want[i])), (blur_kind, seam_rule, i, int((_bits(got[i]) != _bits(want[i])).sum()))
                if n == 2:
                    assert seams[0] != seams[1]
            finally:
                plain.close()
                masked.close()


# ---- other paths: against blend_with_mask on the CPU oracle --------------------------------------------------------------------------
def _paths(cw, ch, seed):
    """zigzag of +-1, a seeded random walk, all 0, all cw, and -5 with cw + 7"""
    rng = np.random.default_rng(seed)
    y = np.arange(ch)
    walk = np.clip(cw // 2 + np.cumsum(rng.integers(-3, 4, ch)), -2, cw + 2)
    return [(cw // 2 + (y & 1)).astype(np.int32), walk.astype(np.int32), np.zeros(ch, np.int32), np.full(ch, cw, np.int32),
            np.where(y % 3 == 0, -5, cw + 7).astype(np.int32)]


def _reference(oracle, cw, ch, dtype, opts, flip):
    """Five pairs with the five paths: numpy frames, paths, branches and blend_with_mask's images; computed once per case."""
    key = ("ref", cw, ch, dtype, tuple(sorted(opts.items())), flip)
    if key not in _cache:
        npd = np.dtype(dtype)
        geo = [_geometry(cw, ch, k) for k in range(5)]
        frames = [_frames(oracle, g, k, npd) for k, g in enumerate(geo)]
        paths = _paths(cw, ch, cw + ch)
        branches = [(k + flip) & 1 for k in range(5)]
        want = []
        for g, (f, m), path, br in zip(geo, frames, paths, branches):
            a = oracle.warp(f, g["p"], g["offx"], g["offy"], cw, ch)
            b = oracle.move(m, g["ox"], g["oy"], cw, ch)
            want.append(sp.blend_with_mask_as(oracle, a, b, sp.mask_from_path(path, br, cw), opts))
        _cache[key] = (geo, frames, paths, branches, want)
    return _cache[key]


@pytest.mark.parametrize("flip", [0, 1])
@pytest.mark.parametrize("dtype", ["uint8", "float32"])
@pytest.mark.parametrize("cw,ch", [(97, 61), (300, 70), (520, 130)], ids=lambda v: str(v))
def test_paths_against_the_oracle(st, gpu, oracle, cw, ch, dtype, flip):
    opts = sp.opts_for(oracle, cw, ch, flip, flip)  # Van Vliet under seam rule 0, Deriche under rule 1 (no seam is scanned either way)
    geo, frames, paths, branches, want = _reference(oracle, cw, ch, dtype, opts, flip)
    plan = capi.Plan(cw, ch, opts, max_pairs=5, masked=True)
    try:
        ins = [(_dev(gpu, f), _dev(gpu, m)) for f, m in frames]
        got = plan.pairs([_item(g, f, m, _out(gpu, g, f, 3)) for g, (f, m) in zip(geo, ins)], paths=[_dev(gpu, p) for p in paths], branches=branches)
        assert all(_status(plan, i)[0] == 0 for i in range(5))
        for i in range(5):
            g_, w_ = _bits(got[i]), (want[i].view(np.uint32) if want[i].dtype == np.float32 else want[i])
            print(f"{cw}x{ch} {dtype} flip {flip} pair {i}: {int((g_ != w_).sum())} of {w_.size} samples differ")
            assert _same(g_, w_), (i, int((g_ != w_).sum()))
    finally:
        plan.close()


@pytest.mark.parametrize("dtype", ["uint8", "float32"])
def test_two_pairs_in_a_call_are_the_pairs_alone(st, gpu, oracle, dtype):
    cw = ch = 1024
    npd = np.dtype(dtype)
    geo = [_geometry(cw, ch, k) for k in range(2)]
    ins = [tuple(_dev(gpu, a) for a in _frames(oracle, geo[k], k, npd)) for k in range(2)]
    all_paths = _paths(cw, ch, 5)
    plan = capi.Plan(cw, ch, max_pairs=2, masked=True)
    try:
        assert "fused_sweep" in plan.call_forms(2) and "fused_sweep" not in plan.call_forms(1)
        for pa, pb, branches in ((0, 1, (0, 1)), (4, 1, (1, 0)), (2, 3, (0, 0))):
            paths = [_dev(gpu, all_paths[pa]), _dev(gpu, all_paths[pb])]
            both = plan.pairs([_item(g, f, m, _out(gpu, g, f, 1)) for g, (f, m) in zip(geo, ins)], paths=paths, branches=branches)
            for i in range(2):
                alone = plan.pairs([_item(geo[i], ins[i][0], ins[i][1], _out(gpu, geo[i], ins[i][0], 2))], paths=[paths[i]], branches=[branches[i]])[0]
                assert _status(plan, 0)[0] == 0
                assert _same(_bits(both[i]), _bits(alone)), (pa, pb, i)
    finally:
        plan.close()


def test_pathed_argument_errors(st, gpu):
    import torch
    g = _geometry(64, 48)
    f = torch.ones((3, g["fh"], g["fw"]), dtype=torch.uint8, device=gpu)
    plan = capi.Plan(64, 48, max_pairs=2, masked=True)
    L = capi.lib()
    try:
        arr = (capi.PairDesc * 3)()
        outs = [_out(gpu, g, f) for _ in arr]
        for d, o in zip(arr, outs):
            d.frame, d.fw, d.fh, d.mosaic, d.mw, d.mh, d.out = f.data_ptr(), g["fw"], g["fh"], f.data_ptr(), g["mw"], g["mh"], o.data_ptr()
            d.p = capi._map8(g["p"])
        path = torch.zeros(48, dtype=torch.int32, device=gpu)
        tab, br = (C.c_void_p * 3)(*[path.data_ptr()] * 3), (C.c_int32 * 3)(0, 1, 0)
        call = L.stitch_dev_pairs_pathed_u8
        assert call(plan._h, None, 1, tab, br, None) == call(plan._h, arr, 1, None, br, None) == call(plan._h, arr, 1, tab, None, None) == capi.ERR_ARG
        assert call(plan._h, arr, 0, tab, br, None) == call(plan._h, arr, 3, tab, br, None) == capi.ERR_ARG  # n out of range
        assert call(plan._h, arr, 2, (C.c_void_p * 2)(path.data_ptr(), None), br, None) == capi.ERR_ARG
        assert call(plan._h, arr, 2, tab, (C.c_int32 * 2)(0, 2), None) == capi.ERR_ARG
        assert call(plan._h, arr, 2, tab, br, None) == 0 and _status(plan, 1)[0] == 0
        with pytest.raises(ValueError):
            plan.pairs([_item(g, f, f, _out(gpu, g, f))], paths=[path[:-1].contiguous()], branches=[0])
        with pytest.raises(ValueError):
            plan.pairs([_item(g, f, f, _out(gpu, g, f))], paths=[path])
    finally:
        plan.close()


# ---- the finder ------------------------------------------------------------------------------------------------------------------------
def _finder_case(oracle, cw, ch):
    """Five pairs on a cw x ch canvas, five maps, with the numpy canvases their costs are stated on.  The frame lies right of the
    mosaic, so branch 1 (a where x >= s) is the side a seam belongs to: 0 true footprints; 1 flat frames under a slanted overlap,
    where a path can be free of cost only by leaning; 2 rows without coverage; 3 flat frames under full masks, where everything
    ties; 4 the other branch, where every column pays."""
    key = ("finder", cw, ch)
    if key in _cache:
        return _cache[key]
    geo = [_geometry(cw, ch, k) for k in range(5)]
    frames = [_frames(oracle, g, k, np.dtype("uint8")) for k, g in enumerate(geo)]
    for k, v in ((1, 100), (3, 0)):  # (black under full masks: the canvases agree outside the footprints too)
        frames[k] = (np.full_like(frames[k][0], v), np.full_like(frames[k][1], v))
    x, y = np.meshgrid(np.arange(cw), np.arange(ch))
    cases = []
    for k, (g, (f, m)) in enumerate(zip(geo, frames)):
        a = oracle.warp(f, g["p"], g["offx"], g["offy"], cw, ch)
        b = oracle.move(m, g["ox"], g["oy"], cw, ch)
        A = (oracle.warp(np.full_like(f, 255), g["p"], g["offx"], g["offy"], cw, ch)[0] != 0).astype(np.uint8)
        B = (oracle.move(np.full_like(m, 255), g["ox"], g["oy"], cw, ch)[0] != 0).astype(np.uint8)
        if k == 1:  # the overlap leans: a's footprint starts later row by row, b's ends later
            A &= (x >= cw // 3 + y // 2).astype(np.uint8)
            B &= (x < cw // 2 + y // 2).astype(np.uint8)
        if k == 2:  # rows nobody covers, a row only a covers, a row only b covers
            A[ch // 2:ch // 2 + 3] = 0
            B[ch // 2:ch // 2 + 2] = 0
            A[0] = 0
        if k == 3:
            A[:], B[:] = 255, 1
        cases.append(dict(g=g, f=f, m=m, a=a, b=b, A=A, B=B, branch=1 if k < 3 else 0))
    _cache[key] = cases
    return cases


def _find(gpu, cases, cw, ch, K, m):
    pairs = [(_dev(gpu, c["f"]), c["g"]["p"], c["g"]["offx"], c["g"]["offy"], _dev(gpu, c["m"]), c["g"]["ox"], c["g"]["oy"]) for c in cases]
    paths, costs = capi.dev_pairs_seam_path(pairs, cw, ch, [_dev(gpu, c["A"]) for c in cases], [_dev(gpu, c["B"]) for c in cases],
                                            [c["branch"] for c in cases], max_step=K, margin=m)
    return paths.cpu().numpy(), costs.cpu().numpy()


@pytest.mark.parametrize("cw", [63, 64, 1023, 1024, 1025])
def test_finder_against_numpy(st, gpu, oracle, cw):
    for ch in (1, 2, 37):
        cases = _finder_case(oracle, cw, ch)
        for K in (1, 8):
            for m in (0, 5):
                paths, costs = _find(gpu, cases, cw, ch, K, m)
                assert paths.shape == (5, ch) and paths.dtype == np.int32 and costs.shape == (5,)
                for i, c in enumerate(cases):
                    cost = sp.cost(c["a"], c["b"], c["A"], c["B"], c["branch"], m)
                    want_path, want_cost = sp.dp_path(cost, K)
                    assert int(costs[i]) == want_cost, (ch, K, m, i, int(costs[i]), want_cost)
                    assert paths[i].tolist() == want_path.tolist(), (ch, K, m, i)
                    assert want_cost == sp.path_cost(cost, paths[i]) <= int(cost.sum(axis=0).min())  # no constant column is cheaper
                assert paths[3].tolist() == [0] * ch and int(costs[3]) == 0  # flat frames, full masks: every state ties at 0
                if m == 0:  # the slanted overlap: the path is free of cost; on the narrow canvases no constant column is
                    c = cases[1]
                    assert int(costs[1]) == 0
                    if ch == 37 and cw <= 64:
                        assert int(sp.cost(c["a"], c["b"], c["A"], c["B"], 1, 0).sum(axis=0).min()) >= sp.WRONG and len(set(paths[1].tolist())) > 1


def test_finder_at_the_widest_canvas(st, gpu, oracle):
    cw, ch = 8192, 4
    g = _geometry(cw, ch)
    f, m = _frames(oracle, g, 0, np.dtype("uint8"))
    a, b = oracle.warp(f, g["p"], 0.0, 0.0, cw, ch), oracle.move(m, 0, 0, cw, ch)
    A = (oracle.warp(np.full_like(f, 255), g["p"], 0.0, 0.0, cw, ch)[0] != 0).astype(np.uint8)
    B = (oracle.move(np.full_like(m, 255), 0, 0, cw, ch)[0] != 0).astype(np.uint8)
    case = dict(g=g, f=f, m=m, a=a, b=b, A=A, B=B, branch=0)
    for K, margin in ((8, 64), (1, 0)):
        paths, costs = _find(gpu, [case], cw, ch, K, margin)
        want_path, want_cost = sp.dp_path(sp.cost(a, b, A, B, 0, margin), K)
        assert int(costs[0]) == want_cost and paths[0].tolist() == want_path.tolist()
    # one column more is refused
    with pytest.raises(capi.StitchError) as e:
        capi.dev_pairs_seam_path([(_dev(gpu, f), g["p"], 0.0, 0.0, _dev(gpu, m), 0, 0)], cw + 1, ch, [_dev(gpu, np.zeros((ch, cw + 1), np.uint8))],
                                 [_dev(gpu, np.zeros((ch, cw + 1), np.uint8))], [0])
    assert e.value.code == capi.ERR_ARG


def test_found_paths_blend(st, gpu, oracle):
    """The finder's output is the pathed blend's input, device to device: the mosaic along the found path is blend_with_mask's."""
    cw, ch = 300, 70
    opts = sp.opts_for(oracle, cw, ch, 0, 0)
    c = _finder_case(oracle, cw, ch)[1]
    paths, costs = capi.dev_pairs_seam_path([(_dev(gpu, c["f"]), c["g"]["p"], 0.0, 0.0, _dev(gpu, c["m"]), 0, 0)], cw, ch, [_dev(gpu, c["A"])], [_dev(gpu, c["B"])],
                                            [c["branch"]], max_step=2, margin=3)
    plan = capi.Plan(cw, ch, opts, masked=True)
    try:
        f = _dev(gpu, c["f"])
        got = plan.pairs([_item(c["g"], f, _dev(gpu, c["m"]), _out(gpu, c["g"], f))], paths=[paths[0]], branches=[c["branch"]])[0]
        want = sp.blend_with_mask_as(oracle, c["a"], c["b"], sp.mask_from_path(paths[0].cpu().numpy(), c["branch"], cw), opts)
        assert _same(got.cpu().numpy(), want)
    finally:
        plan.close()


# ---- the rig on the recorded run "4": four 384 x 512 frames, three steps ---------------------------------------------------------------
@pytest.fixture(scope="module")
def plans():
    """The chains' workspaces, one per canvas size and kind, kept for the module."""
    kept = {}
    yield kept
    pipeline.close_plans(kept)


def _run4_steps():
    with open(os.path.join(GOLD, "golden.json")) as f:
        steps = json.load(f)["runs"]["4"]["steps"]
    with open(os.path.join(GOLD, "exposure.json")) as f:
        rec = json.load(f)["runs"]["4"]["mode1_keep_black1"]["steps"]
    return [dict(s, mosaic_src=r["mosaic_src"]) for s, r in zip(steps, rec)]


def _run4_sets(gpu):
    """Three sets: the committed frames; the same with the last step's warped frame rolled by (2, 3) pixels; a darker, flatter scene."""
    import torch
    if "sets" not in _cache:
        base = [torch.from_numpy(np.ascontiguousarray(bmp.load_bmp(os.path.join(GOLD, "input", f"{i}.bmp")))).to(gpu) for i in range(1, 5)]
        moved = list(base)
        last = _run4_steps()[-1]["src"]
        moved[last] = torch.roll(base[last], shifts=(3, 2), dims=(1, 2)).contiguous()
        _cache["sets"] = [base, moved, [(f // 2 + 40).contiguous() for f in base]]
    return _cache["sets"]


def _sizes(frames):
    return [(f.shape[2], f.shape[1]) for f in frames]


def _geometry_of(rig):
    """-> (the coverage masks (A, B) of every step, the branches of the geometric seams, those seams) of a rig like `rig`."""
    if getattr(rig, "_geo", None) is None:
        cover = [(rig.coverage(k, 0), rig.coverage(k, 1)) for k in range(rig.n_steps)]
        twin = capi.Rig.from_steps(rig._sizes, None, rig._steps)  # (on a twin: fixing them on `rig` would change what clear returns to)
        try:
            geo = twin.geometric_seams().seams
        finally:
            twin.close()
        rig._geo = (cover, [g[4] for g in geo], geo)
    return rig._geo


def _rig(gpu, steps, sets, **kw):
    rig = capi.Rig.from_steps(_sizes(sets[0]), None, steps, **kw)
    rig._sizes, rig._steps = _sizes(sets[0]), steps
    return rig


def _chain(rig, frames, steps, plans, K, m, paths=None, **kw):
    cover, branches, _ = _geometry_of(rig)
    return pipeline.stitch_chain(frames, steps, plans=plans, seam_paths=dict(coverage=cover, branches=branches, max_step=K, margin=m, paths=paths), **kw)


def _same_paths(rig, i, found):
    for k, (path, cost) in enumerate(found):
        got, got_cost = rig.last_seam_paths(i, k)
        if got.tolist() != path.cpu().numpy().tolist() or (cost is not None and got_cost != cost):
            return False
    return True


def test_the_rig_with_found_paths(st, gpu, plans):
    steps, sets = _run4_steps(), _run4_sets(gpu)
    rig = _rig(gpu, steps, sets)
    try:
        assert rig.seam_paths is None
        before = rig.stitch(sets)
        assert rig.set_seam_paths(3, 4).seam_paths == ("found", 3, 4)
        got = rig.stitch(sets)
        _, _, geo = _geometry_of(rig)
        assert got[1] == [0, 0, 0] and got[2] == [geo] * 3  # the geometric records, every set_status OK
        paths_of = []
        for i, frames in enumerate(sets):
            out, found = _chain(rig, frames, steps, plans, 3, 4)
            assert bool((out == got[0][i]).all()) and _same_paths(rig, i, found), f"set {i}"
            assert all(cost < 2 ** 44 for _, cost in found)
            paths_of.append([p.cpu().numpy() for p, _ in found])
        assert any(len(set(p.tolist())) > 1 for p in paths_of[0])  # a path that is no vertical line
        assert not all(np.array_equal(a, b) for a, b in zip(paths_of[0], paths_of[1]))  # every set from its own pixels
        assert not bool((got[0][0] == before[0][0]).all())
        # paths found on one set, then fixed, reproduce that set's output
        assert rig.fix_seam_paths(paths_of[0]).seam_paths == ("fixed",)
        fixed = rig.stitch(sets)
        assert fixed[1] == [0, 0, 0] and fixed[2] == got[2] and bool((fixed[0][0] == got[0][0]).all())
        for i, frames in enumerate(sets):
            out, found = _chain(rig, frames, steps, plans, 3, 4, paths=paths_of[0])
            assert bool((out == fixed[0][i]).all()) and _same_paths(rig, i, found), f"set {i}, fixed"
        assert rig.last_seam_paths(2, 1)[1] == 0
        # after clear, every byte equals the same rig before paths were set
        after = rig.clear_seam_paths().stitch(sets)
        assert rig.seam_paths is None
        assert all(bool((a == b).all()) for a, b in zip(before[0], after[0])) and before[1:] == after[1:]
        with pytest.raises(capi.StitchError):
            rig.last_seam_paths(0, 0)
    finally:
        rig.close()


def test_the_rig_with_an_exposure_template(st, gpu, plans):
    steps, sets = _run4_steps(), _run4_sets(gpu)
    rig = _rig(gpu, steps, sets, exposure=1).set_seam_paths(2, 8)
    try:
        got = rig.stitch(sets, return_stats=True)
        assert got[1] == [0, 0, 0]
        for i, frames in enumerate(sets):
            out, found = _chain(rig, frames, steps, plans, 2, 8, exposure=1)
            assert bool((out == got[0][i]).all()) and _same_paths(rig, i, found), f"set {i}"
    finally:
        rig.close()


def test_the_rig_with_formats(st, gpu, plans):
    import pixfmt_ref as pf
    from test_gpu_pixfmt import from_dev, same_image, to_dev
    steps, sets = _run4_steps(), _run4_sets(gpu)[:2]
    rig = _rig(gpu, steps, sets).set_formats(pf.BGR24, pf.NV12, 1).set_seam_paths(2, 8)
    try:
        packed = [[to_dev(pf.pack(f.cpu().numpy(), pf.BGR24, 1), gpu) for f in frames] for frames in sets]
        got = rig.stitch(packed)
        assert got[1] == [0, 0]
        for i, frames in enumerate(packed):
            out, found = _chain(rig, frames, steps, plans, 2, 8, formats=(pf.BGR24, pf.NV12, 1))
            assert same_image(from_dev(out), from_dev(got[0][i])) and _same_paths(rig, i, found), f"set {i}"
    finally:
        rig.close()


def test_the_rig_with_a_crop(st, gpu, plans):
    steps, sets = _run4_steps(), _run4_sets(gpu)[:2]
    rig = _rig(gpu, steps, sets).set_crop(mode=2).set_seam_paths(2, 8)
    try:
        got = rig.stitch(sets)
        assert got[1] == [0, 0] and tuple(got[0][0].shape) == (3, rig.out_height, rig.out_width) != (3, rig.height, rig.width)
        for i, frames in enumerate(sets):
            out, found = _chain(rig, frames, steps, plans, 2, 8, crop=rig.crop)
            assert bool((out == got[0][i]).all()) and _same_paths(rig, i, found), f"set {i}"
    finally:
        rig.close()


def test_the_rig_with_a_monitor(st, gpu, plans):
    steps, sets = _run4_steps(), _run4_sets(gpu)[:2]
    rig = _rig(gpu, steps, sets).set_monitor(2).set_seam_paths(2, 8)
    try:
        got = rig.stitch(sets)
        res = rig.residuals()
        assert got[1] == [0, 0] and res.shape[:2] == (2, 3)
        domains = [rig.residual_domain(k) for k in range(3)]
        for i, frames in enumerate(sets):
            out, rec, found = _chain(rig, frames, steps, plans, 2, 8, residuals=dict(radius=2, domains=domains))
            assert bool((out == got[0][i]).all()) and _same_paths(rig, i, found), f"set {i}"
            assert np.array_equal(rec.cpu().numpy().astype(np.int64), res[i].astype(np.int64))  # of the inputs the pathed blend received
        plain = rig.clear_monitor().stitch(sets)  # the monitor leaves the pathed outputs alone
        assert all(bool((a == b).all()) for a, b in zip(plain[0], got[0])) and plain[1:] == got[1:]
    finally:
        rig.close()


def test_the_rig_with_a_crop_and_a_monitor(st, gpu, plans):
    steps, sets = _run4_steps(), _run4_sets(gpu)[:2]
    rig = _rig(gpu, steps, sets).set_crop(mode=2).set_monitor(2).set_seam_paths(2, 8)
    try:
        got = rig.stitch(sets)
        res = rig.residuals()
        assert got[1] == [0, 0] and res.shape[:2] == (2, 3)
        domains = [rig.residual_domain(k) for k in range(3)]
        for i, frames in enumerate(sets):
            out, rec, found = _chain(rig, frames, steps, plans, 2, 8, crop=rig.crop, residuals=dict(radius=2, domains=domains))
            assert bool((out == got[0][i]).all()) and _same_paths(rig, i, found), f"set {i}"
            assert np.array_equal(rec.cpu().numpy().astype(np.int64), res[i].astype(np.int64))
    finally:
        rig.close()


@pytest.mark.parametrize("name", ["no_overlap", "clear_of_mid_row"])
@pytest.mark.parametrize("mode", ["found", "fixed"])
def test_a_step_without_a_geometric_seam_fails_the_replay(st, gpu, name, mode):
    """The branch of a step is its geometric seam's: where the footprints give none, the first replay along paths returns that
    error and names the step, and the rig replays as before once the paths are cleared."""
    import torch
    import rig_seams_ref as ref
    sizes, steps, want = ref.failure_cases(capi)[name]
    sets = [[capi.dev_synth(w, h, 3 * i + f, torch.uint8, gpu) for f, (w, h) in enumerate(sizes)] for i in range(2)]
    rig = capi.Rig.from_steps(sizes, 0, steps)
    try:
        before = rig.stitch(sets)
        if mode == "found":
            rig.set_seam_paths(2, 8)
        else:
            rig.fix_seam_paths([np.full(s["ch"], s["cw"] // 2, np.int32) for s in steps])
        rig.stitch(sets)
        assert rig.last_rc == want and b"step 1" in capi.lib().stitch_last_error() and b"seam paths" in capi.lib().stitch_last_error()
        with pytest.raises(capi.StitchError):
            rig.last_seam_paths(0, 0)  # a replay that failed leaves no paths
        after = rig.clear_seam_paths().stitch(sets)
        assert after[1:] == before[1:] and all(bool((a == b).all()) for a, b in zip(after[0], before[0]))
    finally:
        rig.close()


def test_the_rig_over_two_launch_sequences(st, gpu, plans):
    """Three sets at max_sets = 2 are two launch sequences (2 + 1): paths and outputs come back in set order."""
    steps, sets = _run4_steps(), _run4_sets(gpu)
    rig = _rig(gpu, steps, sets, max_sets=2).set_seam_paths(8, 0)
    try:
        got = rig.stitch(sets)
        assert got[1] == [0, 0, 0]
        for i, frames in enumerate(sets):
            out, found = _chain(rig, frames, steps, plans, 8, 0)
            assert bool((out == got[0][i]).all()) and _same_paths(rig, i, found), f"set {i}"
        fixed = rig.fix_seam_paths([rig.last_seam_paths(2, k)[0] for k in range(3)]).stitch(sets)
        assert bool((fixed[0][2] == got[0][2]).all())
    finally:
        rig.close()


def test_rig_argument_errors(st, gpu):
    steps, sets = _run4_steps(), _run4_sets(gpu)
    rig = _rig(gpu, steps, sets)
    L = capi.lib()
    try:
        for K, m in ((0, 8), (9, 8), (2, -1), (2, 65)):
            with pytest.raises(capi.StitchError) as e:
                rig.set_seam_paths(K, m)
            assert e.value.code == capi.ERR_ARG and rig.seam_paths is None
        assert L.stitch_rig_set_seam_paths(None, None) == L.stitch_rig_clear_seam_paths(None) == L.stitch_rig_seam_paths(None, None, None) == capi.ERR_ARG
        assert L.stitch_rig_fix_seam_paths(rig._h, None, 3) == L.stitch_rig_fix_seam_paths(None, None, 0) == capi.ERR_ARG
        with pytest.raises(capi.StitchError):
            rig.fix_seam_paths([np.zeros(s["ch"], np.int32) for s in steps[:2]])  # two paths for three steps
        with pytest.raises(ValueError):
            rig.fix_seam_paths([np.zeros(5, np.int32)] * 3)  # the wrong height
        assert rig.seam_paths is None and L.stitch_rig_set_seam_paths(rig._h, None) == 0 and rig.seam_paths == ("found", 2, 8)
        assert L.stitch_rig_last_seam_paths(rig._h, 0, 0, None, 0, None) == capi.ERR_ARG  # no replay along paths yet
    finally:
        rig.close()
