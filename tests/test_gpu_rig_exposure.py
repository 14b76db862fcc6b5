"""GPU: the exposure-matched rig replay (include/stitch_rig_exposure.h, csrc/k_rig_exposure.inc, csrc/stitch_rig_exposure.inc).
No tolerance anywhere, and nothing is compared with itself.  The yardsticks are code that existed before it:

  * capi.dev_transfer on one image (stitch_dev_transfer_form_u8) for capi.dev_transfer_many: bytes, statistics and counters;
  * pipeline.stitch_chain(..., exposure=, keep_black=) on one set for the rig's mosaics, statuses and seams, and the same chain
    restated from capi.dev_project, pipeline.exposure_match(stats=) and Plan.pair for its statistics (stitch_chain returns none;
    the restatement is itself held to stitch_chain's bytes and to the recorded statistics of run "4");
  * the recorded hashes and statistics bits of tests/golden/exposure.json.

Statistics are compared by their bits, a NaN as a NaN (tests/test_gpu_exposure.py `same` says why its sign is open)."""
import ctypes as C
import hashlib
import json
import os

import numpy as np
import pytest

import chain_sets
from computervisionimagestich2_amd import bmp, capi, pipeline

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
_cache = {}


def _sha(t):
    return hashlib.sha256(t.cpu().numpy().tobytes()).hexdigest()


def _same(a, b):
    return a.shape == b.shape and bool((a == b).all())


def _bits(a):
    a = a.cpu().numpy() if hasattr(a, "cpu") else np.asarray(a)
    return [int(v) for v in np.ascontiguousarray(a, np.float32).reshape(-1).view(np.uint32)]


def _is_nan(b):
    return (b & 0x7fffffff) > 0x7f800000


def _same_bits(a, b):
    """Two lists of float bit patterns are the same -- a NaN compares as a NaN."""
    return len(a) == len(b) and all(x == y or (_is_nan(x) and _is_nan(y)) for x, y in zip(a, b))


def _json(name):
    if name not in _cache:
        with open(os.path.join(GOLD, name)) as f:
            _cache[name] = json.load(f)
    return _cache[name]


def _committed(gpu):
    """The four committed frames on the device (shared, left unchanged)."""
    import torch
    if "frames" not in _cache:
        _cache["frames"] = [torch.from_numpy(np.ascontiguousarray(bmp.load_bmp(os.path.join(GOLD, "input", f"{i}.bmp")))).to(gpu) for i in range(1, 5)]
    return _cache["frames"]


def _lut_mapped(frames):
    """Every byte through a fixed table without a 0 in it (tests/test_gpu_rig.py)."""
    import torch
    lut = torch.from_numpy(((np.arange(256) * 7 + 13) % 255 + 1).astype(np.uint8)).to(frames[0].device)
    return [lut[f.long()].contiguous() for f in frames]


def _sizes(frames):
    return [(f.shape[2], f.shape[1]) for f in frames]


@pytest.fixture(scope="module")
def plans():
    """The single-set chains' workspaces, kept for the module: one per canvas size and option set."""
    kept = {}
    yield kept
    for p in kept.values():
        pipeline.close_plans(p)


def _chain(plans, frames, steps, mode, kb, finish=True):
    """The yardstick on ONE set -> dict(status, out, seams, stats).  out and seams: pipeline.stitch_chain (a step's seam is read
    from its workspace after a chain that ends with it).  stats: the twelve statistics bits of every step, from the chain restated
    with pipeline.exposure_match(stats=); its mosaic must be stitch_chain's.  A chain that raises gives its status alone."""
    import torch
    pl = plans.setdefault("default", {})
    kw = dict(exposure=mode, keep_black=bool(kb), finish=finish)
    try:
        out = pipeline.stitch_chain(frames, steps, plans=pl, **kw)
    except capi.StitchError as e:
        return dict(status=e.code, out=None, seams=None, stats=None)
    seams = [None] * len(steps)
    for k, st in enumerate(steps):
        if all((s["cw"], s["ch"]) != (st["cw"], st["ch"]) for s in steps[k + 1:]):
            seams[k] = pl[st["cw"], st["ch"]].status().as_tuple()
    for k, st in enumerate(steps):
        if seams[k] is None:
            pipeline.stitch_chain(frames, steps[:k + 1], plans=pl, **dict(kw, finish=False))
            seams[k] = pl[st["cw"], st["ch"]].status().as_tuple()
    stats = []
    if mode:
        proj = {}

        def projected(i):
            if i not in proj:
                proj[i] = capi.dev_project(frames[i])
            return proj[i]

        result = projected(steps[0]["start"])
        for st in steps:
            s12 = torch.zeros(12, dtype=torch.float32, device=frames[0].device)
            pipeline.exposure_match(projected(st["src"]), projected(st["mosaic_src"]) if mode == 1 else None, result, mode, bool(kb), stats=s12)
            plan = pl[st["cw"], st["ch"]]
            plan.status()
            result = plan.pair(projected(st["src"]), st["p"], st["offx"], st["offy"], result, st["ox"], st["oy"])
            stats.append(_bits(s12))
        if finish:
            capi.dev_finish(result)
        assert _same(result, out), "the restated chain is not stitch_chain"
    return dict(status=0, out=out, seams=seams, stats=stats)


def _check_set(i, ref, out, status, seams, stats):
    assert status == ref["status"], f"set {i}: status {status}, the chain's {ref['status']}"
    if ref["status"]:
        return
    assert _same(out, ref["out"]), f"set {i}: mosaic"
    assert seams == ref["seams"], f"set {i}: seams"
    if stats is not None:
        for k, want in enumerate(ref["stats"]):
            assert _same_bits(_bits(stats[k]), want), f"set {i} step {k}: statistics {_bits(stats[k])}, the chain's {want}"


# ---- 1. the transfer of many images against the transfer of one -------------------------------------------------------------------
SHAPES = [(64, 48, 64, 48, 5), (128, 96, 96, 50, 3), (50, 37, 64, 48, 3), (64, 48, 64, 48, 1), (384, 512, 384, 512, 2)]


def _pairs(gpu, sw, sh, tw, th, count):
    import torch
    key = ("pairs", sw, sh, tw, th, count)
    if key not in _cache:
        _cache[key] = ([capi.dev_synth(sw, sh, 20 + 2 * i, torch.uint8, gpu) for i in range(count)],
                       [capi.dev_synth(tw, th, 21 + 2 * i, torch.uint8, gpu) for i in range(count)])
    return _cache[key]


def _single(srcs, tems, form, kb):
    """capi.dev_transfer image by image -> [(out, stats bits, diag or None)]"""
    import torch
    res = []
    for s, t in zip(srcs, tems):
        st = torch.zeros(12, dtype=torch.float32, device=s.device)
        dg = torch.full((6, 4), -1, dtype=torch.int32, device=s.device) if form else None
        out = capi.dev_transfer(s, t, stats=st, stats_form=form, keep_black=bool(kb), diag=dg)
        res.append((out, _bits(st), None if dg is None else dg.cpu().numpy()))
    return res


def _check_many(srcs, tems, form, kb, outs=None):
    import torch
    want = _single(srcs, tems, form, kb)  # before the call: `outs` may be the sources themselves
    before = [s.clone() for s in srcs]
    if outs is None:
        outs = [torch.full_like(s, 0x5A) for s in srcs]
    got, stats, diag = capi.dev_transfer_many(srcs, tems, out=outs, stats_form=form, keep_black=bool(kb), want_stats=True, want_diag=True)
    assert all(g.data_ptr() == o.data_ptr() for g, o in zip(got, outs))
    for i, (w_out, w_bits, w_diag) in enumerate(want):
        assert _same(got[i], w_out), f"image {i}: bytes"
        assert _same_bits(_bits(stats[i]), w_bits), f"image {i}: statistics {_bits(stats[i])}, the single call's {w_bits}"
        if form:
            assert np.array_equal(diag[i].cpu().numpy(), w_diag), f"image {i}: counters {diag[i].cpu().numpy().tolist()}, the single call's {w_diag.tolist()}"
        else:
            assert not diag[i].any()  # the serial form counts nothing; the single call zeroes them too
    assert any(bool((w[0] != 0x5A).any()) and not _same(w[0], b) for w, b in zip(want, before))
    return got, stats


@pytest.mark.parametrize("kb", [0, 1])
@pytest.mark.parametrize("form", [0, 1, 2])
@pytest.mark.parametrize("sw,sh,tw,th,count", SHAPES)
def test_transfer_many_equals_transfer(st, gpu, sw, sh, tw, th, count, form, kb):
    srcs, tems = _pairs(gpu, sw, sh, tw, th, count)
    keep = [s.clone() for s in srcs]
    _check_many(srcs, tems, form, kb)
    assert all(_same(a, b) for a, b in zip(srcs, keep))  # out of place: the sources stay
    if count > 1:  # without the optional outputs
        got = capi.dev_transfer_many(srcs[:2], tems[:2], stats_form=form, keep_black=bool(kb))
        assert _same(got[1], capi.dev_transfer(srcs[1], tems[1], stats_form=form, keep_black=bool(kb)))


@pytest.mark.parametrize("form", [0, 2])
def test_transfer_many_in_place(st, gpu, form):
    srcs, tems = _pairs(gpu, 128, 96, 96, 50, 3)
    mine = [s.clone() for s in srcs]
    got, _ = _check_many(mine, tems, form, 1, outs=mine)
    assert all(g.data_ptr() == m.data_ptr() for g, m in zip(got, mine)) and not _same(mine[0], srcs[0])


@pytest.mark.parametrize("form", [0, 1, 2])
def test_transfer_many_with_a_black_source(st, gpu, form):
    """One all-black source among others: its planes are constant and its sd is 0, so the apply pass divides by zero.  Its
    statistics compare as bits or NaN, its bytes are the single call's own, and its neighbours are untouched by it."""
    import torch
    srcs, tems = _pairs(gpu, 64, 48, 64, 48, 5)
    srcs = list(srcs)
    srcs[2] = torch.zeros_like(srcs[2])
    for kb in (0, 1):
        _, stats = _check_many(srcs, tems, form, kb)
        assert _bits(stats[2])[3:6] == [0, 0, 0]


def test_transfer_many_refusals(st, gpu):
    import torch
    srcs, tems = _pairs(gpu, 64, 48, 64, 48, 5)
    outs = [torch.full_like(s, 0x5A) for s in srcs]
    L, tab = capi.lib(), capi._ptr_table
    for form in (3, -1):
        with pytest.raises(capi.StitchError) as e:
            capi.dev_transfer_many(srcs, tems, out=outs, stats_form=form)
        assert e.value.code == capi.ERR_ARG
    null = (C.c_void_p * 5)(*[s.data_ptr() for s in srcs[:4]], None)
    args = (5, 64, 48, 64, 48, 2, 0, None, None, capi._stream())
    assert L.stitch_dev_transfer_many_u8(null, tab(tems), tab(outs), *args) == capi.ERR_ARG
    assert L.stitch_dev_transfer_many_u8(tab(srcs), null, tab(outs), *args) == capi.ERR_ARG
    assert L.stitch_dev_transfer_many_u8(tab(srcs), tab(tems), None, *args) == capi.ERR_ARG
    for count, sw, sh in ((0, 64, 48), (1025, 64, 48), (5, 0, 48), (5, 65536, 32768)):
        assert L.stitch_dev_transfer_many_u8(tab(srcs), tab(tems), tab(outs), count, sw, sh, 64, 48, 2, 0, None, None, capi._stream()) == capi.ERR_ARG
    assert L.stitch_dev_transfer_many_u8(tab(srcs), tab(tems), tab(outs), 5, 64, 48, 65536, 32768, 2, 0, None, None, capi._stream()) == capi.ERR_ARG
    torch.cuda.synchronize()
    assert all(bool((o == 0x5A).all()) for o in outs)  # nothing was enqueued


# ---- 2. run "4" as a rig ----------------------------------------------------------------------------------------------------------
def _run4_steps():
    G = _json("golden.json")["runs"]["4"]
    rec = _json("exposure.json")["runs"]["4"]["mode1_keep_black1"]["steps"]
    return [dict(s, mosaic_src=r["mosaic_src"]) for s, r in zip(G["steps"], rec)]


def _run4_sets(gpu):
    if "run4_sets" not in _cache:
        frames = _committed(gpu)
        _cache["run4_sets"] = [frames, _lut_mapped(frames), _lut_mapped(_lut_mapped(frames))]
    return _cache["run4_sets"]


@pytest.mark.parametrize("mode,kb", [(1, 0), (1, 1), (2, 0), (2, 1)])
def test_run_4_three_sets(st, gpu, plans, mode, kb):
    R = _json("exposure.json")["runs"]["4"][f"mode{mode}_keep_black{kb}"]
    steps, sets = _run4_steps(), _run4_sets(gpu)
    want = [_chain(plans, s, steps, mode, kb) for s in sets]
    rig = capi.Rig.from_steps(_sizes(sets[0]), None, steps, exposure=mode, keep_black=bool(kb))
    outs, status, seams, stats = rig.stitch(sets, return_stats=True)
    assert list(outs[0].shape) == R["final_shape"] and _sha(outs[0]) == R["final_sha256"]
    assert [_bits(stats[0][k]) for k in range(3)] == [s["stats_bits"] for s in R["steps"]]
    for i in range(3):
        _check_set(i, want[i], outs[i], status[i], seams[i], stats[i])
    assert status == [0, 0, 0] and not _same(outs[0], outs[1]) and not _same(outs[1], outs[2])
    assert _bits(stats[0]) != _bits(stats[1])  # per set: each from its own pixels
    # the plain call on the same rig carries the mode
    again, status, _ = rig.stitch(sets[:2])
    assert status == [0, 0] and _same(again[0], outs[0]) and _same(again[1], outs[1])
    rig.close()


def test_run_4_without_the_finish_pass(st, gpu, plans):
    R = _json("exposure.json")["runs"]["4"]["mode1_keep_black1"]
    steps, sets = _run4_steps(), _run4_sets(gpu)
    want = [_chain(plans, s, steps, 1, 1, finish=False) for s in sets]
    rig = capi.Rig.from_steps(_sizes(sets[0]), None, steps, exposure=1, finish=False)
    outs, status, seams, stats = rig.stitch(sets, return_stats=True)
    assert _sha(outs[0]) == R["steps"][-1]["out_sha256"]
    for i in range(3):
        _check_set(i, want[i], outs[i], status[i], seams[i], stats[i])
    rig.close()


# ---- 3. a hand-made small rig -------------------------------------------------------------------------------------------------------
def _hand_steps(sizes, moves, start=0):
    """Step dicts of a hand-made rig: moves = [(frame to warp, the frame it is stitched to, forward map, backward map)]."""
    steps, (mw, mh) = [], sizes[start]
    for dst, src, p_fwd, p_bwd in moves:
        g = capi.step_geometry(sizes[dst][0], sizes[dst][1], p_fwd, mw, mh)
        steps.append(dict(start=start, src=dst, mosaic_src=src, p=p_bwd, p_fwd=p_fwd, offx=g.min_x, offy=g.min_y, ox=g.ox, oy=g.oy, cw=g.cw, ch=g.ch))
        mw, mh = g.cw, g.ch
    return steps


def _shift(tx, ty, c=1e-4, d=5e-5):
    return [1.0, 0.0, c, float(tx), 0.0, 1.0, d, float(ty)], [1.0, 0.0, -c, -float(tx), 0.0, 1.0, -d, -float(ty)]


def _small_steps(scale=1):
    """tests/test_gpu_rig.py `_small_steps` with the frame each step is stitched to; scale 2: the same rig for 128 x 96 frames."""
    sizes = [(64 * scale, 48 * scale)] * 3
    c, d = 1e-4 / scale, 5e-5 / scale
    return sizes, _hand_steps(sizes, [(1, 0) + tuple(_shift(31.5 * scale + (scale - 1) * 0.5, 1.25, c, d)), (2, 0) + tuple(_shift(-29.75 * scale, -0.5, c, d))])


def _small_sets(n_sets, gpu, scale=1):
    import torch
    return [[capi.dev_synth(64 * scale, 48 * scale, 3 * i + f, torch.uint8, gpu) for f in range(3)] for i in range(n_sets)]


def _small_refs(plans, n_sets, gpu, mode, kb=1, scale=1):
    """The chains of the first n_sets small sets, computed once per mode and shared."""
    have = _cache.setdefault(("small", mode, kb, scale), [])
    sets = _small_sets(n_sets, gpu, scale)
    steps = _small_steps(scale)[1]
    while len(have) < n_sets:
        have.append(_chain(plans, sets[len(have)], steps, mode, kb))
    return sets, have[:n_sets]


@pytest.mark.parametrize("n_sets,max_sets", [(5, 2), (17, 16)])
@pytest.mark.parametrize("mode", [1, 2])
def test_small_rig_more_sets_than_one_sequence(st, gpu, plans, mode, n_sets, max_sets):
    """5 sets at 2 run as 2 + 2 + 1 and 17 at 16 as 9 + 8: the scratch, the tables' prefix and the statistics buffer are reused
    from sequence to sequence."""
    sets, want = _small_refs(plans, n_sets, gpu, mode)
    sizes, steps = _small_steps()
    assert (steps[0]["cw"], steps[0]["ch"]) != (steps[1]["cw"], steps[1]["ch"])
    rig = capi.Rig.from_steps(sizes, 0, steps, max_sets=max_sets, exposure=mode)
    outs, status, seams, stats = rig.stitch(sets, return_stats=True)
    assert [w["status"] for w in want] == [0] * n_sets  # the synthetic sets stitch
    for i in range(n_sets):
        _check_set(i, want[i], outs[i], status[i], seams[i], stats[i])
    assert not _same(outs[0], outs[n_sets - 1]) and _bits(stats[0]) != _bits(stats[n_sets - 1])
    plain = capi.Rig.from_steps(sizes, 0, steps, max_sets=max_sets)
    assert not _same(plain.stitch(sets[:1])[0][0], outs[0])  # the option is on
    plain.close()
    rig.close()


@pytest.mark.parametrize("form", [0, 1, 2])
def test_template_grows_across_a_span_boundary(st, gpu, plans, form):
    """128 x 96 frames in mode 2: the frame's planes have 12 288 samples (two spans), the template of step 1 is the mosaic of
    step 0 with more than 16 384 (three spans), so one launch holds planes of different span counts."""
    sets, want = _small_refs(plans, 3, gpu, 2, scale=2)
    sizes, steps = _small_steps(2)
    assert sizes[0][0] * sizes[0][1] == 12288 and steps[0]["cw"] * steps[0]["ch"] > 16384
    rig = capi.Rig.from_steps(sizes, 0, steps, exposure=2, stats_form=form)
    outs, status, seams, stats = rig.stitch(sets, return_stats=True)
    for i in range(3):
        _check_set(i, want[i], outs[i], status[i], seams[i], stats[i])
    assert status == [0, 0, 0]
    rig.close()


# ---- 4. a recoloured frame warped again, or serving as a template -------------------------------------------------------------------
@pytest.mark.parametrize("mode", [1, 2])
def test_dense4(st, gpu, plans, mode):
    import torch
    G = chain_sets.chains()["dense4"]
    order = [(s["srcIndex"], s["dstIndex"]) for s in G["steps"]]
    warped = [d for _, d in order]
    assert max(warped.count(d) for d in set(warped)) >= 2 and any(s in warped[:k] for k, (s, _) in enumerate(order))
    frames = [torch.from_numpy(np.array(f)).to(gpu) for f in chain_sets.frames_of(G["frames"])]
    steps = [dict(s, src=s["dstIndex"], mosaic_src=s["srcIndex"], start=G["start"]) for s in G["steps"]]
    sets = [frames, _lut_mapped(frames)]
    want = [_chain(plans, s, steps, mode, 1) for s in sets]
    rig = capi.Rig.from_steps(_sizes(frames), G["start"], steps, max_sets=2, exposure=mode)
    outs, status, seams, stats = rig.stitch(sets, return_stats=True)
    for i in range(2):
        _check_set(i, want[i], outs[i], status[i], seams[i], stats[i])
    assert status == [0, 0] and _sha(outs[0]) != G["final_sha256"]  # the option is on
    again = next(d for d in warped if warped.count(d) >= 2)
    k2 = [k for k, (_, d) in enumerate(order) if d == again]
    assert _bits(stats[0][k2[0]])[:6] != _bits(stats[0][k2[1]])[:6]  # the second transfer met the recoloured frame
    rig.close()


# ---- 5. a failing set among good ones -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [1, 2])
def test_failing_set_among_good_ones(st, gpu, plans, mode):
    import torch
    sets, want = _small_refs(plans, 3, gpu, mode)
    assert [w["status"] for w in want] == [0, 0, 0]
    sizes, steps = _small_steps()
    bad = [list(s) for s in sets]
    bad[1][1] = torch.zeros_like(bad[1][1])  # the frame step 0 warps
    assert _chain(plans, bad[1], steps, mode, 1)["status"] == capi.ERR_EMPTY_MIDROW
    rig = capi.Rig.from_steps(sizes, 0, steps, exposure=mode)
    outs, status, seams, stats = rig.stitch(bad, return_stats=True)
    assert status == [0, capi.ERR_EMPTY_MIDROW, 0] and rig.last_rc == capi.ERR_EMPTY_MIDROW
    assert b"set 1, step 0" in capi.lib().stitch_last_error()
    for i in (0, 2):
        _check_set(i, want[i], outs[i], status[i], seams[i], stats[i])
    outs, status, seams, stats = rig.stitch(sets, return_stats=True)
    assert status == [0, 0, 0] and rig.last_rc == 0
    for i in range(3):
        _check_set(i, want[i], outs[i], status[i], seams[i], stats[i])
    rig.close()


# ---- 6. the remaining cases ---------------------------------------------------------------------------------------------------------
def test_mode_0_is_the_rig_as_it_is(st, gpu):
    sets = _small_sets(3, gpu)
    sizes, steps = _small_steps()
    old = capi.Rig.from_steps(sizes, 0, steps)  # stitch_rig_create
    want, want_status, want_seams = old.stitch(sets)
    old.close()
    wh = np.ascontiguousarray(np.array(sizes, np.int32).reshape(-1, 2))
    for e in (None, capi.ExposureOpts(0, 2, 1)):
        h = C.c_void_p()
        capi._chk(capi.lib().stitch_rig_create_exposure(capi._p(wh), 3, 0, capi.rig_steps(steps, 0)[1], 2, None, None if e is None else C.byref(e), C.byref(h)))
        rig = capi.Rig(h)
        outs, status, seams = rig.stitch(sets)
        assert status == want_status == [0, 0, 0] and seams == want_seams and all(_same(a, b) for a, b in zip(outs, want))
        with pytest.raises(capi.StitchError) as err:
            rig.stitch(sets, return_stats=True)
        assert err.value.code == capi.ERR_ARG and "mode 0" in str(err.value)
        outs, status, _ = rig.stitch(sets)  # and the rig is as usable as before
        assert status == [0, 0, 0] and _same(outs[2], want[2])
        rig.close()


def test_from_panorama_reproduces_the_exposure_matched_panorama(st, gpu):
    frames = _committed(gpu)
    R = _json("exposure.json")["runs"]["4"]["mode1_keep_black1"]
    pano = capi.dev_panorama_handle(frames, exposure=1)
    mosaic = pano.mosaic()
    assert _sha(mosaic) == R["final_sha256"]
    rig = capi.Rig.from_panorama(pano, frames, exposure=1)
    plain = capi.Rig.from_panorama(pano, frames)  # nothing is inferred from the handle
    pano.close()
    outs, status, _, stats = rig.stitch([frames, _lut_mapped(frames)], return_stats=True)
    assert status == [0, 0] and _same(outs[0], mosaic)
    assert [_bits(stats[0][k]) for k in range(3)] == [s["stats_bits"] for s in R["steps"]]
    outs, status, _ = plain.stitch([frames])
    assert status == [0] and _sha(outs[0]) == _json("golden.json")["runs"]["4"]["final_sha256"]
    rig.close()
    plain.close()


def test_a_stream_of_the_callers_own(st, gpu, plans):
    import torch
    sets, want = _small_refs(plans, 3, gpu, 2)
    sizes, steps = _small_steps()
    rig = capi.Rig.from_steps(sizes, 0, steps, exposure=2)
    outs = [torch.full((3, rig.height, rig.width), 0xEE, dtype=torch.uint8, device=gpu) for _ in range(3)]
    mine = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(mine):
        got, status, seams, stats = rig.stitch(sets, out=outs, return_stats=True)
        srcs, tems = _pairs(gpu, 128, 96, 96, 50, 3)
        many = capi.dev_transfer_many(srcs, tems, stats_form=2)
    # complete when the calls return: both waited for their stream
    for i in range(3):
        _check_set(i, want[i], outs[i], status[i], seams[i], stats[i])
    assert all(_same(m, capi.dev_transfer(s, t, stats_form=2)) for m, s, t in zip(many, srcs, tems))
    rig.close()
