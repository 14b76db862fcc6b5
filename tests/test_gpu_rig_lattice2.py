"""GPU: the rig replay's newer options in combination -- path seams found, anchored and fixed, the 4:2:2 layouts and NV21 on both
sides, smoothed and fixed exposure statistics and the output scale, with crop, finish, monitor and the cut of a stream into calls and
launch sequences -- by the covering array of tests/rig_lattice2.py (every PAIR of levels, 48 rows in 14 creation groups) on the rigs
w64_65 and odd_h of tests/rig_edges.py, whose canvases sit at the edges of the coverage planes' 64-bit words.  Everything is exact.

Per row, every call of the row's stream is held to TWO references:
  * tests/rig_chain_ref.py, the CPU statement of the whole replay: every set's output (formatted outputs as whole images, pitches and
    the untouched 0xEE padding included), statuses, seam records, the statistics returned, last_used_stats(), paths, costs and
    last_seam_moved(), residuals(), and after the call exposure_state() and seam_anchor()[1];
  * pipeline.stitch_chain with the same options, fed set by set with the carried anchors and smoothing state: outputs, paths, costs,
    moved, records, measured and used statistics, the state.
input_form per frame is what a bare formatted rig answers for the same frames (FUSED only for the tight, aligned levels);
out_width / out_height are the scale's.  Rows that share what a handle is created with (mode, finish, calls) run on ONE handle in table
order, switched by the set / clear / fix / reset calls alone, the anchor and the smoothing state reset before each row; then the group's
first row runs again behind all the others and on a fresh handle: all three results are equal.  A group of more than PART rows is
split into cases of PART rows, each on a handle of its own with its own first row repeated, so that no case takes more than twice the
slowest case of tests/test_gpu_rig_lattice.py.

Fixed rows behind the array: one masked workspace serving two steps; frames of odd width in the 4:2:2 layouts and NV21; anchor and
smoothing state carried untouched through switches of scale, crop, monitor and output format, and what clear_seam_paths keeps; a slot
whose seam repeats and then moves (the kept mask pyramid), then path seams, then content seams again; and a dark frame in mid-stream."""
import numpy as np
import pytest

import pixfmt_yuv_ref as pyr
import residual_ref as rr
import rig_chain_ref as rc
import rig_lattice2 as l2
import scale_ref as sr
from computervisionimagestich2_amd import capi, pipeline
from test_gpu_pixfmt import from_dev

pytestmark = pytest.mark.gpu

TABLE = l2.table()
GROUPS = l2.groups(TABLE)
PART = 4  # rows per case: a creation group of more rows is split, each part on a handle of its own (a case stays within twice the
#           slowest case of tests/test_gpu_rig_lattice.py)
CASES = [(name, key, first) for name in l2.RIG_NAMES for key in GROUPS for first in range(0, len(GROUPS[key]), PART)]
NONE, FUSED, CONVERTED = capi.RIG_INPUT_NONE, capi.RIG_INPUT_FUSED, capi.RIG_INPUT_CONVERTED
IN_FMT = l2.IN_FMT
_ctx, _forms = {}, {}


@pytest.fixture(scope="module")
def plans():
    """The chains' workspaces, one per canvas size and kind, kept for the module."""
    kept = {}
    yield kept
    pipeline.close_plans(kept)


class _Ctx(l2.Ctx):
    """tests/rig_lattice2.py's context plus what the chains need on the device: the coverage masks of every step."""

    def __init__(self, oracle, name, gpu):
        super().__init__(capi, oracle, name)
        self.gpu = gpu
        rig = capi.Rig.from_steps(self.sizes, 0, self.steps)
        try:
            self.cover = [(rig.coverage(k, 0), rig.coverage(k, 1)) for k in range(len(self.steps))]
            for k, (a, b) in enumerate(self.cover):  # the rig's geometry is the CPU's
                assert np.array_equal(a.cpu().numpy() != 0, self.geo["cov"][k]["A"]) and np.array_equal(b.cpu().numpy() != 0, self.geo["cov"][k]["B"]), k
            assert rig.inscribed_rect() == tuple(self.inscribed)
            assert [tuple(s) for s in rig.geometric_seams().seams] == self.geo["geometric"]
        finally:
            rig.close()


def _context(oracle, name, gpu):
    if name not in _ctx:
        _ctx[name] = _Ctx(oracle, name, gpu)
    return _ctx[name]


def _make(ctx, opt):
    return capi.Rig.from_steps(ctx.sizes, 0, ctx.steps, exposure=opt["exposure"][0], finish=opt["finish"], max_sets=opt["calls"][1])


def _apply(rig, ctx, opt, chain):
    """The row's options on a handle that may hold another row's, by the set / clear / fix / reset calls alone."""
    rig.clear_seams().clear_seam_paths().clear_seam_anchor()
    s = chain["seams"]
    if s[0] == "given":
        rig.fix_seams(s[1])
    elif s[0] == "paths":
        if chain.get("anchor"):
            rig.set_seam_anchor(*chain["anchor"])
        rig.set_seam_paths(s[1], s[2])
    elif s[0] == "fixed_paths":
        rig.fix_seam_paths(s[1])
    if chain["mode"]:
        rig.clear_exposure_smoothing().clear_fixed_exposure()
        if chain.get("fixed") is not None:
            rig.fix_exposure(chain["fixed"])
        elif chain.get("keep") is not None:
            rig.set_exposure_smoothing(chain["keep"])
        rig.reset_exposure_state()
    rig.reset_seam_anchor().clear_output_scale()
    rig.clear_crop() if chain["crop"] is None else rig.set_crop(*chain["crop"])
    if chain["scale"] is not None:
        rig.set_output_scale(*chain["scale"])
    fmts = (chain["in_fmt"], chain["out_fmt"])
    rig.clear_formats() if fmts == (0, 0) else rig.set_formats(fmts[0], fmts[1], chain["matrix"])
    rig.clear_monitor() if chain["monitor"] is None else rig.set_monitor(chain["monitor"])
    assert rig.formats[:2] == fmts and rig.monitor == chain["monitor"] and rig.output_scale == chain["scale"]
    assert (rig.out_width, rig.out_height) == ctx.out_size(opt)  # the scale's, else the crop's, else the canvas's


def _dev_frame(gpu, im, offset):
    """A reference image (or a planar array) on the device, its planes `offset` bytes into fresh buffers."""
    import torch

    def plane(a):
        if a is None:
            return None
        t = torch.empty(a.size + offset, dtype=torch.uint8, device=gpu)
        t[offset:] = torch.from_numpy(np.ascontiguousarray(a).reshape(-1)).to(gpu)
        return t[offset:]

    if isinstance(im, np.ndarray):
        return plane(im).view(*im.shape)
    return capi.Image(im["fmt"], im["w"], im["h"], plane(im["data"]), plane(im["data2"]), im["pitch"], im["pitch2"])


def _host_out(o):
    if isinstance(o, capi.Image) and o.fmt != pyr.PLANAR:
        return from_dev(o)
    return (o.data if isinstance(o, capi.Image) else o).cpu().numpy()


def _same_stats(a, b):
    """Statistics by their bits, a NaN as a NaN."""
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and bool(((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))).all())


def _stitch(rig, ctx, opt, chain, sets):
    """One stitch() call on device frames -> everything the rig says of it, on the host."""
    n, K = len(sets), rig.n_steps
    outs = None
    if chain["out_fmt"]:
        ow, oh = ctx.out_size(opt)
        pitch, pitch2 = chain["out_pitch"]
        outs = [capi.Image.empty(chain["out_fmt"], ow, oh, ctx.gpu, pitch, pitch2 or None, fill=0xEE) for _ in range(n)]
    got = rig.stitch(sets, out=outs, return_stats=bool(chain["mode"]))
    res = dict(outs=[_host_out(o) for o in got[0]], status=got[1], seams=got[2], stats=got[3] if chain["mode"] else None, rc=rig.last_rc)
    pathed = chain["seams"][0] in ("paths", "fixed_paths")
    res["paths"] = [[rig.last_seam_paths(i, k) + (rig.last_seam_moved(i, k),) for k in range(K)] for i in range(n)] if pathed else None
    res["records"] = rig.residuals()
    res["used"] = rig.last_used_stats() if chain["mode"] else None
    res["state"] = (rig.exposure_state(), rig.exposure_smoothing()[1]) if chain["mode"] else None
    res["anchor"] = rig.seam_anchor()
    res["forms"] = [rig.input_form(f) for f in range(rig.n_frames)]
    # a planar replay call leaves the answer alone (stitch_rig_formats_yuv.h): then it is the handle's last formatted call's
    res["forms_rest"] = getattr(rig, "_forms", [NONE] * rig.n_frames) if (chain["in_fmt"], chain["out_fmt"]) == (0, 0) else None
    rig._forms = res["forms"]
    return res


def _against_cpu(ctx, chain, res, want, state, what):
    """One call's results against tests/rig_chain_ref.py's: want = per set one_set's dict, state = the state after the call."""
    n, K = len(want), len(ctx.steps)
    assert res["status"] == [w["status"] for w in want], what
    assert res["rc"] == next((w["status"] for w in want if w["status"]), 0), what
    failed = any(w["status"] for w in want)
    for i, w in enumerate(want):
        if w["status"]:
            continue
        assert l2.same(res["outs"][i], w["out"]), f"{what}: set {i} against the CPU statement"
        assert [tuple(s)[:len(c)] for s, c in zip(res["seams"][i], w["seams"])] == [tuple(c) for c in w["seams"]], f"{what}: set {i}, seams"
        if chain["mode"]:
            assert _same_stats(res["stats"][i], w["measured"]), f"{what}: set {i}, the statistics returned"
        if res["paths"] is not None and not failed:
            for k, (path, cost, moved) in enumerate(res["paths"][i]):
                assert path.tolist() == w["paths"][k].tolist() and (cost, moved) == (w["costs"][k], w["moved"][k]), f"{what}: set {i}, step {k}, path"
        if chain["monitor"] is not None:
            assert np.array_equal(res["records"][i].astype(np.int64), w["records"]), f"{what}: set {i}, residuals"
    if chain["monitor"] is None:
        assert res["records"].shape[0] == 0
    else:
        assert res["records"].shape == (n, K, rr.words(chain["monitor"]))
    if chain["mode"]:
        temporal = chain.get("fixed") is not None or chain.get("keep") is not None
        if temporal:
            assert res["used"].shape == (n, K, 12) and all(_same_stats(res["used"][i], w["used"]) for i, w in enumerate(want) if not w["status"]), what
        else:
            assert res["used"].shape[0] == 0, what
        has = [p is not None for p in state["smooth"]]
        zeros = np.zeros(12, np.float32)
        assert res["state"][1] == has and _same_stats(res["state"][0], np.stack([zeros if p is None else p for p in state["smooth"]])), f"{what}: the smoothing state"
    assert res["anchor"][1] == (state["anchor"] is not None), f"{what}: whether the rig holds an anchor"


def _chain_kw(ctx, chain, plans, domains):
    kw = dict(finish=chain["finish"], exposure=chain["mode"], crop=chain["crop"], plans=plans, scale=chain["scale"],
              formats=(chain["in_fmt"], chain["out_fmt"], chain["matrix"]) if (chain["in_fmt"], chain["out_fmt"]) != (0, 0) else None)
    s = chain["seams"]
    if s[0] == "given":
        kw["seams"] = s[1]
    elif s[0] == "paths":
        kw["seam_paths"] = dict(coverage=ctx.cover, branches=ctx.geo["branches"], max_step=s[1], margin=s[2])
    elif s[0] == "fixed_paths":
        kw["seam_paths"] = dict(coverage=ctx.cover, branches=ctx.geo["branches"], paths=s[1])
    if chain["monitor"] is not None:
        kw["residuals"] = dict(radius=chain["monitor"], domains=domains)
    return kw


def _against_chain(ctx, chain, plans, rig, res, sets, carried, what):
    """One call's results against pipeline.stitch_chain fed set by set.  carried: dict(anchor=[per step a device path] or None,
    smooth=[per step 12 floats or None]), moved on in place as a rig's state moves."""
    K = len(ctx.steps)
    domains = [rig.residual_domain(k) for k in range(K)] if chain["monitor"] is not None else None
    kw = _chain_kw(ctx, chain, plans, domains)
    anchored = chain["seams"][0] == "paths" and chain.get("anchor")
    temporal = chain["mode"] and (chain.get("fixed") is not None or chain.get("keep") is not None)
    anchors = carried["anchor"]
    found = None
    for i, frames in enumerate(sets):
        if res["status"][i]:  # a chain of a set that fails raises and says nothing of the state the sets behind it lean on: the CPU statement alone holds those
            break
        if anchored:
            kw["seam_paths"].update(anchors=anchors if anchors is not None else [None] * K, weight=chain["anchor"][0], cap=chain["anchor"][1])
        if temporal:
            kw["exposure_temporal"] = dict(fixed=list(chain["fixed"])) if chain.get("fixed") is not None else dict(keep=chain["keep"], state=carried["smooth"])
        got = pipeline.stitch_chain(frames, ctx.steps, **kw)
        out, *extras = got if isinstance(got, tuple) else (got,)
        out = _host_out(out)
        if chain["out_fmt"]:
            out = l2.repitched(out, *chain["out_pitch"])
        assert l2.same(res["outs"][i], out), f"{what}: set {i} against its chain"
        if chain["monitor"] is not None:
            assert np.array_equal(extras.pop(0).cpu().numpy().astype(np.int64), res["records"][i].astype(np.int64)), f"{what}: set {i}, residuals against its chain"
        if "seam_paths" in kw:
            found = extras.pop(0)
            for k, (path, cost, *moved) in enumerate(found):
                got_path, got_cost, got_moved = res["paths"][i][k]
                assert got_path.tolist() == path.cpu().numpy().tolist() and got_cost == (cost or 0) and got_moved == (moved[0] if moved else 0), \
                    f"{what}: set {i}, step {k}, path against its chain"
            if anchored and chain["anchor"][2] == "set":
                anchors = [f[0] for f in found]
        if temporal:
            t = extras.pop(0)
            assert _same_stats(res["used"][i], np.stack(t["used"])), f"{what}: set {i}, used statistics against its chain"
            if chain.get("fixed") is None:
                assert _same_stats(res["stats"][i], np.stack(t["measured"])), f"{what}: set {i}, measured statistics against its chain"
                carried["smooth"] = t["state"]
    if any(res["status"]):
        carried["anchor"], carried["smooth"] = None, [None] * K
        return
    if anchored and found is not None:
        carried["anchor"] = [f[0] for f in found]
    if chain["mode"] and chain.get("keep") is not None and chain.get("fixed") is None:
        zeros = np.zeros(12, np.float32)
        assert _same_stats(res["state"][0], np.stack([zeros if p is None else np.asarray(p, np.float32) for p in carried["smooth"]])), f"{what}: the state against the chains'"


def _bare_forms(ctx, opt, host):
    """What a bare formatted rig -- the input format and nothing else -- answers for the same frames, per call; once per level."""
    key = (ctx.name, opt["input"], opt["calls"])
    if key not in _forms:
        rig = capi.Rig.from_steps(ctx.sizes, 0, ctx.steps, finish=False, max_sets=opt["calls"][1])
        try:
            fmt = IN_FMT[opt["input"]][0]
            _forms[key] = []
            if fmt:
                rig.set_formats(fmt, pyr.PLANAR, ctx.matrix_of(opt))
            for sets in host:
                status = rig.stitch([[_dev_frame(ctx.gpu, im, off) for im, off in fs] for fs in sets])[1]
                assert status == [0] * len(sets)
                _forms[key].append([rig.input_form(f) for f in range(rig.n_frames)])
        finally:
            rig.close()
    return _forms[key]


def _form_of(ctx, level):
    fmt, pad = IN_FMT[level]
    return NONE if not fmt else FUSED if not pad and ctx.sizes[0][0] % 4 == 0 else CONVERTED


def _run_row(rig, ctx, opt, oracle, plans, chain=None, host=None, check=True, state=None, forms_host=None, **frames_kw):
    """A row's calls on `rig` -> per call _stitch's dict; held to both references where `check`.  forms_host: the frames the bare rig of
    _bare_forms is asked with instead of `host` (the form depends on layout, pitch and address, not on bytes; a bare rig refuses what
    content seams refuse)."""
    chain = ctx.chain_options(opt) if chain is None else chain
    _apply(rig, ctx, opt, chain)
    host = ctx.frames(opt["input"], opt["calls"][0], ctx.matrix_of(opt), **frames_kw) if host is None else host
    want = rc.stream(oracle, ctx.geo, ctx.steps, [[[im for im, _ in fs] for fs in sets] for sets in host], chain, state) if check else None
    carried = dict(anchor=None, smooth=[None] * len(ctx.steps))
    out = []
    for c, sets in enumerate(host):
        dev = [[_dev_frame(ctx.gpu, im, off) for im, off in fs] for fs in sets]
        res = _stitch(rig, ctx, opt, chain, dev)
        out.append(res)
        if check:
            what = f"row {opt['index']} of {ctx.name}, call {c}"
            _against_cpu(ctx, chain, res, want[c][0], want[c][1], what)
            _against_chain(ctx, chain, plans, rig, res, dev, carried, what)
            if res["forms_rest"] is not None:
                assert res["forms"] == res["forms_rest"], what
            else:
                assert res["forms"] == [_form_of(ctx, opt["input"])] * 3 == _bare_forms(ctx, opt, host if forms_host is None else forms_host)[c], what
    return out


def _same_runs(x, y):
    def flat(r):
        return [r["status"], r["seams"], None if r["stats"] is None else r["stats"].tobytes(), r["records"].tobytes(), r["anchor"],
                r["forms"] if r["forms_rest"] is None else None,
                None if r["used"] is None else r["used"].tobytes(), None if r["state"] is None else (r["state"][0].tobytes(), r["state"][1]),
                None if r["paths"] is None else [[(p.tolist(), c, m) for p, c, m in row] for row in r["paths"]]]
    return len(x) == len(y) and all(flat(a) == flat(b) and len(a["outs"]) == len(b["outs"]) and all(l2.same(p, q) for p, q in zip(a["outs"], b["outs"]))
                                    for a, b in zip(x, y))


# ---- the covering array ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lattice_contexts(gpu, oracle):
    """The two rigs' contexts -- geometry on the CPU and on the device, held to each other -- computed once, before any case."""
    return {name: _context(oracle, name, gpu) for name in l2.RIG_NAMES}


@pytest.mark.parametrize("name,key,part", CASES, ids=[f"{n}-{l2.key_id(k)}" + (f"-rows{p}" if len(GROUPS[k]) > PART else "") for n, k, p in CASES])
def test_rows_that_share_a_handle(st, gpu, oracle, plans, lattice_contexts, name, key, part):
    ctx = lattice_contexts[name]
    rows = GROUPS[key][part:part + PART]
    rig = _make(ctx, rows[0])
    try:
        first = None
        for opt in rows:
            assert l2.creation_key(opt) == key
            res = _run_row(rig, ctx, opt, oracle, plans)
            first = first or (opt, res)
        opt, res = first
        assert _same_runs(_run_row(rig, ctx, opt, oracle, plans, check=False), res), "the group's first row, repeated on its handle"
    finally:
        rig.close()
    fresh = _make(ctx, opt)
    try:
        assert _same_runs(_run_row(fresh, ctx, opt, oracle, plans, check=False), res), "the group's first row on a fresh handle"
    finally:
        fresh.close()


# ---- fixed rows behind the array --------------------------------------------------------------------------------------------------------
STREAM = ((3, 2), 2)


def test_one_masked_workspace_serves_two_steps(st, gpu, oracle, plans):
    """w64_twice: both steps on one 64 x 33 canvas.  Paths, anchors and the smoothing state are per step."""
    ctx = _context(oracle, "w64_twice", gpu)
    opt = dict(l2.NONE, exposure=(2, ("keep", 64)), seams="paths_set", monitor=2, calls=STREAM, index=1)
    rig = _make(ctx, opt)
    try:
        res = _run_row(rig, ctx, opt, oracle, plans)
        last = res[1]["paths"][-1]
        assert last[0][0].tolist() != last[1][0].tolist() and not _same_stats(res[1]["state"][0][0], res[1]["state"][0][1])
    finally:
        rig.close()


@pytest.mark.parametrize("level", ["yuyv_padded", "nv16_padded", "nv21_tight"])
def test_frames_of_odd_width(st, gpu, oracle, plans, level):
    """odd_w: 41 x 33 frames.  A 4:2:2 row ends in a group of one pixel (a Y1 byte that is no pixel's, 21 chroma columns); NV21 has a
    clamped last chroma column AND row.  No such frame takes the fused projection; the library converts them (the header refuses
    nothing here).  Each against both references and against its planar equivalent on the same handle; the output scaled by 8 into UYVY."""
    ctx = _context(oracle, "odd_w", gpu)
    opt = dict(l2.NONE, input=level, output="uyvy_tight", scale="eighth", calls=((3,), 2), index=TABLE[-1]["index"] + 1 + ["yuyv_padded", "nv16_padded", "nv21_tight"].index(level))
    rig = _make(ctx, opt)
    try:
        host = ctx.frames(level, (3,), ctx.matrix_of(opt))
        assert all(im["w"] % 2 == 1 and im["h"] % 2 == 1 for fs in host[0] for im, _ in fs)
        res = _run_row(rig, ctx, opt, oracle, plans, host=host)
        assert res[0]["forms"] == [CONVERTED] * 3 and ctx.out_size(opt) == (9, 5)
        planar = [[[(pyr.unpack(im, ctx.matrix_of(opt)), 0) for im, _ in fs] for fs in host[0]]]
        twin = _run_row(rig, ctx, dict(opt, input="planar"), oracle, plans, host=planar, check=False)
        assert all(l2.same(a, b) for a, b in zip(res[0]["outs"], twin[0]["outs"])) and twin[0]["seams"] == res[0]["seams"]
    finally:
        rig.close()


def test_state_across_option_switches_on_one_handle(st, gpu, oracle, plans):
    """Found paths with an anchor per set and smoothing stay set; a scale, a crop with a monitor, and an output format come and go
    between calls.  Every call equals the CPU stream that never toggled, after the same scale, crop or pack of its planar result --
    the anchor and the smoothing state carried through untouched.  (The format that toggles is the OUTPUT's: a 4:2:2 input is lossy and
    would make another stream of it.)  Then what clear_seam_paths keeps and drops."""
    ctx = _context(oracle, "w64_65", gpu)
    opt = dict(l2.NONE, exposure=(1, ("keep", 192)), seams="paths_set", calls=((2, 1, 1, 1, 1, 1), 2), index=2)
    chain = ctx.chain_options(opt)
    host = ctx.frames("planar", opt["calls"][0], 0)
    sets = [[[im for im, _ in fs] for fs in c] for c in host]
    want = rc.stream(oracle, ctx.geo, ctx.steps, sets[:4], chain)
    monitored = rc.stream(oracle, ctx.geo, ctx.steps, sets[:4], dict(chain, monitor=2))  # (a monitor changes nothing but its records)
    dev = [[[_dev_frame(gpu, im, 0) for im in fs] for fs in c] for c in sets]
    scale, crop = l2.scale_of("eighth", ctx.cw, ctx.ch), (ctx.inscribed, 1)
    rig = _make(ctx, opt)
    try:
        rig.fix_seams(ctx.given)  # fixed vertical seams rest while paths are set
        rig.set_seam_anchor(*chain["anchor"]).set_seam_paths(l2.MAX_STEP, l2.MARGIN).set_exposure_smoothing(192)
        toggles = [(dict(), lambda p: p),
                   (dict(scale=scale), lambda p: sr.scale(p, *scale)),
                   (dict(crop=crop, monitor=2), lambda p: np.ascontiguousarray(p[:, crop[0][1]:crop[0][1] + crop[0][3], crop[0][0]:crop[0][0] + crop[0][2]])),
                   (dict(out_fmt=pyr.YUYV, matrix=2, out_pitch=pyr.tight(pyr.YUYV, ctx.cw)), lambda p: pyr.pack(p, pyr.YUYV, 2))]
        for c, (extra, after) in enumerate(toggles):
            rig.clear_output_scale().clear_crop().clear_monitor().clear_formats()
            if "scale" in extra:
                rig.set_output_scale(*scale)
            if "crop" in extra:
                rig.set_crop(*crop).set_monitor(2)
            if "out_fmt" in extra:
                rig.set_formats(pyr.PLANAR, pyr.YUYV, 2)
            o = dict(opt, scale="eighth" if "scale" in extra else None, crop=1 if "crop" in extra else 0)
            res = _stitch(rig, ctx, o, dict(chain, **extra), dev[c])
            plain = [dict(w, out=after(w["out"])) for w in want[c][0]]  # (the planar result of the stream that never toggled)
            if "monitor" in extra:
                plain = [dict(w, records=m["records"]) for w, m in zip(plain, monitored[c][0])]
            _against_cpu(ctx, dict(chain, **extra), res, plain, want[c][1], f"call {c}")
        # clear_seam_paths forgets the last paths and the anchor and keeps the anchor's options; the fixed seams are back
        assert rig.seam_anchor() == (chain["anchor"], True)
        rig.clear_formats().clear_seam_paths()
        assert rig.seam_anchor() == (chain["anchor"], False) and rig.seam_paths is None and [tuple(s[:4]) for s in rig.seams] == [tuple(g) for g in ctx.given]
        with pytest.raises(capi.StitchError):
            rig.last_seam_paths(0, 0)
        given = dict(chain, seams=("given", ctx.given), anchor=None)
        state = dict(anchor=None, smooth=want[3][1]["smooth"])  # the smoothing state goes on
        (w4, s4), = rc.stream(oracle, ctx.geo, ctx.steps, sets[4:5], given, state)
        _against_cpu(ctx, given, _stitch(rig, ctx, opt, given, dev[4]), w4, s4, "given seams after the clear")
        rig.set_seam_paths(l2.MAX_STEP, l2.MARGIN)  # paths again: no anchor to lean on, the first set is unanchored
        with pytest.raises(capi.StitchError):
            rig.last_seam_paths(0, 0)
        (w5, s5), = rc.stream(oracle, ctx.geo, ctx.steps, sets[5:6], chain, dict(anchor=None, smooth=s4["smooth"]))
        res = _stitch(rig, ctx, opt, chain, dev[5])
        _against_cpu(ctx, chain, res, w5, s5, "paths after the clear")
        assert all(m == 0 for _, _, m in res["paths"][0]) and rig.seam_anchor() == (chain["anchor"], True)
    finally:
        rig.close()


def test_a_seam_that_repeats_and_then_moves(st, gpu, oracle, plans):
    """Content seams, no exposure mode: the same set three times in one call at max_sets 2, then a set whose seam differs (a hole in
    the overlap) -- a slot keeps its mask pyramid while its seam repeats and must not keep it when it moves.  Then path seams on the
    same handle, then content seams again.  Every output is the CPU's.  (The keep counts are a plan's: tests/test_gpu_mask_keep.py.)"""
    ctx = _context(oracle, "w64_65", gpu)
    opt = dict(l2.NONE, calls=((4,), 2), index=0)
    same = ctx.frames("planar", (1,), 0)[0][0]
    holed = ctx.frames("planar", (1,), 0, hole=(0, ctx.steps[0]["src"]))[0][0]
    host = [[same, same, same, holed]]
    rig = _make(ctx, opt)
    try:
        content = _run_row(rig, ctx, opt, oracle, plans, host=host)
        assert content[0]["seams"][0] == content[0]["seams"][1] == content[0]["seams"][2] != content[0]["seams"][3]
        assert l2.same(content[0]["outs"][0], content[0]["outs"][2]) and not l2.same(content[0]["outs"][2], content[0]["outs"][3])
        pathed = _run_row(rig, ctx, dict(opt, seams="paths"), oracle, plans, host=host)
        assert not l2.same(pathed[0]["outs"][0], content[0]["outs"][0])
        again = _run_row(rig, ctx, opt, oracle, plans, host=[[holed, same, same, holed]])
        assert l2.same(again[0]["outs"][0], content[0]["outs"][3]) and l2.same(again[0]["outs"][1], content[0]["outs"][0])
    finally:
        rig.close()


@pytest.mark.parametrize("seams", ["paths_set", "content"])
def test_a_dark_set_in_mid_stream(st, gpu, oracle, plans, seams):
    """A frame of zeros at step 1's source in set 1 of the 3 + 2 stream, with smoothing, a YUYV output and the coprime scale.
    Along paths no set fails for its pixels (stitch_seam_path.h): the dark set's status is OK, its statistics at step 1 are not valid
    and never enter the state, and the anchor and the state go on into the second call.  With content seams the set fails at step 1,
    and the replay leaves the rig without a state (stitch_rig_exposure_temporal.h); the second call starts a stream of its own."""
    ctx = _context(oracle, "w64_65", gpu)
    opt = dict(l2.NONE, exposure=(1, ("keep", 192)), seams=seams, scale="coprime", output="yuyv_padded", calls=STREAM, index=1)
    rig = _make(ctx, opt)
    try:
        res = _run_row(rig, ctx, opt, oracle, plans, dark=(1, ctx.steps[1]["src"]))
        if seams == "content":
            assert res[0]["status"][0] == 0 and res[0]["status"][2] == 0 and res[0]["status"][1] in (capi.ERR_EMPTY_MIDROW, capi.ERR_ZERO_OVERLAP)
            assert res[0]["state"][1] == [False, False] and not res[0]["state"][0].any() and res[1]["state"][1] == [True, True]
        else:
            assert res[0]["status"] == [0, 0, 0] and res[0]["anchor"][1] and res[0]["state"][1] == [True, True]
            assert not rc.et.valid(res[0]["stats"][1][1]) and rc.et.valid(res[0]["stats"][2][1])
    finally:
        rig.close()
