"""The CPU statement of the WHOLE rig replay (rig_stitch of csrc/stitch_rig.inc): one call of a stream of sets through every option,
composed from the references the project already has -- no arithmetic of its own.  TEST INFRASTRUCTURE ONLY, host only, shared by
tests/test_rig_lattice2_host.py and tests/test_gpu_rig_lattice2.py.

  projection, warp, move, seam scan, transfer, equalize, lummix   tests/oracle_lib.py
  fixed seams, their blend, the coverage recursion                  tests/rig_seams_ref.py (blend_given, coverage_chain)
  path seams, their cost, finder and blend                          tests/seam_path_ref.py, tests/seam_anchor_ref.py
  smoothed and fixed statistics                                     tests/exposure_temporal_ref.py (filter_stream, apply_given)
  the monitor's records, the inscribed rectangle, the scale         tests/residual_ref.py, tests/rect_ref.py, tests/scale_ref.py
  camera layouts                                                    tests/pixfmt_ref.py through tests/pixfmt_yuv_ref.py

THE ORDER, per set, is the one the headers state: unpack; project; per step [the transfer with measured, filtered or fixed statistics
(stitch_rig_exposure_temporal.h); the monitor's record of the blend's two inputs (stitch_rig_monitor.h); the seam or the path
(stitch_rig_seams.h, stitch_seam_path.h, stitch_seam_anchor.h); the blend]; the crop and the finish pass by the crop's mode
(stitch_rig_crop.h); the scale (stitch_rig_scale.h); the pack (stitch_rig_formats.h, stitch_rig_formats_yuv.h).

THE STATE a rig carries from set to set: per step the anchor path (policy "set": set i anchors on set i - 1, across calls; policy
"call": every set of a call anchors on the previous call's last set, and the anchor is replaced once, at the call's end) and per step
the smoothing state of the statistics' filter.  A call in which a set fails leaves the rig with neither.  How a rig cuts a call into
launch sequences (max_sets) does not appear here: its results do not depend on it.

OPTIONS (a dict; every key optional):
  mode      0, 1, 2: the exposure mode the rig was made with                    keep_black  True
  keep      None or 0 .. 255: smoothing                                         fixed       None or (n_steps, 12): fixed statistics
  seams     ("content",) | ("given", [four integers per step]) | ("paths", max_step, margin) | ("fixed_paths", [a path per step])
  anchor    None or (weight, cap, "set" | "call"); read only with ("paths", ...)
  crop      None or ((x0, y0, w, h), mode 1 | 2)                                scale       None or (ow, oh)
  in_fmt, out_fmt, matrix   codes of tests/pixfmt_yuv_ref.py; 0 = planar        out_pitch   None (tight) or (pitch, pitch2)
  finish    True                          num, den  19, 20                      monitor     None or the radius
The three `wrong_*` keys are deliberate MIS-statements that only tests/test_rig_lattice2_host.py sets, to show that the statement is
sensitive where a rig could go wrong: wrong_scale_first (the scale before a mode-2 finish pass), wrong_anchor_cut = n (the anchor
dropped every n sets, as at a launch sequence's boundary), wrong_smoothing_cut (the smoothing state dropped at the call's start).
"""
import numpy as np

import exposure_temporal_ref as et
import pixfmt_yuv_ref as pyr
import rect_ref
import residual_ref as rr
import rig_seams_ref as ref
import scale_ref as sr
import seam_anchor_ref as sa
import seam_path_ref as sp
from oracle_lib import ROOT_OPTS


def geometry(oracle, sizes, steps):
    """What a rig knows of itself before any frame: per step the coverage masks and the geometric seam, and the inscribed rectangle
    of the output."""
    cov, _ = ref.coverage_chain(oracle, sizes, steps[0]["start"], steps)
    assert all(c["rc"] == 0 for c in cov)
    return dict(cov=cov, geometric=[tuple(c["seam"]) for c in cov], branches=[int(c["seam"][4]) for c in cov], inscribed=rect_ref.stack(cov[-1]["U"]))


def empty_state(n_steps):
    return dict(anchor=None, smooth=[None] * n_steps)


def _copy_state(state, n_steps):
    state = state or empty_state(n_steps)
    return dict(anchor=None if state["anchor"] is None else [np.asarray(p, np.int32).copy() for p in state["anchor"]],
                smooth=[None if p is None else np.asarray(p, np.float32).copy() for p in state["smooth"]])


def _finish(oracle, img, opt):
    return oracle.lummix(img, oracle.equalize(img)[0], opt.get("num", 19.0), opt.get("den", 20.0))


def _output(oracle, mosaic, opt):
    """The crop and the finish pass by the crop's mode, the scale, the pack."""
    finish, crop, scale = opt.get("finish", True), opt.get("crop"), opt.get("scale")
    if crop is None:
        out = _finish(oracle, mosaic, opt) if finish else mosaic
    else:
        (x0, y0, w, h), mode = crop
        assert mode in (1, 2)
        if finish and mode == 1:
            mosaic = _finish(oracle, mosaic, opt)
        out = np.ascontiguousarray(mosaic[:, y0:y0 + h, x0:x0 + w])
        if finish and mode == 2:
            if opt.get("wrong_scale_first") and scale is not None:
                out, scale = sr.scale(out, *scale), None
            out = _finish(oracle, out, opt)
    if scale is not None:
        out = sr.scale(np.ascontiguousarray(out), *scale)
    fmt = opt.get("out_fmt", 0)
    if not fmt:
        return np.ascontiguousarray(out)
    pitch, pitch2 = opt.get("out_pitch") or (None, None)
    return pyr.pack(out, fmt, opt.get("matrix", 0), pitch, pitch2 or None, fill=0xEE)


def one_set(oracle, geo, steps, frames, opt, anchors, smooth):
    """One set through every step.  anchors: per step a path or None; smooth: per step the filter's state or None, UPDATED in place.
    -> dict(status, out, seams, measured, used, paths, costs, moved, records)."""
    mode, kb = opt.get("mode", 0), opt.get("keep_black", True)
    keep, fixed = opt.get("keep"), opt.get("fixed")
    seams, radius = opt.get("seams", ("content",)), opt.get("monitor")
    in_fmt, matrix = opt.get("in_fmt", 0), opt.get("matrix", 0)
    proj = {}

    def projected(i):
        if i not in proj:
            planar = pyr.unpack(frames[i], matrix) if in_fmt else np.ascontiguousarray(frames[i])
            proj[i] = oracle.project(planar)
        return proj[i]

    n = len(steps)
    res = dict(status=0, out=None, seams=[], measured=np.zeros((n, 12), np.float32), used=np.zeros((n, 12), np.float32), paths=[], costs=[], moved=[],
               records=None if radius is None else np.zeros((n, rr.words(radius)), np.int64))
    mosaic = projected(steps[0]["start"])
    for k, st in enumerate(steps):
        cw, ch, cov = st["cw"], st["ch"], geo["cov"][k]
        x = projected(st["src"])
        if mode:
            if fixed is not None:  # nothing is measured: the statistics output receives the fixed values
                m = u = np.asarray(fixed[k], np.float32)
                x = et.apply_given(oracle, x, u, kb)
            else:
                out, m = oracle.transfer(x, projected(st["mosaic_src"]) if mode == 1 else mosaic)
                if keep is None:
                    u = m
                    if kb:
                        out[:, (x == 0).all(axis=0)] = 0
                    x = out
                else:
                    used, smooth[k] = et.filter_stream(m[None], keep, smooth[k])
                    u = used[0]
                    x = et.apply_given(oracle, x, u, kb)
            proj[st["src"]] = x
            res["measured"][k], res["used"][k] = m, u
        a = oracle.warp(x, st["p"], st["offx"], st["offy"], cw, ch)
        b = oracle.move(mosaic, st["ox"], st["oy"], cw, ch)
        if radius is not None:
            res["records"][k] = rr.records(a, b, rr.rig_domain(cov["A"], cov["B"], radius), radius)
        if seams[0] in ("paths", "fixed_paths"):
            branch = geo["branches"][k]
            if seams[0] == "paths":
                w, cap = opt["anchor"][:2] if anchors[k] is not None else (0, 1)
                path, cost, moved = sa.anchored_path(sp.cost(a, b, cov["A"], cov["B"], branch, seams[2]), seams[1], anchors[k], w, cap)
            else:
                path, cost, moved = np.asarray(seams[1][k], np.int32), 0, 0
            mosaic = sp.blend_with_mask_as(oracle, a, b, sp.mask_from_path(path, branch, cw), ROOT_OPTS)
            res["paths"].append(np.asarray(path, np.int32))
            res["costs"].append(int(cost))
            res["moved"].append(int(moved))
            res["seams"].append(geo["geometric"][k])
        else:
            if seams[0] == "given":
                four = tuple(int(v) for v in seams[1][k][:4])
            else:
                rc, sm = oracle.seam(a, b, ROOT_OPTS["seam_rule"])
                if rc != 0:  # the set fails here for its pixels; what it has so far means nothing
                    res["status"] = rc
                    return res
                four = sm.as_tuple()
            mosaic = ref.blend_given(oracle, a, b, None, four)
            res["seams"].append(four)
    res["out"] = _output(oracle, mosaic, opt)
    return res


def call(oracle, geo, steps, sets, opt, state=None):
    """One stitch() call.  sets: per set the frames (reference images of in_fmt, or (3, H, W) arrays for a planar input).
    state: what the rig carried into the call (None: nothing).  -> (per set one_set's dict, the state after the call)."""
    n = len(steps)
    state = _copy_state(state, n)
    if opt.get("wrong_smoothing_cut"):
        state["smooth"] = [None] * n
    seams = opt.get("seams", ("content",))
    anchored = seams[0] == "paths" and opt.get("anchor") is not None
    policy = opt["anchor"][2] if anchored else None
    anchors, out = state["anchor"], []
    for i, frames in enumerate(sets):
        if opt.get("wrong_anchor_cut") and i and i % opt["wrong_anchor_cut"] == 0:
            anchors = None
        r = anchors if anchored and anchors is not None else [None] * n
        out.append(one_set(oracle, geo, steps, frames, opt, r, state["smooth"]))
        if policy == "set" and out[-1]["status"] == 0:
            anchors = out[-1]["paths"]
    if any(r["status"] != 0 for r in out):  # a replay in which a set fails leaves the rig without an anchor and without a state
        return out, empty_state(n)
    if anchored and out:  # either policy: the call's last set (under any other seam source the anchor a rig holds rests)
        state["anchor"] = [p.copy() for p in out[-1]["paths"]]
    return out, state  # (one_set moved state["smooth"] on wherever the filter ran; fixed statistics and no option leave it alone)


def stream(oracle, geo, steps, calls, opt, state=None):
    """Calls in a row on one rig -> (per call (results, the state after it))."""
    out = []
    for sets in calls:
        results, state = call(oracle, geo, steps, sets, opt, state)
        out.append((results, state))
    return out
