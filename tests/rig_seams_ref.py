"""The CPU yardstick of fixed seams (include/stitch_rig_seams.h), on tests/oracle_lib.py.  TEST INFRASTRUCTURE ONLY, shared by
tests/test_rig_seams_host.py, tests/test_gpu_rig_seams.py and tests/golden/make_rig_seams_goldens.py.

derive       ratio / ov / branch / start / threshold from the four integers, in numpy scalars (ImageProcess.cpp:686-698)
blend_given  blend_core of oracle/stitch_oracle.c restated over Oracle.blur / decimate / expand / pyramid_levels, with the mask of a
             GIVEN seam: float32 `A - expand`, float32 `a * m`, float64 sum, cast, and a clip to [0, 255] per collapse level.
             tests/test_rig_seams_host.py pins it to Oracle.blend on the oracle's own seam, bit for bit.
chain_given  project, warp, move, blend_given per step, finish: the single-set chain with given seams.
coverage_chain  the coverage recursion on 0 / 255 indicator images through Oracle.project / warp / move (pure gathers), the seam of
             every step from Oracle.seam on the indicators.
"""
import numpy as np

from oracle_lib import ROOT_OPTS


SMALL = [(64, 48)] * 3  # the three-frame rig of tests/test_gpu_rig.py, restated


def shift(tx, ty, c=1e-4, d=5e-5):
    """A translation by (tx, ty) with a small xy term, and (nearly) its inverse: (forward map, backward map)."""
    return [1.0, 0.0, c, float(tx), 0.0, 1.0, d, float(ty)], [1.0, 0.0, -c, -float(tx), 0.0, 1.0, -d, -float(ty)]


def hand_steps(capi, sizes, moves, start=0):
    """Step dicts of a hand-made rig: moves = [(frame to warp, forward map, backward map)], the canvases from capi.step_geometry
    (host arithmetic only)."""
    steps, (mw, mh) = [], sizes[start]
    for dst, p_fwd, p_bwd in moves:
        g = capi.step_geometry(sizes[dst][0], sizes[dst][1], p_fwd, mw, mh)
        steps.append(dict(start=start, src=dst, p=p_bwd, p_fwd=p_fwd, offx=g.min_x, offy=g.min_y, ox=g.ox, oy=g.oy, cw=g.cw, ch=g.ch))
        mw, mh = g.cw, g.ch
    return steps


def small_steps(capi):
    return hand_steps(capi, SMALL, [(1,) + tuple(shift(31.5, 1.25)), (2,) + tuple(shift(-29.75, -0.5))])


def twice_steps(capi):
    """The second frame lies inside the mosaic: both steps have one canvas size and run on one workspace."""
    return hand_steps(capi, SMALL, [(1,) + tuple(shift(31.5, 1.25)), (2,) + tuple(shift(14.0, 0.5, 2e-5, 1e-5))])


def failure_cases(capi):
    """Rigs whose footprints give no seam at step 1, after a good step 0: name -> (sizes, steps, the status of step 1).  Both
    canvases still have a pyramid (no level with a zero dimension), so the rigs replay: the wide one is of taller frames."""
    good = (1,) + tuple(shift(31.5, 1.25))
    tall = [(64, 70)] * 3
    return {"no_overlap": (tall, hand_steps(capi, tall, [good, (2,) + tuple(shift(-100.0, 0.5))]), -3),  # a shift wider than the frame
            "clear_of_mid_row": (SMALL, hand_steps(capi, SMALL, [good, (2,) + tuple(shift(10.0, 80.0))]), -2)}


def derive(four, seam_rule):
    """-> (branch, start, thr): mask = 1 where (double)x < thr (branch 0) or x >= start (branch 1)."""
    s_a, n_a, s_o, n_o = (int(v) for v in four[:4])
    if seam_rule == 0:
        ratio, ov = np.float32(s_a / n_a), np.float32(s_o / n_o)  # a double quotient rounded to float
        return (0 if ratio < ov else 1), int(np.float32(ov + np.float32(1))), float(ov)
    ratio, ov = s_a / n_a, s_o / n_o
    return (0 if ratio < ov else 1), int(ov + 1.0), ov


def seam_mask(four, seam_rule, cw, ch):
    branch, start, thr = derive(four, seam_rule)
    x = np.arange(cw)
    row = (x.astype(np.float64) < thr) if branch == 0 else (x >= start)
    return np.ascontiguousarray(np.broadcast_to(row.astype(np.float32), (1, ch, cw)))


def blend_given(oracle, a, b, opts, four):
    """blendTwoImages on canvases a, b (3, h, w) of one pixel type with the seam stated by its four integers -> the blend, same type."""
    opts = dict(ROOT_OPTS, **(opts or {}))
    _, h, w = a.shape
    L, lw, lh = oracle.pyramid_levels(w, h, opts["level_rule"])
    assert L >= 1
    A, B = [np.ascontiguousarray(a, np.float32)], [np.ascontiguousarray(b, np.float32)]
    M = [seam_mask(four, opts["seam_rule"], w, h)]
    for i in range(1, L):  # REDUCE
        for G in (A, B, M):
            G.append(oracle.decimate(oracle.blur(G[i - 1], opts["sigma"], opts["blur_kind"]), lw[i], lh[i]))
    for i in range(L - 1):  # Laplacian, finest first: G[i + 1] is still Gaussian when it is expanded
        A[i] = A[i] - oracle.expand(A[i + 1], lw[i], lh[i])
        B[i] = B[i] - oracle.expand(B[i + 1], lw[i], lh[i])
    for i in range(L):
        m = M[i]
        am = A[i] * m  # a float product
        A[i] = (am.astype(np.float64) + B[i].astype(np.float64) * (1.0 - m.astype(np.float64))).astype(np.float32)
    E = A[L - 1]
    for i in range(L - 2, -1, -1):
        E = np.clip(A[i] + oracle.expand(E, lw[i], lh[i]), np.float32(0), np.float32(255))
    return E.astype(np.uint8) if a.dtype == np.uint8 else E


def pair_given(oracle, frame, st, mosaic, opts, four):
    """One step with a given seam: Oracle.warp / Oracle.move onto zero canvases, then blend_given."""
    a = oracle.warp(frame, st["p"], st["offx"], st["offy"], st["cw"], st["ch"])
    b = oracle.move(mosaic, st["ox"], st["oy"], st["cw"], st["ch"])
    return blend_given(oracle, a, b, opts, four)


def chain_given(oracle, frames, steps, seams, opts=None, finish=True, num=19.0, den=20.0, fov_deg=15.0):
    """pipeline.stitch_chain(seams=...) on the CPU: frames are (3, H, W) uint8 arrays, steps the step dicts."""
    proj = {}

    def projected(i):
        if i not in proj:
            proj[i] = oracle.project(np.ascontiguousarray(frames[i]), fov_deg)
        return proj[i]

    result = projected(steps[0]["start"])
    for st, four in zip(steps, seams):
        result = pair_given(oracle, projected(st["src"]), st, result, opts, four)
    if finish:
        result = oracle.lummix(result, oracle.equalize(result)[0], num, den)
    return result


def coverage_chain(oracle, sizes, start, steps, fov_deg=15.0, seam_rule=0):
    """-> (per step dict(A, B, U: (ch, cw) bool; rc: Oracle.seam's status; seam: its tuple), C_proj(start)).  sizes: (width, height)
    per frame; steps: step dicts (src = the frame that is warped)."""
    cproj = {}

    def cov(i):
        size = tuple(sizes[i])
        if size not in cproj:
            w, h = size
            cproj[size] = np.ascontiguousarray((oracle.project(np.full((3, h, w), 255, np.uint8), fov_deg) != 0) * np.uint8(255))
            assert (cproj[size][0] == cproj[size][1]).all() and (cproj[size][0] == cproj[size][2]).all()
        return cproj[size]

    mos, out = cov(start), []
    for st in steps:
        a = oracle.warp(cov(st["src"]), st["p"], st["offx"], st["offy"], st["cw"], st["ch"])
        b = oracle.move(mos, st["ox"], st["oy"], st["cw"], st["ch"])
        rc, sm = oracle.seam(a, b, seam_rule)
        out.append(dict(A=a[0] != 0, B=b[0] != 0, U=(a[0] != 0) | (b[0] != 0), rc=rc, seam=sm.as_tuple()))
        mos = np.maximum(a, b)
    return out, cov(start)[0] != 0
