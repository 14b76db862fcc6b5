"""Which launch forms the pair path takes at DEFAULT switches, and the small cases that reach every one of them.  A plain module: no
torch, no GPU.  tests/test_form_cover_host.py holds the table below to the grid with tests/call_form_dump.cpp (the decision compiled by
the host compiler alone), tests/test_gpu_form_cover.py runs every case of the table against the oracle, scripts/trace_call_forms.py
walks the table for a dispatch trace.

signature(record, level): what the launch code (csrc/stitch_hip.hip) branches on, or passes as a template argument, when it reduces
and collapses one level of a call -- taken from call_form_dump's JSON record of the call.  Sizes and counts (NR, NC, nbx, crows,
pitches, grids) are left out: two levels with one signature run the same kernel instances with other arguments.  The fields and
the launch site that reads each:

  level      "L0" | "Ln": run_reduce (fill_mask and the row flags of the fused sweep at l > 0; the flag arrays' index l - 1);
             run_collapse (CollapseArgs<OUT, true> with the seam's step and the caller's output at level 0, <float, false> above it)
  sweep      run_reduce: k_vv_xbyf ("batch"), the separate sweeps ("lone"), k_deriche ("deriche")
  x_fwd      run_reduce: the copy, k_vv_x_fwd, k_vv_x_m<true>
  x_bwd      run_reduce: none, k_vv_x_m<false>, k_vv_x_bwd
  y_fwd      run_reduce: none, k_vv_y_m, k_vv_y_fwd1s, k_vv_y_fwd1, k_vv_y_fwd
  y_bwd      run_reduce: none, launch_y_bwd_dec, k_vv_y_bwd_dec7<dec_odd>, k_vv_y_bwd
  do_x do_y  run_reduce: the two k_deriche launches (the Van Vliet kernels' choice already holds them)
  rcmp stamp launch_xbyf's instances, k_vv_x_fwd<.., CKPT> (always off at default switches; kept so that the tuple names an instance)
  xby        run_reduce: k_vv_xby_m, and where the anticausal y sweep finds the causal one's state
  src0       run_reduce: the SRC instances of k_vv_x_fwd / k_vv_x_m, launch_xbyf; run_collapse: the gathers of level 0 (CallForm::src)
  mask_l0    run_reduce: MaskL0 of every sweep of level 0, Wavefront::mask_l0
  zt rowz    run_reduce: the T flags handed to k_vv_x_fwd, the fused sweep and launch_y_bwd_dec; Wavefront::mask_l0 = 2;
             launch_y_bwd_dec<rowz, ..>
  per_plane  run_reduce: Bands of the x sweeps
  g_in g_out mr_in mr_out   run_reduce: the flag records of k_vv_x_fwd (read) and launch_y_bwd_dec (written); run_collapse: gz / gzn
  fill_mask  run_reduce: fill_l0 of launch_y_bwd_dec, Wavefront::mr
  dec_zt dec_odd   launch_y_bwd_dec's template arguments; k_vv_y_bwd_dec7<dec_odd>
  decimate   run_reduce: k_decimate behind the sweeps
  gen px c_mr   launch_collapse: CollapseKind
  c4         launch_collapse: "none" (xb == xa: k_collapse / k_collapse_px), "full" (the four-column range covers every column: no
             one-column blocks), "part" (both kinds of block in one launch)
  w4         launch_collapse at level 0: the width is a multiple of four (u8_words)
  a_dense    run_collapse at level 0: the dense instances of k_collapse4 at a source-fused level 0
LevelForm::odd_dec is not in the list: no launch site reads it (it decides y_bwd and decimate, which are), and at default switches
it equals dec_odd at every level that is reduced.

call_signature(record): what a call launches around its levels, once per call and whatever the levels' forms -- a signature of its
own, so that it does not multiply the levels':
  src a_dense   run_pairs: k_src_index, k_load_canvases or k_compose in front of the seam scan
  mask_opt   run_seam_mask: k_mask behind the scan, or the implicit mask
  wf_ctrl    run_reduce: the clear of the band-queue heads in front, the fetch of the time-out count behind
  coarse coarse_lds   run_reduce: k_coarse / k_coarse_lds behind the last level; run_collapse: k_blend_top without them
  zi         run_pairs: the index plane's zero-tile flags (source-fused pairs on a plan with zero-tile flags), filled and handed on
  one_pair   run_seam_mask: the seam scan's workgroup of 1024 work-items instead of 256
  top_only   run_collapse: a one-level pyramid reduces nothing, k_blend_top and k_emit_top alone

The grid: canvases SIDES x SIDES, capacities CAPS, n in {1, 2, cap}, pairs for every n and the dense blend for n = 1, the four
option sets OPTION_SETS.  A canvas without a valid pyramid under its rule is no part of it (the dump prints null for it, the library
and the oracle refuse it).  CASES covers what the calls of at most MAX_PIXELS = cw * ch * n reach, each case within that bound;
WIDE_CASES covers what only the larger calls of the grid reach -- 4 or 16 pairs of a large canvas, up to 16 pairs of 2052 x 2052 --
each case the cheapest call that reaches its signatures.  Together they reach every signature of the grid.  Above the grid are the
full-size tests (LARGE)."""
import g_flags_ref

SIDES = [3, 5, 33, 64, 65, 67, 128, 130, 131, 255, 256, 258, 270, 300, 511, 512, 514, 517, 527, 620, 768, 770, 836, 1000, 1022, 1023, 1024, 1025,
         1026, 1027, 1081, 1100, 1101, 1335, 2046, 2047, 2048, 2049, 2050, 2052, 2100]
CAPS = [1, 2, 3, 4, 16]
OPTION_SETS = {
    "vv0": dict(sigma=2.0, blur_kind=0, level_rule=0, seam_rule=0),
    "vv1": dict(sigma=2.0, blur_kind=0, level_rule=1, seam_rule=0),
    "deriche": dict(sigma=2.0, blur_kind=1, level_rule=0, seam_rule=0),
    "skip": dict(sigma=0.3, blur_kind=0, level_rule=0, seam_rule=0),  # below the blur's threshold: REDUCE decimates G itself
}
MAX_SIDE, MAX_PIXELS = 2100, 2100 * 2100 * 2  # the bound of a case: sides, and cw * ch * n

LEVEL_FIELDS = ("sweep", "x_fwd", "x_bwd", "y_fwd", "y_bwd", "do_x", "do_y", "rcmp", "stamp", "xby", "src0", "mask_l0", "zt", "rowz", "per_plane", "g_in", "g_out",
                "mr_in", "mr_out", "fill_mask", "dec_zt", "dec_odd", "decimate", "gen", "px", "c_mr")
CALL_FIELDS = ("src", "a_dense", "mask_opt", "wf_ctrl", "coarse", "coarse_lds")
KERNEL_FIELDS = ("sweep", "x_fwd", "x_bwd", "y_fwd", "y_bwd")  # strings in the record; the rest are 0 / 1


def signature(rec, level):
    """The tuple of (field, value) of one reduced level of a record; field order as in the module's docstring."""
    f = rec["levels"][level]
    cols = f["w"] if level == 0 else f["pitch"]
    c4 = "none" if f["xb"] == f["xa"] else "full" if f["xb"] - f["xa"] == cols else "part"
    sig = [("level", "L0" if level == 0 else "Ln")] + [(k, f[k]) for k in LEVEL_FIELDS]
    return tuple(sig + [("c4", c4), ("w4", int(level == 0 and f["w"] % 4 == 0)), ("a_dense", int(level == 0 and rec["a_dense"]))])


def call_signature(rec):
    """The tuple of (field, value) of what a call launches around its levels."""
    zi = int(bool(rec["src"] and rec["zero_tiles"] and not rec["a_dense"]))
    return (("level", "call"),) + tuple((k, rec[k]) for k in CALL_FIELDS) + (("zi", zi), ("one_pair", int(rec["n"] == 1)), ("top_only", int(rec["l_end"] == 0)))


def signatures(rec):
    """The signatures of a record as names (see name): the call's, and one per reduced level."""
    return {name(call_signature(rec))} | {name(signature(rec, l)) for l in range(rec["l_end"])}


def name(sig):
    """A signature as one line of text: the level class, the kernels of the four sweeps and the collapse's column range, then every
    flag that is set."""
    d = dict(sig)
    short = {"k_vv_x_fwd": "x_fwd", "k_vv_x_m": "x_m", "k_vv_x_bwd": "x_bwd", "k_vv_y_m": "y_m", "k_vv_y_fwd1s": "y_fwd1s", "k_vv_y_fwd1": "y_fwd1",
             "k_vv_y_fwd": "y_fwd", "k_vv_y_bwd_dec": "dec", "k_vv_y_bwd_dec7": "dec7", "k_vv_y_bwd": "y_bwd"}
    words = [d["level"]]
    if d["level"] != "call":
        words += [d["sweep"], "/".join(short.get(d[k], d[k]) for k in KERNEL_FIELDS[1:]), "c4:" + d["c4"]]
    return " ".join(words + [k for k, v in sig if k not in KERNEL_FIELDS and k not in ("level", "c4") and v])


def dump_case(cw, ch, cap, n, dense, opts):
    """A case as tests/test_call_form_host.py's dump() takes it: default switches, source fusion as the library decides it."""
    return (cw, ch, cap, n, -1, bool(dense), OPTION_SETS[opts], False, {})


def grid():
    """Every (cw, ch, cap, n, dense, option set) of the grid, canvases without a valid pyramid included (the dump answers null)."""
    for opts in OPTION_SETS:
        for cw in SIDES:
            for ch in SIDES:
                for cap in CAPS:
                    for n in sorted({1, 2, cap}):
                        if n <= cap:
                            yield (cw, ch, cap, n, False, opts)
                            if n == 1:
                                yield (cw, ch, cap, n, True, opts)


def small(case):
    """The call has at most MAX_PIXELS: a case of CASES; the rest of the grid (4 or 16 pairs of a large canvas) is WIDE_CASES'."""
    return case[0] * case[1] * case[3] <= MAX_PIXELS


# The (cw, ch, cap, n) of the three full-size GPU tests, at default switches and options: what they reach beyond the grid is recorded in
# tests/golden/form_cover_large.json (the lone fused sweep from 20 MPix per plane, a pair that fills the chip, rows of 4096 columns and more)
LARGE = {
    "test_gpu_golden::test_config2_full_size_against_oracle": [(6144, 4096, 1, 1, False, "vv0")],
    "test_gpu_golden::test_config5_size_single_gpu_against_oracle": [(24576, 16384, 1, 1, False, "vv0")],
    "test_gpu_benchpath::test_benchmarked_batch_full_size_against_oracle": [(6144, 4096, 16, 16, False, "vv0"), (6144, 4096, 8, 8, False, "vv0")],
}


def inputs(cw):
    """name -> (frame width, map, mosaic width, mosaic ox, seam branch or None) of the four pair inputs of a canvas cw wide:
    g_flags_ref.cases(cw) wherever its 64-column frames and 40-column margins fit; on a narrower canvas the same four placements with the
    narrow image a third of the canvas and an overlap of half of that (at least one column), a pure shift for every map, and no
    statement about the seam's branch."""
    if cw >= 128:
        return g_flags_ref.cases(cw)
    k = max(1, cw // 3)
    ov = max(1, k // 2)
    wide = cw - k + ov
    return {
        "frame_right": (k, g_flags_ref.shift(cw - k), wide, 0, None),
        "frame_left": (k, g_flags_ref.shift(0), wide, -(cw - wide), None),
        "mosaic_left": (wide, g_flags_ref.shift(cw - wide), k, 0, None),
        "mosaic_right": (wide, g_flags_ref.shift(0), k, -(cw - k), None),
    }


# (cw, ch, cap, n, dense, option set, the signatures the case is in the table for).  Chosen by a greedy cover of the grid's signatures
# that prefers a small cw * ch * n; the search is not kept, tests/test_form_cover_host.py holds the result to the grid.
CASES = [
    (5, 3, 1, 1, False, "deriche", [
        "L0 deriche copy/none/none/none c4:none do_x do_y dec_odd decimate",
    ]),
    (5, 3, 1, 1, True, "deriche", [
        "L0 deriche copy/none/none/none c4:none do_x do_y dec_odd decimate a_dense",
    ]),
    (64, 33, 1, 1, False, "deriche", [
        "L0 deriche copy/none/none/none c4:none do_x do_y decimate w4",
    ]),
    (64, 33, 1, 1, True, "deriche", [
        "L0 deriche copy/none/none/none c4:none do_x do_y decimate w4 a_dense",
        "Ln deriche copy/none/none/none c4:none do_x do_y decimate px",
    ]),
    (67, 33, 1, 1, True, "deriche", [
        "Ln deriche copy/none/none/none c4:none do_x do_y dec_odd decimate px",
    ]),
    (130, 64, 1, 1, False, "deriche", [
        "L0 deriche copy/none/none/none c4:none do_x do_y decimate",
    ]),
    (130, 64, 1, 1, True, "deriche", [
        "L0 deriche copy/none/none/none c4:none do_x do_y decimate a_dense",
    ]),
    (256, 128, 1, 1, False, "deriche", [
        "L0 deriche copy/none/none/none c4:full do_x do_y decimate gen w4",
    ]),
    (256, 128, 1, 1, True, "deriche", [
        "L0 deriche copy/none/none/none c4:full do_x do_y decimate gen w4 a_dense",
    ]),
    (256, 514, 16, 16, False, "deriche", [
        "Ln deriche copy/none/none/none c4:none do_x do_y decimate",
    ]),
    (258, 128, 1, 1, False, "deriche", [
        "L0 deriche copy/none/none/none c4:part do_x do_y decimate gen",
    ]),
    (258, 128, 1, 1, True, "deriche", [
        "L0 deriche copy/none/none/none c4:part do_x do_y decimate gen a_dense",
    ]),
    (300, 128, 1, 1, False, "deriche", [
        "L0 deriche copy/none/none/none c4:part do_x do_y decimate gen w4",
    ]),
    (300, 128, 1, 1, True, "deriche", [
        "L0 deriche copy/none/none/none c4:part do_x do_y decimate gen w4 a_dense",
    ]),
    (511, 128, 1, 1, False, "deriche", [
        "L0 deriche copy/none/none/none c4:part do_x do_y dec_odd decimate gen",
    ]),
    (511, 128, 1, 1, True, "deriche", [
        "L0 deriche copy/none/none/none c4:part do_x do_y dec_odd decimate gen a_dense",
    ]),
    (511, 258, 16, 16, False, "deriche", [
        "Ln deriche copy/none/none/none c4:none do_x do_y dec_odd decimate",
    ]),
    (512, 256, 1, 1, True, "deriche", [
        "Ln deriche copy/none/none/none c4:full do_x do_y decimate gen px",
    ]),
    (514, 256, 1, 1, True, "deriche", [
        "Ln deriche copy/none/none/none c4:part do_x do_y dec_odd decimate gen px",
    ]),
    (514, 1100, 3, 3, False, "deriche", [
        "Ln deriche copy/none/none/none c4:part do_x do_y dec_odd decimate gen",
    ]),
    (517, 256, 1, 1, True, "deriche", [
        "Ln deriche copy/none/none/none c4:part do_x do_y decimate gen px",
    ]),
    (517, 1100, 3, 3, False, "deriche", [
        "Ln deriche copy/none/none/none c4:part do_x do_y decimate gen",
    ]),
    (1024, 2050, 1, 1, True, "deriche", [
        "Ln deriche copy/none/none/none c4:full do_x do_y decimate gen",
    ]),
    (5, 3, 1, 1, False, "skip", [
        "L0 lone copy/none/none/none c4:none dec_odd decimate",
        "call one_pair",
    ]),
    (5, 3, 1, 1, True, "skip", [
        "L0 lone copy/none/none/none c4:none dec_odd decimate a_dense",
        "call a_dense one_pair",
    ]),
    (5, 3, 2, 2, False, "skip", [
        "call",
    ]),
    (64, 33, 1, 1, False, "skip", [
        "L0 lone copy/none/none/none c4:none decimate w4",
    ]),
    (64, 33, 1, 1, True, "skip", [
        "L0 lone copy/none/none/none c4:none decimate w4 a_dense",
        "Ln lone copy/none/none/none c4:none decimate px",
    ]),
    (67, 33, 1, 1, True, "skip", [
        "Ln lone copy/none/none/none c4:none dec_odd decimate px",
    ]),
    (130, 64, 1, 1, False, "skip", [
        "L0 lone copy/none/none/none c4:none decimate",
    ]),
    (130, 64, 1, 1, True, "skip", [
        "L0 lone copy/none/none/none c4:none decimate a_dense",
    ]),
    (256, 128, 1, 1, False, "skip", [
        "L0 lone copy/none/none/none c4:full decimate gen w4",
    ]),
    (256, 128, 1, 1, True, "skip", [
        "L0 lone copy/none/none/none c4:full decimate gen w4 a_dense",
    ]),
    (256, 514, 16, 16, False, "skip", [
        "Ln lone copy/none/none/none c4:none decimate",
    ]),
    (258, 128, 1, 1, False, "skip", [
        "L0 lone copy/none/none/none c4:part decimate gen",
    ]),
    (258, 128, 1, 1, True, "skip", [
        "L0 lone copy/none/none/none c4:part decimate gen a_dense",
    ]),
    (300, 128, 1, 1, False, "skip", [
        "L0 lone copy/none/none/none c4:part decimate gen w4",
    ]),
    (300, 128, 1, 1, True, "skip", [
        "L0 lone copy/none/none/none c4:part decimate gen w4 a_dense",
    ]),
    (511, 128, 1, 1, False, "skip", [
        "L0 lone copy/none/none/none c4:part dec_odd decimate gen",
    ]),
    (511, 128, 1, 1, True, "skip", [
        "L0 lone copy/none/none/none c4:part dec_odd decimate gen a_dense",
    ]),
    (511, 258, 16, 16, False, "skip", [
        "Ln lone copy/none/none/none c4:none dec_odd decimate",
    ]),
    (512, 256, 1, 1, True, "skip", [
        "Ln lone copy/none/none/none c4:full decimate gen px",
    ]),
    (514, 256, 1, 1, True, "skip", [
        "Ln lone copy/none/none/none c4:part dec_odd decimate gen px",
    ]),
    (514, 1100, 3, 3, False, "skip", [
        "Ln lone copy/none/none/none c4:part dec_odd decimate gen",
    ]),
    (517, 256, 1, 1, True, "skip", [
        "Ln lone copy/none/none/none c4:part decimate gen px",
    ]),
    (517, 1100, 3, 3, False, "skip", [
        "Ln lone copy/none/none/none c4:part decimate gen",
    ]),
    (1024, 2050, 1, 1, True, "skip", [
        "Ln lone copy/none/none/none c4:full decimate gen",
    ]),
    (3, 3, 1, 1, False, "vv0", [
        "call one_pair top_only",
    ]),
    (3, 3, 1, 1, True, "vv0", [
        "call a_dense one_pair top_only",
    ]),
    (3, 3, 2, 2, False, "vv0", [
        "call top_only",
    ]),
    (5, 3, 1, 1, False, "vv0", [
        "L0 lone x_m/x_m/y_m/dec7 c4:none do_x do_y mask_l0 per_plane dec_odd",
        "call mask_opt one_pair",
    ]),
    (5, 3, 1, 1, True, "vv0", [
        "L0 lone x_m/x_m/y_m/dec7 c4:none do_x do_y mask_l0 per_plane dec_odd a_dense",
        "call a_dense mask_opt one_pair",
    ]),
    (5, 3, 2, 2, False, "vv0", [
        "call mask_opt",
    ]),
    (33, 33, 1, 1, False, "vv0", [
        "call mask_opt coarse coarse_lds one_pair",
    ]),
    (33, 33, 1, 1, True, "vv0", [
        "call a_dense mask_opt coarse coarse_lds one_pair",
    ]),
    (33, 33, 2, 2, False, "vv0", [
        "call mask_opt coarse coarse_lds",
    ]),
    (255, 255, 16, 16, False, "vv0", [
        "L0 lone x_fwd/x_bwd/y_fwd1s/dec7 c4:none do_x do_y mask_l0 per_plane dec_odd",
    ]),
    (256, 255, 16, 16, False, "vv0", [
        "L0 lone x_fwd/x_bwd/y_fwd1s/dec7 c4:full do_x do_y mask_l0 per_plane gen w4",
    ]),
    (300, 255, 16, 16, False, "vv0", [
        "L0 lone x_fwd/x_bwd/y_fwd1s/dec7 c4:part do_x do_y mask_l0 per_plane gen w4",
    ]),
    (511, 258, 16, 16, False, "vv0", [
        "Ln lone x_m/x_m/y_fwd1s/dec7 c4:none do_x do_y dec_odd",
    ]),
    (511, 1000, 16, 16, False, "vv0", [
        "L0 lone x_fwd/x_bwd/y_fwd1s/dec7 c4:part do_x do_y src0 mask_l0 per_plane dec_odd gen",
        "Ln lone x_fwd/x_bwd/y_fwd1s/dec7 c4:none do_x do_y dec_odd",
    ]),
    (512, 258, 16, 16, False, "vv0", [
        "Ln lone x_m/x_m/y_fwd1s/dec7 c4:full do_x do_y gen",
    ]),
    (512, 1000, 16, 16, False, "vv0", [
        "L0 lone x_fwd/x_bwd/y_fwd1s/dec7 c4:full do_x do_y src0 mask_l0 per_plane gen w4",
        "Ln lone x_fwd/x_bwd/y_fwd1s/dec7 c4:full do_x do_y gen",
    ]),
    (514, 1000, 16, 16, False, "vv0", [
        "L0 lone x_fwd/x_bwd/y_fwd1s/dec7 c4:part do_x do_y src0 mask_l0 per_plane gen",
        "Ln lone x_fwd/x_bwd/y_fwd1s/dec7 c4:part do_x do_y dec_odd gen",
    ]),
    (517, 1100, 3, 3, False, "vv0", [
        "L0 lone x_fwd/x_bwd/y_m/dec7 c4:part do_x do_y mask_l0 per_plane dec_odd gen",
        "Ln lone x_m/x_m/y_m/dec7 c4:part do_x do_y gen",
    ]),
    (836, 620, 16, 16, False, "vv0", [
        "L0 lone x_fwd/x_bwd/y_fwd1s/dec7 c4:part do_x do_y src0 mask_l0 per_plane gen w4",
    ]),
    (1000, 517, 16, 16, False, "vv0", [
        "L0 lone x_m/x_bwd/y_fwd1s/dec7 c4:part do_x do_y src0 mask_l0 per_plane gen w4",
        "Ln lone x_fwd/x_bwd/y_fwd1s/dec7 c4:part do_x do_y gen",
        "Ln lone x_m/x_m/y_fwd1s/dec7 c4:none do_x do_y",
        "call src mask_opt coarse coarse_lds",
    ]),
    (1024, 1024, 2, 1, False, "vv0", [
        "call mask_opt wf_ctrl coarse coarse_lds one_pair",
    ]),
    (1024, 1024, 2, 1, True, "vv0", [
        "call a_dense mask_opt wf_ctrl coarse coarse_lds one_pair",
    ]),
    (1024, 1024, 2, 2, False, "vv0", [
        "L0 batch x_fwd/none/none/dec c4:full do_x do_y mask_l0 zt per_plane fill_mask dec_zt gen w4",
    ]),
    (1024, 1026, 2, 2, False, "vv0", [
        "L0 batch x_fwd/none/none/dec c4:full do_x do_y mask_l0 zt rowz per_plane fill_mask dec_zt gen w4",
        "Ln lone x_m/x_m/y_m/dec7 c4:full do_x do_y gen",
    ]),
    (1024, 2046, 4, 4, False, "vv0", [
        "L0 batch x_fwd/none/none/dec c4:full do_x do_y src0 mask_l0 zt rowz per_plane g_out mr_out fill_mask dec_zt gen w4",
        "Ln lone x_fwd/x_bwd/y_m/dec7 c4:full do_x do_y per_plane g_in mr_in gen c_mr",
        "call src mask_opt wf_ctrl coarse coarse_lds zi",
    ]),
    (1024, 2047, 4, 4, False, "vv0", [
        "L0 batch x_fwd/none/none/dec c4:full do_x do_y src0 mask_l0 zt rowz per_plane g_out fill_mask dec_zt gen w4",
        "Ln lone x_fwd/x_bwd/y_m/dec7 c4:full do_x do_y per_plane g_in gen",
    ]),
    (1024, 2050, 3, 3, False, "vv0", [
        "L0 batch x_fwd/none/none/dec c4:full do_x do_y mask_l0 zt rowz per_plane g_out mr_out fill_mask dec_zt gen w4",
    ]),
    (1025, 1024, 2, 2, False, "vv0", [
        "L0 batch x_fwd/none/none/dec c4:part do_x do_y mask_l0 zt per_plane fill_mask dec_zt dec_odd gen",
    ]),
    (1025, 1025, 2, 2, False, "vv0", [
        "L0 batch x_fwd/none/none/dec c4:part do_x do_y mask_l0 zt rowz per_plane fill_mask dec_zt dec_odd gen",
    ]),
    (1026, 1024, 2, 2, False, "vv0", [
        "L0 batch x_fwd/none/none/dec c4:part do_x do_y mask_l0 zt per_plane fill_mask dec_zt gen",
        "Ln lone x_m/x_m/y_m/dec7 c4:part do_x do_y dec_odd gen",
        "call mask_opt wf_ctrl coarse coarse_lds",
    ]),
    (1026, 1025, 2, 2, False, "vv0", [
        "L0 batch x_fwd/none/none/dec c4:part do_x do_y mask_l0 zt rowz per_plane fill_mask dec_zt gen",
    ]),
    (1026, 2047, 4, 4, False, "vv0", [
        "L0 batch x_fwd/none/none/dec c4:part do_x do_y src0 mask_l0 zt rowz per_plane g_out fill_mask dec_zt gen",
        "Ln lone x_fwd/x_bwd/y_m/dec7 c4:part do_x do_y per_plane g_in dec_odd gen",
    ]),
    (1026, 2050, 3, 3, False, "vv0", [
        "L0 batch x_fwd/none/none/dec c4:part do_x do_y mask_l0 zt rowz per_plane g_out mr_out fill_mask dec_zt gen",
        "Ln lone x_fwd/x_bwd/y_m/dec7 c4:part do_x do_y per_plane g_in mr_in dec_odd gen c_mr",
    ]),
    (1100, 1024, 2, 2, False, "vv0", [
        "L0 batch x_fwd/none/none/dec c4:part do_x do_y mask_l0 zt per_plane fill_mask dec_zt gen w4",
    ]),
    (1100, 1025, 2, 2, False, "vv0", [
        "L0 batch x_fwd/none/none/dec c4:part do_x do_y mask_l0 zt rowz per_plane fill_mask dec_zt gen w4",
    ]),
    (1100, 2050, 3, 3, False, "vv0", [
        "L0 batch x_fwd/none/none/dec c4:part do_x do_y mask_l0 zt rowz per_plane g_out mr_out fill_mask dec_zt gen w4",
        "Ln lone x_fwd/x_bwd/y_m/dec7 c4:part do_x do_y per_plane g_in mr_in gen c_mr",
    ]),
    (2046, 1000, 4, 4, False, "vv0", [
        "L0 lone x_m/x_bwd/y_fwd1s/dec7 c4:part do_x do_y src0 mask_l0 per_plane gen",
    ]),
    (2046, 1335, 3, 3, False, "vv0", [
        "L0 batch x_fwd/none/none/dec c4:part do_x do_y src0 mask_l0 zt rowz per_plane fill_mask dec_zt gen",
    ]),
    (2046, 2048, 2, 2, False, "vv0", [
        "L0 batch x_fwd/none/none/dec c4:part do_x do_y src0 mask_l0 zt per_plane fill_mask dec_zt gen",
    ]),
    (2047, 1000, 4, 4, False, "vv0", [
        "L0 lone x_m/x_bwd/y_fwd1s/dec7 c4:part do_x do_y src0 mask_l0 per_plane dec_odd gen",
    ]),
    (2048, 1024, 4, 4, False, "vv0", [
        "L0 batch x_fwd/none/none/dec c4:full do_x do_y src0 mask_l0 zt per_plane fill_mask dec_zt gen w4",
    ]),
    (2048, 1335, 3, 3, False, "vv0", [
        "L0 batch x_fwd/none/none/dec c4:full do_x do_y src0 mask_l0 zt rowz per_plane fill_mask dec_zt gen w4",
    ]),
    (2048, 2048, 2, 2, False, "vv0", [
        "L0 batch x_fwd/none/none/dec c4:full do_x do_y src0 mask_l0 zt per_plane g_out mr_out fill_mask dec_zt gen w4",
        "Ln batch x_fwd/none/none/dec c4:full do_x do_y zt per_plane g_in mr_in fill_mask dec_zt gen c_mr",
    ]),
    (2048, 2049, 2, 2, False, "vv0", [
        "Ln batch x_fwd/none/none/dec c4:full do_x do_y zt per_plane g_in dec_zt gen",
    ]),
    (2048, 2050, 2, 2, False, "vv0", [
        "Ln batch x_fwd/none/none/dec c4:full do_x do_y zt rowz per_plane g_in mr_in fill_mask dec_zt gen c_mr",
    ]),
    (2049, 2048, 2, 2, False, "vv0", [
        "L0 batch x_fwd/none/none/dec c4:part do_x do_y src0 mask_l0 zt per_plane fill_mask dec_zt dec_odd gen",
        "Ln batch x_fwd/none/none/dec c4:full do_x do_y zt per_plane dec_zt gen",
    ]),
    (2049, 2050, 2, 2, False, "vv0", [
        "L0 batch x_fwd/none/none/dec c4:part do_x do_y src0 mask_l0 zt rowz per_plane fill_mask dec_zt dec_odd gen",
        "Ln batch x_fwd/none/none/dec c4:full do_x do_y zt rowz per_plane dec_zt gen",
    ]),
    (2050, 2048, 2, 2, False, "vv0", [
        "L0 batch x_fwd/none/none/dec c4:part do_x do_y src0 mask_l0 zt per_plane g_out mr_out fill_mask dec_zt gen",
        "Ln batch x_fwd/none/none/dec c4:part do_x do_y zt per_plane g_in mr_in fill_mask dec_zt dec_odd gen c_mr",
    ]),
    (2050, 2049, 2, 2, False, "vv0", [
        "Ln batch x_fwd/none/none/dec c4:part do_x do_y zt per_plane g_in dec_zt dec_odd gen",
    ]),
    (2050, 2050, 2, 2, False, "vv0", [
        "L0 batch x_fwd/none/none/dec c4:part do_x do_y src0 mask_l0 zt rowz per_plane g_out mr_out fill_mask dec_zt gen",
        "Ln batch x_fwd/none/none/dec c4:part do_x do_y zt rowz per_plane g_in mr_in fill_mask dec_zt dec_odd gen c_mr",
    ]),
    (2052, 1024, 4, 4, False, "vv0", [
        "L0 batch x_fwd/none/none/dec c4:part do_x do_y src0 mask_l0 zt per_plane fill_mask dec_zt gen w4",
    ]),
    (2052, 1335, 3, 3, False, "vv0", [
        "L0 batch x_fwd/none/none/dec c4:part do_x do_y src0 mask_l0 zt rowz per_plane fill_mask dec_zt gen w4",
    ]),
    (2052, 2048, 2, 2, False, "vv0", [
        "L0 batch x_fwd/none/none/dec c4:part do_x do_y src0 mask_l0 zt per_plane g_out mr_out fill_mask dec_zt gen w4",
        "Ln batch x_fwd/none/none/dec c4:part do_x do_y zt per_plane g_in mr_in fill_mask dec_zt gen c_mr",
    ]),
    (2052, 2049, 2, 2, False, "vv0", [
        "L0 batch x_fwd/none/none/dec c4:part do_x do_y src0 mask_l0 zt rowz per_plane g_out fill_mask dec_zt gen w4",
        "Ln batch x_fwd/none/none/dec c4:part do_x do_y zt per_plane g_in dec_zt gen",
    ]),
    (2052, 2050, 2, 2, False, "vv0", [
        "L0 batch x_fwd/none/none/dec c4:part do_x do_y src0 mask_l0 zt rowz per_plane g_out mr_out fill_mask dec_zt gen w4",
        "Ln batch x_fwd/none/none/dec c4:part do_x do_y zt rowz per_plane g_in mr_in fill_mask dec_zt gen c_mr",
    ]),
    (5, 1025, 3, 3, False, "vv1", [
        "L0 lone x_fwd/x_bwd/y_m/dec7 c4:none do_x do_y mask_l0 per_plane dec_odd",
    ]),
    (33, 1026, 16, 16, False, "vv1", [
        "Ln lone x_fwd/x_bwd/y_m/dec7 c4:none do_x do_y",
    ]),
    (33, 2100, 3, 3, False, "vv1", [
        "Ln lone x_fwd/x_bwd/y_m/dec7 c4:none do_x do_y px",
    ]),
    (64, 5, 1, 1, False, "vv1", [
        "L0 lone x_m/x_m/y_m/dec7 c4:none do_x do_y mask_l0 per_plane w4",
    ]),
    (64, 5, 1, 1, True, "vv1", [
        "L0 lone x_m/x_m/y_m/dec7 c4:none do_x do_y mask_l0 per_plane w4 a_dense",
    ]),
    (64, 1025, 3, 3, False, "vv1", [
        "L0 lone x_fwd/x_bwd/y_m/dec7 c4:none do_x do_y mask_l0 per_plane w4",
    ]),
    (67, 2100, 3, 3, False, "vv1", [
        "Ln lone x_fwd/x_bwd/y_m/dec7 c4:none do_x do_y dec_odd px",
    ]),
    (128, 33, 1, 1, True, "vv1", [
        "Ln lone x_m/x_m/y_m/dec7 c4:none do_x do_y px",
    ]),
    (130, 5, 1, 1, False, "vv1", [
        "L0 lone x_m/x_m/y_m/dec7 c4:none do_x do_y mask_l0 per_plane",
    ]),
    (130, 5, 1, 1, True, "vv1", [
        "L0 lone x_m/x_m/y_m/dec7 c4:none do_x do_y mask_l0 per_plane a_dense",
    ]),
    (130, 33, 1, 1, True, "vv1", [
        "Ln lone x_m/x_m/y_m/dec7 c4:none do_x do_y dec_odd px",
    ]),
    (130, 1025, 3, 3, False, "vv1", [
        "L0 lone x_fwd/x_bwd/y_m/dec7 c4:none do_x do_y mask_l0 per_plane",
    ]),
    (130, 2050, 4, 4, False, "vv1", [
        "Ln lone x_fwd/x_bwd/y_m/dec7 c4:none do_x do_y dec_odd",
    ]),
    (255, 5, 16, 16, False, "vv1", [
        "L0 lone x_m/x_m/y_fwd1s/dec7 c4:none do_x do_y mask_l0 per_plane dec_odd",
    ]),
    (255, 2046, 16, 16, False, "vv1", [
        "L0 lone x_fwd/x_bwd/y_fwd1s/dec7 c4:none do_x do_y src0 mask_l0 per_plane dec_odd",
    ]),
    (256, 5, 1, 1, False, "vv1", [
        "L0 lone x_m/x_m/y_m/dec7 c4:full do_x do_y mask_l0 per_plane gen w4",
    ]),
    (256, 5, 1, 1, True, "vv1", [
        "L0 lone x_m/x_m/y_m/dec7 c4:full do_x do_y mask_l0 per_plane gen w4 a_dense",
    ]),
    (256, 1025, 3, 3, False, "vv1", [
        "L0 lone x_fwd/x_bwd/y_m/dec7 c4:full do_x do_y mask_l0 per_plane gen w4",
    ]),
    (258, 5, 1, 1, False, "vv1", [
        "L0 lone x_m/x_m/y_m/dec7 c4:part do_x do_y mask_l0 per_plane gen",
    ]),
    (258, 5, 1, 1, True, "vv1", [
        "L0 lone x_m/x_m/y_m/dec7 c4:part do_x do_y mask_l0 per_plane gen a_dense",
    ]),
    (258, 2046, 3, 3, False, "vv1", [
        "L0 lone x_fwd/x_bwd/y_m/dec7 c4:part do_x do_y mask_l0 per_plane gen",
        "Ln lone x_m/x_m/y_m/dec7 c4:none do_x do_y dec_odd",
    ]),
    (300, 5, 1, 1, False, "vv1", [
        "L0 lone x_m/x_m/y_m/dec7 c4:part do_x do_y mask_l0 per_plane gen w4",
    ]),
    (300, 5, 1, 1, True, "vv1", [
        "L0 lone x_m/x_m/y_m/dec7 c4:part do_x do_y mask_l0 per_plane gen w4 a_dense",
    ]),
    (300, 2046, 3, 3, False, "vv1", [
        "L0 lone x_fwd/x_bwd/y_m/dec7 c4:part do_x do_y mask_l0 per_plane gen w4",
        "Ln lone x_m/x_m/y_m/dec7 c4:none do_x do_y",
    ]),
    (511, 5, 1, 1, False, "vv1", [
        "L0 lone x_m/x_m/y_m/dec7 c4:part do_x do_y mask_l0 per_plane dec_odd gen",
    ]),
    (511, 5, 1, 1, True, "vv1", [
        "L0 lone x_m/x_m/y_m/dec7 c4:part do_x do_y mask_l0 per_plane dec_odd gen a_dense",
    ]),
    (511, 33, 16, 16, False, "vv1", [
        "Ln lone x_m/x_m/y_fwd1s/dec7 c4:none do_x do_y dec_odd px",
    ]),
    (512, 33, 1, 1, True, "vv1", [
        "Ln lone x_m/x_m/y_m/dec7 c4:full do_x do_y gen px",
    ]),
    (512, 2100, 3, 3, False, "vv1", [
        "Ln lone x_fwd/x_bwd/y_m/dec7 c4:full do_x do_y gen",
    ]),
    (514, 33, 1, 1, True, "vv1", [
        "Ln lone x_m/x_m/y_m/dec7 c4:part do_x do_y dec_odd gen px",
    ]),
    (514, 255, 16, 16, False, "vv1", [
        "L0 lone x_fwd/x_bwd/y_fwd1s/dec7 c4:part do_x do_y mask_l0 per_plane gen",
        "Ln lone x_m/x_m/y_fwd1s/dec7 c4:part do_x do_y dec_odd gen",
    ]),
    (514, 2100, 3, 3, False, "vv1", [
        "Ln lone x_fwd/x_bwd/y_m/dec7 c4:part do_x do_y dec_odd gen",
    ]),
    (517, 33, 1, 1, True, "vv1", [
        "Ln lone x_m/x_m/y_m/dec7 c4:part do_x do_y gen px",
    ]),
    (517, 255, 16, 16, False, "vv1", [
        "L0 lone x_fwd/x_bwd/y_fwd1s/dec7 c4:part do_x do_y mask_l0 per_plane dec_odd gen",
        "Ln lone x_m/x_m/y_fwd1s/dec7 c4:part do_x do_y gen",
    ]),
    (517, 2100, 3, 3, False, "vv1", [
        "Ln lone x_fwd/x_bwd/y_m/dec7 c4:part do_x do_y gen",
    ]),
    (1000, 33, 16, 16, False, "vv1", [
        "Ln lone x_m/x_m/y_fwd1s/dec7 c4:none do_x do_y px",
    ]),
    (1025, 5, 3, 3, False, "vv1", [
        "L0 lone x_m/x_m/y_fwd1s/dec7 c4:part do_x do_y mask_l0 per_plane dec_odd gen",
    ]),
    (1026, 5, 3, 3, False, "vv1", [
        "L0 lone x_m/x_m/y_fwd1s/dec7 c4:part do_x do_y mask_l0 per_plane gen",
    ]),
    (1100, 5, 3, 3, False, "vv1", [
        "L0 lone x_m/x_m/y_fwd1s/dec7 c4:part do_x do_y mask_l0 per_plane gen w4",
    ]),
    (2046, 5, 16, 16, False, "vv1", [
        "L0 lone x_m/x_m/y_fwd/dec c4:part do_x do_y mask_l0 per_plane gen",
    ]),
    (2046, 255, 16, 16, False, "vv1", [
        "L0 lone x_m/x_bwd/y_fwd/dec c4:part do_x do_y src0 mask_l0 per_plane gen",
        "call src mask_opt",
    ]),
    (2047, 5, 16, 16, False, "vv1", [
        "L0 lone x_m/x_m/y_fwd/dec c4:part do_x do_y mask_l0 per_plane dec_odd gen",
    ]),
    (2047, 255, 16, 16, False, "vv1", [
        "L0 lone x_m/x_bwd/y_fwd/dec c4:part do_x do_y src0 mask_l0 per_plane dec_odd gen",
    ]),
    (2048, 5, 2, 2, False, "vv1", [
        "L0 lone x_m/x_m/y_fwd1s/dec7 c4:full do_x do_y mask_l0 per_plane gen w4",
    ]),
    (2048, 5, 16, 16, False, "vv1", [
        "L0 lone x_m/x_m/y_fwd/dec c4:full do_x do_y mask_l0 per_plane gen w4",
    ]),
    (2048, 33, 4, 4, False, "vv1", [
        "Ln lone x_m/x_m/y_fwd1s/dec7 c4:full do_x do_y gen px",
    ]),
    (2048, 255, 16, 16, False, "vv1", [
        "L0 lone x_m/x_bwd/y_fwd/dec c4:full do_x do_y src0 mask_l0 per_plane gen w4",
    ]),
    (2048, 1000, 4, 4, False, "vv1", [
        "L0 lone x_m/x_bwd/y_fwd1s/dec7 c4:full do_x do_y src0 mask_l0 per_plane gen w4",
    ]),
    (2050, 33, 3, 3, False, "vv1", [
        "Ln lone x_m/x_m/y_fwd1s/dec7 c4:part do_x do_y dec_odd gen px",
    ]),
    (2052, 5, 16, 16, False, "vv1", [
        "L0 lone x_m/x_m/y_fwd/dec c4:part do_x do_y mask_l0 per_plane gen w4",
    ]),
    (2052, 33, 3, 3, False, "vv1", [
        "Ln lone x_m/x_m/y_fwd1s/dec7 c4:part do_x do_y gen px",
    ]),
    (2052, 255, 16, 16, False, "vv1", [
        "L0 lone x_m/x_bwd/y_fwd/dec c4:part do_x do_y src0 mask_l0 per_plane gen w4",
    ]),
]

# The same for the calls of the grid with more than MAX_PIXELS: the signatures they reach and the smaller calls do not (a source-fused
# level 0 of 16 pairs on the separate one-wavefront sweeps; an unfused level 1 that reads flags behind a fused level 0 of four pairs;
# 16 pairs of 2048 x 2048 and more: a fused level 1 that reads and writes flags in front of an unfused level 2 that reads them)
WIDE_CASES = [
    (514, 2046, 16, 16, False, "vv0", [
        "L0 lone x_fwd/x_bwd/y_fwd1/dec7 c4:part do_x do_y src0 mask_l0 per_plane gen",
    ]),
    (517, 2046, 16, 16, False, "vv0", [
        "L0 lone x_fwd/x_bwd/y_fwd1/dec7 c4:part do_x do_y src0 mask_l0 per_plane dec_odd gen",
    ]),
    (768, 2046, 16, 16, False, "vv0", [
        "L0 lone x_fwd/x_bwd/y_fwd1/dec7 c4:full do_x do_y src0 mask_l0 per_plane gen w4",
    ]),
    (1000, 1335, 16, 16, False, "vv0", [
        "L0 lone x_fwd/x_bwd/y_fwd1/dec7 c4:part do_x do_y src0 mask_l0 per_plane gen w4",
        "Ln lone x_fwd/x_bwd/y_fwd1s/dec7 c4:none do_x do_y",
    ]),
    (1100, 2047, 4, 4, False, "vv0", [
        "Ln lone x_fwd/x_bwd/y_m/dec7 c4:part do_x do_y per_plane g_in gen",
    ]),
    (2046, 620, 16, 16, False, "vv0", [
        "L0 lone x_fwd/x_bwd/y_fwd/dec c4:part do_x do_y src0 mask_l0 per_plane gen",
    ]),
    (2046, 2046, 4, 4, False, "vv0", [
        "Ln lone x_fwd/x_bwd/y_fwd1s/dec7 c4:part do_x do_y per_plane g_in mr_in dec_odd gen c_mr",
    ]),
    (2046, 2047, 4, 4, False, "vv0", [
        "Ln lone x_fwd/x_bwd/y_fwd1s/dec7 c4:part do_x do_y per_plane g_in dec_odd gen",
    ]),
    (2047, 620, 16, 16, False, "vv0", [
        "L0 lone x_fwd/x_bwd/y_fwd/dec c4:part do_x do_y src0 mask_l0 per_plane dec_odd gen",
    ]),
    (2048, 2046, 4, 4, False, "vv0", [
        "Ln lone x_fwd/x_bwd/y_fwd1s/dec7 c4:full do_x do_y per_plane g_in mr_in gen c_mr",
    ]),
    (2048, 2047, 4, 4, False, "vv0", [
        "Ln lone x_fwd/x_bwd/y_fwd1s/dec7 c4:full do_x do_y per_plane g_in gen",
    ]),
    (2052, 2046, 4, 4, False, "vv0", [
        "Ln lone x_fwd/x_bwd/y_fwd1s/dec7 c4:part do_x do_y per_plane g_in mr_in gen c_mr",
    ]),
    (2052, 2047, 4, 4, False, "vv0", [
        "Ln lone x_fwd/x_bwd/y_fwd1s/dec7 c4:part do_x do_y per_plane g_in gen",
    ]),
    (2048, 620, 16, 16, False, "vv1", [
        "L0 lone x_fwd/x_bwd/y_fwd/dec c4:full do_x do_y src0 mask_l0 per_plane gen w4",
    ]),
    (2052, 620, 16, 16, False, "vv1", [
        "L0 lone x_fwd/x_bwd/y_fwd/dec c4:part do_x do_y src0 mask_l0 per_plane gen w4",
    ]),
    (2048, 2048, 16, 16, False, "vv0", [
        "Ln batch x_fwd/none/none/dec c4:full do_x do_y zt per_plane g_in g_out mr_in mr_out fill_mask dec_zt gen c_mr",
    ]),
    (2048, 2049, 16, 16, False, "vv0", [
        "Ln batch x_fwd/none/none/dec c4:full do_x do_y zt per_plane g_in g_out dec_zt gen",
    ]),
    (2048, 2050, 16, 16, False, "vv0", [
        "Ln batch x_fwd/none/none/dec c4:full do_x do_y zt rowz per_plane g_in g_out mr_in fill_mask dec_zt gen c_mr",
    ]),
    (2048, 2052, 16, 16, False, "vv0", [
        "Ln batch x_fwd/none/none/dec c4:full do_x do_y zt rowz per_plane g_in g_out mr_in mr_out fill_mask dec_zt gen c_mr",
    ]),
    (2049, 2048, 16, 16, False, "vv0", [
        "Ln batch x_fwd/none/none/dec c4:full do_x do_y zt per_plane g_out dec_zt gen",
    ]),
    (2049, 2050, 16, 16, False, "vv0", [
        "Ln batch x_fwd/none/none/dec c4:full do_x do_y zt rowz per_plane g_out dec_zt gen",
    ]),
    (2052, 2048, 16, 16, False, "vv0", [
        "Ln batch x_fwd/none/none/dec c4:part do_x do_y zt per_plane g_in g_out mr_in mr_out fill_mask dec_zt gen c_mr",
    ]),
    (2052, 2049, 16, 16, False, "vv0", [
        "Ln batch x_fwd/none/none/dec c4:part do_x do_y zt per_plane g_in g_out dec_zt gen",
    ]),
    (2052, 2050, 16, 16, False, "vv0", [
        "Ln batch x_fwd/none/none/dec c4:part do_x do_y zt rowz per_plane g_in g_out mr_in fill_mask dec_zt gen c_mr",
    ]),
    (2052, 2052, 16, 16, False, "vv0", [
        "Ln batch x_fwd/none/none/dec c4:part do_x do_y zt rowz per_plane g_in g_out mr_in mr_out fill_mask dec_zt gen c_mr",
    ]),
]
