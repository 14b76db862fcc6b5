"""The runtime switches of the library (environment variables read by computervisionimagestich2_amd/csrc/, documented in
include/stitch.h) and how the test suite runs each of them.  Plain data: no GPU, no torch import.

include/stitch.h promises that no switch changes a result bit.  Every switch here is a different kernel or launch path, so
tests/test_gpu_switches.py runs each value below against the oracle, bit for bit (output bytes, seam, status code), and
tests/test_switch_inventory.py fails the CPU suite when a `getenv("STITCH_...")` appears in csrc/ that is neither here nor in
EXEMPT.

Compile-time macros (`#ifndef STITCH_...`: STITCH_C4_PREFETCH, STITCH_C4_WAVES, STITCH_XY_BUFS, STITCH_PJ_*, ...) are not
runtime switches and are out of scope here: a build picks one value of each.

Each entry of SWITCHES:
  values  the values to test (strings, as they are put into the environment);
  forms   the call forms where the switch matters:
            "lone"   one pair per call (capi.Plan(max_pairs=1).pair)
            "batch"  several pairs in one launch sequence (capi.Plan(max_pairs=n).pairs)
            "blend"  two dense canvases (capi.Plan.blend, stitch_dev_blend_*)
            "host"   host-buffer entry points (capi.pair), the switch flipped between two calls
            "band"   one pair split into two row bands (pipeline.BandStitcher, ranks as threads)
            "lum"    equalise / luminance mix / finish
            "child"  read once per process: each value runs in a fresh child process
  shapes  canvas shapes (keys of SHAPES) where the switch matters;
  env     extra settings each value runs with as well ({} = the value alone), e.g. strip heights that divide no level height;
  probe   optional name of a check that the switch took effect (test_gpu_switches.PROBES).
"""

# (cw, ch): canvases whose edges the paths differ on
SHAPES = {
    "w1100": (1100, 620),    # width not a multiple of 64, even: level 1 550, level 2 275 (odd: the odd decimation)
    "odd": (1101, 617),      # odd width and height at level 0 already
    # levels 1, 2, 3 (1050, 525, 262 columns; 557, 278, 139 rows) all reach k_collapse4 with a partial last 256-column block,
    # heights that neither 5 nor 7 nor 32 divide
    "c4": (2100, 1114),
    "p4160": (4160, 2080),   # level 0 of >= 4096 columns: the padded row pitch (2048 rows and more: 12 levels)
    "p4097": (4097, 2051),   # the same, odd
}
STD = ("w1100", "odd")
PAIR_FORMS = ("lone", "batch", "blend")


def _sw(values, forms=PAIR_FORMS, shapes=STD, env=({},), probe=None):
    return dict(values=tuple(values), forms=tuple(forms), shapes=tuple(shapes), env=tuple(env), probe=probe)


SWITCHES = {
    # plan switches (Tuning::from_env, read when a plan is created and on every host-buffer call)
    "STITCH_WAVEFRONT": _sw(["0", "1", "2"]),
    "STITCH_NO_FUSE": _sw(["1"], forms=PAIR_FORMS + ("host",), probe="no_fuse"),
    "STITCH_NO_SRC_FUSE": _sw(["1"]),
    "STITCH_NO_ZERO_TILES": _sw(["1"], env=({"STITCH_WAVEFRONT": "2"},)),
    "STITCH_CROWS_L0": _sw(["1", "3", "7", "64"], forms=("lone", "host"), shapes=STD + ("c4",)),
    "STITCH_CROWS_LN": _sw(["1", "5", "32"], forms=("lone",), shapes=STD + ("c4",)),
    "STITCH_CROWS_WGS": _sw(["0", "1", "1000000"], forms=("lone",), shapes=STD + ("c4",)),
    "STITCH_COLLAPSE4": _sw(["0"]),
    "STITCH_XBYF_WGS": _sw(["16"], forms=("batch",), env=({"STITCH_WAVEFRONT": "2"},)),
    "STITCH_XBYF_EARLY": _sw(["0"], forms=("batch",), env=({"STITCH_WAVEFRONT": "2"}, {"STITCH_WAVEFRONT": "2", "STITCH_XBYF_WGS": "16"}),
                             probe="fused_sweep"),
    "STITCH_Y2": _sw(["1"]),
    "STITCH_RECOMPUTE": _sw(["1", "2"], forms=("batch", "blend"), env=({"STITCH_WAVEFRONT": "2"},)),
    "STITCH_GATE64": _sw(["1"]),
    "STITCH_COARSE": _sw(["0", "300"]),
    "STITCH_SINGLE_FAST": _sw(["1"], forms=("lone", "blend")),
    "STITCH_ODD_DEC": _sw(["0"]),
    "STITCH_C4_GEN": _sw(["0", "1"]),
    "STITCH_COLLAPSE_PX": _sw(["0"], forms=("lone", "blend")),
    "STITCH_Y1S": _sw(["0", "2"], forms=("lone", "blend")),
    "STITCH_C4_LOCKSTEP": _sw(["1", "2"], forms=("lone", "batch", "host"), shapes=STD + ("c4",),
                              env=({}, {"STITCH_CROWS_LN": "5"}, {"STITCH_CROWS_LN": "7", "STITCH_CROWS_L0": "3"})),
    "STITCH_C4_SWIZZLE": _sw(["0", "2"]),
    "STITCH_MOVER": _sw(["0"], forms=("lone", "blend")),
    "STITCH_SRC_LONE_MPIX": _sw(["0", "1"], forms=("lone", "blend")),
    "STITCH_DEC7": _sw(["0"], forms=("lone", "blend")),
    "STITCH_XBYM": _sw(["0", "1"], forms=("lone", "blend")),
    "STITCH_XBYM_MPIX": _sw(["0", "1000"], forms=("lone", "host"), env=({"STITCH_XBYM": None},)),
    "STITCH_COARSE_LDS": _sw(["0"]),
    "STITCH_PITCH_PAD": _sw(["1", "64", "100"], forms=PAIR_FORMS + ("host",), shapes=("p4160", "p4097"), probe="pitch_pad"),
    # band switches (stitch_band_create)
    "STITCH_BAND_PLAIN": _sw(["1"], forms=("band",), shapes=()),
    "STITCH_BAND_PLANES": _sw(["1"], forms=("band",), shapes=()),
    # per-call switches of other entry points
    "STITCH_BYTE_KERNELS": _sw(["1"], forms=("lum",), shapes=()),
    # read once per process
    "STITCH_NO_FASTDIV": _sw(["1"], forms=("child",), shapes=()),
    "STITCH_COPY_THREADS": _sw(["0", "1", "16"], forms=("child",), shapes=()),
}

# Names read in csrc/ (or by the package) that this suite does not run through the table, with the reason.
EXEMPT = {
    "STITCH_WAVEFRONT_STAMP": "diagnostics only: time stamps of the fused sweep's workgroups, printed at plan destruction",
    "STITCH_XBYM_STAMP": "diagnostics only: time stamps of k_vv_xby_m's wavefronts",
    "STITCH_COARSE_STAMP": "diagnostics only: time stamps of k_coarse",
    "STITCH_D7_STAMP": "diagnostics only: time stamps of k_vv_y_bwd_dec7 at one level",
    "STITCH_D7_STAMP_MODE": "diagnostics only: what STITCH_D7_STAMP records",
    "STITCH_XBYF_SPIN_LIMIT": "pinned by test_gpu_benchpath.py::test_timed_out_handoff_is_reported_for_every_queued_call (0 forces the bail-out)",
    "STITCH_PLAN_CACHE": "pinned by test_gpu_parity.py::test_host_entry_points_reuse_workspaces_and_trim; read once per process, no kernel path",
    "STITCH_PROJECT1": "pinned by test_gpu_parity.py::test_project_column_strip_kernel_equals_pixel_kernel",
    "STITCH_LIB": "not a switch: the path of the shared library (A/B builds of the same ABI)",
}


def cases():
    """(name, value, extra env) for every value of every switch, in table order."""
    for name, sw in SWITCHES.items():
        for v in sw["values"]:
            for extra in sw["env"]:
                yield name, v, extra


def case_id(name, value, extra):
    more = ",".join(f"{k[len('STITCH_'):]}={v}" for k, v in extra.items())
    return f"{name[len('STITCH_'):]}={value}" + (f"[{more}]" if more else "")
