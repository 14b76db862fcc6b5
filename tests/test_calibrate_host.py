"""CPU: the host side of the calibration from several captures (include/stitch_calibrate.h) -- the header compiles as C99, the
binding's sixth signature table states exactly what it declares and shares no name with the five others; argument errors come
back before a device is needed; the pooled threshold is the plain rule with one capture and an absolute value where one is given
(against stitch_stitch_order on hand-made count matrices)."""
import ctypes as C
import os
import re
import shlex
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "stitch_calibrate.h")

FUNCTIONS = ("stitch_calibrate_opts_default", "stitch_dev_calibrate_u8", "stitch_dev_calibrate_from_features_u8", "stitch_calibrate_u8",
             "stitch_calibration_info", "stitch_calibration_step_at", "stitch_calibration_counts", "stitch_calibration_step_support",
             "stitch_rig_from_calibration", "stitch_calibration_destroy")


def _header_text():
    return re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)


SCALARS = {"int": C.c_int, "int32_t": C.c_int, "float": C.c_float, "double": C.c_double, "size_t": C.c_size_t}
RETURNS = {"int": C.c_int, "void": None}


def _declared():
    """{name: (restype, argtypes)} of every prototype, by the binding's rules (tests/test_capi_abi.py, tests/test_rig_host.py)."""
    sigs = {}
    for ret, name, params in re.findall(r"((?:const\s+)?\w+\s*\*?)\s*\b(stitch_\w+)\s*\(([^()]*)\)\s*;", _header_text()):
        prms = [] if params.strip() == "void" else [" ".join(p.split()) for p in params.split(",")]
        args = [C.c_void_p if ("*" in p or "[" in p) else SCALARS[" ".join(p.split()[:-1])] for p in prms]
        sigs[name] = (RETURNS[" ".join(ret.replace("*", " *").split())], args)
    return sigs


def test_signature_table_states_the_header(st):
    capi = st.capi
    want, lib = _declared(), capi.lib()
    assert sorted(want) == sorted(FUNCTIONS) == sorted(set(re.findall(r"\b(stitch_[a-z0-9_]+)\s*\(", _header_text())))
    assert sorted(capi.CALIBRATE_SIGNATURES) == sorted(want)
    others = set(capi.SIGNATURES) | set(capi.PANORAMA_SIGNATURES) | set(capi.RIG_SIGNATURES) | set(capi.EXPOSURE_SIGNATURES) | set(capi.RIG_EXPOSURE_SIGNATURES)
    assert not set(capi.CALIBRATE_SIGNATURES) & others
    bound = {n: (getattr(lib, n).restype, getattr(lib, n).argtypes) for n in want}  # exported, and bound as declared
    wrong = {n: (bound[n], want[n]) for n in sorted(want) if bound[n] != tuple(want[n])}
    assert not wrong, f"(bound, declared) signatures differ for: {wrong}"
    assert lib.stitch_abi_version() == 5
    for name in ("dev_calibrate", "dev_calibrate_from_features", "calibrate", "Calibration"):
        assert hasattr(capi, name)
    from computervisionimagestich2_amd import pipeline
    assert hasattr(capi.Rig, "from_calibration") and hasattr(pipeline, "calibrate_from_sets")


def test_header_is_c99(st, tmp_path):
    cc = shlex.split(os.environ.get("CC", "cc")) + ["-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include")]
    src = tmp_path / "uses.c"
    src.write_text("\n".join(['#include "stitch_calibrate.h"', "void uses(void) {"] + [f"    (void)(&{n});" for n in FUNCTIONS]
                             + ["    (void)sizeof(stitch_calibrate_opts);", "    (void)STITCH_CALIBRATE_MAX_PAIRS;", "}", ""]))
    r = subprocess.run(cc + ["-fsyntax-only", str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_opts_mirror_and_default(st):
    capi = st.capi
    o = capi.CalibrateOpts(0x1234, 7)
    capi.lib().stitch_calibrate_opts_default(C.byref(o))
    assert o.pano is None and o.pooled_threshold == 0
    assert C.sizeof(capi.CalibrateOpts) == 16 and capi.CalibrateOpts.pooled_threshold.offset == 8


# ---- argument errors: before a device is needed ------------------------------------------------------------------------------
def _frames(capi, sizes):
    """A capture-major FrameU8 array with made-up (never followed) data pointers."""
    return (capi.FrameU8 * len(sizes))(*[capi.FrameU8(0x10000 * (i + 1), w, h) for i, (w, h) in enumerate(sizes)])


def _dev_call(capi, arr, n_sets, n, opts=None):
    h = C.c_void_p(0xdead)
    rc = capi.lib().stitch_dev_calibrate_u8(arr, n_sets, n, None if opts is None else C.byref(opts), None, C.byref(h))
    return rc, h.value, capi.lib().stitch_last_error().decode()


@pytest.mark.parametrize("entry", ["stitch_dev_calibrate_u8", "stitch_calibrate_u8"])
def test_argument_errors_come_before_the_device(st, entry):
    capi = st.capi

    def call(arr, n_sets, n, opts=None):
        h = C.c_void_p(0xdead)
        o = None if opts is None else C.byref(opts)
        args = (arr, n_sets, n, o, None, C.byref(h)) if entry == "stitch_dev_calibrate_u8" else (arr, n_sets, n, o, C.byref(h))
        return getattr(capi.lib(), entry)(*args), h.value, capi.lib().stitch_last_error().decode()

    one = [(64, 48)]
    # n and n_sets out of range, the product over 1024
    for n_sets, n, word in ((1, 0, "cameras"), (1, 65, "cameras"), (0, 1, "captures"), (65, 1, "captures"), (-1, 2, "captures"), (17, 64, "frames"),
                            (64, 17, "frames")):
        rc, h, text = call(_frames(capi, one * max(n_sets * n, 1)), n_sets, n)
        assert rc == capi.ERR_ARG and h is None and word in text, (n_sets, n, rc, text)
    # camera 1 is 64 x 48 in capture 0 and 48 x 64 in capture 2
    sizes = [(32, 32), (64, 48), (40, 40)] * 3
    sizes[2 * 3 + 1] = (48, 64)
    rc, h, text = call(_frames(capi, sizes), 3, 3)
    assert rc == capi.ERR_ARG and h is None and "capture 2 camera 1" in text and "48 x 64" in text and "64 x 48" in text, text
    # a frame without data, a bad size, null arguments, bad options
    arr = _frames(capi, [(32, 32)] * 4)
    arr[3].data = None
    rc, h, text = call(arr, 2, 2)
    assert rc == capi.ERR_ARG and h is None and "capture 1 camera 1" in text
    rc, h, text = call(_frames(capi, [(32, 32), (0, 32)]), 1, 2)
    assert rc == capi.ERR_ARG and h is None and "capture 0 camera 1" in text
    rc, h, text = call(None, 1, 1)
    assert rc == capi.ERR_ARG and h is None
    rc, h, text = call(_frames(capi, one), 1, 1, capi.CalibrateOpts(None, -1))
    assert rc == capi.ERR_ARG and h is None and "pooled_threshold" in text
    bad = capi.PanoramaOpts()
    capi.lib().stitch_panorama_opts_default(C.byref(bad))
    bad.kp_cap = -1
    rc, h, text = call(_frames(capi, one), 1, 1, capi.CalibrateOpts(C.addressof(bad), 0))
    assert rc == capi.ERR_ARG and h is None


def test_from_features_argument_errors(st):
    capi = st.capi
    L = capi.lib()
    wh = np.array([[64, 48], [64, 48]], np.int32)
    sets = (capi.FeatureSet * 4)(*[capi.FeatureSet(0x1000, 0x2000, 0x3000, 5) for _ in range(4)])
    for n_sets, n in ((0, 2), (2, 0), (65, 2), (2, 65), (33, 32)):
        h = C.c_void_p(0xdead)
        assert L.stitch_dev_calibrate_from_features_u8(wh.ctypes.data_as(C.c_void_p), sets, n_sets, n, None, None, C.byref(h)) == capi.ERR_ARG and h.value is None
    h = C.c_void_p(0xdead)
    assert L.stitch_dev_calibrate_from_features_u8(None, sets, 2, 2, None, None, C.byref(h)) == capi.ERR_ARG and h.value is None
    sets[3].d_x = None
    assert L.stitch_dev_calibrate_from_features_u8(wh.ctypes.data_as(C.c_void_p), sets, 2, 2, None, None, C.byref(h)) == capi.ERR_ARG
    assert b"capture 1 camera 1" in L.stitch_last_error()
    sets[3].d_x = 0x2000
    wh[1, 0] = 0
    assert L.stitch_dev_calibrate_from_features_u8(wh.ctypes.data_as(C.c_void_p), sets, 2, 2, None, None, C.byref(h)) == capi.ERR_ARG
    # the result calls refuse a null handle
    assert L.stitch_calibration_info(None, None, None, None, None, None, None) == capi.ERR_ARG
    assert L.stitch_calibration_step_at(None, 0, None) == capi.ERR_ARG and L.stitch_calibration_counts(None, None, None) == capi.ERR_ARG
    assert L.stitch_calibration_step_support(None, 0, None, None) == capi.ERR_ARG
    assert L.stitch_rig_from_calibration(None, None, None, C.byref(h)) == capi.ERR_ARG and h.value is None
    L.stitch_calibration_destroy(None)


def test_valid_arguments_reach_the_device_check(st):
    import torch
    if torch.cuda.is_available():
        pytest.skip("a HIP device is present")
    capi = st.capi
    rc, h, text = _dev_call(capi, _frames(capi, [(64, 48), (32, 32)] * 64), 64, 2)
    assert rc == capi.ERR_NO_DEVICE and h is None and "no HIP device" in text


# ---- the pooled threshold rule -----------------------------------------------------------------------------------------------
def _threshold(n_sets, match_threshold=20, pooled_threshold=0):
    """The rule of include/stitch_calibrate.h, item 5."""
    return pooled_threshold if pooled_threshold else n_sets * match_threshold


def test_pooled_threshold_rule_on_hand_made_counts(st):
    from computervisionimagestich2_amd import pipeline
    capi = st.capi
    # dense4's recorded counts with the unevaluated entries filled in by hand: (0, 3) = 19 and (3, 0) = 11 stay below 20
    one = np.array([[0, 107, 58, 19], [96, 0, 170, 103], [54, 171, 0, 189], [11, 95, 194, 0]], np.int32)
    # with one capture the default is the plain rule
    assert _threshold(1) == 20
    assert capi.stitch_order_c(one, _threshold(1)) == capi.stitch_order_c(one) == pipeline.stitch_order(one)
    nb = lambda order: {frozenset(p) for p in order[1]}
    assert frozenset((0, 3)) not in nb(capi.stitch_order_c(one, _threshold(1)))
    # a second capture in which the pair has 1 and 9 matches: the pooled counts are 20 and 20
    two = np.array([[0, 90, 40, 1], [80, 0, 150, 90], [50, 160, 0, 170], [9, 90, 180, 0]], np.int32)
    pooled = one + two
    assert pooled[0, 3] == 20 and pooled[3, 0] == 20
    # an absolute threshold is honoured: 20 makes cameras 0 and 3 neighbours, the default mean rule (40) does not
    assert _threshold(2, pooled_threshold=20) == 20 and _threshold(2) == 40
    with_abs, with_mean = capi.stitch_order_c(pooled, 20), capi.stitch_order_c(pooled, 40)
    assert frozenset((0, 3)) in nb(with_abs) and frozenset((0, 3)) not in nb(with_mean)
    assert with_abs == pipeline.stitch_order(pooled, 20) and with_mean == pipeline.stitch_order(pooled, 40)
    # the mean rule: a pair at 39 pooled is no neighbour, at 40 it is
    pooled[0, 3], pooled[3, 0] = 39, 39
    assert frozenset((0, 3)) not in nb(capi.stitch_order_c(pooled, _threshold(2)))
    pooled[3, 0] = 40
    assert frozenset((0, 3)) in nb(capi.stitch_order_c(pooled, _threshold(2)))
