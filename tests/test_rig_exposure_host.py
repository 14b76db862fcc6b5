"""CPU: the host side of the exposure-matched rig replay (include/stitch_rig_exposure.h) -- the header compiles as C99, the
binding's fifth signature table states exactly what it declares and shares no name with the four others -- and
stitch_rig_create_exposure, which is host arithmetic only: on the reference's recorded run "4" (tests/golden/golden.json, with each
step's template frame from tests/golden/exposure.json) every mode reports the recorded final shape; mode 1 refuses a step whose
template is not a frame already placed, where modes 0 and 2 take the same record; a mode or a stats_form outside 0 .. 2 is
refused."""
import ctypes as C
import json
import os
import re
import shlex
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
HEADER = os.path.join(ROOT, "include", "stitch_rig_exposure.h")

FUNCTIONS = ("stitch_rig_create_exposure", "stitch_rig_from_panorama_exposure", "stitch_dev_rig_stitch_exposure_u8", "stitch_dev_transfer_many_u8")


# ---- the header ------------------------------------------------------------------------------------------------------------
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
    assert sorted(capi.RIG_EXPOSURE_SIGNATURES) == sorted(want)
    others = set(capi.SIGNATURES) | set(capi.PANORAMA_SIGNATURES) | set(capi.RIG_SIGNATURES) | set(capi.EXPOSURE_SIGNATURES)
    assert not set(capi.RIG_EXPOSURE_SIGNATURES) & others
    bound = {n: (getattr(lib, n).restype, getattr(lib, n).argtypes) for n in want}
    wrong = {n: (bound[n], want[n]) for n in sorted(want) if bound[n] != tuple(want[n])}
    assert not wrong, f"(bound, declared) signatures differ for: {wrong}"
    assert lib.stitch_abi_version() == 5


def test_header_is_c99(st, tmp_path):
    cc = shlex.split(os.environ.get("CC", "cc")) + ["-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include")]
    src = tmp_path / "uses.c"
    src.write_text("\n".join(['#include "stitch_rig_exposure.h"', "void uses(void) {"] + [f"    (void)(&{n});" for n in FUNCTIONS]
                             + ["    (void)sizeof(stitch_rig_opts);", "    (void)sizeof(stitch_exposure_opts);", "    (void)STITCH_STATS_DIAG;", "}", ""]))
    r = subprocess.run(cc + ["-fsyntax-only", str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


# ---- creation on the recorded run "4" ----------------------------------------------------------------------------------------
def _run4():
    """Sizes, start, the step dicts of golden.json with `mosaic_src` from exposure.json, and the final shape."""
    with open(os.path.join(GOLD, "golden.json")) as f:
        run = json.load(f)["runs"]["4"]
    with open(os.path.join(GOLD, "exposure.json")) as f:
        rec = json.load(f)["runs"]["4"]["mode1_keep_black1"]["steps"]
    assert [s["src"] for s in rec] == [s["src"] for s in run["steps"]]
    steps = [dict(s, mosaic_src=r["mosaic_src"]) for s, r in zip(run["steps"], rec)]
    sizes = [(run["steps"][0]["fw"], run["steps"][0]["fh"])] * 4
    return sizes, run["steps"][0]["start"], steps, run["final_shape"]


def _create(capi, sizes, start, steps, exposure):
    """-> (rc, handle value, error text); exposure: None for a NULL pointer, else (mode, stats_form, keep_black)"""
    wh = np.ascontiguousarray(np.array(sizes, np.int32).reshape(-1, 2))
    _, arr = capi.rig_steps(steps, start)
    e = None if exposure is None else C.byref(capi.ExposureOpts(*exposure))
    h = C.c_void_p(0xdead)
    rc = capi.lib().stitch_rig_create_exposure(wh.ctypes.data_as(C.c_void_p), len(sizes), start, arr, len(steps), None, e, C.byref(h))
    return rc, h, capi.lib().stitch_last_error().decode()


def _shape(capi, h):
    w, ht, n, ns, ms = (C.c_int() for _ in range(5))
    assert capi.lib().stitch_rig_info(h, C.byref(w), C.byref(ht), C.byref(n), C.byref(ns), C.byref(ms)) == 0
    return [3, ht.value, w.value], n.value, ns.value, ms.value


@pytest.mark.parametrize("exposure", [None, (0, 0, 0), (0, 2, 1), (1, 2, 1), (1, 0, 0), (2, 2, 1), (2, 1, 0)])
def test_every_mode_reports_the_recorded_shape(st, exposure):
    capi = st.capi
    sizes, start, steps, final_shape = _run4()
    rc, h, text = _create(capi, sizes, start, steps, exposure)
    assert rc == 0 and h.value, text
    assert _shape(capi, h) == (final_shape, 4, 3, 16)
    assert capi.lib().stitch_rig_step_plan(h, 0) is None  # no device was touched
    capi.lib().stitch_rig_destroy(h)


def test_the_binding_takes_the_new_call_for_a_mode(st):
    capi = st.capi
    sizes, start, steps, final_shape = _run4()
    for mode in (0, 1, 2):
        rig = capi.Rig.from_steps(sizes, start, steps, exposure=mode, keep_black=False, stats_form=0, max_sets=3)
        assert [3, rig.height, rig.width] == final_shape and rig.max_sets == 3
        rig.close()
    with pytest.raises(capi.StitchError) as e:
        capi.Rig.from_steps(sizes, start, [dict(s, mosaic_src=-1) for s in steps], exposure=1)
    assert e.value.code == capi.ERR_ARG


def test_mode_1_needs_a_template_that_is_placed(st):
    capi = st.capi
    sizes, start, steps, _ = _run4()
    placed = [start]
    unplaced_later = None  # (step, frame): a frame that no step before `step` has placed, other than the step's own dst
    for k, s in enumerate(steps):
        free = [f for f in range(4) if f not in placed and f != s["src"]]
        if free and unplaced_later is None:
            unplaced_later = (k, free[0])
        placed.append(s["src"])
    assert unplaced_later is not None
    k_own = next(k for k, s in enumerate(steps) if s["src"] not in ([start] + [t["src"] for t in steps[:k]]))
    cases = {"src = -1": (1, -1), "src = a frame no earlier step has placed": unplaced_later, "src = the step's own dst": (k_own, steps[k_own]["src"]),
             "src = n": (2, 4)}
    for what, (k, frame) in cases.items():
        bad = [dict(s) for s in steps]
        bad[k]["mosaic_src"] = frame
        rc, h, text = _create(capi, sizes, start, bad, (1, 2, 1))
        assert rc == capi.ERR_ARG and h.value is None, f"{what}: rc {rc}"
        assert text.startswith("rig") and f"step {k}" in text and f"frame {frame}" in text, f"{what}: '{text}'"
        for exposure in (None, (0, 0, 0), (2, 2, 1), (2, 0, 0)):  # recorded, not checked
            rc, h, text = _create(capi, sizes, start, bad, exposure)
            assert rc == 0 and h.value, f"{what} under {exposure}: '{text}'"
            capi.lib().stitch_rig_destroy(h)
        # stitch_rig_create takes the record, and so does the new call without options
        wh = np.ascontiguousarray(np.array(sizes, np.int32).reshape(-1, 2))
        h = C.c_void_p()
        assert capi.lib().stitch_rig_create(wh.ctypes.data_as(C.c_void_p), 4, start, capi.rig_steps(bad, start)[1], 3, None, C.byref(h)) == 0
        capi.lib().stitch_rig_destroy(h)


def test_bad_options_and_what_stitch_rig_create_checks(st):
    capi = st.capi
    sizes, start, steps, _ = _run4()
    for exposure in ((3, 2, 1), (-1, 2, 1), (1, 3, 1), (2, -1, 0), (0, 3, 0), (3, 0, 0)):
        rc, h, text = _create(capi, sizes, start, steps, exposure)
        assert rc == capi.ERR_ARG and h.value is None and "exposure" in text, (exposure, text)
    # the checks of stitch_rig_create hold under every mode
    for exposure in (None, (1, 2, 1), (2, 2, 1)):
        bad = [dict(s) for s in steps]
        bad[1]["cw"] += 1
        rc, h, text = _create(capi, sizes, start, bad, exposure)
        assert rc == capi.ERR_ARG and h.value is None and "step 1" in text
        rc, h, text = _create(capi, sizes, 4, steps, exposure)
        assert rc == capi.ERR_ARG and h.value is None
        rc, h, text = _create(capi, [(0, 512)] + sizes[1:], start, steps, exposure)
        assert rc == capi.ERR_ARG and h.value is None
    assert capi.lib().stitch_rig_create_exposure(None, 4, 0, None, 0, None, None, None) == capi.ERR_ARG
    assert capi.lib().stitch_rig_from_panorama_exposure(None, None, 4, None, None, None) == capi.ERR_ARG


def test_calls_without_a_device(st):
    """Without a device the replay and the many-image transfer report need_device's status and touch nothing."""
    import torch
    if torch.cuda.is_available():
        pytest.skip("a HIP device is present")
    capi = st.capi
    sizes, start, steps, _ = _run4()
    rig = capi.Rig.from_steps(sizes, start, steps, exposure=1)
    frames = (capi.FrameU8 * 4)(*[capi.FrameU8(0x1000 * (i + 1), 384, 512) for i in range(4)])
    outs, status = (C.c_void_p * 1)(0x9000), (C.c_int32 * 1)(77)
    stats = np.full(36, 5.0, np.float32)
    assert capi.lib().stitch_dev_rig_stitch_exposure_u8(rig._h, frames, 1, outs, status, None, stats.ctypes.data_as(C.c_void_p), None) == capi.ERR_NO_DEVICE
    assert status[0] == 77 and (stats == 5.0).all() and b"no HIP device" in capi.lib().stitch_last_error()
    assert capi.lib().stitch_dev_transfer_many_u8(outs, outs, outs, 1, 8, 8, 8, 8, 2, 0, None, None, None) == capi.ERR_NO_DEVICE
    rig.close()
