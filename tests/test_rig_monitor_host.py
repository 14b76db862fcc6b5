"""CPU: the host side of a rig's alignment monitor (include/stitch_rig_monitor.h) -- the header compiles as C99, the binding's table
RIG_MONITOR_SIGNATURES states exactly what it declares and shares no name with the other tables; stitch_residual_words; every
argument error is reported before a device is needed and leaves the rig as it was; the monitor's radius comes and goes on a rig made
from the recorded run "4"; and stitch_residual_best_shift against tests/residual_ref.py's Python integers on hand-made records."""
import ctypes as C
import json
import os
import re
import shlex
import subprocess

import numpy as np
import pytest

import residual_ref as rr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "stitch_rig_monitor.h")
GOLD = os.path.join(ROOT, "tests", "golden")

FUNCTIONS = ("stitch_residual_words", "stitch_dev_pairs_residual_u8", "stitch_rig_set_monitor", "stitch_rig_clear_monitor", "stitch_rig_monitor",
             "stitch_rig_residuals", "stitch_dev_rig_residual_domain_u8", "stitch_residual_best_shift")


def _header_text():
    return re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)


SCALARS = {"int": C.c_int, "int32_t": C.c_int, "float": C.c_float, "double": C.c_double, "size_t": C.c_size_t}
RETURNS = {"int": C.c_int, "void": None}


def _declared():
    """{name: (restype, argtypes)} of every prototype, by the binding's rules (tests/test_capi_abi.py, tests/test_rig_seams_host.py)."""
    sigs = {}
    for ret, name, params in re.findall(r"((?:const\s+)?\w+\s*\*?)\s*\b(stitch_\w+)\s*\(([^()]*)\)\s*;", _header_text()):
        prms = [] if params.strip() == "void" else [" ".join(p.split()) for p in params.split(",")]
        args = [C.c_void_p if ("*" in p or "[" in p) else SCALARS[" ".join(p.split()[:-1])] for p in prms]
        sigs[name] = (RETURNS[" ".join(ret.replace("*", " *").split())], args)
    return sigs


def _run4_rig(capi, **kw):
    with open(os.path.join(GOLD, "golden.json")) as f:
        steps = json.load(f)["runs"]["4"]["steps"]
    return capi.Rig.from_steps([(384, 512)] * 4, None, steps, **kw)


def test_signature_table_states_the_header(st):
    capi = st.capi
    want, lib = _declared(), capi.lib()
    assert sorted(want) == sorted(FUNCTIONS) == sorted(set(re.findall(r"\b(stitch_[a-z0-9_]+)\s*\(", _header_text())))
    assert sorted(capi.RIG_MONITOR_SIGNATURES) == sorted(want)
    others = set(capi.SIGNATURES) | set(capi.PANORAMA_SIGNATURES) | set(capi.RIG_SIGNATURES) | set(capi.EXPOSURE_SIGNATURES) \
        | set(capi.RIG_EXPOSURE_SIGNATURES) | set(capi.CALIBRATE_SIGNATURES) | set(capi.RIG_SEAMS_SIGNATURES) | set(capi.COLLAPSE_SIDES_SIGNATURES) \
        | set(capi.SRC_RUNS_SIGNATURES) | set(capi.RIG_CROP_SIGNATURES) | set(capi.RIG_FORMAT_SIGNATURES)
    assert not set(capi.RIG_MONITOR_SIGNATURES) & others
    bound = {n: (getattr(lib, n).restype, getattr(lib, n).argtypes) for n in want}  # every name is exported
    wrong = {n: (bound[n], want[n]) for n in sorted(want) if bound[n] != tuple(want[n])}
    assert not wrong, f"(bound, declared) signatures differ for: {wrong}"
    assert lib.stitch_abi_version() == 5  # the ABI version stays


def test_header_is_c99(st, tmp_path):
    cc = shlex.split(os.environ.get("CC", "cc")) + ["-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include")]
    src = tmp_path / "uses.c"
    src.write_text("\n".join(['#include "stitch_rig_monitor.h"', "void uses(void) {"] + [f"    (void)(&{n});" for n in FUNCTIONS]
                             + ["    (void)(STITCH_RESIDUAL_MAX_RADIUS + 0);", "}", ""]))
    r = subprocess.run(cc + ["-fsyntax-only", str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_residual_words(st):
    capi = st.capi
    assert [capi.residual_words(r) for r in range(9)] == [2 + 3 * (2 * r + 1) ** 2 for r in range(9)] == [rr.words(r) for r in range(9)]
    assert capi.residual_words(8) == 869
    assert [capi.residual_words(r) for r in (-1, 9, 2 ** 31 - 1, -2 ** 31)] == [0, 0, 0, 0]


def test_monitor_round_trip_on_the_recorded_run(st):
    capi = st.capi
    L = capi.lib()
    rig = _run4_rig(capi)
    assert rig.n_steps == 3 and rig.monitor is None
    r = C.c_int(77)
    assert L.stitch_rig_monitor(rig._h, C.byref(r)) == 0 and r.value == -1
    for radius in (0, 1, 8, 4):
        assert rig.set_monitor(radius) is rig and rig.monitor == radius
        for bad in (-1, 9, 100, -2 ** 31):
            assert L.stitch_rig_set_monitor(rig._h, bad) == capi.ERR_ARG and b"rig_set_monitor" in L.stitch_last_error()
            assert rig.monitor == radius  # the rig stays as it was
        with pytest.raises(capi.StitchError) as e:
            rig.set_monitor(9)
        assert e.value.code == capi.ERR_ARG and rig.monitor == radius
    # no monitored call has completed: no sets, the rig's steps, the radius set
    n_sets, n_steps, radius = C.c_int(7), C.c_int(7), C.c_int(7)
    assert L.stitch_rig_residuals(rig._h, None, 0, C.byref(n_sets), C.byref(n_steps), C.byref(radius)) == 0
    assert (n_sets.value, n_steps.value, radius.value) == (0, 3, 4)
    assert L.stitch_rig_residuals(rig._h, None, 0, None, None, None) == 0  # every output is optional
    assert rig.residuals().shape == (0, 3, capi.residual_words(4))
    assert rig.clear_monitor() is rig and rig.monitor is None
    assert rig.clear_monitor().monitor is None  # clearing twice is fine
    assert L.stitch_rig_monitor(rig._h, None) == 0
    assert L.stitch_rig_set_monitor(None, 1) == L.stitch_rig_clear_monitor(None) == L.stitch_rig_monitor(None, C.byref(r)) == capi.ERR_ARG
    assert L.stitch_rig_residuals(None, None, 0, None, None, None) == capi.ERR_ARG
    assert rig.step_plan(0) is None  # no device was touched
    rig.close()
    zero = capi.Rig.from_steps([(64, 48)], 0, [])  # nothing to monitor, and the calls succeed
    assert zero.set_monitor(3).monitor == 3 and zero.residuals().shape == (0, 0, capi.residual_words(3)) and zero.clear_monitor().monitor is None
    zero.close()


def test_argument_errors_come_before_a_device(st):
    import torch
    capi = st.capi
    L = capi.lib()
    rig = _run4_rig(capi).set_monitor(2)
    for step in (-2, 3):
        assert L.stitch_dev_rig_residual_domain_u8(rig._h, step, 1, 0x1000, None) == capi.ERR_ARG
    for radius in (-1, 9):
        assert L.stitch_dev_rig_residual_domain_u8(rig._h, 0, radius, 0x1000, None) == capi.ERR_ARG
    assert L.stitch_dev_rig_residual_domain_u8(None, 0, 1, 0x1000, None) == L.stitch_dev_rig_residual_domain_u8(rig._h, 0, 1, None, None) == capi.ERR_ARG
    zero = capi.Rig.from_steps([(64, 48)], 0, [])
    for step in (-1, 0):
        assert L.stitch_dev_rig_residual_domain_u8(zero._h, step, 1, 0x1000, None) == capi.ERR_ARG
    zero.close()
    assert rig.monitor == 2

    def pairs(n=1, **kw):
        arr = (capi.PairDesc * n)()
        for d in arr:
            d.frame, d.fw, d.fh, d.mosaic, d.mw, d.mh = 0x1000, 8, 8, 0x2000, 8, 8
            d.p = capi._map8([1, 0, 0, 0, 0, 1, 0, 0])
            for k, v in kw.items():
                setattr(d, k, v)
        return arr

    dom = (C.c_void_p * 2)(0x3000, 0x3000)
    call = L.stitch_dev_pairs_residual_u8
    assert call(None, 1, 8, 8, dom, 1, 0x4000, None) == call(pairs(), 1, 8, 8, None, 1, 0x4000, None) == call(pairs(), 1, 8, 8, dom, 1, None, None) == capi.ERR_ARG
    for radius in (-1, 9):
        assert call(pairs(), 1, 8, 8, dom, radius, 0x4000, None) == capi.ERR_ARG
    for n in (0, -1, 65536):
        assert call(pairs(), n, 8, 8, dom, 1, 0x4000, None) == capi.ERR_ARG
    for cw, ch in ((0, 8), (8, 0), (-1, 8), (65536, 32768)):
        assert call(pairs(), 1, cw, ch, dom, 1, 0x4000, None) == capi.ERR_ARG, (cw, ch)
    for kw in (dict(frame=None), dict(mosaic=None), dict(fw=0), dict(fh=-1), dict(mw=0), dict(mh=0)):
        assert call(pairs(2, **kw), 2, 8, 8, dom, 1, 0x4000, None) == capi.ERR_ARG, kw
    assert call(pairs(2), 2, 8, 8, (C.c_void_p * 2)(0x3000, None), 1, 0x4000, None) == capi.ERR_ARG
    if not torch.cuda.is_available():  # and what is left needs one
        assert call(pairs(), 1, 8, 8, dom, 1, 0x4000, None) == capi.ERR_NO_DEVICE
        assert call(pairs(), 1, 2, 8, dom, 1, 0x4000, None) == capi.ERR_NO_DEVICE  # cw <= 2r is a valid canvas
        assert L.stitch_dev_rig_residual_domain_u8(rig._h, -1, 8, 0x1000, None) == capi.ERR_NO_DEVICE
    rig.close()


# ---- stitch_residual_best_shift ---------------------------------------------------------------------------------------------------
def _record(r, n, sum_b, shifts, fill=(0, 10 ** 6, 10 ** 12)):
    """shifts: {(dx, dy): (sum_a, sad, ssd)}; every other shift is `fill`."""
    rec = [n, sum_b]
    for dy in range(-r, r + 1):
        for dx in range(-r, r + 1):
            rec += list(shifts.get((dx, dy), fill))
    return rec


def _best(capi, rec, r, zero_mean):
    got = capi.residual_best_shift(np.array(rec, np.uint64), r, zero_mean)
    assert got == rr.best_shift(rec, r, zero_mean)
    return got


def test_best_shift_on_hand_made_records(st):
    capi = st.capi
    L = capi.lib()
    # a plain minimum, both ways, at every radius
    for r in range(9):
        for at in ((0, 0), (r, -r), (-r, r), (-r, -r), (r, r)):
            rec = _record(r, 100, 0, {at: (0, 5, 7)})
            assert _best(capi, rec, r, False) == at and _best(capi, rec, r, True) == at
    # an exact tie, by each rule in turn: the shortest shift ...
    assert _best(capi, _record(2, 10, 0, {(2, 2): (0, 1, 3), (-1, 0): (0, 1, 3), (-2, -2): (0, 1, 3)}), 2, False) == (-1, 0)
    # ... then, at one length, the smallest dy ...
    assert _best(capi, _record(2, 10, 0, {(1, 2): (0, 1, 3), (2, -1): (0, 1, 3), (-2, 1): (0, 1, 3), (2, 1): (0, 1, 3)}), 2, False) == (2, -1)
    # ... then, in one row, the smallest dx
    assert _best(capi, _record(2, 10, 0, {(2, -1): (0, 1, 3), (-2, -1): (0, 1, 3), (1, 2): (0, 1, 3)}), 2, False) == (-2, -1)
    assert _best(capi, _record(1, 10, 0, {}), 1, False) == (0, 0)  # all equal: the shift of no motion
    # zero_mean changes the answer: (1, 0) has the smaller ssd, (-1, 1) is a pure offset of 10 per pixel
    n = 50
    rec = _record(1, n, 1000, {(1, 0): (1000, 300, 2000), (-1, 1): (1000 + 10 * n, 10 * n, 100 * n)})
    assert _best(capi, rec, 1, False) == (1, 0) and _best(capi, rec, 1, True) == (-1, 1)
    # n * ssd beyond 2^64: a 64-bit product would wrap and turn the order around
    n, big = 2 ** 31 - 1, 2 ** 50
    rec = _record(1, n, 0, {(0, 1): (0, 0, big + 2 ** 20), (1, 1): (0, 0, big)}, fill=(0, 0, 2 ** 51 - 1))
    assert n * big > 2 ** 64 and (n * (big + 2 ** 20)) % 2 ** 64 < (n * big) % 2 ** 64
    assert _best(capi, rec, 1, True) == (1, 1) and _best(capi, rec, 1, False) == (1, 1)
    # the square of the difference of the sums beyond 2^64 as well
    rec = _record(1, n, 2 ** 40, {(0, 1): (2 ** 40 + 2 ** 33, 0, big), (1, 1): (2 ** 40, 0, big)}, fill=(2 ** 40, 0, 2 ** 51 - 1))
    assert _best(capi, rec, 1, True) == (0, 1) and _best(capi, rec, 1, False) == (0, 1)
    # n = 0
    empty = np.zeros(capi.residual_words(1), np.uint64)
    dx, dy = C.c_int(5), C.c_int(5)
    assert L.stitch_residual_best_shift(capi._p(empty), 1, 0, C.byref(dx), C.byref(dy)) == capi.ERR_ZERO_OVERLAP and (dx.value, dy.value) == (5, 5)
    assert rr.best_shift(empty, 1) is None
    with pytest.raises(capi.StitchError) as e:
        capi.residual_best_shift(empty, 1, True)
    assert e.value.code == capi.ERR_ZERO_OVERLAP
    # arguments
    one = np.array(_record(0, 1, 0, {}), np.uint64)
    assert L.stitch_residual_best_shift(capi._p(one), 0, 0, None, None) == 0  # the outputs are optional
    assert L.stitch_residual_best_shift(None, 0, 0, C.byref(dx), C.byref(dy)) == capi.ERR_ARG
    for radius in (-1, 9):
        assert L.stitch_residual_best_shift(capi._p(one), radius, 0, C.byref(dx), C.byref(dy)) == capi.ERR_ARG
