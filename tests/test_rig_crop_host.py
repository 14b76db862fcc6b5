"""CPU: the host side of the crop of a rig's output (include/stitch_rig_crop.h) -- the header compiles as C99, the binding's table
RIG_CROP_SIGNATURES states exactly what it declares and shares no name with the other tables; stitch_rig_set_crop refuses every bad
argument and leaves the rig as it was; stitch_rig_clear_crop restores the whole canvas; and every argument error of the device calls
is reported before a device is needed."""
import ctypes as C
import os
import re
import shlex
import subprocess

import pytest

import rig_seams_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "stitch_rig_crop.h")

FUNCTIONS = ("stitch_dev_largest_rect_u8", "stitch_dev_rig_inscribed_rect", "stitch_rig_set_crop", "stitch_rig_clear_crop", "stitch_rig_crop",
             "stitch_rig_output_size")


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


def test_signature_table_states_the_header(st):
    capi = st.capi
    want, lib = _declared(), capi.lib()
    assert sorted(want) == sorted(FUNCTIONS) == sorted(set(re.findall(r"\b(stitch_[a-z0-9_]+)\s*\(", _header_text())))
    assert sorted(capi.RIG_CROP_SIGNATURES) == sorted(want)
    others = set(capi.SIGNATURES) | set(capi.PANORAMA_SIGNATURES) | set(capi.RIG_SIGNATURES) | set(capi.EXPOSURE_SIGNATURES) \
        | set(capi.RIG_EXPOSURE_SIGNATURES) | set(capi.CALIBRATE_SIGNATURES) | set(capi.RIG_SEAMS_SIGNATURES) | set(capi.COLLAPSE_SIDES_SIGNATURES) \
        | set(capi.SRC_RUNS_SIGNATURES)
    assert not set(capi.RIG_CROP_SIGNATURES) & others
    bound = {n: (getattr(lib, n).restype, getattr(lib, n).argtypes) for n in want}  # every name is exported
    wrong = {n: (bound[n], want[n]) for n in sorted(want) if bound[n] != tuple(want[n])}
    assert not wrong, f"(bound, declared) signatures differ for: {wrong}"
    assert lib.stitch_abi_version() == 5
    assert C.sizeof(capi.Rect) == 16 and [f[0] for f in capi.Rect._fields_] == ["x0", "y0", "w", "h"]
    assert (capi.CROP_AFTER_FINISH, capi.CROP_BEFORE_FINISH) == (1, 2)


def test_header_is_c99(st, tmp_path):
    cc = shlex.split(os.environ.get("CC", "cc")) + ["-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include")]
    src = tmp_path / "uses.c"
    src.write_text("\n".join(['#include "stitch_rig_crop.h"', "void uses(void) {"] + [f"    (void)(&{n});" for n in FUNCTIONS]
                             + ["    (void)sizeof(stitch_rect);", "    (void)(STITCH_CROP_AFTER_FINISH + STITCH_CROP_BEFORE_FINISH);", "}", ""]))
    r = subprocess.run(cc + ["-fsyntax-only", str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def _state(capi, rig):
    """What stitch_rig_crop and stitch_rig_output_size report, read through the library."""
    r, mode, w, h = capi.Rect(), C.c_int(-1), C.c_int(-1), C.c_int(-1)
    assert capi.lib().stitch_rig_crop(rig._h, C.byref(r), C.byref(mode)) == 0
    assert capi.lib().stitch_rig_output_size(rig._h, C.byref(w), C.byref(h)) == 0
    return r.as_tuple(), mode.value, w.value, h.value


def test_set_crop_checks_and_clear_crop_restores(st):
    capi = st.capi
    L = capi.lib()
    rig = capi.Rig.from_steps(ref.SMALL, 0, ref.small_steps(capi))
    W, H = rig.width, rig.height
    whole = ((0, 0, W, H), 0, W, H)
    assert _state(capi, rig) == whole and rig.crop == (whole[0], 0) and (rig.out_width, rig.out_height) == (W, H)
    bad = [((0, 0, 0, 5), 1), ((0, 0, 5, 0), 1), ((0, 0, -1, 5), 1), ((-1, 0, 5, 5), 1), ((0, -1, 5, 5), 1), ((0, 0, W + 1, 1), 1), ((0, 0, 1, H + 1), 1),
           ((W - 4, 0, 5, 5), 2), ((0, H - 4, 5, 5), 2), ((W, 0, 1, 1), 1), ((0, 0, 5, 5), 0), ((0, 0, 5, 5), 3), ((0, 0, 5, 5), -1),
           ((2 ** 31 - 1, 0, 2 ** 31 - 1, 1), 1)]
    for before in (None, ((3, 2, 11, 7), 2)):
        if before:
            assert rig.set_crop(*before) is rig
        kept = _state(capi, rig)
        assert kept == (whole if before is None else (before[0], before[1], 11, 7))
        for rect, mode in bad:
            assert L.stitch_rig_set_crop(rig._h, C.byref(capi.Rect(*rect)), mode) == capi.ERR_ARG, (rect, mode)
            assert b"rig_set_crop" in L.stitch_last_error()
            assert _state(capi, rig) == kept
        assert L.stitch_rig_set_crop(rig._h, None, 1) == capi.ERR_ARG and L.stitch_rig_set_crop(None, C.byref(capi.Rect(0, 0, 1, 1)), 1) == capi.ERR_ARG
        assert _state(capi, rig) == kept
        with pytest.raises(capi.StitchError) as e:
            rig.set_crop((0, 0, W + 1, 1))
        assert e.value.code == capi.ERR_ARG and _state(capi, rig) == kept
    # the edges of the canvas are inside it
    for rect in ((0, 0, W, H), (W - 1, H - 1, 1, 1), (0, H - 1, W, 1), (1, 0, 1, H)):
        for mode in (1, 2):
            assert rig.set_crop(rect, mode).crop == (rect, mode) and (rig.out_width, rig.out_height) == rect[2:]
    assert (rig.width, rig.height) == (W, H)  # stitch_rig_info keeps the canvas
    v = [C.c_int() for _ in range(2)]
    assert L.stitch_rig_info(rig._h, C.byref(v[0]), C.byref(v[1]), None, None, None) == 0 and (v[0].value, v[1].value) == (W, H)
    assert rig.clear_crop() is rig and _state(capi, rig) == whole
    assert rig.clear_crop().crop == (whole[0], 0)  # clearing twice is fine
    # outputs are optional, a null handle is not
    assert L.stitch_rig_crop(rig._h, None, None) == 0 and L.stitch_rig_output_size(rig._h, None, None) == 0
    assert L.stitch_rig_crop(None, None, None) == L.stitch_rig_output_size(None, None, None) == L.stitch_rig_clear_crop(None) == capi.ERR_ARG
    assert rig.step_plan(0) is None  # no device was touched
    rig.close()
    zero = capi.Rig.from_steps([(64, 48), (50, 37)], 1, [])
    assert zero.set_crop((1, 1, 49, 36), 2).crop == ((1, 1, 49, 36), 2)
    with pytest.raises(capi.StitchError):
        zero.set_crop((1, 1, 50, 36))
    zero.close()


def test_argument_errors_come_before_a_device(st):
    import torch
    capi = st.capi
    L = capi.lib()
    rig = capi.Rig.from_steps(ref.SMALL, 0, ref.small_steps(capi))
    r = capi.Rect(9, 9, 9, 9)
    for step in (-2, 2):
        assert L.stitch_dev_rig_inscribed_rect(rig._h, step, C.byref(r), None) == capi.ERR_ARG
    assert L.stitch_dev_rig_inscribed_rect(None, -1, C.byref(r), None) == L.stitch_dev_rig_inscribed_rect(rig._h, -1, None, None) == capi.ERR_ARG
    for w, h in ((0, 5), (5, 0), (-1, 5), (65536, 32768), (2 ** 31 - 1, 2)):
        assert L.stitch_dev_largest_rect_u8(0x1000, w, h, C.byref(r), None) == capi.ERR_ARG, (w, h)
    assert L.stitch_dev_largest_rect_u8(None, 4, 4, C.byref(r), None) == L.stitch_dev_largest_rect_u8(0x1000, 4, 4, None, None) == capi.ERR_ARG
    assert r.as_tuple() == (9, 9, 9, 9)
    zero = capi.Rig.from_steps([(64, 48)], 0, [])
    assert L.stitch_dev_rig_inscribed_rect(zero._h, 0, C.byref(r), None) == capi.ERR_ARG
    if not torch.cuda.is_available():  # and what is left needs one
        assert L.stitch_dev_rig_inscribed_rect(rig._h, -1, C.byref(r), None) == capi.ERR_NO_DEVICE
        assert L.stitch_dev_largest_rect_u8(0x1000, 4, 4, C.byref(r), None) == capi.ERR_NO_DEVICE
        assert r.as_tuple() == (9, 9, 9, 9) and rig.crop[1] == 0
    zero.close()
    rig.close()
