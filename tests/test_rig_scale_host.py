"""CPU: the host side of a rig's output scale (include/stitch_rig_scale.h) -- the header compiles as C99, the binding's table
RIG_SCALE_SIGNATURES states exactly what it declares and shares no name with the other tables; every argument error of the
stand-alone call and of a replay whose scale the crop has broken is reported before a device is needed; the scale comes and goes on
a rig made from the recorded run "4"; and tests/scale_ref.py against a brute-force statement of the rule in fractions.Fraction, with
the four properties the header draws from it."""
import ctypes as C
import json
import os
import re
import shlex
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import scale_ref as sr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "stitch_rig_scale.h")
GOLD = os.path.join(ROOT, "tests", "golden")

FUNCTIONS = ("stitch_dev_scale_pack_many_u8", "stitch_rig_set_output_scale", "stitch_rig_clear_output_scale", "stitch_rig_output_scale")


def _header_text():
    return re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)


SCALARS = {"int": C.c_int, "int32_t": C.c_int, "float": C.c_float, "double": C.c_double, "size_t": C.c_size_t}
RETURNS = {"int": C.c_int, "void": None}


def _declared():
    """{name: (restype, argtypes)} of every prototype, by the binding's rules (tests/test_capi_abi.py, tests/test_rig_monitor_host.py)."""
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
    assert sorted(capi.RIG_SCALE_SIGNATURES) == sorted(want)
    others = set()
    for name in dir(capi):
        if name.endswith("SIGNATURES") and name != "RIG_SCALE_SIGNATURES":
            others |= set(getattr(capi, name))
    assert {"stitch_rig_output_size", "stitch_dev_pack_many_u8", "stitch_rig_set_monitor"} <= others  # the other tables were met
    assert not set(capi.RIG_SCALE_SIGNATURES) & others
    bound = {n: (getattr(lib, n).restype, getattr(lib, n).argtypes) for n in want}  # every name is exported
    wrong = {n: (bound[n], want[n]) for n in sorted(want) if bound[n] != tuple(want[n])}
    assert not wrong, f"(bound, declared) signatures differ for: {wrong}"
    assert lib.stitch_abi_version() == 5  # the ABI version stays


def test_header_is_c99(st, tmp_path):
    cc = shlex.split(os.environ.get("CC", "cc")) + ["-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include")]
    src = tmp_path / "uses.c"
    src.write_text("\n".join(['#include "stitch_rig_scale.h"', "void uses(void) {"] + [f"    (void)(&{n});" for n in FUNCTIONS]
                             + ["    (void)(STITCH_SCALE_MAX_FACTOR + 0);", "}", ""]))
    r = subprocess.run(cc + ["-fsyntax-only", str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert st.capi.SCALE_MAX_FACTOR == sr.MAX_FACTOR == int(re.search(r"#define STITCH_SCALE_MAX_FACTOR (\d+)", open(HEADER).read()).group(1))


# ---- argument errors, none of which needs a device -------------------------------------------------------------------------------
def _call(capi, fmt=0, matrix=0, src=(64, 16), rect=None, dst=(64, 16), count=1, planar=0x1000, data=0x100000, data2=0x200000, pitch=None, pitch2=None,
          null_tables=(), sizes=None):
    """stitch_dev_scale_pack_many_u8 on made-up addresses (never read: the checks come first) -> its return value."""
    L = capi.lib()
    tight = capi.tight_pitches(fmt, dst[0]) if fmt in capi._PIX_ALL else (0, 0)
    n = max(count, 1)
    ptrs = (C.c_void_p * n)(*[planar] * n)
    imgs = (capi.ImageDesc * n)()
    for i, im in enumerate(imgs):
        w, h = (sizes[i] if sizes else dst)
        im.data, im.data2, im.width, im.height = data, data2, w, h
        im.pitch, im.pitch2 = tight[0] if pitch is None else pitch, tight[1] if pitch2 is None else pitch2
    r = C.byref(capi.Rect(*rect)) if rect is not None else None
    return L.stitch_dev_scale_pack_many_u8(fmt, matrix, None if "planar" in null_tables else ptrs, src[0], src[1], r, None if "dst" in null_tables else imgs,
                                           count, None)


def test_argument_errors_come_before_a_device(st):
    import torch
    capi = st.capi
    L = capi.lib()
    bad = capi.ERR_ARG
    # a size outside the rule: enlargement, a factor above 8 (at w = 8 ow + 1 and h = 8 oh + 1), zero sizes
    assert _call(capi, src=(64, 16), dst=(65, 16)) == bad and b"scale_pack_many" in L.stitch_last_error()
    assert _call(capi, src=(64, 16), dst=(64, 17)) == bad
    assert _call(capi, src=(8 * 8 + 1, 16), dst=(8, 16)) == bad and _call(capi, src=(64, 8 * 2 + 1), dst=(64, 2)) == bad
    for dst in ((0, 16), (64, 0), (-1, 16), (0, 0)):
        assert _call(capi, dst=dst) == bad, dst
    for src in ((0, 16), (64, 0), (-3, 16), (65536, 32768)):
        assert _call(capi, src=src) == bad, src
    # a rectangle that is empty or not inside the image, and a target outside the rule of the RECTANGLE
    for rect in ((0, 0, 65, 16), (1, 0, 64, 16), (0, 1, 64, 16), (-1, 0, 8, 8), (0, -1, 8, 8), (0, 0, 0, 8), (0, 0, 8, 0), (60, 0, 8, 8), (2 ** 31 - 1, 0, 8, 8)):
        assert _call(capi, rect=rect, dst=(8, 8)) == bad, rect
    assert _call(capi, rect=(1, 1, 32, 8), dst=(33, 8)) == bad and _call(capi, rect=(1, 1, 33, 8), dst=(4, 8)) == bad
    # tables, counts, formats, matrices
    assert _call(capi, null_tables=("planar",)) == bad and _call(capi, null_tables=("dst",)) == bad and _call(capi, planar=None) == bad and _call(capi, data=None) == bad
    for count in (0, -1, 65536):
        assert _call(capi, count=count) == bad, count
    for fmt in (-1, 6, 15, 20):
        assert _call(capi, fmt=fmt) == bad, fmt
    for matrix in (-1, 3):
        assert _call(capi, fmt=capi.PIX_NV12, matrix=matrix) == bad, matrix
    # dst entries of differing sizes, pitches below a row, a missing second plane
    assert _call(capi, count=2, sizes=[(64, 16), (63, 16)]) == bad and _call(capi, count=2, sizes=[(64, 16), (64, 15)]) == bad
    assert _call(capi, fmt=capi.PIX_RGB24, pitch=3 * 64 - 1) == bad and _call(capi, fmt=capi.PIX_BGRX32, pitch=4 * 64 - 1) == bad
    assert _call(capi, fmt=capi.PIX_YUYV, dst=(63, 16), pitch=4 * 32 - 1) == bad
    assert _call(capi, fmt=capi.PIX_NV12, pitch=63) == bad and _call(capi, fmt=capi.PIX_NV21, dst=(63, 16), pitch2=63) == bad
    assert _call(capi, fmt=capi.PIX_NV16, data2=None) == bad
    if not torch.cuda.is_available():  # and what is left needs one: every format, the planar one with pitches that are ignored
        for fmt in capi._PIX_ALL:
            assert _call(capi, fmt=fmt, src=(131, 37), dst=(67, 19)) == capi.ERR_NO_DEVICE, fmt
        assert _call(capi, fmt=capi.PIX_PLANAR, pitch=1, pitch2=-5) == capi.ERR_NO_DEVICE
        assert _call(capi, src=(150, 50), rect=(7, 5, 131, 37), dst=(67, 19), count=5) == capi.ERR_NO_DEVICE
        assert _call(capi, src=(8, 8), dst=(1, 1)) == capi.ERR_NO_DEVICE and _call(capi, src=(64, 16), dst=(64, 16)) == capi.ERR_NO_DEVICE


def test_scale_round_trip_on_the_recorded_run(st):
    capi = st.capi
    L = capi.lib()
    rig = _run4_rig(capi)
    W, H = rig.width, rig.height
    assert (W, H) == (1081, 527) and rig.output_scale is None and (rig.out_width, rig.out_height) == (W, H)
    ow, oh = C.c_int(77), C.c_int(77)
    assert L.stitch_rig_output_scale(rig._h, C.byref(ow), C.byref(oh)) == 0 and (ow.value, oh.value) == (0, 0)
    for size in ((W, H), (540, 263), (136, 66), (W, 66), (136, H), (960, 527)):
        assert rig.set_output_scale(*size) is rig and rig.output_scale == size and (rig.out_width, rig.out_height) == size
        assert (rig.width, rig.height) == (W, H) and rig.crop == ((0, 0, W, H), 0)  # stitch_rig_info and the crop keep reporting the canvas
        for bad in ((W + 1, H), (W, H + 1), (135, 66), (136, 65), (0, 66), (136, 0), (-1, -1), (2 ** 31 - 1, 66)):
            assert L.stitch_rig_set_output_scale(rig._h, *bad) == capi.ERR_ARG and b"rig_set_output_scale" in L.stitch_last_error(), bad
            assert rig.output_scale == size  # the rig stays as it was
        with pytest.raises(capi.StitchError) as e:
            rig.set_output_scale(W + 1, H)
        assert e.value.code == capi.ERR_ARG and rig.output_scale == size
    assert rig.clear_output_scale() is rig and rig.output_scale is None and (rig.out_width, rig.out_height) == (W, H)
    assert rig.clear_output_scale().output_scale is None  # clearing twice is fine
    # the rule is checked against the crop's rectangle while one is set
    rect = (100, 50, 801, 401)
    rig.set_crop(rect, 1)
    assert L.stitch_rig_set_output_scale(rig._h, 802, 401) == capi.ERR_ARG and L.stitch_rig_set_output_scale(rig._h, 100, 401) == capi.ERR_ARG
    assert rig.set_output_scale(101, 51).output_scale == (101, 51) and (rig.out_width, rig.out_height) == (101, 51) and rig.crop == (rect, 1)
    assert L.stitch_rig_output_scale(rig._h, None, None) == 0  # every output is optional
    assert L.stitch_rig_set_output_scale(None, 1, 1) == L.stitch_rig_clear_output_scale(None) == L.stitch_rig_output_scale(None, C.byref(ow), C.byref(oh)) == capi.ERR_ARG
    assert rig.step_plan(0) is None  # no device was touched
    rig.close()


def test_a_crop_that_breaks_the_scale_fails_the_replay_before_a_device(st):
    """101 x 51 is a scale of the 801 x 401 rectangle; without the crop the source is the 1081 x 527 canvas, more than 8 times as wide."""
    capi = st.capi
    L = capi.lib()
    rig = _run4_rig(capi).set_crop((100, 50, 801, 401), 1).set_output_scale(101, 51)
    frames = (capi.FrameU8 * 4)(*[capi.FrameU8(0x1000, 384, 512)] * 4)
    images = (capi.ImageDesc * 4)(*[capi.ImageDesc(0x1000, None, 384, 512, 0, 0)] * 4)
    out = (C.c_void_p * 1)(0x4000000)
    out_image = (capi.ImageDesc * 1)(capi.ImageDesc(0x4000000, None, 101, 51, 0, 0))
    status, seams, stats = (C.c_int32 * 1)(), (capi.Seam * 3)(), (C.c_float * 36)()

    def replays():
        return [L.stitch_dev_rig_stitch_u8(rig._h, frames, 1, out, status, seams, None),
                L.stitch_dev_rig_stitch_exposure_u8(rig._h, frames, 1, out, status, seams, stats, None),
                L.stitch_dev_rig_stitch_fmt_u8(rig._h, images, 1, out_image, status, seams, None, None)]

    rig.clear_crop()
    assert rig.output_scale == (101, 51)  # the crop's calls leave the scale alone ...
    for rc in replays():  # ... and every replay refuses it
        assert rc == capi.ERR_ARG and b"output scale 101 x 51" in L.stitch_last_error() and b"1081 x 527" in L.stitch_last_error()
    rig.set_crop((0, 0, 100, 50), 2)  # smaller than the scale: an enlargement
    assert [rc for rc in replays()] == [capi.ERR_ARG] * 3 and b"100 x 50" in L.stitch_last_error()
    assert rig.step_plan(0) is None  # no device was touched
    rig.close()


# ---- tests/scale_ref.py against the rule in fractions ---------------------------------------------------------------------------------
def _brute(P, ow, oh):
    """The header's sentences, one output sample at a time: the overlap of two intervals per axis, S over all of P, one division."""
    h, w = P.shape
    out = np.zeros((oh, ow), np.int64)
    for Y in range(oh):
        for X in range(ow):
            S = Fraction(0)
            for y in range(h):
                wy = max(0, min((Y + 1) * h, (y + 1) * oh) - max(Y * h, y * oh))
                for x in range(w):
                    wx = max(0, min((X + 1) * w, (x + 1) * ow) - max(X * w, x * ow))
                    S += wy * wx * int(P[y, x])
            mean = S / (w * h)
            out[Y, X] = int(mean + Fraction(1, 2))  # floor(mean + 1/2): rounded half up
    return out


@pytest.mark.parametrize("w,h,ow,oh", [(7, 5, 5, 3), (13, 4, 4, 1), (8, 8, 1, 1), (9, 2, 9, 2)])
def test_scale_ref_against_fractions(w, h, ow, oh):
    rng = np.random.default_rng(1000 * w + ow)
    for kind in ("random", "extremes", "half"):
        P = rng.integers(0, 256, (3, h, w)).astype(np.uint8)
        if kind == "extremes":
            P = (255 * rng.integers(0, 2, (3, h, w))).astype(np.uint8)
        if kind == "half":  # means that end in exactly one half somewhere: 0 and 1 under a factor of two on an axis
            P = rng.integers(0, 2, (3, h, w)).astype(np.uint8)
        got = sr.scale(P, ow, oh)
        assert got.shape == (3, oh, ow) and got.dtype == np.uint8
        for c in range(3):
            assert np.array_equal(got[c], _brute(P[c], ow, oh)), (kind, c)
        # the gathered product is the matrix product
        Wx, Wy = sr.weights(w, ow), sr.weights(h, oh)
        assert np.array_equal(sr.sums(P, ow, oh), np.stack([Wy @ P[c].astype(np.int64) @ Wx.T for c in range(3)]))
    assert not sr.rule(w, h, ow + (w - ow) + 1, oh) and sr.rule(w, h, ow, oh)


def test_the_four_properties():
    rng = np.random.default_rng(7)
    # row sums of Wx equal to w, whatever the ratio; every weight inside [0, ow]
    for w, ow in ((7, 5), (13, 4), (8, 1), (9, 9), (131, 67), (2056, 257), (1081, 540), (4421, 3840)):
        W = sr.weights(w, ow)
        assert W.shape == (ow, w) and (W.sum(1) == w).all() and (W.sum(0) == ow).all() and W.min() >= 0 and W.max() <= ow
        assert ((W != 0).sum(1) <= 9).all()
    # identity
    P = rng.integers(0, 256, (3, 37, 131)).astype(np.uint8)
    assert np.array_equal(sr.scale(P, 131, 37), P)
    # constants stay constant, at a coprime ratio
    for v in (0, 255, 1, 128):
        assert (sr.scale(np.full((3, 37, 131), v, np.uint8), 67, 19) == v).all()
    # a factor of two is (a + b + c + d + 2) >> 2
    P = rng.integers(0, 256, (3, 32, 128)).astype(np.int64)
    want = (P[:, 0::2, 0::2] + P[:, 0::2, 1::2] + P[:, 1::2, 0::2] + P[:, 1::2, 1::2] + 2) >> 2
    assert np.array_equal(sr.scale(P.astype(np.uint8), 64, 16), want)
    # separable without a rounding between: on one axis alone the other is the identity
    P = rng.integers(0, 256, (3, 9, 2056)).astype(np.uint8)
    H = sr.apply(P, sr.weights(2056, 257))
    assert H.max() <= 255 * 2056 and np.array_equal(sr.scale(P, 257, 9), (2 * H + 2056) // (2 * 2056))
    # pack on top: the scaled image is an image of its own
    import pixfmt_yuv_ref as pyr
    im = sr.scale_pack(pyr.NV12, np.pad(P[:, :, :131], ((0, 0), (3, 0), (5, 0))), 67, 5, rect=(5, 3, 131, 9))
    assert (im["w"], im["h"]) == (67, 5) and np.array_equal(im["data"], pyr.pack(sr.scale(P[:, :, :131], 67, 5), pyr.NV12)["data"])
