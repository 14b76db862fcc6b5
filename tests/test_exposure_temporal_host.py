"""CPU: the host side of temporal exposure for rigs (include/stitch_rig_exposure_temporal.h) -- the header compiles as C99 and the
binding's table RIG_EXPOSURE_TEMPORAL_SIGNATURES states exactly what it declares; tests/exposure_temporal_ref.py's apply with given
statistics is the oracle's transfer when fed the transfer's own statistics, bit for bit; its filter has the three properties the
header claims; every argument error of every new call is reported before a device is needed; and the rig's options come and go
without one."""
import ctypes as C
import json
import os
import re
import shlex
import subprocess

import numpy as np
import pytest

import exposure_temporal_ref as et
from test_seam_path_host import RETURNS, SCALARS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
HEADER = os.path.join(ROOT, "include", "stitch_rig_exposure_temporal.h")

FUNCTIONS = ("stitch_dev_transfer_given_many_u8", "stitch_dev_stats_filter_f32", "stitch_rig_set_exposure_smoothing", "stitch_rig_clear_exposure_smoothing",
             "stitch_rig_reset_exposure_state", "stitch_rig_prime_exposure_state", "stitch_rig_exposure_smoothing", "stitch_rig_exposure_state",
             "stitch_rig_fix_exposure", "stitch_rig_clear_fixed_exposure", "stitch_rig_fixed_exposure", "stitch_rig_last_used_stats")


def _header_text():
    return re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)


def _declared():
    """{name: (restype, argtypes)} of every prototype, by the binding's rules (tests/test_seam_path_host.py)."""
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
    assert sorted(capi.RIG_EXPOSURE_TEMPORAL_SIGNATURES) == sorted(want)
    others = set()
    for name in dir(capi):
        if name.endswith("SIGNATURES") and name != "RIG_EXPOSURE_TEMPORAL_SIGNATURES":
            others |= set(getattr(capi, name))
    assert "stitch_dev_transfer_many_u8" in others and not set(capi.RIG_EXPOSURE_TEMPORAL_SIGNATURES) & others
    bound = {n: (getattr(lib, n).restype, getattr(lib, n).argtypes) for n in want}  # every name is exported
    wrong = {n: (bound[n], want[n]) for n in sorted(want) if bound[n] != tuple(want[n])}
    assert not wrong, f"(bound, declared) signatures differ for: {wrong}"
    assert lib.stitch_abi_version() == 5  # the ABI version stays


def test_header_is_c99_and_its_constant(st, tmp_path):
    cc = shlex.split(os.environ.get("CC", "cc")) + ["-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include")]
    src = tmp_path / "uses.c"
    src.write_text("\n".join(['#include "stitch_rig_exposure_temporal.h"', "void uses(void) {"] + [f"    (void)(&{n});" for n in FUNCTIONS]
                             + ["    (void)STITCH_EXPOSURE_KEEP_MAX;", "}", ""]))
    r = subprocess.run(cc + ["-fsyntax-only", str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert int(re.search(r"#define STITCH_EXPOSURE_KEEP_MAX (\d+)", open(HEADER).read()).group(1)) == 255 == st.capi.EXPOSURE_KEEP_MAX
    assert np.float32(255) / np.float32(256) == 255 / 256  # every keep / 256 is exact in float


# ---- the statements ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h,tw,th,seed", [(5, 7, 9, 4, 1), (33, 65, 20, 31, 2), (64, 64, 64, 64, 3)])
def test_apply_given_is_the_transfer_on_its_own_statistics(oracle, w, h, tw, th, seed):
    rng = np.random.default_rng(seed)
    src = rng.integers(0, 256, (3, h, w)).astype(np.uint8)
    src[:, 0, :2] = 0  # black pixels: the transfer recolours them, keep_black is this project's addition
    tem = rng.integers(0, 200, (3, th, tw)).astype(np.uint8)
    want, stats = oracle.transfer(src, tem)
    assert et.valid(stats)
    got = et.apply_given(oracle, src, stats, False)
    assert np.array_equal(got, want)
    kept = et.apply_given(oracle, src, stats, True)
    black = (src == 0).all(axis=0)
    assert black.sum() >= 2 and (kept[:, black] == 0).all() and np.array_equal(kept[:, ~black], want[:, ~black])
    other = stats.copy()
    other[6] += np.float32(0.05)
    assert not np.array_equal(et.apply_given(oracle, src, other, False), want)  # the statistics are read


def _stream(rng, count):
    m = rng.normal(0.5, 0.3, (count, 12)).astype(np.float32)
    m[:, list(et.SD)] = np.abs(m[:, list(et.SD)]) + np.float32(0.01)
    return m


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32).tolist()


def test_filter_rules():
    rng = np.random.default_rng(24)
    m = _stream(rng, 9)
    # keep = 0: the identity, bit for bit, with or without a state; the state follows the stream
    for state in (None, m[3] * np.float32(1.7)):
        used, p = et.filter_stream(m, 0, state)
        assert _bits(used) == _bits(m) and _bits(p) == _bits(m[-1])
    # a constant stream: the identity for any keep
    same = np.repeat(m[:1], 6, axis=0)
    for keep in (1, 128, 192, 255):
        used, p = et.filter_stream(same, keep)
        assert _bits(used) == _bits(same) and _bits(p) == _bits(m[0])
    # no state: the first valid record passes and becomes the state; after it the filter is at work
    used, p = et.filter_stream(m, 192)
    assert _bits(used[0]) == _bits(m[0]) and _bits(used[1]) != _bits(m[1])
    want1 = (m[1] + (np.float32(0.75) * (m[0] - m[1]).astype(np.float32)).astype(np.float32)).astype(np.float32)
    assert _bits(used[1]) == _bits(want1) and _bits(p) == _bits(used[-1])
    # a record that is not valid passes as it came and leaves the state alone: the stream without it filters the same
    for j, bad in ((4, np.nan), (4, np.inf), (9, 0.0), (3, -1.0), (11, -0.0)):
        broken = m.copy()
        broken[4, j] = bad
        assert not et.valid(broken[4])
        used_b, p_b = et.filter_stream(broken, 192)
        used_w, p_w = et.filter_stream(np.delete(m, 4, axis=0), 192)
        assert _bits(used_b[4]) == _bits(broken[4])
        assert _bits(np.delete(used_b, 4, axis=0)) == _bits(used_w) and _bits(p_b) == _bits(p_w)
    # calls in a row are one stream
    a, pa = et.filter_stream(m[:4], 200)
    b, pb = et.filter_stream(m[4:], 200, pa)
    whole, pw = et.filter_stream(m, 200)
    assert _bits(np.concatenate([a, b])) == _bits(whole) and _bits(pb) == _bits(pw)
    # an invalid first record leaves no state
    nan_first = m[:1].copy()
    nan_first[0, 0] = np.nan
    assert et.filter_stream(nan_first, 128)[1] is None


# ---- argument errors that need no device ------------------------------------------------------------------------------------------
def test_argument_errors_come_before_a_device(st):
    import torch
    capi = st.capi
    L = capi.lib()
    tab = (C.c_void_p * 2)(0x1000, 0x2000)
    null = (C.c_void_p * 2)(0x1000, None)

    def given(src=tab, out=tab, count=2, w=8, h=8, stats=0x3000):
        return L.stitch_dev_transfer_given_many_u8(src, out, count, w, h, stats, 1, None)

    for kw in (dict(src=None), dict(out=None), dict(stats=None), dict(count=0), dict(count=-1), dict(count=1025), dict(w=0), dict(h=-3), dict(w=65536, h=32768),
               dict(src=null), dict(out=null)):
        assert given(**kw) == capi.ERR_ARG and b"transfer_given_many" in L.stitch_last_error(), kw

    def filt(m=0x1000, count=3, keep=128, state=0x2000, has=0x3000, used=0x4000):
        return L.stitch_dev_stats_filter_f32(m, count, keep, state, has, used, None)

    for kw in (dict(m=None), dict(state=None), dict(has=None), dict(used=None), dict(count=0), dict(count=-2), dict(keep=-1), dict(keep=256)):
        assert filt(**kw) == capi.ERR_ARG and b"stats_filter" in L.stitch_last_error(), kw
    if not torch.cuda.is_available():  # and what is left needs a device
        assert given() == capi.ERR_NO_DEVICE and filt() == capi.ERR_NO_DEVICE and filt(keep=0) == capi.ERR_NO_DEVICE and filt(keep=255) == capi.ERR_NO_DEVICE


def _run4_steps():
    with open(os.path.join(GOLD, "golden.json")) as f:
        G = json.load(f)["runs"]["4"]
    with open(os.path.join(GOLD, "exposure.json")) as f:
        rec = json.load(f)["runs"]["4"]["mode1_keep_black1"]["steps"]
    return [dict(s, mosaic_src=r["mosaic_src"]) for s, r in zip(G["steps"], rec)]


def _records(seed=5, n=3):
    return _stream(np.random.default_rng(seed), n)


BAD_VALUES = ((0, np.nan), (7, np.inf), (2, -np.inf), (3, 0.0), (4, -0.5), (5, -0.0), (9, 0.0), (10, np.nan), (11, -1.0))


@pytest.mark.parametrize("mode", [1, 2])
def test_rig_options_come_and_go_without_a_device(st, mode):
    capi = st.capi
    L = capi.lib()
    rig = capi.Rig.from_steps([(384, 512)] * 4, None, _run4_steps(), exposure=mode)
    a, b = _records(5), _records(6)
    zeros = np.zeros((3, 12), np.float32)
    try:
        assert rig.exposure_smoothing() == (None, [False] * 3) and rig.fixed_exposure() is None and rig.last_used_stats().shape == (0, 3, 12)
        assert _bits(rig.exposure_state()) == _bits(zeros)
        # smoothing: the option, then a primed state, a reset that keeps the option, a clear that forgets both
        assert rig.set_exposure_smoothing(192).exposure_smoothing() == (192, [False] * 3)
        for keep in (0, 1, 255):
            assert rig.set_exposure_smoothing(keep).exposure_smoothing()[0] == keep
        for keep in (-1, 256, 2 ** 31 - 1, -2 ** 31):
            with pytest.raises(capi.StitchError) as e:
                rig.set_exposure_smoothing(keep)
            assert e.value.code == capi.ERR_ARG and rig.exposure_smoothing() == (255, [False] * 3)  # the rig stays as it was
        assert rig.prime_exposure_state(a).exposure_smoothing() == (255, [True] * 3) and _bits(rig.exposure_state()) == _bits(a)
        assert rig.prime_exposure_state(b).exposure_smoothing()[1] == [True] * 3 and _bits(rig.exposure_state()) == _bits(b)
        for j, v in BAD_VALUES:  # a record the filter would not take up is refused, and the state stays
            bad = a.copy()
            bad[1, j] = v
            with pytest.raises(capi.StitchError) as e:
                rig.prime_exposure_state(bad)
            assert e.value.code == capi.ERR_ARG and b"step 1" in L.stitch_last_error() and _bits(rig.exposure_state()) == _bits(b)
        with pytest.raises(capi.StitchError):
            rig.prime_exposure_state(a[:2])  # two records for three steps
        assert L.stitch_rig_prime_exposure_state(rig._h, None, 3) == capi.ERR_ARG and _bits(rig.exposure_state()) == _bits(b)
        assert rig.reset_exposure_state().exposure_smoothing() == (255, [False] * 3) and _bits(rig.exposure_state()) == _bits(zeros)
        rig.prime_exposure_state(a)
        assert rig.clear_exposure_smoothing().exposure_smoothing() == (None, [False] * 3)
        assert rig.prime_exposure_state(a).exposure_smoothing() == (None, [True] * 3)  # without the option a state rests
        # fixed statistics: set, replaced, refused, cleared; they leave the smoothing option and state alone
        rig.set_exposure_smoothing(64)
        assert _bits(rig.fix_exposure(b).fixed_exposure()) == _bits(b) and rig.exposure_smoothing() == (64, [True] * 3)
        assert _bits(rig.exposure_state()) == _bits(a)
        for j, v in BAD_VALUES:
            bad = a.copy()
            bad[2, j] = v
            with pytest.raises(capi.StitchError) as e:
                rig.fix_exposure(bad)
            assert e.value.code == capi.ERR_ARG and b"step 2" in L.stitch_last_error() and _bits(rig.fixed_exposure()) == _bits(b)
        with pytest.raises(capi.StitchError):
            rig.fix_exposure(np.concatenate([a, a[:1]]))  # four records for three steps
        assert L.stitch_rig_fix_exposure(rig._h, None, 3) == capi.ERR_ARG and _bits(rig.fixed_exposure()) == _bits(b)
        assert _bits(rig.fix_exposure(a).fixed_exposure()) == _bits(a)
        assert rig.clear_fixed_exposure().fixed_exposure() is None and rig.clear_fixed_exposure().fixed_exposure() is None
        assert rig.exposure_smoothing() == (64, [True] * 3) and _bits(rig.exposure_state()) == _bits(a)
        # null handles and outputs
        n = C.c_int()
        assert L.stitch_rig_set_exposure_smoothing(None, 1) == L.stitch_rig_clear_exposure_smoothing(None) == L.stitch_rig_reset_exposure_state(None) \
            == L.stitch_rig_prime_exposure_state(None, capi._p(a), 3) == L.stitch_rig_exposure_smoothing(None, None, None) \
            == L.stitch_rig_exposure_state(None, capi._p(zeros), 3) == L.stitch_rig_fix_exposure(None, capi._p(a), 3) == L.stitch_rig_clear_fixed_exposure(None) \
            == L.stitch_rig_fixed_exposure(None, None, C.byref(n)) == L.stitch_rig_last_used_stats(None, None, 0, None, None) == capi.ERR_ARG
        assert L.stitch_rig_exposure_state(rig._h, None, 3) == L.stitch_rig_exposure_state(rig._h, capi._p(zeros), 2) == capi.ERR_ARG
        assert L.stitch_rig_exposure_smoothing(rig._h, None, None) == L.stitch_rig_fixed_exposure(rig._h, None, None) \
            == L.stitch_rig_last_used_stats(rig._h, None, 0, None, None) == 0  # every output is optional
        assert rig.step_plan(0) is None  # no device was touched
    finally:
        rig.close()


def test_a_rig_without_a_transfer_refuses_every_call(st):
    capi = st.capi
    L = capi.lib()
    rig = capi.Rig.from_steps([(384, 512)] * 4, None, _run4_steps())  # mode 0
    a = _records()
    keep, n = C.c_int(7), C.c_int(7)
    try:
        calls = (lambda: L.stitch_rig_set_exposure_smoothing(rig._h, 128), lambda: L.stitch_rig_clear_exposure_smoothing(rig._h),
                 lambda: L.stitch_rig_reset_exposure_state(rig._h), lambda: L.stitch_rig_prime_exposure_state(rig._h, capi._p(a), 3),
                 lambda: L.stitch_rig_exposure_smoothing(rig._h, C.byref(keep), None), lambda: L.stitch_rig_exposure_state(rig._h, capi._p(a), 3),
                 lambda: L.stitch_rig_fix_exposure(rig._h, capi._p(a), 3), lambda: L.stitch_rig_clear_fixed_exposure(rig._h),
                 lambda: L.stitch_rig_fixed_exposure(rig._h, None, C.byref(n)), lambda: L.stitch_rig_last_used_stats(rig._h, None, 0, C.byref(n), None))
        for i, call in enumerate(calls):
            assert call() == capi.ERR_ARG and b"mode 0" in L.stitch_last_error(), i
        assert keep.value == 7 and n.value == 7
    finally:
        rig.close()
