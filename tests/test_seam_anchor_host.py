"""CPU: the host side of temporally anchored path seams (include/stitch_seam_anchor.h) -- the header compiles as C99 and the
binding's table SEAM_ANCHOR_SIGNATURES states exactly what it declares; tests/seam_anchor_ref.py's statement has the properties the
header claims, against brute force where a table can be enumerated, with anchors at both ends of int32; and every argument error
that needs no device is reported before one is needed."""
import ctypes as C
import json
import os
import re
import shlex
import subprocess

import numpy as np
import pytest

import seam_anchor_ref as sa
import seam_path_ref as sp
from test_seam_path_host import RETURNS, SCALARS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "stitch_seam_anchor.h")

FUNCTIONS = ("stitch_dev_pairs_seam_path_anchored_u8", "stitch_rig_set_seam_anchor", "stitch_rig_prime_seam_anchor", "stitch_rig_reset_seam_anchor",
             "stitch_rig_clear_seam_anchor", "stitch_rig_seam_anchor", "stitch_rig_last_seam_moved")


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
    assert sorted(capi.SEAM_ANCHOR_SIGNATURES) == sorted(want)
    others = set(capi.SIGNATURES) | set(capi.PANORAMA_SIGNATURES) | set(capi.RIG_SIGNATURES) | set(capi.EXPOSURE_SIGNATURES) \
        | set(capi.RIG_EXPOSURE_SIGNATURES) | set(capi.CALIBRATE_SIGNATURES) | set(capi.RIG_SEAMS_SIGNATURES) | set(capi.COLLAPSE_SIDES_SIGNATURES) \
        | set(capi.SRC_RUNS_SIGNATURES) | set(capi.RIG_CROP_SIGNATURES) | set(capi.RIG_FORMAT_SIGNATURES) | set(capi.RIG_MONITOR_SIGNATURES) \
        | set(capi.SEAM_PATH_SIGNATURES)
    assert not set(capi.SEAM_ANCHOR_SIGNATURES) & others
    bound = {n: (getattr(lib, n).restype, getattr(lib, n).argtypes) for n in want}  # every name is exported
    wrong = {n: (bound[n], want[n]) for n in sorted(want) if bound[n] != tuple(want[n])}
    assert not wrong, f"(bound, declared) signatures differ for: {wrong}"
    assert lib.stitch_abi_version() == 5  # the ABI version stays


def test_header_is_c99_and_its_constants(st, tmp_path):
    capi = st.capi
    cc = shlex.split(os.environ.get("CC", "cc")) + ["-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include")]
    src = tmp_path / "uses.c"
    src.write_text("\n".join(['#include "stitch_seam_anchor.h"', "void uses(void) {"] + [f"    (void)(&{n});" for n in FUNCTIONS]
                             + ["    (void)(STITCH_SEAM_ANCHOR_MAX + STITCH_SEAM_ANCHOR_PER_SET + STITCH_SEAM_ANCHOR_PER_CALL);",
                                "    (void)sizeof(stitch_seam_anchor_opts);",
                                "    { typedef char three_words[sizeof(stitch_seam_anchor_opts) == 12 ? 1 : -1]; (void)sizeof(three_words); }", "}", ""]))
    r = subprocess.run(cc + ["-fsyntax-only", str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    text = open(HEADER).read()
    got = [int(re.search(rf"#define {n} (\d+)", text).group(1)) for n in ("STITCH_SEAM_ANCHOR_MAX", "STITCH_SEAM_ANCHOR_PER_SET", "STITCH_SEAM_ANCHOR_PER_CALL")]
    assert got == [2055, 1, 2] == [capi.SEAM_ANCHOR_MAX, capi.SEAM_ANCHOR_PER_SET, capi.SEAM_ANCHOR_PER_CALL] and sa.ANCHOR_MAX == 2055
    assert 2040 + 2055 < sp.WRONG  # one pixel on the wrong side costs more than any crossing plus any temporal penalty
    assert C.sizeof(capi.SeamAnchorOpts) == 12 and [f[0] for f in capi.SeamAnchorOpts._fields_] == ["weight", "cap", "policy"]


# ---- the statement and its properties ------------------------------------------------------------------------------------------------------
def _table(rng, trial, h, w):
    if trial % 3 == 0:  # raw costs, many ties
        return rng.integers(0, 4, (h, w + 1)).astype(np.int64)
    a, b = rng.integers(0, 256, (2, 3, h, w)).astype(np.uint8)
    A, B = rng.integers(0, 2, (2, h, w)).astype(np.uint8)
    return sp.cost(a, b, A, B, trial & 1, int(rng.integers(0, 3)))


def _options(rng):
    w = int(rng.integers(1, 33))
    return w, int(rng.integers(1, sa.ANCHOR_MAX // w + 1))


def test_properties_on_random_tables():
    rng = np.random.default_rng(22)
    for trial in range(300):
        h, w = int(rng.integers(1, 9)), int(rng.integers(1, 13))
        K = int(rng.integers(1, 4))
        c = _table(rng, trial, h, w)
        wt, T = _options(rng)
        free, free_cost = sp.dp_path(c, K)
        r = rng.integers(-3, w + 4, h)
        # (a) weight 0 is the unanchored finder, and so is no anchor
        path, D, moved = sa.anchored_path(c, K, r, 0, T)
        assert (path.tolist(), D) == (free.tolist(), free_cost) and moved == sa.moved_of(free, r, T)
        assert [x.tolist() if hasattr(x, "tolist") else x for x in sa.anchored_path(c, K, None, wt, T)] == [free.tolist(), free_cost, 0]
        # (b) the anchor that is the unanchored path returns it, at the same cost, with moved = 0
        path, D, moved = sa.anchored_path(c, K, free, wt, T)
        assert (path.tolist(), D, moved) == (free.tolist(), free_cost, 0)
        # (c) an anchor at least T away from every column on every row: the unanchored path, D + ch * w * T
        for far in (np.full(h, w + T), np.full(h, -T), np.where(rng.integers(0, 2, h) == 1, w + T + 5, -T - 7)):
            path, D, moved = sa.anchored_path(c, K, far, wt, T)
            assert (path.tolist(), D, moved) == (free.tolist(), free_cost + h * wt * T, h * T)
        # (d) and D = (the path's cost under c) + w * moved, with moved no larger than the unanchored path's
        path, D, moved = sa.anchored_path(c, K, r, wt, T)
        assert D == sp.path_cost(c, path) + wt * moved and moved <= sa.moved_of(free, r, T)
        assert all(abs(int(path[y]) - int(path[y - 1])) <= K for y in range(1, h)) and path.min() >= 0 and path.max() <= w
        if (w + 1) ** h <= 4096:  # small enough to enumerate
            assert D == sa.brute_force(c, K, r, wt, T)


def test_brute_force_on_small_tables():
    rng = np.random.default_rng(23)
    for trial in range(120):
        h, w = int(rng.integers(1, 5)), int(rng.integers(1, 5))
        K = int(rng.integers(1, 4))
        c = _table(rng, trial, h, w)
        wt, T = _options(rng)
        r = rng.integers(-2, w + 3, h)
        path, D, moved = sa.anchored_path(c, K, r, wt, T)
        assert D == sa.brute_force(c, K, r, wt, T) == sp.path_cost(c, path) + wt * moved, (trial, c, r)


def test_anchors_at_the_ends_of_int32():
    rng = np.random.default_rng(24)
    c = rng.integers(0, 2041, (5, 9)).astype(np.int64)
    free, free_cost = sp.dp_path(c, 2)
    for r in ([sa.INT32_MIN] * 5, [sa.INT32_MAX] * 5, [sa.INT32_MIN, sa.INT32_MAX, 0, sa.INT32_MAX, sa.INT32_MIN]):
        pen = sa.penalty(9, r, 3, 685)
        for y, v in enumerate(r):
            assert pen[y].tolist() == [3 * min(abs(s - v), 685) for s in range(9)]  # in Python integers
        far = [y for y, v in enumerate(r) if v != 0]
        assert all((pen[y] == 2055).all() for y in far)
    path, D, moved = sa.anchored_path(c, 2, [sa.INT32_MAX] * 5, 3, 685)
    assert (path.tolist(), D, moved) == (free.tolist(), free_cost + 5 * 2055, 5 * 685)
    path, D, moved = sa.anchored_path(c, 2, [sa.INT32_MIN] * 5, 2055, 1)
    assert (path.tolist(), D, moved) == (free.tolist(), free_cost + 5 * 2055, 5)


def test_a_flat_table_tracks_the_anchor_within_the_step_bound():
    """Every state of c ties: the temporal term alone decides, and a step bound that lets the path follow the anchor makes it the anchor."""
    r, c = [2, 2, 7, 7, 0], np.zeros((5, 8), np.int64)
    path, D, moved = sa.anchored_path(c, 2, r, 1, 64)
    assert all(abs(int(path[y]) - int(path[y - 1])) <= 2 for y in range(1, 5))
    assert D == moved == sa.brute_force(c, 2, r, 1, 64) > 0
    path, D, moved = sa.anchored_path(c, 8, r, 1, 64)
    assert (path.tolist(), D, moved) == (r, 0, 0)


# ---- argument errors that need no device ------------------------------------------------------------------------------------------------------
BAD_OPTS = ((1, 2056), (2056, 1), (8, 257), (-1, 4), (-2 ** 31, 1), (4, 0), (4, -1), (2 ** 31 - 1, 2 ** 31 - 1))
GOOD_OPTS = ((0, 1), (0, 2 ** 31 - 1), (1, 2055), (2055, 1), (32, 64), (5, 411))


def test_argument_errors_come_before_a_device(st):
    import torch
    capi = st.capi
    L = capi.lib()
    arr = (capi.PairDesc * 2)()
    for d in arr:
        d.frame, d.fw, d.fh, d.mosaic, d.mw, d.mh, d.out = 0x1000, 8, 8, 0x2000, 8, 8, 0x5000
        d.p = capi._map8([1, 0, 0, 0, 0, 1, 0, 0])
    cov = (C.c_void_p * 2)(0x3000, 0x3000)
    br = (C.c_int32 * 2)(0, 1)
    anchors = (C.c_void_p * 2)(0x7000, None)  # a null entry is no error: that pair is unanchored
    good = capi.SeamPathOpts(2, 8)

    def find(n=2, cw=8, ch=8, opts=good, a=anchors, ao=(32, 64), paths=0x4000, costs=0x6000, moved=0x8000):
        o = None if ao is None else C.byref(capi.SeamAnchorOpts(ao[0], ao[1], 77))  # the policy is ignored
        return L.stitch_dev_pairs_seam_path_anchored_u8(arr, n, cw, ch, cov, cov, br, C.byref(opts), a, o, paths, costs, moved, None)

    for kw in (dict(a=None), dict(ao=None), dict(moved=None), dict(paths=None), dict(costs=None)):
        assert find(**kw) == capi.ERR_ARG, kw
    for ao in BAD_OPTS:
        assert find(ao=ao) == capi.ERR_ARG and b"pairs_seam_path_anchored" in L.stitch_last_error(), ao
    # what the unanchored call refuses stays refused
    for kw in (dict(n=0), dict(n=65536), dict(cw=8193), dict(ch=65536), dict(opts=capi.SeamPathOpts(9, 8)), dict(opts=capi.SeamPathOpts(2, 65))):
        assert find(**kw) == capi.ERR_ARG, kw
    if not torch.cuda.is_available():  # and what is left needs a device
        for ao in GOOD_OPTS:
            assert find(ao=ao) == capi.ERR_NO_DEVICE, ao


def test_rig_anchor_options_come_and_go_without_a_device(st):
    capi = st.capi
    L = capi.lib()
    with open(os.path.join(ROOT, "tests", "golden", "golden.json")) as f:
        steps = json.load(f)["runs"]["4"]["steps"]
    heights = [s["ch"] for s in steps]
    rig = capi.Rig.from_steps([(384, 512)] * 4, None, steps)
    try:
        assert rig.seam_anchor() == (None, False)
        assert rig.set_seam_anchor(32, 64).seam_anchor() == ((32, 64, "set"), False)  # without a mode the options rest
        assert rig.set_seam_anchor(5, 411, "call").seam_anchor() == ((5, 411, "call"), False) and rig.seam_paths is None
        for w, T in GOOD_OPTS:
            assert rig.set_seam_anchor(w, T, "set").seam_anchor() == ((w, T, "set"), False)
        rig.set_seam_anchor(5, 411, "call")
        for w, T in BAD_OPTS:
            for policy in ("set", "call"):
                with pytest.raises(capi.StitchError) as e:
                    rig.set_seam_anchor(w, T, policy)
                assert e.value.code == capi.ERR_ARG and rig.seam_anchor() == ((5, 411, "call"), False)  # the rig stays as it was
        for policy in (0, 3, -1):
            with pytest.raises(capi.StitchError) as e:
                rig.set_seam_anchor(1, 1, policy)
            assert e.value.code == capi.ERR_ARG and rig.seam_anchor() == ((5, 411, "call"), False)
        # priming: one path per step, any integers
        assert rig.prime_seam_anchor([np.full(h, -2 ** 31) for h in heights]).seam_anchor() == ((5, 411, "call"), True)
        assert rig.reset_seam_anchor().seam_anchor() == ((5, 411, "call"), False)  # the options stay
        with pytest.raises(capi.StitchError):
            rig.prime_seam_anchor([np.zeros(h, np.int32) for h in heights[:2]])  # two paths for three steps
        with pytest.raises(ValueError):
            rig.prime_seam_anchor([np.zeros(5, np.int32)] * 3)  # the wrong height
        assert L.stitch_rig_prime_seam_anchor(rig._h, None, 3) == capi.ERR_ARG
        assert L.stitch_rig_prime_seam_anchor(rig._h, (C.c_void_p * 3)(0x1000, None, 0x1000), 3) == capi.ERR_ARG and rig.seam_anchor()[1] is False
        rig.prime_seam_anchor([np.arange(h) for h in heights])
        assert rig.set_seam_paths().clear_seam_paths().seam_anchor() == ((5, 411, "call"), False)  # clearing the paths forgets the anchor
        rig.prime_seam_anchor([np.arange(h) for h in heights])
        assert rig.clear_seam_anchor().seam_anchor() == (None, False) and rig.clear_seam_anchor().seam_anchor() == (None, False)
        # null handles and outputs
        o = capi.SeamAnchorOpts(1, 1, 1)
        assert L.stitch_rig_set_seam_anchor(None, C.byref(o)) == L.stitch_rig_set_seam_anchor(rig._h, None) == L.stitch_rig_prime_seam_anchor(None, None, 0) \
            == L.stitch_rig_reset_seam_anchor(None) == L.stitch_rig_clear_seam_anchor(None) == L.stitch_rig_seam_anchor(None, None, None) == capi.ERR_ARG
        moved = C.c_uint64()
        assert L.stitch_rig_last_seam_moved(None, 0, 0, C.byref(moved)) == L.stitch_rig_last_seam_moved(rig._h, 0, 0, None) == capi.ERR_ARG
        assert L.stitch_rig_last_seam_moved(rig._h, 0, 0, C.byref(moved)) == capi.ERR_ARG  # no replay along paths yet
        assert L.stitch_rig_seam_anchor(rig._h, None, None) == 0  # both outputs are optional
        assert rig.step_plan(0) is None  # no device was touched
    finally:
        rig.close()
    zero = capi.Rig.from_steps([(64, 48)], 0, [])  # nothing to anchor, and the calls succeed
    assert zero.set_seam_anchor(1, 1).prime_seam_anchor([]).reset_seam_anchor().clear_seam_anchor().seam_anchor() == (None, False)
    zero.close()
