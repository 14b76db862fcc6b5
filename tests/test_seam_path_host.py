"""CPU: the host side of path seams (include/stitch_seam_path.h) -- the header compiles as C99 and the binding's table
SEAM_PATH_SIGNATURES states exactly what it declares; every argument error that needs no plan is reported before a device is
needed; tests/seam_path_ref.py's blend_with_mask on the vertical step is the oracle's blend, bit for bit; and its dynamic programme
against brute force on small canvases, with hand-made ties for each tie rule."""
import ctypes as C
import os
import re
import shlex
import subprocess

import numpy as np
import pytest

import seam_path_ref as sp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "stitch_seam_path.h")

FUNCTIONS = ("stitch_seam_path_opts_default", "stitch_plan_create_masked", "stitch_plan_is_masked", "stitch_dev_pairs_pathed_u8",
             "stitch_dev_pairs_pathed_f32", "stitch_dev_pairs_seam_path_u8", "stitch_rig_set_seam_paths", "stitch_rig_fix_seam_paths",
             "stitch_rig_clear_seam_paths", "stitch_rig_seam_paths", "stitch_rig_last_seam_paths")


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


def test_signature_table_states_the_header(st):
    capi = st.capi
    want, lib = _declared(), capi.lib()
    assert sorted(want) == sorted(FUNCTIONS) == sorted(set(re.findall(r"\b(stitch_[a-z0-9_]+)\s*\(", _header_text())))
    assert sorted(capi.SEAM_PATH_SIGNATURES) == sorted(want)
    others = set(capi.SIGNATURES) | set(capi.PANORAMA_SIGNATURES) | set(capi.RIG_SIGNATURES) | set(capi.EXPOSURE_SIGNATURES) \
        | set(capi.RIG_EXPOSURE_SIGNATURES) | set(capi.CALIBRATE_SIGNATURES) | set(capi.RIG_SEAMS_SIGNATURES) | set(capi.COLLAPSE_SIDES_SIGNATURES) \
        | set(capi.SRC_RUNS_SIGNATURES) | set(capi.RIG_CROP_SIGNATURES) | set(capi.RIG_FORMAT_SIGNATURES) | set(capi.RIG_MONITOR_SIGNATURES)
    assert not set(capi.SEAM_PATH_SIGNATURES) & others
    bound = {n: (getattr(lib, n).restype, getattr(lib, n).argtypes) for n in want}  # every name is exported
    wrong = {n: (bound[n], want[n]) for n in sorted(want) if bound[n] != tuple(want[n])}
    assert not wrong, f"(bound, declared) signatures differ for: {wrong}"
    assert lib.stitch_abi_version() == 5  # the ABI version stays


def test_header_is_c99(st, tmp_path):
    cc = shlex.split(os.environ.get("CC", "cc")) + ["-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include")]
    src = tmp_path / "uses.c"
    src.write_text("\n".join(['#include "stitch_seam_path.h"', "void uses(void) {"] + [f"    (void)(&{n});" for n in FUNCTIONS]
                             + ["    (void)(STITCH_SEAM_PATH_MAX_STEP + STITCH_SEAM_PATH_MAX_MARGIN + STITCH_SEAM_PATH_MAX_WIDTH);",
                                "    (void)sizeof(stitch_seam_path_opts);", "}", ""]))
    r = subprocess.run(cc + ["-fsyntax-only", str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_defaults_and_limits(st):
    capi = st.capi
    o = capi.SeamPathOpts(7, 7)
    capi.lib().stitch_seam_path_opts_default(C.byref(o))
    assert (o.max_step, o.margin) == (2, 8) == (capi.SeamPathOpts().max_step, capi.SeamPathOpts().margin)
    capi.lib().stitch_seam_path_opts_default(None)  # a null pointer is ignored
    text = open(HEADER).read()
    assert [int(re.search(rf"#define {n} (\d+)", text).group(1)) for n in ("STITCH_SEAM_PATH_MAX_STEP", "STITCH_SEAM_PATH_MAX_MARGIN", "STITCH_SEAM_PATH_MAX_WIDTH")] \
        == [8, 64, 8192]


def test_argument_errors_come_before_a_device(st):
    import torch
    capi = st.capi
    L = capi.lib()

    def pairs(n=1, **kw):
        arr = (capi.PairDesc * n)()
        for d in arr:
            d.frame, d.fw, d.fh, d.mosaic, d.mw, d.mh, d.out = 0x1000, 8, 8, 0x2000, 8, 8, 0x5000
            d.p = capi._map8([1, 0, 0, 0, 0, 1, 0, 0])
            for k, v in kw.items():
                setattr(d, k, v)
        return arr

    cov = (C.c_void_p * 2)(0x3000, 0x3000)
    br = (C.c_int32 * 2)(0, 1)
    good = capi.SeamPathOpts(2, 8)

    def find(p=None, n=1, cw=8, ch=8, a=cov, b=cov, branches=br, opts=good, paths=0x4000, costs=0x6000):
        return L.stitch_dev_pairs_seam_path_u8(pairs() if p is None else p, n, cw, ch, a, b, branches, C.byref(opts) if opts is not None else None, paths, costs, None)

    # a null pointer, each in turn
    assert L.stitch_dev_pairs_seam_path_u8(None, 1, 8, 8, cov, cov, br, C.byref(good), 0x4000, 0x6000, None) == capi.ERR_ARG
    for kw in (dict(a=None), dict(b=None), dict(branches=None), dict(paths=None), dict(costs=None)):
        assert find(**kw) == capi.ERR_ARG, kw
    assert b"pairs_seam_path" in L.stitch_last_error()
    # max_step outside 1 .. 8, margin outside 0 .. 64
    for k in (0, -1, 9, 2 ** 31 - 1):
        assert find(opts=capi.SeamPathOpts(k, 8)) == capi.ERR_ARG, k
    for m in (-1, 65, -2 ** 31):
        assert find(opts=capi.SeamPathOpts(2, m)) == capi.ERR_ARG, m
    # the canvas: cw = 8193 is refused, and sizes below 1, and more rows than the cost's bound allows
    for cw, ch in ((8193, 4), (0, 8), (8, 0), (-1, 8), (8, 65536)):
        assert find(cw=cw, ch=ch) == capi.ERR_ARG, (cw, ch)
    # n out of range
    for n in (0, -1, 65536):
        assert find(n=n) == capi.ERR_ARG, n
    # a pair without a frame, a mosaic, a mask, or with a bad size or branch
    for kw in (dict(frame=None), dict(mosaic=None), dict(fw=0), dict(fh=-1), dict(mw=0), dict(mh=0)):
        assert find(p=pairs(2, **kw), n=2) == capi.ERR_ARG, kw
    assert find(p=pairs(2), n=2, a=(C.c_void_p * 2)(0x3000, None)) == find(p=pairs(2), n=2, b=(C.c_void_p * 2)(None, 0x3000)) == capi.ERR_ARG
    for bad in (2, -1):
        assert find(p=pairs(2), n=2, branches=(C.c_int32 * 2)(0, bad)) == capi.ERR_ARG
    # the plan calls: null arguments need no plan
    assert L.stitch_plan_is_masked(None) == capi.ERR_ARG
    for fn in (L.stitch_dev_pairs_pathed_u8, L.stitch_dev_pairs_pathed_f32):
        assert fn(None, pairs(), 1, cov, br, None) == capi.ERR_ARG
    h = C.c_void_p()
    o = capi.BlendOpts()
    assert L.stitch_plan_create_masked(64, 64, C.byref(o), 1, None) == capi.ERR_ARG
    for max_pairs in (0, 17):
        assert L.stitch_plan_create_masked(64, 64, C.byref(o), max_pairs, C.byref(h)) == capi.ERR_ARG and not h.value
    if not torch.cuda.is_available():  # and what is left needs one
        assert find() == find(opts=None) == find(cw=8192, ch=4) == find(opts=capi.SeamPathOpts(8, 64)) == find(opts=capi.SeamPathOpts(1, 0)) == capi.ERR_NO_DEVICE
        assert L.stitch_plan_create_masked(64, 64, C.byref(o), 1, C.byref(h)) == capi.ERR_NO_DEVICE and not h.value
        with pytest.raises(capi.StitchError) as e:
            capi.Plan(64, 64, masked=True)
        assert e.value.code == capi.ERR_NO_DEVICE


def test_rig_modes_come_and_go_without_a_device(st):
    import json
    capi = st.capi
    L = capi.lib()
    with open(os.path.join(ROOT, "tests", "golden", "golden.json")) as f:
        steps = json.load(f)["runs"]["4"]["steps"]
    rig = capi.Rig.from_steps([(384, 512)] * 4, None, steps)
    try:
        assert rig.n_steps == 3 and rig.seam_paths is None
        assert rig.set_seam_paths().seam_paths == ("found", 2, 8) and rig.set_seam_paths(8, 64).seam_paths == ("found", 8, 64)
        for K, m in ((0, 8), (9, 8), (2, -1), (2, 65)):
            with pytest.raises(capi.StitchError) as e:
                rig.set_seam_paths(K, m)
            assert e.value.code == capi.ERR_ARG and rig.seam_paths == ("found", 8, 64)  # the rig stays as it was
        heights = [s["ch"] for s in steps]
        assert rig.fix_seam_paths([np.arange(h) for h in heights]).seam_paths == ("fixed",)
        with pytest.raises(capi.StitchError):
            rig.fix_seam_paths([np.zeros(h, np.int32) for h in heights[:2]])  # two paths for three steps
        with pytest.raises(ValueError):
            rig.fix_seam_paths([np.zeros(5, np.int32)] * 3)  # the wrong height
        assert L.stitch_rig_fix_seam_paths(rig._h, None, 3) == capi.ERR_ARG
        assert L.stitch_rig_fix_seam_paths(rig._h, (C.c_void_p * 3)(0x1000, None, 0x1000), 3) == capi.ERR_ARG and rig.seam_paths == ("fixed",)
        assert L.stitch_rig_last_seam_paths(rig._h, 0, 0, None, 0, None) == capi.ERR_ARG  # no replay along paths yet
        assert rig.clear_seam_paths().seam_paths is None and rig.clear_seam_paths().seam_paths is None
        assert L.stitch_rig_set_seam_paths(None, None) == L.stitch_rig_clear_seam_paths(None) == L.stitch_rig_seam_paths(None, None, None) \
            == L.stitch_rig_fix_seam_paths(None, None, 0) == L.stitch_rig_last_seam_paths(None, 0, 0, None, 0, None) == capi.ERR_ARG
        assert L.stitch_rig_seam_paths(rig._h, None, None) == 0  # both outputs are optional
        assert rig.step_plan(0) is None  # no device was touched
    finally:
        rig.close()
    zero = capi.Rig.from_steps([(64, 48)], 0, [])  # nothing to blend, and the calls succeed
    assert zero.set_seam_paths().seam_paths == ("found", 2, 8) and zero.fix_seam_paths([]).seam_paths == ("fixed",) and zero.clear_seam_paths().seam_paths is None
    zero.close()


# ---- blend_with_mask on the vertical step is the oracle's blend ---------------------------------------------------------------------
def _canvases(oracle, cw, ch, dtype, branch):
    """Two canvases whose scan yields the wanted branch: a covers the left (branch 0: ratio < ov) or the right part, b the rest + overlap."""
    fa, fb = oracle.synth(cw, ch, 3, dtype), oracle.synth(cw, ch, 4, dtype)
    a, b = np.zeros_like(fa), np.zeros_like(fb)
    cut = max(1, cw // 3)
    if branch == 0:
        a[:, :, :cw - cut // 2] = np.maximum(fa[:, :, :cw - cut // 2], 1)
        b[:, :, cut:] = np.maximum(fb[:, :, cut:], 1)
    else:
        a[:, :, cut:] = np.maximum(fa[:, :, cut:], 1)
        b[:, :, :cw - cut // 2] = np.maximum(fb[:, :, :cw - cut // 2], 1)
    return a, b


@pytest.mark.parametrize("blur_kind,seam_rule", [(0, 0), (0, 1), (1, 0), (1, 1)])
@pytest.mark.parametrize("size", [(3, 2), (97, 61), (300, 70), (301, 71)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_blend_with_mask_on_the_vertical_step_is_the_oracle(oracle, size, blur_kind, seam_rule):
    cw, ch = size
    opts = sp.opts_for(oracle, cw, ch, blur_kind, seam_rule)
    seen = set()
    for dtype in (np.uint8, np.float32):
        for want in (0, 1):
            a, b = _canvases(oracle, cw, ch, dtype, want)
            res = oracle.blend(a, b, opts, want_f32=True) if dtype == np.uint8 else oracle.blend(a, b, opts)
            rc, ref, seam = res[:3]
            assert rc == 0
            seen.add(seam.branch)
            path = sp.constant_path(seam, opts["seam_rule"], ch)
            # the path's mask is the step itself
            x = np.arange(cw)
            thr = float(seam.ov) if opts["seam_rule"] == 0 else seam.sum_ov_x / seam.n_ov
            step = (x < thr) if seam.branch == 0 else (x >= seam.start)
            mask = sp.mask_from_path(path, seam.branch, cw)
            assert np.array_equal(mask, np.broadcast_to(step.astype(np.float32), (ch, cw)))
            e = sp.blend_with_mask(oracle, a, b, mask, opts)
            if dtype == np.uint8:
                assert np.array_equal(e.view(np.uint32), res[3].view(np.uint32)) and np.array_equal(e.astype(np.uint8), ref)
            else:
                assert np.array_equal(e.view(np.uint32), ref.view(np.uint32))
    assert seen == {0, 1} or cw < 8  # both branches, wherever the canvas is wide enough to make either


# ---- the dynamic programme ------------------------------------------------------------------------------------------------------------
def test_dp_against_brute_force_on_small_canvases():
    rng = np.random.default_rng(20)
    for trial in range(200):
        h, w = int(rng.integers(1, 5)), int(rng.integers(1, 5))
        K = int(rng.integers(1, 4))
        kind = trial % 3
        if kind == 0:  # raw costs, many ties
            c = rng.integers(0, 4, (h, w + 1)).astype(np.int64)
        else:  # costs of random canvases and masks
            a, b = rng.integers(0, 256, (2, 3, h, w)).astype(np.uint8)
            A, B = rng.integers(0, 2, (2, h, w)).astype(np.uint8)
            c = sp.cost(a, b, A, B, trial & 1, int(rng.integers(0, 3)))
        path, total = sp.dp_path(c, K)
        assert total == sp.brute_force(c, K) == sp.path_cost(c, path), (trial, c)
        assert all(abs(int(path[y]) - int(path[y - 1])) <= K for y in range(1, h)) and path.min() >= 0 and path.max() <= w


def test_dp_tie_rules_by_hand():
    # the end: all final states tie -> the smallest s
    assert sp.dp_path(np.zeros((1, 5), np.int64), 2)[0].tolist() == [0]
    # the predecessor: the smallest |t - s| -- row 1 forces s = 2; row 0 ties at t = 0, 2 (distance 2, 0) -> 2
    c = np.array([[0, 5, 0, 5, 5], [9, 9, 0, 9, 9]], np.int64)
    assert sp.dp_path(c, 2)[0].tolist() == [2, 2]
    # ... then the smaller t -- row 0 ties at t = 1 and t = 3, both one step from s = 2 -> 1
    c = np.array([[5, 0, 5, 0, 5], [9, 9, 0, 9, 9]], np.int64)
    assert sp.dp_path(c, 2)[0].tolist() == [1, 2]
    # a nearer, larger t beats a farther, smaller one: t = 3 (distance 1) against t = 0 (distance 2)
    c = np.array([[0, 5, 5, 0, 5], [9, 9, 0, 9, 9]], np.int64)
    assert sp.dp_path(c, 2)[0].tolist() == [3, 2]
    # the step bound holds: the cheap state of row 0 is out of reach with K = 1
    c = np.array([[0, 7, 7, 7, 3], [9, 9, 9, 9, 0]], np.int64)
    path, total = sp.dp_path(c, 1)
    assert (path.tolist(), total) == ([4, 4], 3) and sp.dp_path(c, 4)[1] == 0


def test_cost_by_hand():
    # one row, cw = 4: A covers 0 .. 2, B covers 1 .. 3, no margin, branch 0: L = B & ~A = {3}, R = A & ~B = {0}
    a = np.zeros((3, 1, 4), np.uint8)
    b = np.zeros((3, 1, 4), np.uint8)
    a[:, 0, 1], b[:, 0, 1] = 10, 12   # d = |40 - 48| = 8
    a[:, 0, 2], b[:, 0, 2] = 255, 0   # d = 1020
    A, B = np.array([[1, 1, 1, 0]], np.uint8), np.array([[0, 1, 1, 1]], np.uint8)
    c = sp.cost(a, b, A, B, 0, 0)
    # s:            0                1              2                  3                   4
    assert c.tolist() == [[4096 * 1 + 0, 4096 * 0 + 8, 0 + 8 + 1020, 0 + 1020 + 0, 4096 * 1 + 0]]
    # branch 1 swaps the sides: L = {0}, R = {3}
    assert sp.cost(a, b, A, B, 1, 0).tolist() == [[4096 * 1 + 0, 4096 * 2 + 8, 4096 * 2 + 1028, 4096 * 2 + 1020, 4096 * 1]]
    # a margin of 1 erodes both masks from their open ends: A' = {0, 1}, B' = {2, 3}; L = B & ~A' = {2, 3}, R = A & ~B' = {0, 1}
    assert sp.cost(a, b, A, B, 0, 1).tolist() == [[4096 * 2, 4096 * 1 + 8, 0 + 1028, 4096 * 1 + 1020, 4096 * 2]]
