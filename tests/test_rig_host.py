"""CPU: the host side of a calibrated rig (include/stitch_rig.h) -- the header compiles as C99, the library exports exactly what it
declares, the binding's third signature table and the stitch_rig_opts mirror state what it says -- and stitch_rig_create, which is
host arithmetic only: it accepts the reference's recorded runs (tests/golden/golden.json, tests/golden/chains.json), reports
their recorded final shape, and refuses a description whose recorded canvas is not the one its forward map gives."""
import ctypes as C
import json
import math
import os
import re
import shlex
import subprocess

import numpy as np
import pytest

import chain_sets

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
HEADER = os.path.join(ROOT, "include", "stitch_rig.h")

RIG_FUNCTIONS = ("stitch_rig_opts_default", "stitch_rig_create", "stitch_rig_from_panorama", "stitch_rig_info", "stitch_rig_step_plan",
                 "stitch_dev_rig_stitch_u8", "stitch_rig_destroy", "stitch_dev_project_many_u8", "stitch_dev_finish_many_u8")


# ---- the header ------------------------------------------------------------------------------------------------------------
def _header_text():
    return re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)


SCALARS = {"int": C.c_int, "int32_t": C.c_int, "float": C.c_float, "double": C.c_double, "size_t": C.c_size_t}
RETURNS = {"int": C.c_int, "void": None, "const void *": C.c_void_p, "const stitch_plan *": C.c_void_p}


def _declared():
    """{name: (restype, argtypes)} of every prototype, by the binding's rules (tests/test_capi_abi.py, tests/test_panorama_host.py)."""
    sigs = {}
    for ret, name, params in re.findall(r"((?:const\s+)?\w+\s*\*?)\s*\b(stitch_\w+)\s*\(([^()]*)\)\s*;", _header_text()):
        prms = [] if params.strip() == "void" else [" ".join(p.split()) for p in params.split(",")]
        args = [C.c_void_p if ("*" in p or "[" in p) else SCALARS[" ".join(p.split()[:-1])] for p in prms]
        sigs[name] = (RETURNS[" ".join(ret.replace("*", " *").split())], args)
    return sigs


def test_signature_table_states_the_header(st):
    capi = st.capi
    want, lib = _declared(), capi.lib()
    assert sorted(want) == sorted(RIG_FUNCTIONS) == sorted(set(re.findall(r"\b(stitch_[a-z0-9_]+)\s*\(", _header_text())))
    assert sorted(capi.RIG_SIGNATURES) == sorted(want)
    assert not set(capi.RIG_SIGNATURES) & (set(capi.SIGNATURES) | set(capi.PANORAMA_SIGNATURES))
    bound = {n: (getattr(lib, n).restype, getattr(lib, n).argtypes) for n in want}
    wrong = {n: (bound[n], want[n]) for n in sorted(want) if bound[n] != tuple(want[n])}
    assert not wrong, f"(bound, declared) signatures differ for: {wrong}"
    assert lib.stitch_abi_version() == 5


def test_header_is_c99_and_the_mirror_matches(st, tmp_path):
    capi = st.capi
    cc = shlex.split(os.environ.get("CC", "cc")) + ["-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include")]
    src = tmp_path / "uses.c"
    src.write_text("\n".join(['#include "stitch_rig.h"', "void uses(void) {"] + [f"    (void)(&{n});" for n in RIG_FUNCTIONS]
                             + ["    (void)sizeof(stitch_rig_opts);", "}", ""]))
    r = subprocess.run(cc + ["-fsyntax-only", str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    m = capi.RigOpts
    have = {"sizeof": C.sizeof(m)}
    have.update({f[0]: getattr(m, f[0]).offset for f in m._fields_})
    prints = [f'    printf("{f} %zu\\n", ' + ("sizeof(stitch_rig_opts));" if f == "sizeof" else f"offsetof(stitch_rig_opts, {f}));") for f in have]
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text("\n".join(["#include <stddef.h>", "#include <stdio.h>", '#include "stitch_rig.h"', "int main(void) {"] + prints + ["    return 0;", "}", ""]))
    r = subprocess.run(cc + ["-o", str(exe), str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    want = {f: int(v) for f, v in (line.split() for line in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines())}
    assert have == want, f"(mirror, header) sizes and offsets differ: {have} / {want}"
    body = re.search(r"typedef struct \w+\s*\{([^{}]*)\}\s*stitch_rig_opts\s*;", _header_text()).group(1)
    assert sum(len(d.split(",")) for d in body.split(";") if d.strip()) == len(m._fields_)


def test_defaults_and_null_handles(st):
    capi, L = st.capi, st.capi.lib()
    o = capi.RigOpts()
    L.stitch_rig_opts_default(C.byref(o))
    assert (o.blend, o.fov_deg, o.finish, o.num, o.den, o.max_sets) == (None, 15.0, 1, 19.0, 20.0, 16)
    L.stitch_rig_opts_default(None)
    L.stitch_rig_destroy(None)
    assert L.stitch_rig_info(None, None, None, None, None, None) == capi.ERR_ARG and L.stitch_last_error()
    assert L.stitch_rig_step_plan(None, 0) is None


# ---- creation from the reference's recorded runs -----------------------------------------------------------------------------
def _golden_run(name):
    with open(os.path.join(GOLD, "golden.json")) as f:
        run = json.load(f)["runs"][name]
    sizes = [(run["steps"][0]["fw"], run["steps"][0]["fh"])] * int(name)  # the committed frames are of one size
    return sizes, run["steps"][0]["start"], run["steps"], run["final_shape"]


def _chain_set(name):
    """A chains.json set in the step dicts' spelling: the warped frame is `dstIndex` there."""
    G = chain_sets.chains()[name]
    sizes = [(f["shape"][2], f["shape"][1]) for f in G["frames"]]
    steps = [dict(s, src=s["dstIndex"], mosaic_src=s["srcIndex"]) for s in G["steps"]]
    return sizes, G["start"], steps, G["final_shape"]


RECORDED = [("golden", "4"), ("golden", "2")] + [("chains", n) for n in sorted(chain_sets.chains())
                                                if all(all(k in s for k in ("p", "p_fwd", "cw", "ch", "offx", "offy", "ox", "oy")) for s in chain_sets.chains()[n]["steps"])]


def _recorded(kind, name):
    return _golden_run(name) if kind == "golden" else _chain_set(name)


def test_every_recorded_chain_set_is_usable():
    assert [n for k, n in RECORDED if k == "chains"] == sorted(chain_sets.chains()) and len(RECORDED) == 6


@pytest.mark.parametrize("kind,name", RECORDED)
def test_create_from_recorded_runs(st, kind, name):
    """No device is touched: the canvases replayed from the forward maps are the recorded ones, bit for bit, step by step."""
    sizes, start, steps, final_shape = _recorded(kind, name)
    rig = st.capi.Rig.from_steps(sizes, start, steps)
    assert [3, rig.height, rig.width] == final_shape
    assert (rig.n_frames, rig.n_steps, rig.max_sets) == (len(sizes), len(steps), 16)
    assert all(rig.step_plan(k) is None for k in range(-1, len(steps) + 1))  # no workspace before the first stitch call
    rig.close()
    rig = st.capi.Rig.from_steps(sizes, start, steps, max_sets=3, finish=False)
    assert rig.max_sets == 3
    rig.close()
    rig.close()


def test_zero_steps(st):
    rig = st.capi.Rig.from_steps([(64, 48), (50, 37)], 1, [])
    assert (rig.width, rig.height, rig.n_frames, rig.n_steps) == (50, 37, 2, 0)


def _create(capi, sizes, start, arr, n_steps, max_sets=16, n=None):
    wh = np.ascontiguousarray(np.array(sizes, np.int32).reshape(-1, 2))
    o, h = capi.RigOpts(), C.c_void_p(0xdead)
    capi.lib().stitch_rig_opts_default(C.byref(o))
    o.max_sets = max_sets
    rc = capi.lib().stitch_rig_create(wh.ctypes.data_as(C.c_void_p), len(sizes) if n is None else n, start, arr, n_steps, C.byref(o), C.byref(h))
    return rc, h


def test_rejections(st):
    capi = st.capi
    sizes, start, steps, _ = _golden_run("4")

    def refused(what, sizes_=sizes, start_=start, max_sets=16, n=None, **change):
        s2 = [dict(s) for s in steps]
        for key, (k, v) in change.items():
            s2[k][key] = v
        _, arr = capi.rig_steps(s2, start_)
        rc, h = _create(capi, sizes_, start_, arr, len(s2), max_sets, n)
        text = capi.lib().stitch_last_error().decode()
        assert rc == capi.ERR_ARG and h.value is None and text.startswith("rig"), f"{what}: rc {rc}, handle {h.value}, '{text}'"
        return text

    rc, h = _create(capi, sizes, start, capi.rig_steps(steps)[1], len(steps))
    assert rc == 0 and h.value
    capi.lib().stitch_rig_destroy(h)
    assert "step 1" in refused("cw off by one", cw=(1, steps[1]["cw"] + 1))
    assert "step 2" in refused("ch off by one", ch=(2, steps[2]["ch"] - 1))
    ulp = float(np.nextafter(np.float32(steps[1]["offx"]), np.float32(0)))
    assert np.float32(ulp) != np.float32(steps[1]["offx"])
    assert "step 1" in refused("min_x changed by one ulp", offx=(1, ulp))
    assert "step 2" in refused("min_y changed by one ulp", offy=(2, float(np.nextafter(np.float32(steps[2]["offy"]), np.float32(-10)))))
    assert "step 1" in refused("ox off by one", ox=(1, steps[1]["ox"] + 1))
    for key in ("p", "p_fwd"):
        for bad in (math.nan, math.inf):
            p = list(steps[0][key])
            p[5] = bad
            assert "finite" in refused(f"{bad} in {key}", **{key: (0, p)})
    assert "frame 4" in refused("dst = n", src=(2, 4))
    refused("dst = -1", src=(0, -1))
    refused("start = n", start_=4)
    refused("n = 0", n=0)
    refused("n = 65", sizes_=[sizes[0]] * 65)
    refused("max_sets = 0", max_sets=0)
    refused("max_sets = 17", max_sets=17)
    refused("zero frame width", sizes_=[(0, 512)] + sizes[1:])
    refused("negative frame height", sizes_=sizes[:3] + [(384, -1)])
    # src is recorded, not checked
    s2 = [dict(s, mosaic_src=99) for s in steps]
    rig = capi.Rig.from_steps(sizes, start, s2)
    rig.close()
    rc = capi.lib().stitch_rig_create(None, 4, 0, None, 0, None, None)
    assert rc == capi.ERR_ARG


def test_stitch_call_without_a_device(st):
    """Without a device the replay reports need_device's status, touches nothing and leaves the rig valid."""
    import torch
    if torch.cuda.is_available():
        pytest.skip("a HIP device is present")
    capi = st.capi
    sizes, start, steps, _ = _golden_run("2")
    rig = capi.Rig.from_steps(sizes, start, steps)
    frames = (capi.FrameU8 * 2)(capi.FrameU8(0x1000, 384, 512), capi.FrameU8(0x2000, 384, 512))
    outs, status = (C.c_void_p * 1)(0x3000), (C.c_int32 * 1)(77)
    assert capi.lib().stitch_dev_rig_stitch_u8(rig._h, frames, 1, outs, status, None, None) == capi.ERR_NO_DEVICE
    assert status[0] == 77 and b"no HIP device" in capi.lib().stitch_last_error()
    assert capi.lib().stitch_dev_project_many_u8(outs, outs, 1, 8, 8, 15.0, None) == capi.ERR_NO_DEVICE
    assert capi.lib().stitch_dev_finish_many_u8(outs, 1, 8, 8, 19.0, 20.0, None) == capi.ERR_NO_DEVICE
    w = C.c_int()
    assert capi.lib().stitch_rig_info(rig._h, C.byref(w), None, None, None, None) == 0 and w.value == 612
    assert rig.step_plan(0) is None
    rig.close()
