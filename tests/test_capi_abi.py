"""CPU: the C-ABI library loads and exports every symbol include/stitch.h declares; without a HIP device every
compute entry point fails loudly (no CPU fallback in the product)."""
import ctypes as C
import os
import re
import shlex
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def header_text():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "stitch.h")).read(), flags=re.S)


def declared_functions():
    return sorted(set(re.findall(r"\b(stitch_[a-z0-9_]+)\s*\(", header_text())))


SCALARS = {"int": C.c_int, "int32_t": C.c_int, "unsigned": C.c_uint, "uint32_t": C.c_uint32, "float": C.c_float, "double": C.c_double,
           "size_t": C.c_size_t}
RETURNS = {"int": C.c_int, "void": None, "size_t": C.c_size_t, "const char *": C.c_char_p, "const void *": C.c_void_p}


def declared_signatures():
    """{name: (restype, argtypes)} of every prototype `ret name(params);` of the header, by the binding's rules: a pointer or
    array parameter is a c_void_p, a scalar has its C type."""
    sigs = {}
    for ret, name, params in re.findall(r"((?:const\s+)?\w+\s*\*?)\s*\b(stitch_\w+)\s*\(([^()]*)\)\s*;", header_text()):
        args = []
        for prm in [] if params.strip() == "void" else params.split(","):
            if "*" in prm or "[" in prm:
                args.append(C.c_void_p)
            else:
                args.append(SCALARS[" ".join(prm.split()[:-1])])  # the type in front of the parameter's name
        sigs[name] = (RETURNS[" ".join(ret.replace("*", " *").split())], args)
    return sigs


def test_header_declares_the_path():
    names = declared_functions()
    for must in ("stitch_project_u8", "stitch_warp_u8", "stitch_move_u8", "stitch_blend_u8", "stitch_equalize_u8",
                 "stitch_lummix_u8", "stitch_pair_f32", "stitch_dev_pair_f32", "stitch_plan_create", "stitch_last_error"):
        assert must in names


def test_library_exports_every_declared_symbol(st):
    lib = st.capi.lib()
    missing = [n for n in declared_functions() if not hasattr(lib, n)]
    assert not missing, missing
    assert lib.stitch_abi_version() == 5


def test_every_declared_function_has_its_signature(st):
    """capi.SIGNATURES, as lib() has applied it, states exactly the header's prototypes: a new or changed entry point without
    its row fails here, before anything runs on a GPU."""
    want, lib = declared_signatures(), st.capi.lib()
    assert sorted(want) == declared_functions() and len(want) == 108  # the parser above saw every prototype
    extra = sorted(set(st.capi.SIGNATURES) - set(want))
    assert not extra, f"capi.SIGNATURES has names include/stitch.h does not declare: {extra}"
    missing = sorted(set(want) - set(st.capi.SIGNATURES))
    assert not missing, f"capi.SIGNATURES lacks a row for: {missing}"
    bound = {n: (getattr(lib, n).restype, getattr(lib, n).argtypes) for n in want}  # argtypes None: never declared
    wrong = {n: (bound[n], want[n]) for n in sorted(want) if bound[n] != want[n]}
    assert not wrong, f"(bound, declared) signatures differ for: {wrong}"


def test_struct_mirrors_match_the_header(st, tmp_path):
    """Size, field count and every field offset of the ctypes mirrors (and of SIFT_KP_DTYPE) against what a C compiler makes of
    the header.  The program is generated from the mirrors' field names, so a renamed field does not compile."""
    capi = st.capi
    mirrors = {"stitch_blend_opts": capi.BlendOpts, "stitch_seam": capi.Seam, "stitch_pair_desc": capi.PairDesc,
               "stitch_bmp_info": capi.BmpInfo, "stitch_step_geom": capi.StepGeom, "stitch_match_desc": capi.MatchDesc,
               "stitch_ransac_opts": capi.RansacOpts, "stitch_ransac_desc": capi.RansacDesc, "StitchSiftOpts": capi.SiftOpts,
               "stitch_sift_desc": capi.SiftDesc}
    have = {}  # (struct, field) -> offset, (struct, "sizeof") -> size, as the binding has them
    for c, m in mirrors.items():
        have[c, "sizeof"] = C.sizeof(m)
        have.update({(c, f[0]): getattr(m, f[0]).offset for f in m._fields_})
    kp = capi.SIFT_KP_DTYPE
    have["StitchSiftKeypoint", "sizeof"] = kp.itemsize
    have.update({("StitchSiftKeypoint", f): kp.fields[f][1] for f in kp.names})
    prints = [f'    printf("{c} {f} %zu\\n", ' + (f"sizeof({c}));" if f == "sizeof" else f"offsetof({c}, {f}));") for c, f in have]
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text("\n".join(["#include <stddef.h>", "#include <stdio.h>", '#include "stitch.h"', "int main(void) {"] + prints
                             + ["    return 0;", "}", ""]))
    cc = subprocess.run(shlex.split(os.environ.get("CC", "cc")) + ["-std=c99", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)],
                        capture_output=True, text=True)
    assert cc.returncode == 0, f"a mirror names a field the header's struct lacks (or there is no C compiler):\n{cc.stderr}"
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout
    want = {(c, f): int(n) for c, f, n in (line.split() for line in out.splitlines())}
    wrong = {f"{c}.{f}": (have[c, f], want[c, f]) for c, f in have if have[c, f] != want[c, f]}
    assert not wrong, f"(mirror, header) sizes and offsets differ: {wrong}"
    # a mirror that stops short of a last field lying in the struct's tail padding agrees on every number above: count the fields
    for c in {c for c, _ in have}:
        body = re.search(r"typedef struct \w+\s*\{([^{}]*)\}\s*%s\s*;" % c, header_text()).group(1)
        declared = sum(len(d.split(",")) for d in body.split(";") if d.strip())
        assert declared == sum(1 for k in have if k[0] == c) - 1, f"{c}: the header declares {declared} fields"


def test_pyramid_levels_host_logic(st):
    n, lw, lh = st.pyramid_levels(6144, 4096)
    assert n == 12 and lw[0] == 6144 and lw[-1] == 3 and lh[-1] == 2
    n, lw, lh = st.pyramid_levels(1081, 527)
    assert (n, lw, lh) == (10, [1081, 540, 270, 135, 67, 33, 16, 8, 4, 2], [527, 263, 131, 65, 32, 16, 8, 4, 2, 1])
    assert st.pyramid_levels(600, 800, 1)[0] == 9
    with pytest.raises(st.StitchError) as e:
        st.pyramid_levels(4096, 4)
    assert e.value.code == st.capi.ERR_PYRAMID


def test_no_device_means_loud_failure(st):
    import torch
    if torch.cuda.is_available():
        pytest.skip("a HIP device is present")
    img = np.ones((3, 8, 8), np.uint8)
    for call in (lambda: st.project(img), lambda: st.blend(img, img), lambda: st.equalize(img),
                 lambda: st.capi.Plan(64, 64)):
        with pytest.raises(st.StitchError) as e:
            call()
        assert e.value.code == st.capi.ERR_NO_DEVICE
    assert st.device_count() == 0


def test_product_does_not_import_oracle():
    """The product package must never route through the oracle (it is test infrastructure)."""
    pkg = os.path.join(ROOT, "computervisionimagestich2_amd")
    for dirpath, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".hip", ".hpp", ".cpp", ".h")):
                text = open(os.path.join(dirpath, f), errors="ignore").read()
                assert "oracle_lib" not in text and "stitch_oracle" not in text and "libref_" not in text, os.path.join(dirpath, f)
