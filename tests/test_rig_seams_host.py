"""CPU: the host side of fixed seams (include/stitch_rig_seams.h) -- the header compiles as C99, the binding's seventh signature
table states exactly what it declares and shares no name with the six others; every argument error is reported before a device is
needed; stitch_seam_from_sums is the oracle's seam on random indicator rows under both rules, parts where float and double part,
and rejects exactly what no middle row can give; and the yardsticks of tests/test_gpu_rig_seams.py (tests/rig_seams_ref.py) are
themselves pinned: blend_given to Oracle.blend on the oracle's own seam, coverage_chain to tests/golden/rig_seams.json."""
import ctypes as C
import hashlib
import json
import os
import re
import shlex
import subprocess

import numpy as np
import pytest

import rig_seams_ref as ref
from oracle_lib import EX6_OPTS, ROOT_OPTS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
HEADER = os.path.join(ROOT, "include", "stitch_rig_seams.h")

FUNCTIONS = ("stitch_seam_from_sums", "stitch_dev_pairs_seamed_u8", "stitch_dev_pairs_seamed_f32", "stitch_rig_fix_seams", "stitch_rig_clear_seams",
             "stitch_rig_seams", "stitch_dev_rig_geometric_seams", "stitch_dev_rig_coverage_u8", "stitch_rig_step_canvas")


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
    assert sorted(capi.RIG_SEAMS_SIGNATURES) == sorted(want)
    others = set(capi.SIGNATURES) | set(capi.PANORAMA_SIGNATURES) | set(capi.RIG_SIGNATURES) | set(capi.EXPOSURE_SIGNATURES) \
        | set(capi.RIG_EXPOSURE_SIGNATURES) | set(capi.CALIBRATE_SIGNATURES)
    assert not set(capi.RIG_SEAMS_SIGNATURES) & others
    bound = {n: (getattr(lib, n).restype, getattr(lib, n).argtypes) for n in want}
    wrong = {n: (bound[n], want[n]) for n in sorted(want) if bound[n] != tuple(want[n])}
    assert not wrong, f"(bound, declared) signatures differ for: {wrong}"
    assert lib.stitch_abi_version() == 5


def test_header_is_c99(st, tmp_path):
    cc = shlex.split(os.environ.get("CC", "cc")) + ["-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include")]
    src = tmp_path / "uses.c"
    src.write_text("\n".join(['#include "stitch_rig_seams.h"', "void uses(void) {"] + [f"    (void)(&{n});" for n in FUNCTIONS]
                             + ["    (void)sizeof(stitch_seam);", "    (void)sizeof(stitch_pair_desc);", "}", ""]))
    r = subprocess.run(cc + ["-fsyntax-only", str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


# ---- a seam from its four integers ------------------------------------------------------------------------------------------
def _from_sums(capi, four, rule, cw):
    s = capi.Seam()
    rc = capi.lib().stitch_seam_from_sums(*[int(v) for v in four], rule, cw, C.byref(s))
    return rc, s


@pytest.mark.parametrize("rule", [0, 1])
def test_seam_from_sums_is_the_oracles_seam(st, oracle, rule):
    """Random indicator rows: a present on a random subset of the columns, b on another; all three channels set, so both rules
    count the same pixels."""
    capi = st.capi
    rng = np.random.default_rng(20 + rule)
    seen = set()
    for w in (1, 2, 7, 64, 95, 130, 1081):
        for _ in range(12):
            h = int(rng.integers(1, 6))
            a, b = np.zeros((3, h, w), np.uint8), np.zeros((3, h, w), np.uint8)
            a[:, h // 2, rng.random(w) < rng.uniform(0.1, 1.0)] = 255
            b[:, h // 2, rng.random(w) < rng.uniform(0.1, 1.0)] = 255
            a[:, h // 2, int(rng.integers(w))] = b[:, h // 2, int(rng.integers(w))] = 255
            rc, want = oracle.seam(a, b, rule)
            if rc:  # no overlap on this row: not a seam anybody can state
                assert _from_sums(capi, (want.sum_a_x, want.n_a, want.sum_ov_x, want.n_ov), rule, w)[0] == capi.ERR_ARG
                continue
            rc, got = _from_sums(capi, want.as_tuple()[:4], rule, w)
            assert rc == 0 and got.as_tuple() == want.as_tuple(), (w, want.as_tuple(), got.as_tuple())
            assert (got.ratio, got.ov) == (want.ratio, want.ov)
            assert ref.derive(want.as_tuple(), rule)[:2] == (want.branch, want.start)
            seen.add(want.branch)
    assert seen == {0, 1}


def test_the_rules_part_where_float_and_double_part(st):
    """cw = 16384, 8191 columns whose sum is 8191 * 8000 - 1: the quotient 8000 - 1/8191 rounds to 8000.0f, so rule 0 starts the
    mask at 8001; rule 1 keeps the double and starts at 8000."""
    capi = st.capi
    four = (8191 * 8000 - 1, 8191, 8191 * 8000 - 1, 8191)
    rc0, s0 = _from_sums(capi, four, 0, 16384)
    rc1, s1 = _from_sums(capi, four, 1, 16384)
    assert rc0 == 0 and rc1 == 0
    assert (s0.ov, s0.start, s0.branch) == (8000.0, 8001, 1) and (s1.start, s1.branch) == (8000, 1)
    assert capi.seam_from_sums(*four, 0, 16384).as_tuple() == s0.as_tuple()


def test_rejection_bounds_at_their_edges(st):
    capi = st.capi
    cw = 100

    def lo(n):
        return n * (n - 1) // 2

    def hi(n):
        return n * cw - n * (n + 1) // 2

    ok = [(0, 1, 0, 1), (cw - 1, 1, cw - 1, 1), (lo(cw), cw, lo(cw), cw), (hi(7), 7, hi(7), 7), (hi(7), 7, lo(7), 7), (hi(7), 7, lo(3), 3), (hi(7), 7, hi(3), 3),
          (lo(7), 7, lo(3), 3), (lo(7), 7, lo(7), 7)]
    bad = [(0, 1, 0, 0), (0, 0, 0, 0), (lo(7), 7, lo(8), 8), (lo(cw + 1), cw + 1, 0, 1), (lo(7) - 1, 7, lo(3), 3), (hi(7) + 1, 7, lo(3), 3),
           (hi(7), 7, lo(3) - 1, 3), (hi(7), 7, hi(3) + 1, 3), (lo(7), 7, lo(7) + 1, 7), (cw, 1, 0, 1), (-1, 1, -1, 1), (5, -1, 5, -1), (lo(7), 7, lo(7) + 1, 6)]
    for rule in (0, 1):
        for four in ok:
            assert _from_sums(capi, four, rule, cw)[0] == 0, four
        for four in bad:
            assert _from_sums(capi, four, rule, cw)[0] == capi.ERR_ARG, four
    assert b"seam_from_sums" in capi.lib().stitch_last_error()
    assert _from_sums(capi, ok[0], 2, cw)[0] == capi.ERR_ARG and _from_sums(capi, ok[0], -1, cw)[0] == capi.ERR_ARG
    assert _from_sums(capi, ok[0], 0, 0)[0] == capi.ERR_ARG
    assert capi.lib().stitch_seam_from_sums(0, 1, 0, 1, 0, cw, None) == capi.ERR_ARG
    with pytest.raises(capi.StitchError) as e:
        capi.seam_from_sums(cw, 1, 0, 1, 0, cw)
    assert e.value.code == capi.ERR_ARG


# ---- argument errors come before a device is needed --------------------------------------------------------------------------
def _small_rig(capi, steps=None, **kw):
    return capi.Rig.from_steps(ref.SMALL, 0, ref.small_steps(capi) if steps is None else steps, **kw)


def test_rig_fix_clear_and_read_are_host_only(st):
    capi = st.capi
    rig = _small_rig(capi)
    steps = ref.small_steps(capi)
    assert rig.seams == []
    recs = [(2000, 50, 900, 30), (700, 35, 400, 25)]
    assert rig.fix_seams(recs) is rig
    want = [capi.seam_from_sums(*r, 0, st_["cw"]).as_tuple() for r, st_ in zip(recs, steps)]
    assert rig.seams == want and capi.lib().stitch_rig_seams(rig._h, None, 0) == 2
    one = (capi.Seam * 1)()
    assert capi.lib().stitch_rig_seams(rig._h, one, 1) == 2 and one[0].as_tuple() == want[0]
    # the other fields of a record passed in are ignored
    full = [capi.Seam(*r, 9.0, 9.0, 7, 7) for r in recs]
    assert rig.fix_seams(full).seams == want
    # a bad record names its step and leaves the rig as it was
    for k, bad in ((0, (2000, 50, 900, 0)), (1, (700, 35, 400, 36)), (1, (steps[1]["cw"], 1, 0, 1))):
        with pytest.raises(capi.StitchError) as e:
            rig.fix_seams([bad if i == k else recs[i] for i in range(2)])
        assert e.value.code == capi.ERR_ARG and f"step {k}" in str(e.value)
        assert rig.seams == want
    for n in (1, 3, 0):
        with pytest.raises(capi.StitchError) as e:
            rig.fix_seams(recs[:1] * n)
        assert e.value.code == capi.ERR_ARG and rig.seams == want
    assert capi.lib().stitch_rig_fix_seams(rig._h, None, 2) == capi.ERR_ARG
    assert rig.clear_seams() is rig and rig.seams == []
    assert rig.step_plan(0) is None  # no device was touched
    rig.close()
    # rule 1 derives the records in double
    rig = _small_rig(capi, opts=EX6_OPTS)
    assert rig.fix_seams(recs).seams == [capi.seam_from_sums(*r, 1, st_["cw"]).as_tuple() for r, st_ in zip(recs, steps)]
    rig.close()
    zero = capi.Rig.from_steps([(64, 48)], 0, [])
    assert zero.fix_seams([]).seams == []
    with pytest.raises(capi.StitchError):
        zero.fix_seams([recs[0]])
    zero.close()
    L = capi.lib()
    assert L.stitch_rig_fix_seams(None, None, 0) == L.stitch_rig_clear_seams(None) == L.stitch_rig_seams(None, None, 0) == capi.ERR_ARG


def test_argument_errors_come_before_a_device(st):
    import torch
    capi = st.capi
    L = capi.lib()
    rig = _small_rig(capi)
    steps = ref.small_steps(capi)
    cw, ch = C.c_int(), C.c_int()
    for step, want in ((-1, (rig.width, rig.height)), (0, (steps[0]["cw"], steps[0]["ch"])), (1, (steps[1]["cw"], steps[1]["ch"]))):
        assert L.stitch_rig_step_canvas(rig._h, step, C.byref(cw), C.byref(ch)) == 0 and (cw.value, ch.value) == want
    for step in (-2, 2):
        assert L.stitch_rig_step_canvas(rig._h, step, C.byref(cw), C.byref(ch)) == capi.ERR_ARG
        assert L.stitch_dev_rig_coverage_u8(rig._h, step, 2, 0x1000, None) == capi.ERR_ARG
    assert L.stitch_rig_step_canvas(None, 0, C.byref(cw), C.byref(ch)) == L.stitch_rig_step_canvas(rig._h, 0, None, C.byref(ch)) == capi.ERR_ARG
    for which in (-1, 3):
        assert L.stitch_dev_rig_coverage_u8(rig._h, -1, which, 0x1000, None) == capi.ERR_ARG
    assert L.stitch_dev_rig_coverage_u8(rig._h, -1, 2, None, None) == L.stitch_dev_rig_coverage_u8(None, -1, 2, 0x1000, None) == capi.ERR_ARG
    assert L.stitch_dev_rig_geometric_seams(None, None, None) == capi.ERR_ARG
    one, seam = (capi.PairDesc * 1)(), (capi.Seam * 1)()
    for fn in (L.stitch_dev_pairs_seamed_u8, L.stitch_dev_pairs_seamed_f32):
        assert fn(None, one, 1, seam, None) == capi.ERR_ARG
    zero = capi.Rig.from_steps([(64, 48)], 0, [])
    assert L.stitch_dev_rig_coverage_u8(zero._h, 0, 2, 0x1000, None) == capi.ERR_ARG
    assert L.stitch_rig_step_canvas(zero._h, -1, C.byref(cw), C.byref(ch)) == 0 and (cw.value, ch.value) == (64, 48)
    if not torch.cuda.is_available():  # and what is left needs one
        assert L.stitch_dev_rig_geometric_seams(rig._h, None, None) == capi.ERR_NO_DEVICE
        assert L.stitch_dev_rig_coverage_u8(rig._h, -1, 2, 0x1000, None) == capi.ERR_NO_DEVICE
        assert rig.seams == []
    zero.close()
    rig.close()


# ---- the yardsticks ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h", [(95, 48), (64, 49), (130, 70)])
@pytest.mark.parametrize("opts", [ROOT_OPTS, EX6_OPTS], ids=["root", "ex6"])
def test_blend_given_is_the_oracles_blend_on_its_own_seam(oracle, w, h, opts):
    rng = np.random.default_rng(w * 7 + h)
    for dtype in (np.uint8, np.float32):
        a, b = (rng.integers(1, 256, (3, h, w)).astype(dtype) for _ in range(2))
        a[:, :, : w // 5] = 0
        b[:, :, 2 * w // 3:] = 0
        rc, want, seam = oracle.blend(a, b, opts)[:3]
        assert rc == 0
        got = ref.blend_given(oracle, a, b, opts, seam.as_tuple())
        assert got.dtype == want.dtype and got.tobytes() == want.tobytes()
        # and another seam gives another image
        assert ref.blend_given(oracle, a, b, opts, (0, 1, 0, 1)).tobytes() != want.tobytes()


def _bits_sha(mask):
    return hashlib.sha256(np.packbits(np.ascontiguousarray(mask, bool)).tobytes()).hexdigest()


def test_coverage_chain_gives_the_recorded_values(st, oracle):
    with open(os.path.join(GOLD, "rig_seams.json")) as f:
        G = json.load(f)
    with open(os.path.join(GOLD, "golden.json")) as f:
        steps = json.load(f)["runs"][G["run"]]["steps"]
    assert G["seams"] == [[150212, 376, 48887, 166, 1, 295], [80166, 372, 52635, 165, 0, 320], [92750, 371, 57974, 164, 0, 354]]
    assert G["content_seams"][:2] == G["seams"][:2] and G["content_seams"][2][2:] == [53820, 150, 0, 359]
    assert (G["proj_fraction"], G["union_fraction"]) == (0.955414, 0.889409)
    cov, c0 = ref.coverage_chain(oracle, [tuple(s) for s in G["sizes"]], steps[0]["start"], steps, G["fov_deg"])
    assert [list(c["seam"]) for c in cov] == G["seams"] and all(c["rc"] == 0 for c in cov)
    assert round(float(c0.mean()), 6) == G["proj_fraction"] and round(float(cov[-1]["U"].mean()), 6) == G["union_fraction"]
    assert _bits_sha(c0) == G["proj_bits_sha256"]
    assert [{k: _bits_sha(c[k]) for k in "ABU"} for c in cov] == G["step_bits_sha256"]
    for c, g in zip(cov, G["seams"]):  # the library's host arithmetic on the same integers
        assert st.capi.seam_from_sums(*g[:4], 0, c["A"].shape[1]).as_tuple() == tuple(g)


def test_geometric_failure_cases_fail_in_the_yardstick(st, oracle):
    capi = st.capi
    assert (capi.ERR_EMPTY_MIDROW, capi.ERR_ZERO_OVERLAP) == (-2, -3)
    for name, (sizes, steps, status) in ref.failure_cases(capi).items():
        cov, _ = ref.coverage_chain(oracle, sizes, 0, steps)
        assert [c["rc"] for c in cov] == [0, status], name
        rig = capi.Rig.from_steps(sizes, 0, steps)  # the description itself is a valid rig
        rig.close()
