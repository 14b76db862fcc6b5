"""The pair path's decision -- which kernels reduce and collapse every level of a call (csrc/stitch_call_form.h: plan_shape, call_form)
-- on the host: tests/call_form_dump.cpp is the header compiled by the host compiler alone.  No GPU.

a  the invariants of a call's form over a grid of canvases, capacities, blend options and every switch value of tests/switch_table.py
   (evaluated by the program itself: the grid has some millions of calls);
b  the records against the rules the GPU tests count flags by (tests/g_flags_ref.py, tests/mask_rows_ref.py: below an even level), and the
   accessors' answers;
c  the records of switch_table.SHAPES at default switches against tests/golden/call_forms.json."""
import json
import os
import subprocess

import pytest

import g_flags_ref
import switch_table as T
from call_form_tool import build_dump, dump, setting
from sift_ref import HERE

SIZES = [1, 2, 3, 63, 64, 65, 128, 129, 512, 1020, 1021, 1024, 1088, 1100, 1101, 1152, 2048, 2100, 4096, 4097, 4160, 4224, 6144, 16384, 24576]
CAPS = [1, 2, 16]
GOLDEN = os.path.join(HERE, "golden", "call_forms.json")
PAIR_FORMS = {"lone", "batch", "blend", "host"}
# diagnostics: whether a stamp buffer is present is an input of the decision
STAMPS = [{"STITCH_WAVEFRONT_STAMP": "1", "STITCH_WAVEFRONT": "2"}, {"STITCH_XBYM_STAMP": "1", "STITCH_XBYM": "1"}, {"STITCH_COARSE_STAMP": "1"},
          {"STITCH_D7_STAMP": "0"}]


def settings():
    """Every switch of the table that a pair call reads, at each of its values, one at a time, with the extras the table lists."""
    out = [{}]
    for name, value, extra in T.cases():
        if PAIR_FORMS & set(T.SWITCHES[name]["forms"]):
            out.append({**extra, name: value})
    return out + list(g_flags_ref.FORMS.values()) + STAMPS


def write_grid(path):
    with open(path, "w") as f:
        f.write("w " + " ".join(map(str, SIZES)) + "\nh " + " ".join(map(str, SIZES)) + "\ncap " + " ".join(map(str, CAPS)) + "\n")
        for env in settings():
            f.write("set " + setting(env) + "\n")


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return build_dump(tmp_path_factory.mktemp("call_form"))


def test_invariants_over_the_grid(exe, tmp_path):
    grid = tmp_path / "grid.txt"
    write_grid(grid)
    r = subprocess.run([exe, "check", str(grid)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-2000:]
    last = r.stdout.splitlines()[-1].split()
    assert last[0] == "cases" and int(last[1]) > 1000000 and last[2:] == ["violations", "0"], r.stdout[-2000:]


FLAG_SHAPES = [(1088, 136), (1152, 192), (1020, 192), (1024, 4224), (1280, 136), (1024, 768), (1088, 392), (1024, 390), (1024, 770), (1022, 768), (1024, 769)]


def flags_of(rec):
    lv = rec["levels"]
    return [bool(lv[l]["g_in"]) for l in (1, 2)], [bool(lv[l]["mr_in"]) for l in (1, 2)]


@pytest.mark.parametrize("form", sorted(g_flags_ref.FORMS))
def test_flags_are_on_where_the_counters_rules_count(exe, tmp_path, form):
    """g_flags_ref.flagged_in_level counts nothing at a level below an odd width, mask_rows_ref.flagged_entries nothing from the first
    level below an odd width or height on; elsewhere the GPU tests expect the counts of set flags, so the flags must be on: at either
    capacity the tests use, for every n."""
    env = g_flags_ref.FORMS[form]
    cases = [(cw, ch, cap, n, -1, False, g_flags_ref.OPTS, False, env) for cw, ch in FLAG_SHAPES for cap in (2, 4) for n in range(1, cap + 1)]
    for case, rec in zip(cases, dump(exe, tmp_path, cases)):
        lv, even, want_g, want_mr = rec["levels"], True, [], []
        for l in (1, 2):
            pw, ph = lv[l - 1]["w"], lv[l - 1]["h"]
            even = even and pw % 2 == 0 and ph % 2 == 0
            want_g.append(pw % 2 == 0)
            want_mr.append(even)
        assert flags_of(rec) == (want_g, want_mr), (case, flags_of(rec))
        for l in (0, 1):  # the collapse and the counters read what the sweep wrote
            assert lv[l]["g_out"] == lv[l + 1]["g_in"] and lv[l]["mr_out"] == lv[l + 1]["mr_in"] == lv[l + 1]["c_mr"], case


def test_flags_are_off_without_the_batch_sweep_and_with_the_other_flags(exe, tmp_path):
    off = [(cw, ch, 2, n, -1, False, g_flags_ref.OPTS, False, env) for cw, ch in FLAG_SHAPES for n in (1, 2)
           for env in ({}, {"STITCH_WAVEFRONT": "0"}, {"STITCH_WAVEFRONT": "3", "STITCH_NO_ZERO_TILES": "1"}, {"STITCH_WAVEFRONT": "3", "STITCH_RECOMPUTE": "1"})]
    off += [(cw, ch, 2, 1, 0, False, g_flags_ref.OPTS, True, g_flags_ref.FORMS["fused3"]) for cw, ch in FLAG_SHAPES]  # the coarse levels of a split pair
    for case, rec in zip(off, dump(exe, tmp_path, off)):
        if not case[8] and case[0] >= 1024 and case[1] >= 1024:
            continue  # (1024 x 4224 takes the batch's sweep by itself)
        assert flags_of(rec) == ([False, False], [False, False]), case


def test_accessor_answers(exe, tmp_path):
    """stitch_plan_fast_paths and stitch_plan_call_forms answer from the shape and the record."""
    FUSED_SWEEP, ZERO_TILES, FUSED_DECIMATE, COARSE = 4, 8, 16, 32
    cases = [(1100, 620, 1, 1, -1, False, {}, False, {}), (1100, 620, 3, 3, -1, False, {}, False, {}), (2048, 2048, 2, 2, -1, False, {}, False, {}),
             (2048, 2048, 2, 1, -1, False, {}, False, {}), (6144, 4096, 1, 1, -1, False, {}, False, {}), (1101, 617, 1, 1, -1, False, {}, False, {"STITCH_ODD_DEC": "0"}),
             (24576, 16384, 1, 1, -1, False, {}, False, {})]
    lone, batch3, batch, one_of_two, big, odd, huge = dump(exe, tmp_path, cases)
    assert not lone["fast_paths"] & (FUSED_SWEEP | ZERO_TILES) and lone["fast_paths"] & FUSED_DECIMATE and lone["fast_paths"] & COARSE
    assert lone["levels"][0]["sweep"] == "lone" and not lone["levels"][0]["xby"] and not lone["src"]
    assert batch3["levels"][0]["sweep"] == "lone" and not batch3["src"]  # 3 x 0.68 MPix: materialised, levels too small to stream
    assert batch["fast_paths"] & FUSED_SWEEP and batch["fast_paths"] & ZERO_TILES and batch["src"]
    assert [v["sweep"] for v in batch["levels"][:3]] == ["batch", "batch", "lone"] and batch["levels"][0]["zt"]
    assert one_of_two["levels"][0]["sweep"] == "lone" and not one_of_two["levels"][0]["zt"]  # a per-call choice
    assert big["levels"][0]["xby"] and big["src"] and not big["levels"][0]["zt"] and not big["levels"][1]["xby"]
    assert not odd["fast_paths"] & FUSED_DECIMATE and odd["levels"][0]["y_bwd"] == "k_vv_y_bwd" and odd["levels"][0]["decimate"]
    assert huge["fast_paths"] & FUSED_SWEEP and huge["levels"][0]["xby"] and huge["levels"][0]["zt"] and huge["src"]


def snapshot_cases():
    out = []
    for shape, (cw, ch) in T.SHAPES.items():
        nb = 2 if cw >= 4096 else 3  # tests/test_gpu_switches.py's batches
        out += [(f"{shape}/lone", (cw, ch, 1, 1, -1, False, {}, False, {})), (f"{shape}/batch", (cw, ch, nb, nb, -1, False, {}, False, {})),
                (f"{shape}/blend", (cw, ch, 1, 1, -1, True, {}, False, {}))]
    return out


def test_snapshot_of_the_default_forms(exe, tmp_path):
    """Guards later changes of the decision: the records the library launched from when the fixture was written (then shown equal,
    dispatch by dispatch, to the launches of the code that decided while it launched: profiles/call_form_trace.txt)."""
    names, cases = zip(*snapshot_cases())
    got = dict(zip(names, dump(exe, tmp_path, cases)))
    if os.environ.get("CALL_FORMS_WRITE"):
        with open(GOLDEN, "w") as f:
            json.dump(got, f, indent=0, sort_keys=True)
    with open(GOLDEN) as f:
        want = json.load(f)
    assert sorted(got) == sorted(want)
    for name in names:
        assert got[name] == want[name], name
