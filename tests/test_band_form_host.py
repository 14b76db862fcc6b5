"""The band path's decisions -- what a band of a split pair holds and what each of its entry points launches at each level
(csrc/stitch_call_form.h: band_shape, band_form, band_zt_after) -- on the host, through tests/call_form_dump.cpp.  No GPU.

a  the invariants of a band's sequence of calls over a grid: the canvases of test_call_form_host.SIZES that admit a split, 1 to 8 ranks
   and every rank of them, every admissible split_levels, the band switches (STITCH_NO_ZERO_TILES, STITCH_BAND_PLANES -- which is
   also stitch_band_set_level0 --, STITCH_BAND_PLAIN), every sequence pipeline.BandStitcher.steps can issue at a level (separate sweeps,
   the fused sweep, plane by plane, column chunks) and the one tests/test_gpu_band.py issues itself (evaluated by the program);
b  the records of tests/test_gpu_band.py's shapes at default switches against tests/golden/band_forms.json;
c  every kernel instance the band path can launch is selected by one of those shapes: the list in test_gpu_band.py's docstring."""
import json
import os
import subprocess

import pytest

from sift_ref import HERE
from test_call_form_host import SIZES, build_dump

GOLDEN = os.path.join(HERE, "golden", "band_forms.json")
# (world, cw, ch, split_levels, form) of tests/test_gpu_band.py.  form -> (the sequence's letter, level 0 source-fused): BandStitcher
# fuses the sweeps by default only without a split, and stores level 0 where the y states cross ranks plane by plane
FORMS = {"fused": ("f", True), "separate": ("s", True), "planes": ("p", False), "stored": ("s", False), "stored+fused": ("f", False), "chunks4": ("c", True),
         "fused+cols": ("x", True)}
GROUP = [(2, 2048, 1024, 3), (3, 768, 384, 2), (8, 2048, 1024, 2), (6, 772, 384, 1)]  # test_band_group_single_host_thread: every form
CASES = ([(2, 2048, 1024, 2, "separate"), (4, 1024, 512, 1, "separate"), (3, 770, 384, 2, "separate"), (3, 768, 384, 2, "planes")]  # test_pair_split_into_row_bands
         + [(2, 2048, 1024, 3, "separate"), (3, 768, 384, 2, "separate"), (2, 770, 384, 2, "separate"), (2, 1540, 768, 2, "separate"), (6, 772, 384, 1, "separate"),
            (8, 2048, 1024, 2, "separate")]  # ..._threads
         + [(w, cw, ch, Ls, f) for w, cw, ch, Ls in GROUP for f in ("fused", "separate", "planes", "stored", "stored+fused", "chunks4")]
         + [(1, 1000, 500, 2, "fused")]  # test_single_rank_band_is_the_whole_pair
         + [(3, 768, 396, 2, "fused"), (1, 768, 396, 2, "fused+cols")])  # the bands whose rows eight does not divide
# every instance of the kernel families the band path chooses between (band_form), and a case above that selects it
INSTANCES = ["k_vv_x_fwd<PX,1>", "k_vv_x_fwd<float,0>", "k_vv_x_bwd", "k_vv_xbyf<0,float,0,0>", "k_vv_xbyf<0,float,0,1>", "k_vv_y_fwd<0>", "k_vv_y_fwd<1>",
             "k_vv_y_bwd_dec<0,YST,1,0,0>", "k_vv_y_bwd_dec<1,YST,1,0,0>", "k_vv_y_bwd_dec<0,YST,1,0,1>", "k_vv_y_bwd_dec<1,YST,1,0,1>", "k_vv_y_bwd", "k_decimate",
             "k_collapse4", "k_collapse", "k_src_index", "k_compose", "k_mask", "k_seam"]


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return build_dump(tmp_path_factory.mktemp("band_form"))


def test_invariants_over_the_grid(exe, tmp_path):
    grid = tmp_path / "grid.txt"
    grid.write_text("w " + " ".join(map(str, SIZES)) + "\nh " + " ".join(map(str, SIZES)) + "\n")
    r = subprocess.run([exe, "bandcheck", str(grid)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-2000:]
    last = r.stdout.splitlines()[-1].split()
    assert last[0] == "bands" and int(last[1]) > 50000 and last[2] == "cases" and int(last[3]) > 1000000 and last[-2:] == ["violations", "0"], r.stdout[-2000:]


def snapshot_cases():
    out = {}
    for world, cw, ch, Ls, form in CASES:
        kinds, src = FORMS[form]
        for rank in sorted({0, min(1, world - 1), world - 1}):  # the first band, one with two neighbours (or the last), the last
            out[f"{world}x{cw}x{ch}/Ls{Ls}/{form}/rank{rank}"] = f"{cw} {ch} {rank} {world} {Ls} 1 {int(src)} 0 {kinds}"
    return out


@pytest.fixture(scope="module")
def records(exe, tmp_path_factory):
    cases = snapshot_cases()
    path = tmp_path_factory.mktemp("band_cases") / "cases.txt"
    path.write_text("\n".join(cases.values()) + "\n")
    out = subprocess.run([exe, "band", str(path)], check=True, capture_output=True, text=True).stdout
    return dict(zip(cases, (json.loads(line) for line in out.splitlines())))


def test_snapshot_of_the_default_forms(records):
    """Guards later changes of the decision: the records the library launched from when the fixture was written (then shown equal,
    dispatch by dispatch, to the launches of the code that decided while it launched: profiles/band_form_trace.txt)."""
    if os.environ.get("BAND_FORMS_WRITE"):
        with open(GOLDEN, "w") as f:
            json.dump(records, f, indent=0, sort_keys=True)
    with open(GOLDEN) as f:
        want = json.load(f)
    assert sorted(records) == sorted(want)
    for name in records:
        assert "refused" not in records[name], name
        assert records[name] == want[name], name


def test_every_instance_is_selected_by_a_gpu_case(records):
    selected = {}
    for name, rec in sorted(records.items()):
        for call in rec["calls"]:
            for k in call["kernels"].split():
                selected.setdefault(k, name)
    assert sorted(selected) == sorted(INSTANCES), (sorted(set(INSTANCES) - set(selected)), sorted(set(selected) - set(INSTANCES)))
