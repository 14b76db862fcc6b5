"""The form word of the mask pyramids that stand (csrc/stitch_call_form.h: mask_keep_word) on the host: tests/mask_keep_check.cpp is
the header compiled by the host compiler alone, and checks over tests/test_call_form_host.py's grid of canvases, capacities, n and
switch sets that calls with equal mask fields have equal words, that any difference in mask_l0 / mr_out / mr_in / fill_mask at any
level gives another word, and that keep_ok is clear whenever a level selects a kernel that does not know the skip.  No GPU."""
import json
import os
import subprocess

import pytest

import g_flags_ref
from call_form_tool import setting
from sift_ref import HERE, ROOT, host_compiler
from test_call_form_host import CAPS, SIZES, settings

KNOWN = {"WAVEFRONT", "NO_FUSE", "NO_SRC_FUSE", "NO_ZERO_TILES", "RECOMPUTE", "SINGLE_FAST", "ODD_DEC", "Y1S", "MOVER", "DEC7", "XBYM", "XBYM_MPIX", "Y2", "GATE64",
         "COARSE", "SRC_LONE_MPIX", "WAVEFRONT_STAMP"}  # the switches tests/mask_keep_check.cpp takes: those that choose a REDUCE kernel or a flag


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    path = os.path.join(str(tmp_path_factory.mktemp("mask_keep")), "mask_keep_check")
    subprocess.check_call([host_compiler(), "-O2", "-std=c++17", "-Wall", "-Wextra", "-I", os.path.join(ROOT, "computervisionimagestich2_amd", "csrc"),
                           "-I", os.path.join(ROOT, "include"), "-o", path, os.path.join(HERE, "mask_keep_check.cpp")])
    return path


def test_words_over_the_grid(exe, tmp_path):
    grid = tmp_path / "grid.txt"
    sets = []
    for env in settings():
        if all(k[len("STITCH_"):] in KNOWN for k in env):
            sets.append(setting(env))
    assert len(sets) > 20 and "" in sets
    with open(grid, "w") as f:
        f.write("w " + " ".join(map(str, SIZES)) + "\nh " + " ".join(map(str, SIZES)) + "\ncap " + " ".join(map(str, CAPS)) + "\n")
        for s in sets:
            f.write("set " + s + "\n")
    r = subprocess.run([exe, str(grid)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-2000:]
    last = r.stdout.splitlines()[-1].split()
    assert last[0] == "cases" and int(last[1]) > 100000 and int(last[3]) > 1000 and last[4:] == ["violations", "0"], r.stdout[-2000:]


def word(exe, cw, ch, cap, n, src=-1, env=None):
    args = [setting({k: v}) for k, v in (env or {}).items()]
    return json.loads(subprocess.run([exe, "word", str(cw), str(ch), str(cap), str(n), str(src), *args], check=True, capture_output=True, text=True).stdout)


@pytest.mark.parametrize("form", sorted(g_flags_ref.FORMS))
def test_the_pinned_batch_forms_keep_and_their_words_do_not_depend_on_n(exe, form):
    """tests/test_gpu_mask_keep.py's plans: every n of a pinned form has one word, with keep_ok."""
    env = {**g_flags_ref.FORMS[form], "STITCH_SINGLE_FAST": "1"}
    for cw, ch in ((1024, 768), (1088, 392)):
        words = [word(exe, cw, ch, 4, n, env=env) for n in (1, 2, 4)]
        assert all(w["keep_ok"] for w in words) and len({w["word"] for w in words}) == 1, words
        assert words[0]["levels"][0][:2] == [1, 1] and words[0]["levels"][1][2] == 1  # the implicit mask, the rows of level 1 recorded and read


def test_the_flagship_keeps_and_a_lone_pair_does_not(exe):
    batch, lone = word(exe, 6144, 4096, 16, 16), word(exe, 6144, 4096, 16, 1)
    assert batch["keep_ok"] and not lone["keep_ok"] and (batch["word"] | 1) != (lone["word"] | 1)
    # 1024 x 1024 without the three-wavefront sweeps: two pairs record the mask rows of level 1, one pair stores them
    two, one = word(exe, 1024, 1024, 4, 2, env={"STITCH_MOVER": "0"}), word(exe, 1024, 1024, 4, 1, env={"STITCH_MOVER": "0"})
    assert two["keep_ok"] and two["levels"][0][1] == 1 and one["levels"][0][1] == 0 and (two["word"] | 1) != (one["word"] | 1)
