"""No GPU: tests/hard_inputs.py held to the oracle and to tests/src_runs_ref.py before any GPU run.

a  the table states the oracle's answer for every item tests/test_gpu_hard_content.py and tests/test_gpu_hard_maps.py run; at most 5 %
   of a content class's items are refusals; every signature of form_cover is run by an accepted item of checker / binary / white and
   by one of holes / band / tiny;
b  every content class does what it is there for, counted on the oracle's output;
c  every map class does what it is there for, by src_runs_ref.classes;
d  the library's host run rule (stitch_src_run_classes) and the rule compiled alone under the address and undefined-behaviour
   sanitizers (tests/src_runs_dump.cpp, as tests/test_src_runs_host.py builds it) equal src_runs_ref.classes on every map class, for
   4-byte and 1-byte samples.
profiles/hard_inputs.txt holds the counts (scripts are not needed: `python tests/test_hard_inputs_host.py` prints the file)."""
import collections
import os
import subprocess

import numpy as np
import pytest

import form_cover as FC
import g_flags_ref
import hard_inputs as H
import src_runs_ref as R
from form_cover_refs import ALL_CASES, build_records, case_id, pixel_types
from oracle_lib import ROOT_OPTS
from sift_ref import HERE, ROOT, host_compiler

CANVASES = (H.PAIR_CANVAS,) + H.RUN_CANVASES + (H.BAND_CANVAS, H.RESIDUAL_CANVAS)
FULL_PAIR_PIXELS = 300 * 300  # below it the item's rc is also taken from the whole Oracle.pair / Oracle.blend


@pytest.fixture(scope="module")
def records(tmp_path_factory):
    return build_records(tmp_path_factory.mktemp("hard_inputs"))


def used_items(records):
    """(index, dtype, j) of every item the GPU test runs."""
    for index, (case, rec) in enumerate(zip(ALL_CASES, records)):
        for dtype in pixel_types(rec):
            for js in H.hard_calls(case[3]):
                for j in js:
                    yield index, dtype, j


# ---- a ---------------------------------------------------------------------------------------------------------------------------
def test_the_table_states_the_oracles_answer(oracle, records):
    per_class, refused = collections.Counter(), collections.Counter()
    for index, dtype, j in used_items(records):
        cw, ch, _, _, dense, opts = ALL_CASES[index][:6]
        want = H.stated_rc(index, dtype, j)
        assert H.item_rc(index, dtype, j) == want, H.item_key(index, dtype, j)
        if cw * ch <= FULL_PAIR_PIXELS:
            if dense:
                _, A, B = H.dense_inputs(index, dtype, j)
                rc = oracle.blend(A, B, FC.OPTION_SETS[opts])[0]
            else:
                _, _, F, P, M, ox = H.pair_inputs(index, dtype, j)
                rc = oracle.pair(F, P, 0.0, 0.0, M, ox, 0, cw, ch, FC.OPTION_SETS[opts])[0]
            assert rc == want, H.item_key(index, dtype, j)
        name = (H.item_class(index, dtype, j), np.dtype(dtype).name)
        per_class[name] += 1
        refused[name] += want != 0
    print({k: (refused[k], v) for k, v in sorted(per_class.items())})
    for k, v in per_class.items():
        assert refused[k] <= 0.05 * v, (k, refused[k], v)
    assert set(per_class) == {(c, "uint8") for c in H.U8_CLASSES} | {(c, "float32") for c in H.F32_CLASSES}
    keys = {(case_id(c), t, j) for c in ALL_CASES for t in ("uint8", "float32") for j in range(len(H.hard_calls(c[3])) * c[3])}
    assert set(H.REFUSED) <= keys and set(H.RESEED) <= keys and set(H.PHASE) <= keys and not set(H.REFUSED) & (set(H.RESEED) | set(H.PHASE))
    assert all(rc in (-2, -3) for rc in H.REFUSED.values())


def test_every_signature_is_run_on_saturating_and_on_holed_content(records):
    """Every signature of form_cover is run by an accepted item of checker / binary / white and by one of holes / band / tiny (in float
    frames the value casts count as their class)."""
    seen = collections.defaultdict(set)
    for index, dtype, j in used_items(records):
        if H.stated_rc(index, dtype, j) == 0:
            for sig in FC.signatures(records[index]):
                seen[sig].add(H.item_class(index, dtype, j))
    every = set().union(*(FC.signatures(r) for r in records))
    assert every == set(seen) >= {s for c in ALL_CASES for s in c[6]}
    missing = {s: sorted(c) for s, c in seen.items() if not (c & set(H.SATURATING) and c & set(H.HOLED))}
    assert not missing, missing


def test_three_consecutive_classes_hold_both_kinds():
    for classes in (H.U8_CLASSES, H.F32_CLASSES):
        for i in range(len(classes)):
            three = {classes[(i + k) % len(classes)] for k in range(3)}
            assert three & set(H.SATURATING) and three & set(H.HOLED), three
    assert [len(c) * len(H.hard_calls(len(c))) >= 3 for c in ([0], [0, 1], [0, 1, 2], list(range(16)))] == [True] * 4


def test_the_map_batches_are_what_the_table_states(oracle, st):
    """Every pair of tests/test_gpu_hard_maps.py: the oracle accepts it, or refuses it with the code stated."""
    got = {}
    for dtype in (np.uint8, np.float32):
        t = np.dtype(dtype).name
        for i, name in enumerate(H.MAP_CLASSES):
            got[("pairs", name, t)] = H.pair_oracle(H.map_pair(name, H.PAIR_CANVAS, dtype, seed=i))[0]
            got[("mix", name, t)] = H.pair_oracle(H.map_pair(name, H.PAIR_CANVAS, dtype, "binary", "holes", seed=i))[0]
        for name, rc in H.REFUSAL_CLASSES.items():
            assert H.pair_oracle(H.map_pair(name, H.PAIR_CANVAS, dtype))[0] == rc, (name, t)
        for name in H.BAND_MAPS:
            got[("bands", name, t)] = H.pair_oracle(H.map_pair(name, H.BAND_CANVAS, dtype))[0]
    for canvas in H.RUN_CANVASES:
        for name in H.RUN_MAPS:
            for seed in (0, 1):
                rc = H.pair_oracle(H.map_pair(name, canvas, np.float32, seed=seed), dict(ROOT_OPTS, level_rule=1))[0]
                assert got.setdefault((f"runs-{canvas[0]}x{canvas[1]}", name, "float32"), rc) == rc
    assert {k: v for k, v in got.items() if v} == H.MAP_REFUSED
    for name, (sizes, steps) in H.rig_cases(st.capi).items():  # the rig's chains have a pyramid and a seam at every step
        for i in range(2):
            frames = [H.content(("fullrange", "holes")[i], w, h, np.uint8, 10 * i + f) for f, (w, h) in enumerate(sizes)]
            result = oracle.project(frames[0])
            for s in steps:
                rc, result = oracle.pair(oracle.project(frames[s["src"]]), s["p"], s["offx"], s["offy"], result, s["ox"], s["oy"], s["cw"], s["ch"])
                assert rc == 0, (name, i, rc)


# ---- b ---------------------------------------------------------------------------------------------------------------------------
def class_pair(name, dtype, canvas=H.PAIR_CANVAS, seed=5):
    r = H.map_pair("near", canvas, dtype, name, name, seed)
    rc, out, seam = H.pair_oracle(r)
    assert rc == 0, (name, rc)
    o = H.oracle()
    ones = lambda a: np.ones(a.shape, np.uint8)
    union = (o.warp(ones(r["F"]), r["p"], 0.0, 0.0, r["cw"], r["ch"]) | o.move(ones(r["M"]), 0, 0, r["cw"], r["ch"])) != 0
    return out, seam, union


def clamp_counts(name, dtype=np.uint8):
    """(samples equal to 255, samples equal to 0 inside the union of the footprints, samples) of the oracle's output."""
    out, _, union = class_pair(name, dtype)
    return int((out == 255).sum()), int(((out == 0) & union).sum()), out.size


def test_content_classes_reach_the_clamps():
    n255, _, n = clamp_counts("synth")
    assert n255 < 1e-4 * n  # the synthetic pair hardly reaches the upper clamp
    for name in ("checker", "binary", "white"):
        n255, n0, n = clamp_counts(name)
        print(name, n255, n0, n)
        assert n255 >= 0.01 * n, (name, n255)
        assert name == "white" or n0 >= 0.01 * n, (name, n0)


@pytest.mark.parametrize("name,dtype", [("holes", np.uint8), ("holes", np.float32), ("tiny", np.float32)])
def test_holes_move_the_seam(name, dtype):
    base, holed = class_pair("synth", dtype)[1].as_tuple()[:4], class_pair(name, dtype)[1].as_tuple()[:4]
    print(name, base, holed)
    assert all(a != b for a, b in zip(base, holed)), (base, holed)
    if name == "tiny":  # the subnormals count for the scan, the -0.0f do not: fewer zeros than `holes` has
        assert holed[1] > class_pair("holes", dtype)[1].n_a


def test_tiny_holds_subnormals_and_negative_zero():
    img = H.tiny(97, 33, np.float32, 4)
    bits = img.view(np.uint32)
    assert ((bits & 0x7F800000 == 0) & (bits & 0x007FFFFF != 0) & (bits >> 31 == 0)).any() and ((bits & 0x7F800000 == 0) & (bits & 0x007FFFFF != 0) & (bits >> 31 == 1)).any()
    assert (bits == 0x80000000).any() and not (bits == 0).any() and np.isfinite(img).all() and np.abs(img).max() < 2 ** 20


def test_band_gives_a_flagged_tile_column_between_data(oracle):
    """A flagged G tile column (g_flags_ref's rule, level 1) with data columns on both sides, at a canvas 1600 wide."""
    canvas = (1600, 128, 100, 300)
    r = H.map_pair("near", canvas, np.uint8, "band", "band", 3)
    a, b = oracle.warp(r["F"], r["p"], 0.0, 0.0, 1600, 128), oracle.move(r["M"], 0, 0, 1600, 128)
    assert g_flags_ref.flagged_columns(oracle, a, b)[0] > 0
    _, lw, lh = oracle.pyramid_levels(1600, 128, g_flags_ref.OPTS["level_rule"])
    g1 = oracle.decimate(oracle.blur(a.astype(np.float32)), lw[1], lh[1])
    nc = g_flags_ref.tile_columns(lw[1])
    zero = [not g1[0, :, t * 64:(t + 1) * 64].view(np.uint32).any() for t in range(nc)]
    flagged = [t for t in range(1, nc - 1) if zero[t - 1] and zero[t] and zero[t + 1]]
    assert [t for t in flagged if not all(zero[:t]) and not all(zero[t + 1:])], (zero, flagged)  # data to the left and to the right


# ---- c ---------------------------------------------------------------------------------------------------------------------------
def classes_of(name, canvas=H.PAIR_CANVAS, px=4):
    cw, ch, x0, _ = canvas
    fw, fh, p, offx, offy = H.map_case(name, cw, ch, x0, cw - x0)
    return R.classes(p, offx, offy, fw, fh, cw, ch, px) + ((p, offx, offy, fw, fh, cw, ch),)


@pytest.mark.parametrize("name", ["mirror_x", "transpose", "minify2", "magnify2"])
def test_maps_without_runs_have_general_tiles_only(name):
    counts, _, _ = classes_of(name)
    assert counts[1] == 0 and counts[2] == 0 and counts[3] > 0, counts


def test_stretch256_has_patched_tiles_inside_the_frame():
    counts, cls, (p, offx, offy, fw, fh, cw, ch) = classes_of("stretch256")
    off = R.offsets(p, offx, offy, fw, fh, cw, ch)
    inside = [(b, t) for b in range(cls.shape[0]) for t in range(cls.shape[1]) if 1 <= cls[b, t] <= R.MAX_PATCHES
              and (b + 1) * 64 <= ch and (t + 1) * 64 <= cw and (off[b * 64:(b + 1) * 64, t * 64:(t + 1) * 64] != 2 ** 32 - 4).all()]
    print(counts, inside[:4])
    assert inside  # tiles of 1 .. 64 patches that no edge of the frame touches


def test_trunc_reads_column_and_row_zero_twice():
    _, _, (p, offx, offy, fw, fh, cw, ch) = classes_of("trunc")
    off = R.offsets(p, offx, offy, fw, fh, cw, ch)
    x0 = H.PAIR_CANVAS[2]
    assert off[5, x0] == off[5, x0 + 1] == 4 * 4 * fw and off[5, x0 - 1] == 2 ** 32 - 4  # X = -0.5 and 0.5 -> column 0, -1.5 -> outside
    assert (off[0] == off[1]).all() and off[0, x0 + 9] == 4 * 8


# ---- d ---------------------------------------------------------------------------------------------------------------------------
def every_map():
    maps = []
    for canvas in CANVASES:
        cw, ch, x0, _ = canvas
        for name in H.MAP_CLASSES + ("fold",):
            fw, fh, p, offx, offy = H.map_case(name, cw, ch, x0, cw - x0)
            for px in (4, 1) if fh > 0 else ():  # (the short frame of `offsets` does not exist on the 71-row canvas)
                maps.append((p, offx, offy, fw, fh, cw, ch, px))
    return maps


def test_the_library_rule_on_hard_maps(st):
    seen = [0, 0, 0, 0]
    for p, offx, offy, fw, fh, cw, ch, px in every_map():
        counts, cls = R.classes(p, offx, offy, fw, fh, cw, ch, px)
        got, gcls = st.capi.src_run_classes(p, offx, offy, fw, fh, cw, ch, px)
        assert got == counts and np.array_equal(gcls, cls), (p, offx, offy, fw, fh, cw, ch, px)
        seen = [a + b for a, b in zip(seen, counts)]
    assert all(v > 0 for v in seen), seen


def test_the_rule_under_sanitizers_on_hard_maps(tmp_path):
    exe = os.path.join(str(tmp_path), "src_runs_dump")
    subprocess.check_call([host_compiler(), "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "computervisionimagestich2_amd", "csrc"), "-o", exe, os.path.join(HERE, "src_runs_dump.cpp")])
    maps = every_map()
    path = os.path.join(str(tmp_path), "maps.txt")
    with open(path, "w") as f:
        for p, offx, offy, fw, fh, cw, ch, px in maps:
            f.write(" ".join([float(v).hex() for v in p] + [float(offx).hex(), float(offy).hex()] + [str(v) for v in (fw, fh, cw, ch, px)]) + "\n")
    r = subprocess.run([exe, path], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = r.stdout.splitlines()
    assert len(lines) == len(maps)
    for (p, offx, offy, fw, fh, cw, ch, px), line in zip(maps, lines):
        counts, cls = R.classes(p, offx, offy, fw, fh, cw, ch, px)
        got = line.split()
        assert tuple(int(v) for v in got[:4]) == counts and (got[4] if len(got) > 4 else "") == cls.tobytes().hex(), (p, offx, offy, fw, fh, cw, ch, px)


# ---- profiles/hard_inputs.txt ----------------------------------------------------------------------------------------------------
def profile_text(records):
    lines = ["Counts of tests/hard_inputs.py on the CPU oracle (tests/test_hard_inputs_host.py prints this file).", "",
             "Clamped samples of the oracle's output, one pair at %d x %d under the map `near`, uint8:" % H.PAIR_CANVAS[:2],
             "class        == 255   == 0 inside the footprints    samples"]
    for name in ("synth",) + H.U8_CLASSES:
        lines.append("%-10s %8d %28d %10d" % ((name,) + clamp_counts(name)))
    lines += ["", "The hard-content table: items (case, pixel type, slot) per class, and the items the oracle refuses:", "class      type     items refused"]
    per_class, refused = collections.Counter(), collections.Counter()
    for index, dtype, j in used_items(records):
        k = (H.item_class(index, dtype, j), np.dtype(dtype).name)
        per_class[k] += 1
        refused[k] += H.stated_rc(index, dtype, j) != 0
    lines += ["%-10s %-8s %5d %7d" % (k[0], k[1], v, refused[k]) for k, v in sorted(per_class.items())]
    lines += ["", "rc of the refused items (every other item: 0):"] + ["%s %s slot %d: %d" % (k + (v,)) for k, v in sorted(H.REFUSED.items())]
    lines += ["", "rc of the map classes at %d x %d (pairs: synthetic frames; mix: binary frames over holes mosaics), uint8 / float32:" % H.PAIR_CANVAS[:2]]
    for i, name in enumerate(H.MAP_CLASSES + tuple(H.REFUSAL_CLASSES)):
        row = []
        for fr, mo in (("synth", "synth"), ("binary", "holes")):
            row += [H.pair_oracle(H.map_pair(name, H.PAIR_CANVAS, dt, fr, mo, seed=i if name in H.MAP_CLASSES else 0))[0] for dt in (np.uint8, np.float32)]
        lines.append("%-11s pairs %2d / %2d   mix %2d / %2d" % ((name,) + tuple(row)))
    lines += ["", "rc of every map class with every uint8 content class in frame and mosaic, seed 5 (checker: the first phase of 0 .. 3 that is accepted):",
              "%-11s" % "" + "".join("%10s" % c for c in H.U8_CLASSES)]
    for name in H.MAP_CLASSES + ("fold",):
        row = []
        for cls in H.U8_CLASSES:
            rcs = []
            for phase in range(4 if cls == "checker" else 1):
                r = H.map_pair(name, H.PAIR_CANVAS, np.uint8, cls, cls, 5)
                if cls == "checker":
                    r["F"], r["M"] = H.checker(r["F"].shape[2], r["F"].shape[1], np.uint8, phase=phase >> 1), H.checker(r["M"].shape[2], r["M"].shape[1], np.uint8, phase=phase & 1)
                rcs.append(H.pair_oracle(r)[0])
            row.append(0 if 0 in rcs else rcs[0])
        lines.append("%-11s" % name + "".join("%10d" % v for v in row))
    return "\n".join(lines) + "\n"


if __name__ == "__main__":
    import tempfile
    print(profile_text(build_records(tempfile.mkdtemp())), end="")
