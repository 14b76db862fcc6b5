"""CPU: csrc/k_sift.inc's own sift_* functions, compiled for the host by tests/sift_emulate.cpp, against what the reference's VLFeat
recorded (tests/golden/sift_*.npz, made by tests/golden/make_sift_goldens.py): the scale space, DoG and gradients by digest, the
candidate lists, and every bit of the keypoints, angles and descriptors.  The parity bar is zero differences; there is no
exemption file.  The library's host-side hooks (filters, fast_expn's table) are pinned to the recorded arrays as well."""
import ctypes as C
import os

import numpy as np
import pytest

import sift_ref as R
from computervisionimagestich2_amd import bmp, capi

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def emulator(tmp_path_factory):
    d = tmp_path_factory.mktemp("sift_emulate")
    return R.build_emulator(d), d


@pytest.fixture(scope="module")
def oracle():
    from oracle_lib import Oracle
    return Oracle()


def input_gray(oracle, i):
    """projection -> gray of a committed frame, through the CPU restatement (bit-exact with the reference, test_oracle_golden)."""
    rgb = bmp.load_bmp(os.path.join(GOLD, "input", f"{i}.bmp"))
    return oracle.gray(oracle.project(np.ascontiguousarray(rgb)))[0]


def check_features(got, z, prefix, what):
    assert R.same_bits(got["kp"], z[prefix + "kp"]), f"{what}: keypoints ({len(got['kp'])} vs {len(z[prefix + 'kp'])})"
    assert R.same_bits(got["fkp"], z[prefix + "fkp"]), f"{what}: feature -> keypoint"
    assert R.same_bits(got["angle"], z[prefix + "angle"]), f"{what}: angles"


def test_filters_and_table_equal_recorded():
    z = np.load(os.path.join(GOLD, "sift_input.npz"))
    lib = capi.lib()
    tab = np.zeros(257)
    lib.stitch_sift_expn_table(tab.ctypes.data_as(C.c_void_p))
    assert R.same_bits(tab, z["expn"])
    widths = []
    for S in (1, 2, 3, 5):
        for k, sigma in enumerate(z[f"taps{S}_sigma"]):
            taps = np.zeros(129, np.float32)
            W = lib.stitch_sift_filter(C.c_double(float(sigma)), taps.ctypes.data_as(C.c_void_p))
            assert R.same_bits(taps[:2 * W + 1], z[f"taps{S}_{k}"]), (S, k, sigma)
            if S == 2:
                widths.append(W)
    assert widths == [7, 7, 10, 13, 19]


@pytest.mark.parametrize("i", [1, 2, 3, 4])
def test_input_frame_equals_reference(emulator, oracle, i):
    exe, d = emulator
    z = np.load(os.path.join(GOLD, "sift_input.npz"))
    got = R.emulate(exe, input_gray(oracle, i), d, dump=True)
    dig = z[f"f{i}_dig"]
    assert len(dig) == 4
    for o in range(4):
        assert R.sha(got["gauss"][o]) == dig[o][0], f"frame {i} octave {o}: Gaussian levels"
        assert R.sha(got["dog"][o]) == dig[o][1], f"frame {i} octave {o}: DoG levels"
        assert (R.sha(got["grad"][o]) if o in got["grad"] else "") == dig[o][2], f"frame {i} octave {o}: gradients"
        assert R.same_bits(got["cand"][o], z[f"f{i}_cand{o}"]), f"frame {i} octave {o}: candidates"
    check_features(got, z, f"f{i}_", f"frame {i}")
    old = np.load(os.path.join(GOLD, f"match_frame{i}.npz"))
    assert R.sha(got["desc"]) == str(z[f"f{i}_desc_sha"]) and R.same_bits(got["desc"], old["desc"]), f"frame {i}: descriptors"
    assert R.same_bits(got["kp"]["x"][got["fkp"]], old["x"]) and R.same_bits(got["kp"]["y"][got["fkp"]], old["y"])
    assert R.same_bits(got["expn"], z["expn"])
    for (sigma, taps), k in zip(got["taps"][:5], range(5)):
        assert sigma == z["taps2_sigma"][k] and R.same_bits(taps, z[f"taps2_{k}"])


def test_input2_frame_equals_reference(emulator):
    exe, d = emulator
    z = np.load(os.path.join(GOLD, "sift_input2.npz"))
    assert z["gray"].shape == (907, 1210)
    got = R.emulate(exe, z["gray"], d)
    check_features(got, z, "", "Input2 frame")
    assert len(got["desc"]) == 2266
    bad = np.nonzero(R.row_crcs(got["desc"]) != z["desc_crc"])[0]
    assert len(bad) == 0, f"descriptor rows {bad[:8]} differ"
    assert R.sha(got["desc"]) == str(z["desc_sha"])


@pytest.mark.parametrize("name,img,opts", R.SYNTH_CASES, ids=[c[0] for c in R.SYNTH_CASES])
def test_options_and_small_frames_equal_reference(emulator, name, img, opts):
    exe, d = emulator
    z = np.load(os.path.join(GOLD, "sift_synth.npz"))
    got = R.emulate(exe, z[f"img_{img}"], d, **opts)
    check_features(got, z, name + "_", name)
    assert R.same_bits(got["desc"], z[name + "_desc"]), f"{name}: descriptors"


def test_fixture_coverage():
    z = np.load(os.path.join(GOLD, "sift_synth.npz"))
    n = {c[0]: len(z[c[0] + "_desc"]) for c in R.SYNTH_CASES}
    assert n["const"] == n["s23x37"] == n["s17x9"] == 0 and n["s64x65"] > 0
    assert min(n["auto3"], n["o3l5"], n["o2l1"], n["peak"], n["norm"]) >= 30
    assert (z["norm_desc"] == 0).all(axis=1).any() and (z["norm_desc"] != 0).any()  # the norm threshold cuts some, not all


# ---- the edge fixtures (sift_edges*.npz): what only the GPU's launch logic can get wrong needs inputs that reach it ------------
@pytest.fixture(scope="module")
def edges():
    return {f: np.load(os.path.join(GOLD, f)) for f in R.EDGE_FILES}


def check_edge(got, z, name):
    """Every bit of a result (emulate()'s or sift_unpack()'s dict) against the case `name` of its fixture file z."""
    check_features(got, z, name + "_", name)
    assert got["desc"].shape == (len(z[name + "_fkp"]), R.DIM)
    bad = np.nonzero(R.row_crcs(got["desc"]) != z[name + "_desc_crc"])[0]
    assert len(bad) == 0, f"{name}: descriptor rows {bad[:8]} differ"
    assert R.sha(got["desc"]) == str(z[name + "_desc_sha"]), f"{name}: descriptors"
    if name + "_desc" in z:
        assert R.same_bits(got["desc"], z[name + "_desc"]), f"{name}: descriptors"


@pytest.mark.parametrize("name,img,opts", R.EDGE_CASES, ids=[c[0] for c in R.EDGE_CASES])
def test_edge_case_equals_reference(emulator, edges, name, img, opts):
    exe, d = emulator
    z = edges[R.edge_file(img)]
    image = R.edge_image(z, img)
    assert image.dtype == (np.float32 if img == "f32" else np.uint8)
    check_edge(R.emulate(exe, image, d, **opts), z, name)


def keypoints_per_octave(z, name, octaves=8):
    return np.bincount(z[name + "_kp"]["o"], minlength=octaves)


def test_edge_fixture_coverage(edges):
    """The edge fixtures reach what they were made for; conditions on the reference's own results, not measurements."""
    z, z2 = (edges[f] for f in R.EDGE_FILES)
    per = keypoints_per_octave(z, "dense")
    assert per[0] >= 2200 > R.GRID_LIMIT and per[2] > 0 and per[3] > 0, per  # a cap of 2 048 cuts inside octave 0
    assert len(z["dense_kp"]) <= 4096  # the capacity the GPU test gives it
    octs = [int(z[c + "_auto_oct"]) for c in R.MIXED_CALL]
    assert len(set(octs)) >= 3, octs
    later = [(a, b) for a in range(len(octs)) for b in range(a + 1, len(octs))
             if octs[b] > octs[a] and keypoints_per_octave(z, R.MIXED_CALL[b] + "_auto")[octs[a]:].any()]
    assert later, octs  # a frame listed after one with fewer octaves has a keypoint in an octave that one lacks
    for c, (x0, y0, w, h) in R.EDGE_CROPS.items():  # the reference runs every octave asked for, pixels or not
        assert int(z[c + "_oct"]) == 4 and int(z[c + "_auto_oct"]) == max(min(w, h).bit_length() - 4, 1)
    for c in ("c200x24", "c150x9", "c200x160"):
        w, h = R.EDGE_CROPS[c][2:]
        assert int(z[c + "_o6_oct"]) == 6 and (R.pixel_octaves(w, h, 6) < 6) == (c != "c200x160")  # h >> o reaches 0 first
    for c in ("squares", "squares_l3"):
        assert np.bincount(z2[c + "_fkp"]).max() == 4, c
    for c in ("strip", "stripT"):
        per = keypoints_per_octave(z2, c)
        assert per[0] > 0 and per[1] > 0, (c, per)
    assert z2["img_strip"].shape == (20, 4096)
    f = z2["img_f32"]
    assert f.dtype == np.float32 and f.min() < 0 and f.max() > 255 and (f != np.rint(f)).any() and len(z2["f32_kp"]) > 0
    for c in ("c3x2", "c1x1"):
        assert len(z[c + "_kp"]) == len(z[c + "_auto_kp"]) == 0
    zi = np.load(os.path.join(GOLD, "sift_input.npz"))  # the capacities of the per-frame GPU test come from these
    k, row = R.split_keypoint(zi, "f4_")  # a feat_cap of row + 1 falls between two angles of keypoint k
    assert zi["f4_fkp"][row] == zi["f4_fkp"][row + 1] == k and zi["f4_fkp"][row - 1] == k - 1 and row + 1 < len(zi["f4_fkp"])
    per = keypoints_per_octave(zi, "f1")
    assert per[0] > 100 and per[1:].sum() > 0  # a kp_cap of per[0] ends octave 0, one of 100 lies inside it


def sweep_crops():
    """48 crops of `dense`: each side drawn from 1..40 or 41..200, every combination of narrow / short / ordinary occurring."""
    rng = np.random.default_rng(4096)
    out = []
    for k in range(48):
        w, h = (int(rng.integers(1, 41)) if small else int(rng.integers(41, 201)) for small in ((k & 1) == 0, (k & 2) == 0))
        out.append((int(rng.integers(0, 760 - w + 1)), int(rng.integers(0, 600 - h + 1)), w, h))
    return out


@pytest.mark.skipif(not os.path.exists(R.REF_SO), reason="the reference library is built only where its sources are")
@pytest.mark.parametrize("opts", [dict(), dict(octaves=-1)], ids=["defaults", "auto"])
def test_crop_sweep_against_live_reference(emulator, edges, opts):
    exe, d = emulator
    L = R.load_reference()
    dense = edges[R.EDGE_FILES[0]]["img_dense"]
    found = 0
    for x0, y0, w, h in sweep_crops():
        img = np.ascontiguousarray(dense[y0:y0 + h, x0:x0 + w])
        got, ref = R.emulate(exe, img, d, **opts), R.reference_sift(L, img, **opts)
        for k in ("kp", "fkp", "angle", "desc"):
            assert R.same_bits(got[k], ref[k]), f"{w} x {h} at ({x0}, {y0}) {opts}: {k}"
        found += len(ref["desc"])
    assert found > 0
