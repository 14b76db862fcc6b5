#!/usr/bin/env python3
"""Generates the SIFT fixtures under tests/golden/ from the REFERENCE ITSELF.

Runs only where oracle/_ref/libref_hotpath.so has been built; it uses nothing but that library's exported symbols through ctypes
(tests/sift_ref.py: VlSiftFilt is extended by the threshold fields so that options can be set), and is not run by the tests.

    sift_input.npz   for the committed frames tests/golden/input/{1..4}.bmp (ref_project_u8, ref_gray_u8, then siftAlgorithm's
                     sequence, ImageProcess.cpp:44-99): f<i>_kp (VlSiftKeypoint records after vl_sift_detect), f<i>_fkp (keypoint
                     index per feature row), f<i>_angle, f<i>_cand<o> (candidates before refinement: the 26-neighbour test
                     restated on the reference's DoG buffer, scan order), f<i>_dig (per octave the SHA-256 of the Gaussian
                     levels, the DoG levels and the gradient planes; "" where the reference never computed gradients),
                     f<i>_desc_sha (all descriptors; they must equal match_frame<i>.npz), the filters taps<S>_<k> with
                     taps<S>_sigma for 1, 2, 3 and 5 levels, and expn (fast_expn's table)
    sift_input2.npz  the projected gray of Input2/2.bmp (1210 x 907) with kp, fkp, angle, a CRC-32 per descriptor row and the
                     SHA-256 of the descriptor array
    sift_synth.npz   a 300 x 401 noise image under (auto octaves, 3 levels), (3, 5), (2, 1) and a non-zero peak threshold, a
                     constant image, and crops of 23 x 37, 17 x 9 and 64 x 65: kp, fkp, angle, desc in full per case

    python tests/golden/make_sift_goldens.py
"""
import ctypes as C
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import sift_ref as R  # noqa: E402


def synth_images():
    rng = np.random.default_rng(20261017)
    base = rng.random((401, 300))
    k = np.array([1, 4, 6, 4, 1], np.float64) / 16  # a little correlation, so that extrema survive the edge test
    for axis in (0, 1):
        base = sum(np.roll(base, s - 2, axis) * k[s] for s in range(5))
    base = (base - base.min()) / (base.max() - base.min())
    noise = np.clip(np.rint(base * 255), 0, 255).astype(np.uint8)
    return dict(noise=noise, const=np.full((40, 56), 97, np.uint8), c23x37=noise[:37, :23].copy(), c17x9=noise[50:59, 40:57].copy(),
                c64x65=noise[100:165, 100:164].copy())


def projected_gray(Ref, path):
    rgb = Ref.load_bmp(path)
    proj = np.empty_like(rgb)
    assert Ref.lib.ref_project_u8(rgb.ctypes.data_as(C.c_void_p), rgb.shape[2], rgb.shape[1], proj.ctypes.data_as(C.c_void_p)) == 0
    gray = np.empty(rgb.shape[1:], np.uint8)
    assert Ref.lib.ref_gray_u8(proj.ctypes.data_as(C.c_void_p), rgb.shape[2], rgb.shape[1], gray.ctypes.data_as(C.c_void_p)) == 0
    return gray


def main():
    from oracle_lib import Reference
    L = R.load_reference()
    Ref = Reference()
    Z = {"expn": R.reference_expn(L)}
    for S in (1, 2, 3, 5):
        taps = R.reference_taps(L, S)
        Z[f"taps{S}_sigma"] = np.array([s for s, _ in taps], np.float64)
        for k, (_, t) in enumerate(taps):
            Z[f"taps{S}_{k}"] = t
    for i in range(1, 5):
        gray = projected_gray(Ref, os.path.join(HERE, "input", f"{i}.bmp"))
        r = R.reference_sift(L, gray, dump=True)
        old = np.load(os.path.join(HERE, f"match_frame{i}.npz"))
        assert R.same_bits(old["desc"], r["desc"]) and R.same_bits(old["x"], r["kp"]["x"][r["fkp"]])
        Z[f"f{i}_kp"], Z[f"f{i}_fkp"], Z[f"f{i}_angle"], Z[f"f{i}_desc_sha"] = r["kp"], r["fkp"], r["angle"], np.array(R.sha(r["desc"]))
        dig = []
        for o in sorted(r["gauss"]):
            Z[f"f{i}_cand{o}"] = r["cand"][o]
            dig.append([R.sha(r["gauss"][o]), R.sha(r["dog"][o]), R.sha(r["grad"][o]) if o in r["grad"] else ""])
        Z[f"f{i}_dig"] = np.array(dig)
        print(f"frame {i}: {gray.shape[1]} x {gray.shape[0]}, {len(r['kp'])} keypoints, {len(r['desc'])} features, candidates "
              f"{[len(r['cand'][o]) for o in sorted(r['cand'])]}")
    np.savez_compressed(os.path.join(HERE, "sift_input.npz"), **Z)
    gray = projected_gray(Ref, os.path.join(os.environ.get("REF", "/root/reference"), "Input2", "2.bmp"))  # REF as in oracle/Makefile
    r = R.reference_sift(L, gray)
    np.savez_compressed(os.path.join(HERE, "sift_input2.npz"), gray=gray, kp=r["kp"], fkp=r["fkp"], angle=r["angle"],
                        desc_crc=R.row_crcs(r["desc"]), desc_sha=np.array(R.sha(r["desc"])))
    print(f"Input2/2: {gray.shape[1]} x {gray.shape[0]}, {len(r['kp'])} keypoints, {len(r['desc'])} features")
    S = {}
    imgs = synth_images()
    for k, v in imgs.items():
        S[f"img_{k}"] = v
    for name, img, o in R.SYNTH_CASES:
        r = R.reference_sift(L, imgs[img], **o)
        S[f"{name}_kp"], S[f"{name}_fkp"], S[f"{name}_angle"], S[f"{name}_desc"] = r["kp"], r["fkp"], r["angle"], r["desc"]
        print(f"{name}: {imgs[img].shape[1]} x {imgs[img].shape[0]} {o}: {len(r['kp'])} keypoints, {len(r['desc'])} features")
    np.savez_compressed(os.path.join(HERE, "sift_synth.npz"), **S)
    for f in sorted(os.listdir(HERE)):
        if f.startswith("sift_") and f.endswith(".npz"):
            size = os.path.getsize(os.path.join(HERE, f))
            assert size < 1 << 20, (f, size)
            print(f, size)


if __name__ == "__main__":
    main()
