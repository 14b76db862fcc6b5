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

    sift_edges.npz   `dense` (760 x 600: anisotropic Gaussian bumps of both signs on a jittered 6 px grid over mid-grey) under the
                     defaults and automatic octaves, and its crops of sift_ref.EDGE_CROPS (380 x 300 down to 1 x 1) under both, the
                     two shallow ones and 200 x 160 under octaves = 6 as well
    sift_edges2.npz  `strip` (the same construction at 4096 x 20) and its transpose, `squares` (80 x 80, axis-aligned squares)
                     under the defaults and (auto octaves, 3 levels), and `f32` (a crop of dense scaled and jittered to negative,
                     fractional and > 255 float32 samples)
                     per case of sift_ref.EDGE_CASES: kp, fkp, angle, oct (the octaves the reference ran), desc_crc, desc_sha,
                     and desc in full up to sift_ref.EDGE_FULL_ROWS rows; the images are stored (their generator uses exp)

    python tests/golden/make_sift_goldens.py          everything
    python tests/golden/make_sift_goldens.py edges    sift_edges*.npz only
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


EDGE_SEED = 20261018


def bumps(rng, w, h, spacing=6, jitter=2.0):
    """Mid-grey plus one anisotropic, rotated Gaussian bump of either sign per cell of a jittered grid."""
    img = np.full((h, w), 128.0)
    for gy in range(spacing // 2, h + spacing // 2, spacing):
        for gx in range(spacing // 2, w + spacing // 2, spacing):
            cx, cy = gx + rng.uniform(-jitter, jitter), gy + rng.uniform(-jitter, jitter)
            su, sv, th = rng.uniform(1.2, 3.0), rng.uniform(1.2, 3.0), rng.uniform(0, np.pi)
            amp = rng.uniform(60, 120) * (1 if rng.random() < 0.5 else -1)
            r = 12
            x0, x1, y0, y1 = max(int(cx) - r, 0), min(int(cx) + r + 1, w), max(int(cy) - r, 0), min(int(cy) + r + 1, h)
            if x0 >= x1 or y0 >= y1:
                continue
            yy, xx = np.mgrid[y0:y1, x0:x1]
            u = (xx - cx) * np.cos(th) + (yy - cy) * np.sin(th)
            v = -(xx - cx) * np.sin(th) + (yy - cy) * np.cos(th)
            img[y0:y1, x0:x1] += amp * np.exp(-0.5 * ((u / su) ** 2 + (v / sv) ** 2))
    return np.clip(np.rint(img), 0, 255).astype(np.uint8)


def edge_images():
    rng = np.random.default_rng(EDGE_SEED)
    dense = bumps(rng, 760, 600)
    strip = bumps(rng, 4096, 20)
    squares = np.full((80, 80), 110, np.uint8)
    for k, (cx, cy) in enumerate((x, y) for y in (13, 40, 66) for x in (14, 39, 66)):  # apart, so that each keeps its symmetry
        r = int(rng.integers(2, 9))
        squares[cy - r:cy + r + 1, cx - r:cx + r + 1] = 215 if k % 2 else 30
    x0, y0, w, h = R.EDGE_CROPS["c200x160"]
    f32 = ((dense[y0:y0 + h, x0:x0 + w].astype(np.float64) - 128) * 3.7 + rng.random((h, w))).astype(np.float32)
    return dict(dense=dense, strip=strip, squares=squares, f32=f32)


def edges(L):
    imgs = edge_images()
    Z = [{"img_dense": imgs["dense"]}, {f"img_{k}": imgs[k] for k in ("strip", "squares", "f32")}]
    for name, image, o in R.EDGE_CASES:
        z = Z[R.EDGE_FILES.index(R.edge_file(image))]
        img = R.edge_image(z, image)
        r = R.reference_sift(L, img, **o)
        z[f"{name}_kp"], z[f"{name}_fkp"], z[f"{name}_angle"], z[f"{name}_oct"] = r["kp"], r["fkp"], r["angle"], np.int32(r["octaves"])
        z[f"{name}_desc_crc"], z[f"{name}_desc_sha"] = R.row_crcs(r["desc"]), np.array(R.sha(r["desc"]))
        if len(r["desc"]) <= R.EDGE_FULL_ROWS:
            z[f"{name}_desc"] = r["desc"]
        per = np.bincount(r["kp"]["o"], minlength=1) if len(r["kp"]) else []
        print(f"{name}: {img.shape[1]} x {img.shape[0]} {img.dtype} {o}: {r['octaves']} octaves, keypoints {list(per)}, "
              f"{len(r['desc'])} features, most angles {np.bincount(r['fkp']).max() if len(r['fkp']) else 0}")
    for z, f in zip(Z, R.EDGE_FILES):
        np.savez_compressed(os.path.join(HERE, f), **z)


def sizes():
    for f in sorted(os.listdir(HERE)):
        if f.startswith("sift_") and f.endswith(".npz"):
            size = os.path.getsize(os.path.join(HERE, f))
            assert size < 1 << 20, (f, size)
            print(f, size)


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
    if sys.argv[1:] == ["edges"]:
        edges(L)
        return sizes()
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
    edges(L)
    sizes()


if __name__ == "__main__":
    main()
