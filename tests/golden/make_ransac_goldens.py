#!/usr/bin/env python3
"""Generates the RANSAC fixtures under tests/golden/ from the REFERENCE ITSELF.

Runs only where oracle/_ref/libref_hotpath.so has been built; it uses nothing but that library's exported symbols (and libc's
srand / rand for the recorded stream) through ctypes, and is not run by the tests.

ImageProcess::RANSAC (ImageProcess.cpp:395-436) is called as the C++ ABI lays the call out: a hidden pointer to the returned
Homography (9 doubles), a dummy `this` (the function reads no member) and a hand-made libstdc++ std::vector<ImgPair> -- three
pointers over an (n, 16) float32 array (ImgPair is two 32-byte VlSiftKeypoints; x, y are floats 4, 5 and 12, 13).  Every call
runs in a child process with a time limit: the reference never returns for n < 4 and terminates the process on an empty
consensus, so a list is sent to it only after the restatement (tests/ransac_ref.py) says that it has an answer.

    ransac_input.npz   for every ordered frame pair (i, j) of tests/golden/input whose accepted list getImgPair(imgs[i], imgs[j])
                       (match_pairs.npz) has >= 4 entries: in<i><j>_{sx,sy,dx,dy} = the ImgPair list (src = frame i's keypoint,
                       dst = frame j's), in<i><j>_p = RANSAC of it, in<i><j>_pm = RANSAC of its mirror
    ransac_synth.npz   s<k>_{sx,sy,dx,dy}, s<k>_p for seeded synthetic lists (sizes 4 .. 20000, outlier shares 0 .. 60 %, duplicated
                       points, winning lists of exactly 4 and of 1 .. 3 entries); d<k>_{sx,sy,dx,dy}, d<k>_status for lists
                       without an answer (n < 4, empty consensus), which the reference is never asked about
    rand_666666.npy    the first 4096 values of rand() after srand(666666), from glibc

    python tests/golden/make_ransac_goldens.py
"""
import ctypes as C
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF_SO = os.path.join(ROOT, "oracle", "_ref", "libref_hotpath.so")
sys.path.insert(0, os.path.join(ROOT, "tests"))
RANSAC_SYM = "_ZN12ImageProcess6RANSACERKSt6vectorI7ImgPairSaIS1_EE"


def call_reference(sx, sy, dx, dy):
    """In this process: ImageProcess::RANSAC on the list -> 8 doubles."""
    L = C.CDLL(REF_SO)
    fn = getattr(L, RANSAC_SYM)
    fn.restype = None
    fn.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    n = len(sx)
    pairs = np.zeros((n, 16), np.float32)
    pairs[:, 4], pairs[:, 5], pairs[:, 12], pairs[:, 13] = sx, sy, dx, dy
    vec = (C.c_void_p * 3)(pairs.ctypes.data, pairs.ctypes.data + pairs.nbytes, pairs.ctypes.data + pairs.nbytes)
    out = (C.c_double * 9)()
    this = (C.c_char * 256)()
    fn(C.addressof(out), C.addressof(this), C.addressof(vec))
    return np.array(out[:8], np.float64)


def reference(sx, sy, dx, dy, timeout=600):
    """The same in a child process with a time limit."""
    with tempfile.TemporaryDirectory() as tmp:
        f = os.path.join(tmp, "list.npy")
        np.save(f, np.stack([sx, sy, dx, dy]).astype(np.float32))
        out = subprocess.run([sys.executable, os.path.abspath(__file__), "--call", f], capture_output=True, text=True, timeout=timeout)
        if out.returncode != 0:
            raise RuntimeError(f"the reference ended with {out.returncode}: {out.stderr[-300:]}")
        return np.array([float.fromhex(t) for t in out.stdout.split()[-8:]], np.float64)


def synth_list(rng, n, outliers, dup=0.0, size=400.0):
    """n pairs related by a bilinear map plus sub-pixel noise; a share of outliers; a share of rows duplicated."""
    sx = (rng.random(n) * size).astype(np.float32)
    sy = (rng.random(n) * size).astype(np.float32)
    p = [1.02, 0.03, -1e-4, 35.0, -0.02, 0.98, 2e-4, -12.0]
    x, y = sx.astype(np.float64), sy.astype(np.float64)
    dx = (p[0] * x + p[1] * y + p[2] * x * y + p[3] + rng.normal(0, 0.6, n)).astype(np.float32)
    dy = (p[4] * x + p[5] * y + p[6] * x * y + p[7] + rng.normal(0, 0.6, n)).astype(np.float32)
    bad = rng.random(n) < outliers
    dx[bad] = (rng.random(int(bad.sum())) * size).astype(np.float32)
    dy[bad] = (rng.random(int(bad.sum())) * size).astype(np.float32)
    k = int(n * dup)
    if k:
        a, b = rng.integers(0, n, k), rng.integers(0, n, k)
        sx[a], sy[a], dx[a], dy[a] = sx[b], sy[b], dx[b], dy[b]
    return sx, sy, dx, dy


def scattered(rng, n, size=500.0):
    """Unrelated points: the four sampled pairs are a hypothesis' only inliers."""
    return tuple((rng.random(n) * size).astype(np.float32) for _ in range(4))


def on_a_line(rng, n, size=300.0):
    """Every src point on y = 0: every sample is singular (two pivots of 1e-20); at most the pivot rows' points fit."""
    sx = (rng.random(n) * size).astype(np.float32)
    return sx, np.zeros(n, np.float32), (rng.random(n) * size).astype(np.float32), (rng.random(n) * size).astype(np.float32)


def same_point(rng, n, size=300.0):
    """One src point n times with scattered dst points: identical rows, three pivots of 1e-20."""
    x, y = np.float32(rng.random() * size), np.float32(rng.random() * size)
    return np.full(n, x, np.float32), np.full(n, y, np.float32), (rng.random(n) * size).astype(np.float32), (rng.random(n) * size).astype(np.float32)


def three_on_a_line(seed=9000):
    """Src points on y = 0 with three dst points affine in x: a sample whose pivot rows are two of them fits exactly those three."""
    rng = np.random.default_rng(seed)
    n = int(rng.integers(5, 9))
    sx = (rng.random(n) * 300).astype(np.float32)
    dx, dy = (rng.random(n) * 300).astype(np.float32), (rng.random(n) * 300).astype(np.float32)
    k = rng.choice(n, 3, replace=False)
    dx[k], dy[k] = (0.9 * sx[k] + 20).astype(np.float32), (0.1 * sx[k] + 50).astype(np.float32)
    return sx, np.zeros(n, np.float32), dx, dy


def one_column(seed=20010):
    """Every src point on one vertical line, scattered dst points; with this seed one round keeps a single inlier (found by
    searching seeds with the restatement: most such lists have an empty consensus)."""
    rng = np.random.default_rng(seed)
    n = int(rng.integers(5, 10))
    sx, sy, dx, dy = ((rng.random(n) * 300).astype(np.float32) for _ in range(4))
    sx[:] = sx[0]
    return sx, sy, dx, dy


def main():
    import ransac_ref
    libc = C.CDLL("libc.so.6")
    libc.srand(666666)
    stream = np.array([libc.rand() for _ in range(4096)], np.int32)
    np.save(os.path.join(HERE, "rand_666666.npy"), stream)
    g = ransac_ref.rand_stream(666666)
    assert [next(g) for _ in range(4096)] == stream.tolist(), "the restated generator differs from glibc"

    def checked(name, lst):
        p, inl, info = ransac_ref.ransac(*lst)
        assert info[0] == ransac_ref.OK, (name, info)
        ref = reference(*lst)
        same = ransac_ref.same_p(p, ref)
        print(f"{name}: n {len(lst[0])}, winner round {info[2]} with {info[3]} inliers, {info[4]} draws, restatement "
              f"{'==' if same else '!='} reference")
        assert same, (name, p, ref)
        return ref

    frames = []
    for i in range(1, 5):
        z = np.load(os.path.join(HERE, f"match_frame{i}.npz"))
        frames.append((z["x"][z["map_idx"]], z["y"][z["map_idx"]]))
    mp = np.load(os.path.join(HERE, "match_pairs.npz"))
    Z = {}
    for i in range(4):
        for j in range(4):
            if i == j or len(mp[f"p{i}{j}_pairs"]) < 4:
                continue
            pr = mp[f"p{i}{j}_pairs"]
            lst = (frames[i][0][pr[:, 0]], frames[i][1][pr[:, 0]], frames[j][0][pr[:, 1]], frames[j][1][pr[:, 1]])
            for k, v in zip(("sx", "sy", "dx", "dy"), lst):
                Z[f"in{i}{j}_{k}"] = v
            Z[f"in{i}{j}_p"] = checked(f"frames {i}->{j}", lst)
            Z[f"in{i}{j}_pm"] = checked(f"frames {i}->{j} mirrored", (lst[2], lst[3], lst[0], lst[1]))
    np.savez_compressed(os.path.join(HERE, "ransac_input.npz"), **Z)

    rng = np.random.default_rng(20261016)
    lists = [synth_list(rng, n, o, d) for n, o, d in ((4, 0, 0), (5, 0.2, 0), (6, 0, 0), (9, 0.3, 0), (64, 0.4, 0.2), (300, 0.6, 0.1),
                                                      (1000, 0.4, 0.05), (5000, 0.5, 0.0), (20000, 0.3, 0.02), (300, 0.0, 0.5))]
    lists += [scattered(rng, n) for n in (4, 5, 6, 9, 12)]          # winning lists of exactly 4 entries (LU for the final fit too)
    few, empty = [], []
    for make, n in ((on_a_line, 5), (on_a_line, 7), (on_a_line, 10), (on_a_line, 20), (same_point, 5), (same_point, 8), (same_point, 13)):
        lst = make(rng, n)                                          # singular samples: winning lists of 1 .. 3 entries, or none
        info = ransac_ref.ransac(*lst)[2]
        if info[0] == ransac_ref.OK and 1 <= info[3] <= 3:
            few.append(lst)
        elif info[0] == ransac_ref.NO_CONSENSUS:
            empty.append(lst)
    lists += few
    lists += [three_on_a_line(), one_column()]                      # winning lists of 3 entries and of 1 entry (height < width)
    S = {}
    wins = []
    for k, lst in enumerate(lists):
        for key, v in zip(("sx", "sy", "dx", "dy"), lst):
            S[f"s{k}_{key}"] = v
        S[f"s{k}_p"] = checked(f"synthetic {k}", lst)
        wins.append(ransac_ref.ransac(*lst)[2][3])
    assert sum(w == 4 for w in wins) >= 3 and sum(1 <= w <= 3 for w in wins) >= 3 and {1, 2, 3} <= set(wins), wins
    inf = np.float32(np.inf)
    far = synth_list(rng, 50, 0.0)
    empty.append((far[0], far[1], np.full(50, inf, np.float32), far[3]))  # no finite distance anywhere
    empty.append((np.full(50, np.nan, np.float32), far[1], far[2], far[3]))
    degenerate = [(e, ransac_ref.NO_CONSENSUS) for e in empty] + [(synth_list(rng, n, 0.0), ransac_ref.TOO_FEW) for n in (0, 1, 2, 3)]
    for k, (lst, status) in enumerate(degenerate):
        assert ransac_ref.ransac(*lst)[2][0] == status
        for key, v in zip(("sx", "sy", "dx", "dy"), lst):
            S[f"d{k}_{key}"] = v
        S[f"d{k}_status"] = np.int32(status)
    print(f"{len(lists)} synthetic lists (winning counts {wins}), {len(degenerate)} without an answer")
    np.savez_compressed(os.path.join(HERE, "ransac_synth.npz"), **S)
    for f in ("ransac_input.npz", "ransac_synth.npz", "rand_666666.npy"):
        size = os.path.getsize(os.path.join(HERE, f))
        assert size < 1 << 20, (f, size)
        print(f, size)


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "--call":
        print(" ".join(float(v).hex() for v in call_reference(*np.load(sys.argv[2]))))
    else:
        main()
