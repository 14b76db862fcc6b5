#!/usr/bin/env python3
"""Generates the descriptor-matching fixtures under tests/golden/ from the REFERENCE ITSELF.

Runs only where oracle/_ref/libref_hotpath.so has been built (the reference's own functions, VLFeat included, compiled in place
by oracle/Makefile); it uses nothing but that library's exported symbols through ctypes, and is not run by the tests.

For each committed frame tests/golden/input/{1..4}.bmp it runs what ImageProcess's constructor does (ImageProcess.cpp:18-20):
ref_project_u8, ref_gray_u8, then siftAlgorithm's VLFeat sequence (:44-99: 4 octaves, 2 levels, first octave 0, every
orientation) and records
    match_frame<i>.npz   desc     (n, 128) float32 descriptors in insertion order
                         x, y     (n,) float32 keypoint coordinates in insertion order
                         map_idx  indices into desc in the std::map's order (lexicographic, an identical descriptor once --
                                  the first inserted), computed here with Python's tuple ordering
For the 12 ordered frame pairs (data = frame i, queries = frame j) it runs getImgPair's sequence (:273-351):
vl_kdforest_new(float, 128, 1 tree, L1), build, new_searcher, query(..., 2, ...) per query, and records per query the
index of neighbour 0 and both distances, and the accepted (data index, query index) list (ratio < 0.5):
    match_pairs.npz      p<i><j>_nn, p<i><j>_d0, p<i><j>_d1, p<i><j>_pairs, counts (4 x 4)
The same for synthetic SIFT-like sets (sparse components in [0, 1), duplicated rows, exact ties, sizes 1, 2, 3):
    match_synth.npz      s<k>_db, s<k>_query, s<k>_nn, s<k>_d0, s<k>_d1, s<k>_pairs
and _vl_distance_l1_f itself on random vectors (values inside and outside [0, 1)):
    match_l1.npz         x, y (m, 128) float32, dist (m,) float32

    python tests/golden/make_match_goldens.py
"""
import ctypes as C
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF_SO = os.path.join(ROOT, "oracle", "_ref", "libref_hotpath.so")
sys.path.insert(0, ROOT)

VL_TYPE_FLOAT, VL_DIST_L1, VL_ERR_EOF = 1, 0, 5
DIM = 128


class VlSiftKeypoint(C.Structure):  # vl/sift.h:19-31
    _fields_ = [("o", C.c_int), ("ix", C.c_int), ("iy", C.c_int), ("is_", C.c_int),
                ("x", C.c_float), ("y", C.c_float), ("s", C.c_float), ("sigma", C.c_float)]


class VlSiftFilt(C.Structure):  # vl/sift.h:38-78 (only `keys` / `nkeys` are read; the accessors are inline, not exported)
    _fields_ = [("sigman", C.c_double), ("sigma0", C.c_double), ("sigmak", C.c_double), ("dsigma0", C.c_double),
                ("width", C.c_int), ("height", C.c_int), ("O", C.c_int), ("S", C.c_int), ("o_min", C.c_int),
                ("s_min", C.c_int), ("s_max", C.c_int), ("o_cur", C.c_int),
                ("temp", C.c_void_p), ("octave", C.c_void_p), ("dog", C.c_void_p),
                ("octave_width", C.c_int), ("octave_height", C.c_int),
                ("gaussFilter", C.c_void_p), ("gaussFilterSigma", C.c_double), ("gaussFilterWidth", C.c_size_t),
                ("keys", C.POINTER(VlSiftKeypoint)), ("nkeys", C.c_int), ("keys_res", C.c_int)]


class VlKDForestNeighbor(C.Structure):  # vl/kdtree.h:60-63
    _fields_ = [("distance", C.c_double), ("index", C.c_size_t)]


def load():
    L = C.CDLL(REF_SO)
    L.vl_sift_new.restype = C.POINTER(VlSiftFilt)
    L.vl_sift_new.argtypes = [C.c_int] * 5
    L.vl_sift_process_first_octave.argtypes = [C.POINTER(VlSiftFilt), C.c_void_p]
    L.vl_sift_process_next_octave.argtypes = [C.POINTER(VlSiftFilt)]
    L.vl_sift_detect.argtypes = [C.POINTER(VlSiftFilt)]
    L.vl_sift_calc_keypoint_orientations.argtypes = [C.POINTER(VlSiftFilt), C.POINTER(C.c_double), C.POINTER(VlSiftKeypoint)]
    L.vl_sift_calc_keypoint_descriptor.argtypes = [C.POINTER(VlSiftFilt), C.POINTER(C.c_float), C.POINTER(VlSiftKeypoint),
                                                   C.c_double]
    L.vl_sift_calc_keypoint_descriptor.restype = None
    L.vl_sift_delete.argtypes = [C.POINTER(VlSiftFilt)]
    L.vl_sift_delete.restype = None
    L.vl_kdforest_new.restype = C.c_void_p
    L.vl_kdforest_new.argtypes = [C.c_uint32, C.c_size_t, C.c_size_t, C.c_int]
    L.vl_kdforest_build.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p]
    L.vl_kdforest_build.restype = None
    L.vl_kdforest_new_searcher.restype = C.c_void_p
    L.vl_kdforest_new_searcher.argtypes = [C.c_void_p]
    L.vl_kdforestsearcher_query.restype = C.c_size_t
    L.vl_kdforestsearcher_query.argtypes = [C.c_void_p, C.POINTER(VlKDForestNeighbor), C.c_size_t, C.c_void_p]
    L.vl_kdforestsearcher_delete.argtypes = [C.c_void_p]
    L.vl_kdforestsearcher_delete.restype = None
    L.vl_kdforest_delete.argtypes = [C.c_void_p]
    L.vl_kdforest_delete.restype = None
    L._vl_distance_l1_f.restype = C.c_float
    L._vl_distance_l1_f.argtypes = [C.c_size_t, C.c_void_p, C.c_void_p]
    return L


def sift(L, gray):
    """siftAlgorithm (ImageProcess.cpp:44-99) on a (h, w) uint8 gray image: descriptors and x, y in insertion order."""
    h, w = gray.shape
    img = np.ascontiguousarray(gray, np.float32)
    f = L.vl_sift_new(w, h, 4, 2, 0)
    descs, xs, ys = [], [], []
    if L.vl_sift_process_first_octave(f, img.ctypes.data) != VL_ERR_EOF:
        while True:
            L.vl_sift_detect(f)
            for i in range(f.contents.nkeys):
                kp = VlSiftKeypoint.from_buffer_copy(f.contents.keys[i])
                angles = (C.c_double * 4)()
                n = L.vl_sift_calc_keypoint_orientations(f, angles, C.byref(kp))
                for j in range(n):
                    d = (C.c_float * DIM)()
                    L.vl_sift_calc_keypoint_descriptor(f, d, C.byref(kp), angles[j])
                    descs.append(np.frombuffer(d, np.float32).copy())
                    xs.append(kp.x)
                    ys.append(kp.y)
            if L.vl_sift_process_next_octave(f) == VL_ERR_EOF:
                break
    L.vl_sift_delete(f)
    return np.array(descs, np.float32).reshape(-1, DIM), np.array(xs, np.float32), np.array(ys, np.float32)


def map_order(desc):
    """std::map<std::vector<float>, ...>::insert in insertion order: Python tuples of floats compare lexicographically with <,
    and -0.0 == 0.0 hash and compare equal, as the map's equivalence treats them."""
    first = {}
    for i, row in enumerate(desc.tolist()):
        first.setdefault(tuple(row), i)
    return np.array([first[k] for k in sorted(first)], np.int32)


def kdforest_pairs(L, db, query, ratio=0.5):
    """getImgPair's sequence (ImageProcess.cpp:280-343): per query (nn0, d0, d1) and the accepted (data, query) list."""
    db = np.ascontiguousarray(db, np.float32)
    query = np.ascontiguousarray(query, np.float32)
    forest = L.vl_kdforest_new(VL_TYPE_FLOAT, DIM, 1, VL_DIST_L1)
    L.vl_kdforest_build(forest, len(db), db.ctypes.data)
    searcher = L.vl_kdforest_new_searcher(forest)
    nb = (VlKDForestNeighbor * 2)()
    nq = len(query)
    nn, d0, d1, acc = np.empty(nq, np.int32), np.empty(nq, np.float32), np.empty(nq, np.float32), []
    for q in range(nq):
        L.vl_kdforestsearcher_query(searcher, nb, 2, query[q].ctypes.data)
        with np.errstate(divide="ignore", invalid="ignore"):
            r = np.float32(np.float64(nb[0].distance) / np.float64(nb[1].distance))  # float ratio = double / double
        for v in (nb[0].distance, nb[1].distance):
            assert np.isnan(v) or float(np.float32(v)) == v  # each distance is a float sum held in a double
        nn[q] = nb[0].index
        d0[q], d1[q] = nb[0].distance, nb[1].distance
        if r < ratio:
            acc.append((nb[0].index, q))
    L.vl_kdforestsearcher_delete(searcher)
    L.vl_kdforest_delete(forest)
    return nn, d0, d1, np.array(acc, np.int32).reshape(-1, 2)


def synth_sets(rng):
    """SIFT-like (db, query) sets, every component in [0, 1)."""
    def sparse(n, levels=8, p_zero=0.85):
        v = rng.integers(1, levels, size=(n, DIM)).astype(np.float32) / levels
        v[rng.random((n, DIM)) < p_zero] = 0
        return v

    def dense(n):
        return (rng.random((n, DIM), dtype=np.float32) * 0.25).astype(np.float32)

    out = []
    db = sparse(300)
    near = db[:100].copy()
    near[:, ::16] = sparse(100)[:, ::16]  # a few components changed: clear nearest neighbours, many accepted
    out.append((db, np.concatenate([sparse(100), near])))  # many exact ties
    base = dense(60)
    out.append((base[rng.integers(0, 60, 120)], np.concatenate([base[:20], dense(40)])))  # duplicated rows, shared rows (d = 0)
    t = sparse(40, levels=2, p_zero=0.97)
    out.append((np.concatenate([t, t]), t.copy()))              # every nearest distance tied (0/0 or d0 == d1)
    q = dense(50)
    for n in (1, 2, 3):
        out.append((dense(n), q))
    out.append((dense(200), dense(1)))
    return out


def main():
    L = load()
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from oracle_lib import Reference
    R = Reference()
    frames = []
    for i in range(1, 5):
        rgb = R.load_bmp(os.path.join(HERE, "input", f"{i}.bmp"))  # (3, h, w) uint8
        proj = np.empty_like(rgb)
        assert R.lib.ref_project_u8(rgb.ctypes.data_as(C.c_void_p), rgb.shape[2], rgb.shape[1], proj.ctypes.data_as(C.c_void_p)) == 0
        gray = np.empty(rgb.shape[1:], np.uint8)
        assert R.lib.ref_gray_u8(proj.ctypes.data_as(C.c_void_p), rgb.shape[2], rgb.shape[1], gray.ctypes.data_as(C.c_void_p)) == 0
        desc, x, y = sift(L, gray)
        idx = map_order(desc)
        np.savez_compressed(os.path.join(HERE, f"match_frame{i}.npz"), desc=desc, x=x, y=y, map_idx=idx)
        frames.append(desc[idx])
        print(f"frame {i}: {len(desc)} descriptors, {len(idx)} distinct, max component {desc.max():.4f}")
    Z = {}
    counts = np.zeros((4, 4), np.int32)
    for i in range(4):
        for j in range(4):
            if i == j:
                continue
            nn, d0, d1, acc = kdforest_pairs(L, frames[i], frames[j])
            Z[f"p{i}{j}_nn"], Z[f"p{i}{j}_d0"], Z[f"p{i}{j}_d1"], Z[f"p{i}{j}_pairs"] = nn, d0, d1, acc
            counts[i, j] = len(acc)
    Z["counts"] = counts
    np.savez_compressed(os.path.join(HERE, "match_pairs.npz"), **Z)
    print("getImgPair counts:\n", counts)
    rng = np.random.default_rng(20261016)
    S = {}
    for k, (db, q) in enumerate(synth_sets(rng)):
        nn, d0, d1, acc = kdforest_pairs(L, db, q)
        S[f"s{k}_db"], S[f"s{k}_query"], S[f"s{k}_nn"], S[f"s{k}_d0"], S[f"s{k}_d1"], S[f"s{k}_pairs"] = db, q, nn, d0, d1, acc
        print(f"synthetic {k}: {len(db)} x {len(q)}: {len(acc)} accepted")
    np.savez_compressed(os.path.join(HERE, "match_synth.npz"), **S)
    x = np.concatenate([rng.random((48, DIM), dtype=np.float32), (rng.standard_normal((16, DIM)) * 4).astype(np.float32)])
    y = np.concatenate([rng.random((48, DIM), dtype=np.float32), (rng.standard_normal((16, DIM)) * 4).astype(np.float32)])
    dist = np.array([L._vl_distance_l1_f(DIM, x[m].ctypes.data, y[m].ctypes.data) for m in range(len(x))], np.float32)
    np.savez_compressed(os.path.join(HERE, "match_l1.npz"), x=x, y=y, dist=dist)
    for f in sorted(os.listdir(HERE)):
        if f.startswith("match_") and f.endswith(".npz"):
            size = os.path.getsize(os.path.join(HERE, f))
            assert size < 1 << 20, (f, size)
            print(f, size)


if __name__ == "__main__":
    main()
