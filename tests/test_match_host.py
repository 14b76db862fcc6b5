"""CPU: the numpy restatement of getImgPair's matcher (tests/match_ref.py) against the reference's recorded results
(tests/golden/match_*.npz, made by tests/golden/make_match_goldens.py), feature_order against the std::map order, and the
C ABI of the GPU matcher (exported, fails loudly without a device)."""
import ctypes as C
import os

import numpy as np
import pytest

import match_ref
from computervisionimagestich2_amd import pipeline

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
GOLD = os.path.join(HERE, "golden")
REF_SO = os.path.join(ROOT, "oracle", "_ref", "libref_hotpath.so")


def frames():
    out = []
    for i in range(1, 5):
        z = np.load(os.path.join(GOLD, f"match_frame{i}.npz"))
        out.append((z["desc"], z["x"], z["y"], z["map_idx"]))
    return out


def test_restatement_equals_recorded_l1_distance():
    z = np.load(os.path.join(GOLD, "match_l1.npz"))
    got = np.array([match_ref.l1_distances(z["x"][m:m + 1], z["y"][m:m + 1])[0, 0] for m in range(len(z["x"]))], np.float32)
    assert np.array_equal(got.view(np.uint32), z["dist"].view(np.uint32))


@pytest.mark.skipif(not os.path.exists(REF_SO), reason="the reference library is built only where its sources are")
def test_restatement_equals_live_vl_distance_l1():
    L = C.CDLL(REF_SO)
    L._vl_distance_l1_f.restype = C.c_float
    L._vl_distance_l1_f.argtypes = [C.c_size_t, C.c_void_p, C.c_void_p]
    rng = np.random.default_rng(7)
    x = np.concatenate([rng.random((200, 128), dtype=np.float32), (rng.standard_normal((56, 128)) * 100).astype(np.float32)])
    y = np.concatenate([rng.random((200, 128), dtype=np.float32), (rng.standard_normal((56, 128)) * 100).astype(np.float32)])
    ref = np.array([L._vl_distance_l1_f(128, x[m].ctypes.data, y[m].ctypes.data) for m in range(len(x))], np.float32)
    got = np.diagonal(match_ref.l1_distances(x, y))
    assert np.array_equal(got.view(np.uint32), ref.view(np.uint32))


def _same_f32(a, b):
    """bit-identical, NaN where the other is NaN"""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(a[~np.isnan(a)], b[~np.isnan(b)])


def _check_against_record(pairs, nn, d0, d1, r_pairs, r_nn, r_d0, r_d1):
    assert np.array_equal(pairs, r_pairs.reshape(-1, 2))
    assert _same_f32(d0, r_d0) and _same_f32(d1, r_d1)
    acc = pairs[:, 1]
    assert np.array_equal(nn[acc], r_nn[acc])  # the index of a rejected query is not pinned by the reference


def test_restatement_reproduces_recorded_kdforest_frames():
    z = np.load(os.path.join(GOLD, "match_pairs.npz"))
    F = [d[idx] for d, _, _, idx in frames()]
    counts = np.zeros((4, 4), np.int64)
    for i in range(4):
        for j in range(4):
            if i == j:
                continue
            res = match_ref.match(F[i], F[j])
            _check_against_record(*res, z[f"p{i}{j}_pairs"], z[f"p{i}{j}_nn"], z[f"p{i}{j}_d0"], z[f"p{i}{j}_d1"])
            counts[i, j] = len(res[0])
    assert np.array_equal(counts, z["counts"])
    assert counts[0, 1] == 87  # SURVEY.md's recorded count for getImgPair(imgs[0], imgs[1])


def test_restatement_reproduces_recorded_kdforest_synthetic():
    z = np.load(os.path.join(GOLD, "match_synth.npz"))
    k = 0
    while f"s{k}_db" in z:
        res = match_ref.match(z[f"s{k}_db"], z[f"s{k}_query"])
        _check_against_record(*res, z[f"s{k}_pairs"], z[f"s{k}_nn"], z[f"s{k}_d0"], z[f"s{k}_d1"])
        k += 1
    assert k >= 7


def test_feature_order_is_the_map_order(st):
    for desc, x, y, idx in frames():
        d, kp, got = pipeline.feature_order(desc, np.stack([x, y], 1))
        assert np.array_equal(got, idx)
        assert np.array_equal(d, desc[idx]) and np.array_equal(kp[:, 0], x[idx])
    # identical descriptors: the first inserted stays; -0.0 and +0.0 are the same key
    a = np.zeros((5, 128), np.float32)
    a[0, 3], a[1, 3], a[2, 3], a[3, 3], a[4, 3] = 0.5, 0.25, 0.5, -0.0, 0.0
    a[4, 5] = 0.0
    d, kp, got = pipeline.feature_order(a, np.arange(5))
    assert got.tolist() == [3, 1, 0]
    b = np.zeros((3, 128), np.float32)
    b[0, 0], b[1, 1], b[2, 0] = 0.1, 0.9, 0.1  # lexicographic: row 1 (0, 0.9, ...) < row 0 (0.1, ...)
    assert pipeline.feature_order(b)[2].tolist() == [1, 0]


def test_match_symbols_exported(st):
    lib = st.capi.lib()
    for n in ("stitch_match_l1_ratio", "stitch_dev_match_l1_ratio", "stitch_dev_match_l1_ratio_many"):
        assert hasattr(lib, n), n
    assert hasattr(st.capi, "match") and hasattr(pipeline, "match_counts") and hasattr(pipeline, "pair_lists")
    # device pointers go through ctypes as 64-bit pointers (an undeclared argument would be passed as a 32-bit int)
    assert lib.stitch_dev_match_l1_ratio.argtypes[0] is C.c_void_p and lib.stitch_dev_match_l1_ratio.argtypes[9] is C.c_void_p


def test_match_without_device_fails_loudly(st):
    import torch
    if torch.cuda.is_available():
        pytest.skip("a HIP device is present")
    d = np.zeros((4, 128), np.float32)
    with pytest.raises(st.StitchError) as e:
        st.capi.match(d, d)
    assert e.value.code == st.capi.ERR_NO_DEVICE
    desc = st.capi.MatchDesc()
    assert st.capi.lib().stitch_dev_match_l1_ratio_many(C.byref(desc), 1, C.c_double(0.5), None) == st.capi.ERR_NO_DEVICE
