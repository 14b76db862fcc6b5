"""GPU: map estimation (k_ransac.inc) against the reference's recorded maps (tests/golden/ransac_*.npz, bit for bit) and against
the restatement (tests/ransac_ref.py, itself pinned to the reference by tests/test_ransac_host.py) where the reference was not
recorded: other round counts, thresholds and seeds, large lists, mirrored lists, lists addressed through the matcher's device
output, and the panorama of the committed frames from their features alone."""
import hashlib
import json
import os

import numpy as np
import pytest

import ransac_ref
from computervisionimagestich2_amd import pipeline

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _fixture_lists():
    """(name, (sx, sy, dx, dy), recorded p or None, expected status)"""
    out = []
    z = np.load(os.path.join(GOLD, "ransac_input.npz"))
    for key in sorted(k[:-3] for k in z.files if k.endswith("_sx")):
        lst = tuple(z[f"{key}_{c}"] for c in ("sx", "sy", "dx", "dy"))
        out.append((key, lst, z[f"{key}_p"], ransac_ref.OK))
        out.append((key + " mirrored", (lst[2], lst[3], lst[0], lst[1]), z[f"{key}_pm"], ransac_ref.OK))
    z = np.load(os.path.join(GOLD, "ransac_synth.npz"))
    k = 0
    while f"s{k}_sx" in z:
        out.append((f"synthetic {k}", tuple(z[f"s{k}_{c}"] for c in ("sx", "sy", "dx", "dy")), z[f"s{k}_p"], ransac_ref.OK))
        k += 1
    k = 0
    while f"d{k}_sx" in z:
        out.append((f"degenerate {k}", tuple(z[f"d{k}_{c}"] for c in ("sx", "sy", "dx", "dy")), None, int(z[f"d{k}_status"])))
        k += 1
    return out


def _entry(lst, gpu, **kw):
    import torch
    e = {k: torch.from_numpy(np.ascontiguousarray(v, np.float32)).to(gpu) for k, v in zip(("src_x", "src_y", "dst_x", "dst_y"), lst)}
    e.update(kw)
    return e


def _assert_as_restatement(got_p, got_info, got_inl, lst, what, **kw):
    p, inl, info = ransac_ref.ransac(*lst, **kw)
    assert list(got_info) == info, f"{what}: info {list(got_info)} != {info}"
    assert ransac_ref.same_p(got_p, p), f"{what}: p {got_p} != {p}"
    m = info[3]
    assert np.array_equal(got_inl[:m], np.asarray(inl, np.int32)), f"{what}: inlier lists differ"
    assert (got_inl[m:] == -1).all(), f"{what}: tail of the inlier list"


def test_fixtures_one_call(st, gpu):
    """Every list of both fixture files in ONE call: the reference's p bit for bit, info and inliers as the restatement, and the
    lists without an answer with exactly their status, next to the others."""
    L = _fixture_lists()
    assert len(L) == 14 + 21 + 9 and len(L) > 16  # more than one launch sequence
    p, info, inl = st.capi.dev_ransac_many([_entry(lst, gpu) for _, lst, _, _ in L])
    p, info = p.cpu().numpy(), info.cpu().numpy()
    for k, (name, lst, ref_p, status) in enumerate(L):
        assert info[k, 0] == status, f"{name}: status {info[k, 0]}, expected {status}"
        if status == ransac_ref.OK:
            assert ransac_ref.same_p(p[k], ref_p), f"{name}: p {p[k]} != reference {ref_p}"
        else:
            assert np.isnan(p[k]).all(), f"{name}: p of a list without an answer"
        _assert_as_restatement(p[k], info[k], inl[k].cpu().numpy(), lst, name)


def test_host_entry_point_and_draw_cap(st, gpu):
    z = np.load(os.path.join(GOLD, "ransac_input.npz"))
    lst = tuple(z[f"in23_{c}"] for c in ("sx", "sy", "dx", "dy"))
    p, inl, info = st.capi.ransac(*lst)
    assert ransac_ref.same_p(p, z["in23_p"]) and info[0] == 0 and info[1] == 119 and len(inl) == info[3]
    p, inl, info = st.capi.ransac(*lst, mirror=True)
    assert ransac_ref.same_p(p, z["in23_pm"])
    # the walk over 119 pairs uses 292 values of rand(): a cap of 291 stops it, 292 does not
    p, inl, info = st.capi.ransac(*lst, opts=st.capi.RansacOpts(max_draws=291))
    assert list(info) == [ransac_ref.DRAW_CAP, 119, -1, 0, 291] and np.isnan(p).all() and len(inl) == 0
    assert list(info) == ransac_ref.ransac(*lst, max_draws=291)[2]
    p, inl, info = st.capi.ransac(*lst, opts=st.capi.RansacOpts(max_draws=292))
    assert ransac_ref.same_p(p, z["in23_p"]) and info[4] == 292
    with pytest.raises(st.capi.StitchError):
        st.capi.ransac(*lst, opts=st.capi.RansacOpts(rounds=16385))


def _synth(rng, n, outliers=0.4):
    sx, sy = (rng.random(n) * 600).astype(np.float32), (rng.random(n) * 450).astype(np.float32)
    x, y = sx.astype(np.float64), sy.astype(np.float64)
    dx = (0.97 * x - 0.02 * y + 1.5e-4 * x * y + 180.0 + rng.normal(0, 0.8, n)).astype(np.float32)
    dy = (0.01 * x + 1.03 * y - 1e-4 * x * y - 7.0 + rng.normal(0, 0.8, n)).astype(np.float32)
    bad = rng.random(n) < outliers
    dx[bad] = (rng.random(int(bad.sum())) * 600).astype(np.float32)
    dy[bad] = (rng.random(int(bad.sum())) * 450).astype(np.float32)
    dup = rng.integers(0, n, max(n // 50, 1))
    sx[dup], sy[dup], dx[dup], dy[dup] = sx[dup[::-1]], sy[dup[::-1]], dx[dup[::-1]], dy[dup[::-1]]
    return sx, sy, dx, dy


@pytest.mark.parametrize("rounds", [1, 73, 4096])
def test_round_counts(st, gpu, rounds):
    lst = _synth(np.random.default_rng(100 + rounds), 5000)
    p, info, inl = st.capi.dev_ransac_many([_entry(lst, gpu)], st.capi.RansacOpts(rounds=rounds))
    _assert_as_restatement(p[0].cpu().numpy(), info[0].cpu().numpy(), inl[0].cpu().numpy(), lst, f"{rounds} rounds", rounds=rounds)


def test_large_list_and_determinism(st, gpu):
    lst = _synth(np.random.default_rng(7), 65536, outliers=0.5)
    a = st.capi.dev_ransac_many([_entry(lst, gpu)])
    b = st.capi.dev_ransac_many([_entry(lst, gpu)])
    for x, y in zip((a[0], a[1], a[2][0]), (b[0], b[1], b[2][0])):
        assert np.array_equal(x.cpu().numpy().view(np.uint8), y.cpu().numpy().view(np.uint8)), "run-to-run difference"
    assert int(a[1][0, 3]) > 20000
    _assert_as_restatement(a[0][0].cpu().numpy(), a[1][0].cpu().numpy(), a[2][0].cpu().numpy(), lst, "n = 65536")


def test_threshold_seed_mirror(st, gpu):
    rng = np.random.default_rng(21)
    lst = _synth(rng, 700)
    mirrored = (lst[2], lst[3], lst[0], lst[1])
    for kw in (dict(threshold=1.25), dict(threshold=9.5), dict(seed=12345), dict(seed=0), dict(seed=4000000000), dict(threshold=0.0),
               dict(threshold=float("nan"))):
        o = st.capi.RansacOpts(**kw)
        p, info, inl = st.capi.dev_ransac_many([_entry(lst, gpu), _entry(lst, gpu, mirror=True), _entry(mirrored, gpu)], o)
        p, info = p.cpu().numpy(), info.cpu().numpy()
        _assert_as_restatement(p[0], info[0], inl[0].cpu().numpy(), lst, str(kw), **kw)
        _assert_as_restatement(p[1], info[1], inl[1].cpu().numpy(), mirrored, f"mirror flag {kw}", **kw)
        assert ransac_ref.same_p(p[1], p[2]) and np.array_equal(info[1], info[2]), f"mirror flag vs mirrored list {kw}"
    assert ransac_ref.ransac(*lst, threshold=0.0)[2][0] == ransac_ref.NO_CONSENSUS


def test_sixty_four_lists_in_one_call(st, gpu):
    """The documented batch limit: 64 lists (four launch sequences of 16) in one call -- the 44 fixture lists and 20 of them
    again, interleaved so that lists with and without an answer share launch sequences -- each compared with the reference's
    recorded p (or its status) and with the restatement's info."""
    L = _fixture_lists()
    L = (L + L[::2])[:64]
    assert len(L) == 64
    p, info, inl = st.capi.dev_ransac_many([_entry(lst, gpu) for _, lst, _, _ in L], want_inliers=False)
    assert inl is None
    p, info = p.cpu().numpy(), info.cpu().numpy()
    for k, (name, lst, ref_p, status) in enumerate(L):
        assert list(info[k]) == ransac_ref.ransac(*lst)[2] and info[k, 0] == status, f"list {k} ({name}): info {list(info[k])}"
        if status == ransac_ref.OK:
            assert ransac_ref.same_p(p[k], ref_p), f"list {k} ({name}): p {p[k]} != reference {ref_p}"
        else:
            assert np.isnan(p[k]).all(), f"list {k} ({name})"


def test_sixteen_thousand_rounds_sixteen_lists(st, gpu):
    """The documented round limit, 16 384, on 16 lists in one launch sequence: 16 x 256 round blocks exceed the consensus
    stage's workgroup target, so every list runs as ONE slab (the host's nslabs = 1 branch).  Four distinct small lists (one of
    them singular: src points on a line), each four times; info, p and the inlier list as the restatement."""
    rng = np.random.default_rng(16384)
    z = np.load(os.path.join(GOLD, "ransac_synth.npz"))
    distinct = [_synth(rng, 300, outliers=0.6), _synth(rng, 97), _synth(rng, 4, outliers=0.0),
                tuple(z[f"s17_{c}"] for c in ("sx", "sy", "dx", "dy"))]
    want = [ransac_ref.ransac(*lst, rounds=16384) for lst in distinct]
    assert all(w[2][0] == ransac_ref.OK and w[2][4] >= 4 * 16384 for w in want)
    lists = [distinct[k % 4] for k in range(16)]
    p, info, inl = st.capi.dev_ransac_many([_entry(lst, gpu) for lst in lists], st.capi.RansacOpts(rounds=16384))
    p, info = p.cpu().numpy(), info.cpu().numpy()
    for k in range(16):
        wp, winl, winfo = want[k % 4]
        assert list(info[k]) == winfo, f"list {k}: info {list(info[k])} != {winfo}"
        assert ransac_ref.same_p(p[k], wp), f"list {k}: p {p[k]} != {wp}"
        got = inl[k].cpu().numpy()
        assert np.array_equal(got[:winfo[3]], np.asarray(winl, np.int32)) and (got[winfo[3]:] == -1).all(), f"list {k}: inliers"


def _frames():
    out = []
    for i in range(1, 5):
        z = np.load(os.path.join(GOLD, f"match_frame{i}.npz"))
        idx = z["map_idx"]
        out.append((z["desc"][idx], np.stack([z["x"][idx], z["y"][idx]], 1)))
    return out


def test_lists_from_the_matcher_on_the_device(st, gpu):
    """pairs / count as dev_match_many leaves them on the device, consumed in the same stream with no synchronisation between."""
    import torch
    F = _frames()
    z = np.load(os.path.join(GOLD, "ransac_input.npz"))
    dev = [torch.from_numpy(d).to(gpu) for d, _ in F]
    xy = [(torch.from_numpy(np.ascontiguousarray(k[:, 0])).to(gpu), torch.from_numpy(np.ascontiguousarray(k[:, 1])).to(gpu)) for _, k in F]
    ij = [(i, j) for i in range(4) for j in range(4) if i != j]
    m = st.capi.dev_match_many([(dev[i], dev[j]) for i, j in ij], want_dist=False)
    lists = []
    for (i, j), o in zip(ij, m):
        for mirror in (False, True):
            lists.append(dict(src_x=xy[i][0], src_y=xy[i][1], dst_x=xy[j][0], dst_y=xy[j][1], pairs=o["pairs"], count=o["count"], mirror=mirror))
    p, info, _ = st.capi.dev_ransac_many(lists, want_inliers=False)
    p, info = p.cpu().numpy(), info.cpu().numpy()
    counts = np.load(os.path.join(GOLD, "match_pairs.npz"))["counts"]
    k = 0
    for i, j in ij:
        for suffix in ("p", "pm"):
            assert info[k, 1] == counts[i, j]
            if counts[i, j] >= 4:
                assert info[k, 0] == ransac_ref.OK and ransac_ref.same_p(p[k], z[f"in{i}{j}_{suffix}"]), f"frames {i}->{j} {suffix}"
            else:
                assert info[k, 0] == ransac_ref.TOO_FEW and np.isnan(p[k]).all()
            k += 1


def _golden():
    with open(os.path.join(GOLD, "golden.json")) as f:
        return json.load(f)


def test_pair_maps_step0(st, gpu):
    F = _frames()
    G = _golden()
    for run, src, dst in (("4", 2, 3), ("2", 1, 0)):  # matching()'s srcIndex (in the mosaic) and dstIndex (warped)
        step = G["runs"][run]["steps"][0]
        assert step["start"] == src and step["src"] == dst
        p_fwd, p_bwd, info = pipeline.pair_maps(F[src][0], F[src][1], F[dst][0], F[dst][1])
        assert ransac_ref.same_p(p_fwd, step["p_fwd"]) and ransac_ref.same_p(p_bwd, step["p"]), f"run {run}"
        assert info[0][0] == 0 and info[1][0] == 0


@pytest.mark.parametrize("run,ids", [("4", (1, 2, 3, 4)), ("2", (1, 2))])
def test_panorama_from_features(st, gpu, run, ids):
    """The reference's panorama from frames + features alone: order, maps, offsets, canvases and every mosaic's hash."""
    import torch
    from computervisionimagestich2_amd import bmp
    G = _golden()["runs"][run]
    F = _frames()
    frames = [torch.from_numpy(np.ascontiguousarray(bmp.load_bmp(os.path.join(GOLD, "input", f"{i}.bmp")))).to(gpu) for i in ids]
    final, steps = pipeline.panorama_from_features(frames, [F[i - 1] for i in ids], return_steps=True)
    assert len(steps) == len(G["steps"])
    for got, ref in zip(steps, G["steps"]):
        assert (got["start"], got["src"]) == (G["steps"][0]["start"], ref["src"])  # golden.json records the start with step 0 only
        assert ransac_ref.same_p(got["p"], ref["p"]) and ransac_ref.same_p(got["p_fwd"], ref["p_fwd"]), f"maps of step src {ref['src']}"
        assert np.float32(got["offx"]) == np.float32(ref["offx"]) and np.float32(got["offy"]) == np.float32(ref["offy"])
        assert (got["ox"], got["oy"], got["cw"], got["ch"]) == (ref["ox"], ref["oy"], ref["cw"], ref["ch"])
        assert hashlib.sha256(got["out"].cpu().numpy().tobytes()).hexdigest() == ref["out_sha256"]
    assert list(final.shape) == G["final_shape"]
    assert hashlib.sha256(final.cpu().numpy().tobytes()).hexdigest() == G["final_sha256"]
