"""CPU: the whole-panorama chain's host logic against runs of the REFERENCE beyond four frames (tests/golden/chains.json, written by
tests/golden/make_chain_goldens.py): the stitch order of both chains against the order the reference printed, from the getImgPair
counts the reference evaluated; the key-point update rule (ImageProcess.cpp:226-227) against the frame the recorder saw shifted;
the step geometry against the recorded canvases; the fixtures' own integrity; and, where the reference is built, one set live."""
import json
import os

import numpy as np
import pytest

import chain_sets
from computervisionimagestich2_amd import pipeline

GOLD = chain_sets.GOLD
SETS = ("chain6", "dense4", "mixed18", "mixed19")
STEP_FIELDS = {"srcIndex", "dstIndex", "p", "p_fwd", "offx", "offy", "ox", "oy", "cw", "ch", "fw", "fh", "mw", "mh", "shift",
               "len_src_dst", "len_dst_src", "out_sha256"}


def _set(name):
    return chain_sets.chains()[name]


# ---- the stitch order and getMiddleIndex against the reference -------------------------------------------------------------------
@pytest.mark.parametrize("fill", [0, 2 ** 30])
@pytest.mark.parametrize("name", SETS)
def test_stitch_order_is_the_references(st, name, fill):
    """Entries the reference never evaluated ((i, j) once (j, i) was a neighbour) are -1 in the recording: the order may not depend
    on them, so they are replaced by 0 and by a huge count."""
    G = _set(name)
    counts = np.array(G["counts"], np.int64)
    assert (counts == -1).any()
    counts[counts == -1] = fill
    want = (G["start"], [(s["srcIndex"], s["dstIndex"]) for s in G["steps"]])
    got = pipeline.stitch_order(counts.tolist())
    assert (got[0], [tuple(p) for p in got[1]]) == want, f"pipeline.stitch_order: {got}, the reference printed {want}"
    got = st.capi.stitch_order_c(counts.astype(np.int32))
    assert got == want, f"stitch_stitch_order: {got}, the reference printed {want}"


# ---- the key-point update rule and the step geometry against the reference ---------------------------------------------------------
@pytest.mark.parametrize("name", SETS)
def test_key_point_updates_are_the_references(st, name, monkeypatch):
    """The Python chain's KeyPointTrack walked over the recorded steps on arrays as long as the recorded feature counts: at every
    step it must put the warped frame through the forward map and shift the frame the recorder saw shifted (identified by its
    feature count, as in the recording), by the recorded offsets, and nothing else.  The C chain states the same rule on device
    arrays (pano_steps); tests/test_gpu_chains.py pins it through the mosaics."""
    capi = st.capi
    G = _set(name)
    n = len(G["frames"])
    assert len(G["features"]) == n
    rng = np.random.default_rng(n)
    kps = [np.stack([rng.uniform(0.0, 383.0, m), rng.uniform(0.0, 511.0, m)], 1).astype(np.float32) for m in G["features"]]
    calls = []
    real_map, real_shift = capi.map_points, capi.shift_points

    def spy_map(x, y, p, offx, offy):
        calls.append(("map", len(x), [float(v) for v in p], np.float32(offx).tobytes(), np.float32(offy).tobytes()))
        return real_map(x, y, p, offx, offy)

    def spy_shift(x, y, ox, oy):
        calls.append(("shift", len(x), int(ox), int(oy)))
        return real_shift(x, y, ox, oy)

    monkeypatch.setattr(capi, "map_points", spy_map)
    monkeypatch.setattr(capi, "shift_points", spy_shift)
    track = pipeline.KeyPointTrack(kps, G["start"])
    mw, mh = G["frames"][G["start"]]["shape"][2], G["frames"][G["start"]]["shape"][1]
    for k, s in enumerate(G["steps"]):
        src, dst, moved = s["srcIndex"], s["dstIndex"], s["shift"]["frame"]
        _, fh, fw = G["frames"][dst]["shape"]
        assert (fw, fh, mw, mh) == (s["fw"], s["fh"], s["mw"], s["mh"])
        # the step's canvas, by the library's host arithmetic from the recorded forward map (:206-216, :224)
        g = capi.step_geometry(fw, fh, s["p_fwd"], mw, mh)
        assert np.float32(g.min_x).tobytes() == np.float32(s["offx"]).tobytes() and np.float32(g.min_y).tobytes() == np.float32(s["offy"]).tobytes()
        assert (g.ox, g.oy, g.cw, g.ch) == (s["ox"], s["oy"], s["cw"], s["ch"]), f"{name} step {k}: canvas"
        before = [a.copy() for a in track.kps]
        del calls[:]
        track.stitched(src, dst, s["p_fwd"], g)
        assert calls == [("map", G["features"][dst], s["p_fwd"], np.float32(s["offx"]).tobytes(), np.float32(s["offy"]).tobytes()),
                         ("shift", s["shift"]["n"], s["shift"]["ox"], s["shift"]["oy"])], f"{name} step {k}: {calls}"
        # ... and in values: forward map on dst first, then the offsets on the recorded frame (which may be dst itself)
        want = [a.copy() for a in before]
        x, y, _, _ = real_map(want[dst][:, 0], want[dst][:, 1], s["p_fwd"], s["offx"], s["offy"])
        want[dst] = np.stack([x, y], 1)
        x, y, _, _ = real_shift(want[moved][:, 0], want[moved][:, 1], s["ox"], s["oy"])
        want[moved] = np.stack([x, y], 1)
        for f in range(n):
            assert track.kps[f].tobytes() == want[f].tobytes(), f"{name} step {k}: key points of frame {f}"
        mw, mh = g.cw, g.ch
    assert [mh, mw] == G["final_shape"][1:]


# ---- the fixtures themselves ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", SETS)
def test_fixture_integrity(name):
    G = _set(name)
    n = len(G["frames"])
    frames = chain_sets.frames_of(G["frames"])
    for r, f in zip(G["frames"], frames):
        assert list(f.shape) == r["shape"] and chain_sets.sha(f) == r["sha256"], f"{name}: frame {r}"
    counts = np.array(G["counts"])
    assert counts.shape == (n, n) and (np.diag(counts) == 0).all() and (counts >= -1).all()
    # exactly the entries matching()'s first loop skips are -1
    replay, used = chain_sets.evaluated_pairs([int(c) for c in counts[(counts >= 0) & ~np.eye(n, dtype=bool)]], n)
    assert replay == G["counts"] and used == int(((counts >= 0) & ~np.eye(n, dtype=bool)).sum())
    assert 0 <= G["start"] < n and G["steps"]
    pre = G["start"]
    for k, s in enumerate(G["steps"]):
        assert set(s) == STEP_FIELDS, f"{name} step {k}: {set(s) ^ STEP_FIELDS}"
        assert set(s["shift"]) == {"n", "ox", "oy", "frame"}
        assert len(s["p"]) == len(s["p_fwd"]) == 8 and len(s["out_sha256"]) == 64
        src, dst = s["srcIndex"], s["dstIndex"]
        assert counts[src][dst] >= 20 or counts[dst][src] >= 20
        # descriptors never change: a step's two lists are as long as the first loop's, where that evaluated the pair
        for c, m in ((counts[src][dst], s["len_src_dst"]), (counts[dst][src], s["len_dst_src"])):
            assert c in (-1, m)
        # the recorder identifies the shifted frame by its feature count alone, which must be unique in the set; it is :227's
        assert G["features"].count(s["shift"]["n"]) == 1 and G["features"][s["shift"]["frame"]] == s["shift"]["n"]
        assert s["shift"]["frame"] == pre and (s["shift"]["ox"], s["shift"]["oy"]) == (s["ox"], s["oy"])
        pre = dst
    assert G["final_shape"] == [3, G["steps"][-1]["ch"], G["steps"][-1]["cw"]] and len(G["final_sha256"]) == 64


def _stitched(G):
    return {s["srcIndex"] for s in G["steps"]} | {s["dstIndex"] for s in G["steps"]}


def test_the_sets_cover_what_they_are_there_for():
    # a chain of at least 6 frames where a shift of `pre` by a non-zero offset is consumed later, with pre != the step's source
    G = _set("chain6")
    assert len(G["frames"]) >= 6 and len(_stitched(G)) >= 6
    assert any((s["ox"] or s["oy"]) and s["shift"]["frame"] != s["srcIndex"] and any(t["srcIndex"] == s["shift"]["frame"] for t in G["steps"][k + 1:])
               for k, s in enumerate(G["steps"]))
    # a frame warped more than once
    dsts = [s["dstIndex"] for s in _set("dense4")["steps"]]
    assert len(set(dsts)) < len(dsts)
    # more than 16 frames, stitched frames on both sides of index 16
    G = _set("mixed18")
    assert len(G["frames"]) > 16 and min(_stitched(G)) < 16 <= max(_stitched(G))
    # frames of different sizes in one call
    G = _set("mixed19")
    assert len({tuple(f["shape"]) for f in G["frames"]}) > 1 and len(G["frames"]) > 16


def test_mixed18_is_the_recorded_four_frame_run_among_fillers():
    """Its four real frames are the committed input/1..4.bmp: the fillers match nothing, so every step is run "4"'s."""
    with open(os.path.join(GOLD, "golden.json")) as f:
        R4 = json.load(f)["runs"]["4"]
    G = _set("mixed18")
    where = {i: int(r["file"][len("input/")]) - 1 for i, r in enumerate(G["frames"]) if "file" in r}
    assert sorted(where.values()) == [0, 1, 2, 3]
    assert where[G["start"]] == R4["steps"][0]["start"] and len(G["steps"]) == len(R4["steps"])
    for a, b in zip(G["steps"], R4["steps"]):
        assert where[a["dstIndex"]] == b["src"]
        assert all(a[k] == b[k] for k in ("p", "p_fwd", "offx", "offy", "ox", "oy", "cw", "ch", "out_sha256"))
    assert G["final_shape"] == R4["final_shape"] and G["final_sha256"] == R4["final_sha256"]


def test_fixture_sizes():
    new = [os.path.join(GOLD, "chains.json")] + [os.path.join(GOLD, "chain_input", f) for f in sorted(os.listdir(os.path.join(GOLD, "chain_input")))]
    assert len(new) == 9
    sizes = [os.path.getsize(p) for p in new]
    assert max(sizes) < 900102 and sum(sizes) < 3500000, sizes


# ---- one set live, where the reference is built ------------------------------------------------------------------------------------------
def test_dense4_live_against_its_recording():
    if not chain_sets.recorder_ready():
        pytest.skip("the reference and its recorder are not built here (oracle/_ref)")
    G = _set("dense4")
    live = chain_sets.run_reference(chain_sets.frames_of(G["frames"]))
    assert live is not None, "the reference did not exit 0"
    recorded = {k: v for k, v in G.items() if k not in ("frames", "properties")}
    assert json.loads(json.dumps(live)) == recorded
