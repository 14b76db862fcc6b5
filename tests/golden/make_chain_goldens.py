#!/usr/bin/env python3
"""Generates tests/golden/chains.json and tests/golden/chain_input/ from the REFERENCE ITSELF: whole-panorama runs beyond the four
frames of golden.json's runs "4" and "2".

Runs only where the reference lies at $REF (default /root/reference) and oracle/Makefile has built oracle/_ref/.  For each set it
builds the frame list, writes the frames as BMPs to a temporary directory, runs the reference's whole program under the argument
recorder (oracle/ref_record.cpp) in a CHILD PROCESS with a time limit -- the reference crashes on some sets (the full half-size
dataset3 makes 22 steps from a star-shaped graph and ends in a segmentation fault), and a set whose child does not exit 0 cannot
be a fixture -- and writes what tests/chain_sets.py parse_run extracts: start frame, per step srcIndex / dstIndex as printed, both
maps, offsets, canvas, which frame updateFeaturesByOffset moved and by how much, the two list lengths, the sha256 of the step's
mosaic; the n x n matrix of getImgPair counts with -1 where the reference made no call; the final shape and sha256.

New image bytes: the reference's src/ex6/dataset3 frames (600 x 800) reduced by a 2 x 2 box mean (a + b + c + d + 2) // 4 to
300 x 400, as tests/golden/chain_input/d3_NN.bmp.  Filler frames are Oracle.synth recipes.  Nothing here is reference source text.

    python tests/golden/make_chain_goldens.py
"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
REF_DIR = os.environ.get("REF", "/root/reference")
HALF_IDS = (1, 2, 3, 4, 5, 7, 9, 11)


def half(i):
    return {"file": f"chain_input/d3_{i:02d}.bmp"}


def inp(i):
    return {"file": f"input/{i}.bmp"}


def filled(n, placed, w, h, first_id):
    """n recipes: `placed` {position: recipe}, Oracle.synth(w, h, first_id + position) everywhere else."""
    return [placed.get(k, {"synth": [w, h, first_id + k]}) for k in range(n)]


SETS = {
    # a chain: the third step uses key points that the second step shifted by the offset of a frame placed to the left
    "chain6": [half(i) for i in (1, 3, 5, 7, 9, 11)],
    # a dense neighbour graph: frames are warped again through another neighbour
    "dense4": [half(i) for i in (1, 2, 3, 4)],
    # more than 16 frames, stitched frames on both sides of index 16; no new image bytes
    "mixed18": filled(18, {17: inp(1), 3: inp(2), 16: inp(3), 15: inp(4)}, 384, 512, 20),
    # frames of two sizes in one call, two disjoint components
    "mixed19": filled(19, {18: half(1), 2: half(4), 16: half(7), 15: half(9), 17: inp(1), 5: inp(2)}, 300, 400, 40),
}


def write_half_size_frames():
    from computervisionimagestich2_amd import bmp
    os.makedirs(os.path.join(HERE, "chain_input"), exist_ok=True)
    for i in HALF_IDS:
        f = bmp.load_bmp(f"{REF_DIR}/src/ex6/dataset3/{i}.bmp").astype(np.uint16)
        assert f.shape == (3, 800, 600)
        q = ((f[:, 0::2, 0::2] + f[:, 0::2, 1::2] + f[:, 1::2, 0::2] + f[:, 1::2, 1::2] + 2) // 4).astype(np.uint8)
        bmp.save_bmp(os.path.join(HERE, half(i)["file"]), q)


def properties(name, rec):
    """The properties a set is there for, as far as the recording itself shows them (test_chain_host.py asserts the same)."""
    steps = rec["steps"]
    out = set()
    for k, s in enumerate(steps):
        assert (s["shift"]["ox"], s["shift"]["oy"]) == (s["ox"], s["oy"])
        if (s["ox"] or s["oy"]) and any(t["srcIndex"] == s["shift"]["frame"] for t in steps[k + 1:]):
            out.add("pre_shift_consumed")
    dsts = [s["dstIndex"] for s in steps]
    if len(set(dsts)) < len(dsts):
        out.add("warped_again")
    used = {s["srcIndex"] for s in steps} | set(dsts)
    if len(rec["frames"]) > 16 and min(used) < 16 and max(used) >= 16:
        out.add("both_sides_of_16")
    if len({tuple(f["shape"]) for f in rec["frames"]}) > 1:
        out.add("mixed_sizes")
    return sorted(out)


def main():
    import chain_sets
    assert chain_sets.recorder_ready(), "build oracle/_ref first (make -C oracle ref)"
    write_half_size_frames()
    J = {}
    for name, recipes in SETS.items():
        frames = chain_sets.frames_of(recipes)
        rec = chain_sets.run_reference(frames)
        assert rec is not None, f"{name}: the reference did not exit 0 on this set; it cannot be a fixture"
        rec["frames"] = [dict(r, shape=list(f.shape), sha256=chain_sets.sha(f)) for r, f in zip(recipes, frames)]
        rec["properties"] = properties(name, rec)
        J[name] = rec
        print(name, "start", rec["start"], "steps", [(s["srcIndex"], s["dstIndex"]) for s in rec["steps"]], "final",
              rec["final_shape"][2], "x", rec["final_shape"][1], rec["properties"])
    have = set().union(*[set(r["properties"]) for r in J.values()])
    assert len(J["chain6"]["frames"]) >= 6 and "pre_shift_consumed" in J["chain6"]["properties"]
    assert have == {"pre_shift_consumed", "warped_again", "both_sides_of_16", "mixed_sizes"}, have
    with open(os.path.join(HERE, "chains.json"), "w") as f:
        json.dump(J, f, indent=1)
        f.write("\n")
    print("wrote chains.json", os.path.getsize(os.path.join(HERE, "chains.json")), "bytes")


if __name__ == "__main__":
    main()
