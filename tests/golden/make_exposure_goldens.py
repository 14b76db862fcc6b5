"""Writes tests/golden/exposure.json: the exposure-matched chain (include/stitch_exposure.h) replayed by the CPU restatements
alone -- no GPU, no reference binary.  Inputs: the committed frames and the recorded steps and maps of golden.json's runs "2"
and "4".  Per step: oracle.project (once per frame), oracle.transfer in specified-function mode, in place on the projected
frame about to be warped, then oracle.pair; at the end equalise + luminance mix.  Modes 1 (the template is the projected frame
the step stitches to) and 2 (the template is the running mosaic), keep_black 0 and 1.

The recorded steps name only the frame they warp.  The committed frames are one strip, 0 - 1 - 2 - 3, stitched outwards from
the start frame, so the frame in the mosaic that a step stitches to is the warped frame's neighbour on the start frame's side
(tests/test_gpu_exposure.py holds the C chain's own stitch order to this).

Recorded per step: the transfer's twelve statistics as bit patterns, the SHA-256 of the recoloured frame and of the step's
mosaic; per chain the final shape and SHA-256.

    python tests/golden/make_exposure_goldens.py        # rewrites tests/golden/exposure.json
"""
import hashlib
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
OUT = os.path.join(HERE, "exposure.json")
RUNS = ("2", "4")
MODES = (1, 2)


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def key_of(mode, keep_black):
    return f"mode{mode}_keep_black{int(bool(keep_black))}"


def mosaic_side(start, warped):
    return warped - 1 if warped > start else warped + 1


def load_inputs():
    sys.path[:0] = [p for p in (ROOT, os.path.join(ROOT, "tests")) if p not in sys.path]
    from computervisionimagestich2_amd import bmp
    J = json.load(open(os.path.join(HERE, "golden.json")))
    frames = [np.ascontiguousarray(bmp.load_bmp(os.path.join(HERE, e["file"]))) for e in J["input"]]
    return J, frames


def chain(oracle, frames, run, mode, keep_black):
    """One exposure-matched chain on the CPU -> the record of exposure.json."""
    start = run["steps"][0]["start"]
    proj = {}

    def projected(i):
        if i not in proj:
            proj[i] = oracle.project(frames[i])
        return proj[i]

    result = projected(start)
    steps = []
    for st in run["steps"]:
        dst, src = st["src"], mosaic_side(start, st["src"])
        x = projected(dst)
        out, stats = oracle.transfer(x, projected(src) if mode == 1 else result)
        if keep_black:
            out[:, (x == 0).all(axis=0)] = 0
        proj[dst] = out
        rc, paired = oracle.pair(out, st["p"], np.float32(st["offx"]), np.float32(st["offy"]), result, st["ox"], st["oy"], st["cw"], st["ch"])
        assert rc == 0, (mode, keep_black, dst, rc)
        result = paired
        steps.append(dict(src=dst, mosaic_src=src, stats_bits=[int(v) for v in np.ascontiguousarray(stats, np.float32).view(np.uint32)],
                          transferred_sha256=sha(out), out_sha256=sha(result)))
    eq, _hist, _lut = oracle.equalize(result)
    final = oracle.lummix(result, eq, 19.0, 20.0)
    return dict(steps=steps, final_shape=list(final.shape), final_sha256=sha(final))


def generate(oracle, runs=RUNS, modes=MODES, keep_blacks=(0, 1)):
    J, frames = load_inputs()
    return {"runs": {n: {key_of(m, kb): chain(oracle, frames, J["runs"][n], m, kb) for m in modes for kb in keep_blacks} for n in runs}}


if __name__ == "__main__":
    sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
    from oracle_lib import Oracle
    with open(OUT, "w") as f:
        json.dump(generate(Oracle()), f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", OUT)
