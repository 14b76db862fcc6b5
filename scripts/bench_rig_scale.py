"""A rig's output scale on one MI355X (include/stitch_rig_scale.h): what the scaled pack costs against the pack it replaces, and
against the scaler a user had to run before.

The rig case is scripts/bench_rig.py's: the recorded run "4" (four 384 x 512 frames, a 1081 x 527 mosaic, three steps), 16 sets per
call, a run = one call ending in a wait for the device, device events and the wall clock around it, the median of `--runs` runs
after `--warmup` calls.  Configurations, all with BGR24 frames in and NV12 out (matrix 1):
  1. `unscaled`: the format rig as it was.  `--unscaled-only` measures this alone: run under STITCH_LIB with a build of the parent
     tree, its result is the yardstick that `unscaled` of this tree is compared with, and `--parent-json` takes it into the output.
  2. `scaled_half` (540 x 263) and `scaled_1920_equivalent` (469 x 246: 1920 / 4421 and 1080 / 2315 of the canvas, the ratios
     that take this project's large canvas to 1920 x 1080): the same rig with an output scale, one call.
  3. `planar_then_scale_*`: what a user has without the rig's scale -- the planar rig, then stitch_dev_scale_pack_many_u8 on its
     16 outputs -- in one timed run.
`unscaled_again` closes the bracket around the scaled runs.  The scaled outputs are checked against (3)'s, which the GPU tests hold to
the reference.  Prints one JSON line and writes it to profiles/rig_scale_bench.json.

    python scripts/bench_rig_scale.py [--runs 5] [--warmup 2] [--unscaled-only] [--parent-json PATH] [--out PATH | --no-write]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
import torch  # noqa: E402

from bench_rig import timeit  # noqa: E402
from computervisionimagestich2_amd import bmp, capi  # noqa: E402

IN_FMT, OUT_FMT, MATRIX = capi.PIX_BGR24, capi.PIX_NV12, 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--unscaled-only", action="store_true")
    ap.add_argument("--parent-json")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rig_scale_bench.json"))
    ap.add_argument("--no-write", action="store_true")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_rig_scale needs the MI355X"
    dev = torch.device("cuda:0")
    gold = os.path.join(ROOT, "tests", "golden")
    with open(os.path.join(gold, "golden.json")) as f:
        steps = json.load(f)["runs"]["4"]["steps"]
    base = [torch.from_numpy(np.ascontiguousarray(bmp.load_bmp(os.path.join(gold, "input", f"{i}.bmp")))).to(dev) for i in range(1, 5)]
    sets = [[f.clone() for f in base] for _ in range(16)]
    packed = [capi.dev_pack_many(fs, IN_FMT, MATRIX) for fs in sets]
    sizes = [(f.shape[2], f.shape[1]) for f in base]
    rig = capi.Rig.from_steps(sizes, None, steps).set_formats(IN_FMT, OUT_FMT, MATRIX)
    W, H = rig.width, rig.height
    res = {"device": torch.cuda.get_device_name(0), "library": "STITCH_LIB" if os.environ.get("STITCH_LIB") else "this tree", "sets": 16, "steps": len(steps),
           "canvas": [W, H], "formats": "BGR24 in, NV12 out, matrix 1", "runs": args.runs, "warmup": args.warmup,
           "timing": "one call of 16 sets per run, ending in a wait for the device; device events and wall clock around it; median of the runs after "
                     "the warm-up calls"}

    def fresh(w, h):
        return [capi.Image.empty(OUT_FMT, w, h, dev) for _ in range(16)]

    outs = fresh(W, H)
    res["unscaled"] = timeit(lambda: rig.stitch(packed, out=outs), args.runs, args.warmup, 16)
    if args.parent_json:
        with open(args.parent_json) as f:
            parent = json.load(f)
        res["unscaled_parent_tree"] = {k: parent["unscaled"][k] for k in ("device_ms_median", "wall_ms_median", "device_ms", "wall_ms")}
    if not args.unscaled_only:
        targets = {"half": (W // 2, H // 2), "1920_equivalent": (round(W * 1920 / 4421), round(H * 1080 / 2315))}
        planar_rig = capi.Rig.from_steps(sizes, None, steps).set_formats(IN_FMT, capi.PIX_PLANAR, MATRIX)
        planar_outs = [capi.Image.empty(capi.PIX_PLANAR, W, H, dev) for _ in range(16)]
        same = True
        for name, (ow, oh) in targets.items():
            scaled_outs, user_outs = fresh(ow, oh), fresh(ow, oh)
            rig.set_output_scale(ow, oh)
            res[f"scaled_{name}"] = dict(timeit(lambda: rig.stitch(packed, out=scaled_outs), args.runs, args.warmup, 16), size=[ow, oh])

            def user():
                planar_rig.stitch(packed, out=planar_outs)
                capi.dev_scale_pack_many([o.data for o in planar_outs], (ow, oh), OUT_FMT, MATRIX, out=user_outs)

            res[f"planar_then_scale_{name}"] = dict(timeit(user, args.runs, args.warmup, 16), size=[ow, oh])
            res[f"scale_pack_many_alone_{name}"] = timeit(lambda: capi.dev_scale_pack_many([o.data for o in planar_outs], (ow, oh), OUT_FMT, MATRIX, out=user_outs),
                                                          args.runs, args.warmup, 16)
            same = same and all(bool((a.data == b.data).all()) and bool((a.data2 == b.data2).all()) for a, b in zip(scaled_outs, user_outs))
            rig.clear_output_scale()
        res["unscaled_again"] = timeit(lambda: rig.stitch(packed, out=outs), args.runs, args.warmup, 16)
        res["scaled_rig_equals_planar_rig_then_scale"] = bool(same)
        planar_rig.close()
        assert same, "the scaled rig and the planar rig followed by the stand-alone call differ"
    rig.close()
    line = json.dumps(res)
    print(line)
    if not args.no_write:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
