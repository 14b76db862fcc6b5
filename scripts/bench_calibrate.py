"""The calibration from several captures on one MI355X (include/stitch_calibrate.h): capi.dev_calibrate on 1, 4 and 16 captures of
the four committed 384 x 512 frames (tests/golden/input), next to capi.dev_panorama on one capture -- the only way to calibrate a
rig before -- and next to pipeline.calibrate_from_sets, the chain spelled out on the stage calls, on the same captures in the same
process.  Captures 1 .. 15 are capture 0 through monotone byte tables, in buffers of their own, so that every capture has features
of its own.  The protocol is scripts/bench_rig.py's: every timed call ends waiting for the device, device events and wall clock
around it, the median of `--runs` runs after `--warmup` calls, min .. max kept.  Two relations are reported, none is gated:
one-capture calibration against dev_panorama (it runs a subset of that call's launches), and 16 captures against 16 times one
capture (SIFT and matching are batched).  Prints one JSON line and writes it to profiles/calibrate_bench.json.

    python scripts/bench_calibrate.py [--runs 5] [--warmup 2] [--out PATH | --no-write]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import torch  # noqa: E402

from bench_rig import timeit  # noqa: E402
from computervisionimagestich2_amd import bmp, capi, pipeline  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "calibrate_bench.json"))
    ap.add_argument("--no-write", action="store_true")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_calibrate needs the MI355X"
    dev = torch.device("cuda:0")
    gold = os.path.join(ROOT, "tests", "golden")
    base = [torch.from_numpy(np.ascontiguousarray(bmp.load_bmp(os.path.join(gold, "input", f"{i}.bmp")))).to(dev) for i in range(1, 5)]
    v = np.arange(256, dtype=np.float64) / 255.0
    sets = [[f.clone() for f in base]]
    for k in range(1, 16):  # gamma 0.70 .. 1.45 without 1: monotone, so the scene stays and the features move
        g = 0.65 + 0.05 * k + (0.05 if k >= 7 else 0.0)
        lut = torch.from_numpy(np.round(255.0 * v ** g).astype(np.uint8)).to(dev)
        sets.append([lut[f.long()].contiguous() for f in base])

    def cal(n):
        capi.dev_calibrate(sets[:n]).close()

    res = {"device": torch.cuda.get_device_name(0), "cameras": 4, "frame_size": [base[0].shape[2], base[0].shape[1]], "runs": args.runs, "warmup": args.warmup,
           "timing": "one call per run, ending in a wait for the device; device events and wall clock around it; median of the runs after the warm-up "
                     "calls; *_per = per capture",
           "dev_calibrate": {}, "calibrate_from_sets": {}}
    one = capi.dev_calibrate(sets[:1])
    _, psteps = capi.dev_panorama(sets[0], return_steps=True)
    res["one_capture_equals_dev_panorama"] = bool(len(one.steps) == len(psteps) and all(
        a["src"] == b["src"] and np.asarray(a["p"]).tobytes() == np.asarray(b["p"]).tobytes() and np.asarray(a["p_fwd"]).tobytes() == np.asarray(b["p_fwd"]).tobytes()
        for a, b in zip(one.steps, psteps)))
    one.close()
    res["dev_panorama_one_capture"] = timeit(lambda: capi.dev_panorama(sets[0]), args.runs, args.warmup)
    res["dev_panorama_one_capture_no_finish"] = timeit(lambda: capi.dev_panorama(sets[0], finish=False), args.runs, args.warmup)
    for n in (1, 4, 16):
        c = capi.dev_calibrate(sets[:n])
        py = pipeline.calibrate_from_sets(sets[:n])
        res.setdefault("steps", {})[str(n)] = [[s["mosaic_src"], s["src"]] for s in c.steps]
        res.setdefault("support", {})[str(n)] = c.support.tolist()
        res.setdefault("c_equals_python", {})[str(n)] = bool(len(c.steps) == len(py["steps"]) and np.array_equal(c.counts, py["counts"]) and all(
            np.asarray(a["p_fwd"]).tobytes() == np.asarray(b["p_fwd"]).tobytes() for a, b in zip(c.steps, py["steps"])))
        c.close()
        res["dev_calibrate"][str(n)] = timeit(lambda: cal(n), args.runs, args.warmup, n)
        res["calibrate_from_sets"][str(n)] = timeit(lambda: pipeline.calibrate_from_sets(sets[:n]), args.runs, args.warmup, n)
    c1, c16, p1 = (res["dev_calibrate"]["1"]["wall_ms_median"], res["dev_calibrate"]["16"]["wall_ms_median"], res["dev_panorama_one_capture"]["wall_ms_median"])
    res["one_capture_over_dev_panorama"] = c1 / p1
    res["sixteen_captures_over_one"] = c16 / c1
    res["python_over_c_at_16"] = res["calibrate_from_sets"]["16"]["wall_ms_median"] / c16
    line = json.dumps(res)
    print(line)
    if not args.no_write:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
