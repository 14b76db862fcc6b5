"""The whole panorama of the four committed frames (tests/golden/input, 384 x 512) on one MI355X, frames on the device in,
mosaic on the device out: the ONE call of the C ABI (capi.dev_panorama = stitch_dev_panorama_u8, include/stitch_panorama.h)
next to the Python chain it restates (pipeline.panorama_from_frames) on the same box.  Both calls wait for the device before
they return, so a run is one call: device events and the wall clock around it, the median of `--runs` runs after `--warmup`
calls.  The two mosaics are compared byte for byte, and with the reference's recorded hash.  Prints one JSON line and writes it to
profiles/panorama_bench.json.

    python scripts/bench_panorama.py [--runs 5] [--warmup 2] [--out PATH | --no-write]
"""
import argparse
import hashlib
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from computervisionimagestich2_amd import bmp, capi, pipeline  # noqa: E402


def timeit(fn, runs, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    dev_ms, wall_ms = [], []
    for _ in range(runs):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        wall_ms.append((time.perf_counter() - t0) * 1e3)
        dev_ms.append(a.elapsed_time(b))
    return {"device_ms_median": statistics.median(dev_ms), "wall_ms_median": statistics.median(wall_ms), "device_ms": dev_ms, "wall_ms": wall_ms}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "panorama_bench.json"))
    ap.add_argument("--no-write", action="store_true")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_panorama needs the MI355X"
    dev = torch.device("cuda:0")
    gold = os.path.join(ROOT, "tests", "golden")
    frames = [torch.from_numpy(np.ascontiguousarray(bmp.load_bmp(os.path.join(gold, "input", f"{i}.bmp")))).to(dev) for i in range(1, 5)]
    c_out = capi.dev_panorama(frames)
    py_out = pipeline.panorama_from_frames(frames)
    equal = c_out.shape == py_out.shape and c_out.cpu().numpy().tobytes() == py_out.cpu().numpy().tobytes()
    with open(os.path.join(gold, "golden.json")) as f:
        recorded = json.load(f)["runs"]["4"]["final_sha256"]
    res = {"device": torch.cuda.get_device_name(0), "frames": 4, "frame_size": [int(frames[0].shape[2]), int(frames[0].shape[1])],
           "mosaic_size": [int(c_out.shape[2]), int(c_out.shape[1])], "runs": args.runs, "warmup": args.warmup,
           "timing": "one call per run, device events and wall clock around it, median of the runs after the warm-up calls",
           "c_chain": timeit(lambda: capi.dev_panorama(frames), args.runs, args.warmup),
           "python_chain": timeit(lambda: pipeline.panorama_from_frames(frames), args.runs, args.warmup),
           "mosaics_equal": bool(equal), "equals_recorded_run": hashlib.sha256(c_out.cpu().numpy().tobytes()).hexdigest() == recorded}
    res["python_over_c_wall"] = res["python_chain"]["wall_ms_median"] / res["c_chain"]["wall_ms_median"]
    line = json.dumps(res)
    print(line)
    assert equal, "the C chain and the Python chain give different mosaics"
    if not args.no_write:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
