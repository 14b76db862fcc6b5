"""SIFT extraction (k_sift.inc) on one MI355X; prints one JSON line and writes it to profiles/sift_bench.json.

  input_frames   the four Input/ frames (tests/golden/input, projected gray 384 x 512) as ONE dev_sift_many call
  input2_frame   the recorded projected gray of Input2/2 (1210 x 907, tests/golden/sift_input2.npz)
  synth_4096     one 4096 x 4096 frame (dev_synth, projected gray)
Device events around back-to-back calls.  Next to each, where oracle/_ref/libref_hotpath.so was built, the reference's own
VLFeat sequence (tests/sift_ref.py: siftAlgorithm's calls through ctypes) on the same gray images on this host's CPU, and
whether its features equal the device's bit for bit (best of three passes; the driver's Python overhead per keypoint is
part of that time).  The launch counts are those of stitch_sift.inc's sequence: two column passes per smoothed level, detect,
scan, emit, gradient, orientations, row scan, descriptors, plus the hand-over in every octave but the first, which instead
smooths level s_min in place (two more passes).

    python scripts/bench_sift.py [--reps 10] [--only NAME] [--no-write]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch  # noqa: E402

import sift_ref as R  # noqa: E402
from computervisionimagestich2_amd import bmp, capi  # noqa: E402


def timeit(fn, reps, runs=5):
    """Median over `runs` of the mean time of `reps` back-to-back calls (device events), after a warm-up."""
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(runs):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b) / reps)
    return statistics.median(out)


def measure(grays, reps, kp_cap, ref):
    def run():
        return capi.dev_sift_many(grays, None, kp_cap)
    first = [capi.sift_unpack(o) for o in run()]
    assert all(f["status"][0] == capi.SIFT_OK for f in first), [f["status"] for f in first]
    ms = timeit(run, reps)
    again = [capi.sift_unpack(o) for o in run()]
    assert all(R.same_bits(a[k], b[k]) for a, b in zip(first, again) for k in ("kp", "fkp", "angle", "desc"))
    r = {"frames": len(grays), "sizes": [[int(g.shape[1]), int(g.shape[0])] for g in grays], "gpu_ms_per_call": ms,
         "keypoints": [len(f["kp"]) for f in first], "features": [len(f["desc"]) for f in first]}
    if ref is not None:
        host = [g.cpu().numpy() for g in grays]
        times = []
        for _ in range(3):  # the first pass warms caches and the allocator; the best of three is reported
            t0 = time.perf_counter()
            want = [R.reference_sift(ref, g) for g in host]
            times.append((time.perf_counter() - t0) * 1e3)
        r["reference_cpu_ms"] = min(times)
        r["reference_cpu_ms_passes"] = times
        r["reference_over_gpu"] = r["reference_cpu_ms"] / ms
        r["reference_features_equal"] = all(R.same_bits(a[k], b[k]) for a, b in zip(first, want) for k in ("kp", "fkp", "angle", "desc"))
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--only", default="")
    ap.add_argument("--no-write", action="store_true")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_sift needs the MI355X"
    dev = torch.device("cuda:0")
    ref = R.load_reference() if os.path.exists(R.REF_SO) else None
    levels = 2
    res = {"device": torch.cuda.get_device_name(0), "reps": args.reps, "launches_first_octave": 6 + 2 * (levels + 3),
           "launches_later_octave": 7 + 2 * (levels + 2), "launches_per_call_fixed": 3,
           "reference_timing": "best of 3 passes of the ctypes driver (tests/sift_ref.py) around the reference's VLFeat calls, one "
                               "thread, this host; the driver's per-keypoint Python overhead is included",
           "timing": "median of 5 runs of `reps` back-to-back calls between device events, after 2 warm-up calls"}
    gold = os.path.join(ROOT, "tests", "golden")

    def want(name):
        return not args.only or args.only == name
    if want("input_frames"):
        frames = [torch.from_numpy(np.ascontiguousarray(bmp.load_bmp(os.path.join(gold, "input", f"{i}.bmp")))).to(dev) for i in range(1, 5)]
        res["input_frames"] = measure([capi.dev_project_gray(f)[1] for f in frames], args.reps * 5, 2048, ref)
    if want("input2_frame"):
        g = torch.from_numpy(np.load(os.path.join(gold, "sift_input2.npz"))["gray"]).to(dev)
        res["input2_frame"] = measure([g], args.reps * 2, 8192, ref)
    if want("synth_4096"):
        g = capi.dev_project_gray(capi.dev_synth(4096, 4096, 3, torch.uint8))[1]
        res["synth_4096"] = measure([g], args.reps, 1 << 18, ref)
    line = json.dumps(res)
    print(line)
    if not args.no_write and not args.only:
        with open(os.path.join(ROOT, "profiles", "sift_bench.json"), "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
