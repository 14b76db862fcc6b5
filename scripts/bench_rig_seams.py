"""Fixed seams on one MI355X: 16 sets of the recorded run "4" (tests/golden/golden.json: four 384 x 512 frames, a 1081 x 527
mosaic) replayed by one rig (capi.Rig, include/stitch_rig.h) with content seams -- the code as it was before fixed seams, the
baseline of this process --, with its seams fixed (include/stitch_rig_seams.h: one small launch per step instead of the scan),
and the geometric_seams() call itself, on a fresh rig each time (coverage planes, scans, the wait).  Every timed call ends waiting
for the device; a run is one call: device events and the wall clock around it, the median of `--runs` runs after `--warmup` calls,
with min .. max.  The fixed seams are set 0's content seams, so both replays must give the same bytes, the reference's recorded
mosaic.  Prints one JSON line and writes it to profiles/rig_seams_bench.json.

    python scripts/bench_rig_seams.py [--runs 5] [--warmup 2] [--out PATH | --no-write]
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

from computervisionimagestich2_amd import bmp, capi  # noqa: E402


def timeit(fn, runs, warmup, per=1):
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
    return {"device_ms_median": statistics.median(dev_ms), "wall_ms_median": statistics.median(wall_ms), "per": per,
            "wall_ms_per": statistics.median(wall_ms) / per, "wall_ms_min_max": [min(wall_ms), max(wall_ms)],
            "device_ms_min_max": [min(dev_ms), max(dev_ms)], "device_ms": dev_ms, "wall_ms": wall_ms}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rig_seams_bench.json"))
    ap.add_argument("--no-write", action="store_true")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_rig_seams needs the MI355X"
    dev = torch.device("cuda:0")
    gold = os.path.join(ROOT, "tests", "golden")
    with open(os.path.join(gold, "golden.json")) as f:
        G = json.load(f)["runs"]["4"]
    steps = G["steps"]
    base = [torch.from_numpy(np.ascontiguousarray(bmp.load_bmp(os.path.join(gold, "input", f"{i}.bmp")))).to(dev) for i in range(1, 5)]
    sets = [[f.clone() for f in base] for _ in range(16)]
    sizes = [(f.shape[2], f.shape[1]) for f in base]
    rig = capi.Rig.from_steps(sizes, None, steps)
    outs = [torch.empty((3, rig.height, rig.width), dtype=torch.uint8, device=dev) for _ in range(16)]
    got, status, seams = rig.stitch(sets, out=outs)
    recorded = status == [0] * 16 and all(hashlib.sha256(o.cpu().numpy().tobytes()).hexdigest() == G["final_sha256"] for o in got)
    res = {"device": torch.cuda.get_device_name(0), "sets": 16, "frames_per_set": 4, "frame_size": list(sizes[0]), "mosaic_size": [rig.width, rig.height],
           "steps": len(steps), "runs": args.runs, "warmup": args.warmup,
           "timing": "one call per run, ending in a wait for the device; device events and wall clock around it; median of the runs after the "
                     "warm-up calls, with min .. max; wall_ms_per = per set"}
    # content, fixed, content, fixed: each form twice, in both orders, so that a drift of the machine shows as a spread
    res["content_seams"] = timeit(lambda: rig.stitch(sets, out=outs), args.runs, args.warmup, 16)
    rig.fix_seams(seams[0])
    res["fixed_seams"] = timeit(lambda: rig.stitch(sets, out=outs), args.runs, args.warmup, 16)
    fixed_out, status, _ = rig.stitch(sets, out=outs)
    same = status == [0] * 16 and all(hashlib.sha256(o.cpu().numpy().tobytes()).hexdigest() == G["final_sha256"] for o in fixed_out)
    rig.clear_seams()
    res["content_seams_again"] = timeit(lambda: rig.stitch(sets, out=outs), args.runs, args.warmup, 16)
    rig.fix_seams(seams[0])
    res["fixed_seams_again"] = timeit(lambda: rig.stitch(sets, out=outs), args.runs, args.warmup, 16)
    res["fixed_over_content_wall"] = (res["fixed_seams"]["wall_ms_median"] + res["fixed_seams_again"]["wall_ms_median"]) / \
        (res["content_seams"]["wall_ms_median"] + res["content_seams_again"]["wall_ms_median"])
    rig.close()

    def geometric():
        r = capi.Rig.from_steps(sizes, None, steps)
        t0 = time.perf_counter()
        r.geometric_seams()
        dt = (time.perf_counter() - t0) * 1e3
        geo = r.seams
        r.close()
        return dt, geo

    for _ in range(args.warmup):
        geometric()
    calls = [geometric() for _ in range(args.runs)]
    res["geometric_seams_call"] = {"what": "stitch_dev_rig_geometric_seams on a fresh rig: the allocation of the planes, 1 + 3 * 2 launches, the copy of the "
                                           "records and the wait (wall clock around the call alone)",
                                   "wall_ms_median": statistics.median(c[0] for c in calls), "wall_ms_min_max": [min(c[0] for c in calls), max(c[0] for c in calls)],
                                   "wall_ms": [c[0] for c in calls]}
    res["geometric_seams"] = [list(s) for s in calls[0][1]]
    res["content_seams_of_set_0"] = [list(s) for s in seams[0]]
    res["equals_recorded_run"] = bool(recorded)
    res["fixed_equals_recorded_run"] = bool(same)
    line = json.dumps(res)
    print(line)
    assert recorded and same, "a replay differs from the recorded run"
    if not args.no_write:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
