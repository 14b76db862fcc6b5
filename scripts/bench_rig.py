"""A calibrated rig on one MI355X: the recorded run "4" (tests/golden/golden.json: four 384 x 512 frames, a 1081 x 527 mosaic)
replayed on 1, 4 and 16 frame sets per call (capi.Rig = stitch_dev_rig_stitch_u8, include/stitch_rig.h), as time per SET, next
to what the library could do before, looped over the same sets in the same process: pipeline.stitch_chain with kept workspaces
and, for orientation, the whole panorama from frames (capi.dev_panorama, which also finds the maps).  Then the two many-image
kernels of the replay against loops of the single-image calls, on the 16 x 4 frames and the 16 mosaics of that case.  Every
timed call ends waiting for the device; a run is one call (or one loop): device events and the wall clock around it, the median
of `--runs` runs after `--warmup` calls.  The mosaics of the rig and of the loop are compared byte for byte, and with the
reference's recorded hash.  Prints one JSON line and writes it to profiles/rig_bench.json.

    python scripts/bench_rig.py [--runs 5] [--warmup 2] [--out PATH | --no-write]
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
            "device_ms_per": statistics.median(dev_ms) / per, "wall_ms_per": statistics.median(wall_ms) / per,
            "wall_ms_per_min_max": [min(wall_ms) / per, max(wall_ms) / per], "device_ms": dev_ms, "wall_ms": wall_ms}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rig_bench.json"))
    ap.add_argument("--no-write", action="store_true")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_rig needs the MI355X"
    dev = torch.device("cuda:0")
    gold = os.path.join(ROOT, "tests", "golden")
    with open(os.path.join(gold, "golden.json")) as f:
        G = json.load(f)["runs"]["4"]
    steps = G["steps"]
    base = [torch.from_numpy(np.ascontiguousarray(bmp.load_bmp(os.path.join(gold, "input", f"{i}.bmp")))).to(dev) for i in range(1, 5)]
    sets = [[f.clone() for f in base] for _ in range(16)]  # 16 sets in buffers of their own
    sizes = [(f.shape[2], f.shape[1]) for f in base]
    rig = capi.Rig.from_steps(sizes, None, steps)
    outs = [torch.empty((3, rig.height, rig.width), dtype=torch.uint8, device=dev) for _ in range(16)]
    plans = {}

    def chain_loop(n):
        res = None
        for i in range(n):
            res = pipeline.stitch_chain(sets[i], steps, plans=plans)
        return res

    def panorama_loop(n):
        for i in range(n):
            capi.dev_panorama(sets[i])

    got, status, _ = rig.stitch(sets, out=outs)
    want = chain_loop(1)
    equal = all(bool((o == want).all()) for o in got) and status == [0] * 16
    recorded = hashlib.sha256(got[15].cpu().numpy().tobytes()).hexdigest() == G["final_sha256"]
    res = {"device": torch.cuda.get_device_name(0), "frames_per_set": 4, "frame_size": list(sizes[0]), "mosaic_size": [rig.width, rig.height],
           "steps": len(steps), "runs": args.runs, "warmup": args.warmup,
           "timing": "one call (or one loop over the sets) per run, ending in a wait for the device; device events and wall clock around it; "
                     "median of the runs after the warm-up calls; *_per = per set (per image for the two kernels)",
           "rig": {}, "stitch_chain_loop_kept_plans": {}, "dev_panorama_loop": {}}
    for n in (1, 4, 16):
        res["rig"][str(n)] = timeit(lambda: rig.stitch(sets[:n], out=outs[:n]), args.runs, args.warmup, n)
        res["stitch_chain_loop_kept_plans"][str(n)] = timeit(lambda: chain_loop(n), args.runs, args.warmup, n)
    res["dev_panorama_loop"]["4"] = timeit(lambda: panorama_loop(4), args.runs, args.warmup, 4)
    res["chain_loop_over_rig_wall_16"] = res["stitch_chain_loop_kept_plans"]["16"]["wall_ms_per"] / res["rig"]["16"]["wall_ms_per"]

    flat = [f for s in sets for f in s]
    proj = [torch.empty_like(f) for f in flat]
    res["project_many_64"] = timeit(lambda: capi.dev_project_many(flat, out=proj), args.runs, args.warmup, 64)
    res["project_loop_64"] = timeit(lambda: [capi.dev_project(f, out=o) for f, o in zip(flat, proj)], args.runs, args.warmup, 64)
    mos = [o.clone() for o in outs]
    res["finish_many_16"] = timeit(lambda: capi.dev_finish_many(mos), args.runs, args.warmup, 16)
    res["finish_loop_16"] = timeit(lambda: [capi.dev_finish(m) for m in mos], args.runs, args.warmup, 16)
    res["mosaics_equal_stitch_chain"] = bool(equal)
    res["equals_recorded_run"] = bool(recorded)
    pipeline.close_plans(plans)
    rig.close()
    line = json.dumps(res)
    print(line)
    assert equal and recorded, "the rig's mosaics differ from stitch_chain's or from the recorded run"
    if not args.no_write:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
