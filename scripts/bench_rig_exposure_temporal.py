"""Temporal exposure for rigs on one MI355X (include/stitch_rig_exposure_temporal.h): the recorded run "4" (tests/golden/golden.json:
four 384 x 512 frames, a 1081 x 527 mosaic; each step's template frame from tests/golden/exposure.json) replayed on 1, 4 and 16 frame
sets per call, as time per SET, in four forms per mode -- the exposure rig as it is (mode 1 with stats_form 0, mode 2 with
stats_form 2: scripts/bench_rig_exposure.py's better form of each), the same rig with smoothing (keep 192), the same rig with fixed
statistics (set 0's measured ones) -- next to the mode-0 rig.  The protocol is scripts/bench_rig_exposure.py's: sets in buffers of
their own, every timed call ends waiting for the device, a run is one call, the median of `--runs` runs after `--warmup` calls,
min .. max kept.  The sixteen sets hold the same frames, so a smoothed stream is constant and a fixed one replays the statistics it
would measure: every mosaic must equal the unsmoothed rig's, byte for byte, and is checked.

`--baseline-only` measures the mode-0 rig and the exposure rig as it is, alone: run under STITCH_LIB with a build of the parent tree
it gives the parent's figures, which `--parent-json` takes into the output.  `--trace-fixed N` replays the fixed-statistics rig N
times on 16 sets and nothing else, for a kernel trace of its own.  Prints one JSON line and writes it to
profiles/rig_exposure_temporal_bench.json.

    python scripts/bench_rig_exposure_temporal.py [--runs 5] [--warmup 2] [--parent-json PATH ...] [--out PATH | --no-write]
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
from computervisionimagestich2_amd import bmp, capi  # noqa: E402

FORMS = {1: 0, 2: 2}  # the stats_form each mode is measured with
KEEP = 192


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--baseline-only", action="store_true")
    ap.add_argument("--trace-fixed", type=int, default=0)
    ap.add_argument("--parent-json", action="append", help="a --baseline-only result of the parent tree; the first is the baseline, further ones show its spread")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rig_exposure_temporal_bench.json"))
    ap.add_argument("--no-write", action="store_true")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_rig_exposure_temporal needs the MI355X"
    dev = torch.device("cuda:0")
    gold = os.path.join(ROOT, "tests", "golden")
    with open(os.path.join(gold, "golden.json")) as f:
        G = json.load(f)["runs"]["4"]
    with open(os.path.join(gold, "exposure.json")) as f:
        E = json.load(f)["runs"]["4"]
    steps = [dict(s, mosaic_src=r["mosaic_src"]) for s, r in zip(G["steps"], E["mode1_keep_black1"]["steps"])]
    base = [torch.from_numpy(np.ascontiguousarray(bmp.load_bmp(os.path.join(gold, "input", f"{i}.bmp")))).to(dev) for i in range(1, 5)]
    sets = [[f.clone() for f in base] for _ in range(16)]  # 16 sets in buffers of their own
    sizes = [(f.shape[2], f.shape[1]) for f in base]
    counts = (1, 4, 16)

    def make(mode):
        return capi.Rig.from_steps(sizes, None, steps, exposure=mode, stats_form=FORMS.get(mode, 2))

    outs = None

    def time_rig(rig):
        return {str(n): timeit(lambda: rig.stitch(sets[:n], out=outs[:n]), args.runs, args.warmup, n) for n in counts}

    plain = make(0)
    outs = [torch.empty((3, plain.height, plain.width), dtype=torch.uint8, device=dev) for _ in range(16)]
    if args.trace_fixed:
        for mode in (1, 2):
            rig = make(mode)
            _, _, _, stats = rig.stitch(sets[:1], out=outs[:1], return_stats=True)
            rig.fix_exposure(stats[0])
            for _ in range(args.trace_fixed):
                rig.stitch(sets, out=outs)
            rig.close()
        plain.close()
        return
    res = {"device": torch.cuda.get_device_name(0), "library": "STITCH_LIB" if os.environ.get("STITCH_LIB") else "this tree", "frames_per_set": 4,
           "frame_size": list(sizes[0]), "steps": len(steps), "runs": args.runs, "warmup": args.warmup, "keep": KEEP, "stats_form": {f"mode{m}": f for m, f in FORMS.items()},
           "timing": "one call per run, ending in a wait for the device; device events and wall clock around it; median of the runs after the "
                     "warm-up calls; *_per = per set",
           "rig_mode0": time_rig(plain), "unsmoothed": {}, "smoothed": {}, "fixed": {}, "equal": {}}
    plain.close()
    ok = True
    for mode in (1, 2):
        key = f"mode{mode}"
        rig = make(mode)
        want, status, _, stats = rig.stitch(sets, out=[torch.empty_like(o) for o in outs], return_stats=True)
        assert status == [0] * 16
        res["unsmoothed"][key] = time_rig(rig)
        if not args.baseline_only:
            rig.set_exposure_smoothing(KEEP)
            got, status, _ = rig.stitch(sets, out=outs)
            eq_s = status == [0] * 16 and all(bool((a == b).all()) for a, b in zip(got, want))
            res["smoothed"][key] = time_rig(rig)
            rig.clear_exposure_smoothing().fix_exposure(stats[0])
            got, status, _ = rig.stitch(sets, out=outs)
            eq_f = status == [0] * 16 and all(bool((a == b).all()) for a, b in zip(got, want))
            res["fixed"][key] = time_rig(rig)
            res["equal"][key] = {"smoothed": bool(eq_s), "fixed": bool(eq_f)}
            ok = ok and eq_s and eq_f
        rig.close()
    for i, path in enumerate(args.parent_json or []):
        with open(path) as f:
            parent = json.loads(f.readline())
        parent = {k: parent[k] for k in ("library", "rig_mode0", "unsmoothed")}
        if i == 0:
            res["parent"] = parent
        else:
            res.setdefault("parent_again", []).append(parent)
    if not args.baseline_only:
        summary = {}
        for mode in (1, 2):
            key = f"mode{mode}"
            base16 = (res.get("parent") or res)["unsmoothed"][key]["16"]
            un, sm, fx = (res[k][key]["16"] for k in ("unsmoothed", "smoothed", "fixed"))
            summary[key] = {"baseline": "parent" if "parent" in res else "this tree", "baseline_wall_ms_per_set": base16["wall_ms_per"],
                            "baseline_min_max": base16["wall_ms_per_min_max"], "unsmoothed_wall_ms_per_set": un["wall_ms_per"], "unsmoothed_min_max": un["wall_ms_per_min_max"],
                            "smoothed_wall_ms_per_set": sm["wall_ms_per"], "smoothing_added_wall_ms_per_call": (sm["wall_ms_per"] - base16["wall_ms_per"]) * 16,
                            "fixed_wall_ms_per_set": fx["wall_ms_per"], "fixed_min_max": fx["wall_ms_per_min_max"],
                            "fixed_faster_beyond_the_ranges": fx["wall_ms_per_min_max"][1] < base16["wall_ms_per_min_max"][0],
                            "fixed_over_mode0_rig_wall_ms_per_set": fx["wall_ms_per"] - res["rig_mode0"]["16"]["wall_ms_per"]}
        res["at_16_sets"] = summary
    line = json.dumps(res)
    print(line)
    assert ok, "a smoothed or fixed replay of identical sets differs from the unsmoothed rig's"
    if not args.no_write:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
