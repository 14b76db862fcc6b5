"""The crop of a rig's output on one MI355X (include/stitch_rig_crop.h): the search for the largest inscribed rectangle, and what
a crop costs the replay.

search   stitch_dev_rig_inscribed_rect (the rig's bit planes) and stitch_dev_largest_rect_u8 (the bytes stitch_dev_rig_coverage_u8
         serves) on the output coverage of the recorded run "4" (1081 x 527) and on the projection coverage of a 6144 x 4096 frame;
         stitch_dev_largest_rect_u8 on a 16 384-wide staircase (heights 1 .. 8192 .. 1), the mask on which a search that walks
         outward from every column is quadratic.  Every call waits for the device, so the wall clock around it is the figure.
replay   the four-frame rig of the recorded run on 16 sets per call: uncropped, with the inscribed rectangle in mode 1 (the slice of
         the finished canvas) and in mode 2 (the finish pass on the slice).  The cropped outputs are compared with the slices first.
parent   with --parent-lib PATH (a libstitch_hip.so built from the parent commit), the uncropped replay is also measured on that
         library, in child processes of this run (STITCH_LIB), once before and once after everything else.

A run is one call; device events and the wall clock around it, the median of `--runs` runs after `--warmup` calls.  Prints one JSON
line and writes it to profiles/crop_bench.json.

    python scripts/bench_crop.py [--runs 9] [--warmup 3] [--parent-lib PATH] [--out PATH | --no-write]
"""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import torch  # noqa: E402

from bench_rig import timeit  # noqa: E402
from computervisionimagestich2_amd import bmp, capi  # noqa: E402


def recorded_rig(dev):
    gold = os.path.join(ROOT, "tests", "golden")
    with open(os.path.join(gold, "golden.json")) as f:
        steps = json.load(f)["runs"]["4"]["steps"]
    base = [torch.from_numpy(np.ascontiguousarray(bmp.load_bmp(os.path.join(gold, "input", f"{i}.bmp")))).to(dev) for i in range(1, 5)]
    sets = [[f.clone() for f in base] for _ in range(16)]
    rig = capi.Rig.from_steps([(f.shape[2], f.shape[1]) for f in base], None, steps)
    return rig, sets


def uncropped(rig, sets, dev, runs, warmup):
    outs = [torch.empty((3, rig.height, rig.width), dtype=torch.uint8, device=dev) for _ in sets]
    return timeit(lambda: rig.stitch(sets, out=outs), runs, warmup, len(sets)), outs


def parent_run(lib, runs, warmup):
    env = dict(os.environ, STITCH_LIB=os.path.abspath(lib))
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--only-uncropped", "--no-write", "--runs", str(runs), "--warmup", str(warmup)], env=env,
                       capture_output=True, text=True, timeout=600)
    if r.returncode:
        raise RuntimeError(f"the parent library's run failed:\n{r.stdout}\n{r.stderr}")
    return json.loads(r.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--only-uncropped", action="store_true", help="the uncropped replay alone, on whatever library STITCH_LIB names")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "crop_bench.json"))
    ap.add_argument("--no-write", action="store_true")
    args = ap.parse_args()
    if args.only_uncropped:
        assert torch.cuda.is_available(), "bench_crop needs the MI355X"
        dev = torch.device("cuda:0")
        rig, sets = recorded_rig(dev)
        t, _ = uncropped(rig, sets, dev, args.runs, args.warmup)
        rig.close()
        print(json.dumps(t))
        return
    parent = [parent_run(args.parent_lib, args.runs, args.warmup)] if args.parent_lib else []  # before this process opens the device
    assert torch.cuda.is_available(), "bench_crop needs the MI355X"
    dev = torch.device("cuda:0")
    res = {"device": torch.cuda.get_device_name(0), "runs": args.runs, "warmup": args.warmup,
           "timing": "one call per run, ending in a wait for the device; device events and wall clock around it; median of the runs after the "
                     "warm-up calls; replay figures *_per = per set of a 16-set call", "search": {}, "replay_16_sets": {}}

    # ---- the search ----
    rig, sets = recorded_rig(dev)
    rect = rig.inscribed_rect()
    cov = rig.coverage()
    assert capi.dev_largest_rect(cov) == rect
    res["search"]["recorded_run_1081x527"] = {"rect": list(rect), "covered_fraction": float((cov != 0).float().mean()),
                                              "bits": timeit(rig.inscribed_rect, args.runs, args.warmup), "bytes": timeit(lambda: capi.dev_largest_rect(cov), args.runs, args.warmup)}
    big = capi.Rig.from_steps([(6144, 4096)], 0, [])
    big_rect = big.inscribed_rect()
    big_cov = big.coverage()
    assert capi.dev_largest_rect(big_cov) == big_rect
    res["search"]["projection_6144x4096"] = {"rect": list(big_rect), "covered_fraction": float((big_cov != 0).float().mean()),
                                             "bits": timeit(big.inscribed_rect, args.runs, args.warmup),
                                             "bytes": timeit(lambda: capi.dev_largest_rect(big_cov), args.runs, args.warmup)}
    big.close()
    del big_cov
    w = 16384
    x = torch.arange(w, device=dev)
    hts = torch.minimum(x + 1, w - x)
    rows = int(hts.max())
    stairs = (torch.arange(rows - 1, -1, -1, device=dev)[:, None] < hts[None, :]).to(torch.uint8) * 255
    s_rect = capi.dev_largest_rect(stairs)
    assert s_rect[2] * s_rect[3] == max(v * (w - 2 * (v - 1)) for v in range(1, rows + 1))
    res["search"]["staircase_16384x8192"] = {"rect": list(s_rect), "bytes": timeit(lambda: capi.dev_largest_rect(stairs), args.runs, args.warmup)}
    row = stairs[-1:].contiguous()  # one row of 16 384 columns: the per-row search alone
    res["search"]["staircase_16384x1"] = {"rect": list(capi.dev_largest_rect(row)), "bytes": timeit(lambda: capi.dev_largest_rect(row), args.runs, args.warmup)}
    del stairs

    # ---- the replay ----
    x0, y0, cw, ch = rect
    t_first, full = uncropped(rig, sets, dev, args.runs, args.warmup)
    res["replay_16_sets"]["uncropped"] = [t_first]
    outs =[torch.empty((3, ch, cw), dtype=torch.uint8, device=dev) for _ in sets]
    for mode in (1, 2):
        rig.set_crop(rect, mode)
        got, status, _ = rig.stitch(sets, out=outs)
        assert status == [0] * 16
        if mode == 1:
            assert all(bool((g == f[:, y0:y0 + ch, x0:x0 + cw]).all()) for g, f in zip(got, full)), "mode 1 is not the slice"
        res["replay_16_sets"][f"mode_{mode}"] = timeit(lambda: rig.stitch(sets, out=outs), args.runs, args.warmup, 16)
    rig.clear_crop()
    res["replay_16_sets"]["uncropped"].append(uncropped(rig, sets, dev, args.runs, args.warmup)[0])
    res["replay_16_sets"]["rect"] = list(rect)
    res["replay_16_sets"]["canvas"] = [rig.width, rig.height]
    rig.close()
    if args.parent_lib:
        parent.append(parent_run(args.parent_lib, args.runs, args.warmup))
        res["replay_16_sets"]["uncropped_parent_commit"] = parent
    r = res["replay_16_sets"]
    res["headline"] = {"uncropped_wall_ms_per_set": [t["wall_ms_per"] for t in r["uncropped"]],
                       "parent_wall_ms_per_set": [t["wall_ms_per"] for t in parent],
                       "mode_1_wall_ms_per_set": r["mode_1"]["wall_ms_per"], "mode_2_wall_ms_per_set": r["mode_2"]["wall_ms_per"],
                       "search_wall_ms": {k: {f: v[f]["wall_ms_median"] for f in ("bits", "bytes") if f in v} for k, v in res["search"].items()}}
    line = json.dumps(res)
    print(line)
    if not args.no_write:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
