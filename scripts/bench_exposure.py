"""What the exposure option costs on one MI355X (include/stitch_exposure.h).  One process, the median of `--runs`
runs after `--warmup` calls, device events and the wall clock around each call.

  statistics   the transfer's statistics alone -- capi.dev_running_stats on six planes, three of a source and three of a
               template of the same size -- in form 0 (the serial walk of k_tr_stats, the yardstick in the same run), 1 (one
               workgroup's scan) and 2 (spans + walk) at 384 x 512, 1081 x 527, 4421 x 2315 and 4096 x 4096.  The planes are
               l, alpha, beta of a synthetic frame; the three forms' results are compared bit for bit.
  panorama     the four committed frames through capi.dev_panorama with the option off, mode 1 and mode 2, each with
               stats_form 0 and 2.

Prints one JSON line and writes it to profiles/exposure_bench.json.

    python scripts/bench_exposure.py [--runs 5] [--warmup 2] [--out PATH | --no-write]
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

from computervisionimagestich2_amd import bmp, capi  # noqa: E402

SIZES = [(384, 512), (1081, 527), (4421, 2315), (4096, 4096)]


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


def lab_planes(w, h, frame_id, dev):
    """l, alpha, beta of a synthetic frame (the oracle's restatement of RGBtoLab) as three float32 device tensors"""
    from oracle_lib import Oracle
    O = Oracle()
    img = O.synth(w, h, frame_id)
    lab = O.rgb_to_lab(np.ascontiguousarray(img.reshape(3, -1).T, np.float32))
    return [torch.from_numpy(np.ascontiguousarray(lab[:, c])).to(dev) for c in range(3)]


def bits(t):
    return t.cpu().numpy().view(np.uint32).tolist()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "exposure_bench.json"))
    ap.add_argument("--no-write", action="store_true")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_exposure needs the MI355X"
    dev = torch.device("cuda:0")
    res = {"device": torch.cuda.get_device_name(0), "runs": args.runs, "warmup": args.warmup,
           "timing": "one call per run, device events and wall clock around it, median of the runs after the warm-up calls",
           "statistics": [], "panorama": {}}
    for w, h in SIZES:
        planes = lab_planes(w, h, 1, dev) + lab_planes(w, h, 8, dev)
        row = {"size": [w, h], "samples_per_plane": w * h, "planes": 6}
        want = None
        for form in (0, 1, 2):
            mean, sd, diag = capi.dev_running_stats(planes, form=form, want_diag=True)
            got = (bits(mean), bits(sd))
            want = want or got
            row[f"form{form}"] = timeit(lambda: capi.dev_running_stats(planes, form=form), args.runs, args.warmup)
            row[f"form{form}"]["equals_form0"] = got == want
            row[f"form{form}"]["ns_per_sample_and_pass"] = row[f"form{form}"]["device_ms_median"] * 1e6 / (2 * w * h)
            if form:
                row[f"form{form}"]["diag"] = diag.cpu().numpy().tolist()
        row["form0_over_form1"] = row["form0"]["device_ms_median"] / row["form1"]["device_ms_median"]
        row["form0_over_form2"] = row["form0"]["device_ms_median"] / row["form2"]["device_ms_median"]
        res["statistics"].append(row)
        print(json.dumps(row), flush=True)
        del planes
    gold = os.path.join(ROOT, "tests", "golden")
    frames = [torch.from_numpy(np.ascontiguousarray(bmp.load_bmp(os.path.join(gold, "input", f"{i}.bmp")))).to(dev) for i in range(1, 5)]
    res["panorama"]["off"] = timeit(lambda: capi.dev_panorama(frames), args.runs, args.warmup)
    for mode in (1, 2):
        outs = {}
        for form in (0, 2):
            e = dict(mode=mode, stats_form=form)
            outs[form] = capi.dev_panorama(frames, exposure=e).cpu().numpy().tobytes()
            res["panorama"][f"mode{mode}_form{form}"] = timeit(lambda: capi.dev_panorama(frames, exposure=e), args.runs, args.warmup)
        res["panorama"][f"mode{mode}_forms_equal"] = outs[0] == outs[2]
    line = json.dumps(res)
    print(line)
    assert all(r[f"form{f}"]["equals_form0"] for r in res["statistics"] for f in (1, 2)), "a form's statistics differ from form 0's"
    assert res["panorama"]["mode1_forms_equal"] and res["panorama"]["mode2_forms_equal"]
    if not args.no_write:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
