"""The exposure-matched rig replay on one MI355X (include/stitch_rig_exposure.h): the recorded run "4" (tests/golden/golden.json:
four 384 x 512 frames, a 1081 x 527 mosaic; each step's template frame from tests/golden/exposure.json) replayed on 1, 4 and 16
frame sets per call with the colour transfer before every step -- modes 1 and 2, stats_form 0 and 2 -- as time per SET, next to
pipeline.stitch_chain(..., plans=kept, exposure=mode) looped over the same sets in the same process and next to the mode-0 rig.
The protocol is scripts/bench_rig.py's: sets in buffers of their own, every timed call ends waiting for the device, a run is one
call (or one loop), the median of `--runs` runs after `--warmup` calls, min .. max kept.  The mosaics of the rig and of the loop
are compared byte for byte and with the recorded hash.  Also times the single-image transfer (capi.dev_transfer, forms 0 and 2)
at 1081 x 527, whose kernels share their device functions with the many-image forms.  Prints one JSON line and writes it to
profiles/rig_exposure_bench.json.

    python scripts/bench_rig_exposure.py [--runs 5] [--warmup 2] [--out PATH | --no-write]
"""
import argparse
import hashlib
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rig_exposure_bench.json"))
    ap.add_argument("--no-write", action="store_true")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_rig_exposure needs the MI355X"
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
    plans = {}

    def chain_loop(n, mode):
        res = None
        for i in range(n):
            res = pipeline.stitch_chain(sets[i], steps, plans=plans, exposure=mode)  # keep_black, spans + walk: the defaults
        return res

    res = {"device": torch.cuda.get_device_name(0), "frames_per_set": 4, "frame_size": list(sizes[0]), "steps": len(steps), "runs": args.runs,
           "warmup": args.warmup,
           "timing": "one call (or one loop over the sets) per run, ending in a wait for the device; device events and wall clock around it; "
                     "median of the runs after the warm-up calls; *_per = per set",
           "rig_mode0": {}, "rig": {}, "stitch_chain_loop_kept_plans": {}, "equal": {}}
    plain = capi.Rig.from_steps(sizes, None, steps)
    outs = [torch.empty((3, plain.height, plain.width), dtype=torch.uint8, device=dev) for _ in range(16)]
    for n in (1, 4, 16):
        res["rig_mode0"][str(n)] = timeit(lambda: plain.stitch(sets[:n], out=outs[:n]), args.runs, args.warmup, n)
    plain.close()
    ok = True
    for mode in (1, 2):
        want = chain_loop(1, mode)
        recorded = hashlib.sha256(want.cpu().numpy().tobytes()).hexdigest() == E[f"mode{mode}_keep_black1"]["final_sha256"]
        res["stitch_chain_loop_kept_plans"][f"mode{mode}"] = {str(n): timeit(lambda: chain_loop(n, mode), args.runs, args.warmup, n) for n in (1, 4, 16)}
        for form in (0, 2):
            key = f"mode{mode}_form{form}"
            rig = capi.Rig.from_steps(sizes, None, steps, exposure=mode, stats_form=form)
            got, status, _ = rig.stitch(sets, out=outs)
            equal = all(bool((o == want).all()) for o in got) and status == [0] * 16 and recorded
            res["equal"][key] = bool(equal)
            ok = ok and equal
            res["rig"][key] = {str(n): timeit(lambda: rig.stitch(sets[:n], out=outs[:n]), args.runs, args.warmup, n) for n in (1, 4, 16)}
            rig.close()
        loop16 = res["stitch_chain_loop_kept_plans"][f"mode{mode}"]["16"]["wall_ms_per"]
        best = min((0, 2), key=lambda f: res["rig"][f"mode{mode}_form{f}"]["16"]["wall_ms_per"])
        rig16 = res["rig"][f"mode{mode}_form{best}"]["16"]["wall_ms_per"]
        res[f"mode{mode}_at_16_sets"] = {"better_stats_form": best, "rig_wall_ms_per_set": rig16, "chain_loop_wall_ms_per_set": loop16,
                                         "chain_loop_over_rig": loop16 / rig16,
                                         "added_wall_ms_per_set_over_mode0_rig": rig16 - res["rig_mode0"]["16"]["wall_ms_per"]}
    # the single-image transfer at the mosaic's size: its kernels run the device functions the many-image forms run
    g = torch.Generator(device="cpu").manual_seed(7)
    src, tem = (torch.randint(1, 256, (3, 527, 1081), dtype=torch.uint8, generator=g).to(dev) for _ in range(2))
    out = torch.empty_like(src)
    res["transfer_1081x527"] = {f"form{form}": timeit(lambda: capi.dev_transfer(src, tem, out=out, stats_form=form, keep_black=True), args.runs, args.warmup)
                                for form in (0, 2)}
    pipeline.close_plans(plans)
    line = json.dumps(res)
    print(line)
    assert ok, "a rig's mosaics differ from stitch_chain's or from the recorded run"
    if not args.no_write:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
