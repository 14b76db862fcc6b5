"""A rig's frames and outputs in the 4:2:2 layouts and NV21 on one MI355X (include/stitch_rig_formats_yuv.h): what the formats cost the
replay, and the two conversions on their own.  The protocol of scripts/bench_rig_formats.py.

baseline the four-frame rig of the recorded run "4" (1081 x 527) on 16 sets per call: the planar replay with no format set, and NV12 on
         both sides in one call -- this library before and after everything else, and with --parent-lib PATH (a libstitch_hip.so built
         from the parent commit) that library in child processes of this run (STITCH_LIB), likewise twice.  The parent's two runs define
         its run-to-run spread.
formats  for YUYV, UYVY, NV21 and NV16 on both sides: the one call of a formatted rig, against capi.dev_unpack_many per frame index +
         the planar rig + capi.dev_pack_many as calls of their own on the same buffers.  The outputs of the two are compared first, and
         Rig.input_form says which form the one call's frames took.
convert  capi.dev_unpack_many and capi.dev_pack_many on 16 images of 4096 x 4096 per format, NV12 beside the four, in GB/s of
         algorithmic bytes (the packed image once and the planar image once) against the 8 TB/s HBM roofline.

One process, every call ends in a wait for the device, device events and the wall clock around it, the median of `--runs` calls after
`--warmup`, with min .. max.  Prints one JSON line and writes it to profiles/rig_formats_yuv_bench.json.

    python scripts/bench_rig_formats_yuv.py [--runs 9] [--warmup 3] [--parent-lib PATH] [--out PATH | --no-write]
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import torch  # noqa: E402

from bench_crop import recorded_rig, uncropped  # noqa: E402
from bench_rig import timeit  # noqa: E402
from bench_rig_formats import same  # noqa: E402
from computervisionimagestich2_amd import capi  # noqa: E402

NAMES = {capi.PIX_YUYV: "YUYV", capi.PIX_UYVY: "UYVY", capi.PIX_NV21: "NV21", capi.PIX_NV16: "NV16"}
FORMS = {capi.RIG_INPUT_NONE: "none", capi.RIG_INPUT_FUSED: "fused", capi.RIG_INPUT_CONVERTED: "converted"}


def baseline(rig, sets, dev, runs, warmup):
    """The planar replay and the NV12 one call, on whatever library is loaded."""
    planar = uncropped(rig, sets, dev, runs, warmup)[0]
    frames = [capi.dev_pack_many(fs, capi.PIX_NV12, 0) for fs in sets]
    outs = [capi.Image.empty(capi.PIX_NV12, rig.width, rig.height, dev) for _ in sets]
    rig.set_formats(capi.PIX_NV12, capi.PIX_NV12, 0)
    nv12 = timeit(lambda: rig.stitch(frames, out=outs), runs, warmup, 16)
    rig.clear_formats()
    return {"planar": planar, "nv12_one_call": nv12}


def parent_run(lib, runs, warmup):
    env = dict(os.environ, STITCH_LIB=os.path.abspath(lib))
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--only-baseline", "--no-write", "--runs", str(runs), "--warmup", str(warmup)], env=env,
                       capture_output=True, text=True, timeout=600)
    if r.returncode:
        raise RuntimeError(f"the parent library's run failed:\n{r.stdout}\n{r.stderr}")
    return json.loads(r.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--only-baseline", action="store_true", help="the planar replay and NV12 alone, on whatever library STITCH_LIB names")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rig_formats_yuv_bench.json"))
    ap.add_argument("--no-write", action="store_true")
    args = ap.parse_args()
    if args.only_baseline:
        assert torch.cuda.is_available(), "bench_rig_formats_yuv needs the MI355X"
        dev = torch.device("cuda:0")
        rig, sets = recorded_rig(dev)
        print(json.dumps(baseline(rig, sets, dev, args.runs, args.warmup)))
        rig.close()
        return
    parent = [parent_run(args.parent_lib, args.runs, args.warmup)] if args.parent_lib else []  # before this process opens the device
    assert torch.cuda.is_available(), "bench_rig_formats_yuv needs the MI355X"
    dev = torch.device("cuda:0")
    res = {"device": torch.cuda.get_device_name(0), "runs": args.runs, "warmup": args.warmup,
           "timing": "one call (or the calls it replaces) per run, ending in a wait for the device; device events and wall clock around it; median of the "
                     "runs after the warm-up calls; *_per = per set of a 16-set call", "baseline_16_sets": {}, "formats_16_sets": {}, "convert_16x4096x4096": {}}
    rig, sets = recorded_rig(dev)
    n = rig.n_frames
    res["baseline_16_sets"]["this_commit"] = [baseline(rig, sets, dev, args.runs, args.warmup)]

    # ---- the one call against the three it replaces ----
    planar_in = [[torch.empty_like(f) for f in fs] for fs in sets]
    planar_out = [torch.empty((3, rig.height, rig.width), dtype=torch.uint8, device=dev) for _ in sets]
    for fmt, name in NAMES.items():
        frames = [capi.dev_pack_many(fs, fmt, 0) for fs in sets]  # the frames as a camera delivers them
        outs = [capi.Image.empty(fmt, rig.width, rig.height, dev) for _ in sets]
        outs3 = [capi.Image.empty(fmt, rig.width, rig.height, dev) for _ in sets]

        def three_calls():
            for f in range(n):  # (frames of one size per call)
                capi.dev_unpack_many([fs[f] for fs in frames], 0, out=[ps[f] for ps in planar_in])
            rig.stitch(planar_in, out=planar_out)
            capi.dev_pack_many(planar_out, fmt, 0, out=outs3)

        rig.clear_formats()
        three_calls()
        rig.set_formats(fmt, fmt, 0)
        _, status, _ = rig.stitch(frames, out=outs)
        assert status == [0] * 16 and all(same(a, b) for a, b in zip(outs, outs3)), f"{name}: the one call and the three differ"
        forms = [FORMS[rig.input_form(f)] for f in range(n)]
        one = timeit(lambda: rig.stitch(frames, out=outs), args.runs, args.warmup, 16)
        rig.clear_formats()
        three = timeit(three_calls, args.runs, args.warmup, 16)
        res["formats_16_sets"][name] = {"one_call": one, "unpack_rig_pack": three, "unpack_calls": n, "input_form": forms}
    res["baseline_16_sets"]["this_commit"].append(baseline(rig, sets, dev, args.runs, args.warmup))
    rig.close()
    del sets, planar_in, planar_out

    # ---- the conversions on their own ----
    w = h = 4096
    planar = [capi.dev_synth(w, h, i, torch.uint8, dev) for i in range(16)]
    for fmt, name in list(NAMES.items()) + [(capi.PIX_NV12, "NV12")]:
        packed = capi.dev_pack_many(planar, fmt, 0)
        back = [torch.empty_like(p) for p in planar]
        nbytes = 16 * (sum(capi.image_bytes(fmt, w, h)) + 3 * w * h)
        row = {"algorithmic_bytes": nbytes}
        for what, fn in (("pack", lambda: capi.dev_pack_many(planar, fmt, 0, out=packed)), ("unpack", lambda: capi.dev_unpack_many(packed, 0, out=back))):
            t = timeit(fn, args.runs, args.warmup)
            row[what] = dict(t, gb_per_s_device=nbytes / (t["device_ms_median"] * 1e-3) / 1e9, fraction_of_8_tb_per_s=nbytes / (t["device_ms_median"] * 1e-3) / 8e12)
        res["convert_16x4096x4096"][name] = row
        del packed, back
    if args.parent_lib:
        parent.append(parent_run(args.parent_lib, args.runs, args.warmup))
        res["baseline_16_sets"]["parent_commit"] = parent
    res["headline"] = {"planar_wall_ms_per_set": [t["planar"]["wall_ms_per"] for t in res["baseline_16_sets"]["this_commit"]],
                       "parent_planar_wall_ms_per_set": [t["planar"]["wall_ms_per"] for t in parent],
                       "nv12_wall_ms_per_set": [t["nv12_one_call"]["wall_ms_per"] for t in res["baseline_16_sets"]["this_commit"]],
                       "parent_nv12_wall_ms_per_set": [t["nv12_one_call"]["wall_ms_per"] for t in parent],
                       "one_call_vs_three_wall_ms_per_set": {k: [v["one_call"]["wall_ms_per"], v["unpack_rig_pack"]["wall_ms_per"]] for k, v in res["formats_16_sets"].items()},
                       "convert_gb_per_s": {k: {d: round(v[d]["gb_per_s_device"], 1) for d in ("pack", "unpack")} for k, v in res["convert_16x4096x4096"].items()}}
    line = json.dumps(res)
    print(line)
    if not args.no_write:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
