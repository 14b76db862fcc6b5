"""A rig's alignment monitor on one MI355X (include/stitch_rig_monitor.h): what it adds to the replay, and the stand-alone call.

The rig case is scripts/bench_rig.py's: the recorded run "4" (four 384 x 512 frames, a 1081 x 527 mosaic, three steps), 16 sets per
call, a run = one call ending in a wait for the device, device events and the wall clock around it, the median of `--runs` runs
after `--warmup` calls.  Configurations: the monitor off, and on at radius 1, 4 and 8; the added time is reported per set and step,
next to an instruction-issue estimate of the residual kernel: (tiles of the domain's bounding box that hold a domain pixel) x 4
wavefronts x shifts x WAVE_INSTR_PER_SHIFT, two cycles per wavefront instruction on each of 1024 SIMDs at 2.4 GHz.  The estimate
covers the shift loop alone -- no staging, no launch, no copy of the records -- and assumes the tiles spread evenly over the SIMDs.
`--off-only` measures "off" alone: run under STITCH_LIB with a build of the parent tree, its result is the yardstick that "off" of
this tree is compared with, and `--parent-json` takes it into the output.

Then the stand-alone call on a 4421 x 2315 canvas with a full-height overlap 600 columns wide at radius 4, with the same estimate;
and, for information, the shift the records favour for three sets of the rig at radius 4: the committed frames, the same with the
last step's frame rolled by (2, 3) pixels, and a darker scene.  Prints one JSON line and writes it to profiles/rig_monitor_bench.json.

    python scripts/bench_rig_monitor.py [--runs 5] [--warmup 2] [--off-only] [--parent-json PATH] [--out PATH | --no-write]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
import torch  # noqa: E402

from bench_rig import timeit  # noqa: E402
from computervisionimagestich2_amd import bmp, capi  # noqa: E402

# One pass of k_pairs_residual's shift loop, read from the gfx950 ISA (make -C computervisionimagestich2_amd/csrc asm): 8 ds_read_u16,
# 56 VALU for the 8 pixels of a lane and their three sums, 21 for the three wavefront reductions (18 of them DPP), 2 LDS stores.
WAVE_INSTR_PER_SHIFT = 87
TILE_W, TILE_H = 64, 32
SIMDS, CYCLES_PER_INSTR, CYCLES_PER_US = 1024, 2, 2400.0


def live_tiles(mask, r):
    """The kernel's tiles of the mask's bounding box (x0 rounded down to 64) that hold a pixel of the domain inside the margin r."""
    m = np.asarray(mask) != 0
    ch, cw = m.shape
    keep = np.zeros_like(m)
    if cw > 2 * r and ch > 2 * r:
        keep[r:ch - r, r:cw - r] = m[r:ch - r, r:cw - r]
    ys, xs = np.nonzero(keep)
    if not len(ys):
        return 0, 0
    x0, y0 = (xs.min() // 64) * 64, ys.min()
    tiles = np.unique(((xs - x0) // TILE_W).astype(np.int64) * (1 << 20) + (ys - y0) // TILE_H)
    return len(tiles), int(keep.sum())


def estimate_us(tiles, r, pairs):
    return tiles * pairs * 4 * (2 * r + 1) ** 2 * WAVE_INSTR_PER_SHIFT * CYCLES_PER_INSTR / SIMDS / CYCLES_PER_US


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--off-only", action="store_true")
    ap.add_argument("--parent-json")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rig_monitor_bench.json"))
    ap.add_argument("--no-write", action="store_true")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_rig_monitor needs the MI355X"
    dev = torch.device("cuda:0")
    gold = os.path.join(ROOT, "tests", "golden")
    with open(os.path.join(gold, "golden.json")) as f:
        steps = json.load(f)["runs"]["4"]["steps"]
    base = [torch.from_numpy(np.ascontiguousarray(bmp.load_bmp(os.path.join(gold, "input", f"{i}.bmp")))).to(dev) for i in range(1, 5)]
    sets = [[f.clone() for f in base] for _ in range(16)]
    sizes = [(f.shape[2], f.shape[1]) for f in base]
    rig = capi.Rig.from_steps(sizes, None, steps)
    outs = [torch.empty((3, rig.height, rig.width), dtype=torch.uint8, device=dev) for _ in range(16)]
    res = {"device": torch.cuda.get_device_name(0), "library": "STITCH_LIB" if os.environ.get("STITCH_LIB") else "this tree", "sets": 16, "steps": len(steps), "runs": args.runs, "warmup": args.warmup,
           "timing": "one rig.stitch call of 16 sets per run, ending in a wait for the device; device events and wall clock around it; median of "
                     "the runs after the warm-up calls",
           "estimate": f"live tiles x 4 wavefronts x shifts x {WAVE_INSTR_PER_SHIFT} wavefront instructions x {CYCLES_PER_INSTR} cycles / {SIMDS} SIMDs / "
                       f"{CYCLES_PER_US:.0f} cycles per us: the shift loop alone, spread evenly"}
    want = [o.clone() for o in rig.stitch(sets, out=outs)[0]]
    res["off"] = timeit(lambda: rig.stitch(sets, out=outs), args.runs, args.warmup, 16)
    if args.off_only:
        rig.close()
        line = json.dumps(res)
        print(line)
        if not args.no_write:
            with open(args.out, "w") as f:
                f.write(line + "\n")
        return
    if args.parent_json:
        with open(args.parent_json) as f:
            parent = json.load(f)
        res["off_parent_tree"] = {k: parent["off"][k] for k in ("device_ms_median", "wall_ms_median", "device_ms", "wall_ms")}
    same = True
    for r in (1, 4, 8):
        rig.set_monitor(r)
        got = rig.stitch(sets, out=outs)[0]
        same = same and all(bool((a == b).all()) for a, b in zip(got, want))
        t = timeit(lambda: rig.stitch(sets, out=outs), args.runs, args.warmup, 16)
        tiles = [live_tiles(rig.residual_domain(k).cpu().numpy(), r) for k in range(len(steps))]
        added = (t["device_ms_median"] - res["off"]["device_ms_median"]) * 1e3 / 16 / len(steps)
        est = sum(estimate_us(n, r, 16) for n, _ in tiles) / 16 / len(steps)
        res[f"on_r{r}"] = dict(t, live_tiles_per_step=[n for n, _ in tiles], domain_pixels_per_step=[p for _, p in tiles],
                               added_us_per_set_and_step=added, estimate_us_per_set_and_step=est, measured_over_estimate=added / est if est else None)
    rig.clear_monitor()
    res["off_again"] = timeit(lambda: rig.stitch(sets, out=outs), args.runs, args.warmup, 16)
    res["outputs_equal_with_and_without_the_monitor"] = bool(same)

    # ---- the stand-alone call: a 4421 x 2315 canvas, the overlap columns 1821 .. 2420 at full height, radius 4 ----
    cw, ch, r = 4421, 2315, 4
    g = torch.Generator(device="cpu").manual_seed(4)
    frame = torch.randint(0, 256, (3, ch, 2600), dtype=torch.uint8, generator=g).to(dev)
    mosaic = torch.randint(0, 256, (3, ch, 2421), dtype=torch.uint8, generator=g).to(dev)
    domain = torch.zeros((ch, cw), dtype=torch.uint8, device=dev)
    domain[:, 1821:2421] = 255
    pair = [(frame, [1, 0, 0, -1821, 0, 1, 0, 0], 0.0, 0.0, mosaic, 0, 0)]
    rec = capi.dev_pairs_residual(pair, cw, ch, [domain], r).cpu().numpy()[0]
    t = timeit(lambda: capi.dev_pairs_residual(pair, cw, ch, [domain], r), args.runs, args.warmup, 1)
    n_tiles, n_px = live_tiles(domain.cpu().numpy(), r)
    # (the stand-alone call tiles the whole canvas inside the margin from x = r, not the bounding box: the live tiles are counted likewise)
    x_tiles = len({(x - r) // TILE_W for x in range(1821, 2421)})
    y_tiles = -(-(ch - 2 * r) // TILE_H)
    est = estimate_us(x_tiles * y_tiles, r, 1)
    res["standalone_4421x2315_r4"] = dict(t, n=int(rec[0]), domain_pixels=n_px, live_tiles=x_tiles * y_tiles, launched_tiles=-(-(cw - 2 * r) // TILE_W) * y_tiles,
                                          estimate_us=est, measured_over_estimate=t["device_ms_median"] * 1e3 / est)

    # ---- for information: what the records say about a camera that moved ----
    last = steps[-1]["src"]
    moved = list(base)
    moved[last] = torch.roll(base[last], shifts=(3, 2), dims=(1, 2)).contiguous()
    three = [base, moved, [(f // 2 + 40).contiguous() for f in base]]
    rig.set_monitor(4)
    rig.stitch(three)
    recs = rig.residuals()
    res["best_shift_r4"] = {name: [{"step": k, "ssd": capi.residual_best_shift(recs[i][k], 4, False), "zero_mean": capi.residual_best_shift(recs[i][k], 4, True)}
                                   for k in range(len(steps))] for i, name in enumerate(("committed_frames", "last_frame_rolled_2_3", "darker_scene"))}
    rig.close()
    line = json.dumps(res)
    print(line)
    assert same, "the monitor changed an output"
    if not args.no_write:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
