"""Path seams on one MI355X (include/stitch_seam_path.h): what they add to a rig's replay, and the stand-alone finder.

The rig case is scripts/bench_rig.py's: the recorded run "4" (four 384 x 512 frames, a 1081 x 527 mosaic, three steps), 16 sets per
call, a run = one call ending in a wait for the device, device events and the wall clock around it, the median of `--runs` runs
after `--warmup` calls.  Variants: vertical seams (the replay as it is), fixed paths (the masked blend alone: a stored level-0 mask,
no implicit mask, no source fusion), and per-set paths (the finder in front of it).  The added microseconds per set and step are
reported for the masked blend (fixed - vertical) and for the finder (per-set - fixed).  `--off-only` measures the vertical seams
alone: run under STITCH_LIB with a build of the parent tree, its result is the yardstick that this tree's is compared with, and
`--parent-json` takes it into the output.

Then the stand-alone finder on a 4421 x 2315 canvas with a full-height overlap 600 columns wide, for K in {1, 8}, beside an
instruction-issue estimate of the dynamic programme's row: one workgroup of 16 wavefronts, 4 per SIMD, every wavefront issuing its
32 K + 15 instructions for each of its 5 states of the row (ceil(4422 / 1024)) at CYCLES_PER_INSTR cycles each while the four take turns,
plus the barrier -- the chain of rows is the launch's time, and the estimate leaves out the cost pass, the walk back and every wait
for memory.

And, for information, the monitor's ssd at shift (0, 0) (capi.dev_pairs_residual at radius 0, through pipeline.stitch_chain) in a
band of 8 columns either side of the seam, for the chain with vertical (geometric) seams against the chain along found paths, each
on its own blend inputs, on the committed frames.  Prints one JSON line and writes it to profiles/seam_path_bench.json.

    python scripts/bench_seam_path.py [--runs 5] [--warmup 2] [--off-only] [--parent-json PATH] [--out PATH | --no-write]
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

# One state of k_seam_path_dp's row, counted in its gfx950 ISA (make -C computervisionimagestich2_amd/csrc asm; the row loop is the
# block of _ZN2sk14k_seam_path_dpIJEEEvPKjiiiPhPimPymDpT_, the instantiation without an anchor, that ends in its one s_barrier, 644 instructions for the nine unrolled states).
# The loop over k = 1 .. K of one state is 32 instructions per pass where both candidates s - k and s + k are inside the row: 2
# ds_read_b64, 2 v_cmp_lt_u64 and 6 v_cndmask_b32 (value low, value high, offset, per candidate), 2 bounds compares, 2 s_waitcnt, and
# 16 of address arithmetic, exec masking and the back edge (25 per pass at the row's ends, where one side is left).  Around it a
# state has 14 to 15: the centre's ds_read_b64, the 64-bit add, ds_write_b64, global_store_byte, the next row's global_load_dword
# and their addresses ((644 - 9 * 57) / 9).
CYCLES_PER_INSTR, CYCLES_PER_US, WAVES_PER_SIMD, BARRIER_CYCLES = 4, 2400.0, 4, 100


def row_instr(K):
    return 32 * K + 15


def dp_estimate_us(cw, ch, K):
    per_thread = -(-(cw + 1) // 1024)
    return ch * (per_thread * row_instr(K) * CYCLES_PER_INSTR * WAVES_PER_SIMD + BARRIER_CYCLES) / CYCLES_PER_US


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--off-only", action="store_true")
    ap.add_argument("--parent-json")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "seam_path_bench.json"))
    ap.add_argument("--no-write", action="store_true")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_seam_path needs the MI355X"
    dev = torch.device("cuda:0")
    gold = os.path.join(ROOT, "tests", "golden")
    with open(os.path.join(gold, "golden.json")) as f:
        steps = json.load(f)["runs"]["4"]["steps"]
    base = [torch.from_numpy(np.ascontiguousarray(bmp.load_bmp(os.path.join(gold, "input", f"{i}.bmp")))).to(dev) for i in range(1, 5)]
    sets = [[f.clone() for f in base] for _ in range(16)]
    sizes = [(f.shape[2], f.shape[1]) for f in base]
    rig = capi.Rig.from_steps(sizes, None, steps)
    outs = [torch.empty((3, rig.height, rig.width), dtype=torch.uint8, device=dev) for _ in range(16)]
    ns = len(steps)
    res = {"device": torch.cuda.get_device_name(0), "library": "STITCH_LIB" if os.environ.get("STITCH_LIB") else "this tree", "sets": 16, "steps": ns, "runs": args.runs,
           "warmup": args.warmup,
           "timing": "one rig.stitch call of 16 sets per run, ending in a wait for the device; device events and wall clock around it; median of "
                     "the runs after the warm-up calls"}
    want = [o.clone() for o in rig.stitch(sets, out=outs)[0]]
    res["vertical"] = timeit(lambda: rig.stitch(sets, out=outs), args.runs, args.warmup, 16)
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
        res["vertical_parent_tree"] = {k: parent["vertical"][k] for k in ("device_ms_median", "wall_ms_median", "device_ms", "wall_ms")}
    K, m = 2, 8
    rig.set_seam_paths(K, m)
    rig.stitch(sets, out=outs)
    res["per_set_paths"] = timeit(lambda: rig.stitch(sets, out=outs), args.runs, args.warmup, 16)
    found = [rig.last_seam_paths(0, k) for k in range(ns)]
    rig.fix_seam_paths([p for p, _ in found])
    rig.stitch(sets, out=outs)
    res["fixed_paths"] = timeit(lambda: rig.stitch(sets, out=outs), args.runs, args.warmup, 16)
    rig.clear_seam_paths()
    again = rig.stitch(sets, out=outs)[0]
    res["vertical_again"] = timeit(lambda: rig.stitch(sets, out=outs), args.runs, args.warmup, 16)
    res["outputs_equal_before_and_after_paths"] = all(bool((a == b).all()) for a, b in zip(again, want))
    base_ms = res["vertical_parent_tree"]["device_ms_median"] if args.parent_json else res["vertical"]["device_ms_median"]
    res["opts"] = {"max_step": K, "margin": m}
    res["added_us_per_set_and_step"] = {"against": "the parent tree's replay" if args.parent_json else "this tree's vertical seams",
                                        "masked_blend": (res["fixed_paths"]["device_ms_median"] - base_ms) * 1e3 / 16 / ns,
                                        "finder": (res["per_set_paths"]["device_ms_median"] - res["fixed_paths"]["device_ms_median"]) * 1e3 / 16 / ns}
    res["path_costs_set0"] = [int(c) for _, c in found]

    # ---- the stand-alone finder: a 4421 x 2315 canvas, the overlap columns 1821 .. 2420 at full height ----
    cw, ch = 4421, 2315
    g = torch.Generator(device="cpu").manual_seed(4)
    frame = torch.randint(0, 256, (3, ch, 2600), dtype=torch.uint8, generator=g).to(dev)
    mosaic = torch.randint(0, 256, (3, ch, 2421), dtype=torch.uint8, generator=g).to(dev)
    cov_a = torch.zeros((ch, cw), dtype=torch.uint8, device=dev)
    cov_b = torch.zeros((ch, cw), dtype=torch.uint8, device=dev)
    cov_a[:, 1821:] = 255
    cov_b[:, :2421] = 255
    pair = [(frame, [1, 0, 0, -1821, 0, 1, 0, 0], 0.0, 0.0, mosaic, 0, 0)]
    res["standalone_4421x2315"] = {}
    for K in (1, 8):
        paths, costs = capi.dev_pairs_seam_path(pair, cw, ch, [cov_a], [cov_b], [1], K, 8)
        t = timeit(lambda: capi.dev_pairs_seam_path(pair, cw, ch, [cov_a], [cov_b], [1], K, 8), args.runs, args.warmup, 1)
        est = dp_estimate_us(cw, ch, K)
        p = paths[0].cpu().numpy()
        res["standalone_4421x2315"][f"K{K}"] = dict(t, cost=int(costs[0]), path_min=int(p.min()), path_max=int(p.max()), row_instr_per_state=row_instr(K),
                                                    dp_estimate_us=est, measured_over_estimate=t["device_ms_median"] * 1e3 / est)
    res["estimate"] = (f"rows x (5 states x (32 K + 15) wavefront instructions x {CYCLES_PER_INSTR} cycles x {WAVES_PER_SIMD} wavefronts per SIMD + "
                       f"{BARRIER_CYCLES} cycles of barrier) / {CYCLES_PER_US:.0f} cycles per us: the dynamic programme's chain of rows alone")

    # ---- for information: the monitor's ssd at shift (0, 0) in a band around the seam, vertical against path, committed frames ----
    # Each variant on its OWN inputs: the chain with vertical (geometric) seams and the chain along the paths it finds, each measured by
    # capi.dev_pairs_residual at radius 0 (pipeline.stitch_chain(residuals=...)) over A & B within 8 columns either side of its seam.
    from computervisionimagestich2_amd import pipeline
    rig2 = capi.Rig.from_steps(sizes, None, steps)
    geo = rig2.geometric_seams().seams
    both = [(rig2.coverage(k, 0), rig2.coverage(k, 1)) for k in range(ns)]
    rig2.close()

    def band(k, cols, half=8):
        x = torch.arange(steps[k]["cw"], device=dev)[None, :]
        c = torch.as_tensor(np.asarray(cols, np.int64), device=dev)[:, None]
        return (((x >= c - half) & (x < c + half) & (both[k][0] != 0) & (both[k][1] != 0)).to(torch.uint8) * 255).contiguous()

    v_cols = [int(np.ceil(s_[2] / s_[3])) if s_[4] == 0 else s_[5] for s_ in geo]
    _, v_rec = pipeline.stitch_chain(base, steps, finish=False, seams=geo,
                                     residuals=dict(radius=0, domains=[band(k, np.full(steps[k]["ch"], v_cols[k])) for k in range(ns)]))
    sp_args = dict(coverage=both, branches=[s_[4] for s_ in geo], max_step=2, margin=8)
    _, found2 = pipeline.stitch_chain(base, steps, finish=False, seam_paths=sp_args)
    paths2 = [p_.cpu().numpy() for p_, _ in found2]
    _, p_rec, _ = pipeline.stitch_chain(base, steps, finish=False, seam_paths=dict(sp_args, paths=paths2),
                                        residuals=dict(radius=0, domains=[band(k, paths2[k]) for k in range(ns)]))
    v_rec, p_rec = v_rec.cpu().numpy(), p_rec.cpu().numpy()
    info = [{"step": k, "branch": geo[k][4], "vertical_column": v_cols[k], "vertical_ssd": int(v_rec[k][4]), "vertical_pixels": int(v_rec[k][0]),
             "path_ssd": int(p_rec[k][4]), "path_pixels": int(p_rec[k][0]), "path_min": int(paths2[k].min()), "path_max": int(paths2[k].max()),
             "path_cost": int(found2[k][1])} for k in range(ns)]
    res["band_ssd_committed_frames"] = {"band": "8 columns either side of the seam, over A & B; each variant's own blend inputs; the monitor's record at radius 0: "
                                                "n and ssd of shift (0, 0)", "steps": info}
    rig.close()
    line = json.dumps(res)
    print(line)
    assert res["outputs_equal_before_and_after_paths"], "paths left a trace in the replay"
    if not args.no_write:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
