"""Temporally anchored path seams on one MI355X (include/stitch_seam_anchor.h): what the anchor adds to a rig's replay along found paths.

The protocol is scripts/bench_seam_path.py's: the recorded run "4" (four 384 x 512 frames, a 1081 x 527 mosaic, three steps), a run =
one call ending in a wait for the device, device events and the wall clock around it, the median of `--runs` runs after `--warmup`
calls; finder options K = 2, m = 8; anchor options weight 32, cap 64.  Measured:
  (i)  16 sets per call: found paths without an anchor, anchored per call (one parallel finder sequence per step, as without),
       anchored per set (the step's 16 dynamic programmes one after another, one launch of one workgroup each);
  (ii) 1 set per call, the live-video form, the 16 sets in turn: without an anchor against anchored (the policies coincide).
The anchored rigs are not reset between calls: the stream goes on, as in video.  `--parent-only` measures the unanchored forms alone:
run under STITCH_LIB with a build of the parent tree it gives the parent's replay, which `--parent-json` takes into the output.

What to expect, written down before the first run (EXPECTED below): DESIGN.md section 21 measured 0.79 ms per step for the finder of
16 sets in parallel, of which about 0.57 ms is the chain of 520 rows of one dynamic programme.  Per set, the step's 16 chains follow
each other, so each step should gain about 15 chains, 3 x 15 x 0.57 = 25.6 ms per call on top of the unanchored replay.  Per call,
and with one set per call, the anchored state adds a subtract, an absolute value, a minimum, a multiply and a wider add to the 79
wavefront instructions of a state at K = 2 -- 5 to 8 per cent of the chain, 0.03 to 0.05 ms per step.

And, for information, the flicker table: 16 sets made of the committed frames plus independent uniform integer noise in [-8, 8] per
set (numpy default_rng(100 + set), clipped to 0 .. 255), through one call per variant; per step the mean |s_i[y] - s_(i-1)[y]| over
the 15 consecutive pairs of sets and all rows, and the mean cost of a path under c (D - weight * moved), for found paths without an
anchor and anchored per set at a few weights with cap 64.  Prints one JSON line and writes it to profiles/seam_anchor_bench.json.

    python scripts/bench_seam_anchor.py [--runs 5] [--warmup 2] [--parent-only] [--parent-json PATH] [--out PATH | --no-write]
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

K, MARGIN, WEIGHT, CAP = 2, 8, 32, 64
CHAIN_MS = 0.57  # the chain of rows of one dynamic programme on these canvases
EXPECTED = {
    "per_set_16_added_ms_per_call": 3 * 15 * CHAIN_MS,
    "per_call_16_added_ms_per_call": [3 * 0.05 * CHAIN_MS, 3 * 0.08 * CHAIN_MS],
    "one_set_added_ms_per_call": [3 * 0.05 * CHAIN_MS, 3 * 0.08 * CHAIN_MS],
    "reasoning": "per set: 15 more chains of 0.57 ms per step, three steps; per call and one set per call: 4 to 6 more wavefront instructions on the 79 of a state",
}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--parent-only", action="store_true")
    ap.add_argument("--parent-json")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "seam_anchor_bench.json"))
    ap.add_argument("--no-write", action="store_true")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_seam_anchor needs the MI355X"
    dev = torch.device("cuda:0")
    gold = os.path.join(ROOT, "tests", "golden")
    with open(os.path.join(gold, "golden.json")) as f:
        steps = json.load(f)["runs"]["4"]["steps"]
    base = [np.ascontiguousarray(bmp.load_bmp(os.path.join(gold, "input", f"{i}.bmp"))) for i in range(1, 5)]
    noisy = []
    for i in range(16):
        rng = np.random.default_rng(100 + i)
        noisy.append([torch.from_numpy(np.clip(f.astype(np.int64) + rng.integers(-8, 9, f.shape), 0, 255).astype(np.uint8)).to(dev) for f in base])
    sets = [[torch.from_numpy(f).to(dev) for f in base] for _ in range(16)]
    sizes = [(f.shape[2], f.shape[1]) for f in base]
    ns = len(steps)
    rig = capi.Rig.from_steps(sizes, None, steps)
    outs = [torch.empty((3, rig.height, rig.width), dtype=torch.uint8, device=dev) for _ in range(16)]
    res = {"device": torch.cuda.get_device_name(0), "library": "STITCH_LIB" if os.environ.get("STITCH_LIB") else "this tree", "steps": ns, "runs": args.runs,
           "warmup": args.warmup, "opts": {"max_step": K, "margin": MARGIN, "weight": WEIGHT, "cap": CAP},
           "timing": "one rig.stitch call per run, ending in a wait for the device; device events and wall clock around it; median of the runs after "
                     "the warm-up calls; the frames are the noisy sets of the flicker table, so that an anchored path has something to hold against",
           "expected_before_the_first_run": EXPECTED}
    turn = [0]

    def one_set():
        i = turn[0] % 16
        turn[0] += 1
        rig.stitch([noisy[i]], out=outs[:1])

    def measure(tag):
        rig.stitch(noisy, out=outs)
        res[f"{tag}_16_sets"] = timeit(lambda: rig.stitch(noisy, out=outs), args.runs, args.warmup, 16)
        turn[0] = 0
        res[f"{tag}_1_set"] = timeit(one_set, 3 * args.runs, 16 + args.warmup, 1)  # (the 16 sets once in the warm-up; 15 timed calls)

    rig.set_seam_paths(K, MARGIN)
    measure("unanchored")
    if args.parent_only:
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
        res["parent_tree"] = {k: {q: parent[k][q] for q in ("device_ms_median", "wall_ms_median", "device_ms", "wall_ms")} for k in ("unanchored_16_sets", "unanchored_1_set")}
    rig.set_seam_anchor(WEIGHT, CAP, "call")
    measure("per_call")
    rig.reset_seam_anchor().set_seam_anchor(WEIGHT, CAP, "set")
    measure("per_set")
    rig.clear_seam_anchor()
    measure("unanchored_again")
    d = {k: res[k]["device_ms_median"] for k in res if k.endswith("_sets") or k.endswith("_set")}
    res["added_ms_per_call"] = {"against": "this tree's unanchored replay (the median of before and after)",
                                "per_call_16": d["per_call_16_sets"] - (d["unanchored_16_sets"] + d["unanchored_again_16_sets"]) / 2,
                                "per_set_16": d["per_set_16_sets"] - (d["unanchored_16_sets"] + d["unanchored_again_16_sets"]) / 2,
                                "per_call_1": d["per_call_1_set"] - (d["unanchored_1_set"] + d["unanchored_again_1_set"]) / 2,
                                "per_set_1": d["per_set_1_set"] - (d["unanchored_1_set"] + d["unanchored_again_1_set"]) / 2}
    res["per_set_launches"] = "one launch of one workgroup per set and step (the one-launch form that walks the sets was not built: not measured)"

    # ---- for information: flicker and cost on 16 noisy sets, one call per variant ----
    def table(weight):
        rig.clear_seam_anchor()
        if weight is not None:
            rig.set_seam_anchor(weight, CAP, "set")
        rig.stitch(noisy, out=outs)
        rows = []
        for k in range(ns):
            paths, under_c = [], []
            for i in range(16):
                p, cost = rig.last_seam_paths(i, k)
                paths.append(p.astype(np.int64))
                under_c.append(cost - (weight or 0) * rig.last_seam_moved(i, k))
            jump = np.mean([np.abs(paths[i] - paths[i - 1]).mean() for i in range(1, 16)])
            rows.append({"step": k, "mean_abs_column_change": float(jump), "mean_cost_under_c": float(np.mean(under_c)), "cost_under_c_set0": int(under_c[0])})
        return rows

    res["flicker"] = {"frames": "the committed run-4 frames plus uniform integer noise in [-8, 8] per set, numpy default_rng(100 + set), clipped to 0 .. 255",
                      "cap": CAP, "policy": "per set, one call of 16 sets, the first set unanchored",
                      "unanchored": table(None), **{f"weight_{w}": table(w) for w in (1, 4, 16, 32)}}
    # and the replay of clean frames is what it was: weight 0 against no anchor, byte for byte
    rig.clear_seam_anchor()
    want = [o.clone() for o in rig.stitch(sets, out=outs)[0]]
    got = rig.set_seam_anchor(0, CAP, "set").stitch(sets, out=outs)[0]
    res["weight_0_equals_unanchored"] = all(bool((a == b).all()) for a, b in zip(got, want))
    rig.close()
    line = json.dumps(res)
    print(line)
    assert res["weight_0_equals_unanchored"], "weight 0 changed the replay"
    if not args.no_write:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
