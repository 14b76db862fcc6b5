"""The mask pyramid kept per slot (include/stitch_mask_keep.h), timed: a 16-pair sequence at 6144 x 4096 with standing pyramids (scanned
and given seams) and with given seams that all change on every call (k_mask_keys plus nothing saved), and the 4421 x 2315 batch of
scripts/bench_realcanvas.py (8 pairs per sequence, 4 sequences in flight).  For the library STITCH_LIB names, or the tree's: run it
once with each for an A/B (profiles/mask_keep_ab.txt).  One JSON line.  Usage: python scripts/bench_mask_keep.py"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
from computervisionimagestich2_amd import capi  # noqa: E402

dev = torch.device("cuda:0")


def timed(fn, n, warm):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    t = time.perf_counter()
    for _ in range(n):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) / n * 1e3


def counts(plan):
    return list(plan.mask_keep_counts()) if hasattr(capi.lib(), "stitch_plan_mask_keep_counts") else None


res = {"lib": os.path.basename(os.environ.get("STITCH_LIB", "tree"))}
# (a) config 2's geometry: 16 pairs per sequence, one sequence in flight
cw, ch, fw, fh, n = 6144, 4096, 4096, 4096, 16
plan = capi.Plan(cw, ch, max_pairs=n)
F = [capi.dev_synth(fw, fh, 2 * i + 1, torch.float32, dev) for i in range(2)]
M = [capi.dev_synth(fw, fh, 2 * i, torch.float32, dev) for i in range(2)]
outs = [torch.empty((3, ch, cw), dtype=torch.float32, device=dev) for _ in range(n)]
items = [(F[i % 2], [1.0, 0.002, 1e-6, -(2048.0 + 8 * i), -0.001, 1.0, 5e-7, 1.5], 0.0, 0.0, M[i % 2], 0, 0, outs[i]) for i in range(n)]
plan.pairs(items)
seams_a = [plan.status(i).as_tuple() for i in range(n)]
seams_b = [(s[0], s[1], s[2] - 8 * s[3], s[3]) + tuple(s[4:]) for s in seams_a]
res["scan_standing_ms_per_call"] = round(timed(lambda: plan.pairs(items), 10, 3), 4)
plan.status()
res["scan_standing_counts"] = counts(plan)
res["given_standing_ms_per_call"] = round(timed(lambda: plan.pairs(items, seams=seams_a), 10, 3), 4)
plan.status()
res["given_standing_counts"] = counts(plan)
flip = [0]


def moving():
    flip[0] ^= 1
    plan.pairs(items, seams=seams_b if flip[0] else seams_a)


res["given_moving_ms_per_call"] = round(timed(moving, 10, 3), 4)
plan.status()
res["given_moving_counts"] = counts(plan)
plan.close()
del F, M, outs, items
# (b) a real canvas: 4421 x 2315, 8 pairs per sequence, 4 sequences in flight
cw, ch, fw, fh, n, lanes = 4421, 2315, 1536, 2048, 8, 4
Fr, Mo = capi.dev_synth(fw, fh, 1, torch.float32, dev), capi.dev_synth(cw - fw // 2, ch - 7, 2, torch.float32, dev)
plans = [capi.Plan(cw, ch, max_pairs=n) for _ in range(lanes)]
streams = [torch.cuda.Stream() for _ in range(lanes)]
its = [[(Fr, [1.0, 0.002, 1e-6, -(cw - fw - 3.0) + 4 * i, -0.001, 1.0, 5e-7, -3.5], -0.25, -1.5, Mo, 0, -2,
         torch.empty((3, ch, cw), dtype=torch.float32, device=dev)) for i in range(n)] for _ in range(lanes)]


def step():
    for p, s, it in zip(plans, streams, its):
        with torch.cuda.stream(s):
            p.pairs(it)


runs = [round(timed(step, 20, 5) / (n * lanes), 4) for _ in range(2)]
res["real_canvas_4421x2315_ms_per_pair"] = runs
for p in plans:
    p.status()
res["real_canvas_counts"] = counts(plans[0])
res["real_canvas_keep_form"] = plans[0].mask_keep_form(n) if hasattr(plans[0], "mask_keep_form") else None
for p in plans:
    p.close()
print(json.dumps(res))
