"""Map estimation (k_ransac.inc) on one MI355X; prints one JSON line and writes it to profiles/ransac_bench.json.

  input_lists     the 14 lists of the reference's Input/ frames (tests/golden/ransac_input.npz: 7 accepted lists and their mirrors)
                  as ONE dev_ransac_many call, device events around back-to-back calls; next to it the reference's own
                  ImageProcess::RANSAC (oracle/_ref/libref_hotpath.so through ctypes) on the same lists on this host's CPU,
                  where that library was built
  n16384_r72, n16384_r4096, lists64_n1000
                  synthetic lists (40 % outliers), device events.  `consensus_valu_bound_ms` is the bound of the consensus stage
                  alone: per (round, point) 14 double multiply/adds and 4 conversions at 4 cycles per
                  wave64 instruction and 8 float instructions at 2, on 256 CUs x 4 SIMDs at CLOCK_GHZ.
Per-stage times come from a kernel trace taken in a run of its own:
    rocprofv3 --kernel-trace --stats -d <dir> -- python scripts/bench_ransac.py --only n16384_r4096 --reps 5
Every timed result is compared with a first run (bit-identical) before it is reported.

    python scripts/bench_ransac.py [--reps 20] [--only NAME] [--no-write]
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
import torch  # noqa: E402

from computervisionimagestich2_amd import capi  # noqa: E402

CLOCK_GHZ = 2.4  # MI355X peak engine clock (the bound is the best case; the chip may hold a lower clock under load)
CYCLES_PER_WAVE_EVAL = 14 * 4 + 4 * 4 + 8 * 2  # one wavefront = 64 (round, point) evaluations
SIMDS = 256 * 4


def timeit(fn, reps, runs=5):
    """Median over `runs` of the mean time of `reps` back-to-back calls (device events), after a warm-up."""
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(runs):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b) / reps)
    return statistics.median(out)


def synth(rng, n, outliers=0.4):
    sx, sy = (rng.random(n) * 600).astype(np.float32), (rng.random(n) * 450).astype(np.float32)
    x, y = sx.astype(np.float64), sy.astype(np.float64)
    dx = (0.97 * x - 0.02 * y + 1.5e-4 * x * y + 180.0 + rng.normal(0, 0.8, n)).astype(np.float32)
    dy = (0.01 * x + 1.03 * y - 1e-4 * x * y - 7.0 + rng.normal(0, 0.8, n)).astype(np.float32)
    bad = rng.random(n) < outliers
    dx[bad] = (rng.random(int(bad.sum())) * 600).astype(np.float32)
    dy[bad] = (rng.random(int(bad.sum())) * 450).astype(np.float32)
    return sx, sy, dx, dy


def entry(lst, dev):
    return {k: torch.from_numpy(np.ascontiguousarray(v)).to(dev) for k, v in zip(("src_x", "src_y", "dst_x", "dst_y"), lst)}


def measure(lists, opts, reps):
    def run():
        return capi.dev_ransac_many(lists, opts, want_inliers=False)
    p0, i0, _ = run()
    p0, i0 = p0.cpu().numpy(), i0.cpu().numpy()
    ms = timeit(run, reps)
    p1, i1, _ = run()
    assert np.array_equal(p0.view(np.uint64), p1.cpu().numpy().view(np.uint64)) and np.array_equal(i0, i1.cpu().numpy())
    return ms, p0, i0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--only", default="")
    ap.add_argument("--no-write", action="store_true")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_ransac needs the MI355X"
    dev = torch.device("cuda:0")
    res = {"device": torch.cuda.get_device_name(0), "clock_ghz_for_bound": CLOCK_GHZ, "reps": args.reps,
           "timing": "median of 5 runs of `reps` back-to-back calls between device events, after 3 warm-up calls"}

    def want(name):
        return not args.only or args.only == name

    gold = os.path.join(ROOT, "tests", "golden")
    if want("input_lists"):
        z = np.load(os.path.join(gold, "ransac_input.npz"))
        host = []
        for key in sorted(k[:-3] for k in z.files if k.endswith("_sx")):
            lst = tuple(z[f"{key}_{c}"] for c in ("sx", "sy", "dx", "dy"))
            host += [lst, (lst[2], lst[3], lst[0], lst[1])]
        ms, p, info = measure([entry(l, dev) for l in host], None, args.reps * 5)
        r = {"lists": len(host), "pairs": [len(l[0]) for l in host], "gpu_ms_per_call": ms, "winning_counts": info[:, 3].tolist()}
        if os.path.exists(os.path.join(ROOT, "oracle", "_ref", "libref_hotpath.so")):
            sys.path.insert(0, gold)
            import make_ransac_goldens as M
            M.call_reference(*host[0])
            t0 = time.perf_counter()
            ref = [M.call_reference(*l) for l in host]
            r["reference_cpu_ms"] = (time.perf_counter() - t0) * 1e3
            r["reference_maps_equal"] = all(np.array_equal(a.view(np.uint64), b.view(np.uint64)) for a, b in zip(ref, p))
        res["input_lists"] = r

    rng = np.random.default_rng(1)
    for name, n, rounds, nlists in (("n16384_r72", 16384, 72, 1), ("n16384_r4096", 16384, 4096, 1), ("lists64_n1000", 1000, 72, 64)):
        if not want(name):
            continue
        lists = [entry(synth(rng, n), dev) for _ in range(nlists)]
        ms, p, info = measure(lists, capi.RansacOpts(rounds=rounds), args.reps)
        evals = n * rounds * nlists
        bound = evals / 64 * CYCLES_PER_WAVE_EVAL / SIMDS / (CLOCK_GHZ * 1e9) * 1e3
        inl = int(info[:, 3].sum())
        res[name] = {"n": n, "rounds": rounds, "lists": nlists, "ms_per_call": ms, "evaluations": evals, "consensus_valu_bound_ms": bound,
                     "inlier_rows_fitted": inl, "all_ok": bool((info[:, 0] == 0).all())}
    line = json.dumps(res)
    print(line)
    if not args.no_write and not args.only:
        with open(os.path.join(ROOT, "profiles", "ransac_bench.json"), "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
