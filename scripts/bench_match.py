"""Descriptor matcher (k_match.inc) on one MI355X; prints one JSON line.

  input_all_pairs   the 12 ordered getImgPair calls of ImageProcess::matching on the reference's Input/ frames (descriptors
                    from tests/golden/match_frame*.npz, map order) as ONE dev_match_many launch sequence, device events;
                    next to it the reference's own kd-forest (vl_kdforest, oracle/_ref/libref_hotpath.so) on the same
                    descriptors on this host's CPU, where that library was built
  square_<n>        n x n synthetic SIFT-like sets (n data rows, n queries), dev_match, device events; the VALU bound is
                    2 VALU instructions per (pair, dimension) -- v_sub_f32 and v_add_f32 with |x| -- at 256 CUs x 4 SIMDs x 32
                    lanes per clock and CLOCK_GHZ, and `of_valu_bound` = that bound / the measured time
Every timed result is checked against a first run (bit-identical) before it is reported.

    python scripts/bench_match.py [--reps 20]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from computervisionimagestich2_amd import capi  # noqa: E402

CLOCK_GHZ = 2.4  # MI355X peak engine clock (the bound is the best case; the chip may hold a lower clock under load)
VALU_LANES_PER_CLK = 256 * 4 * 32


def timeit(fn, reps):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def snapshot(outs):
    return [tuple(t.cpu().numpy().copy() for t in (o["pairs"], o["count"], o["nn"])) for o in outs]


def same(a, b):
    return all(all(np.array_equal(x, y) for x, y in zip(p, q)) for p, q in zip(a, b))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--sizes", default="4096,16384,32768")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_match needs the MI355X"
    dev = torch.device("cuda:0")
    res = {"clock_ghz_for_bound": CLOCK_GHZ}

    gold = os.path.join(ROOT, "tests", "golden")
    F = []
    for i in range(1, 5):
        z = np.load(os.path.join(gold, f"match_frame{i}.npz"))
        F.append(z["desc"][z["map_idx"]])
    d = [torch.from_numpy(f).to(dev) for f in F]
    sets = [(d[i], d[j]) for i in range(4) for j in range(4) if i != j]
    first = snapshot(capi.dev_match_many(sets, want_dist=False))
    ms = timeit(lambda: capi.dev_match_many(sets, want_dist=False), args.reps * 10)
    assert same(first, snapshot(capi.dev_match_many(sets, want_dist=False)))
    counts = [int(c[1][0]) for c in first]
    comparisons = sum(a.shape[0] * b.shape[0] for a, b in sets)
    res["input_all_pairs"] = {"sets": len(sets), "descriptors": [len(f) for f in F], "counts": counts, "gpu_ms": ms,
                              "pair_distances": comparisons}
    ref_so = os.path.join(ROOT, "oracle", "_ref", "libref_hotpath.so")
    if os.path.exists(ref_so):
        sys.path.insert(0, gold)
        import make_match_goldens as M
        L = M.load()
        t0 = time.perf_counter()
        ref_counts = [len(M.kdforest_pairs(L, F[i], F[j])[3]) for i in range(4) for j in range(4) if i != j]
        res["input_all_pairs"]["reference_kdforest_cpu_ms"] = (time.perf_counter() - t0) * 1e3
        res["input_all_pairs"]["reference_counts_equal"] = ref_counts == counts

    rng = np.random.default_rng(1)
    for n in [int(s) for s in args.sizes.split(",")]:
        db = (rng.random((n, 128), dtype=np.float32) * 0.3).astype(np.float32)
        q = db + (rng.random((n, 128), dtype=np.float32) * 0.01).astype(np.float32)
        q[n // 2:] = (rng.random((n - n // 2, 128), dtype=np.float32) * 0.3).astype(np.float32)
        x, y = torch.from_numpy(db).to(dev), torch.from_numpy(q).to(dev)
        first = snapshot([capi.dev_match(x, y)])
        ms = timeit(lambda: capi.dev_match(x, y), args.reps)
        assert same(first, snapshot([capi.dev_match(x, y)]))
        bound_ms = n * n * 128 * 2 / VALU_LANES_PER_CLK / (CLOCK_GHZ * 1e9) * 1e3
        res[f"square_{n}"] = {"ms": ms, "valu_bound_ms": bound_ms, "of_valu_bound": bound_ms / ms, "accepted": int(first[0][1][0]),
                              "Gpair_dims_per_s": n * n * 128 / ms / 1e6}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
