"""Times the single-image projection, equalise and finish calls of the package under the given checkout root, for an A/B of two
builds of the same kernels (run it once per root, alternating, in one GPU session): ms per call, (median, minimum) of 7 runs of
20 back-to-back calls between device events, after 3 warm-up calls.  Prints one JSON line.

    python scripts/ab_single_image_kernels.py ROOT
"""
import statistics, sys, json
root = sys.argv[1]
sys.path.insert(0, root)
import torch
from computervisionimagestich2_amd import capi
dev = torch.device("cuda:0")
def t(fn, runs=7, warm=3, inner=20):
    for _ in range(warm): fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(runs):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(inner): fn()
        b.record(); torch.cuda.synchronize()
        out.append(a.elapsed_time(b) / inner)
    return round(statistics.median(out), 5), round(min(out), 5)
res = {"root": root}
for name, w, h, dt in (("proj_u8_portrait", 4096, 4096, torch.uint8), ("proj_u8_landscape", 4096, 3072, torch.uint8), ("proj_f32_portrait", 4096, 4096, torch.float32),
                       ("proj_u8_untiled", 4094, 4096, torch.uint8), ("proj_u8_small", 384, 512, torch.uint8)):
    src = capi.dev_synth(w, h, 1, dt, dev); out = torch.empty_like(src)
    res[name] = t(lambda: capi.dev_project(src, out=out))
for name, w, h in (("finish_words", 6144, 4096), ("finish_bytes", 4421, 2315), ("finish_small", 1081, 527)):
    img = capi.dev_synth(w, h, 2, torch.uint8, dev)
    res[name] = t(lambda: capi.dev_finish(img))
    res[name.replace("finish", "equalize")] = t(lambda: capi.dev_equalize(img))
print(json.dumps(res))
