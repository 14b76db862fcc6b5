"""Walks the pair path's launch choices in a fixed order, one call per case, so that a kernel trace of the run lists every dispatch
the choices lead to; and compares two such traces.

  rocprofv3 --kernel-trace --output-format csv -d DIR -o NAME -- python scripts/trace_call_forms.py
      every (switch, value, extra environment, shape, form, pixel type) of tests/switch_table.py whose form is a pair call, then the
      flag tests' shapes (tests/g_flags_ref.py's forms) with one and two pairs, then every case of tests/form_cover.py's two tables -- every
      form the decision reaches at default switches -- in both pixel types.  The environment is set before each plan is created.
      Then the band path (pipeline.LocalBandGroup: every band of a pair from one host thread, so the order of launches is fixed): the
      shapes of tests/test_gpu_band.py in every form of test_band_group_single_host_thread, both pixel types, under the band switches.
      Inputs are synthetic; nothing is compared -- the launches do not depend on the data.  STITCH_LIB selects the library.
  python scripts/trace_call_forms.py --compare A_kernel_trace.csv B_kernel_trace.csv [--out FILE] [--note TEXT]
      the two ordered lists of (kernel, grid, workgroup, LDS bytes, scratch bytes), line for line.
"""
import argparse
import csv
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import form_cover  # noqa: E402
import form_cover_refs  # noqa: E402
import g_flags_ref  # noqa: E402
import switch_table as T  # noqa: E402

FLAG_SHAPES = [(1088, 136), (1152, 192), (1020, 192), (1024, 4224), (1024, 768)]
FORMS = ("lone", "batch", "blend", "host")


def image(w, h, seed, dtype):
    y, x = np.mgrid[0:h, 0:w]
    g = np.stack([(x * (3 + c) + y * (5 - c) + 17 * seed) % 251 + 1 for c in range(3)]).astype(np.float32)
    return np.ascontiguousarray(g.astype(dtype))


def pair_inputs(cw, ch, i, dtype):
    fw, fh = cw * 5 // 8 - 13 * i, ch - 5 - 3 * i
    P = [1.0, 0.002, 1e-6, -(cw - fw - 3.0 - 5 * i), -0.001, 1.0, 5e-7, -3.5 + i]
    return image(fw, fh, 2 * i + 1, dtype), P, -0.25, -1.5, image(cw - fw // 2 + 9 * i, ch - 7, 2 * i, dtype), 0, -2


def cover_inputs(cw, ch, i, dtype):
    """Pair i of a case of form_cover.CASES: the placements of tests/test_gpu_form_cover.py's first call (canvases down to 3 x 3)."""
    fw, P, mw, ox, _ = form_cover.inputs(cw)[g_flags_ref.BATCHES[0][i % 2]]
    return image(fw, ch, 2 * i + 1, dtype), P, 0.0, 0.0, image(mw, ch, 2 * i, dtype), ox, 0


def set_env(settings):
    for k in list(T.SWITCHES) + [k for k in T.EXEMPT if k != "STITCH_LIB"]:
        os.environ.pop(k, None)
    for k, v in settings.items():
        if v is not None:
            os.environ[k] = v


def cases():
    for name, value, extra in T.cases():
        sw = T.SWITCHES[name]
        for shape in sw["shapes"]:
            for form in sw["forms"]:
                if form in FORMS:
                    for dtype in (np.uint8, np.float32):
                        cw, ch = T.SHAPES[shape]
                        n = (2 if cw >= 4096 else 3) if form == "batch" else 1
                        yield {**extra, name: value}, cw, ch, form, n, n, dtype, None
    for cw, ch in FLAG_SHAPES:
        for form in sorted(g_flags_ref.FORMS):
            for n in (1, 2):
                for dtype in (np.uint8, np.float32):
                    yield g_flags_ref.FORMS[form], cw, ch, "batch", 2, n, dtype, g_flags_ref.OPTS
    for cw, ch, cap, n, dense, opts, _ in form_cover_refs.ALL_CASES:
        for dtype in (np.uint8, np.float32):
            yield {}, cw, ch, "cover_blend" if dense else "cover", cap, n, dtype, form_cover.OPTION_SETS[opts]


# (world, canvas, split levels) of tests/test_gpu_band.py's parametrised cases and of its 132-row bands; its forms; the band switches
BAND_SHAPES = [(2, 2048, 1024, 2), (2, 2048, 1024, 3), (8, 2048, 1024, 2), (4, 1024, 512, 1), (3, 770, 384, 2), (2, 770, 384, 2), (3, 768, 384, 2), (2, 1540, 768, 2),
               (6, 772, 384, 1), (1, 1000, 500, 2), (3, 768, 396, 2)]
BAND_FORMS = (True, False, "planes", "stored", "stored+fused", "chunks4")
BAND_ENVS = ({}, {"STITCH_NO_ZERO_TILES": "1"}, {"STITCH_BAND_PLAIN": "1"}, {"STITCH_BAND_PLANES": "1"})


def band_cases():
    for world, cw, ch, Ls in BAND_SHAPES:
        for env in BAND_ENVS:
            for fuse in BAND_FORMS:
                if fuse == "chunks4" and "STITCH_BAND_PLAIN" in env:
                    continue  # (column chunks need the fused decimation: the call is refused)
                for dtype in (np.uint8, np.float32):
                    yield env, world, cw, ch, Ls, fuse, dtype


def run_bands(dev):
    import torch
    from computervisionimagestich2_amd import pipeline
    count = 0
    for env, world, cw, ch, Ls, fuse, dtype in band_cases():
        set_env(env)
        F, P, offx, offy, M, ox, oy = pair_inputs(cw, ch, 0, dtype)
        grp = pipeline.LocalBandGroup(cw, ch, Ls, world, dev, fuse_sweeps=fuse in (True, "stored+fused"), plane_pipeline_min=0 if fuse == "planes" else None,
                                      col_chunks=4 if fuse == "chunks4" else 1)
        try:
            if str(fuse).startswith("stored"):
                for b in grp.bands:
                    b.band.set_level0(False)
            for rep in range(2):  # twice: what a call leaves for the next (the live flags' level)
                grp.run(torch.from_numpy(F).to(dev), P, offx, offy, torch.from_numpy(M).to(dev), ox, oy)
            torch.cuda.synchronize()
        finally:
            grp.close()
        count += 1
    return count


def run():
    import torch
    from computervisionimagestich2_amd import capi
    dev = torch.device("cuda")
    cache, count = {}, 0

    def inputs(cw, ch, n, dtype, make):
        key = (cw, ch, n, np.dtype(dtype).name, make.__name__)
        if key not in cache:
            cache.clear()  # (one shape's tensors at a time)
            host = [make(cw, ch, i, dtype) for i in range(n)]
            cache[key] = host, [(torch.from_numpy(F).to(dev), P, ox_, oy_, torch.from_numpy(M).to(dev), ox, oy) for F, P, ox_, oy_, M, ox, oy in host]
        return cache[key]

    for env, cw, ch, form, cap, n, dtype, opts in cases():
        host, items = inputs(cw, ch, max(n, cap), dtype, cover_inputs if form.startswith("cover") else pair_inputs)
        set_env(env)
        if form == "host":
            capi.pair(*host[0], cw, ch)
        else:
            plan = capi.Plan(cw, ch, opts=opts, max_pairs=cap)
            try:
                tdt = torch.uint8 if dtype == np.uint8 else torch.float32
                if form == "cover_blend":
                    a = torch.from_numpy(image(cw, ch, 1, dtype)).to(dev)
                    plan.blend(a, a.flip(2).contiguous())
                elif form == "blend":
                    a = torch.zeros((3, ch, cw), dtype=tdt, device=dev)
                    a[:, : items[0][0].shape[1], : items[0][0].shape[2]] = items[0][0]
                    plan.blend(a, a.flip(2).contiguous())
                elif form == "lone":
                    plan.pair(*items[0])
                else:
                    plan.pairs([it + (torch.empty((3, ch, cw), dtype=tdt, device=dev),) for it in items[:n]])
                torch.cuda.synchronize()
            finally:
                plan.close()
        count += 1
        if count % 100 == 0:
            print(f"... {count}", flush=True)
    bands = run_bands(dev)
    set_env({})
    print(f"cases {count} band cases {bands}")


def dispatches(path):
    with open(path, newline="") as f:
        rows = list(csv.DictReader(f))
    rows.sort(key=lambda r: int(r["Dispatch_Id"]))
    lds = "LDS_Block_Size" if "LDS_Block_Size" in rows[0] else "Group_Segment_Size"  # (the columns' names before rocprofv3 1.0)
    scratch = "Scratch_Size" if "Scratch_Size" in rows[0] else "Private_Segment_Size"
    keep = ("Kernel_Name", "Grid_Size_X", "Grid_Size_Y", "Grid_Size_Z", "Workgroup_Size_X", "Workgroup_Size_Y", "Workgroup_Size_Z", lds, scratch)
    return [tuple(r[k] for k in keep) for r in rows]


def compare(a_path, b_path, out, note):
    """The library's and torch's dispatches are compared.  The HIP runtime's own copy and fill kernels (__amd_rocclr_*) are counted
    apart: whether a hipMemcpy of the host-buffer entry points runs as such a kernel or on a DMA engine is the runtime's choice of
    the moment, and differs between two runs of one library."""
    a, b = dispatches(a_path), dispatches(b_path)
    ra, rb = [r for r in a if r[0].startswith("__amd_rocclr_")], [r for r in b if r[0].startswith("__amd_rocclr_")]
    a, b = [r for r in a if not r[0].startswith("__amd_rocclr_")], [r for r in b if not r[0].startswith("__amd_rocclr_")]
    diff = [i for i, (x, y) in enumerate(zip(a, b)) if x != y]
    lines = [note] if note else []
    lines += [f"dispatches: {len(a)} (first trace), {len(b)} (second trace)", f"distinct kernels: {len({r[0] for r in a})}, {len({r[0] for r in b})}",
              f"the runtime's own copy / fill kernels, not compared: {len(ra)}, {len(rb)}"]
    same = len(a) == len(b) and not diff
    lines.append("verdict: IDENTICAL -- the same (kernel, grid, workgroup, LDS, scratch), dispatch for dispatch" if same else
                 f"verdict: DIFFERENT -- {len(diff)} dispatches differ, the first at index {diff[0] if diff else min(len(a), len(b))}")
    for i in diff[:10]:
        lines += [f"  [{i}] first:  {a[i]}", f"  [{i}] second: {b[i]}"]
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if out:
        with open(out, "w") as f:
            f.write(text)
    return 0 if same else 1


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--compare", nargs=2, metavar="CSV")
    ap.add_argument("--out")
    ap.add_argument("--note", default="")
    args = ap.parse_args()
    sys.exit(compare(*args.compare, args.out, args.note) if args.compare else run())
