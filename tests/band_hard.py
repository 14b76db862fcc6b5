"""Hard pixel content and bands a frame does not reach, for the band path's tests (csrc/stitch_band.inc, capi.Band,
pipeline.BandStitcher, pipeline.LocalBandGroup: ONE pair split into row bands).  A plain module like hard_inputs.py: numpy and the
oracle only, no torch, no GPU.  tests/test_band_hard_host.py holds everything below to the oracle on the CPU before any GPU run;
tests/test_gpu_band_hard.py runs the items through the band drivers.

Why: every older band test composes Oracle.synth frames (samples 1 .. 250.99, never 0) that cover the canvas's whole height.  So a
column block that is zero in one band was zero in all of them, every recurrence state that entered an all-zero tile was +0, the band
collapse's clamps were hardly reached, and no -0.0f, subnormal or negative sample ever crossed ranks.

CANVASES  (cw, ch, x0, mosaic width, bands, split levels): shapes tests/test_gpu_band.py already builds.
  0  (768, 384, 248, 520, 3, 2)   128-row bands, the main canvas
  1  (772, 384, 250, 520, 6, 1)   64-row bands: a rank's rows are ONE band of tiles, so "flagged in every band" is one flag
  2  (770, 384, 248, 520, 2, 2)   192-row bands; level 1 is 385 wide: the stand-alone anticausal sweep and decimation
  3  (768, 396, 248, 520, 3, 2)   132-row bands: the per-row flag look-up

PLACEMENTS  rows(name, ch) -> the canvas rows [f0, f1) of the frame and [m0, m1) of the mosaic.  The frame is cw - x0 wide and
f1 - f0 high, the mosaic m1 - m0 high at ox = 0, oy = -m0 (Oracle.move puts mosaic row r at canvas row r - oy).  The map is
[1, 0, 0, -x0, 0, 1, 0, -f0 + c]: c = 0 is the variant "aligned", which gives exactly the stated rows; c = 1.5 with
hard_inputs.NEAR's other coefficients is "tilted", which moves an edge of the frame by up to two rows.
  frame_mid    frame [ch/3, 2ch/3), mosaic full height
  mosaic_mid   frame full height, mosaic [ch/3, 2ch/3)
  both_mid     frame [ch/3, 2ch/3), mosaic [ch/3 - 28, 2ch/3 + 34)
  top_bottom   frame [0, ch/2 + 38), mosaic [ch/2 - 38, ch)
  bottom_top   frame [ch/2 - 38, ch), mosaic [0, ch/2 + 38)
  frame_low    frame [ch/2, ch), mosaic full height
Both images of an accepted pair hold the canvas's middle row ch/2, the first row of the second of two bands: with two bands no band
can be empty BELOW data, and of the first five placements none leaves one empty at all.  frame_low is there for canvas 2: its band 0
holds no frame row, above data.
EMPTY states, per canvas and placement, the bands that hold no row of the frame and no row of the mosaic (aligned variant).
REFUSAL_PLACEMENTS: mosaic_above_mid (a full-height frame, the mosaic on the rows [0, ch/2 - 116): no overlap on the middle row, -3)
and hard_inputs.map_pair's fold (-2) and miss (-3) on these canvases.

FORMS  the six of tests/test_gpu_band.py::test_band_group_single_host_thread, and separate sweeps with the state in two column chunks.

THE CLASS RULE  Item (canvas c, placement q, form f) of a pixel type takes the FRAME class (c + q + f) mod len(classes_of(type)), the
MOSAIC the class three places further on; seeds 2 s + 1 (frame) and 2 s (mosaic) with s = 7 c + q.  A checkerboard takes the first
of the phases 0 .. 3 (bit 0: the mosaic's, bit 1: the frame's) that the oracle accepts: PHASE lists the items whose phase is not 0.
REFUSED lists the items no phase makes acceptable, with the oracle's answer; every other item's rc is 0.  Both are the result of
derive_tables() and are held to the oracle by the host test.
WHICH ITEMS RUN  items(): on canvas 0 every placement x every form, on the others every placement x the forms fused and separate;
both pixel types, both variants."""
import numpy as np

import hard_inputs as H

CANVASES = ((768, 384, 248, 520, 3, 2), (772, 384, 250, 520, 6, 1), (770, 384, 248, 520, 2, 2), (768, 396, 248, 520, 3, 2))
MAIN = 0
PLACEMENTS = ("frame_mid", "mosaic_mid", "both_mid", "top_bottom", "bottom_top", "frame_low")
RUN_ORDER = ("frame_mid", "top_bottom", "mosaic_mid", "bottom_top", "both_mid", "frame_low")  # consecutive ones differ in their empty bands
VARIANTS = ("aligned", "tilted")
REFUSAL_PLACEMENTS = {"mosaic_above_mid": -3, "fold": -2, "miss": -3}
# name -> the keywords of pipeline.LocalBandGroup (and BandStitcher); "stored": level 0 as seven stored planes (Band.set_level0(False))
FORMS = {"fused": dict(fuse_sweeps=True), "separate": dict(fuse_sweeps=False), "planes": dict(fuse_sweeps=False, plane_pipeline_min=0),
         "stored": dict(fuse_sweeps=False), "stored+fused": dict(fuse_sweeps=True), "chunks4": dict(fuse_sweeps=False, col_chunks=4),
         "chunks2": dict(fuse_sweeps=False, col_chunks=2)}
FORM_NAMES = tuple(FORMS)
DTYPES = (np.uint8, np.float32)


def stored(form):
    return form.startswith("stored")


def forms_of(c):
    return FORM_NAMES if c == MAIN else FORM_NAMES[:2]


def rows(placement, ch):
    """(f0, f1, m0, m1): the canvas rows of the frame and of the mosaic."""
    t, h = ch // 3, ch // 2
    return {"frame_mid": (t, 2 * t, 0, ch), "mosaic_mid": (0, ch, t, 2 * t), "both_mid": (t, 2 * t, t - 28, 2 * t + 34),
            "top_bottom": (0, h + 38, h - 38, ch), "bottom_top": (h - 38, ch, 0, h + 38), "frame_low": (h, ch, 0, ch),
            "mosaic_above_mid": (0, ch, 0, h - 116)}[placement]


def band_rows(c):
    """[r0, r1) of every rank's rows at level 0."""
    ch, n = CANVASES[c][1], CANVASES[c][4]
    return [(b * (ch // n), (b + 1) * (ch // n)) for b in range(n)]


def band_map(x0, f0, variant):
    if variant == "aligned":
        return [1.0, 0.0, 0.0, -float(x0), 0.0, 1.0, 0.0, -float(f0)]
    return [H.NEAR[0], H.NEAR[1], H.NEAR[2], -float(x0), H.NEAR[4], H.NEAR[5], H.NEAR[6], -float(f0) + H.NEAR[7]]


def placed(c, placement, variant, F, M):
    """The pair dict (hard_inputs.map_pair's keys) of a frame and a mosaic of the placement's sizes."""
    cw, ch, x0 = CANVASES[c][:3]
    f0, f1, m0, m1 = rows(placement, ch)
    assert F.shape == (3, f1 - f0, cw - x0) and M.shape == (3, m1 - m0, CANVASES[c][3])
    return dict(name=f"{c}-{placement}-{variant}", F=F, p=band_map(x0, f0, variant), offx=0.0, offy=0.0, M=M, ox=0, oy=-m0, cw=cw, ch=ch)


def synth_pair(c, placement, variant, dtype, seed=0):
    """The placement with Oracle.synth frames: never 0 inside, so what is non-zero on the canvases is the footprint."""
    cw, ch, x0, mw = CANVASES[c][:4]
    f0, f1, m0, m1 = rows(placement, ch)
    o = H.oracle()
    return placed(c, placement, variant, o.synth(cw - x0, f1 - f0, 2 * seed + 1, dtype), o.synth(mw, m1 - m0, 2 * seed, dtype))


def full_height_pair(c, dtype):
    """A synthetic full-height pair, the kind every older band test runs (tests/test_gpu_band.py's _inputs, on this canvas)."""
    cw, ch, x0, mw = CANVASES[c][:4]
    o = H.oracle()
    p = [H.NEAR[0], H.NEAR[1], H.NEAR[2], -float(x0), H.NEAR[4], H.NEAR[5], H.NEAR[6], H.NEAR[7]]
    return dict(name=f"{c}-synth", F=o.synth(cw - x0, ch, 5, dtype), p=p, offx=0.0, offy=0.0, M=o.synth(mw, ch, 4, dtype), ox=0, oy=0, cw=cw, ch=ch)


# ---- the table -------------------------------------------------------------------------------------------------------------------

def item_key(c, placement, form, dtype, variant):
    return (c, placement, form, np.dtype(dtype).name, variant)


def item_classes(c, placement, form, dtype):
    """(frame class, mosaic class)."""
    cl = H.classes_of(dtype)
    i = c + PLACEMENTS.index(placement) + FORM_NAMES.index(form)
    return cl[i % len(cl)], cl[(i + 3) % len(cl)]


def item_seed(c, placement):
    return 7 * c + PLACEMENTS.index(placement)


def item(c, placement, form, dtype, variant, phase=None):
    """The pair dict of an item, by the tables (phase: a trial of the search instead); with the classes as "frame" and "mosaic"."""
    cw, ch, x0, mw = CANVASES[c][:4]
    f0, f1, m0, m1 = rows(placement, ch)
    fc, mc = item_classes(c, placement, form, dtype)
    s = item_seed(c, placement)
    phase = PHASE.get(item_key(c, placement, form, dtype, variant), 0) if phase is None else phase
    r = placed(c, placement, variant, H.content(fc, cw - x0, f1 - f0, dtype, 2 * s + 1, phase >> 1), H.content(mc, mw, m1 - m0, dtype, 2 * s, phase & 1))
    r.update(frame=fc, mosaic=mc, key=item_key(c, placement, form, dtype, variant))
    return r


def stated_rc(c, placement, form, dtype, variant):
    return REFUSED.get(item_key(c, placement, form, dtype, variant), 0)


def items():
    """(c, placement, form, dtype, variant) of every item the GPU test runs."""
    for c in range(len(CANVASES)):
        for form in forms_of(c):
            for dtype in DTYPES:
                for placement in RUN_ORDER:
                    for variant in VARIANTS:
                        yield c, placement, form, dtype, variant


def refusal_pair(c, name, dtype):
    """One pair of REFUSAL_PLACEMENTS on a canvas: mosaic_above_mid with a `holes` frame over a `fullrange` mosaic."""
    if name != "mosaic_above_mid":
        r = H.map_pair(name, CANVASES[c][:4], dtype)
        r["name"] = f"{c}-{name}"
        return r
    cw, ch, x0, mw = CANVASES[c][:4]
    f0, f1, m0, m1 = rows(name, ch)
    return placed(c, name, "aligned", H.content("holes", cw - x0, f1 - f0, dtype, 91), H.content("fullrange", mw, m1 - m0, dtype, 90))


def seam_of(r):
    """(rc, seam) of the pair's seam scan, from the canvases' middle row alone."""
    return H.seam_rc(r["F"], r["p"], r["offx"], r["offy"], r["M"], r["ox"], r["oy"], r["cw"], r["ch"])


def derive_tables():
    """(PHASE, REFUSED) as this module states them: per item with a checkerboard the first of the phases 0 .. 3 that the oracle
    accepts; where none does -- or phase 0 is refused and there is no checkerboard -- the answer to phase 0."""
    phases, refused = {}, {}
    for c, placement, form, dtype, variant in items():
        first = seam_of(item(c, placement, form, dtype, variant, phase=0))[0]
        if first == 0:
            continue
        key = item_key(c, placement, form, dtype, variant)
        ok = [ph for ph in (1, 2, 3) if "checker" in item_classes(c, placement, form, dtype) and seam_of(item(c, placement, form, dtype, variant, phase=ph))[0] == 0]
        if ok:
            phases[key] = ok[0]
        else:
            refused[key] = first
    return phases, refused


def derive_refused():
    return derive_tables()[1]


def empty_bands(a, c):
    """The bands of canvas c in which the canvas-sized image a is zero in every sample (bit patterns: -0.0f is not zero)."""
    bits = a.view(np.uint8 if a.dtype == np.uint8 else np.uint32)
    return tuple(b for b, (r0, r1) in enumerate(band_rows(c)) if not bits[:, r0:r1].any())


def derive_empty():
    """EMPTY as this module states it, from the oracle's warp and move of the aligned synthetic pair."""
    o, out = H.oracle(), {}
    for c in range(len(CANVASES)):
        for placement in PLACEMENTS:
            r = synth_pair(c, placement, "aligned", np.uint8)
            a, b = o.warp(r["F"], r["p"], 0.0, 0.0, r["cw"], r["ch"]), o.move(r["M"], r["ox"], r["oy"], r["cw"], r["ch"])
            out[(c, placement)] = (empty_bands(a, c), empty_bands(b, c))
    return out


PHASE = {}    # the oracle accepts every item at phase 0; an entry here would be (key): 1, 2 or 3
REFUSED = {}  # an entry here would be (key): -2 or -3
# (canvas, placement) -> (bands without a frame row, bands without a mosaic row), aligned variant
EMPTY = {
    (0, "frame_mid"): ((0, 2), ()), (0, "mosaic_mid"): ((), (0, 2)), (0, "both_mid"): ((0, 2), ()),
    (0, "top_bottom"): ((2,), (0,)), (0, "bottom_top"): ((0,), (2,)), (0, "frame_low"): ((0,), ()),
    (1, "frame_mid"): ((0, 1, 4, 5), ()), (1, "mosaic_mid"): ((), (0, 1, 4, 5)), (1, "both_mid"): ((0, 1, 4, 5), (0, 5)),
    (1, "top_bottom"): ((4, 5), (0, 1)), (1, "bottom_top"): ((0, 1), (4, 5)), (1, "frame_low"): ((0, 1, 2), ()),
    (2, "frame_mid"): ((), ()), (2, "mosaic_mid"): ((), ()), (2, "both_mid"): ((), ()),
    (2, "top_bottom"): ((), ()), (2, "bottom_top"): ((), ()), (2, "frame_low"): ((0,), ()),
    (3, "frame_mid"): ((0, 2), ()), (3, "mosaic_mid"): ((), (0, 2)), (3, "both_mid"): ((0, 2), ()),
    (3, "top_bottom"): ((2,), (0,)), (3, "bottom_top"): ((0,), (2,)), (3, "frame_low"): ((0,), ()),
}

if __name__ == "__main__":
    import pprint
    ph, ref = derive_tables()
    print("PHASE = ", end="")
    pprint.pprint(ph, width=140)
    print("REFUSED = ", end="")
    pprint.pprint(ref, width=140)
    print("EMPTY = ", end="")
    pprint.pprint(derive_empty(), width=140)
