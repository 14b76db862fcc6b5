"""Hard pixel content and maps far from the identity, for the pair path's tests.  A plain module like form_cover.py: numpy and the
oracle only, no torch, no GPU.  tests/test_hard_inputs_host.py holds everything below to the oracle on the CPU before any GPU run;
tests/test_gpu_hard_content.py runs the content classes through every default launch form (form_cover_refs.ALL_CASES),
tests/test_gpu_hard_maps.py the map classes through every consumer of the map.

Why: the synthetic generator (Oracle.synth) gives samples between 1 and 250.99 and never 0, so the seam scan's content predicates
reduce to "inside the frame" and the collapse's clamps and truncating store are hardly reached; and nearly every map of the older
tests lies within a few per cent of the identity.

CONTENT CLASSES  (w, h, dtype, seed) -> (3, h, w), see content():
  checker    one-pixel 0/255 checkerboard, channels 0 and 2 in phase, channel 1 in antiphase; `phase` shifts it by one column
  binary     independent random 0/255 per sample and channel
  white      all 255
  fullrange  uniform 0 .. 255
  holes      a synthetic frame with 30 % of channel 0 set to 0 and 10 % of whole pixels set to 0
  band       a synthetic frame with an interior black band of columns (512 wide from 1024 columns on, 896 from 1408 on, else a third of the width)
  (float32: the value casts of those six, and)
  signed     uniform in [-300, 600) with fractional parts
  tiny       holes whose channel-0 holes hold subnormals of both signs (+-1e-40f: non-zero for the seam scan and for every bit-pattern
             zero test) and whose whole-pixel holes hold -0.0f (zero for the scan, not a +0 bit pattern)
No NaN or infinity; magnitudes stay below 2^20.

MAP CLASSES  map_case(name, cw, ch, x0, k) -> (fw, fh, p, offx, offy): the frame is meant to cover the canvas columns [x0, x0 + k) over
the canvas's whole height (the placement), see MAP_CLASSES; REFUSAL_CLASSES are the two the oracle refuses.

THE HARD-CONTENT TABLE  pair_inputs / dense_inputs (index, dtype, j): which class, placement, seed and phase every slot of the hard
calls of a case of form_cover_refs.ALL_CASES takes.  Item j of case i takes class (i + j) mod len(classes) of its pixel type; a case
runs ceil(3 / n) hard calls of n items, so that every case -- and with it every signature of form_cover -- sees three consecutive
classes, and the class orders below put one of checker / binary / white and one of holes / band / tiny into any three consecutive
ones.  PHASE lists the checkerboard items that take another phase than 0 (bit 0: the mosaic's, bit 1: the frame's; with phase 0 the
scan's mid row is empty or has no overlap), RESEED the items that take another seed (the same, on one- and two-column frames and
narrow overlaps), REFUSED the items the oracle refuses whatever the phase or seed, with its answer.  Every other item's rc is 0.
The three tables are the result of search_tables() and are held to the oracle by the host test."""
import numpy as np

import form_cover as FC
from form_cover_refs import ALL_CASES, case_id

U8_CLASSES = ("checker", "holes", "fullrange", "binary", "band", "white")
F32_CLASSES = ("checker", "holes", "fullrange", "binary", "band", "signed", "white", "tiny")
SATURATING = ("checker", "binary", "white")  # at least 1 % of output samples clamp to 255
HOLED = ("holes", "band", "tiny")            # real zeros inside the frame
PLACEMENTS = ("frame_right", "mosaic_left", "frame_left", "mosaic_right")  # form_cover.inputs(cw), both batches of g_flags_ref

_ORACLE = None


def oracle():
    global _ORACLE
    if _ORACLE is None:
        from oracle_lib import Oracle
        _ORACLE = Oracle()
    return _ORACLE


def classes_of(dtype):
    return U8_CLASSES if np.dtype(dtype) == np.uint8 else F32_CLASSES


# ---- content -------------------------------------------------------------------------------------------------------------------

def checker(w, h, dtype, seed=0, phase=0):
    on = ((np.arange(w)[None, :] + np.arange(h)[:, None] + phase) & 1) == 0
    return (np.stack([on, ~on, on]) * 255).astype(dtype)


def binary(w, h, dtype, seed=0):
    return (np.random.default_rng(seed).integers(0, 2, (3, h, w)) * 255).astype(dtype)


def white(w, h, dtype, seed=0):
    return np.full((3, h, w), 255, dtype)


def fullrange(w, h, dtype, seed=0):
    return np.random.default_rng(seed).integers(0, 256, (3, h, w)).astype(dtype)


def hole_masks(w, h, seed):
    """(30 % of channel 0, 10 % of whole pixels), drawn before anything else from the seed's stream."""
    rng = np.random.default_rng(seed)
    return rng.random((h, w)) < 0.3, rng.random((h, w)) < 0.1


def holes(w, h, dtype, seed=0):
    img = oracle().synth(w, h, seed, dtype)
    c0, px = hole_masks(w, h, seed)
    img[0][c0] = 0
    img[:, px] = 0
    return img


def band_columns(w):
    """[x0, x1) of the black band of a frame w wide: data on both sides, and some of it in the frame's middle third (two dense
    canvases, each black over an outer third, still overlap).  512 columns from a width of 1024 on, else a third of the width; 896
    from 1408 on: the blur's tails reach 153 columns into the band from either side before they are +0, and a flagged tile column of
    G_1 needs three of them -- 384 columns of level 0, wherever the 128-column grid falls -- to be +0."""
    if w >= 1408:
        return w - 960, w - 64
    if w >= 1024:
        return w - 576, w - 64
    return w // 2, w // 2 + w // 3


def band(w, h, dtype, seed=0):
    img = oracle().synth(w, h, seed, dtype)
    x0, x1 = band_columns(w)
    img[:, :, x0:x1] = 0
    return img


def signed(w, h, dtype, seed=0):
    assert np.dtype(dtype) == np.float32
    return np.random.default_rng(seed).uniform(-300.0, 600.0, (3, h, w)).astype(np.float32)


def tiny(w, h, dtype, seed=0):
    assert np.dtype(dtype) == np.float32
    img = oracle().synth(w, h, seed, np.float32)
    c0, px = hole_masks(w, h, seed)
    sign = np.where(((np.arange(w)[None, :] + np.arange(h)[:, None]) & 1) == 0, 1.0, -1.0)
    sub = (sign * 1e-40).astype(np.float32)
    assert np.all(sub != 0) and np.all(np.abs(sub) < np.finfo(np.float32).tiny)  # subnormal, and not flushed by numpy
    img[0][c0] = sub[c0]
    img[:, px] = np.float32(-0.0)
    return img


CONTENT = dict(checker=checker, binary=binary, white=white, fullrange=fullrange, holes=holes, band=band, signed=signed, tiny=tiny)


def content(name, w, h, dtype, seed=0, phase=0):
    """One image of a class; `phase` matters to the checkerboard alone."""
    return checker(w, h, dtype, seed, phase) if name == "checker" else CONTENT[name](w, h, dtype, seed)


# ---- maps ----------------------------------------------------------------------------------------------------------------------

NEAR = (1.0, 0.002, 1e-6, 0.0, -0.001, 1.0, 5e-7, 1.5)
MAP_CLASSES = ("near", "mirror_x", "mirror_y", "rot180", "transpose", "minify2", "magnify2", "shear", "twist", "stretch256", "constant", "trunc",
               "offsets")
REFUSAL_CLASSES = {"fold": -2, "miss": -3}
OFFSETS_OY, OFFSETS_SHORTER = 5, 71  # the mosaic's oy and the rows the frame lacks, in the class `offsets`


def map_case(name, cw, ch, x0, k):
    """(fw, fh, p, offx, offy) of a map class whose frame covers the canvas columns [x0, x0 + k) -- X = p0 x + p1 y + p2 x y + p3,
    Y = p4 x + p5 y + p6 x y + p7, truncated toward zero, as the reference warps with whatever bilinear map four matches fit."""
    x0, k = float(x0), int(k)
    if name == "near":
        return k, ch, [NEAR[0], NEAR[1], NEAR[2], -x0, NEAR[4], NEAR[5], NEAR[6], NEAR[7]], 0.0, 0.0
    if name == "mirror_x":
        return k, ch, [-1.0, 0.0, 0.0, x0 + k - 1, 0.0, 1.0, 0.0, 0.0], 0.0, 0.0
    if name == "mirror_y":
        return k, ch, [1.0, 0.0, 0.0, -x0, 0.0, -1.0, 0.0, float(ch - 1)], 0.0, 0.0
    if name == "rot180":
        return k, ch, [-1.0, 0.0, 0.0, x0 + k - 1, 0.0, -1.0, 0.0, float(ch - 1)], 0.0, 0.0
    if name == "transpose":  # X = y, Y = x - x0: a frame of transposed size
        return ch, k, [0.0, 1.0, 0.0, 0.0, 1.0, 0.0, 0.0, -x0], 0.0, 0.0
    if name == "minify2":
        return 2 * k, 2 * ch, [2.0, 0.0, 0.0, -2 * x0, 0.0, 2.0, 0.0, 0.0], 0.0, 0.0
    if name == "magnify2":
        return (k + 1) // 2, (ch + 1) // 2, [0.5, 0.0, 0.0, -0.5 * x0, 0.0, 0.5, 0.0, 0.0], 0.0, 0.0
    if name == "shear":  # X = (x - x0) + (y - ch / 2) / 2: the mid row reads the frame's own columns
        return k, ch, [1.0, 0.5, 0.0, -x0 - 0.25 * ch, 0.0, 1.0, 0.0, 0.0], 0.0, 0.0
    if name == "twist":  # X = s(y) (x - x0), s from 0.5 at the top row to 1.5 at the bottom
        p2 = 1.0 / (ch - 1)
        return (3 * k + 1) // 2, ch, [0.5, -p2 * x0, p2, -0.5 * x0, 0.0, 1.0, 0.0, 0.0], 0.0, 0.0
    if name == "stretch256":
        s = 1.0 + 1.0 / 256
        return k + k // 256 + 1, ch, [s, 0.0, 0.0, -s * x0, 0.0, 1.0, 0.0, 0.0], 0.0, 0.0
    if name == "constant":  # every canvas pixel reads the frame's centre pixel
        return k, ch, [0.0, 0.0, 0.0, float(k // 2), 0.0, 0.0, 0.0, float(ch // 2)], 0.0, 0.0
    if name == "trunc":  # X in (-1, 0) truncates to column 0: column and row 0 are read twice
        return k, ch, [1.0, 0.0, 0.0, -x0 - 0.5, 0.0, 1.0, 0.0, -0.5], 0.0, 0.0
    if name == "offsets":
        fw, fh, p, _, _ = map_case("near", cw, ch, x0, k)
        return fw, ch - OFFSETS_SHORTER, p, -3.25, 1.5
    if name == "fold":  # the x scale 1 + p2 y vanishes on the middle row: X = -x0 < 0 there, an empty mid row
        assert x0 >= 1
        return k, ch, [1.0, 0.0, -1.0 / (ch // 2), -x0, 0.0, 1.0, 0.0, 0.0], 0.0, 0.0
    raise KeyError(name)


def mosaic_oy(name):
    return OFFSETS_OY if name == "offsets" else 0


def seam_rc(F, p, offx, offy, M, ox, oy, cw, ch, seam_rule=0):
    """(rc, seam) of the pair's seam scan, from the canvases' middle row alone: a one-row warp and move at y = ch / 2 (the row
    offset enters as the float the full warp adds to it, and is exact)."""
    o, mid = oracle(), ch // 2
    return o.seam(o.warp(F, p, offx, float(mid) + offy, cw, 1), o.move(M, ox, mid + oy, cw, 1), seam_rule)


# cw, ch, the frame's left edge x0 (it covers the columns from x0 on), the mosaic's width (at ox = 0).  x0 = 3 mod 4: stretch256 skips a
# source column in front of canvas column x0 + 256 m, the LAST of an aligned group of four -- one patch per row, 64 per tile (at a
# group's edge the skip costs no patch, earlier in the group two or three per row: a general tile)
PAIR_CANVAS = (832, 448, 403, 600)
RUN_CANVASES = ((1088, 128, 303, 700), (1024, 192, 303, 600))  # tests/test_gpu_src_runs.py's two canvases, the same four numbers
RUN_MAPS = ("stretch256", "mirror_x", "magnify2", "trunc", "offsets")
BAND_CANVAS = (768, 384, 248, 520)
BAND_MAPS = ("mirror_y", "transpose", "twist", "offsets")
RESIDUAL_CANVAS = (130, 71, 30, 110)
RESIDUAL_MAPS = ("mirror_x", "rot180", "transpose", "constant", "trunc")
# Items the oracle refuses in tests/test_gpu_hard_maps.py's batches, (batch, map class, pixel type) -> rc; every other item's rc is 0.
# "mix": binary frames over holes mosaics -- the one frame sample the constant map reads is 0 in channel 0.  The short frame of
# `offsets` (128 - 71 = 57 rows) ends above the middle row of the 128-row canvas.
MAP_REFUSED = {("mix", "constant", "uint8"): -2, ("mix", "constant", "float32"): -2, ("runs-1088x128", "offsets", "float32"): -2}


def map_pair(name, canvas, dtype, frame="synth", mosaic="synth", seed=0):
    """One pair of a map class on a canvas (cw, ch, x0, mosaic width): dict(F, p, offx, offy, M, ox, oy, cw, ch).  frame / mosaic:
    a content class, or "synth" for Oracle.synth.  The class `miss` is the identity shift with a checkerboard frame over a
    checkerboard mosaic of the opposite phase on the canvas: no overlap whatever the rest says."""
    cw, ch, x0, mw = canvas
    fw, fh, p, offx, offy = map_case("near" if name == "miss" else name, cw, ch, x0, cw - x0)
    if name == "miss":
        p = [1.0, 0.0, 0.0, -float(x0), 0.0, 1.0, 0.0, 0.0]
        F, M = checker(fw, fh, dtype), checker(mw, ch, dtype, phase=(x0 + 1) & 1)
    else:
        make = lambda cls, w, h, s: oracle().synth(w, h, s, dtype) if cls == "synth" else content(cls, w, h, dtype, s)
        F, M = make(frame, fw, fh, 2 * seed + 1), make(mosaic, mw, ch, 2 * seed)
    return dict(name=name, F=F, p=p, offx=offx, offy=offy, M=M, ox=0, oy=mosaic_oy(name), cw=cw, ch=ch)


def pair_oracle(r, opts=None):
    """(rc, output, seam) of a map_pair by the oracle."""
    from oracle_lib import ROOT_OPTS
    opts = opts or ROOT_OPTS
    rc, out = oracle().pair(r["F"], r["p"], r["offx"], r["offy"], r["M"], r["ox"], r["oy"], r["cw"], r["ch"], opts)
    _, seam = seam_rc(r["F"], r["p"], r["offx"], r["offy"], r["M"], r["ox"], r["oy"], r["cw"], r["ch"], opts["seam_rule"])
    return rc, out, seam


# the rig's steps are stated by forward maps (frame -> mosaic; the canvas follows from them): (forward, backward) per class
def rig_mirror_x(c, ty):
    return [-1.0, 0.0, 0.0, float(c), 0.0, 1.0, 0.0, float(ty)], [-1.0, 0.0, 0.0, float(c), 0.0, 1.0, 0.0, -float(ty)]


def rig_transpose(tx, ty):
    return [0.0, 1.0, 0.0, float(tx), 1.0, 0.0, 0.0, float(ty)], [0.0, 1.0, 0.0, -float(ty), 1.0, 0.0, 0.0, -float(tx)]


def rig_magnify2(tx, ty):
    return [2.0, 0.0, 0.0, float(tx), 0.0, 2.0, 0.0, float(ty)], [0.5, 0.0, 0.0, -0.5 * tx, 0.0, 0.5, 0.0, -0.5 * ty]


def rig_cases(capi):
    """name -> (frame sizes, step dicts): a one-step rig whose map mirrors, and a two-step rig that transposes, then magnifies."""
    from rig_seams_ref import hand_steps
    one = [(64, 80), (64, 80)]
    two = [(64, 80), (80, 64), (40, 42)]
    return {"mirror_x": (one, hand_steps(capi, one, [(1,) + rig_mirror_x(95.25, 1.5)])),
            "transpose+magnify2": (two, hand_steps(capi, two, [(1,) + rig_transpose(31.0, -0.5), (2,) + rig_magnify2(40.5, -3.0)]))}


# ---- the hard-content table ----------------------------------------------------------------------------------------------------

def hard_calls(n):
    """The item numbers of every hard call of a case of n pairs: ceil(3 / n) calls, consecutive items."""
    return [list(range(c * n, (c + 1) * n)) for c in range(-(-3 // n))]


def item_key(index, dtype, j):
    return (case_id(ALL_CASES[index]), np.dtype(dtype).name, j)


def item_class(index, dtype, j):
    cl = classes_of(dtype)
    return cl[(index + j) % len(cl)]


def base_seed(index, j):
    return 40 + 5 * (index % 7) + j


def pair_inputs(index, dtype, j, phase=None, reseed=None):
    """(class, placement, F, P, M, ox) of item j of a pair case, by the tables (phase / reseed: a trial of the search instead)."""
    cw, ch = ALL_CASES[index][:2]
    name, where = item_class(index, dtype, j), PLACEMENTS[j % 4]
    key = item_key(index, dtype, j)
    phase = PHASE.get(key, 0) if phase is None else phase
    seed = base_seed(index, j) + 1000 * (RESEED.get(key, 0) if reseed is None else reseed)
    fw, P, mw, ox, _ = FC.inputs(cw)[where]
    return name, where, content(name, fw, ch, dtype, 2 * seed + 1, phase >> 1), P, content(name, mw, ch, dtype, 2 * seed, phase & 1), ox


def dense_inputs(index, dtype, j, reseed=None):
    """(class, A, B) of item j of a dense case: both canvases of the class, a third of each black on opposite sides as
    form_cover_refs.two_canvases has them (the sides swap with j)."""
    cw, ch = ALL_CASES[index][:2]
    name = item_class(index, dtype, j)
    seed = base_seed(index, j) + 1000 * (RESEED.get(item_key(index, dtype, j), 0) if reseed is None else reseed)
    A, B = content(name, cw, ch, dtype, 2 * seed + 1), content(name, cw, ch, dtype, 2 * seed)
    if j % 2 == 0:
        A[:, :, (2 * cw) // 3:] = 0
        B[:, :, : cw // 3] = 0
    else:
        A[:, :, : cw // 3] = 0
        B[:, :, (2 * cw) // 3:] = 0
    return name, A, B


def item_rc(index, dtype, j, **trial):
    """The oracle's answer to item j of a case, from the seam scan alone (every case of the table has a valid pyramid)."""
    cw, ch, _, _, dense = ALL_CASES[index][:5]
    if dense:
        _, A, B = dense_inputs(index, dtype, j, **trial)
        return oracle().seam(A, B)[0]
    _, _, F, P, M, ox = pair_inputs(index, dtype, j, **trial)
    return seam_rc(F, P, 0.0, 0.0, M, ox, 0, cw, ch)[0]


def stated_rc(index, dtype, j):
    return REFUSED.get(item_key(index, dtype, j), 0)


def search_tables(tries=8):
    """(PHASE, RESEED, REFUSED) as this module states them: per item the first of the phases 0 .. 3 (checkerboard), else of `tries`
    seeds, that the oracle accepts; where none does, the answer to the first."""
    phases, reseed, refused = {}, {}, {}
    for index, case in enumerate(ALL_CASES):
        n, dense = case[3], case[4]
        for dtype in (np.uint8, np.float32):
            for j in range(len(hard_calls(n)) * n):
                key, name = item_key(index, dtype, j), item_class(index, dtype, j)
                first = item_rc(index, dtype, j, reseed=0) if dense else item_rc(index, dtype, j, phase=0, reseed=0)
                if first == 0:
                    continue
                ok = [ph for ph in (1, 2, 3) if name == "checker" and not dense and item_rc(index, dtype, j, phase=ph, reseed=0) == 0]
                if ok:
                    phases[key] = ok[0]
                    continue
                ok = [t for t in range(1, tries) if name not in ("checker", "white") and item_rc(index, dtype, j, reseed=t) == 0]
                if ok:
                    reseed[key] = ok[0]
                else:
                    refused[key] = first
    return phases, reseed, refused


PHASE = {
    ('deriche-300x128-cap1-n1-pairs', 'uint8', 0): 1,
    ('deriche-5x3-cap1-n1-pairs', 'float32', 0): 3,
    ('deriche-5x3-cap1-n1-pairs', 'uint8', 0): 3,
    ('skip-300x128-cap1-n1-pairs', 'uint8', 0): 1,
    ('skip-5x3-cap1-n1-pairs', 'float32', 1): 3,
    ('skip-5x3-cap1-n1-pairs', 'uint8', 1): 3,
    ('vv0-1025x1025-cap2-n2-pairs', 'uint8', 3): 1,
    ('vv0-2047x620-cap16-n16-pairs', 'uint8', 0): 1,
    ('vv0-2047x620-cap16-n16-pairs', 'uint8', 12): 1,
    ('vv0-2049x2048-cap16-n16-pairs', 'float32', 3): 1,
    ('vv0-2049x2048-cap16-n16-pairs', 'float32', 11): 1,
    ('vv0-2049x2048-cap16-n16-pairs', 'uint8', 7): 1,
    ('vv0-2049x2050-cap16-n16-pairs', 'uint8', 0): 1,
    ('vv0-2049x2050-cap16-n16-pairs', 'uint8', 12): 1,
    ('vv0-2049x2050-cap2-n2-pairs', 'float32', 3): 1,
    ('vv0-2049x2050-cap2-n2-pairs', 'uint8', 3): 1,
    ('vv0-3x3-cap1-n1-pairs', 'float32', 1): 3,
    ('vv0-3x3-cap1-n1-pairs', 'uint8', 1): 3,
    ('vv0-511x1000-cap16-n16-pairs', 'float32', 4): 1,
    ('vv0-511x1000-cap16-n16-pairs', 'float32', 12): 1,
    ('vv0-511x1000-cap16-n16-pairs', 'uint8', 0): 1,
    ('vv0-511x1000-cap16-n16-pairs', 'uint8', 12): 1,
    ('vv0-511x258-cap16-n16-pairs', 'uint8', 7): 1,
    ('vv0-517x1100-cap3-n3-pairs', 'float32', 0): 1,
    ('vv0-517x2046-cap16-n16-pairs', 'uint8', 7): 1,
    ('vv0-5x3-cap2-n2-pairs', 'uint8', 2): 3,
    ('vv1-2047x5-cap16-n16-pairs', 'uint8', 7): 1,
    ('vv1-2048x5-cap16-n16-pairs', 'uint8', 4): 1,
    ('vv1-2050x33-cap3-n3-pairs', 'uint8', 0): 1,
    ('vv1-2052x33-cap3-n3-pairs', 'float32', 0): 1,
    ('vv1-255x5-cap16-n16-pairs', 'uint8', 11): 1,
    ('vv1-258x5-cap1-n1-pairs', 'float32', 0): 1,
    ('vv1-258x5-cap1-n1-pairs', 'uint8', 0): 1,
    ('vv1-517x255-cap16-n16-pairs', 'uint8', 3): 1,
    ('vv1-517x255-cap16-n16-pairs', 'uint8', 15): 1,
    ('vv1-64x1025-cap3-n3-pairs', 'uint8', 1): 1,
    ('vv1-67x2100-cap3-n3-pairs', 'uint8', 0): 1,
}
RESEED = {
    ('deriche-5x3-cap1-n1-dense', 'float32', 2): 1,
    ('deriche-5x3-cap1-n1-dense', 'uint8', 2): 1,
    ('deriche-5x3-cap1-n1-pairs', 'float32', 1): 5,
    ('deriche-5x3-cap1-n1-pairs', 'uint8', 1): 5,
    ('skip-5x3-cap2-n2-pairs', 'float32', 0): 3,
    ('skip-5x3-cap2-n2-pairs', 'uint8', 0): 3,
    ('vv0-3x3-cap1-n1-pairs', 'float32', 0): 1,
    ('vv0-3x3-cap1-n1-pairs', 'float32', 2): 1,
    ('vv0-3x3-cap1-n1-pairs', 'uint8', 2): 1,
    ('vv0-3x3-cap2-n2-pairs', 'float32', 0): 4,
    ('vv0-3x3-cap2-n2-pairs', 'float32', 2): 1,
    ('vv0-3x3-cap2-n2-pairs', 'uint8', 0): 4,
    ('vv0-3x3-cap2-n2-pairs', 'uint8', 2): 1,
    ('vv0-514x2046-cap16-n16-pairs', 'float32', 1): 1,
    ('vv0-5x3-cap1-n1-dense', 'float32', 0): 2,
    ('vv0-5x3-cap1-n1-dense', 'uint8', 0): 2,
    ('vv0-5x3-cap1-n1-pairs', 'float32', 1): 1,
    ('vv0-5x3-cap1-n1-pairs', 'uint8', 1): 1,
    ('vv0-5x3-cap2-n2-pairs', 'float32', 3): 2,
    ('vv0-5x3-cap2-n2-pairs', 'uint8', 3): 2,
    ('vv1-33x1026-cap16-n16-pairs', 'uint8', 8): 2,
    ('vv1-33x2100-cap3-n3-pairs', 'float32', 1): 1,
    ('vv1-33x2100-cap3-n3-pairs', 'uint8', 1): 1,
    ('vv1-64x1025-cap3-n3-pairs', 'float32', 0): 1,
}
REFUSED = {}  # with the phases and seeds above the oracle accepts every item; an entry here would be (key): -2 or -3
