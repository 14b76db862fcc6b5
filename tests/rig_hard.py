"""Hard frame content and raw camera bytes for the rig replay's tests: tests/hard_inputs.py's content classes, and a seventh of plain
random layout bytes, dealt over the rows of tests/rig_lattice2.py's option table.  TEST INFRASTRUCTURE ONLY, host only: numpy and the
oracle, no torch.  Shared by tests/test_rig_hard_host.py, which holds everything below to the CPU statement (tests/rig_chain_ref.py)
before any GPU run, and tests/test_gpu_rig_hard.py.

Why: every other rig test feeds the replay Oracle.synth frames or pack() of them -- samples between 1 and 250.99, never 0, in gamut,
X bytes 255, both pixels of a 4:2:2 group sharing an averaged chroma.  Zeros inside frames, saturated mosaics, path costs near their
ceiling and the decode's clips are never reached that way.

CONTENT CLASSES of a set of uint8 frames (CLASSES):
  checker, holes, fullrange, binary, band, white   tests/hard_inputs.py's; the checkerboard's phase is the frame index & 1
  raw        for a formatted input level every byte of the layout's planes -- padding, X bytes and the Y1 byte of an odd group
             included -- is uniformly random: no pack of anything, its reference planar frame is unpack(raw).  For the planar level
             raw is fullrange.
Frame f of set i takes seed 3 i + f (the synthetic generator's frame number).

THE CLASS RULE (class_of): set i of table row r on rig number q takes class (r + i + OFFSET q) mod 7, q = 0 for odd_h and 1 for w64_65.
The class changes inside every stream; smoothing state and anchors are carried across the change.  With one rig alone two (level,
class) pairs never meet; the offset of 3 on the second rig closes them (tests/test_rig_hard_host.py).  The derived levels
(fixed_stats, fixed_paths, given) stay derived as tests/rig_lattice2.py derives them, from set 0 of the row's OWN frames.

REFUSED: (rig, row, set) -> the code with which the CPU statement refuses that set; every other set of the table succeeds.

BYTE CLASSES of the stand-alone projection test (image_of): raw, and edges -- every byte drawn from EDGE_BYTES, the values around the
limits of the three matrices' ranges.

THE CONTRAST SET (contrast_frames): frames alternately white and binary by frame index; a white pixel beside a black one costs a path
the d term's ceiling, 2 x 1020 = 2040."""
import numpy as np

import hard_inputs as hi
import pixfmt_ref as pf
import pixfmt_yuv_ref as pyr
import rig_chain_ref as rc
import rig_lattice2 as l2
import seam_path_ref as sp

CLASSES = hi.U8_CLASSES + ("raw",)
SATURATING, HOLED = hi.SATURATING, ("holes", "band")
RIG_NUMBER = {"odd_h": 0, "w64_65": 1}
OFFSET = 3
EDGE_BYTES = np.array([0, 1, 15, 16, 17, 127, 128, 129, 234, 235, 236, 239, 240, 241, 254, 255], np.uint8)
YUV = (pyr.NV12,) + pyr.NEW
ALL_INPUTS = (pyr.RGB24, pyr.BGR24, pyr.RGBX32, pyr.BGRX32, pyr.NV12, pyr.YUYV, pyr.UYVY, pyr.NV21, pyr.NV16)

# (rig, table row, set of the row's stream) -> the CPU statement's status.  Content seams alone refuse a set for its pixels:
# a checkerboard whose two canvases never overlap on the middle row (-3), a middle row left empty once fixed statistics have
# recoloured the frame (-2).  Derived by derive_refused(); tests/test_rig_hard_host.py holds the table to it.
REFUSED = {
    ("odd_h", 0, 0): -3,
    ("odd_h", 35, 0): -3,
    ("w64_65", 16, 0): -2,
    ("w64_65", 16, 2): -2,
}


def class_of(name, row, i):
    return CLASSES[(row + i + OFFSET * RIG_NUMBER[name]) % len(CLASSES)]


def content(cls, w, h, seed, f):
    """One planar frame of a class; raw is fullrange here."""
    return hi.content("fullrange" if cls == "raw" else cls, w, h, np.uint8, seed, f & 1)


def image_of(cls, fmt, w, h, seed, pitch=None, pitch2=None):
    """An image of byte class raw or edges: every byte of both planes, padding included, random."""
    rng = np.random.default_rng(seed)
    b1, b2 = pyr.image_bytes(fmt, w, h, pitch, pitch2)
    t = pyr.tight(fmt, w)

    def plane(n):
        return rng.integers(0, 256, n, dtype=np.uint8) if cls == "raw" else EDGE_BYTES[rng.integers(0, len(EDGE_BYTES), n)]

    return dict(fmt=fmt, w=w, h=h, data=plane(b1), data2=plane(b2) if b2 else None, pitch=t[0] if pitch is None else pitch,
                pitch2=(t[1] if pitch2 is None else pitch2) if b2 else 0)


def decode_clipped(im, matrix):
    """The share of the pixels of a Y Cb Cr image that have a channel the decode clips (below 0 or above 255 before the clip)."""
    assert im["fmt"] in YUV
    yoff, ky, krv, kgu, kgv, kbu = pf.DECODE[matrix]
    Y, Cb, Cr = components(im)
    c, d, e = Y - yoff, Cb - 128, Cr - 128
    r, g, b = (ky * c + krv * e + 32768) >> 16, (ky * c - kgu * d - kgv * e + 32768) >> 16, (ky * c + kbu * d + 32768) >> 16
    return float(((r < 0) | (r > 255) | (g < 0) | (g > 255) | (b < 0) | (b > 255)).mean())


def components(im):
    """Per pixel Y, Cb, Cr of a Y Cb Cr image as int64 (h, w) arrays, by the layouts' rules (tests/pixfmt_yuv_ref.py)."""
    fmt, w, h = im["fmt"], im["w"], im["h"]
    wp, xx = (w + 1) // 2, np.arange(w)[None, :] // 2
    if fmt in pyr.ONE_PLANE_422:
        y0, cb, y1, cr = pyr.GROUP[fmt]
        g = pf._rows(im["data"], h, im["pitch"], 4 * wp).reshape(h, wp, 4)
        Y = np.stack([g[:, :, y0], g[:, :, y1]], axis=2).reshape(h, 2 * wp)[:, :w]
        yy = np.arange(h)[:, None]
        return Y.astype(np.int64), g[yy, xx, cb].astype(np.int64), g[yy, xx, cr].astype(np.int64)
    Y = pf._rows(im["data"], h, im["pitch"], w)
    hp = h if fmt == pyr.NV16 else (h + 1) // 2
    uv = pf._rows(im["data2"], hp, im["pitch2"], 2 * wp).reshape(hp, wp, 2)
    yy = np.arange(h)[:, None] // (1 if fmt == pyr.NV16 else 2)
    cb, cr = (1, 0) if fmt == pyr.NV21 else (0, 1)
    return Y.astype(np.int64), uv[yy, xx, cb].astype(np.int64), uv[yy, xx, cr].astype(np.int64)


def d_term(ctx, frames, in_fmt=0, matrix=0, k=0):
    """The d term d[s - 1] + d[s] of step k's path cost with no exposure mode, (ch, cw + 1): the cost without its wrong-pixel
    multiples (the d term stays below seam_path_ref.WRONG).  Step 0 alone: its mosaic is the projected start frame."""
    assert k == 0
    a, b = step0_canvases(ctx, frames, in_fmt, matrix)
    cov = ctx.geo["cov"][0]
    return sp.cost(a, b, cov["A"], cov["B"], ctx.geo["branches"][0], l2.MARGIN) % sp.WRONG


def _planar_of(frame, in_fmt, matrix):
    return pyr.unpack(frame, matrix) if in_fmt else np.ascontiguousarray(frame)


def step0_canvases(ctx, frames, in_fmt=0, matrix=0):
    st = ctx.steps[0]
    a = ctx.oracle.warp(ctx.oracle.project(_planar_of(frames[st["src"]], in_fmt, matrix)), st["p"], st["offx"], st["offy"], st["cw"], st["ch"])
    b = ctx.oracle.move(ctx.oracle.project(_planar_of(frames[st["start"]], in_fmt, matrix)), st["ox"], st["oy"], st["cw"], st["ch"])
    return a, b


def warped(ctx, frames, k, in_fmt=0, matrix=0):
    """Step k's frame, projected and warped onto the step's canvas (no exposure mode; the transfer keeps black pixels black)."""
    st = ctx.steps[k]
    return ctx.oracle.warp(ctx.oracle.project(_planar_of(frames[st["src"]], in_fmt, matrix)), st["p"], st["offx"], st["offy"], st["cw"], st["ch"])


class Ctx(l2.Ctx):
    """tests/rig_lattice2.py's context with the sets of THE CLASS RULE: frames() and planar() take the table row as `row`, and the
    derived levels are measured on set 0 of that row's own frames."""

    def __init__(self, capi, oracle, name):
        assert name in RIG_NUMBER
        super().__init__(capi, oracle, name)

    def planar(self, i, row=0):
        cls = class_of(self.name, row, i)
        cls = "fullrange" if cls == "raw" else cls
        if (cls, i) not in self._planar:
            self._planar[(cls, i)] = [content(cls, w, h, 3 * i + f, f) for f, (w, h) in enumerate(self.sizes)]
        return self._planar[(cls, i)]

    def frames(self, level, counts, matrix, first=0, row=0):
        """-> per call, per set, per frame (the reference image of the input level, the offset of its planes in their buffers), as
        rig_lattice2.Ctx.frames; set i takes class_of(rig, row, i)."""
        fmt, pad = l2.IN_FMT[level]
        out, i = [], first
        for n in counts:
            sets = []
            for j in range(n):
                off = 1 if level == "uyvy_padded_off" and j == n - 1 else 0
                if fmt and class_of(self.name, row, i) == "raw":
                    fs = [(image_of("raw", fmt, w, h, 3 * i + f, *[p or None for p in l2.pitches(fmt, w, pad)]), off) for f, (w, h) in enumerate(self.sizes)]
                elif fmt:
                    fs = [(pyr.pack(p, fmt, matrix, *[v or None for v in l2.pitches(fmt, p.shape[2], pad)]), off) for p in self.planar(i, row)]
                else:
                    fs = [(p, 0) for p in self.planar(i, row)]
                sets.append(fs)
                i += 1
            out.append(sets)
        return out

    def host(self, opt):
        return self.frames(opt["input"], opt["calls"][0], self.matrix_of(opt), row=opt["index"])

    def _set0(self, opt, chain):
        key = (opt["index"], chain["mode"], repr(chain["seams"]), repr(chain.get("fixed")))
        if key not in self._derived:
            frames = [im for im, _ in self.frames(opt["input"], (1,), self.matrix_of(opt), row=opt["index"])[0][0]]
            plain = dict(chain, crop=None, scale=None, out_fmt=0, out_pitch=None, finish=False, monitor=None)
            self._derived[key] = rc.one_set(self.oracle, self.geo, self.steps, frames, plain, [None] * len(self.steps), [None] * len(self.steps))
        return self._derived[key]

    def run(self, opt, chain=None, state=None):
        calls = [[[im for im, _ in fs] for fs in sets] for sets in self.host(opt)]
        return rc.stream(self.oracle, self.geo, self.steps, calls, self.chain_options(opt) if chain is None else chain, state)


def derive_refused(contexts):
    """REFUSED as the CPU statement gives it: contexts = name -> Ctx."""
    out = {}
    for name, ctx in contexts.items():
        for opt in l2.table():
            i = 0
            for results, _ in ctx.run(opt):
                for r in results:
                    if r["status"]:
                        out[(name, opt["index"], i)] = r["status"]
                    i += 1
    return out


# ---- the contrast set -------------------------------------------------------------------------------------------------------------------
CONTRAST_CALLS = (3, 2)


def contrast_frames(sizes, counts=CONTRAST_CALLS):
    """Per call, per set, per frame a planar frame: white at even frame indices, binary (seed 3 i + f) at odd ones."""
    out, i = [], 0
    for n in counts:
        sets = []
        for _ in range(n):
            sets.append([content("white" if f % 2 == 0 else "binary", w, h, 3 * i + f, f) for f, (w, h) in enumerate(sizes)])
            i += 1
        out.append(sets)
    return out


def contrast_row(mode):
    """The contrast set's row, as rig_lattice2.Ctx.chain_options takes it: found paths with an anchor per set (max_step 2, margin 1,
    weight 32, cap 4) and a monitor of radius 2; mode 2 smoothed with keep 64; 3 + 2 sets on a handle of two sets per sequence."""
    return dict(l2.NONE, exposure=(mode, ("keep", 64) if mode else None), seams="paths_set", monitor=2, calls=(CONTRAST_CALLS, 2), index=0)
