"""The second table of option combinations of the rig replay: the options that came after tests/rig_edges.py's table -- path seams,
anchors, the 4:2:2 layouts and NV21, temporal exposure and the output scale -- with the older ones, on the word-edge canvases of
tests/rig_edges.py.  TEST INFRASTRUCTURE ONLY, host only.  Shared by tests/test_rig_lattice2_host.py and
tests/test_gpu_rig_lattice2.py; the CPU statement of a row is tests/rig_chain_ref.py's.

A ROW is a dict factor -> value (options()); Ctx.chain_options() turns it into the options of tests/rig_chain_ref.py and Ctx.frames()
into its sets.  Rows that share creation_key() run on one handle.  The values:
  exposure  (mode, None | ("keep", k) | "fixed").  Fixed statistics are those the CPU statement of the same row measures on set 0
            with no temporal option, every mean (entries 0 .. 2 and 6 .. 8) moved by MEAN_SHIFT: valid records that no set measures.
  seams     content; given (rig_edges.given_seams); paths found (max_step 2, margin 1); found with an anchor (weight 32, cap 4) of
            policy "set" or "call"; paths fixed: those the CPU statement of the same row finds on set 0 without an anchor, each
            column moved one towards the overlap's centre column (the geometric record's sum_ov_x / n_ov).
  crop      0; 1: mode 1 with the inscribed rectangle; 2: mode 2 with rig_edges.odd_rect
  scale     None; "coprime": the smallest ow >= 3 w / 5 and oh >= 4 h / 7 coprime to w and h; "eighth": (ceil(w / 8), ceil(h / 8));
            (w, h) is what the crop leaves
  input     planar; YUYV tight and aligned; UYVY at padded pitches with the last set of every call one byte off; NV21 tight and
            aligned; NV16 at padded pitches.  Padded: the rule of tests/test_gpu_rig_scale.py's _padded.
  output    planar; YUYV padded, into buffers of 0xEE; UYVY tight; NV16 padded; NV21 tight
  finish, monitor (None or radius 2)
  calls     ((sets per call), max_sets): one call of 2 at 16; one call of 3 at 2; calls of 3 then 2 at 2 on one handle, a stream of 5
A formatted row's matrix is its table index modulo 3.
"""
import math

import numpy as np

import pixfmt_yuv_ref as pyr
import rig_chain_ref as rc
import rig_edges as re_
import rig_seams_ref as ref

FACTORS = ("exposure", "seams", "crop", "scale", "input", "output", "finish", "monitor", "calls")
VALUES = {
    "exposure": ((0, None), (1, None), (2, None), (1, ("keep", 192)), (2, ("keep", 64)), (1, "fixed"), (2, "fixed")),
    "seams": ("content", "given", "paths", "paths_set", "paths_call", "paths_fixed"),
    "crop": (0, 1, 2),
    "scale": (None, "coprime", "eighth"),
    "input": ("planar", "yuyv_tight", "uyvy_padded_off", "nv21_tight", "nv16_padded"),
    "output": ("planar", "yuyv_padded", "uyvy_tight", "nv16_padded", "nv21_tight"),
    "finish": (True, False),
    "monitor": (None, 2),
    "calls": (((2,), 16), ((3,), 2), ((3, 2), 2)),
}
LEVELS = tuple(len(VALUES[f]) for f in FACTORS)
STRENGTH = 2
RIG_NAMES = ("odd_h", "w64_65")
MAX_STEP, MARGIN = 2, 1
WEIGHT, CAP = 32, 4
MEAN_SHIFT = np.float32(0.03125)
IN_FMT = {"planar": (pyr.PLANAR, False), "yuyv_tight": (pyr.YUYV, False), "uyvy_padded_off": (pyr.UYVY, True), "nv21_tight": (pyr.NV21, False),
          "nv16_padded": (pyr.NV16, True),
          "yuyv_padded": (pyr.YUYV, True)}  # level -> (format, padded pitches); yuyv_padded is no level of the table: the odd_w rows' alone
OUT_FMT = {"planar": (pyr.PLANAR, False), "yuyv_padded": (pyr.YUYV, True), "uyvy_tight": (pyr.UYVY, False), "nv16_padded": (pyr.NV16, True),
           "nv21_tight": (pyr.NV21, False)}
NONE = dict(exposure=(0, None), seams="content", crop=0, scale=None, input="planar", output="planar", finish=True, monitor=None)  # every new option off

# odd_w: frames of ODD width -- the last 4:2:2 group of a row holds one pixel ((w + 1) / 2 chroma columns, a Y1 byte that is no pixel's)
# and no frame takes the fused projection.  The moves are w64_65's.
ODD_W = ((41, 33), [(1, (24.0, 1.25)), (2, (-1.0, -0.5))])


def rows():
    return re_.covering_rows(LEVELS, STRENGTH)


def options(row, index=0):
    """A row of rows() as a dict factor -> value, with its table index (the matrix of a formatted row is index % 3)."""
    return dict({f: VALUES[f][i] for f, i in zip(FACTORS, row)}, index=index)


def table():
    return [options(r, i) for i, r in enumerate(rows())]


def creation_key(opt):
    """What a handle is created with: (exposure mode, finish, calls)."""
    return (opt["exposure"][0], opt["finish"], opt["calls"])


def groups(tab=None):
    out = {}
    for opt in (table() if tab is None else tab):
        out.setdefault(creation_key(opt), []).append(opt)
    return out


def key_id(key):
    return f"mode{key[0]}-finish{int(key[1])}-" + "+".join(str(n) for n in key[2][0]) + f"of{key[2][1]}"


def padded(t):
    """A pitch above the tight one that is no multiple of 4 (tests/test_gpu_rig_scale.py)."""
    return 0 if not t else t + 5 if (t + 5) % 4 else t + 6


def pitches(fmt, w, pad):
    t = pyr.tight(fmt, w)
    return (padded(t[0]), padded(t[1])) if pad else t


def scale_of(level, w, h):
    if level is None:
        return None
    if level == "eighth":
        return (-(-w // 8), -(-h // 8))
    ow, oh = -(-3 * w // 5), -(-4 * h // 7)
    while math.gcd(ow, w) != 1:
        ow += 1
    while math.gcd(oh, h) != 1:
        oh += 1
    return (ow, oh)


def repitched(im, pitch, pitch2, fill=0xEE):
    """An image of any layout at other pitches: the same pixel bytes, every byte of padding = fill."""
    fmt, w, h = im["fmt"], im["w"], im["h"]
    t = pyr.tight(fmt, w)
    b1, b2 = pyr.image_bytes(fmt, w, h, pitch, pitch2 or None)
    data, data2 = np.full(b1, fill, np.uint8), (np.full(b2, fill, np.uint8) if b2 else None)
    for y in range(h):
        data[y * pitch:y * pitch + t[0]] = im["data"][y * im["pitch"]:y * im["pitch"] + t[0]]
    if b2:
        for y in range((b2 - t[1]) // pitch2 + 1):
            data2[y * pitch2:y * pitch2 + t[1]] = im["data2"][y * im["pitch2"]:y * im["pitch2"] + t[1]]
    return dict(fmt=fmt, w=w, h=h, data=data, data2=data2, pitch=pitch, pitch2=pitch2 if b2 else 0)


def same(a, b):
    """Two outputs of rig_chain_ref: planar arrays, or images compared whole."""
    if isinstance(a, dict) != isinstance(b, dict):
        return False
    if not isinstance(a, dict):
        return a.shape == b.shape and np.array_equal(a, b)
    return (a["fmt"], a["w"], a["h"], a["pitch"], a["pitch2"]) == (b["fmt"], b["w"], b["h"], b["pitch"], b["pitch2"]) and np.array_equal(a["data"], b["data"]) \
        and ((a["data2"] is None and b["data2"] is None) or np.array_equal(a["data2"], b["data2"]))


class Ctx:
    """What the rows of one rig share, on the CPU alone: steps, geometry, the synthetic sets, the rectangles, the given seams."""

    def __init__(self, capi, oracle, name):
        self.name, self.oracle = name, oracle
        if name == "odd_w":
            self.sizes = [ODD_W[0]] * 3
            moves = [(m[0],) + tuple(ref.shift(*m[1])) for m in ODD_W[1]]
            st = ref.hand_steps(capi, self.sizes, moves)
            self.steps = [dict(s, mosaic_src=(st[k - 1]["src"] if k else s["start"])) for k, s in enumerate(st)]
        else:
            self.sizes, self.steps = re_.sizes(name), re_.steps(capi, name)
        self.cw, self.ch = self.steps[-1]["cw"], self.steps[-1]["ch"]
        self.geo = rc.geometry(oracle, self.sizes, self.steps)
        self.inscribed = self.geo["inscribed"]
        self.odd = re_.odd_rect(self.cw, self.ch)
        self.given = re_.given_seams(self.geo["geometric"], self.steps)
        self._planar, self._derived = {}, {}

    # ---- the sets -------------------------------------------------------------------------------------------------------------------
    def planar(self, i):
        """Synthetic set i: Oracle.synth frames 3 i + f (capi.dev_synth's CPU twin)."""
        if i not in self._planar:
            self._planar[i] = [self.oracle.synth(w, h, 3 * i + f) for f, (w, h) in enumerate(self.sizes)]
        return self._planar[i]

    def frames(self, level, counts, matrix, first=0, dark=None, hole=None):
        """-> per call, per set, per frame (the reference image of the input level -- a (3, H, W) array for planar --, the offset of
        its planes in their device buffers).  counts: sets per call; set numbers run on from `first` through the calls.
        dark = (set, frame): that frame all zero.  hole = (set, frame): its six leftmost columns zero."""
        fmt, pad = IN_FMT[level]
        out, i = [], first
        for n in counts:
            sets = []
            for j in range(n):
                row = []
                for f, p in enumerate(self.planar(i)):
                    p = np.zeros_like(p) if dark == (i, f) else p
                    if hole == (i, f):
                        p = p.copy()
                        p[:, :, :6] = 0
                    if not fmt:
                        row.append((p, 0))
                    else:
                        pitch, pitch2 = pitches(fmt, p.shape[2], pad)
                        row.append((pyr.pack(p, fmt, matrix, pitch, pitch2 or None), 1 if level == "uyvy_padded_off" and j == n - 1 else 0))
                sets.append(row)
                i += 1
            out.append(sets)
        return out

    # ---- a row's options as tests/rig_chain_ref.py takes them ---------------------------------------------------------------------
    def crop_of(self, opt):
        return {0: None, 1: (self.inscribed, 1), 2: (self.odd, 2)}[opt["crop"]]

    def source_size(self, opt):
        crop = self.crop_of(opt)
        return (self.cw, self.ch) if crop is None else tuple(crop[0][2:])

    def out_size(self, opt):
        return scale_of(opt["scale"], *self.source_size(opt)) or self.source_size(opt)

    def matrix_of(self, opt):
        return opt["index"] % 3

    def formats_of(self, opt):
        return IN_FMT[opt["input"]][0], OUT_FMT[opt["output"]][0], self.matrix_of(opt)

    def out_pitches(self, opt):
        fmt, pad = OUT_FMT[opt["output"]]
        return pitches(fmt, self.out_size(opt)[0], pad)

    def base_options(self, opt):
        """The row without its temporal exposure, its anchor and its path source: what the derived levels are measured with."""
        in_fmt, out_fmt, matrix = self.formats_of(opt)
        return dict(mode=opt["exposure"][0], seams=("content",), crop=self.crop_of(opt), scale=scale_of(opt["scale"], *self.source_size(opt)), in_fmt=in_fmt,
                    out_fmt=out_fmt, matrix=matrix, out_pitch=self.out_pitches(opt) if out_fmt else None, finish=opt["finish"], monitor=opt["monitor"])

    def _set0(self, opt, chain):
        """The CPU statement of set 0 under `chain`, once per (what it depends on)."""
        key = (opt["input"], self.matrix_of(opt) if IN_FMT[opt["input"]][0] else 0, chain["mode"], repr(chain["seams"]), repr(chain.get("fixed")))
        if key not in self._derived:
            frames = [im for im, _ in self.frames(opt["input"], (1,), self.matrix_of(opt))[0][0]]
            plain = dict(chain, crop=None, scale=None, out_fmt=0, out_pitch=None, finish=False, monitor=None)
            self._derived[key] = rc.one_set(self.oracle, self.geo, self.steps, frames, plain, [None] * len(self.steps), [None] * len(self.steps))
        return self._derived[key]

    def fixed_stats(self, opt):
        """The `fixed` level of exposure: set 0's measured statistics under the row's mode and vertical seam source, every mean moved."""
        chain = self.base_options(opt)
        chain["seams"] = ("given", self.given) if opt["seams"] == "given" else ("content",)
        st = self._set0(opt, chain)["measured"].copy()
        st[:, [0, 1, 2, 6, 7, 8]] += MEAN_SHIFT
        return st

    def fixed_paths(self, opt, chain):
        """The `paths_fixed` level: set 0's unanchored paths under the row's exposure, each column one nearer the overlap's centre."""
        found = self._set0(opt, dict(chain, seams=("paths", MAX_STEP, MARGIN), anchor=None, keep=None))["paths"]
        out = []
        for path, g in zip(found, self.geo["geometric"]):
            centre = g[2] / g[3]
            out.append(np.where(path < centre, path + 1, path - 1).astype(np.int32))
        return out

    def chain_options(self, opt):
        chain = self.base_options(opt)
        temporal = opt["exposure"][1]
        if temporal == "fixed":
            chain["fixed"] = self.fixed_stats(opt)
        elif temporal is not None:
            chain["keep"] = temporal[1]
        s = opt["seams"]
        if s == "given":
            chain["seams"] = ("given", self.given)
        elif s == "paths_fixed":
            chain["seams"] = ("fixed_paths", self.fixed_paths(opt, chain))
        elif s.startswith("paths"):
            chain["seams"] = ("paths", MAX_STEP, MARGIN)
            if s != "paths":
                chain["anchor"] = (WEIGHT, CAP, s.split("_")[1])
        return chain

    def run(self, opt, chain=None, state=None, **frames_kw):
        """The CPU statement of a row's calls -> per call (results per set, the state after the call)."""
        host = self.frames(opt["input"], opt["calls"][0], self.matrix_of(opt), **frames_kw)
        calls = [[[im for im, _ in fs] for fs in sets] for sets in host]
        return rc.stream(self.oracle, self.geo, self.steps, calls, self.chain_options(opt) if chain is None else chain, state)
