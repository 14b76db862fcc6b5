"""GPU: the rig replay on hard frame content and raw camera bytes (tests/rig_hard.py, held to the CPU statement by
tests/test_rig_hard_host.py).  Everything is exact: every comparison is bit equality, statistics by their bits, a NaN as a NaN.

1. THE TABLE ON HARD CONTENT.  The 48 rows of tests/rig_lattice2.py on odd_h and w64_65, in the creation groups and parts of
   tests/test_gpu_rig_lattice2.py and through that file's driver, with rig_hard.Ctx's frames: set i of row r takes class
   (r + i + 3 q) mod 7 of checker, holes, fullrange, binary, band, white and raw, so the class changes inside every stream and the
   smoothing state and the anchors are carried across the change.  Every call is held to tests/rig_chain_ref.py (outputs whole,
   statuses, last_rc, seam records, returned and used statistics, smoothing state, paths, costs, moved, residuals, whether an anchor is
   held) and, up to a call's first refused set, to pipeline.stitch_chain.  A set of rig_hard.REFUSED is exactly that refusal, the other
   sets of its call are still compared, and after the call the rig holds neither state nor anchor.  input_form is a matter of layout,
   pitch and address: the bare rig of the driver is asked with the lattice's synthetic frames of the same level.
   Behind the table, two streams on odd_h in which step 0 refuses a checkerboard set under smoothing -- the first set of two launch
   sequences, and the middle set of one: the sets behind it are still the CPU statement's (the refused set takes no part in a later
   step's filter), which the table's row 35 found not to hold.
2. THE FUSED PROJECTION ON CAMERA BYTES: the narrowest test of fmt_lds_4 (csrc/k_rig_formats.inc).  A zero-step rig without a finish
   pass writes the projection of its start frame.  Nine input layouts, three matrices for the Y Cb Cr ones, the byte classes raw and
   edges, 1 and 3 sets per call on a handle of two sets per sequence; each input once at tight pitches on an aligned base (FUSED) and
   once with the same bytes one byte off (CONVERTED): the two outputs equal each other and oracle.project(unpack(image, matrix)).
3. THE CONTRAST SET: white frames against binary ones, where a path weighs columns at the d term's ceiling (2040) against wrong
   pixels (4096) -- found paths anchored per set over a call of 3 and a call of 2, mode 0 and mode 2 smoothed, with a monitor."""
import numpy as np
import pytest

import pixfmt_yuv_ref as pyr
import rig_hard as rh
import rig_lattice2 as l2
import test_gpu_rig_lattice2 as lat
from computervisionimagestich2_amd import capi, pipeline
from test_gpu_pixfmt import to_dev

pytestmark = pytest.mark.gpu

_ctx = {}


@pytest.fixture(scope="module")
def plans():
    kept = {}
    yield kept
    pipeline.close_plans(kept)


class _Ctx(lat._Ctx, rh.Ctx):
    """rig_hard.Ctx's frames and derived levels, with what the lattice's driver needs on the device (the coverage masks)."""


def _context(oracle, name, gpu):
    if name not in _ctx:
        _ctx[name] = _Ctx(oracle, name, gpu)
    return _ctx[name]


def _flat(res, key):
    return [v for r in res for v in r[key]]


# ---- 1. the table --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,key,part", lat.CASES, ids=[f"{n}-{l2.key_id(k)}" + (f"-rows{p}" if len(lat.GROUPS[k]) > lat.PART else "") for n, k, p in lat.CASES])
def test_rows_on_hard_content(st, gpu, oracle, plans, name, key, part):
    ctx, synthetic = _context(oracle, name, gpu), lat._context(oracle, name, gpu)
    rows = lat.GROUPS[key][part:part + lat.PART]
    rig = lat._make(ctx, rows[0])
    try:
        for opt in rows:
            forms_host = synthetic.frames(opt["input"], opt["calls"][0], ctx.matrix_of(opt))
            res = lat._run_row(rig, ctx, opt, oracle, plans, chain=ctx.chain_options(opt), host=ctx.host(opt), forms_host=forms_host)
            assert _flat(res, "status") == [rh.REFUSED.get((name, opt["index"], i), 0) for i in range(sum(opt["calls"][0]))], (name, opt["index"])
            for r in res:
                refused = [s for s in r["status"] if s]
                if refused:  # exactly that refusal; the rig is left with neither state nor anchor
                    assert r["rc"] == refused[0] and not r["anchor"][1]
                    assert r["state"] is None or (r["state"][1] == [False] * len(ctx.steps) and not r["state"][0].any())
                else:
                    assert r["rc"] == 0
    finally:
        rig.close()


REFUSED_STREAMS = {  # on odd_h, the table's classes by the row index: a checkerboard set that step 0's scan refuses (-3), under smoothing
    "first_of_two_sequences": (dict(l2.NONE, exposure=(2, ("keep", 64)), calls=((3, 2), 2), index=35), [[-3, 0, 0], [0, 0]]),
    "second_of_one_sequence": (dict(l2.NONE, exposure=(1, ("keep", 192)), calls=((3,), 16), index=34), [[0, -3, 0]]),
}


@pytest.mark.parametrize("stream", list(REFUSED_STREAMS))
def test_a_refused_set_takes_no_further_part_in_the_filter(st, gpu, oracle, plans, stream):
    """include/stitch_rig_exposure_temporal.h: a set refused at step 0 enters step 0's filter and no later one, so the sets behind it
    -- in its launch sequence, and in the next, whose flags start clear -- are the CPU statement's, which ends a refused set at the
    step that refuses it.  The call leaves no state; the call after it starts a stream of its own."""
    ctx = _context(oracle, "odd_h", gpu)
    opt, statuses = REFUSED_STREAMS[stream]
    rig = lat._make(ctx, opt)
    try:
        res = lat._run_row(rig, ctx, opt, oracle, plans, chain=ctx.chain_options(opt), host=ctx.host(opt))
        assert [r["status"] for r in res] == statuses
        assert res[0]["state"][1] == [False, False] and (len(res) == 1 or res[1]["state"][1] == [True, True])
    finally:
        rig.close()


# ---- 2. the fused projection ------------------------------------------------------------------------------------------------------------------
SIZES = (((64, 48), None), ((40, 32), None), ((48, 64), capi.EX6_OPTS), ((64, 37), None))  # landscape tiled twice, the portrait kernel, an odd height
FMT_NAMES = {pyr.RGB24: "rgb24", pyr.BGR24: "bgr24", pyr.RGBX32: "rgbx32", pyr.BGRX32: "bgrx32", pyr.NV12: "nv12", pyr.YUYV: "yuyv", pyr.UYVY: "uyvy",
             pyr.NV21: "nv21", pyr.NV16: "nv16"}


@pytest.mark.parametrize("fmt", rh.ALL_INPUTS, ids=[FMT_NAMES[f] for f in rh.ALL_INPUTS])
@pytest.mark.parametrize("size,opts", SIZES, ids=[f"{w}x{h}" for (w, h), _ in SIZES])
def test_the_fused_projection_on_camera_bytes(st, gpu, oracle, size, opts, fmt):
    w, h = size
    rig = capi.Rig.from_steps([size], 0, [], opts=opts, finish=False, max_sets=2)
    try:
        assert (rig.width, rig.height, rig.n_steps) == (w, h, 0)
        for matrix in ((0, 1, 2) if fmt in rh.YUV else (0,)):
            rig.set_formats(fmt, pyr.PLANAR, matrix)
            for cls in ("raw", "edges"):
                for n in (1, 3):
                    images = [rh.image_of(cls, fmt, w, h, 1000 * fmt + 10 * n + i) for i in range(n)]
                    want = [oracle.project(pyr.unpack(im, matrix)) for im in images]
                    outs = {}
                    for offset, form in ((0, capi.RIG_INPUT_FUSED), (1, capi.RIG_INPUT_CONVERTED)):
                        got = rig.stitch([[to_dev(im, gpu, offset)] for im in images])
                        what = (FMT_NAMES[fmt], matrix, cls, n, offset)
                        assert got[1] == [0] * n and rig.last_rc == 0 and rig.input_form(0) == form, what
                        outs[form] = [lat._host_out(o) for o in got[0]]
                    for i in range(n):
                        fused, converted = outs[capi.RIG_INPUT_FUSED][i], outs[capi.RIG_INPUT_CONVERTED][i]
                        assert fused.shape == converted.shape == want[i].shape == (3, h, w)
                        assert np.array_equal(converted, want[i]), f"{what}: set {i}, the converted input against the oracle"
                        assert np.array_equal(fused, converted), f"{what}: set {i}, the fused input against the converted one"
    finally:
        rig.close()


# ---- 3. the contrast set ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [0, 2])
def test_the_contrast_set(st, gpu, oracle, plans, mode):
    ctx = _context(oracle, "w64_65", gpu)
    opt = rh.contrast_row(mode)
    host = [[[(p, 0) for p in fs] for fs in sets] for sets in rh.contrast_frames(ctx.sizes)]
    rig = lat._make(ctx, opt)
    try:
        res = lat._run_row(rig, ctx, opt, oracle, plans, chain=ctx.chain_options(opt), host=host)  # paths, costs, moved, records, outputs: the CPU statement's
        assert [len(r["status"]) for r in res] == [3, 2] and not any(_flat(res, "status")) and res[0]["anchor"][1] and res[1]["anchor"][1]
        assert all(len(r["paths"]) == len(r["status"]) and r["records"].shape[0] == len(r["status"]) for r in res)
    finally:
        rig.close()
