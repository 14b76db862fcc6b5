"""CPU: the oracle against the reference's own functions on fixed seeded inputs.

The reference runs where oracle/Makefile could compile it (oracle/_ref/libref_hotpath.so, libref6_hotpath.so); everywhere
else its results for exactly these inputs are replayed from tests/golden/reference_results.json (the colour transfer, whose last bit belongs to the platform's libm, has a
recording of its own: tests/golden/transfer.npz, see the section at the end).  A result is kept as what
the comparison needs: a digest of an array's shape and values (as float64, so -0.0 == 0.0 as in np.array_equal), numbers
as they are; the key is the function and a digest of its inputs, so changed inputs find no recording and fail.  Where the
reference is built, every result is also checked against its recording; STITCH_RECORD_REFERENCE=1 rewrites the recording
from the live reference (run this module there)."""
import hashlib
import json
import os

import numpy as np
import pytest

import transfer_cases as T
from oracle_lib import REF6_SO, Reference, ReferenceEx6, have_reference, have_reference_transfer

RECORDING = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reference_results.json")


def digest(v):
    """What an equality comparison needs of a value, as JSON."""
    if isinstance(v, np.ndarray):
        a = np.ascontiguousarray(v).astype(np.float64) + 0.0
        return "sha256:" + hashlib.sha256(repr(a.shape).encode() + a.tobytes()).hexdigest()
    if isinstance(v, (bytes, bytearray)):
        return "sha256:" + hashlib.sha256(bytes(v)).hexdigest()
    if isinstance(v, (list, tuple)):
        return [digest(x) for x in v]
    if isinstance(v, (bool, np.bool_)):
        return bool(v)
    if isinstance(v, (int, np.integer)):
        return int(v)
    if isinstance(v, (float, np.floating)):
        return float(v)
    return v


class Recorded:
    """The reference's functions (live: Reference / ReferenceEx6 or None), every result returned as digest(result);
    NAME_bits is NAME's float32 result as bit patterns."""

    def __init__(self, live, prefix, recording):
        self.live, self.prefix, self.recording = live, prefix, recording

    def __getattr__(self, name):
        def call(*args):
            inputs = [a for a in args if not isinstance(a, os.PathLike)]  # a scratch directory is not an input
            key = self.prefix + name + ":" + hashlib.sha256(json.dumps(digest(inputs)).encode()).hexdigest()[:40]
            if self.live is None:
                assert key in self.recording["results"], f"no recorded reference result of {name} for these inputs"
                return self.recording["results"][key]
            res = getattr(self.live, name[:-len("_bits")] if name.endswith("_bits") else name)(*args)
            got = json.loads(json.dumps(digest(bits(res) if name.endswith("_bits") else res)))
            if not self.recording["rewrite"]:
                assert self.recording["results"].get(key) == got, f"the reference's {name} differs from its recording"
            self.recording["new"][key] = got
            return got
        return call


@pytest.fixture(scope="module")
def recording():
    rewrite = os.environ.get("STITCH_RECORD_REFERENCE") == "1"
    with open(RECORDING) as f:
        rec = {"results": json.load(f), "new": {}, "rewrite": rewrite}
    yield rec
    if rewrite:
        with open(RECORDING, "w") as f:
            json.dump(dict(sorted(rec["new"].items())), f, indent=0)
            f.write("\n")


@pytest.fixture(scope="module")
def ref(recording):
    return Recorded(Reference() if have_reference() else None, "", recording)


@pytest.fixture(scope="module")
def ref6(recording):
    return Recorded(ReferenceEx6() if os.path.exists(REF6_SO) else None, "ex6.", recording)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.mark.parametrize("w,h,f", [(384, 512, 1), (400, 300, 2), (97, 61, 3), (61, 97, 4), (2, 2, 5), (1, 9, 6), (9, 1, 7)])
def test_project(oracle, ref, w, h, f):
    src = oracle.synth(w, h, f)
    assert digest(oracle.project(src)) == ref.project(src)


def test_map_and_bbox(oracle, ref):
    rng = np.random.default_rng(3)
    for _ in range(200):
        p = [1 + rng.normal() * 0.05, rng.normal() * 0.05, rng.normal() * 1e-4, rng.normal() * 300,
             rng.normal() * 0.05, 1 + rng.normal() * 0.05, rng.normal() * 1e-5, rng.normal() * 20]
        x, y = np.float32(rng.uniform(-500, 1500)), np.float32(rng.uniform(-500, 1500))
        assert digest(oracle.map_xy(x, y, p)) == ref.map_xy(x, y, p)


@pytest.mark.parametrize("seed", range(4))
def test_warp_move_random_maps(oracle, ref, seed):
    rng = np.random.default_rng(seed)
    src = oracle.synth(200, 150, seed)
    p = [1 + rng.normal() * 0.03, rng.normal() * 0.03, rng.normal() * 1e-4, rng.normal() * 80,
         rng.normal() * 0.03, 1 + rng.normal() * 0.03, rng.normal() * 1e-5, rng.normal() * 10]
    offx, offy = np.float32(rng.uniform(-40, 0.99)), np.float32(rng.uniform(-9, 0.99))
    assert digest(oracle.warp(src, p, offx, offy, 333, 177)) == ref.warp(src, p, offx, offy, 333, 177)
    ox, oy = int(rng.integers(-50, 50)), int(rng.integers(-20, 20))
    assert digest(oracle.move(src, ox, oy, 333, 177)) == ref.move(src, ox, oy, 333, 177)


def test_warp_truncation_toward_zero(oracle, ref):
    """coordinates in (-1,0) truncate to 0 and are therefore INSIDE the source (ImageProcess.cpp:598-600)"""
    src = oracle.synth(40, 30, 1)
    p = [1, 0, 0, -0.5, 0, 1, 0, -0.75]
    a, b = oracle.warp(src, p, 0.0, 0.0, 50, 40), ref.warp(src, p, 0.0, 0.0, 50, 40)
    assert digest(a) == b and a[0, 0, 0] == src[0, 0, 0]


@pytest.mark.parametrize("w,h,c", [(540, 3, 1), (17, 9, 3), (2, 2, 1), (3, 5, 2), (64, 1, 1), (1, 64, 1), (300, 200, 3)])
@pytest.mark.parametrize("gauss", [True, False])
def test_blur(oracle, ref, w, h, c, gauss):
    x = (np.random.default_rng(w * h).random((c, h, w)) * 255).astype(np.float32)
    assert digest(bits(oracle.blur(x, 2.0, 0 if gauss else 1))) == ref.cimg_blur_bits(x, 2.0, gauss)


@pytest.mark.parametrize("w,h", [(1081, 527), (67, 33), (4, 2), (3, 3), (135, 65), (600, 800)])
def test_resize(oracle, ref, w, h):
    rng = np.random.default_rng(w + h)
    w2, h2 = max(1, w // 2), max(1, h // 2)
    x = (rng.random((3, h, w)) * 255).astype(np.float32)
    assert digest(bits(oracle.decimate(x, w2, h2))) == ref.cimg_resize_bits(x, w2, h2)
    y = (rng.random((3, h2, w2)) * 255).astype(np.float32)
    assert digest(bits(oracle.expand(y, w, h))) == ref.cimg_resize_bits(y, w, h)


@pytest.mark.parametrize("w,h", [(67, 33), (270, 131), (333, 222), (100, 64), (33, 67), (640, 480)])
def test_blend(oracle, ref, w, h):
    for a_left in (True, False):
        A, B = oracle.synth(w, h, 21), oracle.synth(w, h, 22)
        if a_left:
            A[:, :, (2 * w) // 3:] = 0
            B[:, :, : w // 3] = 0
        else:
            A[:, :, : w // 3] = 0
            B[:, :, (2 * w) // 3:] = 0
        rc, out, _ = oracle.blend(A, B)
        assert rc == 0 and digest(out) == ref.blend(A, B)


def test_equalize(oracle, ref):
    for f in range(3):
        img = oracle.synth(311, 173, 30 + f)
        img[f % 3] = np.maximum(img[f % 3], 150 + 40 * f)
        img[:, :50, :70] = 0
        assert digest(oracle.equalize(img)[0]) == ref.equalize(img)


def test_blend_random_sizes_sweep(oracle, ref):
    """40 random canvas sizes (odd/even mixes at every pyramid level, both seam branches, ragged content): the oracle
    equals the reference byte for byte or reports the degenerate-pyramid case the reference cannot express."""
    rng = np.random.default_rng(1234)
    done = 0
    while done < 40:
        w, h = int(rng.integers(2, 260)), int(rng.integers(2, 200))
        n, _, _ = oracle.pyramid_levels(w, h)
        A, B = oracle.synth(w, h, int(rng.integers(0, 50))), oracle.synth(w, h, int(rng.integers(50, 100)))
        ca, cb = sorted(int(v) for v in rng.integers(0, w + 1, 2))
        if rng.random() < 0.5:
            A[:, :, cb:] = 0
            B[:, :, :ca] = 0
        else:
            A[:, :, :ca] = 0
            B[:, :, cb:] = 0
        rc, out, seam = oracle.blend(A, B)
        if n < 0:
            assert rc == -4
            continue
        if rc != 0:
            assert rc in (-2, -3)  # empty mid row / no overlap: the reference hangs or divides 0/0 here
            continue
        assert digest(out) == ref.blend(A, B), (w, h)
        done += 1


def test_bbox(oracle, ref):
    # the reference's canvas sizing inputs (ImageProcess.cpp:206-216) -- used by stitch_canvas_bbox's test as well
    p = [0.9724, -0.0398, 0.000149, 206.67, 0.00141, 1.00076, -1.2e-06, 4.55]
    mn_x, mn_y, mx_x, mx_y = ref.bbox(384, 512, p)
    corners = [oracle.map_xy(np.float32(x), np.float32(y), p) for x in (0, 383) for y in (0, 511)]
    assert mn_x == min(c[0] for c in corners) and mx_x == max(c[0] for c in corners)
    assert mn_y == min(c[1] for c in corners) and mx_y == max(c[1] for c in corners)


def test_gray_bbox_features(oracle, ref):
    """toGrayScale, canvas sizing, feature updates."""
    rng = np.random.default_rng(7)
    for f in range(3):
        img = oracle.synth(123, 77, 40 + f)
        g, gf = oracle.gray(img)
        assert digest(g) == ref.gray(img) and np.array_equal(gf, g.astype(np.float32))
    for _ in range(100):
        p = [1 + rng.normal() * 0.05, rng.normal() * 0.05, rng.normal() * 2e-4, rng.normal() * 300,
             rng.normal() * 0.05, 1 + rng.normal() * 0.05, rng.normal() * 2e-5, rng.normal() * 20]
        fw, fh, rw, rh = (int(v) for v in rng.integers(50, 900, 4))
        assert digest(oracle.canvas_bbox(fw, fh, p, rw, rh)) == ref.canvas(fw, fh, p, rw, rh)
    p = [0.9724, -0.0398, 0.000149, 206.67, 0.00141, 1.00076, -1.2e-06, 4.55]
    x, y = rng.uniform(0, 384, 200).astype(np.float32), rng.uniform(0, 512, 200).astype(np.float32)
    a, b = oracle.map_points(x, y, p, -230.579239, -4.68064785), ref.update_features(x, y, p, -230.579239, -4.68064785, 0, 0, False)
    assert len(a) == len(b) == 4 and digest(list(a)) == b
    a, b = oracle.shift_points(x, y, -230, -4), ref.update_features(x, y, p, 0, 0, -230, -4, True)
    assert len(a) == len(b) == 4 and digest(list(a)) == b


@pytest.mark.parametrize("w,h", [(257, 129), (5, 3), (1, 7), (64, 64), (2, 2), (1027, 3), (1368, 17)])
def test_bmp_load_save(oracle, ref, w, h, tmp_path):
    """oracle_bmp_decode/encode against CImg::load_bmp / save_bmp for every 24/32-bit header
    layout the loader distinguishes, including files that end early."""
    from oracle_lib import make_bmp
    img = oracle.synth(w, h, 3)
    for kw in [dict(), dict(bpp=32), dict(top_down=True), dict(header_size=108), dict(extra_gap=10), dict(extra_gap=1), dict(size_field=0),
               dict(size_field=60), dict(truncate=7), dict(truncate=3 * w + 5), dict(bpp=32, top_down=True, header_size=124, extra_gap=3)]:
        data = make_bmp(img, **kw)
        if len(data) < 54:
            continue
        rc, got = oracle.bmp_decode(data)
        want = ref.load_bmp_bytes(data, tmp_path)
        assert rc == 0 and digest(got) == want, kw  # the digest covers the shape
    assert digest(oracle.bmp_encode(img)) == ref.save_bmp_bytes(img, tmp_path)


# ---- the src/ex6 variant of the blend (Deriche blur, depth from min(w,h), three-channel seam scan with double ratios) ----
@pytest.mark.parametrize("w,h", [(67, 33), (270, 131), (333, 222), (100, 64), (33, 67), (640, 480), (600, 800)])
def test_blend_ex6_whole_function(oracle, ref6, w, h):
    """oracle.blend with the variant options against the variant's own ImageProcess::blend
    (src/ex6/ImageProcess.cpp:638-742, compiled in place): byte for byte, both seam branches."""
    from oracle_lib import EX6_OPTS
    for a_left in (True, False):
        A, B = oracle.synth(w, h, 21), oracle.synth(w, h, 22)
        if a_left:
            A[:, :, (2 * w) // 3:] = 0
            B[:, :, : w // 3] = 0
        else:
            A[:, :, : w // 3] = 0
            B[:, :, (2 * w) // 3:] = 0
        rc, out, _ = oracle.blend(A, B, EX6_OPTS)
        assert rc == 0 and digest(out) == ref6.blend(A, B), (w, h, a_left)


def test_blend_ex6_random_sizes_sweep(oracle, ref6):
    from oracle_lib import EX6_OPTS
    rng = np.random.default_rng(99)
    done = 0
    while done < 25:
        w, h = int(rng.integers(4, 260)), int(rng.integers(4, 200))
        A, B = oracle.synth(w, h, int(rng.integers(0, 50))), oracle.synth(w, h, int(rng.integers(50, 100)))
        ca, cb = sorted(int(v) for v in rng.integers(0, w + 1, 2))
        if rng.random() < 0.5:
            A[:, :, cb:] = 0
            B[:, :, :ca] = 0
        else:
            A[:, :, :ca] = 0
            B[:, :, cb:] = 0
        if rng.random() < 0.3:  # a channel that is empty where the others are not: the three-channel "non-empty" rule differs from the root's
            A[int(rng.integers(0, 3)), :, ca:ca + 5] = 0
        rc, out, seam = oracle.blend(A, B, EX6_OPTS)
        if rc != 0:
            continue  # empty mid row / no overlap / degenerate pyramid: the variant hangs or divides 0/0 there
        assert digest(out) == ref6.blend(A, B), (w, h)
        done += 1


# ---- the l-alpha-beta colour transfer against the reference's transfer.cpp (oracle/ref_transfer.cpp) ----------------------
# Two modes.  With use_libm the restatement calls the same logf / pow as the reference built next to it, so the two must agree
# in every bit: that pins every promotion, the order of the running sums, the == 0 -> 1 rule, the clamps, the final cast and
# the layout of the statistics.  Live only, because the bits belong to the libm both sides share.  Without it the restatement
# evaluates include/stitch_elem.h (what the HIP kernels evaluate), which is the same on every platform: its result is replayed
# from tests/golden/transfer.npz, which also holds the few bytes where a glibc build of the reference differs.
@pytest.fixture(scope="module")
def ref_transfer():
    if not have_reference_transfer():
        pytest.skip("the reference's transfer is not built here (make -C oracle ref); the replay tests below run everywhere")
    return Reference()


@pytest.fixture(scope="module")
def transfer_recording():
    return T.Recording()


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


@pytest.mark.parametrize("name,rs,rt", T.CASES, ids=T.CASE_NAMES)
def test_transfer_libm_mode_is_the_reference(oracle, ref_transfer, name, rs, rt):
    """oracle.transfer(use_libm=True) == transfer::transfer of the reference: every output byte, every bit of the twelve
    statistics.  The cases are what transfer.cpp distinguishes (tests/transfer_cases.py says which is which)."""
    src, tem = T.build_image(rs, oracle), T.build_image(rt, oracle)
    want, wst = ref_transfer.transfer(src, tem)
    got, gst = oracle.transfer(src, tem, use_libm=True)
    assert np.array_equal(bits(gst), bits(wst)), (gst, wst)
    assert np.array_equal(got, want), int((got != want).sum())


def test_transfer_per_pixel_every_colour(oracle, ref_transfer):
    """The reference's two public per-pixel functions against the restatement's (libm mode), bit for bit: RGBtoLab for all
    2^24 colours, LabToRGB for the l-alpha-beta values those colours give, shifted and scaled so that the clamps at 0 and
    255 are both met."""
    rgb = np.ascontiguousarray(T.every_colour(1).reshape(3, -1).T, np.float32)
    want = ref_transfer.rgb_to_lab(rgb)
    assert np.array_equal(bits(oracle.rgb_to_lab(rgb, use_libm=True)), bits(want))
    lab = want[::7] * np.float32(1.25) - np.float32(0.5)
    back = ref_transfer.lab_to_rgb(lab)
    assert back.min() == 0 and back.max() == 255
    assert np.array_equal(bits(oracle.lab_to_rgb(lab, use_libm=True)), bits(back))


def test_transfer_without_libm_dependence(oracle, ref):
    """Where no libm rounding enters, both modes of the restatement equal the reference on any platform, so these go through
    the recording: black images (log(1) = 0, sd = 0, 0 * 0 / 0 = NaN through pow and the clamps), and LabToRGB of values
    whose powers are 0, 1, inf or NaN (IEEE pow fixes those)."""
    inf, nan = np.float32(np.inf), np.float32(np.nan)
    lab = np.array([[0, 0, 0], [inf, 0, 0], [-inf, 0, 0], [nan, 0, 0], [0, inf, 0], [0, -inf, 0], [0, 0, inf], [0, 0, -inf], [0, nan, 0], [0, 0, nan],
                    [1e30, 0, 0], [-1e30, 0, 0], [0, 1e30, 0], [0, -1e30, 0], [0, 0, 1e30], [0, 0, -1e30], [inf, -inf, 0], [nan, inf, -inf]], np.float32)
    want = ref.lab_to_rgb_bits(lab)
    black, black_tem = np.zeros((3, 17, 20), np.uint8), np.zeros((3, 3, 5), np.uint8)
    want_t = ref.transfer(black, black_tem)
    for use_libm in (False, True):
        assert digest(bits(oracle.lab_to_rgb(lab, use_libm=use_libm))) == want
        out, st = oracle.transfer(black, black_tem, use_libm=use_libm)
        assert digest([out, st]) == want_t and not out.any() and not st.any()


def test_transfer_recording_covers_the_cases(transfer_recording):
    assert list(transfer_recording.cases) == T.CASE_NAMES
    m = transfer_recording.meta
    assert m["total_differing_bytes"] == sum(c["differing_bytes"] for c in m["cases"].values()) <= 1e-5 * m["total_bytes"]


@pytest.mark.parametrize("name", T.CASE_NAMES)
def test_transfer_specified_mode_replay(oracle, transfer_recording, name):
    """oracle.transfer with the specified functions of include/stitch_elem.h against the recording, no tolerance: its bytes
    and statistic bits are the recorded specified-function ones, and with the recorded differing bytes (each one grey level,
    18 of 1.06e8 over all cases) replaced it IS the reference's output, by SHA-256 and in full where the output is stored."""
    c = transfer_recording.cases[name]
    src, tem = transfer_recording.images(name, oracle)
    assert sha(src) == c["src_sha256"] and sha(tem) == c["tem_sha256"]
    out, st = oracle.transfer(src, tem)
    assert list(out.shape) == c["shape"] and sha(out) == c["spec_sha256"]
    assert [int(v) for v in bits(st)] == c["spec_stats_bits"]
    as_ref = transfer_recording.as_reference(name, out)
    assert sha(as_ref) == c["ref_sha256"]
    pos, ref_b, spec_b = transfer_recording.diffs(name)
    assert pos.size == c["differing_bytes"] and np.all(np.abs(ref_b.astype(int) - spec_b.astype(int)) == 1)
    full = transfer_recording.ref_out(name)
    assert (full is not None) == (out.nbytes <= T.FULL_OUTPUT_LIMIT)
    if full is not None:
        assert np.array_equal(as_ref, full)
