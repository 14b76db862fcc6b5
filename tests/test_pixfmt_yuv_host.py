"""CPU: the host side of the 4:2:2 layouts and NV21 (include/stitch_rig_formats_yuv.h) -- the header compiles as C99, the binding's
table RIG_FORMAT_YUV_SIGNATURES states exactly what it declares and shares no name with the other tables, stitch_image keeps its size
and offsets; tests/pixfmt_yuv_ref.py obeys the identities the header promises; stitch_image_bytes answers and refuses as the header
says; stitch_rig_set_formats takes every pair of {0 .. 5, 16 .. 19} and refuses 6 .. 15 and 20, leaving the rig as it was; every
argument error of the calls is reported before a device is needed; stitch_rig_input_form refuses what it must and says NONE before
any replay."""
import ctypes as C
import os
import re
import shlex
import subprocess

import numpy as np
import pytest

import pixfmt_yuv_ref as yf
import rig_seams_ref as ref
from test_pixfmt_host import RETURNS, SCALARS, _formats

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "stitch_rig_formats_yuv.h")
FUNCTIONS = ("stitch_rig_input_form",)
NAMES = {"YUYV": 16, "UYVY": 17, "NV21": 18, "NV16": 19}
FORMS = {"NONE": 0, "FUSED": 1, "CONVERTED": 2}
SIZES = [(1, 1), (2, 3), (3, 2), (67, 5), (50, 37), (4096, 4096)]


def _header_text():
    return re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)


def _declared():
    sigs = {}
    for ret, name, params in re.findall(r"((?:const\s+)?\w+\s*\*?)\s*\b(stitch_\w+)\s*\(([^()]*)\)\s*;", _header_text()):
        prms = [] if params.strip() == "void" else [" ".join(p.split()) for p in params.split(",")]
        args = [C.c_void_p if ("*" in p or "[" in p) else SCALARS[" ".join(p.split()[:-1])] for p in prms]
        sigs[name] = (RETURNS[" ".join(ret.replace("*", " *").split())], args)
    return sigs


def pitches(fmt, w):
    """Tight, tight + 5, and rounded up to 16 plus 16."""
    t = yf.tight(fmt, w)
    up = lambda v: (-(-v // 16) * 16 + 16) if v else 0  # noqa: E731
    return [t, (t[0] + 5, t[1] + 5 if t[1] else 0), (up(t[0]), up(t[1]))]


def test_signature_table_states_the_header(st):
    capi = st.capi
    want, lib = _declared(), capi.lib()
    assert sorted(want) == sorted(FUNCTIONS) == sorted(set(re.findall(r"\b(stitch_[a-z0-9_]+)\s*\(", _header_text())))
    assert sorted(capi.RIG_FORMAT_YUV_SIGNATURES) == sorted(want)
    others = set()
    for name in dir(capi):
        if name.endswith("SIGNATURES") and name != "RIG_FORMAT_YUV_SIGNATURES":
            others |= set(getattr(capi, name))
    assert "stitch_image_bytes" in others and not set(capi.RIG_FORMAT_YUV_SIGNATURES) & others
    bound = {n: (getattr(lib, n).restype, getattr(lib, n).argtypes) for n in want}  # every name is exported
    wrong = {n: (bound[n], want[n]) for n in sorted(want) if bound[n] != tuple(want[n])}
    assert not wrong, f"(bound, declared) signatures differ for: {wrong}"
    # the constants: the header's, the binding's and the reference's
    assert {k: int(v) for k, v in re.findall(r"#define\s+STITCH_PIX_(\w+)\s+(\d+)", _header_text())} == NAMES
    assert {k: int(v) for k, v in re.findall(r"#define\s+STITCH_RIG_INPUT_(\w+)\s+(\d+)", _header_text())} == FORMS
    for n, v in NAMES.items():
        assert getattr(capi, "PIX_" + n) == getattr(yf, n) == v
    for n, v in FORMS.items():
        assert getattr(capi, "RIG_INPUT_" + n) == v


def test_header_is_c99_and_stitch_image_keeps_its_layout(st, tmp_path):
    capi = st.capi
    cc = shlex.split(os.environ.get("CC", "cc")) + ["-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include")]
    fields = ["data", "data2", "width", "height", "pitch", "pitch2"]
    src = tmp_path / "uses.c"
    src.write_text("\n".join(['#include "stitch_rig_formats_yuv.h"', "int main(void) {"] + [f"    (void)(&{n});" for n in FUNCTIONS]
                             + [f"    (void)(STITCH_PIX_{n});" for n in NAMES] + [f"    (void)(STITCH_RIG_INPUT_{n});" for n in FORMS] + ["    return 0;", "}", ""]))
    r = subprocess.run(cc + ["-c", str(src), "-o", str(tmp_path / "uses.o")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    got = []
    for header in ("stitch_rig_formats.h", "stitch_rig_formats_yuv.h"):  # the same struct with and without the new header
        lay = tmp_path / "layout.c"
        lay.write_text("\n".join(["#include <stdio.h>", f'#include "{header}"', "int main(void) {", '    printf("%zu", sizeof(stitch_image));']
                                 + [f'    printf(" %zu", offsetof(stitch_image, {f}));' for f in fields] + ["    return 0;", "}", ""]))
        exe = tmp_path / "layout"
        r = subprocess.run(cc + [str(lay), "-o", str(exe)], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        got.append([int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()])
    assert got[0] == got[1] == [32, 0, 8, 16, 20, 24, 28] == [C.sizeof(capi.ImageDesc)] + [getattr(capi.ImageDesc, f).offset for f in fields]


# ---- the reference itself -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("matrix", [0, 1, 2])
def test_ref_grey_has_neutral_chroma_through_422(matrix):
    grey = np.broadcast_to(np.arange(256, dtype=np.uint8)[None, None, :], (3, 2, 256)).copy()
    for shift in (0, 1):  # every grey beside its neighbour, on either side of a pair
        planar = np.roll(grey, shift, axis=2)[:, :, :255 if shift else 256]  # (an odd width: the clamped last pair too)
        for fmt in (yf.YUYV, yf.UYVY, yf.NV16):
            im = yf.pack(planar, fmt, matrix)
            if fmt == yf.NV16:
                assert (im["data2"] == 128).all()
            else:
                g = im["data"].reshape(2, -1, 4)
                assert (g[:, :, yf.GROUP[fmt][1]] == 128).all() and (g[:, :, yf.GROUP[fmt][3]] == 128).all()
            back = yf.unpack(im, matrix)
            assert (back[0] == back[1]).all() and (back[1] == back[2]).all() and np.abs(back.astype(int) - planar).max() <= 2


def test_ref_yuyv_to_uyvy_and_nv12_to_nv21_are_byte_permutations():
    rng = np.random.default_rng(5)
    for w, h in ((1, 1), (3, 2), (8, 3), (67, 5)):
        planar = rng.integers(0, 256, (3, h, w), dtype=np.uint8)
        for matrix in (0, 1, 2):
            a, b = yf.pack(planar, yf.YUYV, matrix, pitch=yf.tight(yf.YUYV, w)[0] + 5), yf.pack(planar, yf.UYVY, matrix, pitch=yf.tight(yf.UYVY, w)[0] + 5)
            ga, gb = (np.stack([x["data"][y * x["pitch"]:][:4 * ((w + 1) // 2)] for y in range(h)]).reshape(h, -1, 4) for x in (a, b))
            assert np.array_equal(ga[:, :, [1, 0, 3, 2]], gb) and len(a["data"]) == len(b["data"])
            c, d = yf.pack(planar, yf.NV12, matrix, pitch2=2 * ((w + 1) // 2) + 3), yf.pack(planar, yf.NV21, matrix, pitch2=2 * ((w + 1) // 2) + 3)
            assert np.array_equal(c["data"], d["data"]) and len(c["data2"]) == len(d["data2"])
            pc, pd = (np.stack([x["data2"][j * x["pitch2"]:][:2 * ((w + 1) // 2)] for j in range((h + 1) // 2)]).reshape((h + 1) // 2, -1, 2) for x in (c, d))
            assert np.array_equal(pc[:, :, ::-1], pd)
            # and the decode reads them back alike
            assert np.array_equal(yf.unpack(a, matrix), yf.unpack(b, matrix)) and np.array_equal(yf.unpack(c, matrix), yf.unpack(d, matrix))


def test_ref_422_of_equal_column_pairs_is_the_per_pixel_encode_and_decode():
    import pixfmt_ref as pf
    rng = np.random.default_rng(6)
    for w, h in ((2, 1), (7, 3), (64, 5)):
        half = rng.integers(0, 256, (3, h, (w + 1) // 2), dtype=np.uint8)
        planar = np.repeat(half, 2, axis=2)[:, :, :w]
        for matrix in (0, 1, 2):
            want = np.stack(pf.decode(*pf.encode(planar[0], planar[1], planar[2], matrix), matrix))
            for fmt in (yf.YUYV, yf.UYVY, yf.NV16):
                assert np.array_equal(yf.unpack(yf.pack(planar, fmt, matrix), matrix), want), (fmt, matrix, w, h)


def test_ref_layouts_padding_and_the_clamped_y1():
    planar = np.arange(3 * 2 * 3, dtype=np.uint8).reshape(3, 2, 3) * 13
    import pixfmt_ref as pf
    Y, u, v = pf.encode(planar[0], planar[1], planar[2], 0)
    im = yf.pack(planar, yf.YUYV, 0, pitch=11)
    assert len(im["data"]) == 11 + 8 == yf.image_bytes(yf.YUYV, 3, 2, 11)[0] and im["data2"] is None and yf.image_bytes(yf.YUYV, 3, 2, 11)[1] == 0
    assert (im["data"][8:11] == 0xEE).all()
    for y in range(2):
        row = im["data"][11 * y:11 * y + 8]
        assert row.tolist() == [Y[y, 0], (int(u[y, 0]) + int(u[y, 1]) + 1) >> 1, Y[y, 1], (int(v[y, 0]) + int(v[y, 1]) + 1) >> 1, Y[y, 2], u[y, 2], Y[y, 2], v[y, 2]]
    # the Y1 byte of the last group is ignored on input
    other = dict(im, data=im["data"].copy())
    other["data"][[6, 17]] ^= 0xFF
    assert np.array_equal(yf.unpack(other, 0), yf.unpack(im, 0))
    nv = yf.pack(planar, yf.NV16, 0, pitch=5, pitch2=7)
    assert (len(nv["data"]), len(nv["data2"])) == (5 + 3, 7 + 4) == yf.image_bytes(yf.NV16, 3, 2, 5, 7)
    assert nv["data2"][:4].tolist() == im["data"][[1, 3, 5, 7]].tolist() and (nv["data2"][4:7] == 0xEE).all()
    assert yf.image_bytes(yf.NV21, 3, 2, 5, 7) == pf.image_bytes(pf.NV12, 3, 2, 5, 7)
    for fmt in range(6):  # the old codes pass through
        assert yf.tight(fmt, 7) == pf.tight(fmt, 7) and yf.image_bytes(fmt, 7, 3) == pf.image_bytes(fmt, 7, 3)


# ---- the library's host side ----------------------------------------------------------------------------------------------------
def test_image_bytes_answers_and_refusals(st):
    capi = st.capi
    L = capi.lib()
    for fmt in yf.NEW:
        for w, h in SIZES:
            for pitch, pitch2 in pitches(fmt, w):
                assert capi.image_bytes(fmt, w, h, pitch, pitch2) == yf.image_bytes(fmt, w, h, pitch, pitch2), (fmt, w, h, pitch, pitch2)
            assert capi.image_bytes(fmt, w, h) == yf.image_bytes(fmt, w, h) and capi.tight_pitches(fmt, w) == yf.tight(fmt, w)
    assert capi.image_bytes(capi.PIX_YUYV, 3, 2) == (16, 0) and capi.image_bytes(capi.PIX_NV16, 3, 2) == (6, 8) and capi.image_bytes(capi.PIX_NV21, 3, 3) == (9, 8)
    b = (C.c_size_t * 2)(7, 7)
    bad = [(6, 4, 4, 64, 64), (15, 4, 4, 64, 64), (20, 4, 4, 64, 64)]
    for fmt in yf.NEW:  # each minimum pitch less one, at an even and an odd width
        for w in (4, 5):
            t = yf.tight(fmt, w)
            bad.append((fmt, w, 4, t[0] - 1, t[1]))
            if t[1]:
                bad.append((fmt, w, 4, t[0], t[1] - 1))
        bad += [(fmt, 0, 4, 64, 64), (fmt, 4, 0, 64, 64)]
    for args in bad:
        assert L.stitch_image_bytes(*args, C.byref(b, 0), C.byref(b, C.sizeof(C.c_size_t))) == capi.ERR_ARG, args
        assert b"image_bytes" in L.stitch_last_error() and list(b) == [7, 7]
        assert yf.image_bytes(*args) is None
    assert L.stitch_image_bytes(16, 5, 4, 12, -1, None, None) == 0  # one plane: pitch2 is ignored; outputs are optional
    assert L.stitch_image_bytes(19, 5, 4, 5, 6, None, None) == 0


def test_set_formats_takes_every_pair_and_refuses_the_gap(st):
    capi = st.capi
    L = capi.lib()
    rig = capi.Rig.from_steps(ref.SMALL, 0, ref.small_steps(capi))
    for before in ((0, 0, 0), (capi.PIX_UYVY, capi.PIX_NV16, 2)):
        assert rig.set_formats(*before).formats == before == _formats(capi, rig)
        for code in list(range(6, 16)) + [20, 21, 255]:
            for args in ((code, 0, 0), (0, code, 0), (code, code, 1), (capi.PIX_YUYV, code, 0), (code, capi.PIX_NV21, 0)):
                assert L.stitch_rig_set_formats(rig._h, *args) == capi.ERR_ARG, args
                assert b"rig_set_formats" in L.stitch_last_error() and _formats(capi, rig) == before
        assert L.stitch_rig_set_formats(rig._h, capi.PIX_YUYV, capi.PIX_YUYV, 3) == capi.ERR_ARG and _formats(capi, rig) == before
    for i in yf.ALL:
        for o in yf.ALL:
            assert rig.set_formats(i, o, (i + o) % 3).formats == (i, o, (i + o) % 3)
    assert rig.clear_formats().formats == (0, 0, 0)
    assert rig.step_plan(0) is None  # no device was touched
    rig.close()


def _desc(capi, fmt, w, h, base=0x100000, pitch=None, pitch2=None, base2=0x800000):
    t = yf.tight(fmt, w)
    return capi.ImageDesc(base, base2 if t[1] else None, w, h, t[0] if pitch is None else pitch, t[1] if pitch2 is None else pitch2)


def test_argument_errors_come_before_a_device(st):
    import torch
    capi = st.capi
    L = capi.lib()
    planar = (C.c_void_p * 2)(0x4000000, 0x5000000)
    for call, who in ((lambda fmt, m, im, n: L.stitch_dev_unpack_many_u8(fmt, m, im, planar, n, None), b"unpack_many"),
                      (lambda fmt, m, im, n: L.stitch_dev_pack_many_u8(fmt, m, planar, im, n, None), b"pack_many")):
        two = lambda fmt, **kw: (capi.ImageDesc * 2)(_desc(capi, fmt, 9, 6), _desc(capi, fmt, 9, 6, base=0x200000, base2=0x900000, **kw))  # noqa: E731
        for fmt in (6, 15, 20):
            assert call(fmt, 0, two(16), 2) == capi.ERR_ARG and who in L.stitch_last_error()
        for fmt in yf.NEW:
            t = yf.tight(fmt, 9)
            for matrix in (-1, 3):
                assert call(fmt, matrix, two(fmt), 2) == capi.ERR_ARG
            assert call(fmt, 0, two(fmt, pitch=t[0] - 1), 2) == capi.ERR_ARG and who in L.stitch_last_error()
            if t[1]:
                assert call(fmt, 0, two(fmt, pitch2=t[1] - 1), 2) == capi.ERR_ARG
                bad = two(fmt)
                bad[1].data2 = None
                assert call(fmt, 0, bad, 2) == capi.ERR_ARG and b"null plane" in L.stitch_last_error()
            bad = two(fmt)
            bad[1].width = 10
            assert call(fmt, 0, bad, 2) == capi.ERR_ARG
            if not torch.cuda.is_available():
                assert call(fmt, 0, two(fmt), 2) == capi.ERR_NO_DEVICE

    # ---- the replay: UYVY in, NV16 out -----
    rig = capi.Rig.from_steps(ref.SMALL, 0, ref.small_steps(capi)).set_formats(capi.PIX_UYVY, capi.PIX_NV16)
    W, H = rig.width, rig.height

    def frames(fmt=capi.PIX_UYVY, **kw):
        return (capi.ImageDesc * 3)(*[_desc(capi, fmt, 64, 48, base=0x100000 * (i + 1), base2=0x100000 * (i + 1) + 0x80000, **kw) for i in range(3)])

    def out(fmt=capi.PIX_NV16, **kw):
        return (capi.ImageDesc * 1)(_desc(capi, fmt, kw.pop("w", W), kw.pop("h", H), base=0x4000000, base2=0x6000000, **kw))

    status = (C.c_int32 * 1)(77)
    call = lambda fr, o, n=1: L.stitch_dev_rig_stitch_fmt_u8(rig._h, fr, n, o, status, None, None, None)  # noqa: E731
    assert call(frames(pitch=2 * 64 - 1), out()) == capi.ERR_ARG and b"pitch" in L.stitch_last_error()
    assert call(frames(), out(pitch=W - 1)) == capi.ERR_ARG and call(frames(), out(pitch2=2 * ((W + 1) // 2) - 1)) == capi.ERR_ARG
    o = out()
    o[0].data2 = None
    assert call(frames(), o) == capi.ERR_ARG and b"null plane" in L.stitch_last_error()
    # overlap is judged by stitch_image_bytes, plane by plane, to the byte: the NV16 chroma plane's last byte on frame 1's first, and
    # its first byte on frame 1's last (a pass would run on these made-up addresses, so those are made without a device only)
    b1, b2 = capi.image_bytes(capi.PIX_NV16, W, H)
    f1 = capi.image_bytes(capi.PIX_UYVY, 64, 48, 2 * 64 + 5)[0]
    assert b2 == (H - 1) * 2 * ((W + 1) // 2) + 2 * ((W + 1) // 2) and f1 == 47 * 133 + 128
    for base2, overlaps in ((0x200000 - b2 + 1, True), (0x200000 - b2, False), (0x200000 + f1 - 1, True), (0x200000 + f1, False)):
        o = out()
        o[0].data2 = base2
        if overlaps:
            assert call(frames(pitch=2 * 64 + 5), o) == capi.ERR_ARG and b"overlaps frame 1" in L.stitch_last_error(), base2
        elif not torch.cuda.is_available():
            assert call(frames(pitch=2 * 64 + 5), o) == capi.ERR_NO_DEVICE, base2
    # the other way round: NV21 and NV16 frames need their second plane
    for fmt in (capi.PIX_NV21, capi.PIX_NV16):
        rig.set_formats(fmt, capi.PIX_YUYV)
        fr = frames(fmt)
        fr[2].data2 = None
        assert call(fr, out(capi.PIX_YUYV)) == capi.ERR_ARG and b"null plane" in L.stitch_last_error()
        assert call(frames(fmt, pitch2=63), out(capi.PIX_YUYV)) == capi.ERR_ARG and b"pitch" in L.stitch_last_error()
        assert call(frames(fmt), out(capi.PIX_YUYV, pitch=4 * ((W + 1) // 2) - 1)) == capi.ERR_ARG
    assert status[0] == 77 and rig.step_plan(0) is None
    rig.close()


def test_input_form_refusals_and_none_before_any_replay(st):
    capi = st.capi
    L = capi.lib()
    rig = capi.Rig.from_steps(ref.SMALL, 0, ref.small_steps(capi))
    form = C.c_int(77)
    for fmts in ((0, 0), (capi.PIX_YUYV, capi.PIX_NV16), (capi.PIX_BGR24, 0)):
        rig.set_formats(*fmts)
        assert [rig.input_form(f) for f in range(rig.n_frames)] == [capi.RIG_INPUT_NONE] * 3
    assert L.stitch_rig_input_form(rig._h, 0, C.byref(form)) == 0 and form.value == 0
    form.value = 77
    for args in ((None, 0, C.byref(form)), (rig._h, 0, None), (rig._h, -1, C.byref(form)), (rig._h, 3, C.byref(form)), (rig._h, 2 ** 31 - 1, C.byref(form))):
        assert L.stitch_rig_input_form(*args) == capi.ERR_ARG and b"rig_input_form" in L.stitch_last_error()
    assert form.value == 77
    with pytest.raises(capi.StitchError) as e:
        rig.input_form(3)
    assert e.value.code == capi.ERR_ARG and rig.step_plan(0) is None
    rig.close()
