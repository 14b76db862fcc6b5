"""CPU: the host side of a rig's camera layouts (include/stitch_rig_formats.h) -- the header compiles as C99, the binding's table
RIG_FORMAT_SIGNATURES states exactly what it declares and shares no name with the other tables, the stitch_image mirror has the
compiler's offsets; tests/pixfmt_ref.py obeys the identities the header promises; stitch_image_bytes answers and refuses as the header
says; stitch_rig_set_formats refuses every bad value and leaves the rig as it was, stitch_rig_clear_formats restores (0, 0); the old
replay calls refuse a formatted rig, and every argument error of the new calls is reported, before a device is needed."""
import ctypes as C
import os
import re
import shlex
import subprocess

import numpy as np
import pytest

import pixfmt_ref as pf
import rig_seams_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "stitch_rig_formats.h")

FUNCTIONS = ("stitch_image_bytes", "stitch_dev_unpack_many_u8", "stitch_dev_pack_many_u8", "stitch_rig_set_formats", "stitch_rig_formats",
             "stitch_rig_clear_formats", "stitch_dev_rig_stitch_fmt_u8")
NAMES = ("PLANAR", "RGB24", "BGR24", "RGBX32", "BGRX32", "NV12")


def _header_text():
    return re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)


SCALARS = {"int": C.c_int, "int32_t": C.c_int, "float": C.c_float, "double": C.c_double, "size_t": C.c_size_t}
RETURNS = {"int": C.c_int, "void": None}


def _declared():
    """{name: (restype, argtypes)} of every prototype, by the binding's rules (tests/test_capi_abi.py, tests/test_rig_crop_host.py)."""
    sigs = {}
    for ret, name, params in re.findall(r"((?:const\s+)?\w+\s*\*?)\s*\b(stitch_\w+)\s*\(([^()]*)\)\s*;", _header_text()):
        prms = [] if params.strip() == "void" else [" ".join(p.split()) for p in params.split(",")]
        args = [C.c_void_p if ("*" in p or "[" in p) else SCALARS[" ".join(p.split()[:-1])] for p in prms]
        sigs[name] = (RETURNS[" ".join(ret.replace("*", " *").split())], args)
    return sigs


def test_signature_table_states_the_header(st):
    capi = st.capi
    want, lib = _declared(), capi.lib()
    assert sorted(want) == sorted(FUNCTIONS) == sorted(set(re.findall(r"\b(stitch_[a-z0-9_]+)\s*\(", _header_text())))
    assert sorted(capi.RIG_FORMAT_SIGNATURES) == sorted(want)
    others = set(capi.SIGNATURES) | set(capi.PANORAMA_SIGNATURES) | set(capi.RIG_SIGNATURES) | set(capi.EXPOSURE_SIGNATURES) \
        | set(capi.RIG_EXPOSURE_SIGNATURES) | set(capi.CALIBRATE_SIGNATURES) | set(capi.RIG_SEAMS_SIGNATURES) | set(capi.COLLAPSE_SIDES_SIGNATURES) \
        | set(capi.SRC_RUNS_SIGNATURES) | set(capi.RIG_CROP_SIGNATURES)
    assert not set(capi.RIG_FORMAT_SIGNATURES) & others
    bound = {n: (getattr(lib, n).restype, getattr(lib, n).argtypes) for n in want}  # every name is exported
    wrong = {n: (bound[n], want[n]) for n in sorted(want) if bound[n] != tuple(want[n])}
    assert not wrong, f"(bound, declared) signatures differ for: {wrong}"
    assert lib.stitch_abi_version() == 5
    # the constants: the header's, the binding's and the reference's
    defined = dict(re.findall(r"#define\s+STITCH_PIX_(\w+)\s+(\d+)", _header_text()))
    assert {k: int(v) for k, v in defined.items()} == {n: i for i, n in enumerate(NAMES)}
    assert [getattr(capi, "PIX_" + n) for n in NAMES] == [getattr(pf, n) for n in NAMES] == list(range(6))


def test_header_is_c99_and_the_mirror_has_its_offsets(st, tmp_path):
    capi = st.capi
    cc = shlex.split(os.environ.get("CC", "cc")) + ["-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include")]
    fields = [f[0] for f in capi.ImageDesc._fields_]
    assert fields == ["data", "data2", "width", "height", "pitch", "pitch2"]
    src = tmp_path / "uses.c"
    src.write_text("\n".join(['#include <stdio.h>', '#include "stitch_rig_formats.h"', "int main(void) {"] + [f"    (void)(&{n});" for n in FUNCTIONS]
                             + [f"    (void)(STITCH_PIX_{n});" for n in NAMES]
                             + ['    printf("%zu", sizeof(stitch_image));']
                             + [f'    printf(" %zu", offsetof(stitch_image, {f}));' for f in fields] + ['    return 0;', "}", ""]))
    exe = tmp_path / "uses"
    r = subprocess.run(cc + ["-c", str(src), "-o", str(tmp_path / "uses.o")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    # (taking the functions' addresses needs the library at link time: print the layout from a second unit without them)
    lay = tmp_path / "layout.c"
    lay.write_text("\n".join(['#include <stdio.h>', '#include "stitch_rig_formats.h"', "int main(void) {", '    printf("%zu", sizeof(stitch_image));']
                             + [f'    printf(" %zu", offsetof(stitch_image, {f}));' for f in fields] + ['    return 0;', "}", ""]))
    r = subprocess.run(cc + [str(lay), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    got = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert got == [C.sizeof(capi.ImageDesc)] + [getattr(capi.ImageDesc, f).offset for f in fields]


# ---- the reference itself -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", pf.PACKED)
def test_ref_pack_then_unpack_is_the_identity(fmt):
    rng = np.random.default_rng(fmt)
    for (w, h), extra in (((1, 1), 0), ((7, 5), 0), ((7, 5), 5), ((16, 3), 16)):
        planar = rng.integers(0, 256, (3, h, w), dtype=np.uint8)
        im = pf.pack(planar, fmt, pitch=pf.tight(fmt, w)[0] + extra)
        assert len(im["data"]) == pf.image_bytes(fmt, w, h, im["pitch"])[0] and im["data2"] is None
        assert (pf.unpack(im) == planar).all()
        if pf.BPP[fmt] == 4:
            assert (np.stack([im["data"][y * im["pitch"]:][3:4 * w:4] for y in range(h)]) == 255).all()
        pad = np.concatenate([im["data"][y * im["pitch"] + pf.BPP[fmt] * w:(y + 1) * im["pitch"]] for y in range(h - 1)] + [np.zeros(0, np.uint8)])
        assert (pad == 0xEE).all() and pad.size == (h - 1) * extra


@pytest.mark.parametrize("matrix", [0, 1, 2])
def test_ref_grey_has_neutral_chroma_and_everything_fits_int32(matrix):
    g = np.arange(256)
    Y, Cb, Cr = pf.encode(g, g, g, matrix)
    assert (Cb == 128).all() and (Cr == 128).all()
    assert sum(pf.ENCODE[matrix][3:6] * np.array([-1, -1, 1])) == 0 == sum(pf.ENCODE[matrix][6:9] * np.array([1, -1, -1]))
    assert np.all(np.diff(Y.astype(int)) >= 0) and (Y[0], Y[255]) == ((16, 235) if matrix < 2 else (0, 255))
    # the extremes: every corner of the two input cubes (the forms are linear, so their extremes lie there)
    track = [0, 0]
    c = np.array([0, 255])
    a, b, d = (v.reshape(-1) for v in np.meshgrid(c, c, c, indexing="ij"))
    pf.decode(a, b, d, matrix, track)
    pf.encode(a, b, d, matrix, track)
    assert -2 ** 31 <= track[0] < 0 < track[1] < 2 ** 31
    # a 2 x 2 grid of a clamped odd image: the last column and row count twice
    c = np.array([[0, 1, 2], [4, 8, 16], [32, 64, 128]], np.uint8)
    assert pf.chroma_down(c).tolist() == [[(0 + 1 + 4 + 8 + 2) >> 2, (2 + 2 + 16 + 16 + 2) >> 2], [(32 + 64 + 32 + 64 + 2) >> 2, 128]]


def test_ref_nv12_roundtrip_of_grey_and_layout():
    planar = np.broadcast_to(np.arange(15, dtype=np.uint8).reshape(3, 5)[None] * 17, (3, 3, 5)).copy()
    for matrix in (0, 1, 2):
        im = pf.pack(planar, pf.NV12, matrix, pitch=9, pitch2=8)
        assert (len(im["data"]), len(im["data2"])) == (2 * 9 + 5, 1 * 8 + 6) == pf.image_bytes(pf.NV12, 5, 3, 9, 8)
        assert (im["data2"][[0, 1, 2, 3, 4, 5, 8, 9, 10, 11, 12, 13]] == 128).all() and (im["data2"][6:8] == 0xEE).all()
        back = pf.unpack(im, matrix)
        assert np.abs(back.astype(int) - planar).max() <= 2 and (back[0] == back[1]).all() and (back[1] == back[2]).all()


# ---- the library's host side ----------------------------------------------------------------------------------------------------
def test_image_bytes_answers_and_refusals(st):
    capi = st.capi
    L = capi.lib()
    for fmt in range(6):
        for w, h in ((1, 1), (2, 3), (67, 5), (50, 37), (4096, 4096)):
            t = pf.tight(fmt, w)
            for pitch, pitch2 in (t, (t[0] + 5, t[1] + 3), (-(-t[0] // 16) * 16 + 16, -(-t[1] // 16) * 16)):
                assert capi.image_bytes(fmt, w, h, pitch, pitch2) == pf.image_bytes(fmt, w, h, pitch, pitch2), (fmt, w, h, pitch, pitch2)
            assert capi.image_bytes(fmt, w, h) == pf.image_bytes(fmt, w, h)
    b = (C.c_size_t * 2)(7, 7)
    bad = [(-1, 4, 4, 64, 64), (6, 4, 4, 64, 64), (1, 0, 4, 64, 64), (1, 4, 0, 64, 64), (1, -4, 4, 64, 64), (1, 4, 4, 11, 0), (2, 4, 4, 11, 0), (3, 4, 4, 15, 0),
           (4, 4, 4, 15, 0), (5, 4, 4, 3, 4), (5, 4, 4, 4, 3), (5, 5, 4, 5, 5), (1, 4, 4, -12, 0)]
    for args in bad:
        assert L.stitch_image_bytes(*args, C.byref(b, 0), C.byref(b, C.sizeof(C.c_size_t))) == capi.ERR_ARG, args
        assert b"image_bytes" in L.stitch_last_error() and list(b) == [7, 7]
        assert pf.image_bytes(*args) is None
    assert L.stitch_image_bytes(5, 5, 4, 5, 6, None, None) == 0  # outputs are optional; NV12's smallest pitches
    assert L.stitch_image_bytes(0, 4, 4, -1, -1, None, None) == 0  # planar ignores its pitches
    with pytest.raises(capi.StitchError):
        capi.image_bytes(capi.PIX_RGB24, 4, 4, 11)


def _formats(capi, rig):
    v = [C.c_int(-1) for _ in range(3)]
    assert capi.lib().stitch_rig_formats(rig._h, *[C.byref(x) for x in v]) == 0
    return tuple(x.value for x in v)


def test_set_formats_checks_and_clear_formats_restores(st):
    capi = st.capi
    L = capi.lib()
    rig = capi.Rig.from_steps(ref.SMALL, 0, ref.small_steps(capi))
    assert _formats(capi, rig) == (0, 0, 0) == rig.formats
    bad = [(-1, 0, 0), (6, 0, 0), (0, -1, 0), (0, 6, 0), (1, 1, -1), (1, 1, 3), (5, 5, 3), (2 ** 31 - 1, 0, 0)]
    for before in (None, (capi.PIX_BGR24, capi.PIX_NV12, 2)):
        if before:
            assert rig.set_formats(*before) is rig
        kept = _formats(capi, rig)
        assert kept == (before or (0, 0, 0)) == rig.formats
        for args in bad:
            assert L.stitch_rig_set_formats(rig._h, *args) == capi.ERR_ARG, args
            assert b"rig_set_formats" in L.stitch_last_error() and _formats(capi, rig) == kept
        assert L.stitch_rig_set_formats(None, 1, 1, 0) == capi.ERR_ARG and _formats(capi, rig) == kept
        with pytest.raises(capi.StitchError) as e:
            rig.set_formats(1, 9)
        assert e.value.code == capi.ERR_ARG and _formats(capi, rig) == kept
    for i in range(6):
        for o in range(6):
            assert rig.set_formats(i, o, (i + o) % 3).formats == (i, o, (i + o) % 3)
    assert rig.clear_formats() is rig and _formats(capi, rig) == (0, 0, 0)
    assert rig.clear_formats().formats == (0, 0, 0)  # clearing twice is fine
    assert L.stitch_rig_formats(rig._h, None, None, None) == 0
    assert L.stitch_rig_formats(None, None, None, None) == L.stitch_rig_clear_formats(None) == capi.ERR_ARG
    assert rig.step_plan(0) is None and rig.crop[1] == 0  # no device was touched, nothing else changed
    rig.close()


def test_the_old_calls_refuse_a_formatted_rig_before_a_device(st):
    capi = st.capi
    L = capi.lib()
    rig = capi.Rig.from_steps(ref.SMALL, 0, ref.small_steps(capi))
    ex = capi.Rig.from_steps(ref.SMALL, 0, [dict(s, mosaic_src=0) for s in ref.small_steps(capi)][:1], exposure=1)
    frames = (capi.FrameU8 * 3)(*[capi.FrameU8(0x10000 * (i + 1), 64, 48) for i in range(3)])
    outs, status = (C.c_void_p * 1)(0x900000), (C.c_int32 * 1)(77)
    stats = (C.c_float * 24)()
    for fmts in ((1, 0), (0, 5), (3, 4)):
        rig.set_formats(*fmts)
        ex.set_formats(*fmts)
        assert L.stitch_dev_rig_stitch_u8(rig._h, frames, 1, outs, status, None, None) == capi.ERR_ARG
        assert b"stitch_dev_rig_stitch_fmt_u8" in L.stitch_last_error()
        assert L.stitch_dev_rig_stitch_exposure_u8(ex._h, frames, 1, outs, status, None, stats, None) == capi.ERR_ARG
        assert b"stitch_dev_rig_stitch_fmt_u8" in L.stitch_last_error()
    assert status[0] == 77 and rig.step_plan(0) is None
    rig.close()
    ex.close()


def _desc(capi, fmt, w, h, base=0x100000, pitch=None, pitch2=None, base2=0x800000):
    t = pf.tight(fmt, w)
    return capi.ImageDesc(base, base2 if fmt == pf.NV12 else None, w, h, t[0] if pitch is None else pitch, t[1] if pitch2 is None else pitch2)


def test_argument_errors_of_the_new_calls_come_before_a_device(st):
    import torch
    capi = st.capi
    L = capi.lib()
    planar = (C.c_void_p * 2)(0x4000000, 0x5000000)
    for call, who in ((lambda fmt, m, im, n: L.stitch_dev_unpack_many_u8(fmt, m, im, planar, n, None), b"unpack_many"),
                      (lambda fmt, m, im, n: L.stitch_dev_pack_many_u8(fmt, m, planar, im, n, None), b"pack_many")):
        two = lambda fmt, **kw: (capi.ImageDesc * 2)(_desc(capi, fmt, 8, 6), _desc(capi, fmt, 8, 6, base=0x200000, base2=0x900000, **kw))  # noqa: E731
        for fmt in (0, -1, 6):
            assert call(fmt, 0, two(1), 2) == capi.ERR_ARG and who in L.stitch_last_error()
        for matrix in (-1, 3):
            assert call(5, matrix, two(5), 2) == capi.ERR_ARG
        for n in (0, -1, 65536):
            assert call(1, 0, two(1), n) == capi.ERR_ARG
        assert call(1, 0, None, 2) == capi.ERR_ARG
        assert call(1, 0, two(1, pitch=23), 2) == capi.ERR_ARG and call(5, 0, two(5, pitch2=7), 2) == capi.ERR_ARG and call(5, 0, two(5, pitch=7), 2) == capi.ERR_ARG
        bad = two(5)
        bad[1].data2 = None
        assert call(5, 0, bad, 2) == capi.ERR_ARG
        bad = two(3)
        bad[1].width = 9
        assert call(3, 0, bad, 2) == capi.ERR_ARG
        bad = two(3)
        bad[0].height = 0
        assert call(3, 0, bad, 2) == capi.ERR_ARG
        if not torch.cuda.is_available():
            assert call(1, 0, two(1), 2) == capi.ERR_NO_DEVICE
    assert L.stitch_dev_unpack_many_u8(1, 0, two(1), None, 2, None) == capi.ERR_ARG
    holes = (C.c_void_p * 2)(0x4000000, None)
    assert L.stitch_dev_unpack_many_u8(1, 0, two(1), holes, 2, None) == capi.ERR_ARG

    # ---- the replay -----
    rig = capi.Rig.from_steps(ref.SMALL, 0, ref.small_steps(capi)).set_formats(capi.PIX_BGR24, capi.PIX_NV12)
    W, H = rig.width, rig.height

    def frames(**kw):
        return (capi.ImageDesc * 3)(*[_desc(capi, capi.PIX_BGR24, 64, 48, base=0x100000 * (i + 1), **kw) for i in range(3)])

    def out(**kw):
        return (capi.ImageDesc * 1)(_desc(capi, capi.PIX_NV12, kw.pop("w", W), kw.pop("h", H), base=0x4000000, base2=0x6000000, **kw))

    status = (C.c_int32 * 1)(77)
    stats = (C.c_float * 24)()
    call = lambda fr, o, n=1, st_=None: L.stitch_dev_rig_stitch_fmt_u8(rig._h, fr, n, o, status, None, st_, None)  # noqa: E731
    assert L.stitch_dev_rig_stitch_fmt_u8(None, frames(), 1, out(), status, None, None, None) == capi.ERR_ARG
    assert call(None, out()) == call(frames(), None) == call(frames(), out(), 0) == capi.ERR_ARG
    assert L.stitch_dev_rig_stitch_fmt_u8(rig._h, frames(), 1, out(), None, None, None, None) == capi.ERR_ARG
    assert call(frames(), out(), 1, stats) == capi.ERR_ARG and b"statistics" in L.stitch_last_error()
    assert call(frames(pitch=3 * 64 - 1), out()) == capi.ERR_ARG and b"pitch" in L.stitch_last_error()  # a wrong pitch, either side
    assert call(frames(), out(pitch=W - 1)) == capi.ERR_ARG and call(frames(), out(pitch2=2 * ((W + 1) // 2) - 1)) == capi.ERR_ARG
    assert call(frames(), out(w=W - 1)) == capi.ERR_ARG and call(frames(), out(h=H + 1)) == capi.ERR_ARG
    fr = frames()
    fr[1].width = 63
    assert call(fr, out()) == capi.ERR_ARG
    fr = frames()
    fr[2].data = None
    assert call(fr, out()) == capi.ERR_ARG
    o = out()
    o[0].data2 = None
    assert call(frames(), o) == capi.ERR_ARG
    # overlap is judged by stitch_image_bytes, plane by plane: the chroma plane's last byte on a frame's first, then one clear of it
    b1, b2 = capi.image_bytes(capi.PIX_NV12, W, H)
    f1 = capi.image_bytes(capi.PIX_BGR24, 64, 48, 3 * 64 + 5)[0]
    # (frame 1 lies at 0x200000; with a device a call that passes would run on these made-up addresses, so those are made without one only)
    for base2, overlaps in ((0x200000 - b2 + 1, True), (0x200000 - b2, False), (0x200000 + f1 - 1, True), (0x200000 + f1, False)):
        o = out()
        o[0].data2 = base2
        if overlaps:
            assert call(frames(pitch=3 * 64 + 5), o) == capi.ERR_ARG and b"overlaps frame 1" in L.stitch_last_error(), base2
        elif not torch.cuda.is_available():
            assert call(frames(pitch=3 * 64 + 5), o) == capi.ERR_NO_DEVICE, base2
    o = (capi.ImageDesc * 2)(out()[0], out()[0])
    o[1].data = 0x4000000 + b1 - 1  # two outputs: the second one's Y plane starts on the first one's last byte
    o[1].data2 = 0x7000000
    two_sets = (capi.ImageDesc * 6)(*(list(frames()) + list(frames())))
    assert call(two_sets, o, 2) == capi.ERR_ARG and b"outputs of sets 0 and 1 overlap" in L.stitch_last_error()
    assert status[0] == 77 and rig.step_plan(0) is None
    rig.close()
