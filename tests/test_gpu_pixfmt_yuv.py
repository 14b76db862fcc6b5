"""GPU: the conversions of include/stitch_rig_formats_yuv.h on their own (csrc/k_rig_formats.inc: k_unpack_many, k_pack_many for YUYV,
UYVY, NV21 and NV16) against tests/pixfmt_yuv_ref.py.  Everything is exact.  Sizes 1 x 1, 2 x 3, 3 x 2 (an odd width: the clamped
group and its Y1 byte), 67 x 5, 50 x 37 and 64 x 48 (the wide form); the three matrices; pitches tight, tight + 5 (nothing aligned:
the byte form) and rounded up to 16 plus 16; a base one byte off; 1 and 3 images per call.  Outputs go into buffers of 0xEE and are
compared whole: padding must come back untouched.  The decode and the encode are the functions tests/test_gpu_pixfmt.py sweeps over
every colour; what is new here is byte position and chroma averaging."""
import numpy as np
import pytest

import pixfmt_yuv_ref as yf
from computervisionimagestich2_amd import capi
from test_gpu_pixfmt import from_dev, same_image, to_dev
from test_pixfmt_yuv_host import pitches

pytestmark = pytest.mark.gpu

SIZES = [(1, 1), (2, 3), (3, 2), (67, 5), (50, 37), (64, 48)]


def random_image(rng, fmt, w, h, pitch, pitch2):
    b1, b2 = yf.image_bytes(fmt, w, h, pitch, pitch2)
    return dict(fmt=fmt, w=w, h=h, data=rng.integers(0, 256, b1, dtype=np.uint8), data2=rng.integers(0, 256, b2, dtype=np.uint8) if b2 else None, pitch=pitch,
                pitch2=pitch2)


@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("fmt", yf.NEW, ids=["yuyv", "uyvy", "nv21", "nv16"])
def test_unpack_and_pack_against_the_reference(st, gpu, fmt, size):
    import torch
    w, h = size
    rng = np.random.default_rng(1000 * fmt + w)
    wide = 0
    for matrix in (0, 1, 2):
        for pitch, pitch2 in pitches(fmt, w):
            for offset in (0, 1):
                for count in (1, 3):
                    # ---- to planar ----
                    ims = [random_image(rng, fmt, w, h, pitch, pitch2) for _ in range(count)]
                    got = capi.dev_unpack_many([to_dev(im, gpu, offset) for im in ims], matrix)
                    for i in range(count):
                        assert np.array_equal(got[i].cpu().numpy(), yf.unpack(ims[i], matrix)), ("unpack", matrix, pitch, offset, count, i)
                    # ---- from planar, into buffers of 0xEE ----
                    planar = [rng.integers(0, 256, (3, h, w), dtype=np.uint8) for _ in range(count)]
                    blank = dict(ims[0], data=np.full_like(ims[0]["data"], 0xEE), data2=None if ims[0]["data2"] is None else np.full_like(ims[0]["data2"], 0xEE))
                    outs = capi.dev_pack_many([torch.from_numpy(p).to(gpu) for p in planar], fmt, matrix, out=[to_dev(blank, gpu, offset) for _ in range(count)])
                    for i in range(count):
                        want = yf.pack(planar[i], fmt, matrix, pitch, pitch2, fill=0xEE)
                        assert same_image(from_dev(outs[i]), want), ("pack", matrix, pitch, offset, count, i)
                    wide += offset == 0 and pitch % 4 == 0 and pitch2 % 4 == 0 and w % 4 == 0
    assert wide or w % 4  # 64 x 48 took the wide form at the tight and the rounded pitch
    # fresh outputs are allocated by image_bytes at tight pitch
    fresh = capi.dev_pack_many([torch.from_numpy(planar[0]).to(gpu)], fmt, 1)[0]
    assert (fresh.pitch, fresh.pitch2) == yf.tight(fmt, w) and (fresh.data.numel(), 0 if fresh.data2 is None else fresh.data2.numel()) == yf.image_bytes(fmt, w, h)
    assert same_image(from_dev(fresh), yf.pack(planar[0], fmt, 1))


def test_the_y1_byte_of_an_odd_width_is_ignored_on_input(st, gpu):
    rng = np.random.default_rng(7)
    for fmt in (yf.YUYV, yf.UYVY):
        im = random_image(rng, fmt, 3, 2, 13, 0)
        other = dict(im, data=im["data"].copy())
        y1 = 4 + yf.GROUP[fmt][2]
        other["data"][[y1, 13 + y1]] ^= 0xFF
        a, b = capi.dev_unpack_many([to_dev(im, gpu), to_dev(other, gpu)], 0)
        assert bool((a == b).all()) and np.array_equal(a.cpu().numpy(), yf.unpack(im, 0))


def test_argument_errors(st, gpu):
    import torch
    with pytest.raises(ValueError):
        capi.dev_unpack_many([capi.Image.empty(capi.PIX_YUYV, 8, 6, gpu), capi.Image.empty(capi.PIX_UYVY, 8, 6, gpu)])
    with pytest.raises(ValueError):  # a chroma plane shorter than image_bytes says: NV16 has h rows of it
        capi.Image(capi.PIX_NV16, 8, 6, torch.empty(48, dtype=torch.uint8, device=gpu), torch.empty(24, dtype=torch.uint8, device=gpu))
    with pytest.raises(capi.StitchError):
        capi.Image.empty(capi.PIX_UYVY, 7, 6, gpu, pitch=15)
    with pytest.raises(capi.StitchError) as e:
        capi.dev_unpack_many([capi.Image.empty(capi.PIX_NV21, 8, 6, gpu)], matrix=3)
    assert e.value.code == capi.ERR_ARG
