"""GPU: the l-alpha-beta colour transfer (k_tr_to_lab / k_tr_stats / k_tr_apply, csrc/k_formats.inc) against what the
REFERENCE's transfer.cpp produced, replayed from tests/golden/transfer.npz (tests/golden/make_transfer_goldens.py; the
cases and what each is there for: tests/transfer_cases.py).  No tolerance anywhere:

  * output bytes and the bits of the twelve statistics equal the recorded specified-function result (the kernels evaluate
    include/stitch_elem.h, whose logarithm is the correctly rounded one);
  * with the recorded differing bytes replaced -- 18 of 1.06e8 over all cases, each by one grey level, where glibc's logf
    is not correctly rounded -- the output IS the reference's, by SHA-256 and in full where the recording stores it.

Every entry point: stitch_transfer_u8 (host pointers), stitch_dev_transfer_u8 out of place and in place (out = src), and
the C++ adaptor's `transfer` class.  The every-colour case (4096 x 4096, source and template) puts every possible input of
k_tr_to_lab against the reference and drives k_tr_stats' float running sums through 2^24 samples per chain."""
import hashlib
import json
import os
import subprocess
import sys
import time

import numpy as np
import pytest

import transfer_cases as T

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
DROPIN = os.path.join(os.path.dirname(HERE), "oracle", "_ref", "libstitch_dropin.so")


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


@pytest.fixture(scope="module")
def rec():
    r = T.Recording()
    assert list(r.cases) == T.CASE_NAMES
    return r


@pytest.fixture(scope="module")
def images(rec, oracle):
    """case name -> (src, tem), built once and never written to"""
    cache = {}

    def get(name):
        if name not in cache:
            src, tem = rec.images(name, oracle)
            c = rec.cases[name]
            assert sha(src) == c["src_sha256"] and sha(tem) == c["tem_sha256"], name
            src.setflags(write=False)
            tem.setflags(write=False)
            cache[name] = (src, tem)
        return cache[name]
    return get


def check(rec, name, out, stats, what):
    c = rec.cases[name]
    assert list(out.shape) == c["shape"], (what, name)
    if stats is not None:
        assert [int(v) for v in np.ascontiguousarray(stats, np.float32).view(np.uint32)] == c["spec_stats_bits"], (what, name, stats)
    assert sha(out) == c["spec_sha256"], (what, name)
    as_ref = rec.as_reference(name, out)
    assert sha(as_ref) == c["ref_sha256"], (what, name)
    full = rec.ref_out(name)
    if full is not None:
        assert np.array_equal(as_ref, full), (what, name)


@pytest.mark.parametrize("name", T.CASE_NAMES)
def test_host_pointers(st, gpu, rec, images, name):
    from computervisionimagestich2_amd import capi
    src, tem = images(name)
    t0 = time.perf_counter()
    out, stats = capi.transfer(src, tem)
    print(f"stitch_transfer_u8 {name}: {time.perf_counter() - t0:.3f} s")
    check(rec, name, out, stats, "host")


@pytest.mark.parametrize("name", T.CASE_NAMES)
def test_device_resident(st, gpu, rec, images, name):
    import torch
    from computervisionimagestich2_amd import capi
    src, tem = images(name)
    d_src, d_tem = torch.from_numpy(src.copy()).to(gpu), torch.from_numpy(tem.copy()).to(gpu)
    d_stats = torch.zeros(12, dtype=torch.float32, device=gpu)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    d_out = capi.dev_transfer(d_src, d_tem, stats=d_stats)
    torch.cuda.synchronize()
    print(f"stitch_dev_transfer_u8 {name}: {time.perf_counter() - t0:.3f} s")
    assert np.array_equal(d_src.cpu().numpy(), src) and np.array_equal(d_tem.cpu().numpy(), tem)  # inputs untouched
    check(rec, name, d_out.cpu().numpy(), d_stats.cpu().numpy(), "device")
    # in place: the output aliases the source, as ImageProcess.cpp:180 would call it
    d_stats.zero_()
    back = capi.dev_transfer(d_src, d_tem, out=d_src, stats=d_stats)
    assert back.data_ptr() == d_src.data_ptr()
    check(rec, name, d_src.cpu().numpy(), d_stats.cpu().numpy(), "device, in place")


ADAPTOR_SCRIPT = r'''
import ctypes as C, json, sys
import numpy as np
dropin = C.CDLL(sys.argv[1], mode=C.RTLD_GLOBAL)
src, tem = np.load(sys.argv[2]), np.load(sys.argv[3])
got = np.ascontiguousarray(src).copy()
rc = dropin.stitch_dropin_transfer_in_place(got.ctypes.data_as(C.c_void_p), src.shape[2], src.shape[1], tem.ctypes.data_as(C.c_void_p), tem.shape[2], tem.shape[1])
np.save(sys.argv[4], got)
print("RESULT " + json.dumps({"rc": rc, "calls": dropin.stitch_dropin_call_count(6)}))
'''


def test_adaptor_transfer_class(rec, images, tmp_path):
    """The reference's `transfer` class as the C++ adaptor defines it (adaptor/cimg_dropin.cpp), constructed as
    ImageProcess.cpp:180 would -- output aliasing the source -- in a fresh interpreter without torch, on the committed
    frames 3 -> 4 (the case with a recorded differing byte)."""
    assert os.path.exists(DROPIN), f"drop-in adaptor missing (built by `make -C oracle ref` next to the reference): {DROPIN}"
    name = "frames_3_4"
    src, tem = images(name)
    np.save(tmp_path / "src.npy", src)
    np.save(tmp_path / "tem.npy", tem)
    out = subprocess.run([sys.executable, "-c", ADAPTOR_SCRIPT, DROPIN, str(tmp_path / "src.npy"), str(tmp_path / "tem.npy"), str(tmp_path / "out.npy")],
                         capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    r = json.loads([l for l in out.stdout.splitlines() if l.startswith("RESULT ")][-1][7:])
    assert r == {"rc": 0, "calls": 1}, r
    assert rec.cases[name]["differing_bytes"] == 1
    check(rec, name, np.load(tmp_path / "out.npy"), None, "adaptor")
