"""GPU: exposure-matched panoramas (include/stitch_exposure.h, csrc/k_exposure.inc, csrc/stitch_exposure.inc).  No tolerance
anywhere.

  * capi.dev_running_stats, forms 1 (one workgroup's scan) and 2 (spans + walk), against form 0 (the serial walk of k_tr_stats)
    bit for bit: the crafted series of tests/exposure_series.py (the arrays the CPU test uses, uploaded), lengths around the
    wavefront's staging block, the tile and the span, six planes of different lengths in one call, a stream of the caller's.
  * capi.dev_transfer(stats_form = 1, 2) on every case of tests/transfer_cases.py against the recorded statistics and output
    hashes of tests/golden/transfer.npz, out of place and in place; keep_black on `black_rows`.
  * The fast path on real planes, from the device's counters: at most 1 % plain float adds, no tile finished serially.
  * The chain: runs "2" and "4", modes 1 and 2, both keep_black values, through capi.dev_panorama(exposure=...) against
    tests/golden/exposure.json (CPU restatements alone); the host and from-features entry points and
    pipeline.panorama_from_frames(exposure=...) against it byte for byte; mode 0 through the new entry point against the chain
    as it is; chains.json's `dense4` (frames warped more than once) in mode 1, C chain against Python chain; refusals."""
import ctypes as C
import hashlib
import json
import os

import numpy as np
import pytest

import chain_sets
import exposure_series as XS
import transfer_cases as T
from computervisionimagestich2_amd import bmp, capi, pipeline

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
_cache = {}


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def tsha(t):
    return sha(t.cpu().numpy())


def bits(t):
    a = t.cpu().numpy() if hasattr(t, "cpu") else np.asarray(t)
    return [int(v) for v in np.ascontiguousarray(a, np.float32).reshape(-1).view(np.uint32)]


# ---- the running sums ------------------------------------------------------------------------------------------------------------
def _is_nan(b):
    return (b & 0x7fffffff) > 0x7f800000


def same(a, b):
    """Two results' bit patterns are the same -- or both are NaN.  IEEE 754 leaves a NaN's sign open, and on this ISA it follows
    from operand order and source modifiers, which the compiler chooses per kernel: k_tr_stats forms x - mean with v_sub_f32,
    k_ex_walk with v_subrev_f32, and on the plane with one NaN sample the serial form's sd is 0x7fc00000 where the scan's is
    0xffc00000 (the mean is 0x7fc00000 in both).  No C++ source pins that bit; every result that is a number is held bit for bit."""
    return a == b or (_is_nan(a) and _is_nan(b))


@pytest.fixture(scope="module")
def series(gpu):
    import torch
    return {k: torch.from_numpy(np.array(v)).to(gpu) for k, v in XS.crafted().items()}


def _stats_in_groups(planes, form):
    """name -> (mean bits, sd bits), six planes per call"""
    names, out = list(planes), {}
    for i in range(0, len(names), 6):
        grp = names[i:i + 6]
        mean, sd = capi.dev_running_stats([planes[n] for n in grp], form=form)
        mb, sb = bits(mean), bits(sd)
        out.update({n: (mb[k], sb[k]) for k, n in enumerate(grp)})
    return out


@pytest.fixture(scope="module")
def serial(series):
    """form 0 on every crafted series: computed once, shared"""
    return _stats_in_groups(series, 0)


def test_the_serial_form_is_the_plain_loop(gpu, series, serial):
    """the yardstick itself, against numpy's sequential float32 cumsum on a few series"""
    for name in ("uniform_257", "ties_signed", "negative_sum"):
        x = series[name].cpu().numpy()
        mean = np.float32(np.cumsum(x, dtype=np.float32)[-1] / np.float32(x.size))
        sq = (x - mean) * (x - mean)
        sd = np.sqrt(np.float32(np.cumsum(sq, dtype=np.float32)[-1] / np.float32(x.size)))
        assert serial[name] == (bits(mean)[0], bits(sd)[0]), name


@pytest.mark.parametrize("form", [1, 2])
def test_crafted_series_bit_for_bit(gpu, series, serial, form):
    got = _stats_in_groups(series, form)
    wrong = {n: (got[n], serial[n]) for n in series if not (same(got[n][0], serial[n][0]) and same(got[n][1], serial[n][1]))}
    assert not wrong, wrong
    nans = [n for n in series if _is_nan(serial[n][0]) or _is_nan(serial[n][1])]
    assert sorted(nans) == ["one_inf", "one_nan"]  # `same` forgives nothing anywhere else


@pytest.mark.parametrize("form", [1, 2])
def test_lengths_and_six_planes_of_different_lengths(gpu, series, form):
    import torch
    base = series["zero_mean_normal"] * 0.25 + 1.5
    lens = [1, 255, 256, 257, XS.TILE - 1, XS.TILE + 1, XS.SPAN - 1, XS.SPAN + 1, XS.TILE, XS.SPAN, 2 * XS.SPAN + 1, 100000]
    for i in range(0, len(lens), 6):
        planes = [base[k:k + n].contiguous() for k, n in enumerate(lens[i:i + 6])]
        want = capi.dev_running_stats(planes, form=0)
        got = capi.dev_running_stats(planes, form=form, want_diag=True)
        assert bits(got[0]) == bits(want[0]) and bits(got[1]) == bits(want[1]), lens[i:i + 6]
        one = capi.dev_running_stats(planes[2:3], form=form)  # a plane alone gives what it gives among six
        assert bits(one[0])[0] == bits(want[0])[2] and bits(one[1])[0] == bits(want[1])[2]
    # counts of the caller's own: the divisor is not the length
    planes = [base[:5000].contiguous(), base[7:9000].contiguous()]
    want = capi.dev_running_stats(planes, form=0, counts=[4096.0, 12345.0])
    got = capi.dev_running_stats(planes, form=form, counts=[4096.0, 12345.0])
    assert bits(got[0]) == bits(want[0]) and bits(got[1]) == bits(want[1])
    assert bits(want[0]) != bits(capi.dev_running_stats(planes, form=0)[0])
    assert torch.isfinite(got[0]).all()


def test_a_stream_of_the_callers_own(gpu, series, serial):
    import torch
    names = ["alternating_sign", "uniform_16385", "ties_unsigned", "falls_out_downwards", "one_nan", "zeros_then_values"]
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        planes = [series[n].clone() for n in names]
        out = [capi.dev_running_stats(planes, form=f) for f in (2, 1, 2)]
    s.synchronize()
    for mean, sd in out:
        for n, m, d in zip(names, bits(mean), bits(sd)):
            assert same(m, serial[n][0]) and same(d, serial[n][1]), n


# ---- the transfer with its statistics by scan ------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def rec():
    r = T.Recording()
    assert list(r.cases) == T.CASE_NAMES
    return r


@pytest.fixture(scope="module")
def images(rec, oracle):
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


@pytest.mark.parametrize("form", [1, 2])
@pytest.mark.parametrize("name", T.CASE_NAMES)
def test_transfer_cases(gpu, rec, images, name, form):
    import torch
    src, tem = images(name)
    c = rec.cases[name]
    d_src, d_tem = torch.from_numpy(src.copy()).to(gpu), torch.from_numpy(tem.copy()).to(gpu)
    d_stats = torch.zeros(12, dtype=torch.float32, device=gpu)
    d_out = capi.dev_transfer(d_src, d_tem, stats=d_stats, stats_form=form)
    assert bits(d_stats) == c["spec_stats_bits"], (name, form)
    assert tsha(d_out) == c["spec_sha256"], (name, form)
    assert np.array_equal(d_src.cpu().numpy(), src)
    d_stats.zero_()
    back = capi.dev_transfer(d_src, d_tem, out=d_src, stats=d_stats, stats_form=form)  # in place, as ImageProcess.cpp:180 calls it
    assert back.data_ptr() == d_src.data_ptr()
    assert bits(d_stats) == c["spec_stats_bits"] and tsha(d_src) == c["spec_sha256"], (name, form, "in place")


@pytest.mark.parametrize("form", [0, 1, 2])
def test_keep_black(gpu, rec, images, form):
    """`black_rows`: three black rows at the top of the source.  They stay black; every other byte, and every statistic (they
    run over all pixels), is the recorded one."""
    import torch
    name = "black_rows"
    src, tem = images(name)
    c = rec.cases[name]
    black = (src == 0).all(axis=0)
    assert black[:3].all() and 0 < black.sum() < black.size
    d_src, d_tem = torch.from_numpy(src.copy()).to(gpu), torch.from_numpy(tem.copy()).to(gpu)
    d_stats = torch.zeros(12, dtype=torch.float32, device=gpu)
    plain_out = capi.dev_transfer(d_src, d_tem, stats_form=form).cpu().numpy()
    assert sha(plain_out) == c["spec_sha256"] and plain_out[:, black].any()  # the literal transfer paints them
    for out in (None, d_src):
        got = capi.dev_transfer(d_src, d_tem, out=out, stats=d_stats, stats_form=form, keep_black=True).cpu().numpy()
        assert bits(d_stats) == c["spec_stats_bits"]
        assert not got[:, black].any()
        assert np.array_equal(got[:, ~black], plain_out[:, ~black])


def test_fast_path_on_real_planes(gpu, rec, images):
    """From the device's counters, on the committed frames 1 and 2: at most 1 % of the samples are added by a plain float add and
    no tile finishes serially (both passes together, so 2 n samples per plane)."""
    import torch
    src, tem = images("frames_1_2")
    d_src, d_tem = torch.from_numpy(src.copy()).to(gpu), torch.from_numpy(tem.copy()).to(gpu)
    for form in (1, 2):
        diag = torch.full((6, 4), -1, dtype=torch.int32, device=gpu)
        d_stats = torch.zeros(12, dtype=torch.float32, device=gpu)
        capi.dev_transfer(d_src, d_tem, stats=d_stats, stats_form=form, diag=diag)
        assert bits(d_stats) == rec.cases["frames_1_2"]["spec_stats_bits"]
        d = diag.cpu().numpy()
        n = src.shape[1] * src.shape[2]
        print(f"form {form}: plain adds {d[:, 0].tolist()} of {2 * n} per plane; spans O(1) {d[:, 1].tolist()}, redone {d[:, 2].tolist()}, serial tiles {d[:, 3].tolist()}")
        assert (d[:, 0] >= 1).all() and (d[:, 0] <= 0.01 * 2 * n).all() and (d[:, 3] == 0).all()
        spans = 2 * -(-n // XS.SPAN)
        assert (d[:, 1] + d[:, 2] == (spans if form == 2 else 0)).all()
        if form == 2:
            assert (d[:, 1] > d[:, 2]).all()


# ---- the chain -------------------------------------------------------------------------------------------------------------------
RUNS = {"2": (1, 2), "4": (1, 2, 3, 4)}
CHAINS = [(run, mode, kb) for run in ("2", "4") for mode in (1, 2) for kb in (0, 1)]


def _host_frame(i):
    if ("bmp", i) not in _cache:
        _cache["bmp", i] = np.ascontiguousarray(bmp.load_bmp(os.path.join(GOLD, "input", f"{i}.bmp")))
    return _cache["bmp", i]


def _frames(ids, gpu):
    import torch
    return [torch.from_numpy(_host_frame(i)).to(gpu) for i in ids]


def _recorded(run, mode, kb):
    if "exposure" not in _cache:
        with open(os.path.join(GOLD, "exposure.json")) as f:
            _cache["exposure"] = json.load(f)
    return _cache["exposure"]["runs"][run][f"mode{mode}_keep_black{kb}"]


def _c_chain(run, mode, kb, gpu, form=2):
    key = ("c", run, mode, kb, form)
    if key not in _cache:
        _cache[key] = capi.dev_panorama(_frames(RUNS[run], gpu), return_steps=True, keep_steps=True,
                                        exposure=dict(mode=mode, keep_black=kb, stats_form=form))
    return _cache[key]


@pytest.mark.parametrize("run,mode,kb", CHAINS)
def test_recorded_chains(gpu, run, mode, kb):
    R = _recorded(run, mode, kb)
    final, steps = _c_chain(run, mode, kb, gpu)
    assert len(steps) == len(R["steps"])
    for got, ref in zip(steps, R["steps"]):
        assert (got["src"], got["mosaic_src"]) == (ref["src"], ref["mosaic_src"])
        assert bits(got["exposure_stats"]) == ref["stats_bits"], (run, mode, kb, ref["src"])
        assert tsha(got["transferred"]) == ref["transferred_sha256"]
        assert tsha(got["out"]) == ref["out_sha256"]
    assert list(final.shape) == R["final_shape"] and tsha(final) == R["final_sha256"]


@pytest.mark.parametrize("run,mode,kb", [("4", 1, 1), ("4", 2, 0), ("2", 2, 1)])
def test_every_form_and_entry_point_gives_the_same_bytes(gpu, run, mode, kb):
    final, steps = _c_chain(run, mode, kb, gpu)
    want = final.cpu().numpy().tobytes()
    ids = RUNS[run]
    for form in (0, 1):
        f2, s2 = _c_chain(run, mode, kb, gpu, form=form)
        assert f2.cpu().numpy().tobytes() == want
        assert [bits(s["exposure_stats"]) for s in s2] == [bits(s["exposure_stats"]) for s in steps]
    e = dict(mode=mode, keep_black=kb)
    got = capi.panorama([_host_frame(i) for i in ids], exposure=e)
    assert got.shape == tuple(final.shape) and got.tobytes() == want
    feats = []
    for i in ids:
        z = np.load(os.path.join(GOLD, f"match_frame{i}.npz"))
        import torch
        feats.append(tuple(torch.from_numpy(np.ascontiguousarray(z[k][z["map_idx"]])).to(gpu) for k in ("desc", "x", "y")))
    got, gsteps = capi.dev_panorama_from_features(_frames(ids, gpu), feats, return_steps=True, keep_steps=True, exposure=e)
    assert got.cpu().numpy().tobytes() == want
    for a, b in zip(gsteps, steps):
        assert bits(a["exposure_stats"]) == bits(b["exposure_stats"]) and a["transferred"].cpu().numpy().tobytes() == b["transferred"].cpu().numpy().tobytes()


@pytest.mark.parametrize("run,mode,kb", [("4", 1, 1), ("4", 2, 1), ("2", 1, 0)])
def test_python_chain(gpu, run, mode, kb):
    final, steps = _c_chain(run, mode, kb, gpu)
    want, wsteps = pipeline.panorama_from_frames(_frames(RUNS[run], gpu), return_steps=True, exposure=mode, keep_black=bool(kb))
    assert want.cpu().numpy().tobytes() == final.cpu().numpy().tobytes()
    for a, b in zip(steps, wsteps):
        assert bits(a["exposure_stats"]) == bits(b["exposure_stats"])
        assert a["transferred"].cpu().numpy().tobytes() == b["transferred"].cpu().numpy().tobytes()
        assert a["out"].cpu().numpy().tobytes() == b["out"].cpu().numpy().tobytes()
    # the recorded order and maps replayed: pipeline.stitch_chain
    rec_steps = [dict(s, mosaic_src=t["mosaic_src"]) for s, t in zip(json.load(open(os.path.join(GOLD, "golden.json")))["runs"][run]["steps"], steps)]
    again = pipeline.stitch_chain(_frames(RUNS[run], gpu), rec_steps, exposure=mode, keep_black=bool(kb))
    assert again.cpu().numpy().tobytes() == final.cpu().numpy().tobytes()


def test_mode_0_is_the_chain_as_it_is(gpu):
    ids = RUNS["4"]
    want, wsteps = capi.dev_panorama(_frames(ids, gpu), return_steps=True, keep_steps=True)
    G = json.load(open(os.path.join(GOLD, "golden.json")))["runs"]["4"]
    assert tsha(want) == G["final_sha256"]
    for e in (dict(mode=0), dict(mode=0, stats_form=1, keep_black=0), 0):
        got, gsteps = capi.dev_panorama(_frames(ids, gpu), return_steps=True, keep_steps=True, exposure=e)
        assert got.cpu().numpy().tobytes() == want.cpu().numpy().tobytes()
        assert all("exposure_stats" not in s for s in gsteps)
        assert [tsha(s["out"]) for s in gsteps] == [s["out_sha256"] for s in G["steps"]]
    assert capi.panorama([_host_frame(i) for i in ids], exposure=dict(mode=0)).tobytes() == want.cpu().numpy().tobytes()
    # and the Python chain's defaults
    assert pipeline.panorama_from_frames(_frames(ids, gpu)).cpu().numpy().tobytes() == want.cpu().numpy().tobytes()


def test_dense4_frames_warped_again(gpu):
    """chains.json `dense4`, mode 1: frames are warped more than once, and a frame warped earlier is stitched to later, so a
    recoloured frame is recoloured again and serves as a template.  The C chain against the Python chain, step by step."""
    import torch
    G = chain_sets.chains()["dense4"]
    order = [(s["srcIndex"], s["dstIndex"]) for s in G["steps"]]
    warped = [d for _, d in order]
    assert max(warped.count(d) for d in set(warped)) >= 2 and any(s in warped[:k] for k, (s, _) in enumerate(order))
    frames = [torch.from_numpy(np.array(f)).to(gpu) for f in chain_sets.frames_of(G["frames"])]
    want, wsteps = pipeline.panorama_from_frames(frames, return_steps=True, exposure=1)
    got, gsteps = capi.dev_panorama(frames, return_steps=True, keep_steps=True, exposure=1)
    assert [(s["mosaic_src"], s["src"]) for s in gsteps] == order == [(s["mosaic_src"], s["src"]) for s in wsteps]
    for a, b in zip(gsteps, wsteps):
        assert bits(a["exposure_stats"]) == bits(b["exposure_stats"])
        assert a["transferred"].cpu().numpy().tobytes() == b["transferred"].cpu().numpy().tobytes()
        assert a["out"].cpu().numpy().tobytes() == b["out"].cpu().numpy().tobytes()
    assert got.cpu().numpy().tobytes() == want.cpu().numpy().tobytes()
    assert tsha(got) != G["final_sha256"]  # the option is on
    again = next(d for d in warped if warped.count(d) >= 2)
    k2 = [k for k, (_, d) in enumerate(order) if d == again]
    assert bits(gsteps[k2[0]]["exposure_stats"])[:6] != bits(gsteps[k2[1]]["exposure_stats"])[:6]  # the second transfer met other colours


def test_refusals_leave_the_library_usable(gpu, series):
    import torch
    frames = _frames(RUNS["2"], gpu)
    for bad in (dict(mode=3), dict(mode=-1), dict(mode=1, stats_form=3), dict(mode=2, stats_form=-1)):
        with pytest.raises(capi.StitchError) as e:
            capi.dev_panorama(frames, exposure=bad)
        assert e.value.code == capi.ERR_ARG and "exposure" in str(e.value)
        with pytest.raises(capi.StitchError) as e:
            capi.panorama([_host_frame(i) for i in RUNS["2"]], exposure=bad)
        assert e.value.code == capi.ERR_ARG
    x = series["uniform_257"]
    for form in (3, -1):
        with pytest.raises(capi.StitchError) as e:
            capi.dev_running_stats([x], form=form)
        assert e.value.code == capi.ERR_ARG
        with pytest.raises(capi.StitchError) as e:
            capi.dev_transfer(frames[0], frames[1], stats_form=form)
        assert e.value.code == capi.ERR_ARG
    with pytest.raises(capi.StitchError):
        capi.dev_running_stats([x] * 7)
    R = _recorded("2", 1, 1)
    final = capi.dev_panorama(frames, exposure=dict(mode=1))  # the library's defaults: spans + walk, keep_black
    assert tsha(final) == R["final_sha256"]
