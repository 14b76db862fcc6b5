"""GPU: ONE pair split into row bands over several ranks (BASELINE.json configs[4]).  The GPU box has
one device, so the ranks of these tests are processes that all drive cuda:0 and exchange through gloo, staged through the
host (pipeline.RankTransport(staged=True)); on a node the same BandStitcher runs with backend "nccl" (RCCL over xGMI) on
device tensors.  Every rank's band of the mosaic must equal the oracle's rows bit for bit.

Which case selects each kernel instance the band path chooses between (csrc/stitch_call_form.h: band_form; the records of these shapes
are tests/golden/band_forms.json, and tests/test_band_form_host.py checks that the list is complete).  "group" is
test_band_group_single_host_thread, the canvas and band count name its case:
  k_src_index, k_vv_x_fwd<PX, true>         level 0 from the frames: every case but group "stored", "stored+fused", "planes"
  k_compose, k_mask, k_vv_x_fwd<float, false> at level 0   group "stored", "stored+fused", "planes"; test_pair_split_into_row_bands planes=True
  k_vv_x_fwd<float, false>, k_vv_x_bwd      every case (levels >= 1; the separate x sweeps: every case that is not fused)
  k_vv_xbyf<false>                          the plain instance, no halo rows and no resume state: test_single_rank_band_is_the_whole_pair;
                                            level 0 of the first band of group True
  k_vv_xbyf<false, float, 0, true>          BANDED: group True, 2048 x 1024 in 2 and 8 bands, 768 x 384 in 3 (level 1: halo rows; bands below the first)
  k_vv_y_fwd, k_vv_y_fwd<true>              every case that is not fused; XCH: group "chunks4"
  k_vv_y_bwd_dec<false>                     even widths, no flags or rows that 8 divides: test_pair_split_into_row_bands_threads, 1540 x 768
  k_vv_y_bwd_dec<true>                      the per-row flag look-up: test_single_rank_band_is_the_whole_pair (500 and 250 rows);
                                            with neighbours, test_fused_band_rows_that_eight_does_not_divide (132 rows)
  k_vv_y_bwd_dec<false, YST, true, false, true>   XCH: group "chunks4", 2048 x 1024 and 768 x 384
  k_vv_y_bwd_dec<true, YST, true, false, true>    XCH with the per-row look-up: test_fused_sweep_then_decimation_over_a_column_range (no sequence of
                                            BandStitcher.steps selects it)
  k_vv_y_bwd + k_decimate                   odd level widths: 770 x 384 (level 1 is 385 wide); STITCH_BAND_PLAIN=1 in test_gpu_switches.py
  k_collapse4, k_collapse                   widths with and without a regular run of 256 columns: every case (2048 x 1024: levels 0 and 1 / level 2)"""
import os
import socket
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def _inputs(oracle, fw, fh, dtype):
    A, B = oracle.synth(fw, fh, 4, dtype), oracle.synth(fw, fh, 5, dtype)
    P = [1.0, 0.002, 1e-6, -(fw // 2) - 40.0, -0.001, 1.0, 5e-7, 1.5]
    return A, B, P


def _worker(rank, world, port, outdir, fw, fh, cw, ch, Ls, dt, planes=False):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, HERE)
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    import torch
    import torch.distributed as dist
    from computervisionimagestich2_amd import pipeline
    from oracle_lib import Oracle
    dist.init_process_group("gloo", rank=rank, world_size=world)
    dev = torch.device("cuda:0")
    torch.cuda.set_device(0)
    dtype = np.uint8 if dt == "u8" else np.float32
    A, B, P = _inputs(Oracle(), fw, fh, dtype)
    st = pipeline.BandStitcher(cw, ch, Ls, pipeline.RankTransport(staged=True), dev, plane_pipeline_min=0 if planes else None)
    for rep in range(2):  # twice: the workspace is reused
        out = st.run(torch.from_numpy(B).to(dev), P, 0.0, 0.0, torch.from_numpy(A).to(dev), 0, 0)
    np.save(os.path.join(outdir, f"band{rank}.npy"), out.cpu().numpy())
    np.save(os.path.join(outdir, f"seam{rank}.npy"), np.array(st.seam.as_tuple()))
    st.close()
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize("world,fw,fh,cw,ch,Ls,dt,planes", [(2, 1408, 1024, 2048, 1024, 2, "f32", False), (4, 704, 512, 1024, 512, 1, "f32", False),
                                                             (3, 520, 384, 770, 384, 2, "u8", False), (3, 520, 384, 768, 384, 2, "f32", True)])
def test_pair_split_into_row_bands(tmp_path, oracle, gpu, world, fw, fh, cw, ch, Ls, dt, planes):
    """planes: the recurrence state crosses ranks plane by plane (blocking send / recv in pipeline order), the form of levels
    that are bound by bytes; forced here at a small size."""
    import torch.multiprocessing as mp
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    mp.spawn(_worker, args=(world, port, str(tmp_path), fw, fh, cw, ch, Ls, dt, planes), nprocs=world, join=True)
    dtype = np.uint8 if dt == "u8" else np.float32
    A, B, P = _inputs(oracle, fw, fh, dtype)
    rc, ref = oracle.pair(B, P, 0.0, 0.0, A, 0, 0, cw, ch)
    assert rc == 0
    got = np.concatenate([np.load(tmp_path / f"band{r}.npy") for r in range(world)], axis=1)
    assert got.shape == ref.shape
    bad = np.argwhere(got != ref)
    assert bad.size == 0, f"banded mosaic differs from the oracle at {len(bad)} samples; rows {bad[:, 1].min()}..{bad[:, 1].max()}, " \
                          f"columns {bad[:, 2].min()}..{bad[:, 2].max()}, first {bad[0].tolist()}"
    seams = [tuple(np.load(tmp_path / f"seam{r}.npy")) for r in range(world)]
    assert len(set(seams)) == 1  # every rank derived the same seam, without communication


def test_single_rank_band_is_the_whole_pair(st, gpu, oracle):
    """nranks = 1: the band code path without any exchange (unfused sweeps, replicated coarse levels through an ordinary plan
    whose level 0 is handed in as planes) equals the oracle."""
    import torch
    import torch.distributed as dist
    from computervisionimagestich2_amd import pipeline
    if not dist.is_initialized():
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29533")
        dist.init_process_group("gloo", rank=0, world_size=1)
    fw, fh, cw, ch = 700, 500, 1000, 500
    for dtype in (np.uint8, np.float32):
        A, B, P = _inputs(oracle, fw, fh, dtype)
        bs = pipeline.BandStitcher(cw, ch, 2, pipeline.RankTransport(staged=True), gpu)
        out = bs.run(torch.from_numpy(B).to(gpu), P, 0.0, 0.0, torch.from_numpy(A).to(gpu), 0, 0)
        rc, ref = oracle.pair(B, P, 0.0, 0.0, A, 0, 0, cw, ch)
        assert rc == 0 and np.array_equal(out.cpu().numpy().view(np.uint8), ref.view(np.uint8))
        bs.close()
    dist.destroy_process_group()


@pytest.mark.parametrize("world,fw,fh,cw,ch,Ls,dt", [(2, 1408, 1024, 2048, 1024, 3, "u8"), (3, 520, 384, 768, 384, 2, "u8"), (2, 520, 384, 770, 384, 2, "f32"),
                                                      (2, 1040, 768, 1540, 768, 2, "u8"), (6, 520, 384, 772, 384, 1, "f32"), (8, 1408, 1024, 2048, 1024, 2, "u8")])
def test_pair_split_into_row_bands_threads(st, gpu, oracle, world, fw, fh, cw, ch, Ls, dt):
    """The same split with the ranks as threads on separate HIP streams, handing over on the device (pipeline.LocalTransport:
    a device copy and an event per hand-off, no host synchronisation): more shapes (odd level widths -> the stand-alone
    decimation, band counts that are not powers of two -> the level's, not the band's, decimation weights, 8 bands), two
    repetitions on the same workspaces."""
    import threading
    import torch
    from computervisionimagestich2_amd import pipeline
    dtype = np.uint8 if dt == "u8" else np.float32
    A, B, P = _inputs(oracle, fw, fh, dtype)
    rc, ref = oracle.pair(B, P, 0.0, 0.0, A, 0, 0, cw, ch)
    assert rc == 0
    qs = pipeline.LocalTransport.make_queues(world)
    outs, errs = [[None, None] for _ in range(world)], []

    def work(r):
        try:
            torch.cuda.set_device(0)
            with torch.cuda.stream(torch.cuda.Stream()):
                bs = pipeline.BandStitcher(cw, ch, Ls, pipeline.LocalTransport(r, world, qs), gpu)
                for rep in range(2):
                    outs[r][rep] = bs.run(torch.from_numpy(B).to(gpu), P, 0.0, 0.0, torch.from_numpy(A).to(gpu), 0, 0).cpu().numpy()
                bs.close()
        except Exception as e:  # a failing rank must not leave the others waiting on their queues for ever
            errs.append((r, repr(e)))
            for k in qs:
                if k[0] == r:
                    qs[k].put(None)

    th = [threading.Thread(target=work, args=(r,)) for r in range(world)]
    [t.start() for t in th]
    [t.join(timeout=300) for t in th]
    assert not errs, errs
    for rep in range(2):
        got = np.concatenate([outs[r][rep] for r in range(world)], axis=1)
        bad = np.argwhere(got != ref)
        assert bad.size == 0, (rep, len(bad), bad[:3].tolist())


@pytest.mark.parametrize("world,fw,fh,cw,ch,Ls,dt", [(2, 1408, 1024, 2048, 1024, 3, "u8"), (3, 520, 384, 768, 384, 2, "f32"), (8, 1408, 1024, 2048, 1024, 2, "f32"),
                                                      (6, 520, 384, 772, 384, 1, "u8")])
@pytest.mark.parametrize("fuse", [True, False, "planes", "stored", "stored+fused", "chunks4"])
def test_band_group_single_host_thread(st, gpu, oracle, world, fw, fh, cw, ch, Ls, dt, fuse):
    """pipeline.LocalBandGroup: all bands of a pair on one device, their launch sequences (BandStitcher.steps) interleaved by ONE
    host thread, hand-offs as device copies ordered by events -- the same generator a rank of its own executes over RCCL.  Two
    repetitions on the same workspaces; every band equals the oracle's rows.  fuse: the anticausal x sweep fused with the
    causal y sweep, which resumes from the state of the band above (stitch_band_reduce_xy_fwd), or the three separate sweeps, or
    ("planes") the separate sweeps with the state handed from band to band plane by plane (level 0 stored as planes).  Level 0 is
    source-fused by default (index plane + gathers from the frames, implicit mask); "stored": the materialised level 0."""
    import torch
    from computervisionimagestich2_amd import pipeline
    dtype = np.uint8 if dt == "u8" else np.float32
    A, B, P = _inputs(oracle, fw, fh, dtype)
    rc, ref = oracle.pair(B, P, 0.0, 0.0, A, 0, 0, cw, ch)
    assert rc == 0
    grp = pipeline.LocalBandGroup(cw, ch, Ls, world, gpu, fuse_sweeps=fuse in (True, "stored+fused"), plane_pipeline_min=0 if fuse == "planes" else None,
                                  col_chunks=4 if fuse == "chunks4" else 1)  # "chunks4": the y states cross bands in four column chunks
    if str(fuse).startswith("stored"):  # level 0 as seven stored planes (k_compose + k_mask) instead of source-fused
        for b in grp.bands:
            b.band.set_level0(False)
    dA, dB = torch.from_numpy(A).to(gpu), torch.from_numpy(B).to(gpu)
    for rep in range(2):
        outs = grp.run(dB, P, 0.0, 0.0, dA, 0, 0)
        got = torch.cat(outs, dim=1).cpu().numpy()
        bad = np.argwhere(got != ref)
        assert bad.size == 0, (rep, len(bad), bad[:3].tolist())
    assert len({b.seam.as_tuple() for b in grp.bands}) == 1
    grp.close()


def test_fused_band_rows_that_eight_does_not_divide(st, gpu, oracle):
    """The per-row flag look-up of the decimating sweep (k_vv_y_bwd_dec<true>): bands of 132 rows at level 0 behind the fused sweep,
    so that a chunk of eight rows straddles two 64-row bands of tiles.  Three bands, two split levels, against the oracle."""
    import torch
    from computervisionimagestich2_amd import pipeline
    world, fw, fh, cw, ch, Ls = 3, 520, 396, 768, 396, 2
    A, B, P = _inputs(oracle, fw, fh, np.uint8)
    rc, ref = oracle.pair(B, P, 0.0, 0.0, A, 0, 0, cw, ch)
    assert rc == 0
    grp = pipeline.LocalBandGroup(cw, ch, Ls, world, gpu, fuse_sweeps=True)
    assert [g["rows"] for g in grp.bands[0].geom[:2]] == [132, 66]
    dA, dB = torch.from_numpy(A).to(gpu), torch.from_numpy(B).to(gpu)
    for rep in range(2):
        got = torch.cat(grp.run(dB, P, 0.0, 0.0, dA, 0, 0), dim=1).cpu().numpy()
        bad = np.argwhere(got != ref)
        assert bad.size == 0, (rep, len(bad), bad[:3].tolist())
    grp.close()


def test_fused_sweep_then_decimation_over_a_column_range(st, gpu, oracle):
    """The same look-up in the column-chunk instance (k_vv_y_bwd_dec<true, YST, true, false, true>).  BandStitcher.steps never selects
    it -- its column chunks follow the separate x sweeps, which leave no flags -- so the calls are issued here: one band (no exchange),
    at both split levels the fused sweep, then the decimating sweep over the column range [0, pitch).  The pitches are multiples of 128,
    so the range's state arrays are laid out as the fused sweep leaves them.  396 and 198 rows; against the oracle."""
    import torch
    from computervisionimagestich2_amd import capi
    fw, fh, cw, ch, Ls = 520, 396, 768, 396, 2
    A, B, P = _inputs(oracle, fw, fh, np.float32)
    rc, ref = oracle.pair(B, P, 0.0, 0.0, A, 0, 0, cw, ch)
    assert rc == 0
    band = capi.Band(cw, ch, 0, 1, Ls)
    geom = band.geom
    assert all(g["pitch"] % 128 == 0 and g["rows"] % 8 for g in geom[:Ls])
    f64 = dict(dtype=torch.float64, device=gpu)
    out = torch.empty((3, geom[0]["rows"], geom[0]["w"]), dtype=torch.float32, device=gpu)
    for rep in range(2):
        band.compose(torch.from_numpy(B).to(gpu), P, 0.0, 0.0, torch.from_numpy(A).to(gpu), 0, 0)
        for l in range(Ls):
            fwd, bwd = torch.zeros(4 * 7 * geom[l]["pitch"], **f64), torch.zeros(3 * 7 * geom[l]["pitch"], **f64)
            band.reduce_xy_fwd(l, None, fwd)
            band.reduce_y_bwd_cols(l, 0, geom[l]["pitch"], fwd, None, bwd)
        top = torch.empty((7, geom[Ls]["rows"], geom[Ls]["w"]), dtype=torch.float32, device=gpu)
        band.rows(Ls, 2, 0, geom[Ls]["rows"], top, True)
        band.top(top)
        for l in range(Ls - 1, -1, -1):
            band.collapse(l, out if l == 0 else None)
        band.status()
        got = out.cpu().numpy()
        assert np.array_equal(got.view(np.uint8), ref.view(np.uint8)), (rep, int((got != ref).sum()))
    band.close()


def test_band_random_configs(st, gpu, oracle):
    """Seeded random band splits against the oracle: 1-4 ranks, 1-3 split levels, even and odd canvas widths (odd widths keep the
    separate anticausal sweep + decimation and no zero-tile flags), both pixel types, every form of the reduce (fused sweep with
    and without neighbours, separate sweeps, stored level 0, plane-by-plane hand-off, the state handed over in 2, 3 or 5 column chunks),
    frames that cover part of the canvas."""
    import torch
    from computervisionimagestich2_amd import pipeline
    rng = np.random.default_rng(int(os.environ.get("FUZZ_BANDS_SEED", "20261006")))
    forms = [dict(fuse_sweeps=True), dict(fuse_sweeps=False), dict(fuse_sweeps=None), dict(fuse_sweeps=False, plane_pipeline_min=0), dict(fuse_sweeps=True, stored=True),
             dict(fuse_sweeps=False, col_chunks=2), dict(fuse_sweeps=False, col_chunks=3, stored=True), dict(fuse_sweeps=None, col_chunks=5)]
    ran, skipped = 0, []
    n_cases = int(os.environ.get("FUZZ_BANDS", "30"))  # FUZZ_BANDS=500 FUZZ_BANDS_SEED=n: a campaign
    for case in range(n_cases):
        world, Ls = int(rng.integers(1, int(os.environ.get("FUZZ_BANDS_WORLD", "4")) + 1)), int(rng.integers(1, 4))
        cw = int(rng.integers(200, 900))
        base = world << Ls  # band heights even on every split level
        ch = base * max(4, int(cw * rng.uniform(0.55, 1.1)) // base)  # tall enough for the pyramid the width asks for
        fw, fh = int(cw * rng.uniform(0.55, 0.8)), ch - int(rng.integers(0, 6))
        dtype = np.uint8 if case % 2 else np.float32
        form = dict(forms[case % len(forms)])
        stored = form.pop("stored", False)
        A, B = oracle.synth(fw, fh, 40 + case, dtype), oracle.synth(fw, fh, 80 + case, dtype)
        P = [1.0, 0.002, 1e-6, -(cw - fw) + 3.0, -0.001, 1.0, 5e-7, 1.5]
        rc, ref = oracle.pair(B, P, 0.0, 0.0, A, 0, 0, cw, ch)
        if rc != 0:
            skipped.append((case, "oracle", rc))
            continue
        try:
            grp = pipeline.LocalBandGroup(cw, ch, Ls, world, gpu, **form)
        except st.capi.StitchError as e:
            skipped.append((case, world, Ls, cw, ch, str(e)[:80]))
            continue  # a pyramid too shallow for this split
        if stored:
            for b in grp.bands:
                b.band.set_level0(False)
        outs = grp.run(torch.from_numpy(B).to(gpu), P, 0.0, 0.0, torch.from_numpy(A).to(gpu), 0, 0)
        got = torch.cat(outs, dim=1).cpu().numpy()
        bad = np.argwhere(got.view(np.uint8) != ref.view(np.uint8))
        assert bad.size == 0, (case, world, Ls, cw, ch, str(dtype), form, stored, len(bad), bad[:3].tolist())
        grp.close()
        ran += 1
    print(f"band configs compared: {ran} of {n_cases}")
    assert ran >= n_cases // 2, skipped[:6]


def test_config5_size_two_bands_equal_the_plan(st, gpu):
    """BASELINE.json configs[4] at its full size through the band split: one 16384 x 16384 x 3 f32 pair -> 24576 x 16384 mosaic as
    TWO row bands (ranks as threads on two streams of this GPU, device-side hand-offs) equals the single-GPU plan's mosaic bit for
    bit -- and that plan is compared with the oracle at this size by test_config5_size_single_gpu_against_oracle."""
    import threading
    import torch
    from computervisionimagestich2_amd import capi, pipeline
    F, Ls, world = 16384, 4, 2
    cw, ch = pipeline.config_canvas(F)
    A, B = capi.dev_synth(F, F, 0, torch.float32, gpu), capi.dev_synth(F, F, 1, torch.float32, gpu)
    p = pipeline.config_map(0, F)
    plan = capi.Plan(cw, ch)
    ref = plan.pair(B, p, 0.0, 0.0, A, 0, 0)
    plan.status()
    plan.close()
    qs = pipeline.LocalTransport.make_queues(world)
    outs, errs = [None] * world, []

    def work(r):
        try:
            torch.cuda.set_device(0)
            with torch.cuda.stream(torch.cuda.Stream()):
                bs = pipeline.BandStitcher(cw, ch, Ls, pipeline.LocalTransport(r, world, qs), gpu)
                outs[r] = bs.run(B, p, 0.0, 0.0, A, 0, 0)
                torch.cuda.current_stream().synchronize()
                bs.close()
        except Exception as e:
            errs.append((r, repr(e)))
            for k in qs:
                if k[0] == r:
                    qs[k].put(None)

    th = [threading.Thread(target=work, args=(r,)) for r in range(world)]
    [t.start() for t in th]
    [t.join(timeout=600) for t in th]
    assert not errs, errs
    assert torch.equal(torch.cat(outs, dim=1), ref)


def test_rccl_transport_single_rank_smoke(st, gpu):
    """pipeline.RankTransport(staged=False) -- the form a node runs: device tensors straight into RCCL -- with the one rank this
    box has: all_gather and an (empty) neighbour exchange go through backend "nccl", and a one-band BandStitcher on top of it equals
    the staged transport's result.  More ranks need more GPUs; the multi-rank logic is covered over gloo and by LocalTransport."""
    import torch
    import torch.distributed as dist
    from computervisionimagestich2_amd import pipeline
    from oracle_lib import Oracle
    oracle = Oracle()
    if dist.is_initialized():
        dist.destroy_process_group()
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    os.environ["MASTER_PORT"] = "29541"
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=gpu)
    try:
        T = pipeline.RankTransport(staged=False)
        t = torch.arange(24, dtype=torch.float32, device=gpu).reshape(2, 3, 4)
        g = T.all_gather(t)
        assert g.shape == (1, 2, 3, 4) and g.is_cuda and torch.equal(g[0], t)
        T.swap(None, None, None, None)
        fw, fh, cw, ch = 700, 500, 1000, 500
        A, B, P = _inputs(oracle, fw, fh, np.float32)
        bs = pipeline.BandStitcher(cw, ch, 2, T, gpu)
        out = bs.run(torch.from_numpy(B).to(gpu), P, 0.0, 0.0, torch.from_numpy(A).to(gpu), 0, 0)
        rc, ref = oracle.pair(B, P, 0.0, 0.0, A, 0, 0, cw, ch)
        assert rc == 0 and np.array_equal(out.cpu().numpy().view(np.uint8), ref.view(np.uint8))
        bs.close()
    finally:
        dist.destroy_process_group()
