"""GPU: the band path (csrc/stitch_band.inc, capi.Band, pipeline.BandStitcher, pipeline.LocalBandGroup) on hard pixel content and on
bands an image does not reach -- tests/band_hard.py's table, which tests/test_band_hard_host.py holds to the oracle on the CPU.  Every
comparison is bit equality with the oracle, every seam record equals the oracle's, every refusal is the oracle's code.

a  test_band_group_on_hard_rows: per canvas, form and pixel type ONE LocalBandGroup runs a synthetic full-height pair, then every
   placement's item aligned and tilted -- consecutive placements leave other bands empty, so the zero-tile flags of one run are
   followed by a run whose zero tiles lie elsewhere -- then the synthetic pair again.
b  test_state_entering_an_empty_band_matters: (a) is not vacuous.  With the recurrence states one band sends another replaced by
   zeros, the band the frame does not reach differs from the oracle: the kernels may not treat its all-zero tiles as zeros under a
   zero state.
c  test_refused_pairs_on_bands: refused pairs (-3, -2, -3) between accepted ones, on a group and on BandStitchers run by threads:
   every band reports the oracle's code, nobody waits, and the accepted pairs around them are bit-equal.
d  test_hard_rows_over_processes: three processes, one rank each, over gloo; `tiny` over `signed`: -0.0f, subnormals and negative
   samples in the states and halo rows that cross ranks as raw bytes."""
import os
import socket
import sys

import numpy as np
import pytest

import band_hard as BH
import hard_inputs as H

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)

IDS = {np.uint8: "u8", np.float32: "f32"}
GROUPS = [(c, form, dtype) for c in range(len(BH.CANVASES)) for form in BH.forms_of(c) for dtype in BH.DTYPES]


def group_id(g):
    return f"{BH.CANVASES[g[0]][0]}x{BH.CANVASES[g[0]][1]}-{g[1]}-{IDS[g[2]]}"


def tensor(a, gpu):
    import torch
    return torch.from_numpy(np.array(a)).to(gpu)


@pytest.fixture(scope="module")
def world():
    """Pairs with the oracle's answer (rc, ref, seam), computed once per key and left unchanged.  keep=False: an item only one test
    runs is not retained."""
    cache = {}

    def get(key, make, keep=True):
        if key in cache:
            return cache[key]
        r = make()
        r["rc"], r["ref"], r["seam"] = H.pair_oracle(r)
        for a in (r["F"], r["M"], r["ref"]):
            a.setflags(write=False)
        if keep:
            cache[key] = r
        return r
    return get


def synth_of(world, c, dtype):
    r = world(("synth", c, IDS[dtype]), lambda: BH.full_height_pair(c, dtype))
    assert r["rc"] == 0
    return r


def item_of(world, c, placement, form, dtype, variant, keep=False):
    r = world(BH.item_key(c, placement, form, dtype, variant), lambda: BH.item(c, placement, form, dtype, variant), keep)
    assert r["rc"] == BH.stated_rc(c, placement, form, dtype, variant), (r["key"], r["rc"])  # the statement, and what the oracle answers
    return r


def refusal_of(world, c, name, dtype):
    r = world(("refusal", c, name, IDS[dtype]), lambda: BH.refusal_pair(c, name, dtype))
    assert r["rc"] == BH.REFUSAL_PLACEMENTS[name], (name, r["rc"])
    return r


def make_group(cls, c, form, gpu):
    cw, ch, _, _, bands, Ls = BH.CANVASES[c]
    grp = cls(cw, ch, Ls, bands, gpu, **BH.FORMS[form])
    if BH.stored(form):  # level 0 as seven stored planes (k_compose + k_mask) instead of source-fused
        for b in grp.bands:
            b.band.set_level0(False)
    return grp


def run_group(grp, r, gpu):
    import torch
    return torch.cat(grp.run(tensor(r["F"], gpu), r["p"], r["offx"], r["offy"], tensor(r["M"], gpu), r["ox"], r["oy"]), dim=1).cpu().numpy()


def differing(got, r):
    """The samples whose bits differ from the oracle's, as np.argwhere gives them (channel, row, column)."""
    assert got.shape == r["ref"].shape and got.dtype == r["ref"].dtype, (got.shape, got.dtype)
    px = np.uint8 if got.dtype == np.uint8 else np.uint32
    return np.argwhere(got.view(px) != r["ref"].view(px))


def check_run(grp, r, gpu, what):
    """One pair on the group: the oracle's bits and seam in every band, or the oracle's refusal from run and from every band."""
    from computervisionimagestich2_amd import capi
    if r["rc"] == 0:
        bad = differing(run_group(grp, r, gpu), r)
        assert bad.size == 0, (what, r["name"], len(bad), bad[:3].tolist(), int(bad[:, 1].min()), int(bad[:, 1].max()))
        assert [b.seam.as_tuple() for b in grp.bands] == [r["seam"].as_tuple()] * len(grp.bands), (what, r["name"])
        assert [b.band.status().as_tuple() for b in grp.bands] == [r["seam"].as_tuple()] * len(grp.bands), (what, r["name"])
        return
    assert r["rc"] in (capi.ERR_EMPTY_MIDROW, capi.ERR_ZERO_OVERLAP)
    with pytest.raises(capi.StitchError) as e:
        run_group(grp, r, gpu)
    assert e.value.code == r["rc"], (what, r["name"], e.value.code)
    for b in grp.bands:  # every band answers alike
        with pytest.raises(capi.StitchError) as e:
            b.band.status()
        assert e.value.code == r["rc"], (what, r["name"], b.rank, e.value.code)
    assert not any(grp.box.values()), (what, "a message nobody took")


# ---- a ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("group", GROUPS, ids=group_id)
def test_band_group_on_hard_rows(st, gpu, world, group):
    from computervisionimagestich2_amd import pipeline
    c, form, dtype = group
    grp = make_group(pipeline.LocalBandGroup, c, form, gpu)
    try:
        assert [g["rows"] for g in (b.geom[0] for b in grp.bands)] == [r1 - r0 for r0, r1 in BH.band_rows(c)]
        check_run(grp, synth_of(world, c, dtype), gpu, "synthetic, first")
        for placement in BH.RUN_ORDER:
            for variant in BH.VARIANTS:
                check_run(grp, item_of(world, c, placement, form, dtype, variant), gpu, (placement, variant))
        check_run(grp, synth_of(world, c, dtype), gpu, "synthetic, last")
    finally:
        grp.close()


# ---- b ---------------------------------------------------------------------------------------------------------------------------
def zeroing_group(base, pair):
    class ZeroedStates(base):
        """Posts zeros in place of every float64 message (the recurrence states) from pair[0] to pair[1]; the float32 halo rows and
        gathers pass untouched."""
        zeroed = 0

        def _post(self, t, src, dst):
            import torch
            if (src, dst) == pair and t.dtype == torch.float64:
                t = torch.zeros_like(t)
                self.zeroed += 1
            super()._post(t, src, dst)
    return ZeroedStates


@pytest.mark.parametrize("placement,pair", [("top_bottom", (1, 2)), ("bottom_top", (1, 0))], ids=["causal", "anticausal"])
@pytest.mark.parametrize("form", ["fused", "separate"])
def test_state_entering_an_empty_band_matters(st, gpu, world, form, placement, pair):
    """float32 frames on the main canvas.  top_bottom: the frame ends above band 2, and the causal states band 1 sends it are zeroed;
    bottom_top: the frame begins below band 0, and the anticausal states band 1 sends it are zeroed.  The untampered run equals the
    oracle; the tampered one differs inside the receiving band, which no frame row reaches."""
    from computervisionimagestich2_amd import pipeline
    c, dtype, dst = BH.MAIN, np.float32, pair[1]
    assert dst in BH.EMPTY[(c, placement)][0] and pair[0] not in BH.EMPTY[(c, placement)][0]  # the frame reaches the sender alone
    r = item_of(world, c, placement, form, dtype, "aligned", keep=True)
    assert r["rc"] == 0
    grp = make_group(pipeline.LocalBandGroup, c, form, gpu)
    try:
        check_run(grp, r, gpu, "untampered")
    finally:
        grp.close()
    grp = make_group(zeroing_group(pipeline.LocalBandGroup, pair), c, form, gpu)
    try:
        bad = differing(run_group(grp, r, gpu), r)
        assert grp.zeroed == BH.CANVASES[c][5], grp.zeroed  # one state message per split level
    finally:
        grp.close()
    r0, r1 = BH.band_rows(c)[dst]
    inside = bad[(bad[:, 1] >= r0) & (bad[:, 1] < r1)]
    print(f"{form} {placement}: states {pair[0]} -> {pair[1]} zeroed: {len(bad)} samples differ, {len(inside)} of them in band {dst}"
          + (f", rows {inside[:, 1].min()} .. {inside[:, 1].max()}" if len(inside) else ""))
    assert len(inside) > 0


# ---- c ---------------------------------------------------------------------------------------------------------------------------
def refusal_sequence(world, form, dtype):
    c = BH.MAIN
    first = item_of(world, c, "top_bottom", form, dtype, "aligned", keep=True)
    third = item_of(world, c, "frame_mid", form, dtype, "tilted", keep=True)
    seq = [first, refusal_of(world, c, "mosaic_above_mid", dtype), third, refusal_of(world, c, "fold", dtype), refusal_of(world, c, "miss", dtype), first]
    assert [r["rc"] for r in seq] == [0, -3, 0, -2, -3, 0]
    return seq


@pytest.mark.parametrize("dtype", BH.DTYPES, ids=["u8", "f32"])
@pytest.mark.parametrize("form", ["fused", "separate", "planes"])
def test_refused_pairs_on_bands(st, gpu, world, form, dtype):
    import threading
    import torch
    from computervisionimagestich2_amd import capi, pipeline
    c = BH.MAIN
    cw, ch, _, _, bands, Ls = BH.CANVASES[c]
    seq = refusal_sequence(world, form, dtype)
    grp = make_group(pipeline.LocalBandGroup, c, form, gpu)
    try:
        for i, r in enumerate(seq):
            check_run(grp, r, gpu, ("group", i))
    finally:
        grp.close()

    # the same through ranks that are threads (pipeline.LocalTransport), every rank on its own stream
    qs = pipeline.LocalTransport.make_queues(bands)
    got, errs = [[None] * len(seq) for _ in range(bands)], []

    def work(rank):
        try:
            torch.cuda.set_device(0)
            with torch.cuda.stream(torch.cuda.Stream()):
                bs = pipeline.BandStitcher(cw, ch, Ls, pipeline.LocalTransport(rank, bands, qs), gpu, **BH.FORMS[form])
                for i, r in enumerate(seq):
                    try:
                        out = bs.run(tensor(r["F"], gpu), r["p"], r["offx"], r["offy"], tensor(r["M"], gpu), r["ox"], r["oy"])
                        got[rank][i] = (0, out.cpu().numpy(), bs.seam.as_tuple())
                    except capi.StitchError as e:  # a refusal: this rank goes on with the next pair
                        got[rank][i] = (e.code, None, None)
                bs.close()
        except Exception as e:  # a failing rank must not leave the others waiting on their queues for ever
            errs.append((rank, repr(e)))
            for k in qs:
                if k[0] == rank:
                    qs[k].put(None)

    th = [threading.Thread(target=work, args=(rank,)) for rank in range(bands)]
    [t.start() for t in th]
    [t.join(timeout=300) for t in th]
    assert not errs, errs
    assert not any(t.is_alive() for t in th), "a rank is left waiting"
    assert all(q.empty() for q in qs.values()), "a message nobody took"
    for i, r in enumerate(seq):
        assert [got[rank][i][0] for rank in range(bands)] == [r["rc"]] * bands, (i, r["name"])  # every rank answers alike
        if r["rc"] == 0:
            bad = differing(np.concatenate([got[rank][i][1] for rank in range(bands)], axis=1), r)
            assert bad.size == 0, ("threads", i, r["name"], len(bad), bad[:3].tolist())
            assert [got[rank][i][2] for rank in range(bands)] == [r["seam"].as_tuple()] * bands, (i, r["name"])


# ---- d ---------------------------------------------------------------------------------------------------------------------------
PROCESS_CASE = dict(c=BH.MAIN, dtype=np.float32, frame="tiny", mosaic="signed", placements=("top_bottom", "bottom_top"))


def process_pairs():
    """The two pairs of (d): `tiny` frames over `signed` mosaics, seeds as the class rule gives them."""
    c, dtype = PROCESS_CASE["c"], PROCESS_CASE["dtype"]
    cw, ch, x0, mw = BH.CANVASES[c][:4]
    out = []
    for placement in PROCESS_CASE["placements"]:
        f0, f1, m0, m1 = BH.rows(placement, ch)
        s = BH.item_seed(c, placement)
        out.append(BH.placed(c, placement, "aligned", H.content(PROCESS_CASE["frame"], cw - x0, f1 - f0, dtype, 2 * s + 1),
                             H.content(PROCESS_CASE["mosaic"], mw, m1 - m0, dtype, 2 * s)))
    return out


def _worker(rank, world_size, port, outdir):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, HERE)
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    import torch
    import torch.distributed as dist
    from computervisionimagestich2_amd import pipeline
    dist.init_process_group("gloo", rank=rank, world_size=world_size)
    dev = torch.device("cuda:0")
    torch.cuda.set_device(0)
    cw, ch, _, _, bands, Ls = BH.CANVASES[PROCESS_CASE["c"]]
    st = pipeline.BandStitcher(cw, ch, Ls, pipeline.RankTransport(staged=True), dev)
    for i, r in enumerate(process_pairs()):  # the same stitcher: the second pair's zero tiles lie where the first's data was
        out = st.run(torch.from_numpy(r["F"]).to(dev), r["p"], r["offx"], r["offy"], torch.from_numpy(r["M"]).to(dev), r["ox"], r["oy"])
        np.save(os.path.join(outdir, f"band{i}_{rank}.npy"), out.cpu().numpy())
        np.save(os.path.join(outdir, f"seam{i}_{rank}.npy"), np.array(st.seam.as_tuple()))
    st.close()
    dist.barrier()
    dist.destroy_process_group()


def test_hard_rows_over_processes(tmp_path, gpu, world):
    import torch.multiprocessing as mp
    bands = BH.CANVASES[PROCESS_CASE["c"]][4]
    pairs = process_pairs()
    refs = [world(("processes", i), lambda r=r: r) for i, r in enumerate(pairs)]
    assert [r["rc"] for r in refs] == [0, 0]
    bits = refs[0]["F"].view(np.uint32)
    assert (bits == 0x80000000).any() and ((bits & 0x7F800000 == 0) & (bits & 0x007FFFFF != 0)).any() and (refs[0]["M"] < 0).any()
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    mp.spawn(_worker, args=(bands, port, str(tmp_path)), nprocs=bands, join=True)
    for i, r in enumerate(refs):
        got = np.concatenate([np.load(tmp_path / f"band{i}_{rank}.npy") for rank in range(bands)], axis=1)
        bad = differing(got, r)
        assert bad.size == 0, (i, r["name"], len(bad), bad[:3].tolist())
        seams = [tuple(np.load(tmp_path / f"seam{i}_{rank}.npy")) for rank in range(bands)]
        assert seams == [r["seam"].as_tuple()] * bands, (i, seams)
