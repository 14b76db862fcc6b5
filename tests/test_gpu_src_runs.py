"""GPU: the level-0 index planes kept in 16-byte runs and the causal x sweep that gathers through them (csrc/k_compose.inc k_src_runs,
csrc/k_sweeps.inc k_vv_x_fwd<float, true>; include/stitch_src_runs.h).  Every output is compared with Oracle.pair bit for bit, and
Plan.src_run_counts() with the rule restated in tests/src_runs_ref.py and with the library's own host function.

At these sizes the causal sweep of a source-fused call defaults to k_vv_x_m; STITCH_SINGLE_FAST=1 and STITCH_MOVER=0 pin
k_vv_x_fwd<PX, true>, and non-zero counts prove that its fast path was handed the runs."""
import numpy as np
import pytest

import src_runs_ref as R
from oracle_lib import ROOT_OPTS
from test_gpu_collapse_sides import geometry

pytestmark = pytest.mark.gpu

OPTS = dict(ROOT_OPTS, level_rule=1)
PIN = {"STITCH_SINGLE_FAST": "1", "STITCH_MOVER": "0"}


def translation(tx, ty):
    return (1.0, 0.0, 0.0, -float(tx), 0.0, 1.0, 0.0, -float(ty))


# name -> (cw, ch, fw, fh, map, (mw, mh, ox, oy))
CASES = {
    # skips in both directions: tiles without patches, with a few, and general ones
    "skips": (1024, 192) + geometry(1024, 192)[:2] + (geometry(1024, 192)[2], (682, 192, 0, 0)),
    # the frame's left edge inside a tile, a map that stretches x: every group has patches, most tiles are general
    "stretched": (1088, 128, 700, 128, (1.3, 0.002, 1e-6, -100.0, -0.001, 1.0, 5e-7, 1.5), (700, 128, 0, 0)),
    # a pure translation by multiples of 4, a frame width that is one: every tile without patches; the last row's last group ends
    # exactly at the plane's end
    "translation": (1024, 192, 512, 192, translation(128, 0), (600, 192, 0, 0)),
    # by an odd number of pixels: every 16-byte load 4-byte aligned only; the frame's edges cut groups
    "odd translation": (1024, 192, 513, 150, translation(131, 8), (600, 192, 0, 0)),
    # a frame inside one tile whose edges cut groups: 2 + 2 patches in each of 16 rows = 64, the last record of the block; the last
    # row's last group would read past the plane's end (its base is "outside", its samples are patches)
    "64 patches": (1024, 192, 8, 16, translation(130, 90), (600, 192, 0, 0)),
    # 3 + 2 patches in each of 13 rows = 65: general
    "65 patches": (1024, 192, 9, 13, translation(129, 90), (600, 192, 0, 0)),
    # Canvas pixel (x, y) shows mosaic pixel (x + ox, y + oy).  The mosaic's four edges inside tiles, ox no multiple of 4, negative offsets
    "mosaic edges": (1024, 192, 682, 192, geometry(1024, 192)[2], (500, 150, -37, -21)),
    "mosaic inside": (1024, 192, 682, 192, geometry(1024, 192)[2], (390, 100, -70, -30)),
    # positive offsets: the canvas cuts the mosaic's left and top, its right edge lies inside a tile
    "mosaic cut": (1024, 192, 682, 192, geometry(1024, 192)[2], (700, 222, 37, 13)),
    # a mosaic narrower than one tile, where the frame is (the seam scan needs an overlap)
    "narrow mosaic": (1024, 192, 682, 192, geometry(1024, 192)[2], (50, 192, -400, 0)),
}
WANT = {"translation": lambda c: c[1] > 0 and c[2] == 0 and c[3] == 0, "64 patches": lambda c: c[1:] == (0, 1, 0), "65 patches": lambda c: c[1:] == (0, 0, 1),
        "skips": lambda c: c[1] > 0 and c[2] > 0 and c[3] > 0, "stretched": lambda c: c[3] > c[1] + c[2]}


def rule(name, px=4):
    cw, ch, fw, fh, p, _ = CASES[name]
    return R.classes(p, 0.0, 0.0, fw, fh, cw, ch, px)[0]


@pytest.fixture(scope="module")
def world(oracle):
    """Frames, mosaics and oracle outputs per (case, dtype, seed), computed once and left unchanged."""
    cache = {}

    def get(name, dtype=np.float32, seed=0):
        k = (name, np.dtype(dtype).name, seed)
        if k not in cache:
            cw, ch, fw, fh, p, (mw, mh, ox, oy) = CASES[name]
            F, M = oracle.synth(fw, fh, 2 * seed + 1, dtype), oracle.synth(mw, mh, 2 * seed, dtype)
            rc, out = oracle.pair(F, list(p), 0.0, 0.0, M, ox, oy, cw, ch, OPTS)
            assert rc == 0, (name, rc)
            for a in (F, M, out):
                a.setflags(write=False)
            cache[k] = (F, M, out)
        return cache[k]
    return get


@pytest.fixture
def make_plan(st, gpu, monkeypatch):
    made = []

    def make(cw, ch, max_pairs=2, env=PIN):
        for k in ("STITCH_NO_SRC_FUSE", "STITCH_SINGLE_FAST", "STITCH_MOVER"):
            monkeypatch.delenv(k, raising=False)
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        plan = st.capi.Plan(cw, ch, OPTS, max_pairs=max_pairs)
        made.append(plan)
        return plan
    yield make
    for p in made:
        p.close()


def tensor(a, gpu):
    import torch
    return torch.from_numpy(np.array(a)).to(gpu)


def same_bits(t, want):
    got = t.cpu().numpy()
    return got.dtype == want.dtype and got.shape == want.shape and np.array_equal(got.view(np.uint8), want.view(np.uint8))


def items_of(gpu, world, name, seeds, dtype=np.float32, p=None):
    import torch
    cw, ch, fw, fh, p0, (mw, mh, ox, oy) = CASES[name]
    its = []
    for s in seeds:
        F, M, _ = world(name, dtype, s)
        f = tensor(F, gpu)
        its.append((f, list(p or p0), 0.0, 0.0, tensor(M, gpu), ox, oy, torch.full((3, ch, cw), 77, dtype=f.dtype, device=gpu)))
    return its


def check(plan, its, world, name, seeds, dtype=np.float32):
    for i, s in enumerate(seeds):
        plan.status(i)
        assert same_bits(its[i][7], world(name, dtype, s)[2]), (name, "pair", i)


@pytest.mark.parametrize("name", sorted(CASES))
def test_two_pairs_equal_the_oracle_and_the_counts_the_rule(st, gpu, world, make_plan, name):
    cw, ch, fw, fh, p, _ = CASES[name]
    want = rule(name)
    assert WANT.get(name, lambda c: True)(want), (name, want)  # the case holds what it is there for, on the CPU first
    host, _ = st.capi.src_run_classes(p, 0.0, 0.0, fw, fh, cw, ch)
    assert host == want
    plan = make_plan(cw, ch)
    its = items_of(gpu, world, name, (0, 1))
    plan.pairs(its)
    check(plan, its, world, name, (0, 1))
    counts = plan.src_run_counts()
    print(name, counts)
    assert sum(counts) > 0, "the sweep was not handed the runs: the form is not k_vv_x_fwd<PX, true>"
    assert counts == want  # two pairs with one map share one set of arrays: each tile once
    assert plan.index_counts() == (1, 0, 1)


def test_fast_path_ran():
    """The cases together show tiles without patches and tiles with 1..64 of them (evaluated by the rule the counts are held to)."""
    assert rule("skips")[1] > 0 and rule("skips")[2] > 0


def test_byte_frames_are_general(st, gpu, world, make_plan):
    cw, ch, fw, fh, p, _ = CASES["skips"]
    want = rule("skips", 1)
    assert want[1] == 0 and want[2] == 0 and want[3] > 0
    assert st.capi.src_run_classes(p, 0.0, 0.0, fw, fh, cw, ch, 1)[0] == want
    plan = make_plan(cw, ch)
    its = items_of(gpu, world, "skips", (0, 1), np.uint8)
    plan.pairs(its)
    check(plan, its, world, "skips", (0, 1), np.uint8)
    assert plan.src_run_counts() == want


def test_lifecycle_of_the_arrays(st, gpu, world, make_plan, oracle):
    import torch
    cw, ch, fw, fh, p, (mw, mh, ox, oy) = CASES["skips"]
    want = rule("skips")
    plan = make_plan(cw, ch)
    its = items_of(gpu, world, "skips", (0, 1))
    its[1] = its[1][:1] + ([v + (1e-9 if j == 1 else 0.0) for j, v in enumerate(p)],) + its[1][2:]  # another key, the same offsets: a slot of its own
    assert R.classes(its[1][1], 0.0, 0.0, fw, fh, cw, ch)[0] == want
    refs = [world("skips", np.float32, 0)[2], world("skips", np.float32, 1)[2]]

    def run(what, idx, counts):
        for it in its:
            it[7].fill_(-3.0)
        plan.pairs(its)
        for i in range(2):
            plan.status(i)
            assert same_bits(its[i][7], refs[i]), (what, i)
        assert plan.index_counts() == idx, what
        assert plan.src_run_counts() == counts, what

    two = tuple(2 * v for v in want)
    run("first call", (2, 0, 0), two)
    run("same maps", (0, 2, 0), two)
    # pair 1's map changes (to one that moves the frame by 4 columns): only its slot is recomputed
    p2 = list(p)
    p2[3] -= 4.0
    F1, M1 = world("skips", np.float32, 1)[:2]
    rc, ref2 = oracle.pair(F1, p2, 0.0, 0.0, M1, ox, oy, cw, ch, OPTS)
    assert rc == 0
    its[1] = its[1][:1] + (p2,) + its[1][2:]
    refs[1] = ref2
    want2 = R.classes(p2, 0.0, 0.0, fw, fh, cw, ch)[0]
    mixed = tuple(a + b for a, b in zip(want, want2))
    run("one map changed", (1, 1, 0), mixed)
    plan.clear_fault()
    run("after clear_fault", (2, 0, 0), mixed)


def test_a_materialised_call_in_between_forgets_the_arrays(st, gpu, world, make_plan):
    """An output that overlaps an input sends a call of a source-fused plan through k_compose: the level-0 slots then hold planes, the
    records are dropped, and the next source-fused call writes every byte of the arrays again (they are garbage by then)."""
    import torch
    cw, ch, fw, fh, p, (mw, mh, ox, oy) = CASES["skips"]
    plan = make_plan(cw, ch)
    its = items_of(gpu, world, "skips", (0, 1))
    plan.pairs(its)
    assert plan.index_counts() == (1, 0, 1) and plan.src_run_counts() == rule("skips")
    buf = torch.empty(3 * ch * cw, dtype=torch.float32, device=gpu)
    frame = buf[:3 * fh * fw].view(3, fh, fw)
    frame.copy_(its[0][0])
    over = [(frame,) + its[0][1:7] + (buf.view(3, ch, cw),), its[1]]
    plan.pairs(over)
    plan.status(0)
    assert same_bits(over[0][7], world("skips", np.float32, 0)[2])
    assert plan.index_counts() == (0, 0, 0) and plan.src_run_counts() == (0, 0, 0, 0)
    plan.src_runs_fill(0xFF)
    for it in its:
        it[7].fill_(-3.0)
    plan.pairs(its)
    check(plan, its, world, "skips", (0, 1))
    assert plan.index_counts() == (1, 0, 1) and plan.src_run_counts() == rule("skips")


@pytest.mark.parametrize("byte", [0xFF, 0x00])
def test_stale_arrays_do_not_reach_the_output(st, gpu, world, make_plan, byte):
    cw, ch = CASES["skips"][:2]
    plan = make_plan(cw, ch)
    plan.src_runs_fill(byte)
    for name in ("skips",):
        its = items_of(gpu, world, name, (0, 1))
        plan.pairs(its)
        check(plan, its, world, name, (0, 1))
        assert plan.src_run_counts() == rule(name)


def test_a_captured_call_replays_on_new_frame_contents(st, gpu, world, make_plan):
    import torch
    cw, ch, fw, fh, p, (mw, mh, ox, oy) = CASES["skips"]
    plan = make_plan(cw, ch)
    its = items_of(gpu, world, "skips", (0, 1))
    s, g = torch.cuda.Stream(), torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        plan.pairs(its)  # warm: nothing is allocated or compiled inside the capture
        torch.cuda.synchronize()
        with torch.cuda.graph(g, stream=s):
            plan.pairs(its)
    for seeds in ((2, 3), (0, 2)):
        for it, sd in zip(its, seeds):
            F, M, _ = world("skips", np.float32, sd)
            it[0].copy_(tensor(F, gpu))
            it[4].copy_(tensor(M, gpu))
            it[7].fill_(-1.0)
        torch.cuda.synchronize()
        with torch.cuda.stream(s):
            g.replay()
        torch.cuda.synchronize()
        check(plan, its, world, "skips", seeds)
        assert plan.src_run_counts() == rule("skips")
