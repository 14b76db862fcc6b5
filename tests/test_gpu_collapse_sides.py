"""GPU: the level-0 collapse that reads only the image the seam's step selects (csrc/k_pyramid.inc, k_collapse4 / collapse_cols4;
include/stitch_collapse_sides.h).  Every output is compared with the CPU oracle bit for bit -- tests/rig_seams_ref.py's blend_given
where the seam is given, Oracle.pair / Oracle.blend where it is the content's -- and Plan.collapse_sides() with the rule of
tests/collapse_sides_ref.py evaluated on the oracle's seam.

Canvases (level rule 1: these heights have a pyramid only under it): 1024 x 192, whole blocks; 1100 x 136, whose four-column range
ends at 1024 with columns behind it; 1021 x 70, an odd width and a height that is no multiple of the strip.  Seams are placed through
stitch_dev_pairs_seamed_*: the step at 1, 255, 256, 257, inside a block, at the end of the four-column range, at w - 1 and (branch 1)
past w.  A step at column 0 is reachable by no four integers (collapse_sides_ref.seam_for); stitch_dev_check_collapse_sides covers it."""
import numpy as np
import pytest

import collapse_sides_ref as cs
import rig_seams_ref as ref
from oracle_lib import ROOT_OPTS

pytestmark = pytest.mark.gpu

OPTS = dict(ROOT_OPTS, level_rule=1)
CANVASES = [(1024, 192), (1100, 136), (1021, 70)]
ENVS = {"source_fused": {"STITCH_SINGLE_FAST": "1"}, "materialised": {"STITCH_NO_SRC_FUSE": "1"}}


def geometry(cw, ch):
    """Frame = mosaic size and the map: the mosaic covers the left two thirds of the canvas, the warped frame the right two."""
    fw = (2 * cw) // 3
    return fw, ch, (1.0, 0.002, 1e-6, -float(cw - fw), -0.001, 1.0, 5e-7, 1.5)


def steps_of(cw, xa, xb):
    """[(branch, t)]: the mask is 1 on x < t (branch 0) or x >= t (branch 1)."""
    ts = sorted({1, 255, 256, 257, 256 + 130, xb - 1, xb, min(xb + 1, cw - 1), cw - 1})
    return [(0, t) for t in ts if 1 <= t <= cw - 1] + [(1, t) for t in ts + [cw] if 1 <= t <= cw]


def dark(F, k0, k1):
    """Channel 0 of the middle rows of the frame's columns k0 .. k1 - 1 set to 0: another content seam, the same footprint."""
    F = np.array(F)
    h = F.shape[1]
    F[0, h // 2 - 6: h // 2 + 7, k0:k1] = 0
    return F


@pytest.fixture(scope="module")
def world(oracle):
    """Inputs and oracle outputs, computed once per key and left unchanged."""
    cache = {}

    def keep(k, make):
        if k not in cache:
            v = make()
            for a in (v if isinstance(v, tuple) else (v,)):
                if isinstance(a, np.ndarray):
                    a.setflags(write=False)
            cache[k] = v
        return cache[k]

    class W:
        def frames(self, cw, ch, dtype, seed=0):
            fw, fh, _ = geometry(cw, ch)
            return keep(("F", cw, ch, np.dtype(dtype).name, seed), lambda: (oracle.synth(fw, fh, 2 * seed + 1, dtype), oracle.synth(fw, fh, 2 * seed, dtype)))

        def canvases(self, cw, ch, dtype, seed=0):
            F, M = self.frames(cw, ch, dtype, seed)
            return keep(("C", cw, ch, np.dtype(dtype).name, seed), lambda: (oracle.warp(F, list(geometry(cw, ch)[2]), 0.0, 0.0, cw, ch), oracle.move(M, 0, 0, cw, ch)))

        def given(self, cw, ch, dtype, four):
            a, b = self.canvases(cw, ch, dtype)
            return keep(("G", cw, ch, np.dtype(dtype).name, tuple(four)), lambda: ref.blend_given(oracle, a, b, OPTS, four))

        def content(self, cw, ch, F, M, tag):
            """-> (the oracle's output, the four integers of its seam) of frame F and mosaic M with the content seam."""
            def make():
                p = list(geometry(cw, ch)[2])
                rc, out = oracle.pair(F, p, 0.0, 0.0, M, 0, 0, cw, ch, OPTS)
                assert rc == 0
                rc, _, seam = oracle.blend(oracle.warp(F, p, 0.0, 0.0, cw, ch), oracle.move(M, 0, 0, cw, ch), OPTS)
                assert rc == 0
                return out, tuple(seam.as_tuple()[:4])
            return keep(("P", cw, ch, F.dtype.name, tag), make)
    return W()


def tensor(a, gpu):
    import torch
    return torch.from_numpy(np.array(a)).to(gpu)


def same_bits(t, want):
    got = t.cpu().numpy()
    return got.dtype == want.dtype and got.shape == want.shape and np.array_equal(cs.bits(got), cs.bits(want))


@pytest.fixture
def make_plan(st, gpu, monkeypatch):
    """-> make(env, cw, ch, max_pairs): a plan under the switches of ENVS[env], its level-0 four-column range; closed at the end."""
    made = []

    def make(env, cw, ch, max_pairs):
        for k in ("STITCH_NO_SRC_FUSE", "STITCH_SINGLE_FAST"):
            monkeypatch.delenv(k, raising=False)
        for k, v in ENVS[env].items():
            monkeypatch.setenv(k, v)
        plan = st.capi.Plan(cw, ch, OPTS, max_pairs=max_pairs)
        made.append(plan)
        assert "implicit_mask" in plan.fast_paths
        for n in range(1, max_pairs + 1):
            assert ("source_fused" in plan.call_forms(n)) == (env == "source_fused"), (env, n)
        xa, xb, _ = plan.collapse_range(0)
        assert xa % 256 == 0 and xb % 256 == 0 and xb - xa >= 512, (xa, xb)  # level 0 takes the four-column collapse, several blocks of it
        return plan, xa, xb
    yield make
    for p in made:
        p.close()


def call_given(plan, gpu, world, cw, ch, dtype, fours, xa, xb, what):
    """One stitch_dev_pairs_seamed_* call: pair i = the canvas's frames under seam fours[i]; outputs and counts checked; -> the counts."""
    import torch
    F, M = world.frames(cw, ch, dtype)
    f, m = tensor(F, gpu), tensor(M, gpu)
    p = list(geometry(cw, ch)[2])
    outs = [torch.full((3, ch, cw), 77, dtype=f.dtype, device=gpu) for _ in fours]
    plan.pairs([(f, p, 0.0, 0.0, m, 0, 0, o) for o in outs], seams=fours)
    counts = []
    for i, four in enumerate(fours):
        assert plan.status(i).as_tuple()[:4] == tuple(four)
        assert same_bits(outs[i], world.given(cw, ch, dtype, four)), (what, "pair", i, four)
        counts.append(plan.collapse_sides(i))
        assert counts[-1] == cs.counts_of(four, OPTS["seam_rule"], xa, xb), (what, "pair", i, four)
    print(what, [(ref.derive(four, 0)[:2], c) for four, c in zip(fours, counts)])
    return counts


@pytest.mark.parametrize("env", sorted(ENVS))
@pytest.mark.parametrize("dtype", [np.float32, np.uint8], ids=["f32", "u8"])
@pytest.mark.parametrize("cw,ch", CANVASES)
def test_given_seams_at_every_step_position(gpu, world, make_plan, cw, ch, dtype, env):
    plan, xa, xb = make_plan(env, cw, ch, 8)
    steps = steps_of(cw, xa, xb)
    nb = (xb - xa) // 256
    counts = {}
    for branch in (0, 1):  # one call per branch, up to eight seams in it
        mine = [s for s in steps if s[0] == branch]
        for o in range(0, len(mine), 8):
            fours = [cs.seam_for(b, t, cw) for b, t in mine[o:o + 8]]
            for s, c in zip(mine[o:o + 8], call_given(plan, gpu, world, cw, ch, dtype, fours, xa, xb, f"{env} branch {branch}")):
                counts[s] = c
    # what the cases are there for: nothing of a, nothing of b, a block boundary hit exactly, everything one-sided
    assert counts[(1, cw)] == (0, nb, 0)  # the step past w: every block reads b alone
    assert counts[(0, xb)] == (nb, 0, 0) if xb <= cw - 1 else counts[(0, cw - 1)][0] == nb - 1
    if xa == 0:
        assert counts[(0, 256)] == (1, nb - 1, 0) and counts[(1, 256)] == (nb - 1, 1, 0)  # the boundary itself: no block reads both
        assert counts[(0, 255)] == (0, nb - 1, 1) and counts[(0, 257)] == (1, nb - 2, 1)
    assert counts[(0, 256 + 130)][2] == 1 and counts[(1, 256 + 130)][2] == 1
    assert any(c[0] and c[1] for c in counts.values())
    # fewer pairs on the same plan with the seams moved: four, three, two, one
    moved = [cs.seam_for(b, t, cw) for b, t in ((0, 256 + 130), (1, 257), (1, cw), (0, 255))]
    for n in (4, 3, 2, 1):
        call_given(plan, gpu, world, cw, ch, dtype, moved[:n], xa, xb, f"{env} {n} pairs")
        moved = moved[1:] + moved[:1]


@pytest.mark.parametrize("env", sorted(ENVS))
@pytest.mark.parametrize("dtype", [np.float32, np.uint8], ids=["f32", "u8"])
@pytest.mark.parametrize("cw,ch", CANVASES)
def test_blend_of_two_canvases(gpu, world, make_plan, oracle, cw, ch, dtype, env):
    """stitch_blend_*: both images dense (no index plane), the content's seam."""
    plan, xa, xb = make_plan(env, cw, ch, 1)
    a, b = world.canvases(cw, ch, dtype)
    rc, want, seam = oracle.blend(a, b, OPTS)
    assert rc == 0
    got = plan.blend(tensor(a, gpu), tensor(b, gpu))
    four = plan.status().as_tuple()[:4]
    assert four == tuple(seam.as_tuple()[:4])
    assert same_bits(got, want)
    counts = plan.collapse_sides()
    assert counts == cs.counts_of(four, OPTS["seam_rule"], xa, xb)
    assert counts[0] > 0 and counts[1] > 0, counts  # the seam lies inside the range: blocks of either kind


@pytest.mark.parametrize("cw,ch", CANVASES)
def test_signed_zero_blocks_on_either_side_of_the_seam(gpu, world, make_plan, cw, ch):
    """float frames with blocks of -0.0 in the frame and in the mosaic, clear of the middle rows the seam scan reads."""
    plan, xa, xb = make_plan("source_fused", cw, ch, 2)
    F, M = (np.array(a) for a in world.frames(cw, ch, np.float32, seed=3))
    fw, fh, p = geometry(cw, ch)
    for img in (F, M):
        img[:, 2: fh // 2 - 10, 5: fw // 3] = -0.0
        img[:, fh // 2 + 10: fh - 1, fw // 2: fw - 7] = -0.0
        img[1, :, fw // 3: fw // 3 + 9] = -0.0
    want, four = world.content(cw, ch, F, M, "signed zeros")
    import torch
    outs = [torch.empty((3, ch, cw), dtype=torch.float32, device=gpu) for _ in range(2)]
    plan.pairs([(tensor(F, gpu), list(p), 0.0, 0.0, tensor(M, gpu), 0, 0, o) for o in outs])
    for i in range(2):
        assert plan.status(i).as_tuple()[:4] == four
        assert same_bits(outs[i], want), i
        counts = plan.collapse_sides(i)
        assert counts == cs.counts_of(four, OPTS["seam_rule"], xa, xb) and counts[0] > 0 and counts[1] > 0


@pytest.mark.parametrize("cw,ch", CANVASES[:2])
def test_a_captured_call_whose_seam_moves_between_replays(gpu, world, make_plan, cw, ch):
    """The form of a block is decided on the device from the seam record of the replay, not from the record of the capture."""
    import torch
    plan, xa, xb = make_plan("source_fused", cw, ch, 2)
    fw, fh, p = geometry(cw, ch)
    F0, M = world.frames(cw, ch, np.float32)
    variants = [("as synthesised", F0), ("columns 0 to 300 dark", dark(F0, 0, 300)), ("columns 100 to 400 dark", dark(F0, 100, 400))]
    refs = [world.content(cw, ch, F, M, what) for what, F in variants]
    rules = [cs.counts_of(four, OPTS["seam_rule"], xa, xb) for _, four in refs]
    assert len({four for _, four in refs}) == 3 and len(set(rules)) >= 2, (refs, rules)  # the seam moves, and across a block boundary
    items = [(torch.zeros((3, fh, fw), dtype=torch.float32, device=gpu), list(p), 0.0, 0.0, tensor(M, gpu), 0, 0,
              torch.empty((3, ch, cw), dtype=torch.float32, device=gpu)) for _ in range(2)]

    def load(k0, k1):
        for it, k in zip(items, (k0, k1)):
            it[0].copy_(tensor(variants[k][1], gpu))
            it[7].fill_(-1.0)
        torch.cuda.synchronize()

    def check(k0, k1, what):
        torch.cuda.synchronize()
        for i, k in enumerate((k0, k1)):
            assert plan.status(i).as_tuple()[:4] == refs[k][1], (what, i)
            assert same_bits(items[i][7], refs[k][0]), (what, i)
            assert plan.collapse_sides(i) == rules[k], (what, i)

    load(0, 0)
    s, g = torch.cuda.Stream(), torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        plan.pairs(items)  # warm: nothing is allocated or compiled inside the capture
        torch.cuda.synchronize()
        with torch.cuda.graph(g, stream=s):
            plan.pairs(items)
        for k0, k1 in ((1, 2), (2, 0), (0, 1)):
            load(k0, k1)
            g.replay()
            check(k0, k1, f"replay with variants {k0}, {k1}")


@pytest.mark.parametrize("w,h", [(512, 8), (1024, 64)])
@pytest.mark.parametrize("probe", [0, 1])
def test_one_sided_forms_against_the_full_arithmetic(st, gpu, w, h, probe):
    """stitch_dev_check_collapse_sides: k_collapse4's forms against k_collapse on synthetic planes; probe 1 has kept terms of +-0 under
    an E of -0 on both sides of the seam, where the row has to be redone with the dropped image."""
    for branch in (0, 1):
        for seam_x in (256, 300, 0, w):
            compared, bad, counts = st.capi.dev_check_collapse_sides(w, h, probe, branch, seam_x)
            assert compared == 3 * w * h and bad == 0, (branch, seam_x, bad)
            assert counts == cs.side_counts(branch, seam_x, float(seam_x), 0, w), (branch, seam_x)
            nb = w // 256
            if seam_x == 256:
                assert counts == ((1, nb - 1, 0) if branch == 0 else (nb - 1, 1, 0))
            if seam_x == 300:
                assert counts[2] == 1 and counts[branch] == 1 and counts[1 - branch] == nb - 2
            if seam_x in (0, w):
                assert counts == ((nb, 0, 0) if (seam_x == 0) == (branch == 1) else (0, nb, 0))
