"""G column flags (csrc/k_compose.inc, g_cols) in every kernel that reads them, at the shapes tests/test_gpu_g_flags.py leaves out:
levels whose producing level has an odd count of tile columns, every collapse implementation (k_collapse4's two column ranges,
k_collapse, k_collapse_px) with set flags of its own and of the coarser level, more than 64 row bands, planes that are +0 from edge
to edge, calls smaller than the plan's capacity, the dense blend, and replays of a captured launch sequence whose zero regions move.
Every test makes several calls on ONE plan with the zero regions moved between them, so that a reader which loads a flagged --
unstored -- column sees an earlier call's data.  Outputs and seams are compared with the oracle bit for bit, Plan.g_flag_counts()
with the rule (tests/g_flags_ref.py) evaluated on the oracle's planes, and the rule's counts must be above zero at every level a
case is there for."""
import numpy as np
import pytest

from g_flags_ref import BATCHES, FORMS, OPTS, cases, flagged_columns

pytestmark = pytest.mark.gpu

# the black channel of (frames, mosaics): such a plane is +0 at every level, flagged from edge to edge.  Channel 0 stays: it is
# what the seam scan reads, and a black one has no seam
BLACK = {"k21": (2, 1), "k12": (1, 2)}


@pytest.fixture(scope="module")
def refs(oracle):
    """Inputs, oracle output, oracle seam and the rule's counts (with and without the exception for a ragged producing level) of every
    case, computed once per (canvas, pixel type, variant).  variant: None, or a key of BLACK."""
    cache = {}

    def get(cw, ch, dtype, variant=None):
        key = (cw, ch, np.dtype(dtype).name, variant)
        if key not in cache:
            out = {}
            for i, (name, (fw, P, mw, ox, branch)) in enumerate(cases(cw).items()):
                F, M = oracle.synth(fw, ch, 2 * i + 1, dtype), oracle.synth(mw, ch, 2 * i, dtype)
                if variant:
                    F[BLACK[variant][0]] = 0
                    M[BLACK[variant][1]] = 0
                rc, ref = oracle.pair(F, P, 0.0, 0.0, M, ox, 0, cw, ch, OPTS)
                assert rc == 0, (name, rc)
                a, b = oracle.warp(F, P, 0.0, 0.0, cw, ch), oracle.move(M, ox, 0, cw, ch)
                rcs, seam = oracle.seam(a, b)
                assert rcs == 0 and seam.branch == branch, (name, seam.as_tuple())
                ref.setflags(write=False)
                out[name] = dict(name=name, F=F, P=P, M=M, ox=ox, ref=ref, seam=seam.as_tuple(), a=a, b=b,
                                 counts=flagged_columns(oracle, a, b), documented=flagged_columns(oracle, a, b, ragged_exception=False))
            cache[key] = out
        return cache[key]
    return get


def expected(recs, key="counts"):
    return tuple(sum(r[key][lv] for r in recs) for lv in range(2))


def same_bits(got, ref):
    return np.array_equal(got.cpu().numpy().view(np.uint8), ref.view(np.uint8))


def run_calls(capi, gpu, calls, cw, ch, max_pairs=2, with_plan=None):
    """calls: one list of records per call, all through one plan.  After every call: each output and seam against the oracle, the
    plan's counts against the rule for the pairs of that call.  Returns the expected counts of every call."""
    import torch
    plan = capi.Plan(cw, ch, capi.BlendOpts(**OPTS), max_pairs=max_pairs)
    if with_plan:
        with_plan(plan)
    wants = []
    for call, recs in enumerate(calls):
        items = [(torch.from_numpy(r["F"]).to(gpu), r["P"], 0.0, 0.0, torch.from_numpy(r["M"]).to(gpu), r["ox"], 0,
                  torch.empty((3, ch, cw), dtype=torch.from_numpy(r["F"]).dtype, device=gpu)) for r in recs]
        outs = plan.pairs(items)
        names = [r["name"] for r in recs]
        for slot, r in enumerate(recs):
            assert plan.status(slot).as_tuple() == r["seam"], (call, names[slot])
            assert same_bits(outs[slot], r["ref"]), (call, names[slot], cw, ch)
        got, want = plan.g_flag_counts(), expected(recs)
        print("call", call, names, "flagged tile columns (level 1, level 2)", got, "rule on the oracle's planes", want,
              "rule without the ragged-level exception", expected(recs, "documented"))
        assert got == want, (call, got, want)
        wants.append(want)
    plan.close()
    return wants


def set_env(monkeypatch, form, extra=None):
    for k, v in {**FORMS[form], "STITCH_SINGLE_FAST": "1", **(extra or {})}.items():
        monkeypatch.setenv(k, v)


def batches(R, which=BATCHES):
    return [[R[n] for n in names] for names in which]


def black_calls(refs, cw, ch, dtype):
    """Four calls with a black channel 2 of the frames and channel 1 of the mosaics, or the other way round, on alternating batches:
    every such plane is flagged from edge to edge in one call and stored in the next."""
    A, B = refs(cw, ch, dtype, "k21"), refs(cw, ch, dtype, "k12")
    return [[A[n] for n in BATCHES[0]], [B[n] for n in BATCHES[1]], [B[n] for n in BATCHES[0]], [A[n] for n in BATCHES[1]]]


def all_calls(refs, cw, ch, dtype):
    """The two coloured batches, then black_calls.  Where a coloured image is absent the blend's mask gives its planes the weight 0, so
    data read in place of a flagged column shows only near the seam; a black channel is flagged where its image has the weight 1."""
    return batches(refs(cw, ch, dtype)) + black_calls(refs, cw, ch, dtype)


# 1088 x 136: 17 tile columns at level 0, 9 (8.5) at level 1, 5 (4.25) at level 2; 1152 x 192: 18, 9, 5 (4.5).  The workgroup of
# k_vv_y_bwd_dec that produces a level's last tile column reads a second input tile column that does not exist where the producing
# level has an odd count of them; it then neither takes the all-zero path nor is it a zero neighbour, so the level's last two tile
# columns are never flagged (they are stored and read: exact, only not skipped).  g_flags_ref.flagged_in_level has that exception.
@pytest.mark.parametrize("form", sorted(FORMS))
@pytest.mark.parametrize("dtype", [np.float32, np.uint8])
@pytest.mark.parametrize("cw,ch", [(1088, 136), (1152, 192)])
def test_levels_produced_from_an_odd_count_of_tile_columns(st, gpu, refs, cw, ch, dtype, form, monkeypatch):
    """What the counter returns on the MI355X for the two coloured calls: (27, 3) at 1088 x 136 and (36, 6) at 1152 x 192, the rule WITH
    the exception; the rule without it gives (33, 9) and (36, 12)."""
    from computervisionimagestich2_amd import capi
    set_env(monkeypatch, form)
    calls = all_calls(refs, cw, ch, dtype)
    for recs in calls:  # the shapes are here because the two statements of the rule part on them
        assert expected(recs) != expected(recs, "documented"), (expected(recs), expected(recs, "documented"))
    for want in run_calls(capi, gpu, calls, cw, ch):
        assert want[0] > 0 and want[1] > 0, want


# 1020 x 192: levels of 510 and 255 columns.  Level 2 has no four-column range: k_collapse_px with its own flags.  Level 1 runs
# k_collapse4's four-column part on [0, 256) and collapse_cols1 on the other 254 columns, with level 2's flags as the coarser level.
@pytest.mark.parametrize("form", sorted(FORMS))
@pytest.mark.parametrize("dtype", [np.float32, np.uint8])
def test_collapse_px_and_the_one_column_part_see_set_flags(st, gpu, refs, dtype, form, monkeypatch):
    from computervisionimagestich2_amd import capi
    set_env(monkeypatch, form)
    cw, ch = 1020, 192

    def ranges(plan):
        assert plan.level_w[1:3] == [510, 255]
        assert plan.collapse_range(2)[0] == plan.collapse_range(2)[1]
        assert plan.collapse_range(1)[:2] == (0, 256)
    wants = run_calls(capi, gpu, all_calls(refs, cw, ch, dtype), cw, ch, with_plan=ranges)
    assert wants == 2 * [(30, 6)] + 4 * [(52, 20)], wants  # 15 and 3 per coloured pair, 26 and 10 with a black channel


# what each setting reaches (run_collapse, stitch_hip.hip); the pixel types it is run with
SETTINGS = {
    "px_off": ({"STITCH_COLLAPSE_PX": "0"}, "fu"),  # k_collapse<float, false> at level 2 of the 1020-wide canvas
    # k_collapse<OUT, true> at level 0 with the coarser level's flags; levels this small then take k_collapse_px at levels 1 and 2 ...
    "c4_off": ({"STITCH_COLLAPSE4": "0"}, "fu"),
    "c4_px_off": ({"STITCH_COLLAPSE4": "0", "STITCH_COLLAPSE_PX": "0"}, "fu"),  # ... and k_collapse at every level with both off
    "c4_fixed": ({"STITCH_C4_GEN": "0"}, "f"),  # the fixed-pattern k_collapse4, whose range starts at 256
    "lockstep2": ({"STITCH_C4_LOCKSTEP": "2"}, "f"),  # the shared mask sample
    "crows": ({"STITCH_CROWS_LN": "5", "STITCH_CROWS_L0": "3"}, "f"),  # strips that divide no level height
    "swizzle_off": ({"STITCH_C4_SWIZZLE": "0"}, "f"),
}


@pytest.mark.parametrize("setting,dtype", [(s, d) for s, (_, types) in SETTINGS.items()
                                           for d in ([np.float32, np.uint8] if "u" in types else [np.float32])])
@pytest.mark.parametrize("cw,ch,form", [(1020, 192, "fused3"), (1280, 136, "fused2")])
def test_every_collapse_implementation_with_set_flags(st, gpu, refs, cw, ch, form, setting, dtype, monkeypatch):
    from computervisionimagestich2_amd import capi
    set_env(monkeypatch, form, SETTINGS[setting][0])
    for want in run_calls(capi, gpu, all_calls(refs, cw, ch, dtype), cw, ch):
        assert want[0] > 0 and want[1] > 0, want


def test_neighbour_test_above_64_bands(st, gpu, refs, monkeypatch):
    """1024 x 4224: 66 row bands at level 0, 33 at level 1: the producer's neighbour test gathers the input flags in two rounds of 64
    bands.  16 and 8 tile columns: the exception for a ragged level plays no part."""
    from computervisionimagestich2_amd import capi
    set_env(monkeypatch, "fused3")
    cw, ch = 1024, 4224
    R = refs(cw, ch, np.float32)
    for want in run_calls(capi, gpu, batches(R), cw, ch):
        assert want == (30, 6), want


@pytest.mark.parametrize("dtype", [np.float32, np.uint8])
@pytest.mark.parametrize("cw", [1024, 1020])
def test_planes_of_zeros_from_edge_to_edge(st, gpu, refs, cw, dtype, monkeypatch):
    """A black channel 2 of the frames and channel 1 of the mosaics, then the other way round: the whole plane is flagged at both
    levels, edges included (k_vv_x_fwd starts in a flagged tile and takes a zero sample behind the last one), and in the next call the
    same plane is stored over memory that no call has written."""
    from computervisionimagestich2_amd import capi
    set_env(monkeypatch, "fused3")
    ch = 192
    for want in run_calls(capi, gpu, black_calls(refs, cw, ch, dtype), cw, ch):
        assert want == (52, 20), want  # 26 and 10 per pair: the 15 and 3 of the coloured cases, and every tile column of the black planes


def test_calls_smaller_than_the_plan(st, gpu, refs, monkeypatch):
    """A plan for four pairs, calls of three, two and one: the collapse finds its zeros behind the plan's LAST plane whatever the call's
    size (behind the call's last plane lies a pair of an earlier call), and the counter covers the pairs of the last call only.  With
    a black channel, so that a flagged plane's samples carry the weight 1 somewhere."""
    from computervisionimagestich2_amd import capi
    set_env(monkeypatch, "fused3")
    cw, ch = 1024, 192
    A, B = refs(cw, ch, np.float32, "k21"), refs(cw, ch, np.float32, "k12")
    calls = [[A["frame_right"], A["mosaic_left"], A["frame_left"]], [B["frame_left"], B["mosaic_right"]], [A["mosaic_left"]]]
    wants = run_calls(capi, gpu, calls, cw, ch, max_pairs=4)
    assert wants == [(78, 30), (52, 20), (26, 10)], wants


@pytest.mark.parametrize("dtype", [np.float32, np.uint8])
def test_dense_blend_with_set_flags(st, gpu, refs, oracle, dtype, monkeypatch):
    """Plan.blend on the canvases the oracle's warp and move make of the same cases (a_dense: level 0's k_collapse4<.., true, true> with
    the coarser level's flags), the zero regions moved from call to call."""
    import torch
    from computervisionimagestich2_amd import capi
    set_env(monkeypatch, "fused3")
    cw, ch = 1024, 192
    R = refs(cw, ch, dtype)
    plan = capi.Plan(cw, ch, capi.BlendOpts(**OPTS), max_pairs=1)
    for name in ("frame_right", "frame_left", "mosaic_left", "mosaic_right"):
        r = R[name]
        rc, ref, seam = oracle.blend(r["a"], r["b"], OPTS)
        assert rc == 0 and seam.as_tuple() == r["seam"], (name, rc)
        out = plan.blend(torch.from_numpy(r["a"]).to(gpu), torch.from_numpy(r["b"]).to(gpu))
        assert plan.status(0).as_tuple() == r["seam"], name
        assert same_bits(out, ref), name
        got, want = plan.g_flag_counts(), tuple(r["counts"])
        print(name, "flagged tile columns (level 1, level 2)", got, "rule on the oracle's planes", want)
        assert want[0] > 0 and want[1] > 0, want
        assert got == want, (name, got, want)
    plan.close()


def test_captured_sequence_whose_zero_regions_move_between_replays(st, gpu, refs, monkeypatch):
    """One launch sequence captured into a graph, its geometry fixed; between replays the black channel moves from channel 2 to
    channel 1 and back, so a plane that one replay flags from edge to edge is stored by the next.  Every replay gives the oracle's
    bits and the counts of the contents just loaded."""
    import torch
    from computervisionimagestich2_amd import capi
    set_env(monkeypatch, "fused3")
    cw, ch, names = 1024, 192, BATCHES[0]
    V = {v: refs(cw, ch, np.float32, v) for v in (None, "k21", "k12")}
    plan = capi.Plan(cw, ch, capi.BlendOpts(**OPTS), max_pairs=2)
    items = [(torch.zeros(V[None][n]["F"].shape, dtype=torch.float32, device=gpu), V[None][n]["P"], 0.0, 0.0,
              torch.zeros(V[None][n]["M"].shape, dtype=torch.float32, device=gpu), V[None][n]["ox"], 0,
              torch.empty((3, ch, cw), dtype=torch.float32, device=gpu)) for n in names]

    def load(variant):
        for it, n in zip(items, names):
            it[0].copy_(torch.from_numpy(V[variant][n]["F"]))
            it[4].copy_(torch.from_numpy(V[variant][n]["M"]))
            it[7].fill_(-1.0)
        torch.cuda.synchronize()
        return [V[variant][n] for n in names]

    load(None)
    s, g = torch.cuda.Stream(), torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        plan.pairs(items)  # warm: nothing is allocated or compiled inside the capture
        torch.cuda.synchronize()
        with torch.cuda.graph(g, stream=s):
            plan.pairs(items)
    for rep, variant in enumerate(("k21", "k12", "k21", "k12")):
        recs = load(variant)
        with torch.cuda.stream(s):
            g.replay()
        torch.cuda.synchronize()
        for slot, r in enumerate(recs):
            assert plan.status(slot).as_tuple() == r["seam"], (rep, slot)
            assert same_bits(items[slot][7], r["ref"]), (rep, variant, slot)
        got, want = plan.g_flag_counts(), expected(recs)
        print("replay", rep, variant, "flagged tile columns (level 1, level 2)", got, "rule on the oracle's planes", want)
        assert want == (52, 20), want
        assert got == want, (rep, got, want)
    plan.close()
