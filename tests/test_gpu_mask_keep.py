"""The mask pyramid a plan keeps per slot while the slot's seam record repeats (csrc/k_compose.inc, MaskKey and k_mask_keys;
csrc/stitch_call_form.h, mask_keep_word; include/stitch_mask_keep.h): a call of the batch forms leaves the mask planes of G_1 .. and
their row-repeat flags as an earlier call of the same form wrote them, and every kernel between two levels drops the work of such a
plane.  Every output and seam is compared with the oracle bit for bit, Plan.mask_keep_counts() with (computed, stood) as the sequence
of calls implies, and no call may leave a hand-off time-out behind.

Canvases 1024 x 768 and 1088 x 392 with the forms of tests/g_flags_ref.py pinned (tests/test_gpu_mask_rows.py: flags and fused forms
at both levels, partial last bands, heights that are no multiple of the row chunk); 1024 x 1024 where a call of one pair takes another
form than a call of two; 203 x 139 for the smallest default-switch source-fused call (tests/test_gpu_index_plane.py)."""
import numpy as np
import pytest

from g_flags_ref import BATCHES, FORMS, OPTS, cases, shift

pytestmark = pytest.mark.gpu

SIZES = [(1024, 768), (1088, 392)]


@pytest.fixture(scope="module")
def refs(oracle):
    """Per (canvas, pixel type): every case of g_flags_ref.cases with its inputs, the oracle's output and seam -- and `new`, the same
    geometry with other contents, whose seam the fixture shows to be the same.  Computed once, left unchanged."""
    cache = {}

    def one(name, fw, P, mw, ox, branch, seeds, cw, ch, dtype):
        F, M = oracle.synth(fw, ch, seeds[0], dtype), oracle.synth(mw, ch, seeds[1], dtype)
        for img in (F, M):
            img[0] = np.maximum(img[0], 1)  # channel 0 is what the seam scan reads: covered wherever the image is
        rc, ref = oracle.pair(F, P, 0.0, 0.0, M, ox, 0, cw, ch, OPTS)
        assert rc == 0, (name, rc)
        rcs, seam = oracle.seam(oracle.warp(F, P, 0.0, 0.0, cw, ch), oracle.move(M, ox, 0, cw, ch))
        assert rcs == 0 and seam.branch == branch, (name, seam.as_tuple())
        for a in (F, M, ref):
            a.setflags(write=False)
        return dict(name=name, F=F, P=P, M=M, ox=ox, ref=ref, seam=seam.as_tuple())

    def get(cw, ch, dtype, new=False):
        key = (cw, ch, np.dtype(dtype).name, new)
        if key not in cache:
            out = {}
            for i, (name, (fw, P, mw, ox, branch)) in enumerate(cases(cw).items()):
                out[name] = one(name, fw, P, mw, ox, branch, (2 * i + 11, 2 * i + 10) if new else (2 * i + 1, 2 * i), cw, ch, dtype)
            cache[key] = out
        return cache[key]
    return get


def tensor(a):
    import torch
    return torch.from_numpy(np.array(a))


def same_bits(got, ref):
    return np.array_equal(got.cpu().numpy().view(np.uint8), ref.view(np.uint8))


def items_of(gpu, recs, cw, ch):
    import torch
    return [(tensor(r["F"]).to(gpu), r["P"], 0.0, 0.0, tensor(r["M"]).to(gpu), r["ox"], 0,
             torch.empty((3, ch, cw), dtype=tensor(r["F"]).dtype, device=gpu)) for r in recs]


def call(plan, gpu, recs, what, seams=None, check=None):
    """One call of the records' pairs; every output and seam against the oracle (check = False for a pair: its output is the
    caller's to compare), no time-out; -> the plan's (computed, stood)."""
    cw, ch = plan.cw, plan.ch
    outs = plan.pairs(items_of(gpu, recs, cw, ch), seams=seams)
    for slot, r in enumerate(recs):
        if check is None or check[slot]:
            assert plan.status(slot).as_tuple() == r["seam"], (what, slot, r["name"])  # (raises on a hand-off time-out)
            assert same_bits(outs[slot], r["ref"]), (what, slot, r["name"])
        else:
            plan.status(slot)
    counts = plan.mask_keep_counts()
    print(what, [r["name"] for r in recs], "mask pyramids (computed, stood):", counts)
    assert sum(counts) == len(recs)
    return counts, outs


@pytest.fixture
def make_plan(st, gpu, monkeypatch):
    """-> make(cw, ch, env, max_pairs): a plan under FORMS-style switches; closed at the end of the test."""
    from computervisionimagestich2_amd import capi
    made = []

    def make(cw, ch, env, max_pairs=2, opts=OPTS, masked=False):
        for k, v in {"STITCH_SINGLE_FAST": "1", **env}.items():
            monkeypatch.setenv(k, v)
        p = capi.Plan(cw, ch, capi.BlendOpts(**opts), max_pairs=max_pairs, **({"masked": True} if masked else {}))
        made.append(p)
        return p
    yield make
    for p in made:
        p.close()


@pytest.mark.parametrize("form", sorted(FORMS))
@pytest.mark.parametrize("dtype", [np.float32, np.uint8])
@pytest.mark.parametrize("cw,ch", SIZES)
def test_the_same_pairs_again_and_with_new_contents(gpu, refs, make_plan, cw, ch, dtype, form):
    plan = make_plan(cw, ch, FORMS[form])
    assert plan.mask_keep_form(2), "the pinned batch forms know the skip"
    R, N = refs(cw, ch, dtype), refs(cw, ch, dtype, new=True)
    a, b = BATCHES[0]
    assert (N[a]["seam"], N[b]["seam"]) == (R[a]["seam"], R[b]["seam"]), "new contents, the seams where they were"
    assert call(plan, gpu, [R[a], R[b]], "first")[0] == (2, 0)
    rows = plan.mask_row_counts()  # what the computing call recorded ...
    assert rows[0] > 0 and rows[1] > 0
    assert call(plan, gpu, [R[a], R[b]], "again")[0] == (0, 2)
    assert plan.mask_row_counts() == rows  # ... is what a standing call still reports: the flags that stand
    assert call(plan, gpu, [N[a], N[b]], "new contents")[0] == (0, 2)
    assert plan.mask_row_counts() == rows


@pytest.mark.parametrize("form", sorted(FORMS))
@pytest.mark.parametrize("dtype", [np.float32, np.uint8])
@pytest.mark.parametrize("cw,ch", SIZES)
def test_seams_that_move_recompute_exactly_their_slots(gpu, refs, make_plan, cw, ch, dtype, form):
    """g_flags_ref.BATCHES back and forth (tests/test_gpu_mask_rows.py, moving_seam): both records change in every call.  Then one
    slot alone changes, and a pair moves from slot 0 to slot 1: records are per slot."""
    plan = make_plan(cw, ch, FORMS[form])
    R = refs(cw, ch, dtype)
    for k, names in enumerate((BATCHES[0], BATCHES[1], BATCHES[0])):
        assert call(plan, gpu, [R[n] for n in names], f"call {k}")[0] == (2, 0)
    fr, ml = BATCHES[0]
    assert R[BATCHES[1][1]]["seam"] != R[ml]["seam"] and R[fr]["seam"] != R[ml]["seam"]
    assert call(plan, gpu, [R[fr], R[BATCHES[1][1]]], "slot 1 alone changes")[0] == (1, 1)
    assert call(plan, gpu, [R[fr], R[ml]], "and back")[0] == (1, 1)
    assert call(plan, gpu, [R[ml], R[fr]], "the pairs swap slots")[0] == (2, 0)
    assert call(plan, gpu, [R[ml], R[fr]], "again")[0] == (0, 2)


@pytest.mark.parametrize("dtype", [np.float32, np.uint8])
def test_given_seams(gpu, refs, make_plan, dtype):
    """stitch_dev_pairs_seamed_*: the oracle's own integers give the oracle's bits; the same integers twice stand, one integer changed
    recomputes that slot -- whose output is compared with a fresh plan's, which computes everything."""
    cw, ch = SIZES[1]
    R = refs(cw, ch, dtype)
    recs = [R[n] for n in BATCHES[0]]
    seams = [r["seam"] for r in recs]
    plan = make_plan(cw, ch, FORMS["fused3"])
    assert call(plan, gpu, recs, "given", seams)[0] == (2, 0)
    assert call(plan, gpu, recs, "the same integers", seams)[0] == (0, 2)
    s1 = list(seams[1])
    s1[2] -= 16 * s1[3]  # the overlap's mean column, and with it the step, moves 16 columns to the left
    moved = [seams[0], tuple(s1)]
    counts, outs = call(plan, gpu, recs, "one integer changed", moved, check=[True, False])
    assert counts == (1, 1)
    assert plan.status(1).as_tuple()[:4] == tuple(s1[:4])
    fresh = make_plan(cw, ch, FORMS["fused3"])
    c2, outs2 = call(fresh, gpu, recs, "fresh plan", moved, check=[True, False])
    assert c2 == (2, 0)
    assert same_bits(outs[1], outs2[1].cpu().numpy())
    assert call(plan, gpu, recs, "changed, again", moved, check=[True, False])[0] == (0, 2)


@pytest.mark.parametrize("dtype", [np.float32, np.uint8])
def test_a_call_of_another_form_neither_stands_nor_leaves_a_pyramid_to_stand(gpu, oracle, make_plan, dtype):
    """1024 x 1024, a plan for four pairs: two pairs take the fused sweep at level 0 and record the mask rows of level 1 (mr_out), one
    pair takes the separate sweeps and stores every row.  The call of one pair computes and takes slot 0 over under its own form; the
    call of two that follows computes slot 0 again and finds slot 1 standing."""
    cw = ch = 1024
    plan = make_plan(cw, ch, {"STITCH_MOVER": "0", "STITCH_SINGLE_FAST": "0"}, max_pairs=4)
    assert plan.mask_keep_form(2) and plan.mask_keep_form(1)  # both forms know the skip: what differs is what they store
    recs = []
    for i, name in enumerate(BATCHES[0]):
        fw, P, mw, ox, branch = cases(cw)[name]
        F, M = oracle.synth(fw, ch, 2 * i + 1, dtype), oracle.synth(mw, ch, 2 * i, dtype)
        for img in (F, M):
            img[0] = np.maximum(img[0], 1)
        rc, ref = oracle.pair(F, P, 0.0, 0.0, M, ox, 0, cw, ch, OPTS)
        assert rc == 0
        rcs, seam = oracle.seam(oracle.warp(F, P, 0.0, 0.0, cw, ch), oracle.move(M, ox, 0, cw, ch))
        assert rcs == 0
        recs.append(dict(name=name, F=F, P=P, M=M, ox=ox, ref=ref, seam=seam.as_tuple()))
    assert call(plan, gpu, recs, "two pairs")[0] == (2, 0)
    assert plan.mask_row_counts()[0] > 0, "the call of two records mask rows"
    assert call(plan, gpu, recs[:1], "one pair: another form")[0] == (1, 0)
    assert plan.mask_row_counts() == (0, 0)
    assert call(plan, gpu, recs, "two pairs again")[0] == (1, 1)
    assert call(plan, gpu, recs, "and again")[0] == (0, 2)


@pytest.mark.parametrize("dtype", [np.float32, np.uint8])
def test_clear_fault_forgets_and_a_dense_blend_takes_its_slot_over(gpu, refs, oracle, make_plan, dtype):
    """clear_fault: every slot is computed again.  A dense blend (one pair, slot 0, another seam) overwrites the blur scratch and the
    sweep states of every plane it has: slot 0 is computed again, slot 1 stands and gives the right bits."""
    cw, ch = SIZES[0]
    R = refs(cw, ch, dtype)
    recs = [R[n] for n in BATCHES[0]]
    plan = make_plan(cw, ch, FORMS["fused3"])
    assert call(plan, gpu, recs, "first")[0] == (2, 0)
    plan.clear_fault()
    assert call(plan, gpu, recs, "after clear_fault")[0] == (2, 0)
    assert call(plan, gpu, recs, "again")[0] == (0, 2)
    other = R[BATCHES[1][0]]
    a, b = oracle.warp(other["F"], other["P"], 0.0, 0.0, cw, ch), oracle.move(other["M"], other["ox"], 0, cw, ch)
    rc, want = oracle.blend(a, b, OPTS)[:2]
    assert rc == 0
    got = plan.blend(tensor(a).to(gpu), tensor(b).to(gpu))
    assert plan.status(0).as_tuple() == other["seam"] != recs[0]["seam"]
    assert same_bits(got, want)
    assert plan.mask_keep_counts()[0] == 1
    assert call(plan, gpu, recs, "after the dense blend")[0] == (1, 1)


def test_a_plan_without_the_implicit_mask_never_keeps(gpu, refs, make_plan):
    """STITCH_NO_FUSE=1: the level-0 mask is a stored plane that k_mask writes in every call; nothing stands."""
    cw, ch = SIZES[1]
    R = refs(cw, ch, np.float32)
    recs = [R[n] for n in BATCHES[0]]
    plan = make_plan(cw, ch, {"STITCH_NO_FUSE": "1"})
    assert not plan.mask_keep_form(2)
    for k in range(2):
        assert call(plan, gpu, recs, f"call {k}")[0] == (2, 0)


def test_the_smallest_default_switch_source_fused_call(gpu, oracle, make_plan):
    """203 x 139, three pairs, default switches but for STITCH_SINGLE_FAST=1 (tests/test_gpu_index_plane.py): no fused level, the
    separate sweeps in their few-workgroup forms (k_vv_x_m, k_vv_y_m, k_vv_y_bwd_dec7), all of which know the skip -- the pyramids
    stand.  Then the same form with fewer pairs and with all again: the records are per slot, whatever the call's size."""
    cw, ch = 203, 139
    fw = (2 * cw) // 3
    plan = make_plan(cw, ch, {}, max_pairs=3, opts=dict(sigma=2.0, blur_kind=0, level_rule=0, seam_rule=0))
    assert "source_fused" in plan.call_forms(3)
    recs = []
    for i in range(3):
        P = [1.0, 0.002, 1e-6, -float(cw - fw) - 8.0 * i, -0.001, 1.0, 5e-7, 1.5]
        F, M = oracle.synth(fw, ch, 2 * i + 1, np.float32), oracle.synth(fw, ch, 2 * i, np.float32)
        rc, ref = oracle.pair(F, P, 0.0, 0.0, M, 0, 0, cw, ch)
        assert rc == 0
        rcs, seam = oracle.seam(oracle.warp(F, P, 0.0, 0.0, cw, ch), oracle.move(M, 0, 0, cw, ch))
        assert rcs == 0
        recs.append(dict(name=f"pair{i}", F=F, P=P, M=M, ox=0, ref=ref, seam=seam.as_tuple()))
    assert plan.mask_keep_form(3) and plan.mask_keep_form(2)
    assert call(plan, gpu, recs[:2], "two of three")[0] == (2, 0)
    assert call(plan, gpu, recs, "all three")[0] == (1, 2)
    assert call(plan, gpu, recs, "again")[0] == (0, 3)
    assert call(plan, gpu, recs[:2], "two")[0] == (0, 2)
    assert call(plan, gpu, recs, "three")[0] == (0, 3)


def test_one_form_with_two_four_and_two_pairs(gpu, refs, make_plan):
    """The form word leaves out the number of pairs: planes and flags of a slot lie where they lie whatever the call's size.  Two pairs,
    four, two, four on one plan of a pinned form: only the slots a call sees for the first time are computed."""
    cw, ch = SIZES[1]
    R = refs(cw, ch, np.float32)
    four = [R[n] for n in BATCHES[0] + BATCHES[1]]
    plan = make_plan(cw, ch, FORMS["fused3"], max_pairs=4)
    assert call(plan, gpu, four[:2], "two")[0] == (2, 0)
    assert call(plan, gpu, four, "four")[0] == (2, 2)
    assert call(plan, gpu, four[:2], "two")[0] == (0, 2)
    assert call(plan, gpu, four, "four")[0] == (0, 4)


@pytest.mark.parametrize("dtype", [np.float32, np.uint8])
def test_a_captured_sequence_decides_on_every_replay(gpu, oracle, make_plan, dtype):
    """tests/test_gpu_mask_rows.py's captured sequence, one stream: the contents move the seam between replays.  Seam on the right,
    on the left, on the right again: every replay computes; a fourth replay with nothing changed stands."""
    import torch
    cw, ch = SIZES[0]
    plan = make_plan(cw, ch, FORMS["fused3"])

    def variant(seed, f_cols, m_cols, branch):
        F, M = oracle.synth(cw, ch, seed, dtype), oracle.synth(cw, ch, seed + 1, dtype)
        for img, (lo, hi) in ((F, f_cols), (M, m_cols)):
            img[0] = np.maximum(img[0], 1)
            img[:, :, :lo] = 0
            img[:, :, hi:] = 0
        rc, ref = oracle.pair(F, shift(0), 0.0, 0.0, M, 0, 0, cw, ch, OPTS)
        assert rc == 0
        rcs, seam = oracle.seam(oracle.warp(F, shift(0), 0.0, 0.0, cw, ch), oracle.move(M, 0, 0, cw, ch))
        assert rcs == 0 and seam.branch == branch, seam.as_tuple()
        return dict(F=F, M=M, ref=ref, seam=seam.as_tuple())
    left = [variant(1, (0, 300), (200, cw), 0), variant(3, (0, 280), (180, cw), 0)]
    right = [variant(5, (700, cw), (0, 800), 1), variant(7, (720, cw), (0, 820), 1)]
    items = [(torch.from_numpy(v["F"]).to(gpu), shift(0), 0.0, 0.0, torch.from_numpy(v["M"]).to(gpu), 0, 0,
              torch.empty((3, ch, cw), dtype=torch.from_numpy(v["F"]).dtype, device=gpu)) for v in left]
    s, g = torch.cuda.Stream(), torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        plan.pairs(items)  # warm: nothing is allocated or compiled inside the capture
        torch.cuda.synchronize()
        with torch.cuda.graph(g, stream=s):
            plan.pairs(items)
    for rep, (recs, want) in enumerate(((right, (2, 0)), (left, (2, 0)), (right, (2, 0)), (right, (0, 2)))):
        for it, v in zip(items, recs):
            it[0].copy_(torch.from_numpy(v["F"]))
            it[4].copy_(torch.from_numpy(v["M"]))
            it[7].fill_(7)
        torch.cuda.synchronize()
        with torch.cuda.stream(s):
            g.replay()
        torch.cuda.synchronize()
        for slot, v in enumerate(recs):
            assert plan.status(slot).as_tuple() == v["seam"], (rep, slot)
            assert same_bits(items[slot][7], v["ref"]), (rep, slot)
        got = plan.mask_keep_counts()
        print("replay", rep, "mask pyramids (computed, stood):", got)
        assert got == want, (rep, got, want)


@pytest.mark.parametrize("dtype", [np.float32, np.uint8])
def test_a_timed_out_handoff_leaves_no_pyramid_to_stand(st, gpu, oracle, make_plan, dtype):
    """A fused sweep whose hand-off waits give up (a spin limit of 0; the canvas and pairs of tests/test_gpu_benchpath.py, which are
    known to reach the limit) writes planes nobody may trust, and a healthy call may be queued right behind it, before anybody has
    seen the report: that call computes every slot, whatever the records say, and gives the oracle's bits.  After clear_fault the
    plan computes once more and keeps again."""
    fw, fh, cw, ch, B = 1408, 1024, 2048, 1024, 3
    plan = make_plan(cw, ch, {"STITCH_WAVEFRONT": "2", "STITCH_SINGLE_FAST": "0"}, max_pairs=B, opts=dict(sigma=2.0, blur_kind=0, level_rule=0, seam_rule=0))
    assert plan.mask_keep_form(B)
    recs = []
    for i in range(B):
        A, Bf = oracle.synth(fw, fh, 2 * i, dtype), oracle.synth(fw, fh, 2 * i + 1, dtype)
        for img in (A, Bf):
            img[0] = np.maximum(img[0], 1)
        P = [1.0, 0.002, 1e-6, -660.0 - 8.0 * i, -0.001, 1.0, 5e-7, 1.5]
        rc, ref = oracle.pair(Bf, P, 0.0, 0.0, A, 0, 0, cw, ch)
        assert rc == 0
        rcs, seam = oracle.seam(oracle.warp(Bf, P, 0.0, 0.0, cw, ch), oracle.move(A, 0, 0, cw, ch))
        assert rcs == 0
        recs.append(dict(name=f"pair{i}", F=Bf, P=P, M=A, ox=0, ref=ref, seam=seam.as_tuple()))
    assert call(plan, gpu, recs, "first")[0] == (B, 0)
    assert call(plan, gpu, recs, "again")[0] == (0, B)
    plan.clear_fault()  # (forgets: the call below computes, so that its mask bands wait for hand-offs like the others)
    plan.set_handoff_spin_limit(0)
    plan.pairs(items_of(gpu, recs, cw, ch))  # bands deep in the pipeline give up at their first check
    plan.set_handoff_spin_limit(1 << 20)
    outs = plan.pairs(items_of(gpu, recs, cw, ch))  # a healthy call queued behind it
    with pytest.raises(st.StitchError) as e:
        plan.status(0)
    assert e.value.code == st.capi.ERR_HIP and "timed out" in str(e.value)
    assert plan.mask_keep_counts() == (B, 0), "no record is trusted behind a time-out"
    for slot, r in enumerate(recs):
        assert same_bits(outs[slot], r["ref"]), slot
    plan.clear_fault()
    assert call(plan, gpu, recs, "after clear_fault")[0] == (B, 0)
    assert call(plan, gpu, recs, "again")[0] == (0, B)


@pytest.mark.parametrize("dtype", [np.float32, np.uint8])
def test_a_materialised_call_in_between_stands_and_leaves_standing(gpu, refs, make_plan, dtype):
    """The form word leaves out whether level 0 is evaluated from the frames: with the implicit mask the mask planes of G_1 .. do not
    depend on it.  A source-fused call, the same pairs materialised (the output of pair 0 starts where its frame starts, as in
    tests/test_gpu_index_plane.py: k_compose runs, no index plane), the first call again -- the pyramids the first call wrote serve all
    three, and all three give the oracle's bits."""
    cw, ch = SIZES[0]
    R = refs(cw, ch, dtype)
    recs = [R[n] for n in BATCHES[0]]
    plan = make_plan(cw, ch, FORMS["fused3"])
    assert "source_fused" in plan.call_forms(2)
    assert call(plan, gpu, recs, "source-fused")[0] == (2, 0)
    assert plan.index_counts() == (2, 0, 0)
    items = items_of(gpu, recs, cw, ch)
    F, out = recs[0]["F"], items[0][7]
    assert F.size <= out.numel()
    f = out.view(-1)[:F.size].view(F.shape)
    f.copy_(tensor(F))
    items[0] = (f,) + items[0][1:]
    outs = plan.pairs(items)
    for slot, r in enumerate(recs):
        assert plan.status(slot).as_tuple() == r["seam"], slot
        assert same_bits(outs[slot], r["ref"]), slot
    assert plan.index_counts() == (0, 0, 0), "the call in between was materialised"
    assert plan.mask_keep_counts() == (0, 2)
    assert call(plan, gpu, recs, "source-fused again")[0] == (0, 2)
    assert plan.index_counts() == (2, 0, 0)  # (the materialised call overwrote the index planes; the mask pyramids it left alone)


@pytest.mark.parametrize("dtype", [np.float32, np.uint8])
def test_pathed_calls_on_a_masked_plan_never_stand(gpu, refs, make_plan, dtype):
    """stitch_dev_pairs_pathed_* (tests/test_gpu_seam_path.py): k_mask_keys runs behind k_seam_pathed's zeroed records under a form
    word without keep_ok, and REDUCE is handed no words.  A path whose columns are all equal is the vertical seam, so the same paths
    twice give the oracle's bits twice, and nothing stands."""
    import seam_path_ref as sp
    from computervisionimagestich2_amd import capi
    cw, ch = SIZES[0]
    R = refs(cw, ch, dtype)
    recs = [R[n] for n in BATCHES[0]]
    plan = make_plan(cw, ch, FORMS["fused3"], masked=True)
    assert not plan.mask_keep_form(2) and plan.fused_sweep_levels >= 1
    paths, branches = [], []
    for r in recs:
        s = capi.Seam()
        s.sum_a_x, s.n_a, s.sum_ov_x, s.n_ov, s.branch, s.start = r["seam"]
        paths.append(tensor(sp.constant_path(s, OPTS["seam_rule"], ch)).to(gpu))
        branches.append(s.branch)
    for k in range(2):
        outs = plan.pairs(items_of(gpu, recs, cw, ch), paths=paths, branches=branches)
        for slot, r in enumerate(recs):
            assert plan.status(slot).as_tuple() == (0, 0, 0, 0, branches[slot], 0), (k, slot)
            assert same_bits(outs[slot], r["ref"]), (k, slot)
        assert plan.mask_keep_counts() == (2, 0), k
