"""Every launch form the pair path takes at DEFAULT switches (tests/form_cover.py: CASES and WIDE_CASES, held to the grid by
tests/test_form_cover_host.py), each at the smallest canvas that reaches it, against the oracle bit for bit.

Per case: an empty switch environment, ONE plan of the case's capacity, two calls of n pairs (or two dense blends) whose zero regions,
seam side and seam branch move between the calls -- a reader that takes a stale flag or an unstored tile sees the other call's data --
in float and, where level 0 is gathered from the frames or carries the implicit mask, in unsigned char as well.  Every output and
seam record equals the oracle's; the plan's accessors answer what the decision's record (tests/call_form_dump.cpp) says; where the record
has G column flags or mask-row flags the plan's counters equal the rules of tests/g_flags_ref.py and tests/mask_rows_ref.py evaluated
on the oracle's planes, and the rule counts something in at least one of the two calls."""
import os

import numpy as np
import pytest

import form_cover as FC
import switch_table as T
from form_cover_refs import ALL_CASES, References, build_records, case_id, expected_counts, pixel_types

pytestmark = pytest.mark.gpu

FAST_PATHS = ("implicit_mask", "source_fused", "fused_sweep", "zero_tiles", "fused_decimate", "coarse_levels")  # bits 0.. of stitch_plan_fast_paths


@pytest.fixture(scope="module")
def records(tmp_path_factory):
    return build_records(tmp_path_factory.mktemp("form_cover"))


@pytest.fixture(scope="module")
def refs(oracle):
    return References(oracle)


def same_bits(got, ref):
    return np.array_equal(got.cpu().numpy().view(np.uint8), ref.view(np.uint8))


def check_plan(plan, gpu, refs, rec, case):
    """The accessors of the case's plan against its record, then the two calls in every pixel type against the oracle."""
    import torch
    cw, ch, cap, n, dense, opts = case[:6]
    assert plan.fast_paths == {name for bit, name in enumerate(FAST_PATHS) if rec["fast_paths"] >> bit & 1}, (plan.fast_paths, rec["fast_paths"])
    l0 = rec["levels"][0] if rec["levels"] else None
    want_forms = ({"source_fused"} if rec["src"] else set()) | ({"fused_sweep"} if l0 and (l0["sweep"] == "batch" or l0["xby"]) else set())
    assert plan.call_forms(n) == want_forms, (plan.call_forms(n), want_forms)
    assert ("coarse_levels" in plan.fast_paths) == bool(rec["coarse"]) and plan.fused_sweep_levels == rec["wf_levels"] and plan.levels == rec["L"]
    for l, f in enumerate(rec["levels"]):  # the record is of this plan: its collapse ranges are the plan's
        assert plan.collapse_range(l) == (f["xa"], f["xb"], f["gen"]), (l, plan.collapse_range(l))

    counted = [False, False, False, False]
    for dtype in pixel_types(rec):
        for call in range(2):
            if dense:
                r = refs.dense(cw, ch, opts, dtype, call)
                out = plan.blend(torch.from_numpy(r["A"]).to(gpu), torch.from_numpy(r["B"]).to(gpu))
                assert plan.status(0).as_tuple() == r["seam"].as_tuple(), (np.dtype(dtype).name, call)
                assert same_bits(out, r["ref"]), (np.dtype(dtype).name, call)
                assert plan.g_flag_counts() == (0, 0) and plan.mask_row_counts() == (0, 0)
                continue
            recs = [refs.pair(cw, ch, opts, dtype, call, slot) for slot in range(n)]
            items = [(torch.from_numpy(r["F"]).to(gpu), r["P"], 0.0, 0.0, torch.from_numpy(r["M"]).to(gpu), r["ox"], 0,
                      torch.empty((3, ch, cw), dtype=torch.from_numpy(r["F"]).dtype, device=gpu)) for r in recs]
            outs = plan.pairs(items)
            for slot, r in enumerate(recs):
                assert plan.status(slot).as_tuple() == r["seam"].as_tuple(), (np.dtype(dtype).name, call, slot, r["name"])
                assert same_bits(outs[slot], r["ref"]), (np.dtype(dtype).name, call, slot, r["name"])
            g_on, mr_on, want_g, want_mr = expected_counts(refs, rec, recs, cw, ch)
            got_g, got_mr = plan.g_flag_counts(), plan.mask_row_counts()
            print(np.dtype(dtype).name, "call", call, "G column flags", got_g, "rule", want_g, "mask-row flags", got_mr, "rule", want_mr)
            assert got_g == want_g and got_mr == want_mr, (np.dtype(dtype).name, call, got_g, want_g, got_mr, want_mr)
            counted = [c or v > 0 for c, v in zip(counted, want_g + want_mr)]
    if not dense:  # a flagged form with nothing flagged tests nothing
        assert [c for c, on in zip(counted, g_on + mr_on) if on] == [True for on in g_on + mr_on if on], (g_on, mr_on, counted)


@pytest.mark.parametrize("index", range(len(ALL_CASES)), ids=[case_id(c) for c in ALL_CASES])
def test_default_form_against_oracle(st, gpu, oracle, records, refs, monkeypatch, index):
    from computervisionimagestich2_amd import capi
    cw, ch, cap, n, dense, opts = ALL_CASES[index][:6]
    names = list(T.SWITCHES) + list(T.EXEMPT)
    for k in names:
        monkeypatch.delenv(k, raising=False)
    assert not [k for k in names if k in os.environ]
    plan = capi.Plan(cw, ch, capi.BlendOpts(**FC.OPTION_SETS[opts]), max_pairs=cap)
    try:
        check_plan(plan, gpu, refs, records[index], ALL_CASES[index])
    finally:
        plan.close()
