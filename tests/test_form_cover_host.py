"""tests/form_cover.py's tables of cases held to its grid, on the host: tests/call_form_dump.cpp gives the record of every call of the
grid at default switches, form_cover.signatures what the launch code makes of each.  No GPU.

a  CASES and WIDE_CASES together reach every signature that any call of the grid reaches, without exemption; CASES alone every one
   that the calls of at most MAX_PIXELS reach;
b  every case reaches the signatures it is listed for, and every signature of the grid is listed by one case;
c  every case lies inside the grid, a case of CASES within its bound; a case of WIDE_CASES is there for signatures no smaller call reaches;
d  every case whose record has G column flags or mask-row flags has something flagged by the rules on the oracle's planes;
e  what the three full-size GPU tests reach beyond the grid is what tests/golden/form_cover_large.json records."""
import json
import os

import numpy as np
import pytest

import form_cover as FC
import form_cover_refs as R
from call_form_tool import build_dump, dump
from sift_ref import HERE

LARGE_GOLDEN = os.path.join(HERE, "golden", "form_cover_large.json")
CHUNK = 4000  # records parsed at a time


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return build_dump(tmp_path_factory.mktemp("form_cover"))


def signatures_of(exe, directory, cases):
    """One set of signature names per case (None: no valid pyramid)."""
    out = []
    for i in range(0, len(cases), CHUNK):
        recs = dump(exe, directory, [FC.dump_case(*c[:6]) for c in cases[i:i + CHUNK]])
        out += [None if r is None else FC.signatures(r) for r in recs]
    assert len(out) == len(cases)
    return out


@pytest.fixture(scope="module")
def grid_signatures(exe, tmp_path_factory):
    """Over EVERY call of the grid: option set -> the signatures it reaches; what the calls of at most MAX_PIXELS reach; the number
    of calls with a valid pyramid."""
    cases = list(FC.grid())
    per_opts, small, valid = {k: set() for k in FC.OPTION_SETS}, set(), 0
    for c, s in zip(cases, signatures_of(exe, tmp_path_factory.mktemp("grid"), cases)):
        if s is not None:
            valid += 1
            per_opts[c[5]] |= s
            if FC.small(c):
                small |= s
    return per_opts, small, valid


@pytest.fixture(scope="module")
def case_signatures(exe, tmp_path_factory):
    return signatures_of(exe, tmp_path_factory.mktemp("cases"), R.ALL_CASES)


def in_grid(case):
    cw, ch, cap, n, dense, opts = case[:6]
    return cw in FC.SIDES and ch in FC.SIDES and cap in FC.CAPS and n in (1, 2, cap) and n <= cap and opts in FC.OPTION_SETS and (not dense or n == 1)


def test_cases_reach_every_signature_of_the_grid(grid_signatures, case_signatures):
    per_opts, small, valid = grid_signatures
    assert valid > 50000  # (a grid that the dump refuses from end to end would be covered by nothing)
    assert all(s is not None for s in case_signatures)
    grid, reached = set().union(*per_opts.values()), set().union(*case_signatures)
    by_cases = set().union(*case_signatures[:len(FC.CASES)])
    print("signatures on the grid", len(grid), {k: len(v) for k, v in per_opts.items()}, "calls", valid, "; of calls within the bound", len(small),
          "; reached by the", len(FC.CASES), "cases", len(by_cases), "and with the", len(FC.WIDE_CASES), "wide cases", len(reached))
    assert reached == grid, (sorted(grid - reached), sorted(reached - grid))
    assert by_cases == small, (sorted(small - by_cases), sorted(by_cases - small))


def test_every_case_reaches_what_it_is_listed_for(grid_signatures, case_signatures):
    per_opts, small, _ = grid_signatures
    listed = set()
    for case, sigs in zip(R.ALL_CASES, case_signatures):
        assert case[6] and set(case[6]) <= sigs, (case[:6], sorted(set(case[6]) - sigs))
        assert not listed & set(case[6]), (case[:6], "a signature listed twice")
        if not FC.small(case):
            assert not small & set(case[6]), (case[:6], "a wide case listed for what a call within the bound reaches")
        listed |= set(case[6])
    assert listed == set().union(*per_opts.values())


def test_cases_lie_inside_the_grid():
    assert len(set(c[:6] for c in R.ALL_CASES)) == len(R.ALL_CASES)
    for case in R.ALL_CASES:
        assert in_grid(case), case[:6]
    for cw, ch, cap, n, dense, opts, _ in FC.CASES:
        assert max(cw, ch) <= FC.MAX_SIDE and cw * ch * n <= FC.MAX_PIXELS, (cw, ch, n)
    assert not [c[:6] for c in FC.WIDE_CASES if FC.small(c)]


def test_flagged_cases_have_something_flagged(oracle, exe, tmp_path):
    """A flagged form with nothing flagged tests nothing: for every case whose record has G column flags or mask-row flags, at each
    level where they are on, the rule counts something on the oracle's planes of the case's inputs -- before any GPU run.  Checked on
    the two placements of a call (slots 0 and 1, float: every further slot only adds to the call's count), call 2 only where call 1
    leaves a level at zero."""
    recs = dump(exe, tmp_path, [FC.dump_case(*c[:6]) for c in R.ALL_CASES])
    refs, flagged = R.References(oracle), 0
    for case, rec in sorted(zip(R.ALL_CASES, recs), key=lambda t: t[0][:6]):
        cw, ch, cap, n, dense, opts = case[:6]
        g_on, mr_on = R.flags_on(rec)
        if not any(g_on + mr_on):
            continue
        assert not dense and mr_on[0] <= g_on[0] and mr_on[1] <= g_on[1]
        flagged += 1
        counted = [False] * 4
        for call in range(2):
            pairs = [refs.pair(cw, ch, opts, np.float32, call, slot) for slot in range(min(n, 2))]
            _, _, want_g, want_mr = R.expected_counts(refs, rec, pairs, cw, ch)
            counted = [c or v > 0 for c, v in zip(counted, want_g + want_mr)]
            if [c for c, on in zip(counted, g_on + mr_on) if on].count(False) == 0:
                break
        assert not [i for i, on in enumerate(g_on + mr_on) if on and not counted[i]], (case[:6], g_on, mr_on, counted)
    print("cases with flags", flagged)
    assert flagged >= 30


def test_full_size_tests_reach_the_forms_above_the_grid(exe, tmp_path, grid_signatures):
    """The lone fused sweep (k_vv_xby_m, from 20 MPix per plane), one pair that fills the chip (the same sweep with zero-tile flags)
    and the levels of a 6144 x 4096 batch lie above the grid's bound; the three tests named in form_cover.LARGE run them."""
    grid = set().union(*grid_signatures[0].values())  # (every call of the grid)
    got = {}
    for test, cases in FC.LARGE.items():
        sigs = signatures_of(exe, tmp_path, cases)
        assert all(s is not None for s in sigs)
        got[test] = sorted(set().union(*sigs) - grid)
    with open(LARGE_GOLDEN) as f:
        want = json.load(f)
    assert got == want, "the fixture would now read:\n" + json.dumps(got, indent=1, sort_keys=True)
    config2, config5, batch = (got[k] for k in FC.LARGE)
    assert any(" xby " in s and " zt " not in s for s in config2)
    assert any(" xby " in s and " zt " in s for s in config5)
    assert batch
