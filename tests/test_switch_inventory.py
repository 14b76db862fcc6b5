"""CPU: the runtime switches the library reads are the ones tests/switch_table.py lists.  A `getenv("STITCH_...")` added to
csrc/ without a table entry (and so without a test) or an exemption fails here."""
import importlib.util
import os
import re

import switch_table as T

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "computervisionimagestich2_amd", "csrc")
HEADER = os.path.join(ROOT, "include", "stitch.h")
READ = re.compile(r'\b(?:getenv|env_int)\s*\(\s*"(STITCH_[A-Z0-9_]+)"')


def switches_read(root=CSRC):
    """Every STITCH_* name that the sources under `root` read from the environment."""
    names = set()
    for dirpath, _, files in os.walk(root):
        for f in files:
            if f.endswith((".hip", ".inc", ".hpp", ".cpp", ".h")):
                with open(os.path.join(dirpath, f), encoding="utf-8") as fh:
                    names |= set(READ.findall(fh.read()))
    return names


def test_the_parser_sees_the_switches():
    names = switches_read()
    assert {"STITCH_WAVEFRONT", "STITCH_NO_FUSE", "STITCH_COPY_THREADS", "STITCH_BAND_PLAIN", "STITCH_D7_STAMP_MODE"} <= names
    assert len(names) >= 40, sorted(names)


def test_every_switch_read_is_in_the_table_or_exempt():
    missing = sorted(n for n in switches_read() if n not in T.SWITCHES and n not in T.EXEMPT)
    assert not missing, f"switches read in csrc/ without an entry in tests/switch_table.py (or an EXEMPT reason): {missing}"


def test_table_and_exemptions_are_disjoint_and_current():
    assert not set(T.SWITCHES) & set(T.EXEMPT)
    read = switches_read()
    stale = sorted(n for n in T.SWITCHES if n not in read)
    assert not stale, f"table entries that csrc/ no longer reads: {stale}"
    for name, reason in T.EXEMPT.items():
        assert reason.strip(), name


def test_every_table_entry_is_documented_in_the_header():
    with open(HEADER, encoding="utf-8") as fh:
        header = fh.read()
    undocumented = sorted(n for n in T.SWITCHES if not re.search(r"\b" + n + r"=", header))
    assert not undocumented, f"switches of tests/switch_table.py not documented in include/stitch.h: {undocumented}"


def test_table_entries_are_well_formed():
    forms = set(T.PAIR_FORMS) | {"host", "band", "lum", "child"}
    for name, sw in T.SWITCHES.items():
        assert sw["values"] and all(isinstance(v, str) for v in sw["values"]), name
        assert sw["forms"] and set(sw["forms"]) <= forms, name
        assert set(sw["shapes"]) <= set(T.SHAPES), name
        if set(sw["forms"]) & (set(T.PAIR_FORMS) | {"host"}):
            assert sw["shapes"], name
        assert sw["probe"] is None or isinstance(sw["probe"], str), name
    ids = [T.case_id(*c) for c in T.cases()]
    assert len(ids) == len(set(ids))


def test_fuzz_switches_are_runtime_switches_of_the_table():
    spec = importlib.util.spec_from_file_location("fuzz_pairs", os.path.join(ROOT, "scripts", "fuzz_pairs.py"))
    fz = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(fz)
    stray = sorted(k for k in fz.SWITCHES if k not in T.SWITCHES)
    assert not stray, f"fuzz_pairs.SWITCHES draws switches that are not in tests/switch_table.py: {stray}"
    for k in ("STITCH_C4_LOCKSTEP", "STITCH_NO_FUSE", "STITCH_XBYF_EARLY", "STITCH_CROWS_L0", "STITCH_CROWS_LN", "STITCH_CROWS_WGS",
              "STITCH_XBYM_MPIX"):
        assert k in fz.SWITCHES, k
    assert {"1", "2"} <= set(fz.SWITCHES["STITCH_C4_LOCKSTEP"])
    draws = fz.SWITCHES["STITCH_NO_FUSE"]
    assert draws.count("1") / len(draws) <= 0.25  # the fused sweep stays in most of the fuzz cases


def test_inventory_catches_an_unlisted_switch(tmp_path):
    """The parser finds a switch in a source it has not seen: a new getenv without a table entry would fail the test above."""
    src = tmp_path / "k_new.inc"
    src.write_text('const char* e = std::getenv("STITCH_SOMETHING_NEW");\nint v = Tuning::env_int( "STITCH_OTHER_NEW" );\n')
    assert switches_read(str(tmp_path)) == {"STITCH_SOMETHING_NEW", "STITCH_OTHER_NEW"}
