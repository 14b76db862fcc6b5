"""The inputs and expected results of tests/form_cover.py's cases: what tests/test_gpu_form_cover.py compares the library with, and
what tests/test_form_cover_host.py checks on the CPU before any GPU run (every flagged case has something flagged).  The oracle and
numpy alone: no torch, no GPU.

Pairs: the four placements of form_cover.inputs(cw); call 1 cycles g_flags_ref.BATCHES[0] over the call's slots, call 2 BATCHES[1], a
seed per (call, slot): the zero regions and the seam's side and branch move between the calls.  Dense blends: two canvases a third
black on opposite sides, the sides swapped in call 2."""
import numpy as np

import form_cover as FC
import g_flags_ref
import mask_rows_ref

ALL_CASES = FC.CASES + FC.WIDE_CASES


def case_id(case):
    cw, ch, cap, n, dense, opts = case[:6]
    return f"{opts}-{cw}x{ch}-cap{cap}-n{n}-{'dense' if dense else 'pairs'}"


def two_canvases(oracle, w, h, fa, fb, dtype, a_left):
    """Two dense canvases as tests/test_gpu_parity.py::test_blend_u8 builds them: a third of each is black, on opposite sides."""
    A, B = oracle.synth(w, h, fa, dtype), oracle.synth(w, h, fb, dtype)
    if a_left:
        A[:, :, (2 * w) // 3:] = 0
        B[:, :, : w // 3] = 0
    else:
        A[:, :, : w // 3] = 0
        B[:, :, (2 * w) // 3:] = 0
    return A, B


class References:
    """Inputs and oracle results of (canvas, options, pixel type, call, slot), computed once and shared by the cases of one canvas:
    slot s of call c is the same pair whatever the call's size.  Only the last canvas is kept."""

    def __init__(self, oracle):
        self.oracle, self.key, self.cache = oracle, None, {}

    def _slot(self, cw, ch, opts, dtype, what):
        key = (cw, ch, opts, np.dtype(dtype).name)
        if key != self.key:
            self.key, self.cache = key, {}
        return self.cache.setdefault(what, {})

    def pair(self, cw, ch, opts, dtype, call, slot):
        r = self._slot(cw, ch, opts, dtype, ("pair", call, slot))
        if not r:
            o, oo = self.oracle, FC.OPTION_SETS[opts]
            which = g_flags_ref.BATCHES[call][slot % 2]
            fw, P, mw, ox, branch = FC.inputs(cw)[which]
            seed = 16 * call + slot
            F, M = o.synth(fw, ch, 2 * seed + 1, dtype), o.synth(mw, ch, 2 * seed, dtype)
            rc, ref = o.pair(F, P, 0.0, 0.0, M, ox, 0, cw, ch, oo)
            assert rc == 0, (which, rc)
            rcs, seam = o.seam(o.warp(F, P, 0.0, 0.0, cw, ch), o.move(M, ox, 0, cw, ch))
            assert rcs == 0 and branch in (None, seam.branch), (which, rcs, seam.as_tuple())
            ref.setflags(write=False)
            r.update(name=which, F=F, P=P, M=M, ox=ox, ref=ref, seam=seam, level_rule=oo["level_rule"])
        return r

    def flag_counts(self, r, cw, ch):
        """(G column counts, mask-row counts) of levels 1 and 2 by the rules, on the oracle's planes of the pair r."""
        if "counts" not in r:  # (the two canvases are made again: 16 pairs of 2052 x 2052 would keep 3 GB of them)
            a, b = self.oracle.warp(r["F"], r["P"], 0.0, 0.0, cw, ch), self.oracle.move(r["M"], r["ox"], 0, cw, ch)
            r["counts"] = (g_flags_ref.flagged_columns(self.oracle, a, b),
                           mask_rows_ref.flagged_entries(self.oracle, r["seam"], cw, ch, r["level_rule"]))
        return r["counts"]

    def dense(self, cw, ch, opts, dtype, call):
        r = self._slot(cw, ch, opts, dtype, ("dense", call))
        if not r:
            A, B = two_canvases(self.oracle, cw, ch, 5 + 2 * call, 6 + 2 * call, dtype, a_left=call == 0)  # the black regions move
            rc, ref, seam = self.oracle.blend(A, B, FC.OPTION_SETS[opts])
            assert rc == 0, rc
            ref.setflags(write=False)
            r.update(A=A, B=B, ref=ref, seam=seam)
        return r


def expected_counts(refs, rec, recs, cw, ch):
    """What Plan.g_flag_counts() and Plan.mask_row_counts() must return after a call of the pairs recs, by the record's flags."""
    g_on, mr_on = flags_on(rec)
    g, mr = [0, 0], [0, 0]
    if any(g_on):
        for r in recs:
            cg, cm = refs.flag_counts(r, cw, ch)
            for i in range(2):
                g[i] += cg[i] if g_on[i] else 0
                mr[i] += cm[i] if mr_on[i] else 0
    return g_on, mr_on, tuple(g), tuple(mr)


def pixel_types(rec):
    """float always; unsigned char as well where level 0 is evaluated from the frames or carries the implicit mask (the gathers and
    the level-0 kernels differ by pixel type)."""
    l0 = rec["levels"][0] if rec["levels"] else {}
    return [np.float32, np.uint8] if l0.get("src0") or l0.get("mask_l0") else [np.float32]


def flags_on(rec):
    """([G column flags at level 1, 2], [mask-row flags at level 1, 2]) of a record."""
    lv = rec["levels"]
    return [len(lv) > l and bool(lv[l]["g_in"]) for l in (1, 2)], [len(lv) > l and bool(lv[l]["mr_in"]) for l in (1, 2)]


def build_records(directory):
    """The decision's record of every case of ALL_CASES."""
    from call_form_tool import build_dump, dump
    return dump(build_dump(directory), directory, [FC.dump_case(*c[:6]) for c in ALL_CASES])
