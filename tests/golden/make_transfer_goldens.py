"""Records the REFERENCE's colour transfer (transfer.cpp, compiled in place by oracle/Makefile into
oracle/_ref/libref_transfer.so) for the cases of tests/transfer_cases.py -> tests/golden/transfer.npz.

Run where the reference is built (make -C oracle ref):  python tests/golden/make_transfer_goldens.py

Per case: the two recipes (random images in full), the reference's output as SHA-256 (in full up to 64 KiB) and its twelve
statistics as bit patterns; the same of oracle.transfer in specified-function mode (include/stitch_elem.h, what the HIP
kernels evaluate); and position and both values of every byte in which the two differ.  The reference built here calls
this platform's libm, whose logf is not correctly rounded everywhere, hence the handful of differing bytes.

Conditions on the fixture set, fulfilled by the reference on its own and asserted here:
  * oracle.transfer(use_libm=True) equals the reference in every byte and statistic bit (same libm on both sides);
  * every recorded difference is exactly one grey level;
  * the differing bytes over all cases number at most 1e-5 of all bytes."""
import hashlib
import json
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from oracle_lib import Oracle, Reference, have_reference_transfer  # noqa: E402
import transfer_cases as T  # noqa: E402


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def bits(a):
    return [int(v) for v in np.ascontiguousarray(a, np.float32).view(np.uint32)]


def main():
    assert have_reference_transfer(), "oracle/_ref/libref_transfer.so is missing: make -C oracle ref"
    O, ref = Oracle(), Reference()
    arrays, cases = {}, {}
    total_bytes = total_diff = 0
    for name, rs, rt in T.CASES:
        src, tem = T.build_image(rs, O), T.build_image(rt, O)
        for k, r, img in (("src", rs, src), ("tem", rt, tem)):
            if "random" in r:
                arrays[f"{name}.{k}"] = img
        want, wst = ref.transfer(src, tem)
        libm, lst = O.transfer(src, tem, use_libm=True)
        assert np.array_equal(libm, want) and bits(lst) == bits(wst), (name, "the restatement with this libm is not the reference")
        spec, sst = O.transfer(src, tem)
        pos = np.flatnonzero(spec.reshape(-1) != want.reshape(-1)).astype(np.int64)
        d_ref, d_spec = want.reshape(-1)[pos], spec.reshape(-1)[pos]
        assert np.all(np.abs(d_ref.astype(int) - d_spec.astype(int)) == 1), (name, "a difference of more than one grey level")
        arrays[f"{name}.diff_pos"], arrays[f"{name}.diff_ref"], arrays[f"{name}.diff_spec"] = pos, d_ref, d_spec
        if want.nbytes <= T.FULL_OUTPUT_LIMIT:
            arrays[f"{name}.ref_out"] = want
        total_bytes += want.size
        total_diff += pos.size
        cases[name] = dict(src=rs, tem=rt, shape=list(want.shape), src_sha256=sha(src), tem_sha256=sha(tem),
                           ref_sha256=sha(want), ref_stats_bits=bits(wst), spec_sha256=sha(spec), spec_stats_bits=bits(sst),
                           differing_bytes=int(pos.size), differing_stats=int(sum(a != b for a, b in zip(bits(wst), bits(sst)))))
        print(f"{name:30s} {want.shape}  differing bytes {pos.size}  differing statistics {cases[name]['differing_stats']}")
    assert total_diff <= 1e-5 * total_bytes, (total_diff, total_bytes)

    # information about this platform's libm, not an assertion: how many of the log() inputs of all 2^24 colours its logf
    # rounds otherwise than the correctly rounded value, which stitch_elem_logf returns everywhere (tests/test_oracle_golden.py)
    with tempfile.TemporaryDirectory() as d:
        logf, pow10 = T.elem_check(d)
        lg = logf()
        ec = T.every_colour(1)
        pw = pow10(O.transfer_exponents(ec, ec))
    print("logf over the domain:", lg)
    print("pow10 over the every-colour exponents:", pw)
    meta = dict(cases=cases, total_bytes=int(total_bytes), total_differing_bytes=int(total_diff), logf_domain=lg, pow10_every_colour=pw)
    out = os.path.join(HERE, "transfer.npz")
    np.savez_compressed(out, meta=np.array(json.dumps(meta)), **arrays)
    size = os.path.getsize(out)
    assert size < 1 << 20, size
    print(f"{out}: {size} bytes, {len(cases)} cases, {total_diff} differing bytes of {total_bytes}")


if __name__ == "__main__":
    main()
