"""The recorded whole-panorama runs beyond four frames (tests/golden/chains.json): frame recipes -> frames, and the reference's
whole program under the argument recorder in a child process.  TEST INFRASTRUCTURE ONLY, shared by
tests/golden/make_chain_goldens.py, tests/test_chain_host.py and tests/test_gpu_chains.py.

A frame recipe is {"file": path under tests/golden} or {"synth": [w, h, frame_id]} (oracle_lib.Oracle.synth, an INPUT recipe);
chains.json adds the frame's shape and the sha256 of its planar bytes.
"""
import hashlib
import json
import os
import re
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
GOLD = os.path.join(HERE, "golden")
CHAINS = os.path.join(GOLD, "chains.json")
RECORDER_SO = os.path.join(ROOT, "oracle", "_ref", "libref_record.so")
MATCH_THRESHOLD = 20  # THRESHOLD, ImageProcess.h:18

RECORDER_VERSION = 2  # rec_version() of oracle/ref_record.cpp: the hooks parse_run needs

_cache = {}


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def chains():
    if "chains" not in _cache:
        with open(CHAINS) as f:
            _cache["chains"] = json.load(f)
    return _cache["chains"]


def frame_of(recipe):
    """One recipe -> the (3, H, W) uint8 frame (cached by recipe, never modified by callers)."""
    key = json.dumps({k: recipe[k] for k in ("file", "synth") if k in recipe}, sort_keys=True)
    if key not in _cache:
        if "file" in recipe:
            from computervisionimagestich2_amd import bmp
            img = bmp.load_bmp(os.path.join(GOLD, recipe["file"]))
        else:
            from oracle_lib import Oracle
            if "oracle" not in _cache:
                _cache["oracle"] = Oracle()
            w, h, frame_id = recipe["synth"]
            img = _cache["oracle"].synth(w, h, frame_id)
        img = np.ascontiguousarray(img, np.uint8)
        img.setflags(write=False)
        _cache[key] = img
    return _cache[key]


def frames_of(recipes):
    return [frame_of(r) for r in recipes]


def evaluated_pairs(lengths_in_call_order, n, threshold=MATCH_THRESHOLD):
    """matching()'s first loop (ImageProcess.cpp:117-137) replayed over the lengths getImgPair returned, in call order: the
    n x n count matrix with -1 where the reference made no call ((i, j) once (j, i) was a neighbour), and how many calls the
    loop made.  Only the loop's own skip rule is restated here; the lengths are the reference's."""
    counts = [[-1 if i != j else 0 for j in range(n)] for i in range(n)]
    mat = [[False] * n for _ in range(n)]
    used = 0
    for i in range(n):
        for j in range(n):
            if i == j:
                continue
            if mat[j][i]:
                mat[i][j] = True
                continue
            counts[i][j] = lengths_in_call_order[used]
            used += 1
            if counts[i][j] >= threshold:
                mat[i][j] = True
    return counts, used


def parse_run(stdout, log_text, dump_dir, n):
    """What one run of the reference's whole program left behind -> the record chains.json keeps (without the frame recipe)."""
    # stdout: getMiddleIndex prints the start frame (:391), every step prints "srcIndex dstIndex" (:183)
    lines = [ln.split() for ln in stdout.strip().split("\n") if ln.strip()]
    assert len(lines[0]) == 1, f"expected the start frame first, got {lines[0]}"
    start = int(lines[0][0])
    printed = [(int(a), int(b)) for a, b in lines[1:]]
    calls, steps, cur = [], [], {}
    for ln in log_text.strip().split("\n"):
        kv = dict(re.findall(r"(\w+)=([^ ]+)", ln))
        if ln.startswith("pairs"):
            assert int(kv["call"]) == len(calls)
            calls.append((int(kv["na"]), int(kv["nb"]), int(kv["len"])))
        elif ln.startswith("warp"):
            cur = {"p": [float(v) for v in kv["p"].split(",")], "offx": float(kv["offx"]), "offy": float(kv["offy"]), "cw": int(kv["cw"]),
                   "ch": int(kv["ch"]), "fw": int(kv["sw"]), "fh": int(kv["sh"])}
        elif ln.startswith("move"):
            cur.update({"ox": int(kv["ox"]), "oy": int(kv["oy"]), "mw": int(kv["sw"]), "mh": int(kv["sh"])})
        elif ln.startswith("fwd"):
            cur.update({"p_fwd": [float(v) for v in kv["p"].split(",")], "mapped_n": int(kv["n"])})
            assert float(kv["offx"]) == cur["offx"] and float(kv["offy"]) == cur["offy"]
        elif ln.startswith("shift"):
            cur["shift"] = {"n": int(kv["n"]), "ox": int(kv["ox"]), "oy": int(kv["oy"])}
        elif ln.startswith("blend"):
            k = len(steps)
            assert int(kv["step"]) == k and (int(kv["w"]), int(kv["h"])) == (cur["cw"], cur["ch"])
            out = np.fromfile(os.path.join(dump_dir, f"step{k}_out_{cur['cw']}x{cur['ch']}.raw"), np.uint8)
            assert out.size == 3 * cur["cw"] * cur["ch"]
            cur["out_sha256"] = sha(out)
            steps.append(cur)
            cur = {}
    assert len(steps) == len(printed), f"{len(printed)} steps printed, {len(steps)} recorded"
    assert calls, "the recorder logged no getImgPair call: oracle/_ref/libref_record.so lacks the hook (rec_version() < 2)"
    counts, used = evaluated_pairs([c[2] for c in calls], n)
    assert len(calls) == used + 2 * len(steps), f"{len(calls)} getImgPair calls, {used} + 2 * {len(steps)} expected"
    # every frame's feature count, from the arguments of the first loop's calls
    features = [None] * n
    k = 0
    for i in range(n):
        for j in range(n):
            if i != j and counts[i][j] >= 0:
                for f, v in ((i, calls[k][0]), (j, calls[k][1])):
                    assert features[f] in (None, v)
                    features[f] = v
                k += 1
    for k, (s, (src, dst)) in enumerate(zip(steps, printed)):
        a, b = calls[used + 2 * k], calls[used + 2 * k + 1]
        assert (a[0], a[1]) == (features[src], features[dst]) and (b[0], b[1]) == (features[dst], features[src])
        assert s["mapped_n"] == features[dst]
        s.update({"srcIndex": src, "dstIndex": dst, "len_src_dst": a[2], "len_dst_src": b[2]})
        who = [f for f in range(n) if features[f] == s["shift"]["n"]]
        assert len(who) == 1, f"step {k}: frames {who} have the shifted map's {s['shift']['n']} features: change the set"
        s["shift"]["frame"] = who[0]
        del s["mapped_n"]
    return {"start": start, "features": features, "counts": counts, "steps": steps}


def _recorder_version():
    """rec_version() of the built recorder, asked in a child process (0: built from a source without it; None: not loadable)."""
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--recorder-version"], stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                       timeout=60, text=True)
    return int(r.stdout.strip()) if r.returncode == 0 and r.stdout.strip().isdigit() else None


def recorder_ready():
    """True where the reference is built (oracle/_ref) together with a recorder that has this tree's hooks.  A recorder that is
    older than its source, or that was built from an earlier state of it, is rebuilt first -- as oracle_lib.build_oracle does for
    the oracle -- which needs the reference's headers; where that cannot be done the answer is False."""
    from oracle_lib import REF_SO
    if "recorder_ready" not in _cache:
        src = os.path.join(ROOT, "oracle", "ref_record.cpp")
        ok = os.path.exists(REF_SO) and os.path.exists(RECORDER_SO)
        if ok:
            stale = os.path.getmtime(RECORDER_SO) < os.path.getmtime(src)
            if stale or _recorder_version() != RECORDER_VERSION:
                made = subprocess.run(["make", "-s", "-B", "-C", os.path.join(ROOT, "oracle"), RECORDER_SO], stdout=subprocess.PIPE,
                                      stderr=subprocess.PIPE)
                ok = made.returncode == 0 and _recorder_version() == RECORDER_VERSION
        _cache["recorder_ready"] = ok
    return _cache["recorder_ready"]


def run_reference(frames, timeout=120):
    """The reference's whole program (ImageProcess(dir, n), oracle/ref_harness.cpp ref_pipeline) on `frames` under the recorder, in
    a child process with a time limit.  Returns the record of parse_run plus final_shape / final_sha256, or None when the child
    did not exit 0 (the reference crashes on some sets: such a set cannot be a fixture)."""
    from computervisionimagestich2_amd import bmp
    with tempfile.TemporaryDirectory() as tmp:
        d = os.path.join(tmp, "in")
        dump = os.path.join(tmp, "dump")
        os.makedirs(d)
        os.makedirs(dump)
        for i, f in enumerate(frames):
            bmp.save_bmp(os.path.join(d, f"{i + 1}.bmp"), f)
        logp, finalp = os.path.join(tmp, "log.txt"), os.path.join(tmp, "final.npy")
        try:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", d + "/", str(len(frames)), logp, dump, finalp],
                               stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=timeout, text=True)
        except subprocess.TimeoutExpired:
            return None
        if r.returncode != 0:
            assert "AssertionError" not in r.stderr, r.stderr[-2000:]  # the harness's own check, not the reference's exit
            return None
        with open(logp) as f:
            rec = parse_run(r.stdout, f.read(), dump, len(frames))
        final = np.load(finalp)
        rec.update({"final_shape": list(final.shape), "final_sha256": sha(final)})
        return rec


def _child(directory, n, logp, dump, finalp):
    import ctypes as C
    # the recorder must be in the global namespace BEFORE the reference library is loaded (symbol interposition)
    rec = C.CDLL(RECORDER_SO, mode=C.RTLD_GLOBAL)
    assert hasattr(rec, "rec_version") and rec.rec_version() == RECORDER_VERSION, "oracle/_ref/libref_record.so was built from another ref_record.cpp"
    from oracle_lib import REF_SO, Reference
    R = Reference()
    assert rec.rec_init(REF_SO.encode(), logp.encode(), dump.encode()) == 0
    final = R.pipeline(directory, n)
    rec.rec_close()
    np.save(finalp, final)
    sys.stdout.flush()


if __name__ == "__main__":
    if sys.argv[1] == "--recorder-version":
        import ctypes
        lib = ctypes.CDLL(RECORDER_SO)
        print(lib.rec_version() if hasattr(lib, "rec_version") else 0)
        sys.exit(0)
    assert sys.argv[1] == "--child"
    sys.path.insert(0, ROOT)
    _child(sys.argv[2], int(sys.argv[3]), sys.argv[4], sys.argv[5], sys.argv[6])
