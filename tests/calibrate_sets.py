"""Captures for the calibration tests (tests/golden/calibrate.json): capture recipes -> frames, the CPU reference's match counts
of a capture, and the calibration chain composed from the stage calls of capi.  TEST INFRASTRUCTURE ONLY, shared by
tests/golden/make_calibrate_goldens.py and tests/test_gpu_calibrate.py.

A frame recipe is a recipe of tests/chain_sets.py ({"file": ...} or {"synth": ...}) with optional derivations, applied in this
order, so that the derived frame's features really differ from the committed frame's:
    "crop":  [x0, y0, w, h]   a window of the frame
    "table": "dark" | "light" a monotone byte table (integer arithmetic only)
    "shift": [dx, dy]         out[y][x] = in[y + dy][x + dx], the border repeated: a crop moved by a few pixels, padded back to size
    "const": v                every byte v (a frame without features)
    "dot":   [x, y, r, v]     a constant frame of value 128 with one disc of value v (a frame with very few features)
"""
import json
import os

import numpy as np

import chain_sets

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, "golden", "calibrate.json")

_V = np.arange(256, dtype=np.int64)
TABLES = {"dark": ((_V + _V * _V // 255 + 1) // 2).astype(np.uint8),
          "light": (255 - ((255 - _V) + (255 - _V) ** 2 // 255 + 1) // 2).astype(np.uint8)}

_cache = {}


def fixture():
    if "fixture" not in _cache:
        with open(FIXTURE) as f:
            _cache["fixture"] = json.load(f)
    return _cache["fixture"]


def frame_of(recipe):
    """One recipe -> the (3, H, W) uint8 frame (cached, read-only)."""
    key = json.dumps(recipe, sort_keys=True)
    if key not in _cache:
        img = np.array(chain_sets.frame_of(recipe))
        if "crop" in recipe:
            x0, y0, w, h = recipe["crop"]
            img = img[:, y0:y0 + h, x0:x0 + w]
            assert img.shape == (3, h, w)
        if "table" in recipe:
            img = TABLES[recipe["table"]][img]
        if "shift" in recipe:
            dx, dy = recipe["shift"]
            h, w = img.shape[1:]
            ys, xs = np.clip(np.arange(h) + dy, 0, h - 1), np.clip(np.arange(w) + dx, 0, w - 1)
            img = img[:, ys][:, :, xs]
        if "const" in recipe:
            img = np.full_like(img, recipe["const"])
        if "dot" in recipe:
            x, y, r, v = recipe["dot"]
            h, w = img.shape[1:]
            yy, xx = np.mgrid[:h, :w]
            img = np.full_like(img, 128)
            img[:, (yy - y) ** 2 + (xx - x) ** 2 <= r * r] = v
        img = np.ascontiguousarray(img, np.uint8)
        img.setflags(write=False)
        _cache[key] = img
    return _cache[key]


def captures_of(case):
    """A fixture case -> [[frame per camera] per capture]."""
    return [[frame_of(r) for r in cap] for cap in case["captures"]]


# ---- the CPU reference: the reference's projection, gray and VLFeat, the std::map order, the exact L1 ratio test -----------------
def reference_features(frame):
    """(descriptors in map order, rows) of one decoded frame by the reference's own code (tests/sift_ref.py)."""
    import sift_ref
    from computervisionimagestich2_amd import pipeline
    from oracle_lib import Reference
    if "ref" not in _cache:
        _cache["ref"] = (Reference(), sift_ref.load_reference())
    R, L = _cache["ref"]
    r = sift_ref.reference_sift(L, R.gray(R.project(np.ascontiguousarray(frame))))
    d, _, _ = pipeline.feature_order(r["desc"])
    return d


def reference_counts(frames):
    """(rows per frame, n x n counts of getImgPair(frame i, frame j)) of one capture."""
    import match_ref
    desc = [reference_features(f) for f in frames]
    n = len(frames)
    counts = [[0 if i == j else int(len(match_ref.match(desc[i], desc[j])[0])) for j in range(n)] for i in range(n)]
    return [int(len(d)) for d in desc], counts


# ---- the chain composed from the EXISTING stage calls of capi -----------------------------------------------------------------
def ordered_features(capi, frames, kp_cap=4096):
    """Per frame (descriptors (n, 128), x, y) float32 device tensors in map order, from dev_project_gray, dev_sift_many and
    feature_order_c.  Also the SIFT heads' key-point counts."""
    import torch
    grays = [capi.dev_project_gray(f)[1] for f in frames]
    outs = capi.dev_sift_many(grays, None, kp_cap)
    feats, found = [], []
    for o in outs:
        u = capi.sift_unpack(o)
        assert u["status"][0] == capi.SIFT_OK
        found.append(int(u["status"][1]))
        idx = capi.feature_order_c(u["desc"])
        kp = u["kp"][u["fkp"][idx]] if len(idx) else u["kp"][:0]
        dev = frames[0].device
        feats.append((torch.from_numpy(np.ascontiguousarray(u["desc"][idx], np.float32).reshape(-1, 128)).to(dev),
                      torch.from_numpy(np.ascontiguousarray(kp["x"], np.float32)).to(dev), torch.from_numpy(np.ascontiguousarray(kp["y"], np.float32)).to(dev)))
    return feats, found


def compose(capi, frame_sizes, features, pooled_threshold=0, match_threshold=20):
    """The calibration of include/stitch_calibrate.h stated WITHOUT pooled arrays or bases: every capture keeps its own x / y per
    camera, and a step's pooled list is the concatenation of the matched COORDINATES (pair i = row i of four arrays).  features:
    per capture, per camera (desc, x, y) device tensors, which are left unchanged.  Returns a dict like
    pipeline.calibrate_from_features's; raises capi.StitchError(ERR_NO_MAP) for a step without two maps."""
    import torch
    n_sets, n = len(features), len(features[0])
    x = [[f[1].clone() for f in fs] for fs in features]
    y = [[f[2].clone() for f in fs] for fs in features]
    kij = [(k, i, j) for k in range(n_sets) for i in range(n) for j in range(n) if i != j]
    outs = capi.dev_match_many([(features[k][i][0], features[k][j][0]) for k, i, j in kij], want_dist=False)
    lists = {key: o["pairs"][:int(o["count"].item())].long() for key, o in zip(kij, outs)}
    counts = np.zeros((n_sets, n, n), np.int32)
    for (k, i, j), l in lists.items():
        counts[k, i, j] = l.shape[0]
    pooled = counts.sum(0, dtype=np.int32)
    start, order = capi.stitch_order_c(pooled, pooled_threshold or n_sets * match_threshold)
    rw, rh = frame_sizes[start]
    steps, support, pre = [], [], start
    for src, dst in order:
        use_sd = int(pooled[src, dst]) > int(pooled[dst, src])
        cols, seg = [[], [], [], []], []
        for k in range(n_sets):
            l = lists[k, src, dst] if use_sd else lists[k, dst, src]
            a, b = (l[:, 0], l[:, 1]) if use_sd else (l[:, 1], l[:, 0])  # rows of src, rows of dst
            for c, v in zip(cols, (x[k][src][a], y[k][src][a], x[k][dst][b], y[k][dst][b])):
                c.append(v)
            seg.append(int(l.shape[0]))
        sx, sy, dx, dy = (torch.cat(c).contiguous() for c in cols)
        lst = dict(src_x=sx, src_y=sy, dst_x=dx, dst_y=dy)
        p, info, inl = capi.dev_ransac_many([dict(lst, mirror=True), dict(lst, mirror=False)])
        p, info = p.cpu().numpy(), info.cpu().numpy().astype(np.int64)
        if info[0][0] != capi.RANSAC_OK or info[1][0] != capi.RANSAC_OK:
            raise capi.StitchError(capi.ERR_NO_MAP, f"cameras {src} -> {dst}: no map")
        win = inl[0][:int(info[0][3])].cpu().numpy()
        off = np.concatenate([[0], np.cumsum(seg)])
        support.append([[seg[k], int(((win >= off[k]) & (win < off[k + 1])).sum())] for k in range(n_sets)])
        g = capi.step_geometry(frame_sizes[dst][0], frame_sizes[dst][1], p[0], rw, rh)
        for k in range(n_sets):
            capi.dev_map_points(x[k][dst], y[k][dst], p[0], g.min_x, g.min_y, want_int=False)
        for k in range(n_sets):
            capi.dev_shift_points(x[k][pre], y[k][pre], g.ox, g.oy, want_int=False)
        pre, rw, rh = dst, g.cw, g.ch
        steps.append(dict(start=start, src=dst, mosaic_src=src, p=p[1].copy(), p_fwd=p[0].copy(), offx=g.min_x, offy=g.min_y, ox=g.ox, oy=g.oy, cw=g.cw,
                          ch=g.ch, info=info))
    return dict(start=start, steps=steps, counts=counts, pooled=pooled, support=np.array(support, np.int32).reshape(len(steps), n_sets, 2), width=rw, height=rh)


def same_calibration(got, want):
    """Every bit of two results: `got` a capi.Calibration or a dict, `want` a dict.  Returns the list of differences."""
    g = got if isinstance(got, dict) else dict(start=got.start, steps=got.steps, counts=got.counts, pooled=got.pooled, support=got.support, width=got.width,
                                               height=got.height)
    bad = []
    for key in ("start", "width", "height"):
        if int(g[key]) != int(want[key]):
            bad.append((key, g[key], want[key]))
    for key in ("counts", "pooled", "support"):
        if not np.array_equal(np.asarray(g[key]), np.asarray(want[key])):
            bad.append((key, np.asarray(g[key]).tolist(), np.asarray(want[key]).tolist()))
    if len(g["steps"]) != len(want["steps"]):
        return bad + [("n_steps", len(g["steps"]), len(want["steps"]))]
    for k, (a, b) in enumerate(zip(g["steps"], want["steps"])):
        for key in ("src", "mosaic_src", "ox", "oy", "cw", "ch"):
            if int(a[key]) != int(b[key]):
                bad.append((k, key, a[key], b[key]))
        for key in ("p", "p_fwd"):
            if np.asarray(a[key], np.float64).tobytes() != np.asarray(b[key], np.float64).tobytes():
                bad.append((k, key, list(a[key]), list(b[key])))
        for key in ("offx", "offy"):
            if np.float32(a[key]).tobytes() != np.float32(b[key]).tobytes():
                bad.append((k, key, a[key], b[key]))
        if not np.array_equal(np.asarray(a["info"]), np.asarray(b["info"])):
            bad.append((k, "info", np.asarray(a["info"]).tolist(), np.asarray(b["info"]).tolist()))
    return bad
