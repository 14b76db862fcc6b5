"""numpy statements of include/stitch_rig_exposure_temporal.h: the first-order filter of a stream of twelve-statistics records, in
float32 with every operation rounded, and the colour transfer's apply pass with GIVEN statistics, composed from the oracle's own
RGBtoLab and LabToRGB (tests/oracle_lib.py) -- no arithmetic of the transfer is restated here.  Helper module, not a test."""
import numpy as np

F = np.float32
SD = (3, 4, 5, 9, 10, 11)  # where the six standard deviations sit among the twelve


def valid(m):
    """A record the filter takes up: twelve finite values, the six sds above 0."""
    m = np.asarray(m, F)
    return bool(np.isfinite(m).all() and (m[list(SD)] > 0).all())


def filter_stream(measured, keep, state=None):
    """measured: (count, 12) float32; keep: 0 .. 255; state: None or 12 floats -> (used (count, 12), state or None).
    Not valid: u = m, copied, the state untouched.  Valid and no state: u = m, which becomes the state.  Valid and a state:
    u = fl(m + fl(kf * fl(p - m))), which becomes the state; kf = keep / 256."""
    assert 0 <= int(keep) <= 255
    kf = F(int(keep)) / F(256)
    m = np.ascontiguousarray(np.asarray(measured, F).reshape(-1, 12))
    used = m.copy()  # bits and all: a NaN record leaves as it came
    p = None if state is None else np.asarray(state, F).copy()
    with np.errstate(all="ignore"):
        for i in range(m.shape[0]):
            if not valid(m[i]):
                continue
            if p is not None:
                used[i] = (m[i] + (kf * (p - m[i]).astype(F)).astype(F)).astype(F)
            p = used[i].copy()
    return used, p


def apply_given(oracle, src, st, keep_black):
    """src: (3, H, W) uint8; st: 12 float32 -> (3, H, W) uint8: RGBtoLab, v_c = ((x_c - st[c]) * st[9 + c]) / st[3 + c] + st[6 + c] in
    float32, LabToRGB (clamped), the C-cast truncation; with keep_black a (0, 0, 0) source pixel stays (0, 0, 0)."""
    src = np.ascontiguousarray(src, np.uint8)
    st = np.asarray(st, F)
    px = src.reshape(3, -1).T.astype(F)
    x = oracle.rgb_to_lab(px)
    v = np.empty_like(x)
    with np.errstate(all="ignore"):
        for c in range(3):
            v[:, c] = (((x[:, c] - st[c]).astype(F) * st[9 + c]).astype(F) / st[3 + c]).astype(F) + st[6 + c]
        rgb = oracle.lab_to_rgb(v.astype(F))
        out = rgb.astype(np.int32).astype(np.uint8)  # values are in [0, 255]; a NaN's cast is whatever the platform gives
    if keep_black:
        out[(px == 0).all(axis=1)] = 0
    return np.ascontiguousarray(out.T.reshape(src.shape))
