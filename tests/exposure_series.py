"""The float series at which the exact running sums of csrc/k_exposure.inc are held against a plain float loop: shared by
tests/test_exposure_host.py (the device functions compiled for the CPU) and tests/test_gpu_exposure.py (the kernels; the same
arrays are uploaded, not regenerated).  TILE and SPAN are k_exposure.inc's EX_TILE and EX_SPAN; the host test holds them to the
source."""
import numpy as np

TILE, SPAN = 2048, 8192
F = np.float32


def lengths():
    return [1, 255, 256, 257, TILE - 1, TILE, TILE + 1, SPAN - 1, SPAN, SPAN + 1, 2 * SPAN + 1]


def crafted():
    """name -> float32 array.  What each one is there for is said next to it."""
    rng = np.random.default_rng(20261018)
    out = {}
    for n in lengths():  # lengths around the tile and the span
        out[f"uniform_{n}"] = (rng.random(n) * 3).astype(F)
    # multiples of u/2 for the binade the sum reaches: with ones added first the state is in [2^12, 2^13), u = 2^-11, and
    # every later addend is an odd multiple of 2^-12 -- a tie at every step, unsigned and signed
    head = np.ones(4096, F)
    ties = ((2 * rng.integers(0, 64, 6000) + 1) * 2.0 ** -12).astype(F)
    out["ties_unsigned"] = np.concatenate([head, ties])
    out["ties_signed"] = np.concatenate([head, ties * np.where(rng.random(6000) < 0.5, -1, 1).astype(F)])
    out["zero_mean_normal"] = rng.standard_normal(200000).astype(F)
    out["alternating_sign"] = ((rng.random(200000) + 0.5) * np.where(np.arange(200000) % 2, 1, -1)).astype(F)
    b = rng.integers(1, 100, 3000).astype(F)  # integers: the partial sums are exact, so the sum is exactly 0 mid-way
    out["returns_to_zero"] = np.concatenate([b, -b[::-1], b])
    out["negative_sum"] = (-rng.random(50000) * 2).astype(F)
    out["falls_out_downwards"] = np.concatenate([np.full(5000, 1.0, F), np.full(4990, -1.0, F), (rng.random(3000) * 0.01).astype(F)])
    # the 2^23 - 0.3 trap: a state at the bottom of its binade and an addend that takes the exact sum just below it.  State
    # 1.0 is S = 2^23 (u = 2^-23); state 1 + 2^-23 is S = 2^23 + 1.  The addends are -(0.3 u) and -(1.3 u).
    u = 2.0 ** -23
    out["trap_entry_S_2p23"] = np.array([1.0, -0.3 * u, 0.25, 0.5 * u], F)
    out["trap_entry_S_2p23_plus_1"] = np.array([1.0, u, -1.3 * u, 0.25, 0.5 * u], F)
    # a binade crossing exactly on a span boundary: SPAN ones minus one give 2^13 - 1, the sample that opens the next span
    # takes the sum to 2^13
    out["crossing_on_span_boundary"] = np.concatenate([np.ones(SPAN - 1, F), np.array([0.0], F), np.ones(SPAN, F), (rng.random(100)).astype(F)])
    c = np.ones(20000, F)
    c[5000] = 2.0 ** 30
    out["one_2p30_among_ones"] = c
    c = np.ones(20000, F)
    c[7000] = np.inf
    out["one_inf"] = c
    c = np.ones(20000, F)
    c[7000] = np.nan
    out["one_nan"] = c
    out["all_zero"] = np.zeros(3 * TILE + 5, F)
    z = (rng.random(30000)).astype(F)
    z[:9000] = 0
    out["zeros_then_values"] = z
    out["subnormal_sum"] = np.concatenate([np.full(3000, 1e-42, F), (rng.random(3000) * 1e-37).astype(F)])
    # the sum overflows.  A multiple of 256 samples: k_tr_stats pads its last block of 256 with (mean - mean)^2, which is NaN for
    # a mean that is not finite, so only there is the serial form the plain loop on such a plane
    out["huge_values"] = (rng.random(5120) * 1e37).astype(F)
    for k in out:
        out[k] = np.ascontiguousarray(out[k], F)
        out[k].setflags(write=False)
    return out
