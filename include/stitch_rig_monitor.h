/* stitch_rig_monitor.h -- a rig's alignment monitor: overlap residuals over integer shifts (libstitch_hip.so, same ABI version).
 *
 * An addition to include/stitch_rig.h and include/stitch_rig_seams.h, kept in a header of its own so that their tables of entry
 * points stay as they are.  A rig replays one panorama's maps for as long as it lives; nothing else tells the caller when a
 * camera has moved and those maps have stopped fitting.  The monitor measures, per step and per set, how much the two inputs of
 * the blend disagree where both cameras see the scene -- as they are, and under every integer shift of the warped frame within a
 * radius.  All of it is exact integer arithmetic, so a record is the same bits on every run.  A rig that never sets a monitor
 * allocates nothing, launches nothing more and writes every byte it wrote before; no call of the other headers changes.
 *
 * THE DEFINITION.  For one pair on a cw x ch canvas:
 *   a = the zero-initialised canvas after stitch_warp_u8(frame, p, offx, offy),
 *   b = the zero-initialised canvas after stitch_move_u8(mosaic, ox, oy),
 * both exactly as the stitch step builds them (ImageProcess.cpp:218-230): unsigned char, three planes.
 * The gray value of a pixel is g = R + 2 * G + B (0 .. 1020).
 * For a radius r (0 .. STITCH_RESIDUAL_MAX_RADIUS) and a domain D (a set of canvas pixels) the effective domain is
 *   D' = { (x, y) in D : r <= x < cw - r, r <= y < ch - r },
 * so that every shifted read stays inside the canvas.  For each shift (dx, dy), |dx|, |dy| <= r, with the index
 * j = (dy + r) * (2r + 1) + (dx + r):
 *   n        = |D'|
 *   sum_b    = sum over D' of g_b[y][x]
 *   sum_a[j] = sum over D' of g_a[y + dy][x + dx]
 *   sad[j]   = sum over D' of | g_a[y + dy][x + dx] - g_b[y][x] |
 *   ssd[j]   = sum over D' of ( g_a[y + dy][x + dx] - g_b[y][x] )^2
 * One RECORD is 2 + 3 * (2r + 1)^2 uint64_t words: n, sum_b, then sum_a[j], sad[j], ssd[j] for j ascending.
 * The bound: a canvas has cw * ch <= 2^31 - 1 pixels and a squared difference is at most 1020^2 = 1 040 400 < 2^20, so every
 * sum is below 2^51 and fits 64 bits.  An empty D' gives an all-zero record and is not an error.
 * sum_a and sum_b let a caller remove an exposure difference exactly: the zero-mean score of shift j is the integer
 *   n * ssd[j] - (sum_a[j] - sum_b)^2        (below 2^102: compare it in 128 bits, as stitch_residual_best_shift does).
 *
 * THE RIG'S DOMAIN of step k at radius r, with A_k and B_k the coverage planes of stitch_rig_seams.h:
 *   D_k = { (x, y) : B_k[y][x], and A_k[y + dy][x + dx] for all |dx|, |dy| <= r with (x + dx, y + dy) inside the canvas }
 * -- the moved mosaic's footprint, and the warped frame's footprint eroded by the shift box.  No zero that only means "no camera
 * sees this" enters a sum, and n is the same for every shift.
 */
#ifndef STITCH_RIG_MONITOR_H
#define STITCH_RIG_MONITOR_H
#include <stddef.h>
#include <stdint.h>

#include "stitch.h"
#include "stitch_rig.h"
#include "stitch_rig_seams.h"

#ifdef __cplusplus
extern "C" {
#endif

#define STITCH_RESIDUAL_MAX_RADIUS 8

/* HOST ONLY: the words of a record, 2 + 3 * (2 * radius + 1)^2, or 0 for a radius outside 0 .. 8. */
int stitch_residual_words(int radius);

/* ---- the stand-alone call: enqueued on `stream` ----------------------------------------------------------------------------
 * pairs: a HOST array of n descriptors, 1 <= n <= 65535; frame, fw, fh, p, offx, offy, mosaic, mw, mh, ox, oy are read, out and
 * out_u8 are ignored.  d_domain: a HOST array of n device pointers to dense cw * ch byte masks (non-zero = in the domain; entries
 * may alias).  d_records: device memory of n records of stitch_residual_words(radius) words, which the call itself zeroes.
 * The descriptors go up to the device from a host copy, so the call WAITS for `stream`, as the _many calls of stitch_rig.h do.
 * A canvas with cw <= 2 * radius or ch <= 2 * radius is valid and gives empty records.  Argument errors (a null pointer, a pair
 * without a frame, a mosaic or a mask, a radius outside 0 .. 8, a size < 1, cw * ch > 2^31 - 1, ch > 65535 * 32, n out of range)
 * are reported before a device is needed. */
int stitch_dev_pairs_residual_u8(const stitch_pair_desc *pairs, int n, int cw, int ch, const uint8_t *const *d_domain, int radius,
                                 uint64_t *d_records, void *stream);

/* ---- a rig with a monitor: HOST ONLY ---------------------------------------------------------------------------------------
 * stitch_rig_set_monitor: a radius outside 0 .. 8 or a null rig is STITCH_ERR_ARG and leaves the rig as it was.  While a
 * monitor is set every replay -- stitch_dev_rig_stitch_u8, stitch_dev_rig_stitch_exposure_u8, stitch_dev_rig_stitch_fmt_u8 --
 * computes, per set and step, the record of that step over D_k from exactly the inputs that step's blend receives: the projected
 * frame after the exposure transfer where the rig has a mode, and the running mosaic.  That is one more launch per step and launch
 * sequence; the records of a sequence leave the device in one stream-ordered copy.  Outputs, statuses, seams and statistics are
 * what they are without the monitor.  The first monitored replay computes the coverage planes if the rig has none yet (as
 * stitch_dev_rig_coverage_u8 does), then D_k and its bounding box for every step, once: bit planes the rig owns, freed by
 * stitch_rig_destroy.  Changing the radius recomputes them on the next replay.  A rig with zero steps has nothing to monitor,
 * and the calls succeed.
 * stitch_rig_clear_monitor: no monitor (also forgets the last records).  stitch_rig_monitor: *radius = the radius, or -1 when
 * none is set (`radius` may be null). */
int stitch_rig_set_monitor(stitch_rig *rig, int radius);
int stitch_rig_clear_monitor(stitch_rig *rig);
int stitch_rig_monitor(const stitch_rig *rig, int *radius);

/* HOST ONLY: the records of the last monitored replay, set-major then step: n_sets * n_steps * stitch_residual_words(radius)
 * words to `out` (optional; cap_words is its capacity, and STITCH_ERR_ARG if it is too small).  n_sets, n_steps and radius are
 * optional outputs; n_sets = 0 if no monitored replay has completed.  A set whose seam scan failed at step k has defined records
 * up to and including step k and unspecified ones after it.  A replay that failed with STITCH_ERR_HIP leaves no records. */
int stitch_rig_residuals(const stitch_rig *rig, uint64_t *out, size_t cap_words, int *n_sets, int *n_steps, int *radius);

/* D_step at `radius` as cw * ch bytes, 0 or 255, to d_mask (device), under the conventions of stitch_dev_rig_coverage_u8:
 * step == -1 is the last step; the first coverage call on a rig computes the planes and waits for `stream`, after that the call is
 * enqueued and returns.  Works whether or not a monitor is set and does not change the rig's monitor.  A rig with zero steps, a
 * null argument, a step outside -1 .. n_steps-1 and a radius outside 0 .. 8 are STITCH_ERR_ARG, reported before a device is
 * needed. */
int stitch_dev_rig_residual_domain_u8(stitch_rig *rig, int step, int radius, uint8_t *d_mask, void *stream);

/* HOST ONLY: the shift a record favours: the argmin over j of ssd[j] (zero_mean = 0) or of n * ssd[j] - (sum_a[j] - sum_b)^2
 * (zero_mean = 1), compared as exact integers in 128 bits.  Ties go to the smallest dx^2 + dy^2, then the smallest dy, then the
 * smallest dx.  dx and dy are optional.  n == 0 is STITCH_ERR_ZERO_OVERLAP; a null record or a radius outside 0 .. 8 is
 * STITCH_ERR_ARG. */
int stitch_residual_best_shift(const uint64_t *record, int radius, int zero_mean, int *dx, int *dy);

#ifdef __cplusplus
}
#endif
#endif /* STITCH_RIG_MONITOR_H */
