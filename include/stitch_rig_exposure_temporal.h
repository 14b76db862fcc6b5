/* stitch_rig_exposure_temporal.h -- temporal exposure for rigs: smoothed or fixed transfer statistics (libstitch_hip.so, same ABI
 * version).
 *
 * An addition to include/stitch_rig_exposure.h, kept in a header of its own so that its table of entry points stays as it is.  A rig
 * made with a mode (stitch_rig_create_exposure) recolours frame `dst` of every set before every step, each set from the twelve
 * statistics of its own pixels (the layout of stitch_panorama_exposure_stats: mean[3] and sd[3] of the frame's l, alpha, beta, then of
 * the template's).  The calls below let the statistics the apply pass READS differ from the ones just MEASURED:
 *
 *   smoothing   a first-order filter per step, carried on the device from set to set across launch sequences and calls, so that a
 *               person walking through one camera's view does not make the mosaic pump;
 *   fixed       one 12-vector per step, given once and replayed for every set: no template is converted, nothing is measured, no
 *               lab plane is stored -- one pass of 3 bytes in and 3 bytes out per pixel.
 *
 * A rig that sets neither allocates nothing more, launches nothing more and writes every byte and statistic it wrote before.
 * Everything here is stated exactly enough that a numpy restatement gives the same bits (tests/exposure_temporal_ref.py).
 */
#ifndef STITCH_RIG_EXPOSURE_TEMPORAL_H
#define STITCH_RIG_EXPOSURE_TEMPORAL_H
#include <stddef.h>
#include <stdint.h>

#include "stitch_rig_exposure.h"

#ifdef __cplusplus
extern "C" {
#endif

#define STITCH_EXPOSURE_KEEP_MAX 255 /* keep = 0 .. 255; the filter's factor is keep / 256, exact in float */

/* ---- the apply with given statistics: enqueued on `stream` ---------------------------------------------------------------------
 * 1 <= count <= 1024 planar uint8 images of w x h; d_src / d_out are HOST arrays of count device pointers, d_out[i] may be d_src[i].
 * d_stats12: DEVICE memory of count * 12 floats, st = d_stats12 + 12 * i for image i.  Per pixel, in float, no contraction:
 *     (x0, x1, x2) = RGBtoLab(R, G, B)                                       the transfer's own conversion
 *     v_c = ((x_c - st[c]) * st[9 + c]) / st[3 + c] + st[6 + c]              every operation rounded to float
 *     (R', G', B') = LabToRGB(v0, v1, v2), clamped to 0 .. 255, truncated    the transfer's own
 * and with keep_black a source pixel that is (0, 0, 0) stays (0, 0, 0).  Byte for byte what stitch_dev_transfer_form_u8 writes when
 * the statistics it measured are st -- in ONE launch whatever count is, with no float plane stored or read.  The pointer table goes up
 * from a host copy the call makes, so the call WAITS for `stream` before it returns, as stitch_dev_transfer_many_u8 does.
 * STITCH_ERR_ARG for a null pointer, a count outside 1 .. 1024, a bad size or a product that overflows int -- reported before a
 * device is needed. */
int stitch_dev_transfer_given_many_u8(const uint8_t *const *d_src, uint8_t *const *d_out, int count, int w, int h, const float *d_stats12,
                                      int keep_black, void *stream);

/* ---- the filter: enqueued on `stream`, does NOT wait -----------------------------------------------------------------------------
 * kf = keep / 256.  State: p[12] and a flag `has`.  A measured record m[12] is VALID when its twelve values are finite and its six
 * standard deviations (m[3..5], m[9..11]) are > 0.  Record after record, in order:
 *     m not valid             u = m (copied, not computed); the state is untouched
 *     m valid, no state       u = m; the state becomes m, has = 1
 *     m valid, a state        u[j] = m[j] + kf * (p[j] - m[j]), every operation rounded to float; the state becomes u
 * keep = 0 gives u = m bit for bit; a stream of identical records gives u = m for any keep.
 * d_measured, d_used: DEVICE, count * 12 floats each (d_used may be d_measured); d_state12: DEVICE, 12 floats, read where *d_has is
 * not 0 and written back; d_has: DEVICE, one int32.  count >= 1, 0 <= keep <= 255, else STITCH_ERR_ARG -- before a device is needed.
 * One launch of one wavefront. */
int stitch_dev_stats_filter_f32(const float *d_measured, int count, int keep, float *d_state12, int32_t *d_has, float *d_used, void *stream);

/* ---- the rig: HOST ONLY, no device needed.  Valid on a rig made with mode 1 or 2; on any other STITCH_ERR_ARG ------------------
 * Smoothing.  From the next replay on every step filters the statistics of its sets through the filter above, one state per step,
 * set after set across launch sequences and calls; the apply pass reads u.  What it adds to the rig's workspaces: a second buffer of
 * 64 * max_sets * n_steps bytes, 4 * max_sets bytes of flags and 64 * n_steps bytes of state, allocated by the first replay with the
 * option set; per step and launch sequence ONE launch of one wavefront between the statistics and the apply pass.
 *
 * A replay that returns an error, or in which any set's status is not STITCH_OK, leaves the rig WITHOUT a state (the option stays).
 * Within that call a set that a step's seam scan refuses enters the filter up to and including that step -- its statistics there are
 * measured before the scan, on a mosaic that still means something -- and at no later step: the sets behind it are filtered as if the
 * refused set had ended there.  A set whose statistics are not valid never enters the state. */
int stitch_rig_set_exposure_smoothing(stitch_rig *rig, int keep);
/* forgets the option and the state */
int stitch_rig_clear_exposure_smoothing(stitch_rig *rig);
/* forgets the state and keeps the option: a scene cut */
int stitch_rig_reset_exposure_state(stitch_rig *rig);
/* stats12: n_steps * 12 floats, one record per step, each valid in the sense above (else STITCH_ERR_ARG); n_steps must be the rig's.
 * Kept on the host; it goes up with the next replay's one upload. */
int stitch_rig_prime_exposure_state(stitch_rig *rig, const float *stats12, int n_steps);
/* *keep = -1 where no smoothing is set.  has (optional): n_steps ints, 1 where the step has a state. */
int stitch_rig_exposure_smoothing(const stitch_rig *rig, int *keep, int32_t *has);
/* The state as the last completed replay, or a later prime, left it: n_steps * 12 floats (zeros for a step without a state).
 * n_steps must be the rig's. */
int stitch_rig_exposure_state(const stitch_rig *rig, float *out, int n_steps);

/* Fixed statistics.  stats12: n_steps * 12 floats, one record per step, the same for every set; every record valid (else
 * STITCH_ERR_ARG).  While set they win over smoothing, whose state is neither read nor written.  A step then runs ONLY the apply with
 * given statistics over the sequence's frames: no template is converted, nothing is measured, no lab plane is touched; a rig whose
 * first replay finds fixed statistics set does not allocate them until a replay needs them. */
int stitch_rig_fix_exposure(stitch_rig *rig, const float *stats12, int n_steps);
int stitch_rig_clear_fixed_exposure(stitch_rig *rig);
/* *n_steps = 0 where none are fixed, else the rig's steps, and out (optional) receives n_steps * 12 floats. */
int stitch_rig_fixed_exposure(const stitch_rig *rig, float *out, int *n_steps);

/* The statistics the apply passes of the last replay READ, set-major, 12 floats per set and step: u under smoothing, the fixed values
 * with fixed statistics.  Copies min(cap_floats, n_sets * n_steps * 12) floats to out (optional) and returns the counts.  n_sets = 0
 * before the first replay, after a replay with neither option at work (it keeps nothing: what it read is what it measured, the
 * `stats` output) and after a replay that returned anything but STITCH_OK or the status of a set; as with `stats`, the records of a
 * set whose status is not STITCH_OK mean nothing.  The `stats` output of stitch_dev_rig_stitch_exposure_u8 stays the MEASURED values
 * under smoothing; with fixed statistics nothing is measured and it receives the fixed values. */
int stitch_rig_last_used_stats(const stitch_rig *rig, float *out, size_t cap_floats, int *n_sets, int *n_steps);

#ifdef __cplusplus
}
#endif
#endif /* STITCH_RIG_EXPOSURE_TEMPORAL_H */
