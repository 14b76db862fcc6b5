/* stitch_rig_seams.h -- fixed seams for a rig: given or geometric, with coverage masks (libstitch_hip.so, same ABI version).
 *
 * An addition to include/stitch.h and include/stitch_rig.h, kept in a header of its own so that their tables of entry points
 * stay as they are.  The blend of a pair finds its seam by walking the middle row of both canvases and calling a pixel
 * "present" when it is not 0 -- so a dark pixel moves the seam and a dark frame fails its set.  A rig of fixed cameras can
 * instead keep ONE seam per step for its lifetime: GIVEN by the caller (for example the records of the calibrating
 * panorama), or GEOMETRIC, derived on the device from the cameras' footprints alone.  Content seams stay the default; no
 * call of the other headers changes a byte.
 *
 * A seam is ALWAYS stated by the four integers of the mid-row scan: sum_a_x / n_a (the column sum and the count of the
 * pixels where the warped canvas a is present) and sum_ov_x / n_ov (the same where a and the moved mosaic b both are).
 * ratio, ov, branch, start and the double threshold of branch 0 are recomputed from them under the plan's seam_rule; the
 * other fields of a stitch_seam passed IN are ignored (`float ov` cannot carry rule 1's double threshold).
 */
#ifndef STITCH_RIG_SEAMS_H
#define STITCH_RIG_SEAMS_H
#include <stddef.h>
#include <stdint.h>

#include "stitch.h"
#include "stitch_rig.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- a seam from its four integers: HOST ONLY ------------------------------------------------------------------------------
 * Exactly the arithmetic that ends the device's seam scan: seam_rule 0 divides in double and rounds ratio and ov to float
 * (start = (int)(ov + 1.f)), seam_rule 1 keeps both in double (start = (int)(ov + 1.0)); branch = ratio < ov ? 0 : 1.  cw
 * is the width of the canvas the seam is for.  STITCH_ERR_ARG unless 1 <= n_ov <= n_a <= cw, sum_ov_x <= sum_a_x, and each
 * sum is a possible sum of n distinct columns of 0 .. cw-1: n(n-1)/2 <= sum <= n*cw - n(n+1)/2.  seam_rule outside 0 .. 1,
 * cw < 1 and a null `out` are STITCH_ERR_ARG as well. */
int stitch_seam_from_sums(int32_t sum_a_x, int32_t n_a, int32_t sum_ov_x, int32_t n_ov, int seam_rule, int cw, stitch_seam *out);

/* ---- pairs with given seams: enqueued on `stream` --------------------------------------------------------------------------
 * Byte for byte stitch_dev_pairs_u8 / _f32, except that pair i's seam comes from the four integers of seams[i] (a HOST
 * array of n records, read before the call returns) instead of the scan.  stitch_plan_status_at afterwards returns
 * STITCH_OK and the record as stitch_seam_from_sums derives it under the plan's seam_rule.  A record that fails the checks
 * above against the plan's canvas width is STITCH_ERR_ARG naming the pair, reported before anything is enqueued. */
int stitch_dev_pairs_seamed_u8(stitch_plan *plan, const stitch_pair_desc *pairs, int n, const stitch_seam *seams, void *stream);
int stitch_dev_pairs_seamed_f32(stitch_plan *plan, const stitch_pair_desc *pairs, int n, const stitch_seam *seams, void *stream);

/* ---- a rig with fixed seams: HOST ONLY -------------------------------------------------------------------------------------
 * stitch_rig_fix_seams: n_steps must be the rig's step count; record k is checked against step k's canvas width (an error
 * is STITCH_ERR_ARG naming the step and leaves the rig as it was).  From then on every replay -- stitch_dev_rig_stitch_u8
 * and stitch_dev_rig_stitch_exposure_u8 -- uses these seams for every set: every set_status is STITCH_OK (a dark frame is
 * stitched dark), and `seams` out holds the fixed records for every set.  The calls still wait for the stream; the rest of
 * the contract of stitch_rig.h stays.  A rig with zero steps takes n_steps = 0 and fixes nothing.
 * stitch_rig_clear_seams returns to content seams.  stitch_rig_seams returns the number of fixed steps (0: content seams)
 * and copies up to `cap` of the records to `out` (optional), as the rig's blend options derive them. */
int stitch_rig_fix_seams(stitch_rig *rig, const stitch_seam *seams, int n_steps);
int stitch_rig_clear_seams(stitch_rig *rig);
int stitch_rig_seams(const stitch_rig *rig, stitch_seam *out, int cap);

/* ---- geometric seams and coverage ------------------------------------------------------------------------------------------
 * Coverage is where an image CAN have data, whatever its pixels hold:
 *   C_proj(i)[y][x] = the cylindrical projection's own inside test for frame i's size and the rig's fov_deg (the source
 *                     coordinate (u, v) of output pixel (x, y) satisfies 0 <= u < width and 0 <= v < height);
 *   step k, canvas cw x ch, warping frame dst with map p and offsets (offx, offy), the mosaic shifted by (ox, oy):
 *     A[y][x] = the map sends (x + offx, y + offy) to a sample (nx, ny) inside frame dst, and C_proj(dst)[ny][nx];
 *     B[y][x] = (x + ox, y + oy) lies inside the mosaic before the step, and C_mos(k-1)[y + oy][x + ox];
 *     C_mos(k) = A | B;       C_mos(-1) = C_proj(start).
 * The geometric seam of step k is the reference's scan of row ch / 2 over coverage: sum_a_x / n_a over A, sum_ov_x / n_ov
 * over A & B.
 *
 * stitch_dev_rig_geometric_seams computes them on the device (once per rig: the coverage planes stay in the rig, one bit
 * per pixel, and are freed by stitch_rig_destroy), fixes them as stitch_rig_fix_seams does and copies them to seams_out
 * (optional, n_steps records).  A step whose scan has n_a == 0 or n_ov == 0 makes the call return STITCH_ERR_EMPTY_MIDROW /
 * STITCH_ERR_ZERO_OVERLAP naming the step; the rig's seams are then exactly what they were.  Zero steps: succeeds, fixes
 * nothing.  The call WAITS for `stream`.
 *
 * stitch_dev_rig_coverage_u8 writes cw * ch bytes, 0 or 255, of step `step`'s canvas to d_mask (device): which = 0: A,
 * 1: B, 2: A | B.  step == -1 is the last step, whose A | B is the validity mask of the output mosaic; for a rig with zero
 * steps that is C_proj(start), whatever `which`.  Works on any rig, whatever its seam mode, and does not change it.  The
 * first of these two calls on a rig computes the planes on the current device and waits for `stream`; after that
 * stitch_dev_rig_coverage_u8 is enqueued on `stream` and returns.  Later calls must run on the same device.
 * Argument errors (a null rig or d_mask, step outside -1 .. n_steps-1, which outside 0 .. 2) are reported before a device
 * is needed. */
int stitch_dev_rig_geometric_seams(stitch_rig *rig, stitch_seam *seams_out, void *stream);
int stitch_dev_rig_coverage_u8(stitch_rig *rig, int step, int which, uint8_t *d_mask, void *stream);
/* HOST ONLY: the canvas of step `step`, the size of its masks (-1: the last step, i.e. the output; for a rig with zero steps the
 * projected start frame).  STITCH_ERR_ARG for a null argument or a step outside -1 .. n_steps-1. */
int stitch_rig_step_canvas(const stitch_rig *rig, int step, int *cw, int *ch);

#ifdef __cplusplus
}
#endif
#endif /* STITCH_RIG_SEAMS_H */
