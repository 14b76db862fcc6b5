/* The mask pyramid a plan keeps per slot while the slot's seam repeats (csrc/k_compose.inc, MaskKey; csrc/stitch_call_form.h,
 * mask_keep_word): an addition to include/stitch.h (same library, same ABI version), kept in a header of its own like
 * stitch_index_plane.h so that stitch.h's table of entry points stays as it is. */
#ifndef STITCH_MASK_KEEP_H
#define STITCH_MASK_KEEP_H
#include <stdint.h>

#include "stitch.h"

#ifdef __cplusplus
extern "C" {
#endif
/* The blend mask of a pair is a vertical step, and its pyramid -- the mask plane of every level below the first, the row-repeat flags
 * of levels 1 and 2, the level-0 blur handed down to them -- is a function of the seam record's branch, start and thr, the plan, and
 * the call's form (which tiles of a mask plane its kernels store at all).  No pixel reaches it except through the seam scan.  The plan
 * keeps, on the device, what the pyramid in each of its slots was computed from (by bit pattern), and a call whose kernels all know
 * the skip leaves the pyramid of a slot standing, bit for bit, where the record repeats: behind the launch that writes the call's seam
 * records, in stream order, so a captured call decides again on every replay.
 *   A slot stands only under the form it was written under, never where the seam scan failed (status != 0), and only on a plan with
 * the implicit level-0 mask in calls whose kernels all know the skip.  Every other call -- one pair whose level takes the five-wavefront
 * fused sweep, path seams, a plan without the implicit mask, STITCH_RECOMPUTE, Deriche -- computes every mask plane and takes the
 * slots it wrote over with a form under which nothing stands; stitch_plan_clear_fault forgets every record.  The band
 * path and the coarse plan of a split pair never take part.
 *   For the plan's LAST call (waits for that call):
 *   out[0]  slots whose mask planes the call computed,
 *   out[1]  slots whose mask planes stood from an earlier call.
 * out[0] + out[1] = the call's pairs.  A library built with STITCH_NO_MASK_KEEP computes every mask plane on every call: (pairs, 0). */
int stitch_plan_mask_keep_counts(stitch_plan *plan, uint32_t out[2]);
/* stitch_plan_call_forms: a call with that many pairs is of a form under which mask pyramids stand.  The bit shares the answer with
 * the STITCH_FAST_* values of stitch.h (1 .. 32 are taken there): the next value added on either side is 128. */
#define STITCH_CALL_MASK_KEEP 64
#ifdef __cplusplus
}
#endif
#endif
