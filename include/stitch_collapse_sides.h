/* Observability of the level-0 collapse that reads only the image the seam's step selects (csrc/k_pyramid.inc, k_collapse4 /
 * collapse_cols4): an addition to include/stitch.h (same library, same ABI version), kept in a header of its own like
 * stitch_g_flags.h so that stitch.h's table of entry points stays as it is. */
#ifndef STITCH_COLLAPSE_SIDES_H
#define STITCH_COLLAPSE_SIDES_H
#include <stdint.h>

#include "stitch.h"

#ifdef __cplusplus
extern "C" {
#endif
/* At level 0 of a call whose mask is the seam's step, a workgroup of the four-column collapse owns 256 adjacent columns of the range
 * stitch_plan_collapse_range reports for level 0 (as the last call's addresses left it).  Where the step has one value over all of
 * them the workgroup reads one image only.  For pair `pair` of the plan's LAST call (waits for that call; the rule is evaluated on
 * the host, on the seam record stitch_plan_status_at copies, by the function the kernel evaluates):
 *   counts[0]  column blocks that read only image a (the step is 1),
 *   counts[1]  column blocks that read only image b (the step is 0),
 *   counts[2]  column blocks that read both.
 * All zero for a call whose level 0 does not take the four-column collapse.  Every block counts as "both" for a call without the step
 * mask (planes handed in) and in a library built with STITCH_NO_C4_SIDES. */
int stitch_plan_collapse_sides(stitch_plan *plan, int pair, int counts[3]);

/* Verification hook beside stitch_dev_check_collapse_taps: ONE level-0 collapse of a w x h level (even w >= 256, even h >= 4, both
 * <= 16384) over materialised synthetic planes, under the step of the given branch (0: 1 where x < seam_x, 1: 1 where x >= seam_x;
 * 0 <= seam_x <= w), once by k_collapse4 with its one-sided forms and once by k_collapse, which keeps the full arithmetic; the two
 * outputs are compared bit for bit.
 *   probe 0  pseudo-random finite samples of both signs;
 *   probe 1  signed zeros: every kept Laplacian term is +0 or -0 while the dropped one has either sign, E of the coarser level holds
 *            -0 and tiny negative samples next to zeros (their interpolation underflows to -0): rows on both sides of the seam have to
 *            be redone with the dropped image, or signs of zeros come out wrong.
 * counts (may be NULL): the a-only / b-only / both column blocks of the k_collapse4 launch. */
int stitch_dev_check_collapse_sides(int w, int h, int probe, int branch, int seam_x, unsigned long long *compared, unsigned long long *mismatches,
                                    int counts[3]);
#ifdef __cplusplus
}
#endif
#endif
