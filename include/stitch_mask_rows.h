/* Observability of the row-repeat flags of the mask plane (csrc/k_compose.inc, mask_rows): an addition to include/stitch.h (same
 * library, same ABI version), kept in a header of its own like stitch_g_flags.h so that stitch.h's table of entry points stays as
 * it is.
 *
 * The rule.  The blend's mask is a vertical step, so every row of the level-0 mask is the same row, and below a level whose width
 * AND height are even the blurred and decimated mask still repeats its row 0, bit for bit, except in the last few rows at the
 * bottom, in the columns of the seam's ramp, where the anticausal y sweep starts from its Triggs boundary instead of its fixed
 * point.  For the mask plane of pyramid levels 1 and 2 of a batch the producing sweep keeps one byte per (pair, 64-column tile
 * column, 64-row band).  A set byte of a band b >= 1 means: every existing row of that tile equals row 0 of the plane in its 64
 * columns, and the tile was not stored.  Band 0 is always stored and never flagged; every byte is written on every call.  Below an
 * odd height the decimation's overlap weights change from row to row and nearly every column differs, so a level below a level of
 * odd width or height has no flags, and neither has any level below that one. */
#ifndef STITCH_MASK_ROWS_H
#define STITCH_MASK_ROWS_H
#include <stdint.h>

#include "stitch.h"

#ifdef __cplusplus
extern "C" {
#endif
/* Flagged (tile column, band) entries of the mask plane of the pyramid levels 1 (out[0]) and 2 (out[1]) in the plan's LAST call,
 * summed over the call's pairs and counted on the host from the flag bytes (waits for that call).  0 for a level whose flags the
 * call did not use: an odd width or height of a level above, no G column flags (stitch_g_flags.h), STITCH_NO_ZERO_TILES=1, a
 * library built with STITCH_NO_MASK_ROWS. */
int stitch_plan_mask_row_counts(stitch_plan *plan, uint64_t out[2]);
#ifdef __cplusplus
}
#endif
#endif
