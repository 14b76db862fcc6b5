/* Observability of the G column flags (csrc/k_compose.inc, g_cols): an addition to include/stitch.h (same library, same ABI
 * version), kept in a header of its own like stitch_handoff.h so that stitch.h's table of entry points stays as it is. */
#ifndef STITCH_G_FLAGS_H
#define STITCH_G_FLAGS_H
#include <stdint.h>

#include "stitch.h"

#ifdef __cplusplus
extern "C" {
#endif
/* Tile columns (64 columns, all rows of one plane) of the pyramid levels 1 (out[0]) and 2 (out[1]) that the plan's LAST call
 * recorded as all +0 instead of storing them, summed over the call's pairs and planes (waits for that call).  0 for a level
 * whose flags the call did not use: an odd width of the level above, a lone pair's kernels, the band path, a library built
 * with STITCH_NO_G_FLAGS.  A tile column is recorded only if both neighbouring tile columns are all +0 as well (the plane's edge
 * counts as one), and tile column t of level l only if 2t + 1 < ceil(w_{l-1} / 64): where the level above has an odd count of
 * tile columns, the last two tile columns of level l are never recorded, whatever they hold. */
int stitch_plan_g_flag_counts(stitch_plan *plan, uint64_t out[2]);
#ifdef __cplusplus
}
#endif
#endif
