/* Observability of the fused sweep's hand-offs: an addition to include/stitch.h (same library, same ABI version), kept in a
 * header of its own so that stitch.h's table of 108 entry points stays as it is. */
#ifndef STITCH_HANDOFF_H
#define STITCH_HANDOFF_H
#include <stdint.h>

#include "stitch.h"

#ifdef __cplusplus
extern "C" {
#endif
/* What the fused sweeps of the plan's calls have handed from row band to row band since the plan was created (waits for the
 * plan's last call): out[0] y states published in full, out[1] y states that were +0 in every column and went out as one word,
 * out[2] tiles of the level-0 mask blur recorded instead of stored.  Cumulative, like the count of timed-out waits.  A call adds the
 * hand-offs of the planes it sweeps: the mask plane of a slot whose pyramid stands (stitch_mask_keep.h) is not swept, so a call adds
 * one plane in seven less per standing slot, and nothing to out[2] for it. */
int stitch_plan_handoff_counts(stitch_plan *plan, uint64_t out[3]);
#ifdef __cplusplus
}
#endif
#endif
