/* Observability of the level-0 index planes a plan keeps (csrc/k_compose.inc, IndexKey): an addition to include/stitch.h (same
 * library, same ABI version), kept in a header of its own like stitch_g_flags.h so that stitch.h's table of entry points stays as it
 * is. */
#ifndef STITCH_INDEX_PLANE_H
#define STITCH_INDEX_PLANE_H
#include <stdint.h>

#include "stitch.h"

#ifdef __cplusplus
extern "C" {
#endif
/* A source-fused call of stitch_dev_pairs_* gathers each pair's warped frame through an index plane: 4 bytes per canvas pixel, a
 * function of the pair's map p[8], offx, offy, fw, fh and the pixel type alone.  The plan keeps, on the device, what the plane in each
 * of its slots was computed from (all by bit pattern: -0.0 is not 0.0), so a slot whose descriptor repeats these fields keeps its plane,
 * and pairs of one call with equal fields share the plane of the first of them.  For the plan's LAST call (waits for that call):
 *   out[0]  slots whose plane the call computed,
 *   out[1]  slots whose plane stood from an earlier call,
 *   out[2]  pairs that read the plane of an earlier pair of the same call.
 * out[0] + out[1] + out[2] = the call's pairs.  All zero for a call without index planes: a materialised level 0 (which also forgets
 * the planes of the slots it overwrote), stitch_blend_*.  A captured call decides again on every replay; the counts are those of the
 * last launch whose copy has arrived.  stitch_plan_clear_fault forgets every plane.  A library built with STITCH_NO_INDEX_REUSE
 * computes every plane on every call: (pairs, 0, 0). */
int stitch_plan_index_counts(stitch_plan *plan, uint32_t out[3]);
#ifdef __cplusplus
}
#endif
#endif
