/* Observability of the level-0 index planes kept in 16-byte runs (csrc/k_compose.inc, SrcRuns / k_src_runs; the rule itself:
 * csrc/src_runs_rule.h): an addition to include/stitch.h (same library, same ABI version), kept in a header of its own like
 * stitch_index_plane.h so that stitch.h's table of entry points stays as it is. */
#ifndef STITCH_SRC_RUNS_H
#define STITCH_SRC_RUNS_H
#include <stdint.h>

#include "stitch.h"

#ifdef __cplusplus
extern "C" {
#endif
/* Behind every index plane it computes, a plan that can run source-fused derives a compact form per 64 x 64 tile.  A group is four
 * horizontally adjacent canvas pixels, the first at a column that is a multiple of 4; its base is the byte offset of its first
 * pixel's frame sample within a channel plane, usable only if that sample exists and the 16 bytes from it lie wholly inside the plane
 * (otherwise the base is "outside" and delivers zeros).  A patch is a pixel whose sample is not base + 4j (or, under an outside base,
 * any pixel that has a sample).  A tile's class is its number of patches, 0 .. 64, or 255 = general: more than 64 patches, or byte
 * frames.  The causal x sweep of a frame channel (k_vv_x_fwd<float, true>) takes a tile of class <= 64 with 16 loads of 16 bytes and
 * at most one patch per lane, and a general tile through the full index plane as before; results are the same bit for bit.
 *
 * For the plan's LAST call (waits for that call), over the planes its pairs read, each plane once:
 *   out[0]  tiles wholly outside the frame (never gathered),
 *   out[1]  tiles with 0 patches,
 *   out[2]  tiles with 1 .. 64 patches,
 *   out[3]  general tiles.
 * All zero for a call whose sweep was not handed the runs: a materialised level 0, stitch_blend_*, the forms that gather in another
 * kernel (one pair in flight, STITCH_RECOMPUTE), a library built with STITCH_NO_SRC_RUNS. */
int stitch_plan_src_run_counts(stitch_plan *plan, uint32_t out[4]);

/* The rule restated on the host, from the map: classes of the tiles of a cw x ch canvas for a frame of fw x fh samples of px_bytes
 * (4 or 1) bytes under map p[8] and offsets (offx, offy).  cls (may be NULL): ceil(ch / 64) * ceil(cw / 64) bytes, row bands
 * outermost.  counts as above.  Needs no device. */
int stitch_src_run_classes(const double p[8], float offx, float offy, int fw, int fh, int cw, int ch, int px_bytes, uint32_t counts[4], uint8_t *cls);

/* Test hook: every byte of the plan's run arrays (all slots) set to `byte`, and no record touched -- a slot whose plane stands is NOT
 * recomputed, so only a plan that has made no source-fused call yet (or one after stitch_plan_clear_fault) may be filled without
 * changing results.  Proves that a computed slot depends on nothing the arrays held before. */
int stitch_plan_src_runs_fill(stitch_plan *plan, int byte);
#ifdef __cplusplus
}
#endif
#endif
