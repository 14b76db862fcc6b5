/* stitch_seam_path.h -- path seams: a least-cost seam column per row, for pairs and rigs (libstitch_hip.so, same ABI version).
 *
 * An addition to include/stitch.h and include/stitch_rig_seams.h, kept in a header of its own so that their tables of entry points
 * stay as they are.  Every other blend of the library cuts its two inputs along one vertical line: the level-0 mask is the step
 * `x < thr` or `x >= start` of a stitch_seam.  Here the level-0 mask is STORED, written from one column per row, a finder
 * chooses those columns by a least-cost dynamic programme over the overlap, and a rig does both per set and step inside its
 * replay.  No call of the other headers changes a byte.
 *
 * A PATH on a cw x ch canvas is ch values s[y] of int32_t, plus a branch:
 *   branch 0: the level-0 mask is M[y][x] = 1 (take a, the warped frame) where x <  s[y];
 *   branch 1:                     M[y][x] = 1                            where x >= s[y].
 * Any integer is valid: s <= 0 or s >= cw makes the row all one side.  The vertical seam of a stitch_seam is the path whose columns
 * are all ceil(thr) (branch 0) or all `start` (branch 1); a blend with that path is the blend with that seam, bit for bit.
 *
 * THE PATH'S COST.  For one pair:
 *   a = the zero-initialised canvas after stitch_warp_u8(frame, p, offx, offy),
 *   b = the zero-initialised canvas after stitch_move_u8(mosaic, ox, oy),
 * both exactly as the stitch step builds them (as in include/stitch_rig_monitor.h), g = R + 2 * G + B (0 .. 1020), two coverage
 * masks A and B (where a and b can have data), a margin m (0 .. STITCH_SEAM_PATH_MAX_MARGIN) and a step bound K
 * (1 .. STITCH_SEAM_PATH_MAX_STEP):
 *   A'[y][x]    = A[y][x'] for every x' in [x - m, x + m] inside the canvas (horizontal erosion; positions outside the canvas ask
 *                 nothing); B' likewise.
 *   d[y][x]     = | g_a[y][x] - g_b[y][x] | where A & B, 0 elsewhere; columns -1 and cw read as 0.
 *   wrong(y, s) = #{ x < s : x in L } + #{ x >= s : x in R }, for s in 0 .. cw, with
 *                 branch 0: L = B & ~A',  R = A & ~B';      branch 1: L = A & ~B',  R = B & ~A'.
 *   c(y, s)     = 4096 * wrong(y, s) + d[y][s - 1] + d[y][s]          (4096 exceeds the largest crossing cost, 2040)
 *   D(0, s)     = c(0, s)
 *   D(y, s)     = c(y, s) + min over t in [s - K, s + K] and [0, cw] of D(y - 1, t)
 * The predecessor of (y, s) is the minimising t; ties go to the smallest |t - s|, then to the smaller t.
 * s[ch - 1] = argmin over s of D(ch - 1, s), ties to the smallest s; the path follows the predecessors upward.  The result is the
 * path and its total D as a uint64_t.  c is below 2^26 and ch at most 65535, so D stays below 2^44: all arithmetic is exact.
 */
#ifndef STITCH_SEAM_PATH_H
#define STITCH_SEAM_PATH_H
#include <stddef.h>
#include <stdint.h>

#include "stitch.h"
#include "stitch_rig.h"

#ifdef __cplusplus
extern "C" {
#endif

#define STITCH_SEAM_PATH_MAX_STEP 8
#define STITCH_SEAM_PATH_MAX_MARGIN 64
#define STITCH_SEAM_PATH_MAX_WIDTH 8192 /* the finder: two rows of 64-bit states for cw + 1 columns fit one CU's LDS */

typedef struct stitch_seam_path_opts {
    int32_t max_step; /* K: 1 .. 8 */
    int32_t margin;   /* m: 0 .. 64 */
} stitch_seam_path_opts;

/* max_step = 2, margin = 8 */
void stitch_seam_path_opts_default(stitch_seam_path_opts *opts);

/* ---- a masked plan ---------------------------------------------------------------------------------------------------------
 * A workspace as stitch_plan_create_batched makes it, except that its level-0 mask is a stored plane: no implicit mask, no source
 * fusion, no G column or mask-row flags.  Level 0 is composed from the pairs' frames.  It is the workspace of
 * stitch_dev_pairs_pathed_* (below) and of nothing else: stitch_dev_pair_*, stitch_dev_pairs_*, stitch_dev_pairs_seamed_* and
 * stitch_dev_blend_* on a masked plan are STITCH_ERR_ARG.  Arguments as stitch_plan_create_batched;
 * released by stitch_plan_destroy.  stitch_plan_is_masked: 1 for such a plan, 0 for any other, STITCH_ERR_ARG for null. */
int stitch_plan_create_masked(int cw, int ch, const stitch_blend_opts *opts, int max_pairs, stitch_plan **plan_out);
int stitch_plan_is_masked(const stitch_plan *plan);

/* ---- the blend along given paths: enqueued on `stream`, no host wait --------------------------------------------------------
 * n pairs (1 <= n <= the plan's capacity) through ONE launch sequence: level 0 from the frames, the mask from the paths, REDUCE,
 * collapse.  pairs as stitch_dev_pairs_*.  d_paths: a HOST array of n DEVICE pointers to ch int32_t each (entries may alias);
 * branches: a HOST array of n values, 0 or 1.  There is no seam scan: stitch_plan_status_at returns STITCH_OK and a zeroed record
 * that carries the pair's branch.  The plan must be masked; a null pointer, an unmasked plan, n out of range, a null path and a
 * branch other than 0 or 1 are STITCH_ERR_ARG. */
int stitch_dev_pairs_pathed_u8(stitch_plan *plan, const stitch_pair_desc *pairs, int n, const int32_t *const *d_paths, const int32_t *branches,
                               void *stream);
int stitch_dev_pairs_pathed_f32(stitch_plan *plan, const stitch_pair_desc *pairs, int n, const int32_t *const *d_paths, const int32_t *branches,
                                void *stream);

/* ---- the finder: the least-cost path of each of n pairs, by the definition above ---------------------------------------------
 * pairs: a HOST array of n descriptors, 1 <= n <= 65535; frame, fw, fh, p, offx, offy, mosaic, mw, mh, ox, oy are read, out and
 * out_u8 are ignored.  d_cov_a, d_cov_b: HOST arrays of n device pointers to dense cw * ch byte masks (non-zero = covered;
 * entries may alias).  branches: a HOST array of n values, 0 or 1.  d_paths: device memory of n * ch int32_t, pair-major;
 * d_costs: device memory of n uint64_t.  Two launches: the costs c of every row in parallel, then one workgroup per pair for the
 * dynamic programme and the walk back.  Scratch (4 * (cw + 1) * ch bytes of costs and (cw + 1) * ch bytes of predecessors per pair)
 * comes from the stream-ordered allocator.  The descriptors go up from a host copy, so the call WAITS for `stream`, as
 * stitch_dev_pairs_residual_u8 does.  Argument errors -- a null pointer, a pair without a frame, a mosaic or a mask, a size < 1,
 * max_step outside 1 .. 8, margin outside 0 .. 64, cw > 8192, ch > 65535, n out of range, a branch other than 0 or 1 -- are
 * reported before a device is needed.  opts may be null: the defaults. */
int stitch_dev_pairs_seam_path_u8(const stitch_pair_desc *pairs, int n, int cw, int ch, const uint8_t *const *d_cov_a, const uint8_t *const *d_cov_b,
                                  const int32_t *branches, const stitch_seam_path_opts *opts, int32_t *d_paths, uint64_t *d_costs, void *stream);

/* ---- a rig with path seams: HOST ONLY ------------------------------------------------------------------------------------------
 * While a mode is set every replay -- stitch_dev_rig_stitch_u8, stitch_dev_rig_stitch_exposure_u8, stitch_dev_rig_stitch_fmt_u8,
 * with or without a crop or a monitor -- blends every step along paths, on masked plans the rig creates beside its own from the
 * first such replay on.  The branch of a step is that of its geometric seam over coverage (stitch_dev_rig_geometric_seams): the
 * first such replay computes the coverage planes if the rig has none yet, and a step whose geometric scan fails makes it return
 * that error (STITCH_ERR_EMPTY_MIDROW, STITCH_ERR_ZERO_OVERLAP), the message naming the step.  The `seams` output of a replay
 * carries the geometric records, and every set_status is STITCH_OK, as with fixed seams; fixed seams (stitch_rig_fix_seams) rest
 * while a mode is set.  A rig that never sets a mode allocates nothing, launches nothing more and writes every byte it wrote
 * before.
 * stitch_rig_set_seam_paths (mode 1): every set finds its own path per step -- one finder sequence per step over the sets in
 * flight, from exactly the inputs that step's blend receives (the projected frame after the exposure transfer where the rig has
 * one, and the running mosaic), over the step's coverage planes A_k and B_k -- and blends along it, with no host round trip.
 * opts may be null: the defaults.  Options out of range, or a step whose canvas is wider than 8192 or higher than 65535, are
 * STITCH_ERR_ARG and leave the rig as it was.
 * stitch_rig_fix_seam_paths (mode 2): one HOST path per step (the step's ch columns, copied), shared by all sets.  n_steps other
 * than the rig's, or a null path, is STITCH_ERR_ARG and leaves the rig as it was.
 * stitch_rig_clear_seam_paths: no mode (also forgets the last paths).  stitch_rig_seam_paths: *mode = 0, 1 or 2 and *opts = the
 * finder's options (both optional). */
int stitch_rig_set_seam_paths(stitch_rig *rig, const stitch_seam_path_opts *opts);
int stitch_rig_fix_seam_paths(stitch_rig *rig, const int32_t *const *paths, int n_steps);
int stitch_rig_clear_seam_paths(stitch_rig *rig);
int stitch_rig_seam_paths(const stitch_rig *rig, int *mode, stitch_seam_path_opts *opts);

/* HOST ONLY: the path of `set` at `step` in the last replay along paths: up to `cap` of its ch columns to `out` (optional when cap
 * is 0), *cost = its cost under the finder's definition (optional; 0 for fixed paths, whose cost nobody computed).  Returns ch.  So
 * a caller can find paths on one set and fix them for all.  A set or step the last such replay did not have is STITCH_ERR_ARG; a
 * replay that failed leaves no paths. */
int stitch_rig_last_seam_paths(const stitch_rig *rig, int set, int step, int32_t *out, int cap, uint64_t *cost);

#ifdef __cplusplus
}
#endif
#endif /* STITCH_SEAM_PATH_H */
