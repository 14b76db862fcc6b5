/* stitch_seam_anchor.h -- temporally anchored path seams: coherent seam paths across a rig's sets (libstitch_hip.so, same ABI version).
 *
 * An addition to include/stitch_seam_path.h, kept in a header of its own so that its table of entry points stays as it is.  The
 * finder of that header gives every set of a rig its own least-cost path, independently of the set before it; where two routes
 * through the overlap cost nearly the same, sensor noise decides between them and the seam jumps from frame to frame.  Here the
 * finder's cost takes a term that prices moving away from a given path, the ANCHOR, and a rig carries the previous set's path
 * forward on the device as the next set's anchor, with no host round trip.  No call of the other headers changes a byte.
 *
 * An ANCHOR of a cw x ch canvas is ch values r[y] of int32_t.  Any integer is valid.  With a weight w and a cap T the row cost of
 * stitch_seam_path.h becomes
 *   c_t(y, s) = c(y, s) + w * min(|s - r[y]|, T)        for s = 0 .. cw,
 * |s - r[y]| taken in 64 bits, so r = INT32_MIN and r = INT32_MAX are valid.  c, D, the predecessor tie rule, the end tie rule and
 * the walk back are exactly those of stitch_seam_path.h with c_t in place of c; row 0 is included.
 * Limits: 0 <= w, 1 <= T, w * T <= STITCH_SEAM_ANCHOR_MAX (2055), so 2040 + w * T < 4096: one pixel on the wrong side still costs
 * more than any crossing plus any temporal penalty, and coverage always wins.  c_t stays below 2^26, so all arithmetic stays exact
 * in the words stitch_seam_path.h uses.
 * Besides the path and its total D the result carries
 *   moved = sum over y of min(|s[y] - r[y]|, T)        (uint64_t),
 * so D = (the path's cost under c) + w * moved.  With no anchor the term is absent: the result is the unanchored finder's, bit for
 * bit, with moved = 0.  It follows that w = 0 gives the unanchored result; that with w > 0 the anchor that is a pair's own
 * unanchored path returns that path, with the same D and moved = 0; and that an anchor at least T away from every column 0 .. cw on
 * every row gives the unanchored path with D + ch * w * T.
 */
#ifndef STITCH_SEAM_ANCHOR_H
#define STITCH_SEAM_ANCHOR_H
#include <stddef.h>
#include <stdint.h>

#include "stitch.h"
#include "stitch_rig.h"
#include "stitch_seam_path.h"

#ifdef __cplusplus
extern "C" {
#endif

#define STITCH_SEAM_ANCHOR_MAX 2055 /* the largest weight * cap */
#define STITCH_SEAM_ANCHOR_PER_SET 1
#define STITCH_SEAM_ANCHOR_PER_CALL 2

/* No defaults: which weight suits which footage is the caller's to state. */
typedef struct stitch_seam_anchor_opts {
    int32_t weight; /* w: 0 .. 2055 */
    int32_t cap;    /* T: 1 .. 2055, weight * cap <= 2055 */
    int32_t policy; /* a rig's: STITCH_SEAM_ANCHOR_PER_SET or STITCH_SEAM_ANCHOR_PER_CALL; ignored by the stand-alone call */
} stitch_seam_anchor_opts;

/* ---- the anchored finder ---------------------------------------------------------------------------------------------------------
 * stitch_dev_pairs_seam_path_u8 (every argument, rule and error of that call) plus: d_anchors, a HOST array of n DEVICE pointers to
 * ch int32_t each -- a null entry leaves that pair unanchored, entries may alias each other; aopts, the weight and the cap (policy
 * is ignored); d_moved, device memory of n uint64_t.  An anchor must not lie inside the call's own d_paths.  Null d_anchors, aopts
 * or d_moved, and options outside the limits above, are STITCH_ERR_ARG, reported before a device is needed. */
int stitch_dev_pairs_seam_path_anchored_u8(const stitch_pair_desc *pairs, int n, int cw, int ch, const uint8_t *const *d_cov_a,
                                           const uint8_t *const *d_cov_b, const int32_t *branches, const stitch_seam_path_opts *opts,
                                           const int32_t *const *d_anchors, const stitch_seam_anchor_opts *aopts, int32_t *d_paths, uint64_t *d_costs,
                                           uint64_t *d_moved, void *stream);

/* ---- a rig that anchors: HOST ONLY -------------------------------------------------------------------------------------------------
 * The options take effect while mode 1 (stitch_rig_set_seam_paths) is set; mode 2 and mode 0 ignore them.  The rig keeps one anchor
 * per step on the device -- the rows of a set's paths -- and whether it has one.  A rig that never sets the options allocates
 * nothing more, launches nothing more and writes every path and byte it wrote before.
 * STITCH_SEAM_ANCHOR_PER_SET: set i of the stream of sets anchors on set i - 1.  The stream runs across launch sequences and across
 * calls; the first set after a reset is unanchored.  Within a sequence the dynamic programmes of a step run one after another.
 * STITCH_SEAM_ANCHOR_PER_CALL: every set of a call anchors on the last set of the previous call: one parallel finder sequence per
 * step, as without an anchor.  The anchor is replaced once, at the end of the call.
 * Neither depends on how the rig's max_sets cuts a call into sequences, PER_SET not on how the caller cuts the stream into calls
 * either; with one set per call the two coincide.  A replay that fails leaves the rig without an anchor.
 * stitch_rig_set_seam_anchor: options outside the limits, or a policy other than the two, are STITCH_ERR_ARG and leave the rig as
 * it was; an anchor the rig has stays.
 * stitch_rig_prime_seam_anchor: one HOST path per step (the step's ch columns, copied) becomes the anchor -- paths saved from an
 * earlier run, or the geometric seam's constant path.  n_steps other than the rig's, or a null path, is STITCH_ERR_ARG and leaves
 * the rig as it was.
 * stitch_rig_reset_seam_anchor forgets the anchor and keeps the options: the call for a scene cut.
 * stitch_rig_clear_seam_anchor forgets both; so does stitch_rig_clear_seam_paths with the anchor (it keeps the options).
 * stitch_rig_seam_anchor: *opts = the options (all zero where none are set), *has_anchor = 0 or 1 (both optional). */
int stitch_rig_set_seam_anchor(stitch_rig *rig, const stitch_seam_anchor_opts *opts);
int stitch_rig_prime_seam_anchor(stitch_rig *rig, const int32_t *const *paths, int n_steps);
int stitch_rig_reset_seam_anchor(stitch_rig *rig);
int stitch_rig_clear_seam_anchor(stitch_rig *rig);
int stitch_rig_seam_anchor(const stitch_rig *rig, stitch_seam_anchor_opts *opts, int *has_anchor);

/* HOST ONLY: *moved of the path of `set` at `step` in the last replay along paths (0 where that set had no anchor, and for fixed
 * paths); the cost stitch_rig_last_seam_paths returns for it is then the anchored D.  A set or step the last such replay did not
 * have, or a null pointer, is STITCH_ERR_ARG. */
int stitch_rig_last_seam_moved(const stitch_rig *rig, int set, int step, uint64_t *moved);

#ifdef __cplusplus
}
#endif
#endif /* STITCH_SEAM_ANCHOR_H */
