/* stitch_calibrate.h -- a rig calibrated from several captures: pooled matches, one set of maps (libstitch_hip.so, same ABI
 * version).
 *
 * An addition to include/stitch_panorama.h and include/stitch_rig.h, kept in a header of its own so that their tables of entry
 * points stay as they are.  A rig (stitch_rig.h) replays one stitch order and one set of maps.  stitch_rig_from_panorama takes
 * them from ONE whole-panorama call on ONE frame set: that call blends every step although the maps depend on key points only,
 * decides which cameras are neighbours on one capture's match counts, and fits every map to one capture's accepted pairs.  The
 * calls below take n_sets captures of the same n cameras and return one stitch order and one set of steps that feed
 * stitch_rig_create / stitch_rig_create_exposure unchanged.  No pixel is warped or blended.
 *
 * The chain (computervisionimagestich2_amd/pipeline.py calibrate_from_sets spells it out on the stage calls):
 *   1. Per frame: projection + gray, SIFT, the std::map order -- as stitch_dev_panorama_u8 does, over all n_sets * n frames in
 *      ONE stitch_dev_sift_many call.  The heads come back in one read-back for all frames, the descriptor rows in one more, the
 *      index arrays go up once: the host waits as often as for one capture.
 *   2. Camera i must have the same decoded size in every capture.
 *   3. The ordered x and y of camera i from all captures lie in ONE device array per camera, capture-major; capture k's rows
 *      start at the base B[k][i] = the number of rows of camera i in the captures before k.  One stitch_dev_map_points or
 *      stitch_dev_shift_points launch updates a camera's points in every capture, and one RANSAC list can address a pooled list.
 *   4. getImgPair for every capture and every ordered camera pair in ONE stitch_dev_match_l1_ratio_many call.
 *      pooled[i][j] = the sum over the captures of count_k[i][j], formed on the device; the host reads the counts once.
 *   5. The order is stitch_stitch_order(pooled, n, T): T = pooled_threshold, or n_sets * match_threshold when that is 0 -- two
 *      cameras are neighbours when their MEAN count reaches the reference's 20.
 *   6. Step (src, dst): the pooled list for (data = src, queries = dst) is the captures' accepted lists one behind the other in
 *      capture order, capture k's indices moved by B[k][src] and B[k][dst]; likewise for the other direction.  The longer-list
 *      rule of ImageProcess.cpp:185-198 is decided ONCE, on the device, on the pooled totals: the first list on a strict >, else
 *      the mirror of the second.  Then both RANSAC runs on the pooled list (stitch_dev_ransac_many, forward = the mirrored list
 *      first), stitch_step_geometry from p_fwd and the running mosaic's size, dst's key points of all captures through the forward
 *      map, and those of the camera warped before (the start camera at first) moved by the integer offsets.
 *   7. With one capture every step is stitch_dev_panorama_u8's, bit for bit: the chain is then the reference's matching()
 *      without the pixels.
 */
#ifndef STITCH_CALIBRATE_H
#define STITCH_CALIBRATE_H
#include <stddef.h>
#include <stdint.h>

#include "stitch_exposure.h"
#include "stitch_panorama.h"
#include "stitch_rig.h"

#ifdef __cplusplus
extern "C" {
#endif

#define STITCH_CALIBRATE_MAX_SETS 64     /* captures per call                                                              */
#define STITCH_CALIBRATE_MAX_FRAMES 1024 /* n_sets * n per call                                                            */
#define STITCH_CALIBRATE_MAX_PAIRS 65536 /* pairs of a pooled list: what stitch_dev_ransac_many tests                       */

typedef struct stitch_calibrate_opts {
    const stitch_panorama_opts *pano; /* NULL: the defaults.  blend, finish, num, den and keep_steps are ignored           */
    int32_t pooled_threshold;         /* 0: n_sets * pano->match_threshold; else the absolute pooled count of neighbours   */
} stitch_calibrate_opts;
void stitch_calibrate_opts_default(stitch_calibrate_opts *o);

typedef struct stitch_calibration stitch_calibration; /* a result: host data only */

/* ---- the chain ---------------------------------------------------------------------------------------------------------
 * 1 <= n <= 64 cameras, 1 <= n_sets <= 64 captures, n_sets * n <= 1024; frames are capture-major (capture 0's cameras first).
 * Outside these limits, for a frame without data or with a bad size, and for a camera whose size differs between captures the
 * calls return STITCH_ERR_ARG before a device is needed and before anything is enqueued.  They report failures of stages that
 * run on the device, so they WAIT for `stream` before they return, as the whole-panorama calls do:
 *   STITCH_ERR_CAPACITY  a frame's SIFT reported STITCH_SIFT_OVERFLOW (the text names the capture and the camera), or a step's
 *                        pooled list is longer than STITCH_CALIBRATE_MAX_PAIRS
 *   STITCH_ERR_NO_MAP    a step's RANSAC did not return STITCH_RANSAC_OK twice: the text names both cameras, both statuses
 *                        and the pooled pair count
 * On failure *out is NULL.  Every return path releases what the call took; all device memory is stream-ordered on `stream`. */
/* From decoded frames on the device. */
int stitch_dev_calibrate_u8(const stitch_frame_u8 *frames, int n_sets, int n, const stitch_calibrate_opts *opts, void *stream,
                            stitch_calibration **out);
/* From features in map order: frame_wh = n (width, height) pairs of the decoded frames, feats = n_sets * n sets of device
 * pointers, capture-major, left unchanged (the steps work on the call's own pooled copies of x and y). */
int stitch_dev_calibrate_from_features_u8(const int32_t *frame_wh, const stitch_feature_set *feats, int n_sets, int n,
                                          const stitch_calibrate_opts *opts, void *stream, stitch_calibration **out);
/* From frames in HOST memory: uploads them and runs on the null stream. */
int stitch_calibrate_u8(const stitch_frame_u8 *frames, int n_sets, int n, const stitch_calibrate_opts *opts,
                        stitch_calibration **out);

/* ---- the result: HOST ONLY ---------------------------------------------------------------------------------------------
 * Every output pointer is optional.  width / height: the mosaic after the last step (the start camera's frame without steps). */
int stitch_calibration_info(const stitch_calibration *cal, int *n_sets, int *n, int *start, int *n_steps, int *width, int *height);
/* Step k as stitch_rig_create takes it: src, dst, p_fwd, p_bwd, geom and both RANSAC info rows; seam is zeroed. */
int stitch_calibration_step_at(const stitch_calibration *cal, int k, stitch_panorama_step *step);
/* per_capture: n_sets matrices of n x n int32, capture-major, row-major count_k[i][j] = pairs of getImgPair(camera i, camera j)
 * in capture k; pooled: their n x n sum. */
int stitch_calibration_counts(const stitch_calibration *cal, int32_t *per_capture, int32_t *pooled);
/* Diagnostic: which capture disagrees with the calibration.  pairs[c] = the pairs capture c put into step k's chosen pooled
 * list; inliers[c] = the entries of the forward map's winning inlier list inside capture c's segment.  n_sets int32 each. */
int stitch_calibration_step_support(const stitch_calibration *cal, int k, int32_t *pairs, int32_t *inliers);
/* stitch_rig_create (exposure NULL) or stitch_rig_create_exposure with the calibration's frame sizes, start and steps. */
int stitch_rig_from_calibration(const stitch_calibration *cal, const stitch_rig_opts *opts, const stitch_exposure_opts *exposure,
                                stitch_rig **out);
void stitch_calibration_destroy(stitch_calibration *cal);

#ifdef __cplusplus
}
#endif
#endif /* STITCH_CALIBRATE_H */
