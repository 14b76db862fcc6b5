/* stitch_rig_crop.h -- the crop of a rig's output: the largest rectangle the cameras fully cover (libstitch_hip.so, same ABI version).
 *
 * An addition to include/stitch_rig.h and include/stitch_rig_seams.h, kept in a header of its own so that their tables of entry
 * points stay as they are.  A rig's output is the bounding canvas of its warped frames and carries the black wedges of the
 * projection and of every map.  A rig can instead write ONE rectangle of that canvas per set: any rectangle the caller states,
 * or the largest axis-aligned rectangle inside the output's coverage (stitch_rig_seams.h), found on the device.  A rig without
 * a crop writes every byte it wrote before; no call of the other headers changes.
 *
 * THE RULE of the search, on a mask of w x h: among the rectangles (x0, y0, w, h) whose pixels are all covered, the one with
 *   1. the largest area w * h;  2. among those the smallest y0;  3. then the smallest x0;  4. then the largest w.
 * A rectangle of maximal area cannot be extended, so the rule has one answer whatever way the search takes.  A mask without a
 * covered pixel is not an error: the result is {0, 0, 0, 0} with STITCH_OK.  Sizes: w >= 1, h >= 1, w * h <= 2^31 - 1.
 */
#ifndef STITCH_RIG_CROP_H
#define STITCH_RIG_CROP_H
#include <stddef.h>
#include <stdint.h>

#include "stitch.h"
#include "stitch_rig.h"
#include "stitch_rig_seams.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct stitch_rect {
    int32_t x0, y0, w, h;
} stitch_rect;

#define STITCH_CROP_AFTER_FINISH 1  /* the rectangle of the finished full canvas */
#define STITCH_CROP_BEFORE_FINISH 2 /* the finish pass runs on the rectangle alone */

/* ---- the search ------------------------------------------------------------------------------------------------------------
 * stitch_dev_largest_rect_u8: on a dense mask (device, w * h bytes, any non-zero byte = covered).
 * stitch_dev_rig_inscribed_rect: on step `step`'s A | B coverage plane, read as bits (-1: the last step = the output's validity
 * mask; a rig with zero steps: C_proj(start)).  Computes the coverage planes first if the rig has none yet, exactly as
 * stitch_dev_rig_coverage_u8 does; changes nothing else in the rig.
 * Both take their scratch from the stream-ordered allocator per call and WAIT for `stream`: `out` is a HOST record.  Argument
 * errors (a null pointer, a bad size, a step outside -1 .. n_steps-1) are reported before a device is needed. */
int stitch_dev_largest_rect_u8(const uint8_t *d_mask, int w, int h, stitch_rect *out, void *stream);
int stitch_dev_rig_inscribed_rect(stitch_rig *rig, int step, stitch_rect *out, void *stream);

/* ---- a rig with a crop: HOST ONLY ------------------------------------------------------------------------------------------
 * stitch_rig_set_crop: mode 1 (STITCH_CROP_AFTER_FINISH) or 2 (STITCH_CROP_BEFORE_FINISH).  STITCH_ERR_ARG, leaving the rig as it
 * was, for a null argument, a mode outside 1 .. 2, w < 1, h < 1, or a rectangle that is not inside the output canvas of
 * stitch_rig_info.  From then on every replay -- stitch_dev_rig_stitch_u8 and stitch_dev_rig_stitch_exposure_u8 -- writes
 * 3 * rect.w * rect.h bytes per set (planar, dense, channel-major) to d_out[i]; statuses, seams and statistics are exactly what
 * they are without the crop, and the rest of the contract of stitch_rig.h stays.
 *   mode 1: byte for byte the slice [:, y0 : y0 + h, x0 : x0 + w] of what the same rig writes without a crop.
 *   mode 2: the slice of the unfinished mosaic (what the rig writes with finish = 0) is taken first, and the finish pass runs
 *           on it as an image of rect.w x rect.h: byte for byte stitch_dev_finish_u8 on that slice with the rig's num, den.
 *           The black border no longer enters the equalisation histogram.
 *   finish = 0: both modes give the same bytes.
 * The last step of a cropped rig writes a full-canvas buffer per set that the rig owns (max_sets of them, allocated by the
 * first cropped replay and freed by stitch_rig_destroy); a rig without a crop allocates none.
 * stitch_rig_clear_crop returns to the whole canvas.  stitch_rig_crop reads the crop back (mode 0: no crop, rect = the whole
 * canvas; either output may be null).  stitch_rig_output_size: what a replay writes per set -- the rectangle's size, or the
 * canvas.  stitch_rig_info keeps reporting the uncropped canvas. */
int stitch_rig_set_crop(stitch_rig *rig, const stitch_rect *rect, int mode);
int stitch_rig_clear_crop(stitch_rig *rig);
int stitch_rig_crop(const stitch_rig *rig, stitch_rect *rect_out, int *mode_out);
int stitch_rig_output_size(const stitch_rig *rig, int *width, int *height);

#ifdef __cplusplus
}
#endif
#endif /* STITCH_RIG_CROP_H */
