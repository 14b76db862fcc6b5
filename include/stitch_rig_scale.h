/* stitch_rig_scale.h -- a rig's output at the size its consumer wants: an exact area-average downscale inside the one pack launch
 * (libstitch_hip.so, same ABI version).
 *
 * An addition to include/stitch_rig_crop.h, include/stitch_rig_formats.h and include/stitch_rig_formats_yuv.h, kept in a header of
 * its own so that their tables of entry points stay as they are.  A rig's canvases are 1081 x 527, 4421 x 2315 and the like; an
 * encoder, a display or a preview window wants 3840 x 2160, 1920 x 1080 or 960 x 540.  A rig with an output scale writes that size
 * per set, in any layout, from the launch that packs its output anyway.  A rig that never sets a scale allocates nothing more,
 * launches nothing more and writes every byte it wrote before; no call of the other headers changes.
 *
 * THE SPECIFICATION.  The source is an RGB image P of w x h bytes per channel: what the rig would write as planar output without a
 * scale -- after the crop, after the finish pass, in either crop mode.  The target is ow x oh.
 *   Sizes:    1 <= ow <= w <= 8 * ow and 1 <= oh <= h <= 8 * oh.  A delivery scaler: it never enlarges and makes no thumbnails.
 *   Weights:  per axis.  Source column x covers [x * ow, (x + 1) * ow), output column X covers [X * w, (X + 1) * w), and
 *             wx(X, x) = max(0, min((X + 1) * w, (x + 1) * ow) - max(X * w, x * ow)); wy(Y, y) likewise with h, oh.
 *             So sum_x wx(X, x) = w and sum_y wy(Y, y) = h.
 *   Value:    per channel, S = sum_y wy(Y, y) * sum_x wx(X, x) * P[y][x], D = w * h, and
 *             out[Y][X] = (2 * S + D) div (2 * D): the area average, rounded half up, ONE rounding.
 *             S <= 255 * D with D <= 2^31 - 1, so S takes 64 bits in general.  Dividing w, ow (and h, oh) by their greatest common
 *             divisor first gives the same rational, and an implementation may.
 *   It follows that ow == w && oh == h is the identity, that a constant image stays constant, that w == 2 * ow && h == 2 * oh gives
 *   (a + b + c + d + 2) >> 2, and that the sums are separable without a rounding between them: horizontal sums of at most 255 * w,
 *   then the vertical ones.
 *   Output:   the scaled image is an image of its own.  pack(out_fmt) applies to it exactly as stitch_rig_formats.h and
 *             stitch_rig_formats_yuv.h state; its 2 x 2 or 2 x 1 chroma grid starts at its own corner.  STITCH_PIX_PLANAR is the
 *             dense (3, oh, ow) image.
 * Out of scope: enlargement, factors above 8, filters other than the box, float frames, the whole-panorama calls, the C++ adaptor
 * and a second (preview) output per replay.
 */
#ifndef STITCH_RIG_SCALE_H
#define STITCH_RIG_SCALE_H
#include <stddef.h>
#include <stdint.h>

#include "stitch.h"
#include "stitch_rig.h"
#include "stitch_rig_crop.h"
#include "stitch_rig_formats.h"
#include "stitch_rig_formats_yuv.h"

#ifdef __cplusplus
extern "C" {
#endif

#define STITCH_SCALE_MAX_FACTOR 8 /* w <= 8 * ow, h <= 8 * oh */

/* ---- the stand-alone call --------------------------------------------------------------------------------------------------
 * stitch_dev_scale_pack_many_u8: `count` (1 .. 65535) dense planar (3, src_h, src_w) device images; of each, `rect` (NULL: the
 * whole image; else a rectangle inside it) is scaled to dst[0].width x dst[0].height by the rule above and written to dst[i] in
 * `fmt` -- every code stitch_image_bytes takes, STITCH_PIX_PLANAR included (dst[i].data is then the dense (3, oh, ow) image and the
 * pitches are ignored).  matrix: 0 .. 2, read by the Y Cb Cr layouts.  There is no finish pass.  One launch; it WAITS for `stream`,
 * as stitch_dev_pack_many_u8 does.  Every argument error is reported before a device is needed: a null table or entry, a bad
 * count, format or matrix, src_w * src_h above (2^31 - 1) / 3, a rectangle that is empty or not inside the image, a target outside
 * the rule above, dst entries of differing sizes, a pitch below a row. */
int stitch_dev_scale_pack_many_u8(int fmt, int matrix, const uint8_t *const *d_planar, int src_w, int src_h, const stitch_rect *rect,
                                  const stitch_image *dst, int count, void *stream);

/* ---- a rig with an output scale: HOST ONLY ---------------------------------------------------------------------------------
 * stitch_rig_set_output_scale: from now on every replay -- stitch_dev_rig_stitch_u8, stitch_dev_rig_stitch_exposure_u8 and
 * stitch_dev_rig_stitch_fmt_u8 -- writes ow x oh per set, and stitch_rig_output_size reports (ow, oh).  The rule is checked against
 * the rig's source size at the time of the call (the crop's rectangle, else the canvas); STITCH_ERR_ARG, leaving the rig as it was,
 * for a null handle or a size outside the rule.  A replay checks again, before a device is needed: a crop set or cleared afterwards
 * may have left a scale the rule no longer admits, and that replay returns STITCH_ERR_ARG.
 *   The contract, per set: the output is pack(out_fmt)(scale(what the same rig writes as planar output with the scale cleared)),
 *   byte for byte; statuses, seams, statistics, residuals and paths are exactly the unscaled rig's.  stitch_rig_info keeps
 *   reporting the canvas, stitch_rig_crop the rectangle.
 * The histogram and LUT of the finish pass are computed where they are without a scale (the full canvas in crop mode 1, the
 * rectangle in mode 2); the finish function is applied to the source pixels inside the scaled pack launch, which replaces the pack
 * launch of a formatted output and is the one additional launch per sequence of a planar one.  The planar calls' last step writes
 * rig-owned buffers (max_sets of them, allocated by the first scaled replay and freed by stitch_rig_destroy).
 * stitch_rig_clear_output_scale returns to the source size.  stitch_rig_output_scale reads the scale back: 0, 0 when none is set
 * (either output may be null). */
int stitch_rig_set_output_scale(stitch_rig *rig, int ow, int oh);
int stitch_rig_clear_output_scale(stitch_rig *rig);
int stitch_rig_output_scale(const stitch_rig *rig, int *ow, int *oh);

#ifdef __cplusplus
}
#endif
#endif /* STITCH_RIG_SCALE_H */
