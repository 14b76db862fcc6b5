/* stitch_rig_formats_yuv.h -- a rig's frames and mosaics in the 4:2:2 layouts of cameras and capture cards (YUYV, UYVY, NV16) and
 * in NV21 (libstitch_hip.so, same ABI version).
 *
 * An addition to include/stitch_rig_formats.h, kept in a header of its own so that that header's table of entry points and of
 * constants stays as it is.  Every call of stitch_rig_formats.h takes the four codes below with the contract it states there;
 * `stitch_image` is used as it is (no new field, same size and offsets).  A rig that never sets a format takes none of the paths
 * below, allocates and launches nothing more and writes every byte it wrote before.
 * THIS HEADER IS THE SPECIFICATION of the four formats; tests/pixfmt_yuv_ref.py restates it in numpy.  Integers only: every result is
 * exact.
 *
 * THE CODES are 16 and up.  Every value outside 0 .. 5 and 16 .. 19 (6 .. 15 and 20 and up among them) stays STITCH_ERR_ARG in every
 * call.
 *
 * THE LAYOUTS of an image of w x h pixels:
 *   STITCH_PIX_YUYV  one plane (`data`); a row is ceil(w/2) groups of 4 bytes  Y0 Cb Y1 Cr ; group i holds pixels 2i and 2i+1.
 *   STITCH_PIX_UYVY  the same groups as                                        Cb Y0 Cr Y1.
 *   STITCH_PIX_NV21  STITCH_PIX_NV12 with every chroma pair stored Cr Cb.
 *   STITCH_PIX_NV16  plane 0 (`data`):  Y, w bytes per row, h rows;
 *                    plane 1 (`data2`): Cb Cr interleaved, ceil(w/2) pairs per row, h rows.
 *   pitch   YUYV, UYVY: >= 4 * ceil(w/2).   NV21, NV16: >= w.
 *   pitch2  NV21, NV16: >= 2 * ceil(w/2); ignored for YUYV and UYVY, as is data2.
 *   stitch_image_bytes:  YUYV, UYVY: (h - 1) * pitch + 4 * ceil(w/2), and 0 for the second plane.
 *                        NV21: as NV12.   NV16: (h - 1) * pitch + w and (h - 1) * pitch2 + 2 * ceil(w/2).
 *   Row padding (the bytes of a row behind its pixel bytes) is never read on input and never written on output.  No alignment is
 *   required of a pointer or a pitch: aligned rows move in wider accesses, the bytes are the same.
 *   Odd width, YUYV and UYVY: the Y1 byte of a row's last group is a pixel byte, not padding.  It is ignored on input; on output it
 *   is written with the luma of pixel w - 1, the clamped coordinate (NV12's rule for its clamped block).
 *
 * COLOUR.  The three matrices (`matrix` 0, 1, 2), the decode, the per-pixel encode and the clip are those of stitch_rig_formats.h,
 * unchanged; `matrix` is read for the four formats as it is for NV12.
 *   chroma in:   4:2:2 (YUYV, UYVY, NV16): pixel (x, y) takes the pair at (x / 2, y): replication, no interpolation.  NV21: as NV12.
 *   chroma out:  4:2:2: the pair at (i, y) is (s + 1) >> 1 per component, s the sum of the per-pixel 8-bit values (after their clip)
 *                at (2i, y) and (min(2i+1, w-1), y).  NV21: NV12's 2 x 2 rule.
 *   A cropped output (include/stitch_rig_crop.h) is an image of its own: its chroma grid starts at the rectangle's corner.
 *
 * THE REPLAY (stitch_dev_rig_stitch_fmt_u8).  Any mix of these formats and those of stitch_rig_formats.h on the two sides.  The
 * projection stages a frame index straight from its YUYV, UYVY, NV16 or NV21 frames under the rule stated there: a frame size that
 * takes the tiled projection, a width that is a multiple of 4 (which keeps every 4:2:2 group whole) and every plane address and
 * pitch of that frame index in the call a multiple of 4.  Any other frame index takes the fallback stated there.
 */
#ifndef STITCH_RIG_FORMATS_YUV_H
#define STITCH_RIG_FORMATS_YUV_H
#include "stitch_rig_formats.h"

#ifdef __cplusplus
extern "C" {
#endif

#define STITCH_PIX_YUYV 16
#define STITCH_PIX_UYVY 17
#define STITCH_PIX_NV21 18
#define STITCH_PIX_NV16 19

#define STITCH_RIG_INPUT_NONE 0      /* no such replay yet, a planar in_fmt, or a frame that no step and no start uses */
#define STITCH_RIG_INPUT_FUSED 1     /* the tiled projection staged the packed source itself */
#define STITCH_RIG_INPUT_CONVERTED 2 /* one conversion launch into planar scratch, then the planar projection */

/* ---- the form a frame index took: HOST ONLY ----------------------------------------------------------------------------------
 * *form: how the last completed stitch_dev_rig_stitch_fmt_u8 of this rig read frame index `frame`, one of the three values above,
 * for every in_fmt (those of stitch_rig_formats.h too).  A replay has completed when all its work has run: one that returns a
 * set's status (STITCH_ERR_EMPTY_MIDROW, STITCH_ERR_ZERO_OVERLAP) has; one that fails on an argument or a HIP call has not, and
 * leaves the previous answer.  The planar replay calls do not change it.  STITCH_ERR_ARG for a null argument or a frame outside
 * 0 .. n_frames - 1. */
int stitch_rig_input_form(const stitch_rig *rig, int frame, int *form);

#ifdef __cplusplus
}
#endif
#endif /* STITCH_RIG_FORMATS_YUV_H */
