/* stitch_rig_formats.h -- a rig's frames and mosaics in the layouts cameras, decoders, encoders and displays use: packed RGB with a
 * row pitch, and NV12 (libstitch_hip.so, same ABI version).
 *
 * An addition to include/stitch_rig.h and the headers behind it, kept in a header of its own so that their tables of entry points
 * stay as they are.  A rig left at (STITCH_PIX_PLANAR, STITCH_PIX_PLANAR) -- the state of every rig that never called
 * stitch_rig_set_formats -- takes none of the paths below, allocates none of their buffers and writes every byte it wrote before.
 * THIS HEADER IS THE SPECIFICATION of the formats; tests/pixfmt_ref.py restates it in numpy.  Integers only: every result is exact.
 *
 * THE LAYOUTS of an image of w x h pixels:
 *   STITCH_PIX_PLANAR  (3, h, w) bytes, dense, channel-major: the layout of every other call.  Only `data` is read; pitches ignored.
 *   STITCH_PIX_RGB24   bytes R G B per pixel        STITCH_PIX_BGR24   bytes B G R per pixel        (bpp = 3)
 *   STITCH_PIX_RGBX32  bytes R G B X per pixel      STITCH_PIX_BGRX32  bytes B G R X per pixel      (bpp = 4)
 *   STITCH_PIX_NV12    plane 0 (`data`):  Y, w bytes per row, h rows;
 *                      plane 1 (`data2`): Cb Cr interleaved, ceil(w/2) pairs per row, ceil(h/2) rows.
 *   pitch   bytes from one row of plane 0 to the next: >= bpp * w (packed), >= w (NV12).
 *   pitch2  bytes from one row of the CbCr plane to the next: >= 2 * ceil(w/2).  NV12 only, as is data2.
 *   X is ignored on input and written as 255 on output.  Row padding (the bytes of a row behind its pixels) is never read on input
 *   and never written on output.  No alignment is required of a pointer or a pitch: aligned rows move in wider accesses, the bytes
 *   are the same.
 *
 * NV12, one of three matrices (`matrix` 0, 1, 2), in 16.16 fixed point.  `>>` is an arithmetic shift (floor division by 65536),
 * clip is to 0 .. 255, and every intermediate fits an int32.
 *   decode:  c = Y - yoff, d = Cb - 128, e = Cr - 128
 *            R = clip((ky*c + krv*e + 32768) >> 16)
 *            G = clip((ky*c - kgu*d - kgv*e + 32768) >> 16)
 *            B = clip((ky*c + kbu*d + 32768) >> 16)
 *     matrix              yoff  ky     krv     kgu    kgv    kbu
 *     0 BT.601 limited    16    76309  104597  25675  53279  132201
 *     1 BT.709 limited    16    76309  117489  13975  34925  138438
 *     2 BT.601 full       0     65536  91881   22553  46802  116130
 *   encode, per pixel:
 *            Y  = clip((( yr*R + yg*G + yb*B + 32768) >> 16) + yoff)
 *            Cb = clip(((-ur*R - ug*G + ub*B + 32768) >> 16) + 128)
 *            Cr = clip((( vr*R - vg*G - vb*B + 32768) >> 16) + 128)
 *     matrix  yr     yg     yb    ur     ug     ub     vr     vg     vb
 *     0       16829  33039  6416  9714   19070  28784  28784  24103  4681
 *     1       11966  40254  4064  6596   22188  28784  28784  26145  2639
 *     2       19595  38470  7471  11058  21710  32768  32768  27439  5329
 *     (each chroma row sums to zero: a grey pixel gives Cb = Cr = 128)
 *   chroma in:   pixel (x, y) takes the pair at (x / 2, y / 2): replication, no interpolation.
 *   chroma out:  the pair at (i, j) is (s + 2) >> 2 per component, s the sum of the per-pixel 8-bit values (after their clip) at
 *                (2i, 2j), (2i+1, 2j), (2i, 2j+1), (2i+1, 2j+1); a coordinate beyond the last column or row is clamped to it.
 *   A cropped output (include/stitch_rig_crop.h) is an image of its own: its 2 x 2 grid starts at the rectangle's corner.
 */
#ifndef STITCH_RIG_FORMATS_H
#define STITCH_RIG_FORMATS_H
#include <stddef.h>
#include <stdint.h>

#include "stitch.h"
#include "stitch_rig.h"
#include "stitch_rig_seams.h"

#ifdef __cplusplus
extern "C" {
#endif

#define STITCH_PIX_PLANAR 0
#define STITCH_PIX_RGB24 1
#define STITCH_PIX_BGR24 2
#define STITCH_PIX_RGBX32 3
#define STITCH_PIX_BGRX32 4
#define STITCH_PIX_NV12 5

typedef struct stitch_image {
    uint8_t *data;  /* plane 0 */
    uint8_t *data2; /* the CbCr plane of NV12; ignored otherwise */
    int32_t width, height, pitch, pitch2;
} stitch_image;

/* ---- sizes: HOST ONLY --------------------------------------------------------------------------------------------------------
 * The extent in bytes of each plane, from its first byte to the last byte of its last row's pixels (the last row has no padding
 * behind it): (h - 1) * pitch + bpp * w, and for NV12 (h - 1) * pitch + w and (ceil(h/2) - 1) * pitch2 + 2 * ceil(w/2).  *bytes2 is 0
 * for every format but NV12.  STITCH_PIX_PLANAR: 3 * w * h, pitches ignored.  STITCH_ERR_ARG for a format outside 0 .. 5, w < 1,
 * h < 1 or a pitch below the minimum above.  Either output may be null. */
int stitch_image_bytes(int fmt, int w, int h, int pitch, int pitch2, size_t *bytes, size_t *bytes2);

/* ---- the conversions on their own ----------------------------------------------------------------------------------------------
 * `count` (1 .. 65535) images of one size (src[0] / dst[0] state it; every other entry must agree; 3 * w * h <= 2^31 - 1, else
 * STITCH_ERR_ARG) in one launch.  The planar side
 * is dense (3, h, w).  fmt = STITCH_PIX_PLANAR is refused; matrix (0 .. 2) is read for NV12 only but always checked.  Both WAIT for
 * `stream`: their table of images goes up from a host copy.  Argument errors are reported before a device is needed. */
int stitch_dev_unpack_many_u8(int fmt, int matrix, const stitch_image *src, uint8_t *const *d_planar, int count, void *stream);
int stitch_dev_pack_many_u8(int fmt, int matrix, const uint8_t *const *d_planar, const stitch_image *dst, int count, void *stream);

/* ---- a rig with formats: HOST ONLY ---------------------------------------------------------------------------------------------
 * stitch_rig_set_formats: the layout of the frames (in_fmt) and of the outputs (out_fmt) of stitch_dev_rig_stitch_fmt_u8, and the
 * NV12 matrix of both sides.  STITCH_ERR_ARG, leaving the rig as it was, for a null handle, a format outside 0 .. 5 or a matrix
 * outside 0 .. 2.  While either format is not planar, stitch_dev_rig_stitch_u8 and stitch_dev_rig_stitch_exposure_u8 return
 * STITCH_ERR_ARG (before a device is needed).  stitch_rig_clear_formats returns to (PLANAR, PLANAR), matrix 0;
 * stitch_rig_formats reads the state back (any output may be null). */
int stitch_rig_set_formats(stitch_rig *rig, int in_fmt, int out_fmt, int matrix);
int stitch_rig_formats(const stitch_rig *rig, int *in_fmt, int *out_fmt, int *matrix);
int stitch_rig_clear_formats(stitch_rig *rig);

/* ---- the replay ------------------------------------------------------------------------------------------------------------------
 * The contract of stitch_dev_rig_stitch_u8 (stitch_rig.h), with frames[set * n_frames + f] in in_fmt and out[set] in out_fmt: per
 * set exactly pack(out_fmt) of what the planar rig writes on unpack(in_fmt) of the same frames; statuses, seams and statistics are
 * the planar rig's.  out[set] has the size of stitch_rig_output_size (the crop's, or the canvas).  A planar side is dense and its
 * pitches are ignored.  `stats` (12 floats per set and step, stitch_rig_exposure.h) may be null and is allowed only on a rig made
 * with an exposure mode.  Overlap between outputs and frames is judged by stitch_image_bytes, plane by plane.
 *   in:   the projection stages its source straight from the packed or NV12 frames where a frame size takes the tiled projection
 *         (a width that is a multiple of 4, a source box within the LDS budget) and every plane address and pitch of that frame
 *         index in the call is a multiple of 4.  Any other frame index takes the fallback, which is a form, not an error: one
 *         conversion launch per sequence into planar scratch the rig owns (max_sets frames, from the first such call on, freed by
 *         stitch_rig_destroy), then the planar projection.  The bytes are the same, pixels whose source lies outside the frame
 *         included: they are 0 in either form.
 *   out:  the last step writes planar buffers the rig owns (max_sets, likewise; none where the crop below makes them unread); ONE launch per sequence then writes the caller's
 *         images: it applies the finish pass's per-pixel function from the set's LUT on the way (the finished planar image is never
 *         stored), and with crop mode 1 reads the rectangle straight out of the full canvases (no crop copy).
 * Works on a rig at (PLANAR, PLANAR) too, as the planar call with images for arguments. */
int stitch_dev_rig_stitch_fmt_u8(stitch_rig *rig, const stitch_image *frames, int n_sets, const stitch_image *out, int32_t *set_status,
                                 stitch_seam *seams, float *stats, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* STITCH_RIG_FORMATS_H */
