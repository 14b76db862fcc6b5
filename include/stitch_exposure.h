/* stitch_exposure.h -- exposure-matched panoramas: the colour transfer inside the chain (libstitch_hip.so, same ABI version).
 *
 * An addition to include/stitch.h, include/stitch_panorama.h and include/stitch_rig.h, kept in a header of its own so that
 * their tables of entry points stay as they are.  The reference's matching() was meant to match each incoming frame's colours
 * to what is already stitched: ImageProcess.cpp:180-182 holds `transfer tran(imgs[dst].projectedSrc, imgs[src].projectedSrc,
 * imgs[dst].projectedSrc)` and the variant with `result` as the template, both commented out.  The entry points below run the
 * chain of stitch_panorama.h with one of the two switched on.
 *
 * What makes that affordable is the statistics kernel.  transfer.cpp:128-164 accumulates mean and standard deviation in FLOAT,
 * in raster order; stitch_dev_transfer_u8 reproduces that with one dependent add per sample.  The forms 1 and 2 below give the
 * same bits from a parallel scan (csrc/k_exposure.inc).
 */
#ifndef STITCH_EXPOSURE_H
#define STITCH_EXPOSURE_H
#include <stddef.h>
#include <stdint.h>

#include "stitch.h"
#include "stitch_panorama.h"

#ifdef __cplusplus
extern "C" {
#endif

/* How the float running sums are formed.  Every form gives the same bits on every input. */
#define STITCH_STATS_SERIAL 0 /* one wavefront per plane walks it sample by sample (stitch_dev_transfer_u8's kernel)      */
#define STITCH_STATS_SCAN 1   /* one workgroup per plane, tile by tile: scan, restart behind the first violation          */
#define STITCH_STATS_SPANS 2  /* spans reduced side by side under a guessed state, then one walk over the span table      */
#define STITCH_STATS_DIAG 4   /* counters per plane: samples added by a plain float add, spans taken in O(1), spans redone,
                                 tiles finished serially (both passes together) */

/* mean = fl(sum x) / count and sd = sqrtf(fl(sum fl((x - mean) * (x - mean))) / count) of 1 .. 6 float planes, each sum a
 * float accumulated in index order from 0 (transfer.cpp:128-164).  d_planes, lengths (>= 1 each) and counts are HOST arrays
 * of n_planes entries, d_planes holding device pointers; d_mean and d_sd receive n_planes floats on the device; d_diag
 * (optional) n_planes * STITCH_STATS_DIAG uint32, overwritten.  Enqueued on `stream`; scratch is stream-ordered on it. */
int stitch_dev_running_stats_f32(const float *const *d_planes, const size_t *lengths, const float *counts, int n_planes, int form,
                                 float *d_mean, float *d_sd, uint32_t *d_diag, void *stream);

/* stitch_dev_transfer_u8 with the form of its statistics and keep_black: with keep_black != 0 a source pixel that is (0,0,0)
 * stays (0,0,0) in the output; the statistics still run over all pixels, as the reference's do.  d_out may be d_src.  d_diag
 * (optional): 6 * STITCH_STATS_DIAG uint32, the planes in the order l, alpha, beta of the source, then of the template. */
int stitch_dev_transfer_form_u8(const uint8_t *d_src, int sw, int sh, const uint8_t *d_tem, int tw, int th, uint8_t *d_out,
                                float *d_stats12, int stats_form, int keep_black, uint32_t *d_diag, void *stream);

typedef struct stitch_exposure_opts {
    int32_t mode;       /* 0: no transfer, the chain of stitch_panorama.h; 1: the template is the stored projected frame of
                           `src` (ImageProcess.cpp:180), which an earlier step may have recoloured; 2: the template is the
                           running mosaic before the step (the variant with `result`)                                      */
    int32_t stats_form; /* STITCH_STATS_SERIAL / _SCAN / _SPANS                                                            */
    int32_t keep_black; /* 0 is the reference's literal behaviour: it paints the black corners that the cylinder projection
                           leaves, and the warp then treats them as image.  1 keeps them black, and is the default of
                           stitch_exposure_opts_default for that reason.                                                   */
} stitch_exposure_opts;
/* mode 1, stats_form STITCH_STATS_SPANS, keep_black 1 */
void stitch_exposure_opts_default(stitch_exposure_opts *o);

/* The three whole-chain calls of stitch_panorama.h with one transfer in every step: right before the stitch step, in place on
 * the stored projected frame of `dst`, as the reference's `transfer tran(X, T, X)` overwrites imgs[dst].projectedSrc.
 * Features, maps, the stitch order and the canvases do not depend on the mode: SIFT ran before the transfer, as in readFile.
 * A seam-scan failure that the recoloured frame causes is reported as any other.  exposure NULL: mode 0.  A mode or a
 * stats_form outside 0 .. 2 is STITCH_ERR_ARG before anything is enqueued.  With opts->keep_steps the handle also keeps each
 * step's recoloured frame. */
int stitch_dev_panorama_exposure_from_features_u8(const stitch_frame_u8 *frames, const stitch_feature_set *feats, int n,
                                                  const stitch_panorama_opts *opts, const stitch_exposure_opts *exposure,
                                                  void *stream, stitch_panorama **out);
int stitch_dev_panorama_exposure_u8(const stitch_frame_u8 *frames, int n, const stitch_panorama_opts *opts,
                                    const stitch_exposure_opts *exposure, void *stream, stitch_panorama **out);
int stitch_panorama_exposure_u8(const stitch_frame_u8 *frames, int n, const stitch_panorama_opts *opts,
                                const stitch_exposure_opts *exposure, stitch_panorama **out);
/* The twelve statistics of step k's transfer: mean and sd of the frame's l, alpha, beta, then of the template's.
 * STITCH_ERR_ARG for a panorama made with mode 0. */
int stitch_panorama_exposure_stats(const stitch_panorama *pano, int k, float stats[12]);
/* Copies step k's recoloured frame (3 x height x width of frame dst; kept with keep_steps only) into dst, as
 * stitch_panorama_copy copies a mosaic. */
int stitch_panorama_exposure_frame_copy(const stitch_panorama *pano, int k, void *dst, size_t capacity, int dst_is_device,
                                        void *stream);

#ifdef __cplusplus
}
#endif
#endif /* STITCH_EXPOSURE_H */
