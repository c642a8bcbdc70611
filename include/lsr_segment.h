/*
 * lsr_segment.h -- C ABI of the open-vocabulary segmentation step (relevancy maps -> masks, level
 * scores and IoU counts), part of liblsr.so.  It consumes what lsr_query_relevancy produces.
 *
 * Reference behaviour replaced:
 *   activate_stream      eval/eval.py:143-315 (the per level, per phrase loop: smooth, blend, stretch,
 *                        threshold, clean, IoU, level score)
 *   smooth_cuda          eval/eval_utils.py:95-100 (the 7 x 7 majority filter)
 *
 * For every map v = rel[m] of [H, W], float32 throughout:
 *   a        = AvgPool2d(scale, stride 1, padding scale / 2, count_include_pad = False)(v)
 *   b        = 0.5 * (a + v)                                         -> blended[m]
 *   o        = clip((b - min b) / (max (b - min b) + 1e-9f) * 2 + (-1), 0, 1)      min / max propagate NaN
 *   mask_raw = o > thresh                                            -> mask_raw[m], bytes 0 / 1
 *   mask     = 2 * (ones of mask_raw in the 7 x 7 window) > (in-image pixels of that window)
 *              which is AvgPool2d(7, 1, 3, count_include_pad = False)(mask_raw) > 0.5   -> mask[m]
 *   score    = max b                                   (strategy LSR_SEGMENT_POINT)
 *            = mean of b over mask_raw, 0 if empty     (strategy LSR_SEGMENT_MEAN; summed in double)
 *   inter    = sum(gt != 0 & mask), union = sum(gt != 0 | mask)      with gt = gt[m % gt_count]
 * Window sums are taken in a fixed order that does not depend on the pixel's position; sums over a map
 * are added in a fixed order or are integers: no float atomics, two calls give the same bits.
 *
 * Supported: scale odd in 1 ... 63, 1 <= H, W <= 16384, n_maps >= 0 (0: nothing is launched and no
 * pointer is read), strategy 0 or 1, gt_count >= 1 when gt is given.  gt, inter_count and union_count
 * are given together or all NULL.  Anything else, and any other NULL pointer, is LSR_EINVAL, decided
 * before the device is touched.
 *
 * Conventions: device pointers, contiguous arrays; blended must not overlap rel; the library
 * allocates nothing: the caller provides lsr_segment_workspace_bytes(n_maps, H, W) bytes, 16-byte
 * aligned; everything runs on `stream` with no host synchronisation.  Return 0 or an LSR_E* code
 * (lsr.h); lsr_last_error().
 */
#ifndef LSR_SEGMENT_H_
#define LSR_SEGMENT_H_
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define LSR_SEGMENT_POINT 0
#define LSR_SEGMENT_MEAN 1
#define LSR_SEGMENT_MAX_SCALE 63
#define LSR_SEGMENT_MAX_SIDE 16384

/* Bytes of workspace for any scale and strategy; -1 (and lsr_last_error) for invalid sizes. */
int64_t lsr_segment_workspace_bytes(int32_t n_maps, int32_t H, int32_t W);

/* rel, blended [n_maps, H, W] float32; gt [gt_count, H, W], mask_raw, mask [n_maps, H, W] uint8;
 * score [n_maps] float32; inter_count, union_count [n_maps] int64. */
int lsr_segment(int32_t n_maps, int32_t H, int32_t W, const float *rel, int32_t scale, float thresh,
                int32_t strategy, const uint8_t *gt, int32_t gt_count, float *blended, uint8_t *mask_raw,
                uint8_t *mask, float *score, int64_t *inter_count, int64_t *union_count, void *workspace,
                void *stream);

#ifdef __cplusplus
}
#endif
#endif /* LSR_SEGMENT_H_ */
