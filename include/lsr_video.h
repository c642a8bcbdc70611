/*
 * lsr_video.h -- C ABI of the time-sensitive query's hot path (the wide video-feature decode and its
 * cosine similarity with the phrase embeddings), part of liblsr.so.
 *
 * Reference behaviour replaced:
 *   cal_avg_video_feature               eval/eval.py:317-327, called at :652-653: the video Autoencoder's
 *                                       decode (6 -> 32 -> ... -> 4096) of the pixels of one mask, sklearn's
 *                                       cosine_similarity with the phrase's E5 embedding, the mean over them
 *
 * Per row, with x0 = rows[row, 0:c_in]:
 *   x_{i+1} = W_i . (i > 0 ? relu(x_i) : x_i) + b_i          W_i [out_i, in_i] row-major (nn.Linear)
 *   y       = x_n                                             the last layer, before normalisation
 *   cosine[j, row] = (y . q_j) / sqrt(y . y)                  no epsilon: a zero y gives NaN (lsr_query.h)
 * and per segment s (a run of rows, one mask)
 *   mean[s] = mean of cosine[seg_query[s], seg_offsets[s] .. seg_offsets[s + 1])     float64, fixed order
 *
 * The decoder is lsr_query.h's lsr_decoder; the layers are a tiled GEMM on the exact f32-input MFMA with
 * the activations staged in the caller's workspace.  The d_out-wide row is never stored: the last layer
 * reduces y . y and y . q_j per column tile, and the tiles' partial sums are added in tile order.  No
 * atomics: two calls give the same bits, and a row's result does not depend on the other rows of the call.
 *
 * Supported: 1 <= n_layers <= 8, 1 <= c_in = dims[0] <= 32, every other width a multiple of 16 and
 * <= LSR_VIDEO_MAX_WIDTH, 1 <= n_q <= LSR_VIDEO_MAX_QUERIES, n_rows >= 0 (0: nothing is launched),
 * n_seg >= 0.  Anything else, any NULL pointer, and a workspace that is too small is LSR_EINVAL, decided
 * before the device is touched.
 *
 * Conventions: device pointers, float32, contiguous; the library allocates nothing: the caller provides
 * lsr_video_workspace_bytes(...) bytes, 16-byte aligned, which a call may overwrite; everything runs on
 * `stream` with no host synchronisation.  Return 0 or an LSR_E* code (lsr.h); lsr_last_error().
 */
#ifndef LSR_VIDEO_H_
#define LSR_VIDEO_H_
#include <stdint.h>

#include "lsr_query.h"
#ifdef __cplusplus
extern "C" {
#endif

#define LSR_VIDEO_API_VERSION 1
#define LSR_VIDEO_MAX_WIDTH 4096
#define LSR_VIDEO_MAX_QUERIES 16
#define LSR_VIDEO_ROW_TILE 128      /* rows of one block: every weight tile meets this many rows */
#define LSR_VIDEO_COL_TILE 128      /* output features of one block and of one partial sum */

/* Call once before the other lsr_video_* entry points with LSR_VIDEO_API_VERSION of the header the
 * caller was built against; a caller of another version is refused (LSR_EINVAL, every entry point). */
int lsr_video_require_api(int32_t caller_version);

/* Bytes of workspace of an lsr_video_cosine call of n_rows rows (the two activation images and the last
 * layer's partial sums; only n_layers and dims of the decoder are read); a negative return is an LSR_E*
 * code, negated. */
int64_t lsr_video_workspace_bytes(const lsr_decoder *dec, int64_t n_rows);

/* rows [n_rows, c_in], queries [n_q, d_out] (used as given), cosine [n_q, n_rows]. */
int lsr_video_cosine(const lsr_decoder *dec, int64_t n_rows, const float *rows, int32_t n_q, const float *queries,
                     float *cosine, void *ws, int64_t ws_bytes, void *stream);

/* cosine [n_q, n_rows]; seg_offsets [n_seg + 1] int64 (non-decreasing, within [0, n_rows]: not checked,
 * they are device memory), seg_query [n_seg] int32 in [0, n_q); mean [n_seg].  An empty segment gives NaN. */
int lsr_video_segment_mean(int64_t n_rows, int32_t n_q, const float *cosine, int32_t n_seg,
                           const int64_t *seg_offsets, const int32_t *seg_query, float *mean, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* LSR_VIDEO_H_ */
