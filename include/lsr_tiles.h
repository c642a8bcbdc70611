/*
 * lsr_tiles.h -- C ABI of the language-feature tiles: the label census, the segment maps and the
 * 224 x 224 crops that an image embedder (CLIP) consumes, part of liblsr.so.  It produces what
 * lsr_train.h's lsr_seg_loss_views and the autoencoder read: the stage before the `_s.npy` / `_f.npy`
 * files.
 *
 * Reference behaviour replaced (preprocess/generate_clip_features.py, with --precompute_seg):
 *   sam_encoder          :319-347  per level and label: np.where, the bbox [xmin, ymin, xmax - xmin, ymax - ymin]
 *   mask2segmap          :356-379  the w != 0 and h != 0 filter, get_seg_img (black-out and crop), pad_img,
 *                                  cv2.resize to 224 x 224, seg_map[mask] = i
 *   create               :156-170  v[v != -1] += lengths_cumsum[j - 1]
 *
 * One frame is L = 4 label maps `labels` [L, H, W] int32 (levels default, s, m, l) and an image [H, W, 3]
 * uint8, RGB.  Three steps:
 *
 *   lsr_tiles_census   one pass over the label maps: for every (level, label) with 1 <= label <=
 *                      LSR_TILES_MAX_LABEL the pixel count and xmin, xmax, ymin, ymax, into the workspace.
 *                      Label 0, negative labels and labels above the maximum do not count; whether any
 *                      label above the maximum was seen is kept for the plan.
 *   lsr_tiles_plan     per level, in ascending label order, the labels with pixels, w = xmax - xmin != 0 and
 *                      h = ymax - ymin != 0 are kept.  rank[level][label] (workspace) = the position in the
 *                      level's kept list plus the kept counts of the lower levels, or -1.  desc[rank] =
 *                      {level, label, x = xmin, y = ymin, w, h}: the tiles in the order default, s, m, l.
 *                      counts[0..3] = the levels' kept counts, counts[4] = 1 if a label above the maximum
 *                      was seen (else 0).  `counts` is an address the device can write: device memory, or
 *                      page-locked host memory, which makes it the frame's one host read.
 *   lsr_tiles_render   seg_maps [L, H, W] int32 = rank[level][label], -1 where the label does not count
 *                      or was filtered; tiles [n, 3, 224, 224] float32, n = the sum of the kept counts.
 *                      `lengths` [4] is a HOST array: the counts the caller read back after the plan.
 *
 * Tile arithmetic (exact, in integers).  A tile {level, label, x, y, w, h} crops rows y .. y + h - 1 and
 * columns x .. x + w - 1: the bbox without its last row and column, as the reference's
 * image[y:y+h, x:x+w] with its w and h.  The padded square has side l = max(w, h); with h > w the crop
 * sits at column offset (h - w) / 2, otherwise at row offset (w - h) / 2 (integer division).  A padded
 * pixel outside the crop is 0; inside it is the image byte where labels[level] equals the tile's label,
 * else 0.  The resize is bilinear with half-pixel centres, no antialiasing and a replicated edge (the
 * geometry of cv2.resize(., (224, 224)), INTER_LINEAR).  Per axis, for output index d, with
 * t = (2 d + 1) l - 224:  t < 0: s = 0, a = 0;  else s = t / 448, a = t % 448;  s >= l - 1: s = l - 1,
 * a = 0.  The taps are s and min(s + 1, l - 1) with weights 448 - a and a.  With S the sum over the four
 * taps of wx wy byte, the output byte is (S + 100352) / 200704 and the tile value that byte / 255.0f.
 *
 * Only integer atomics are used: two calls give the same bits.
 *
 * Supported: L == 4, 1 <= H, W <= LSR_TILES_MAX_SIDE.  Anything else, any NULL pointer, a workspace
 * smaller than lsr_tiles_workspace_size, lengths outside 0 .. LSR_TILES_MAX_LABEL and n != their sum are
 * LSR_EINVAL, decided before the device is touched.  n == 0 renders the segment maps alone (`tiles`
 * may then be NULL).
 *
 * Conventions: device pointers (but `lengths`, and `counts` as said); contiguous arrays; the library
 * allocates nothing: the caller provides lsr_tiles_workspace_size(L) bytes, 16-byte aligned, which carry
 * the census and the ranks from one step to the next, and desc [LSR_TILES_MAX_TILES * 6] int32;
 * everything runs on `stream` with no host synchronisation.  Return 0 or an LSR_E* code (lsr.h);
 * lsr_last_error().
 */
#ifndef LSR_TILES_H_
#define LSR_TILES_H_
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define LSR_TILES_LEVELS 4
#define LSR_TILES_MAX_LABEL 1023
#define LSR_TILES_MAX_TILES (LSR_TILES_LEVELS * LSR_TILES_MAX_LABEL)
#define LSR_TILES_SIDE 224          /* the tiles' height and width */
#define LSR_TILES_MAX_SIDE 16384    /* H and W */
#define LSR_TILES_DESC_INTS 6       /* level, label, x, y, w, h */
#define LSR_TILES_COUNTS 5          /* the plan's counts: four levels and the label-overflow flag */
#define LSR_TILES_CENSUS_ROWS 4     /* image rows of one census workgroup */

/* Bytes of workspace for one frame; -1 (and lsr_last_error) if L != 4. */
int64_t lsr_tiles_workspace_size(int32_t L);

int lsr_tiles_census(int32_t L, int32_t H, int32_t W, const int32_t *labels, int64_t workspace_bytes,
                     void *workspace, void *stream);

int lsr_tiles_plan(int32_t L, int32_t H, int32_t W, int64_t workspace_bytes, void *workspace, int32_t *desc,
                   int32_t *counts, void *stream);

int lsr_tiles_render(int32_t L, int32_t H, int32_t W, const int32_t *labels, const uint8_t *image,
                     int64_t workspace_bytes, const void *workspace, const int32_t *desc, const int32_t *lengths,
                     int32_t n, int32_t *seg_maps, float *tiles, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* LSR_TILES_H_ */
