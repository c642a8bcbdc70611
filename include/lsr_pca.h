/*
 * lsr_pca.h -- C ABI of the PCA colouring of language images (moments, basis, projection), part of
 * liblsr.so.  It consumes what the renderer produces: the low-dimensional language image.
 *
 * Reference behaviour replaced:
 *   pca_compress         render.py:52-65 (sklearn PCA(n_components=3).fit_transform over the pixels,
 *                        one min-max over the three channels), called at render.py:113-124
 *   to8b                 render.py: (255 * clip(x, 0, 1)).astype(uint8)
 *
 * With x[p, c] = frame[p * pix_stride + c * chan_stride] (in floats; the renderer's [C, H, W] image is
 * pix_stride = 1, chan_stride = H * W; an [H, W, C] array is pix_stride = C, chan_stride = 1) and N
 * pixels in all:
 *   m    = sum_p x / N
 *   cov  = sum_p (x - m)(x - m)^T / (N - 1)
 *   v_k  = eigenvector of the k-th largest eigenvalue of cov, k = 0, 1, 2, its sign chosen so that its
 *          entry of largest magnitude is positive (sklearn's svd_flip(u_based_decision=False))
 *   y    = (x - m) . v_k                                              -> y [n_pix, 3]
 *   out  = (y - min y) / (max y - min y)     one min and one max over all three channels and all pixels
 * The departure from the reference: max y == min y (a constant image, where the reference divides
 * 0 by 0) gives zeros.
 *
 * The work is split into accumulating over pixels (lsr_pca_sums, then lsr_pca_gram), solving
 * (lsr_pca_basis) and applying (lsr_pca_project, lsr_pca_colorize_*), so that one basis and one range
 * can serve many frames: the sweeps add into float64 accumulators `sums` [32] and `gram` [32 * 32]
 * (row-major, channels past C are zero), and lsr_pca_project folds each frame's min and max into
 * `range` [2].  `reset` != 0 makes a call overwrite its accumulator instead of adding to it: set it
 * on the first frame of a fit.  The Gram matrix is centred while it is summed (lsr_pca_gram takes the
 * finished sums), never corrected by N m m^T afterwards.
 *
 * The pixel sums are taken in float64; the centred Gram products run on the exact f32-input MFMA into
 * per-block float32 partials (2048 pixels each) that are added in float64; every sum has a fixed
 * order and nothing uses atomics: two calls give the same bits.  The eigen-solve is a cyclic Jacobi
 * iteration in float64 with a fixed round-robin ordering and a fixed convergence rule.
 *
 * Supported: 4 <= C <= 32, n_pix >= 0 (0: the call launches nothing, `reset` included), strides >= 0
 * that address memory the caller owns for every pixel and channel (the library cannot check that),
 * n_total >= 2 at the basis step.  Anything else, and any NULL pointer, is LSR_EINVAL, decided before
 * the device is touched; the exceptions are lsr_pca_project's `y` (NULL: only the range is taken) and
 * `range` (NULL: only y is written, no fold is launched and no workspace is needed), not both.
 *
 * Conventions: device pointers; accumulators, outputs and y contiguous; the library allocates
 * nothing: the caller provides lsr_pca_workspace_bytes(C, n_pix) bytes, 8-byte aligned, which a call
 * may overwrite; everything runs on `stream` with no host synchronisation.  Return 0 or an LSR_E*
 * code (lsr.h); lsr_last_error().
 */
#ifndef LSR_PCA_H_
#define LSR_PCA_H_
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define LSR_PCA_MIN_CHANNELS 4
#define LSR_PCA_MAX_CHANNELS 32
#define LSR_PCA_BLOCK_PIXELS 2048   /* pixels of one per-block partial */
#define LSR_PCA_TILE_PIXELS 256     /* pixels a block stages at once */
#define LSR_PCA_FINISH_WAVES 16     /* the cross-block sums: wave w adds the partials of blocks w, w + 16, ... */
#define LSR_PCA_RANGE_THREADS 256   /* the cross-block min / max: thread t folds blocks t, t + 256, ... */

/* Bytes of workspace for any of the sweeps over n_pix pixels; -1 (and lsr_last_error) if invalid. */
int64_t lsr_pca_workspace_bytes(int32_t C, int64_t n_pix);

/* sums [32] float64 += (or =, with reset) the per-channel sums of the frame. */
int lsr_pca_sums(int32_t C, int64_t n_pix, const float *frame, int64_t pix_stride, int64_t chan_stride,
                 int32_t reset, double *sums, void *workspace, void *stream);

/* gram [32 * 32] float64 += (or =) sum_p (x - m)(x - m)^T of the frame, with m = sums / n_total: sums
 * is the finished accumulator of lsr_pca_sums over all n_total pixels of the fit. */
int lsr_pca_gram(int32_t C, int64_t n_pix, const float *frame, int64_t pix_stride, int64_t chan_stride,
                 const double *sums, int64_t n_total, int32_t reset, double *gram, void *workspace,
                 void *stream);

/* mean [C], components [3, C], eigenvalues [3] (of cov, descending) float32, from the accumulators. */
int lsr_pca_basis(int32_t C, int64_t n_total, const double *sums, const double *gram, float *mean,
                  float *components, float *eigenvalues, void *stream);

/* y [n_pix, 3] float32 (or NULL); range [2] (or NULL) = {min, max} of y, folded into what range holds
 * unless reset. */
int lsr_pca_project(int32_t C, int64_t n_pix, const float *frame, int64_t pix_stride, int64_t chan_stride,
                    const float *mean, const float *components, int32_t reset, float *y, float *range,
                    void *workspace, void *stream);

/* out [n_pix, 3] = clip((y - range[0]) / (range[1] - range[0]), 0, 1); zeros if range[1] == range[0]. */
int lsr_pca_colorize_f32(int64_t n_pix, const float *y, const float *range, float *out, void *stream);

/* the same as bytes: floor(255 * clip(., 0, 1)), the reference's to8b. */
int lsr_pca_colorize_u8(int64_t n_pix, const float *y, const float *range, uint8_t *out, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* LSR_PCA_H_ */
