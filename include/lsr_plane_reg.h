/*
 * lsr_plane_reg.h -- C ABI of the HexPlane regularisers (second-difference smoothness of the planes, the
 * L1 pull of the time planes towards 1) with their gradient, part of liblsr.so.
 *
 * Reference behaviour replaced:
 *   compute_plane_smoothness      scene/regulation.py:22-28
 *   GaussianModel._plane_regulation / _time_regulation / _l1_regulation / compute_regulation
 *                                 scene/gaussian_model.py:763-802
 *
 * A plane is a contiguous float32 tensor t [1, C, H, W] (the field's grid.grids.{s}.{ci}).  Per plane:
 *   d2[c, i, w]  = (t[c, i+2, w] - 2 t[c, i+1, w]) + t[c, i, w]            i in [0, H - 2)
 *   smooth       = sum d2^2 / N_s,   N_s = C (H - 2) W                     (along dimension 2 only)
 *   d smooth / d t[c, j, w] = (2 / N_s) ((d2[j-2] - 2 d2[j-1]) + d2[j]),   d2 = 0 outside [0, H - 2)
 *   l1           = sum |1 - t| / N,  N = C H W
 *   d l1 / d t   = -sign(1 - t) / N,  sign(0) = 0                          (torch's abs backward)
 * and over the planes of one call
 *   total        = sum_p (w_smooth[p] smooth[p] + w_l1[p] l1[p])           in plane order
 *   grad[p]      = w_smooth[p] d smooth + w_l1[p] d l1
 * compute_regulation(time_smoothness_weight, l1_time_planes_weight, plane_tv_weight) is this with
 * w_smooth = plane_tv_weight, w_l1 = 0 on the spatial planes (ci 0, 1, 3) and w_smooth =
 * time_smoothness_weight, w_l1 = l1_time_planes_weight on the time planes (ci 2, 4, 5).
 *
 * Precision: inputs and gradients are float32; the differences, squares, sums and the weighted gradient
 * are float64, the gradient rounded to float32 once (accumulate != 0: then added in float32 to what
 * grad holds).  Every sum has a fixed order and nothing uses atomics: two calls give the same bits.
 *
 * terms [n_planes][2] float64 receives the unweighted {smooth, l1} of every plane whatever its weights
 * (smooth is 0 for a plane with H < 3, where the reference's mean over nothing is NaN: such a plane
 * must have w_smooth == 0); total (float32) and total64 (float64) receive the weighted total.
 *
 * Supported: 0 <= n_planes <= LSR_PLANE_REG_MAX_PLANES (0: total 0), C, H, W >= 1, C H W <= 2^31 - 1,
 * H >= 3 where w_smooth != 0.  Anything else, and any NULL pointer but a plane's grad (NULL: that plane
 * contributes to the loss only), is LSR_EINVAL, decided before the device is touched.
 *
 * Conventions: device pointers; the descriptors themselves are host memory, read before the call
 * returns; the library allocates nothing: the caller provides lsr_plane_reg_workspace_bytes(...) bytes,
 * 8-byte aligned, which a call may overwrite; everything runs on `stream` with no host synchronisation.
 * Return 0 or an LSR_E* code (lsr.h); lsr_last_error().
 */
#ifndef LSR_PLANE_REG_H_
#define LSR_PLANE_REG_H_
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define LSR_PLANE_REG_API_VERSION 1
#define LSR_PLANE_REG_MAX_PLANES 24      /* 6 planes of up to 4 scales */
#define LSR_PLANE_REG_BLOCK_ELEMS 1024   /* plane elements of one block and of one partial */

typedef struct lsr_plane_desc {
    const float *t;      /* [1, C, H, W] contiguous */
    float *grad;         /* the same layout, or NULL */
    int32_t C, H, W;
    double w_smooth;     /* weight of the smoothness term in total and grad */
    double w_l1;         /* weight of the L1 term */
} lsr_plane_desc;

/* Bytes of workspace for a call on these planes (only their shapes are read); -1 (and lsr_last_error)
 * if invalid. */
int64_t lsr_plane_reg_workspace_bytes(int32_t n_planes, const lsr_plane_desc *planes);

/* terms [n_planes][2], total [1], total64 [1] and every non-NULL grad are written (grads added to when
 * accumulate != 0). */
int lsr_plane_reg(int32_t n_planes, const lsr_plane_desc *planes, int32_t accumulate, void *workspace,
                  double *terms, float *total, double *total64, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* LSR_PLANE_REG_H_ */
