/*
 * lsr_train.h -- C ABI of the MI355X-native training-step glue, part of liblsr.so (SURVEY.md 8f
 * row 4): the optimizer step over the Gaussian SoA, the densification statistics, and the
 * densify / prune / opacity-reset row surgery of scene/gaussian_model.py.
 *
 * Reference interfaces these replace:
 *   - torch.optim.Adam(groups, lr=0.0, eps=1e-15).step()   scene/gaussian_model.py:301, train.py:420
 *       -> lsr_adam_step (one launch over every parameter group)
 *   - max_radii2D[vis] = max(max_radii2D[vis], radii[vis]);
 *     add_densification_stats(viewspace_grad, vis)        train.py:388-389, gaussian_model.py:746-748
 *       -> lsr_densify_stats
 *   - densify = densify_and_clone + densify_and_split      gaussian_model.py:726-731, 607-627, 575-605
 *       -> lsr_densify_plan (+ lsr_gather_rows, lsr_split_fixup)
 *   - prune                                                gaussian_model.py:714-723, 487-508
 *       -> lsr_prune_plan (+ lsr_gather_rows)
 *   - reset_opacity                                        gaussian_model.py:391-394, 446-459
 *       -> lsr_reset_opacity
 *   - exp / normalize / sigmoid of the render path          gaussian_renderer/__init__.py:191-193
 *       -> lsr_activate, lsr_activate_backward
 *   - the base stages' L1 image loss                         train.py:272-276
 *       -> lsr_l1_loss_views, lsr_l1_loss_views_backward
 *   - the same with its D-SSIM term, and the squared error of PSNR      train.py:335-337, utils/loss_utils.py:29-69
 *       -> lsr_image_loss_views, lsr_image_loss_views_backward
 *   - the 'lang' stages' masked L1 (+ cosine) loss against table[seg]   train.py:287-292, scene/cameras.py:92-118
 *       -> lsr_seg_loss_views, lsr_seg_loss_views_backward
 *
 * Conventions as lsr.h: device pointers, float32 unless stated, contiguous rows; the library
 * allocates nothing (plans take a workspace of lsr_train_workspace_bytes(P)); every launch on
 * `stream`; no host synchronisation (the plans leave their row counts in device memory, the
 * caller reads them to size the new tensors, as upstream's boolean indexing does).
 * Return 0 or an LSR_E* code (lsr.h); lsr_last_error().
 */
#ifndef LSR_TRAIN_H_
#define LSR_TRAIN_H_
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define LSR_ADAM_MAX_GROUPS 16

/* One parameter group of torch.optim.Adam (one tensor each, as gaussian_model.py:238-288). */
typedef struct lsr_adam_group {
    float *param;
    const float *grad;     /* NULL: the group is skipped (torch skips params whose .grad is None) */
    float *exp_avg;
    float *exp_avg_sq;
    int64_t n;             /* floats */
    double lr;
    int64_t step;          /* the group's step count including this update (1 on the first) */
} lsr_adam_group;

/* torch.optim.Adam (amsgrad = False, weight_decay = 0, maximize = False), per element:
 *   m = lerp(m, g, 1 - beta1);  v = v * beta2 + (1 - beta2) * g * g
 *   p -= lr / (1 - beta1^step) * m / (sqrt(v) / sqrt(1 - beta2^step) + eps)
 * with the bias corrections and step size computed in double on the host (as torch does with
 * Python floats) and the element arithmetic in float32.  All groups in one launch. */
int lsr_adam_step(const lsr_adam_group *groups, int32_t n_groups, double beta1, double beta2, double eps,
                  void *stream);

/* Densification statistics of one training iteration, for the Gaussians with radii[i] > 0
 * (radii = max over the iteration's views, train.py:266):
 *   max_radii2D[i] = max(max_radii2D[i], radii[i])
 *   xyz_gradient_accum[i] += |(g[i,0], g[i,1])|   (g = viewspace_point_tensor grad summed over views)
 *   denom[i] += 1
 * means2D_grad rows are grad_stride floats apart (3 for the [P,3] screen-space tensor). */
int lsr_densify_stats(int32_t P, const int32_t *radii, const float *means2D_grad, int32_t grad_stride,
                      float *max_radii2D, float *xyz_gradient_accum, float *denom, void *stream);

int64_t lsr_train_workspace_bytes(int32_t P);

/* Row map of densify (clone, then split into n_copies; the reference's N = 2):
 *   g[i] = xyz_gradient_accum[i] / denom[i]  (NaN -> 0)
 *   s[i] = max_k exp(scaling[i,k])            (raw log-scales, [P,3])
 *   clone[i] = |g[i]| >= grad_threshold and s[i] <= percent_dense * extent
 *   split[i] =  g[i]  >= grad_threshold and s[i] >  percent_dense * extent
 * Output row j of the densified model takes source row index[j]:
 *   [ rows not split, in order | cloned rows, in order | split rows, copy 0 | ... | copy n_copies-1 ]
 * which is the order the reference's cat-then-prune produces.  index holds at least
 * (n_copies + 1) * P int32; counts (device int64[3]) = {rows not split, cloned, split}. */
int lsr_densify_plan(int32_t P, const float *xyz_gradient_accum, const float *denom, const float *scaling,
                     float grad_threshold, float percent_dense, float extent, int32_t n_copies, int32_t *index,
                     int64_t *counts, void *workspace, void *stream);

/* Row map of prune: prune[i] = sigmoid(opacity[i]) < min_opacity, or, when max_screen_size > 0,
 * max_radii2D[i] > max_screen_size or max_k exp(scaling[i,k]) > 0.1 * extent.
 * index[0 .. counts[0]) = the kept rows in order; counts (device int64[1]). */
int lsr_prune_plan(int32_t P, const float *opacity, const float *max_radii2D, const float *scaling,
                   float min_opacity, float max_screen_size, float extent, int32_t *index, int64_t *counts,
                   void *workspace, void *stream);

/* One tensor of the row surgery: dst row j = src row index[j] for j < zero_from, and zeros for
 * j >= zero_from (the optimizer moments of appended rows).  row_bytes is any positive size. */
typedef struct lsr_row_tensor {
    const void *src;
    void *dst;
    int64_t row_bytes;
    int64_t zero_from;
} lsr_row_tensor;
#define LSR_GATHER_MAX_TENSORS 32
/* Every tensor in one launch (n_tensors <= LSR_GATHER_MAX_TENSORS); src and dst must not overlap. */
int lsr_gather_rows(int32_t n_tensors, const lsr_row_tensor *t, const int32_t *index, int64_t n_rows, void *stream);

/* The new rows of a split (gaussian_model.py:587-593), rows base .. base + n_new of the gathered
 * model (copy c of split row k is row base + c * n_split + k, n_new = n_copies * n_split):
 *   xyz[j]     = R(rotation[index[j]]) (exp(scaling[index[j]]) * sample[j - base]) + xyz[index[j]]
 *   scaling[j] = log(exp(scaling[index[j]]) / (0.8 n_copies))
 * R = build_rotation of the normalised quaternion (utils/general_utils.py:84-110); samples are
 * standard-normal [n_new, 3] draws (the reference's torch.normal(0, std) = std * z). */
int lsr_split_fixup(int64_t n_new, int64_t base, int32_t n_copies, const int32_t *index, const float *xyz_src,
                    const float *scaling_src, const float *rotation_src, const float *samples, float *xyz_dst,
                    float *scaling_dst, void *stream);

/* opacity = inverse_sigmoid(min(sigmoid(opacity), 0.01)); its Adam moments zeroed (exp_avg and
 * exp_avg_sq may be NULL). */
int lsr_reset_opacity(int32_t P, float *opacity, float *exp_avg, float *exp_avg_sq, void *stream);

/* render_views' V views of P Gaussians (gaussian_scene.py), every tensor in one launch (t[k].src /
 * dst / row_bytes, rows of whole floats; zero_from unused):
 *   lsr_repeat_rows:    dst row j = src row j mod n_rows, j < n_blocks * n_rows  (torch.Tensor.repeat)
 *   lsr_sum_row_blocks: dst row j = sum over b < n_blocks of src row b * n_rows + j, in b order (its
 *                       backward; torch sums two blocks the same way) */
int lsr_repeat_rows(int32_t n_tensors, const lsr_row_tensor *t, int64_t n_rows, int32_t n_blocks, void *stream);
int lsr_sum_row_blocks(int32_t n_tensors, const lsr_row_tensor *t, int64_t n_rows, int32_t n_blocks, void *stream);

/* The base stages' image loss (train.py:272-276: l1_loss(cat(images), cat(gts)[:, :3]) = mean |x - y|)
 * over V <= 8 views without stacking them: images[v] [n] floats (one [3,H,W] render), the view's
 * gt at gt + v * gt_view_stride (its first n floats: gts[v, :3]).  loss: one device float,
 * sum * (1 / (V n)), the partial sums added in a fixed order (deterministic; not PyTorch's order);
 * workspace >= lsr_l1_workspace_bytes(V).  The backward writes d_images[v] = sign(x - y) * (d_loss * (1 / (V n))),
 * PyTorch's abs / mean backward bit for bit. */
int64_t lsr_l1_workspace_bytes(int32_t V);
int lsr_l1_loss_views(int32_t V, int64_t n, const float *const *images, const float *gt, int64_t gt_view_stride,
                      float *loss, void *workspace, void *stream);
int lsr_l1_loss_views_backward(int32_t V, int64_t n, const float *const *images, const float *gt,
                               int64_t gt_view_stride, const float *d_loss, float *const *d_images, void *stream);

/* The image loss with its D-SSIM term (train.py:284,335-337: l1_loss + lambda_dssim * (1 - ssim), utils/loss_utils.py:29-69
 * with window_size 11) over V <= 8 views of one [C, H, W] shape without stacking them: images[v] the render of
 * view v, its ground truth at gt + v * gt_view_stride (gt_view_stride >= C H W: gts[:, :3] of a [V, 4, H, W] tensor
 * has 4 H W).  ssim_map per pixel and plane from the five zero-padded (padding 5) correlations with the separable,
 * normalised 11-tap Gaussian of sigma 1.5 (its float32 taps), C1 = 0.01^2, C2 = 0.03^2:
 *   ssim_map = (2 mu1 mu2 + C1)(2 s12 + C2) / ((mu1^2 + mu2^2 + C1)(s1 + s2 + C2)),  s = E[.] - mu^2.
 *   stats  [V][3]: per view  mean |x - y|, mean ssim_map, mean (x - y)^2  (the last is what PSNR needs,
 *                  utils/image_utils.py:17-38)
 *   totals [2]:    mean |x - y| and mean ssim_map over all V views (l1_loss and ssim(size_average=True) of the
 *                  stacked tensors)
 * One launch for the maps and one short launch that adds the block sums in a fixed order, in double (no atomics:
 * two calls give the same bits).  workspace >= lsr_image_loss_workspace_bytes(V, C, H, W) (-1 on invalid sizes:
 * V outside 1..8, C, H or W < 1, V C > 65535), 16-byte aligned; the forward leaves the per-pixel partial
 * derivatives of ssim_map towards (mu1, E[x^2], E[xy]) there (3 V C H W floats) and the backward reads them.
 * The backward writes every element of d_images[v] once:
 *   d_l1[0] * sign(x - y) / (V C H W)  +  d_ssim[0] * d (mean ssim_map) / d x,
 *   d (mean ssim_map) / d x = (conv(P_mu1) + 2 x conv(P_xx) + y conv(P_xy)) / (V C H W), conv the same correlation.
 * Either of d_l1 / d_ssim may be NULL (treated as 0).  With d_ssim NULL or a 0 behind it the maps are not read and
 * the result is lsr_l1_loss_views_backward's bit for bit.  No alignment beyond 4 bytes is asked of the images. */
int64_t lsr_image_loss_workspace_bytes(int32_t V, int32_t C, int32_t H, int32_t W);
int lsr_image_loss_views(int32_t V, int32_t C, int32_t H, int32_t W, const float *const *images, const float *gt,
                         int64_t gt_view_stride, float *stats, float *totals, void *workspace, void *stream);
int lsr_image_loss_views_backward(int32_t V, int32_t C, int32_t H, int32_t W, const float *const *images,
                                  const float *gt, int64_t gt_view_stride, const float *d_l1, const float *d_ssim,
                                  float *const *d_images, const void *workspace, void *stream);

/* The 'lang' stages' loss (train.py:287-292, utils/loss_utils.py:20-27) straight from the supervision files'
 * contents (scene/cameras.py:92-118), the dense ground truth never built.  One view: */
typedef struct lsr_seg_view {
    const float *image;    /* [C, H, W] the rendered language image */
    float *d_image;        /* [C, H, W] its gradient: written by the backward, ignored by the forward */
    const int32_t *seg;    /* [H, W] segment of each pixel; labelled iff 0 <= seg < n_seg, any other value
                              (the reference's -1, anything >= n_seg) is unlabelled and never used as an index */
    const float *table;    /* [n_seg, C] the segments' features */
    int32_t n_seg;
} lsr_seg_view;
/* Over V <= 8 views of one shape, with m the labelled mask, t = table[seg], a = x m, b = t m, N = V C H W:
 *   L1   = sum |a - b| / N
 *   cos  = mean over (v, c, h) of  sum_w a b / (max(|a|_w, 1e-8) max(|b|_w, 1e-8))
 *          (cos_loss's dim = -1 is the width axis: one similarity per image row and channel; 0 for a row
 *          without labelled pixels)
 *   loss = lam L1 (+ beta (1 - cos) when with_cos), one device float.
 * Every partial sum is added in a fixed order (no atomics: two calls give the same bits).  workspace >=
 * lsr_seg_loss_workspace_bytes(V, C, H, W) (-1 on invalid sizes), 16-byte aligned; with with_cos the forward leaves the rows'
 * (a.b, |a|^2, |b|^2) there and the backward of the same call reads them (it needs no workspace otherwise).
 * The backward writes every element of d_image:
 *   m (sign(x - t) ((d_loss lam) (1 / N)) - (d_loss beta / (V C H)) d cos / d a),  +0 where unlabelled;
 * its L1 part is PyTorch's mul / mean / abs backward bit for bit, and d cos / d a has no |a| term where
 * |a| <= 1e-8 (the clamp's constant branch).  16-byte loads and stores when W % 4 == 0 and every image, gradient
 * and map is 16-byte aligned, scalar ones otherwise. */
int64_t lsr_seg_loss_workspace_bytes(int32_t V, int32_t C, int32_t H, int32_t W);
int lsr_seg_loss_views(int32_t V, int32_t C, int32_t H, int32_t W, const lsr_seg_view *views, float lam, float beta,
                       int32_t with_cos, float *loss, void *workspace, void *stream);
int lsr_seg_loss_views_backward(int32_t V, int32_t C, int32_t H, int32_t W, const lsr_seg_view *views, float lam,
                                float beta, int32_t with_cos, const float *d_loss, void *workspace, void *stream);

/* The render path's activations over P rows in one launch (gaussian_renderer/__init__.py:191-193,
 * gaussian_model.py:38-46; replaces torch.exp / torch.nn.functional.normalize / torch.sigmoid and
 * their autograd backward there, GaussianScene.render_views):
 *   scales = exp(raw_scales) [P,3];  rotations = raw / max(|raw|, 1e-12) [P,4];  opacity = sigmoid(raw) [P]
 * Any raw input may be NULL (that output is skipped); rotation rows 16-byte aligned. */
int lsr_activate(int32_t P, const float *raw_scales, const float *raw_rotations, const float *raw_opacity,
                 float *scales, float *rotations, float *opacity, void *stream);
/* Their backward from the forward's outputs (scales, opacity) and the raw rotations:
 *   d_raw_scales = d_scales * scales;  d_raw_opacity = d_opacity * opacity * (1 - opacity);
 *   d_raw_rotations = (d - y (y . d)) / |raw| with y = raw / |raw| (d / 1e-12 when |raw| <= 1e-12).
 * A NULL upstream gradient counts as zero; a NULL output gradient is not computed. */
int lsr_activate_backward(int32_t P, const float *scales, const float *raw_rotations, const float *opacity,
                          const float *d_scales, const float *d_rotations, const float *d_opacity,
                          float *d_raw_scales, float *d_raw_rotations, float *d_raw_opacity, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* LSR_TRAIN_H_ */
