/*
 * lsr_autoencoder.h -- C ABI of the language autoencoder (eval-mode encode, eval-mode reconstruction
 * loss, one fused training step), part of liblsr.so.  It produces what the rest of the library starts
 * from: the compressed *_f.npy tables and the checkpoint whose decoder half lsr_query.h / lsr_video.h run.
 *
 * Reference behaviour replaced:
 *   Autoencoder                         autoencoder/model.py:5-46
 *   the training step, the eval loss    autoencoder/train.py:114-129, 149-182 (l2_loss, cos_loss, Adam)
 *   the compression pass                autoencoder/test.py:85-99 (eval-mode encode of every row)
 *
 * With e_i = enc_dims[i], d_j = dec_dims[j], x [rows, feature_dim]:
 *   h_0 = x W_0^T + b_0                                       W_i [e_i, e_{i-1}] row-major (nn.Linear)
 *   h_i = relu(bn_i(h_{i-1})) W_i^T + b_i      0 < i < n_enc  bn_i over the e_{i-1} columns
 *   u   = z / |z|,  z = h_{n_enc - 1}                         no epsilon: a zero z gives NaN (lsr_query.h)
 *   g_0 = u V_0^T + c_0,  g_j = relu(g_{j-1}) V_j^T + c_j     V_j [d_j, d_{j-1}], d_{-1} = the latent width
 *   out = y / |y|,  y = g_{n_dec - 1},  d_{n_dec - 1} = feature_dim
 * bn_i(h) = (h - mean) / sqrt(var + 1e-5) * weight + bias: eval mode takes the running statistics,
 * train mode the batch's mean and biased variance, and moves the running statistics by momentum 0.1
 * (the running variance gets the unbiased batch variance) and adds one to the batch count.
 *   l2  = sum((out - x)^2) / (B * feature_dim)
 *   cos = 1 - mean_b (out_b . x_b) / (max(|out_b|, 1e-8) max(|x_b|, 1e-8))
 *   loss = l2 + cos_weight * cos, followed by torch.optim.Adam's update of every parameter:
 *   m = m + (1 - beta1) (g - m);  v = beta2 v + (1 - beta2) g^2
 *   p -= lr / (1 - beta1^t) * m / (sqrt(v) / sqrt(1 - beta2^t) + eps)
 *
 * Every product runs on the exact f32-input MFMA.  One kernel per layer and direction: bias, the
 * BatchNorm statistics, normalise and ReLU are prologues and epilogues of the layer kernels, and a
 * layer's weight gradient is applied by Adam in the kernel that computes it (no gradient of a weight is
 * stored).  Fixed summation order, no atomics: two calls from the same state give the same bits, and in
 * eval mode a row's result does not depend on the other rows of the call.
 *
 * Supported: 1 <= n_enc, n_dec <= LSR_AE_MAX_LAYERS; feature_dim and every hidden width a multiple of 16
 * and <= LSR_AE_MAX_WIDTH; the latent width enc_dims[n_enc - 1] in [1, LSR_AE_MAX_LATENT];
 * dec_dims[n_dec - 1] == feature_dim; n_rows >= 0 (0: nothing is launched); 2 <= batch <=
 * LSR_AE_MAX_BATCH.  Anything else, any NULL pointer, and a workspace that is too small is LSR_EINVAL,
 * decided before the device is touched.
 *
 * Conventions: device pointers, float32 (bn_count int64), contiguous; the library allocates nothing: the
 * caller provides lsr_ae_workspace_size(...) bytes, 16-byte aligned, which a call may overwrite;
 * everything runs on `stream` with no host synchronisation.  Return 0 or an LSR_E* code (lsr.h);
 * lsr_last_error().
 */
#ifndef LSR_AUTOENCODER_H_
#define LSR_AUTOENCODER_H_
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define LSR_AE_API_VERSION 1
#define LSR_AE_MAX_LAYERS 8       /* Linear layers of one half */
#define LSR_AE_MAX_WIDTH 4096
#define LSR_AE_MAX_LATENT 32
#define LSR_AE_MAX_BATCH 64       /* rows of one training step: one block holds a column slab of the batch */
#define LSR_AE_EVAL_CHUNK 2048    /* rows of one pass of encode / eval_loss: what the workspace is sized for */

/* The trainable tensors of the autoencoder, or Adam's first or second moments of them.  bn_*[i] belong
 * to the BatchNorm in front of encoder layer i (width enc_dims[i - 1]); index 0 is unused. */
typedef struct lsr_ae_params {
    float *enc_w[LSR_AE_MAX_LAYERS];
    float *enc_b[LSR_AE_MAX_LAYERS];
    float *bn_w[LSR_AE_MAX_LAYERS];
    float *bn_b[LSR_AE_MAX_LAYERS];
    float *dec_w[LSR_AE_MAX_LAYERS];
    float *dec_b[LSR_AE_MAX_LAYERS];
} lsr_ae_params;

typedef struct lsr_autoencoder {
    int32_t n_enc, n_dec;
    int32_t feature_dim;
    int32_t enc_dims[LSR_AE_MAX_LAYERS];        /* enc_dims[n_enc - 1]: the latent width */
    int32_t dec_dims[LSR_AE_MAX_LAYERS];        /* dec_dims[n_dec - 1] == feature_dim */
    lsr_ae_params p;
    float *bn_mean[LSR_AE_MAX_LAYERS];          /* running_mean, running_var, num_batches_tracked */
    float *bn_var[LSR_AE_MAX_LAYERS];
    int64_t *bn_count[LSR_AE_MAX_LAYERS];
} lsr_autoencoder;

/* Call once before the other lsr_ae_* entry points with LSR_AE_API_VERSION of the header the caller was
 * built against; a caller of another version is refused (LSR_EINVAL, every entry point). */
int lsr_ae_require_api(int32_t caller_version);

/* Bytes of workspace of a call over n_rows rows: training != 0 for lsr_ae_train_step (n_rows is the
 * batch), 0 for lsr_ae_encode and lsr_ae_eval_loss.  Only the dims of the net are read; a negative
 * return is an LSR_E* code, negated. */
int64_t lsr_ae_workspace_size(const lsr_autoencoder *net, int64_t n_rows, int32_t training);

/* Eval mode: rows [n_rows, feature_dim] -> latents [n_rows, latent], unit vectors. */
int lsr_ae_encode(const lsr_autoencoder *net, int64_t n_rows, const float *rows, float *latents, void *ws,
                  int64_t ws_bytes, void *stream);

/* Eval mode: sums[0] = sum over rows and features of (out - x)^2, sums[1] = sum over rows of the cosine of
 * out and x (float64, fixed order).  The reconstruction is not stored. */
int lsr_ae_eval_loss(const lsr_autoencoder *net, int64_t n_rows, const float *rows, double *sums, void *ws,
                     int64_t ws_bytes, void *stream);

/* One training step on rows [batch, feature_dim]: forward in train mode, the loss, its gradient and
 * Adam's update of every parameter with the moments m and v; t is the step's number, from 1.
 * losses[0] = l2, losses[1] = cos of this step (before the update). */
int lsr_ae_train_step(const lsr_autoencoder *net, const lsr_ae_params *m, const lsr_ae_params *v, int32_t batch,
                      const float *rows, double lr, double beta1, double beta2, double eps, int64_t t,
                      double cos_weight, float *losses, void *ws, int64_t ws_bytes, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* LSR_AUTOENCODER_H_ */
