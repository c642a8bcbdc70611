/*
 * lsr_query.h -- C ABI of the open-vocabulary query (fused feature decode + relevancy maps), part
 * of liblsr.so.  It consumes what the renderer produces: the low-dimensional language image.
 *
 * Reference behaviour replaced:
 *   Autoencoder.decode                  autoencoder/model.py:42-46 (Linear / ReLU chain, L2 norm),
 *                                       called at eval/eval.py:611-616
 *   OpenCLIPNetwork.get_max_across /    eval/openclip_encoder.py:41-56, 96-112 (pairwise softmax of
 *   get_relevancy                       each positive against every negative, minimum over negatives)
 *
 * Per pixel, with x0 = latent[pixel, 0:c_in]:
 *   x_{i+1} = W_i . (i > 0 ? relu(x_i) : x_i) + b_i          W_i [out_i, in_i] row-major (nn.Linear)
 *   f       = x_n / |x_n|                                     no epsilon: a zero vector gives NaN
 *   s_j     = f . e_j                                         positives, then negatives
 *   relevancy_j = sigmoid(scale * (s_pos_j - max_i s_neg_i))  == min_i softmax(scale [s_pos_j, s_neg_i])[0]
 * Every layer and the phrase product run on the exact f32-input MFMA; the d_out-wide vector of the
 * relevancy entry point never leaves the chip.  Fixed summation order, no atomics: two calls give
 * the same bits.
 *
 * Supported: 1 <= n_layers <= 8, 1 <= c_in = dims[0] <= 32, every other width a multiple of 16 and
 * <= 512, n_pos >= 1, n_neg >= 1, n_pos + n_neg <= 64, n_pix >= 0 (0: nothing is launched).
 * Anything else, and any NULL pointer, is LSR_EINVAL, decided before the device is touched.
 *
 * Conventions: device pointers, float32; weights, biases, embeddings ([n, d_out]) and outputs
 * contiguous; the library allocates nothing; everything runs on `stream` with no host
 * synchronisation.  Return 0 or an LSR_E* code (lsr.h); lsr_last_error().
 *
 * The latent is addressed as latent[pixel * pix_stride + channel * chan_stride] (in floats): the
 * renderer's [C, H, W] image is pix_stride = 1, chan_stride = H * W; an [H, W, C] array (the
 * renders_npy files) is pix_stride = C, chan_stride = 1.
 */
#ifndef LSR_QUERY_H_
#define LSR_QUERY_H_
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define LSR_QUERY_API_VERSION 1
#define LSR_QUERY_MAX_LAYERS 8
#define LSR_QUERY_MAX_PHRASES 64   /* n_pos + n_neg of one call */
#define LSR_QUERY_MAX_WIDTH 512
#define LSR_QUERY_MAX_INPUT 32     /* c_in */

typedef struct lsr_decoder {
    int32_t n_layers;
    int32_t dims[LSR_QUERY_MAX_LAYERS + 1];     /* dims[0] = c_in, dims[n_layers] = d_out */
    const float *weight[LSR_QUERY_MAX_LAYERS];  /* [dims[i + 1], dims[i]] */
    const float *bias[LSR_QUERY_MAX_LAYERS];    /* [dims[i + 1]] */
} lsr_decoder;

/* Call once before the other lsr_query_* entry points with LSR_QUERY_API_VERSION of the header the
 * caller was built against; a caller of another version is refused (LSR_EINVAL, every entry point)
 * instead of having its lsr_decoder misread. */
int lsr_query_require_api(int32_t caller_version);

/* relevancy [n_pos, n_pix]: the relevancy of every positive phrase at every pixel. */
int lsr_query_relevancy(const lsr_decoder *dec, int64_t n_pix, const float *latent, int64_t pix_stride,
                        int64_t chan_stride, int32_t n_pos, const float *pos_embeds, int32_t n_neg,
                        const float *neg_embeds, float scale, float *relevancy, void *stream);

/* features [n_pix, d_out]: the decoded unit vectors themselves (Autoencoder.decode). */
int lsr_query_decode(const lsr_decoder *dec, int64_t n_pix, const float *latent, int64_t pix_stride,
                     int64_t chan_stride, float *features, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* LSR_QUERY_H_ */
