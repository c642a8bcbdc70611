/*
 * lsr_centers.h -- C ABI of the status centres of the discrete language stage (time sampling of the
 * language field and per-Gaussian k-means, fused), part of liblsr.so.  It produces the
 * [P, centers, lang_dim] language tensor that a LSR_DEFORM_LANG_DISCRETE field reads (lsr_deform.h).
 *
 * Reference behaviour replaced:
 *   GaussianModel.generate_multi_feature_centers   scene/gaussian_model.py:804-845, the
 *                        init_from_stage == 'fine-lang' branch (:826-843): the language feature of every
 *                        Gaussian through the field at 100 random times, the [P, 100, D] result moved to
 *                        the host, one sklearn.cluster.KMeans(n_clusters = centers_num) fit per Gaussian
 * Two departures, both deliberate.  The reference takes [-1] of the field's outputs (:830), which is
 * coff and None there; the language output (index -2) is what is sampled here.  sklearn's k-means++
 * random stream is not reproduced: the seeding below is deterministic.
 *
 * The k-means of one row x[S, D] (all arithmetic float32, every sum in ascending s, d, j order):
 *   seeding (maximin)   m = (sum_s x_s) / S;  c_0 = the sample of largest |x_s - m|^2;
 *                       c_j = the sample of largest min_{i<j} |x_s - c_i|^2;  ties: the lowest s
 *   assignment          a_s = argmin_j |x_s - c_j|^2 as sum_d (x - c)^2 (never the expanded form);
 *                       ties: the lowest j
 *   update              a centre with n >= 1 samples becomes their mean, evaluated as
 *                       c + (sum_{s: a_s = j} (x_s - c)) / n  (c the centre before the update: the
 *                       mean of identical samples is that sample bit for bit); an empty centre keeps
 *                       its value
 *   loop                assign; then { update, iters += 1, assign } until the assignment changed
 *                       nothing or iters == max_iter.  So iters >= 1, and the last assignment is
 *                       against the returned centres: counts and inertia (sum_s |x_s - c_{a_s}|^2) come
 *                       from it.
 * Centres stay in seeding order and are not normalised (the discrete field normalises each centre).
 * No float atomics and a fixed summation order: two calls give the same bits.
 *
 * The sample times of lsr_centers_from_field, when none are given: stateless, from (seed, g, s) alone,
 *   h = seed ^ (g * 0x9E3779B1) ^ (s * 0x85EBCA77)                      (uint32, wrapping)
 *   h ^= h >> 16;  h *= 0x7FEB352D;  h ^= h >> 15;  h *= 0x846CA68B;  h ^= h >> 16
 *   t = (h >> 8) * 2^-24                                                 in [0, 1), exact in float32
 *
 * Supported: 1 <= K <= 8, K <= S <= 256, 1 <= D <= 32, max_iter >= 1, P >= 0 (0: nothing is launched);
 * for lsr_centers_from_field the net's lang_mode is RESIDUAL or NORESNET and D is its lang_dim.
 * Anything else, and a NULL required pointer, is LSR_EINVAL, decided before the device is touched.
 *
 * Conventions: device pointers, contiguous; the library allocates nothing; everything runs on
 * `stream` with no host synchronisation.  Return 0 or an LSR_E* code (lsr.h); lsr_last_error().
 */
#ifndef LSR_CENTERS_H_
#define LSR_CENTERS_H_
#include <stdint.h>
#include "lsr_deform.h"
#ifdef __cplusplus
extern "C" {
#endif

#define LSR_CENTERS_MAX_K 8
#define LSR_CENTERS_MAX_SAMPLES 256
#define LSR_CENTERS_MAX_DIM 32

/* k-means of every row of x [P, S, D]: centers [P, K, D], counts [P, K] int32, inertia [P],
 * iters [P] int32. */
int lsr_centers_kmeans(const float *x, int32_t P, int32_t S, int32_t D, int32_t K, int32_t max_iter,
                       float *centers, int32_t *counts, float *inertia, int32_t *iters, void *stream);

/* The fused path.  For every Gaussian g: l = lang[g] / (|lang[g]| + 1e-9); S times (times [P, S], or
 * NULL: the generator above with `seed`); x_s = the language output of lsr_deform_forward for the
 * language input l at time t_s (the same arithmetic: normalize((l +) lang_deform(relu([l, poc_fre(t_s)])))),
 * which depends on nothing else of the Gaussian; then the k-means above on the S rows, which never
 * leave the chip unless samples_out [P, S, D] is given.  times_out [P, S] (or NULL) receives the
 * times used.  `net` and `workspace` are a prepared field's (lsr_deform_prepare); D = net->lang_dim. */
int lsr_centers_from_field(const lsr_deform_net *net, const void *workspace, int32_t P, const float *lang,
                           const float *times, uint32_t seed, int32_t S, int32_t K, int32_t max_iter,
                           float *centers, int32_t *counts, float *inertia, int32_t *iters, float *samples_out,
                           float *times_out, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* LSR_CENTERS_H_ */
