// centers.hip -- C ABI of the status centres (include/lsr_centers.h) and the k-means of rows that
// are already in memory.  The fused kernel (time sampling through lang_deform, then the same k-means)
// lives beside the language MLP in deform_lang.hip (launch_centers_from_field).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>

#include "../../include/lsr.h"
#include "../../include/lsr_centers.h"
#include "centers_kmeans.h"
#include "deform_internal.h"
#include "lsr_host.h"

static_assert(lsr::CK_MAX_K == LSR_CENTERS_MAX_K && lsr::CK_MAX_S == LSR_CENTERS_MAX_SAMPLES &&
                  lsr::CK_MAX_D == LSR_CENTERS_MAX_DIM, "the kernel's limits are the header's");

namespace lsr {
int deform_lang_args(const lsr_deform_net* net, const void* workspace, int32_t P, LangDeformArgs* out);   // deform_api.hip

namespace {

constexpr int KM_WAVES = 4;   // rows per block at most: one wave each

// One wave per row; a block stages the rows of its waves ([S][D | 1] each) in the 33 KB sample buffer,
// so `rpb` = min(4, rows that fit) of its waves work.
__global__ void __launch_bounds__(64 * KM_WAVES) k_centers_kmeans(const float* __restrict__ x, int P, int S, int D, int K,
                                                                  int max_iter, int rpb, float* __restrict__ centers,
                                                                  int32_t* __restrict__ counts, float* __restrict__ inertia,
                                                                  int32_t* __restrict__ iters) {
    __shared__ float s_x[CK_XFLOATS];
    __shared__ float s_c[KM_WAVES][CK_MAX_K * CK_MAX_D];
    __shared__ uint8_t s_a[KM_WAVES][CK_MAX_S];
    const int tid = threadIdx.x, wave = tid >> 6, xp = ck_pitch(D);
    const size_t row0 = (size_t)blockIdx.x * rpb, total = (size_t)P * S * D;
    for (int i = tid; i < rpb * S * D; i += 64 * KM_WAVES) {
        const size_t src = row0 * S * D + i;
        if (src < total) s_x[(i / D) * xp + i % D] = x[src];   // i / D = local row * S + s
    }
    __syncthreads();
    const size_t row = row0 + wave;
    if (wave < rpb && row < (size_t)P)
        kmeans_wave(s_x + wave * S * xp, xp, S, D, K, max_iter, s_c[wave], s_a[wave], centers + row * K * D,
                    counts + row * K, inertia + row, iters + row);
}

int check_shape(int32_t P, int32_t S, int32_t D, int32_t K, int32_t max_iter) {
    if (K < 1 || K > LSR_CENTERS_MAX_K) return fail(LSR_EINVAL, "centres: 1 <= K <= 8");
    if (S < K || S > LSR_CENTERS_MAX_SAMPLES) return fail(LSR_EINVAL, "centres: K <= S <= 256 samples");
    if (D < 1 || D > LSR_CENTERS_MAX_DIM) return fail(LSR_EINVAL, "centres: 1 <= D <= 32 channels");
    if (max_iter < 1) return fail(LSR_EINVAL, "centres: max_iter >= 1");
    if (P < 0) return fail(LSR_EINVAL, "centres: P >= 0");
    return LSR_OK;
}

}  // namespace
}  // namespace lsr

extern "C" int lsr_centers_kmeans(const float* x, int32_t P, int32_t S, int32_t D, int32_t K, int32_t max_iter,
                                  float* centers, int32_t* counts, float* inertia, int32_t* iters, void* stream) {
    int rc = lsr::check_shape(P, S, D, K, max_iter);
    if (rc) return rc;
    if (P == 0) return LSR_OK;
    if (!x || !centers || !counts || !inertia || !iters)
        return lsr::fail(LSR_EINVAL, "centres: x, centers, counts, inertia and iters are required");
    const int rpb = std::max(1, std::min(lsr::KM_WAVES, lsr::CK_XFLOATS / (S * lsr::ck_pitch(D))));
    hipLaunchKernelGGL(lsr::k_centers_kmeans, dim3((P + rpb - 1) / rpb), dim3(64 * lsr::KM_WAVES), 0,
                       reinterpret_cast<hipStream_t>(stream), x, P, S, D, K, max_iter, rpb, centers, counts, inertia, iters);
    return lsr::launched("centres: k-means launch failed");
}

extern "C" int lsr_centers_from_field(const lsr_deform_net* net, const void* workspace, int32_t P, const float* lang,
                                      const float* times, uint32_t seed, int32_t S, int32_t K, int32_t max_iter,
                                      float* centers, int32_t* counts, float* inertia, int32_t* iters,
                                      float* samples_out, float* times_out, void* stream) {
    lsr::CentersArgs a{};
    int rc = lsr::deform_lang_args(net, workspace, P, &a.f);
    if (rc) return rc;
    rc = lsr::check_shape(P, S, net->lang_dim, K, max_iter);
    if (rc) return rc;
    if (P == 0) return LSR_OK;
    if (!lang || !centers || !counts || !inertia || !iters)
        return lsr::fail(LSR_EINVAL, "centres: lang, centers, counts, inertia and iters are required");
    a.f.lang = lang;
    a.times = times;
    a.seed = seed;
    a.S = S;
    a.K = K;
    a.max_iter = max_iter;
    // Gaussians per block: as many as the sample buffer holds, at most 16 (1600 rows = 25 full tiles of
    // the MLP at S = 100)
    a.gpb = std::max(1, std::min(16, lsr::CK_XFLOATS / (S * lsr::ck_pitch(net->lang_dim))));
    a.centers = centers;
    a.counts = counts;
    a.inertia = inertia;
    a.iters = iters;
    a.samples_out = samples_out;
    a.times_out = times_out;
    lsr::launch_centers_from_field(a, reinterpret_cast<hipStream_t>(stream));
    return lsr::launched("centres: fused launch failed");
}
