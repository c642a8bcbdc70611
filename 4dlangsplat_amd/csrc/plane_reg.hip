// plane_reg.hip -- the HexPlane regularisers with their gradient (include/lsr_plane_reg.h;
// scene/regulation.py:22-28 compute_plane_smoothness, scene/gaussian_model.py:763-802 compute_regulation).
// DESIGN.md 4.13.
//
// k_plane_reg         every plane of the call in one launch.  A block of 256 threads owns PR_BLOCK = 1024
//                     consecutive elements of one plane (the planes' block ranges are a prefix array in the
//                     kernel arguments; a block finds its plane by walking it, at most 24 uniform steps); a
//                     thread takes the four elements tid, tid + 256, ... of them, each on its own, so w is
//                     fastest across the lanes and each of the five rows an element reads (j - 2 ... j + 2 of
//                     its column) is read coalesced; four of the five come from the cache, where the
//                     neighbouring rows' threads put them.  The element's own second difference d2[j] (where
//                     j < H - 2) goes to the loss, the three that contain it to its gradient, |1 - t| to the
//                     L1 term.  Everything between the float32 loads and the one float32 store is float64.
//                     The block's two raw sums go to the workspace as float64: a thread's four in ascending
//                     order, xor butterflies inside the waves, the four waves added in wave order.
// k_plane_reg_finish  one block of 16 waves: wave w adds the partials of planes w and w + 16, lane l those
//                     of the plane's blocks l, l + 64, ..., then the same butterfly; thread 0 adds the
//                     planes' weighted terms in plane order.  A fixed order throughout, no atomics: two
//                     calls give the same bits.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>

#include "../../include/lsr.h"
#include "../../include/lsr_plane_reg.h"
#include "lsr_host.h"
#include "lsr_wave.h"

namespace {

using lsr::wave_sum;

constexpr int PR_MAX = LSR_PLANE_REG_MAX_PLANES;
constexpr int PR_BLOCK = LSR_PLANE_REG_BLOCK_ELEMS;     // elements of one block
constexpr int PR_THREADS = 256, PR_WAVES = PR_THREADS / 64, PR_PER_THREAD = PR_BLOCK / PR_THREADS;
static_assert(PR_BLOCK % PR_THREADS == 0, "a thread takes whole elements");
constexpr int PR_FINISH_WAVES = 16;
constexpr int64_t PR_MAX_ELEMS = 0x7fffffffLL;          // an element's index inside its plane is an int32

struct Plane {
    const float* t;
    float* grad;
    int32_t C, H, W;
    int32_t n;               // C H W
    double w_smooth, w_l1;
    double two_over_ns;      // 2 / (C (H - 2) W); 0 where H < 3
    double inv_n;            // 1 / (C H W)
};

struct Args {
    Plane p[PR_MAX];
    int32_t first_block[PR_MAX + 1];   // plane k owns blocks [first_block[k], first_block[k + 1])
    int32_t n_planes, accumulate;
};
static_assert(sizeof(Args) <= 4096, "the descriptors travel as kernel arguments");

__global__ void __launch_bounds__(PR_THREADS) k_plane_reg(const Args a, double* __restrict__ partial) {
    __shared__ double red[2][PR_WAVES];
    const int tid = threadIdx.x, b = blockIdx.x;
    int k = 0;
    while (k + 1 < a.n_planes && b >= a.first_block[k + 1]) ++k;
    const Plane& P = a.p[k];
    const int64_t e0 = (int64_t)(b - a.first_block[k]) * PR_BLOCK + tid;
    double sq = 0.0, ab = 0.0;
#pragma unroll
    for (int r = 0; r < PR_PER_THREAD; ++r) {
        const int64_t e = e0 + r * PR_THREADS;
        if (e >= P.n) break;
        const int W = P.W, H = P.H;
        const int j = ((int)e / W) % H;                  // the row inside the channel (e < n fits an int32)
        const float* t = P.t + e;
        const double t0 = (double)t[0];
        ab += fabs(1.0 - t0);
        double g_s = 0.0;
        if (H >= 3) {
            // rows outside the channel are never read
            const double tm2 = j >= 2 ? (double)t[-2 * (int64_t)W] : 0.0;
            const double tm1 = j >= 1 ? (double)t[-(int64_t)W] : 0.0;
            const double tp1 = j + 1 < H ? (double)t[W] : 0.0;
            const double tp2 = j + 2 < H ? (double)t[2 * (int64_t)W] : 0.0;
            const double da = j >= 2 ? (t0 - 2.0 * tm1) + tm2 : 0.0;                  // d2[j - 2]
            const double db = (j >= 1 && j + 1 < H) ? (tp1 - 2.0 * t0) + tm1 : 0.0;  // d2[j - 1]
            const double dc = j + 2 < H ? (tp2 - 2.0 * tp1) + t0 : 0.0;               // d2[j], the element's own
            sq += dc * dc;
            g_s = P.two_over_ns * ((da - 2.0 * db) + dc);
        }
        if (P.grad) {
            const double g_l1 = t0 < 1.0 ? -P.inv_n : (t0 > 1.0 ? P.inv_n : 0.0);   // -sign(1 - t) / N, sign(0) = 0
            const float g = (float)(P.w_smooth * g_s + P.w_l1 * g_l1);
            float* dst = P.grad + e;
            *dst = a.accumulate ? *dst + g : g;
        }
    }
    sq = wave_sum(sq);
    ab = wave_sum(ab);
    if ((tid & 63) == 0) { red[0][tid >> 6] = sq; red[1][tid >> 6] = ab; }
    __syncthreads();
    if (tid == 0) {
        for (int w = 1; w < PR_WAVES; ++w) { sq += red[0][w]; ab += red[1][w]; }
        partial[2 * (int64_t)b] = sq;
        partial[2 * (int64_t)b + 1] = ab;
    }
}

__global__ void __launch_bounds__(64 * PR_FINISH_WAVES)
k_plane_reg_finish(const Args a, const double* __restrict__ partial, double* __restrict__ terms,
                   float* __restrict__ total, double* __restrict__ total64) {
    __shared__ double weighted[PR_MAX];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int k = wave; k < a.n_planes; k += PR_FINISH_WAVES) {
        const Plane& P = a.p[k];
        double sq = 0.0, ab = 0.0;
#pragma unroll 8
        for (int b = a.first_block[k] + lane; b < a.first_block[k + 1]; b += 64) {
            sq += partial[2 * (int64_t)b];
            ab += partial[2 * (int64_t)b + 1];
        }
        sq = wave_sum(sq);
        ab = wave_sum(ab);
        if (lane == 0) {
            const double smooth = P.H >= 3 ? sq / ((double)P.C * (double)(P.H - 2) * (double)P.W) : 0.0;
            const double l1 = ab / (double)P.n;
            terms[2 * k] = smooth;
            terms[2 * k + 1] = l1;
            weighted[k] = (P.w_smooth != 0.0 ? P.w_smooth * smooth : 0.0) + (P.w_l1 != 0.0 ? P.w_l1 * l1 : 0.0);
        }
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double s = 0.0;
        for (int k = 0; k < a.n_planes; ++k) s += weighted[k];
        *total64 = s;
        *total = (float)s;
    }
}

// the checks the size query and the call share; fills `a` (pointers included: the query ignores them)
int check_planes(const char* what, int32_t n_planes, const lsr_plane_desc* planes, bool need_pointers, Args* a) {
    const std::string w(what);
    if (n_planes < 0 || n_planes > PR_MAX)
        return lsr::fail(LSR_EINVAL, w + ": n_planes must be in [0, " + std::to_string(PR_MAX) + "], got " +
                                         std::to_string(n_planes));
    if (n_planes > 0 && !planes) return lsr::fail(LSR_EINVAL, w + ": the plane descriptors are required");
    int64_t blocks = 0;
    a->n_planes = n_planes;
    a->first_block[0] = 0;
    for (int k = 0; k < n_planes; ++k) {
        const lsr_plane_desc& d = planes[k];
        const std::string pk = w + ": plane " + std::to_string(k);
        if (need_pointers && !d.t) return lsr::fail(LSR_EINVAL, pk + " is null");
        if (d.C < 1 || d.H < 1 || d.W < 1) return lsr::fail(LSR_EINVAL, pk + ": C, H and W must be >= 1");
        if (d.w_smooth != 0.0 && d.H < 3)
            return lsr::fail(LSR_EINVAL, pk + ": a second difference needs H >= 3 where w_smooth != 0, got H = " +
                                             std::to_string(d.H));
        const int64_t ch = (int64_t)d.C * d.H;           // < 2^62
        if (ch > PR_MAX_ELEMS || ch * d.W > PR_MAX_ELEMS)
            return lsr::fail(LSR_EINVAL, pk + ": C * H * W must fit an int32 element index (at most 2^31 - 1)");
        const int64_t n = ch * d.W;
        Plane& P = a->p[k];
        P.t = d.t;
        P.grad = d.grad;
        P.C = d.C; P.H = d.H; P.W = d.W;
        P.n = (int32_t)n;
        P.w_smooth = d.w_smooth;
        P.w_l1 = d.w_l1;
        P.two_over_ns = d.H >= 3 ? 2.0 / ((double)d.C * (double)(d.H - 2) * (double)d.W) : 0.0;
        P.inv_n = 1.0 / (double)n;
        blocks += (n + PR_BLOCK - 1) / PR_BLOCK;         // 24 planes of at most 2^21 blocks: fits an int32
        a->first_block[k + 1] = (int32_t)blocks;
    }
    return LSR_OK;
}

}  // namespace

extern "C" int64_t lsr_plane_reg_workspace_bytes(int32_t n_planes, const lsr_plane_desc* planes) {
    Args a;
    if (check_planes("lsr_plane_reg_workspace_bytes", n_planes, planes, false, &a)) return -1;
    const int64_t blocks = a.first_block[n_planes];
    return (blocks > 0 ? blocks : 1) * (int64_t)(2 * sizeof(double));
}

extern "C" int lsr_plane_reg(int32_t n_planes, const lsr_plane_desc* planes, int32_t accumulate, void* workspace,
                             double* terms, float* total, double* total64, void* stream) {
    Args a;
    if (int rc = check_planes("lsr_plane_reg", n_planes, planes, true, &a)) return rc;
    if (!workspace || !terms || !total || !total64)
        return lsr::fail(LSR_EINVAL, "lsr_plane_reg: workspace, terms, total and total64 are required");
    if (reinterpret_cast<uintptr_t>(workspace) & 7)
        return lsr::fail(LSR_EINVAL, "lsr_plane_reg: workspace must be 8-byte aligned");
    a.accumulate = accumulate != 0;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const int32_t blocks = a.first_block[n_planes];
    if (blocks > 0)
        hipLaunchKernelGGL(k_plane_reg, dim3((unsigned)blocks), dim3(PR_THREADS), 0, st, a, static_cast<double*>(workspace));
    hipLaunchKernelGGL(k_plane_reg_finish, dim3(1), dim3(64 * PR_FINISH_WAVES), 0, st, a,
                       static_cast<const double*>(workspace), terms, total, total64);
    return lsr::launched("lsr_plane_reg launch failed");
}
