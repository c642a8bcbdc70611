// lang_loss.hip -- the 'lang' stages' loss straight from (language image, segment map, feature table)
// (include/lsr_train.h: lsr_seg_loss_views / _backward; train.py:287-292, utils/loss_utils.py:20-27,
// scene/cameras.py:92-118).  The dense ground truth table[seg] and the masked copies of image and
// ground truth are never materialised: the forward reads each image once, the backward reads it once
// more and writes its gradient.
//
// One workgroup per (view, image row): the row's labels are range-checked once (anything outside
// [0, n_seg) becomes -1 and is never used as an index) and kept in LDS, then the channels stream by,
// coalesced along w, 16 bytes per lane where the rows are 16-byte aligned.  The table lookups are plain
// global gathers (the table is L2-resident and neighbouring pixels share a segment).  Every sum is
// added in a fixed order (lanes by butterfly, waves and rows in index order): no atomics, two calls
// give the same bits.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>

#include "../../include/lsr.h"
#include "../../include/lsr_train.h"
#include "lsr_host.h"
#include "lsr_wave.h"

namespace {

using lsr::aligned16;
using lsr::launched;
using lsr::wave_sum;

constexpr int SL_MAX_VIEWS = 8, SL_THREADS = 256, SL_WAVES = SL_THREADS / 64;
constexpr int SL_SEG_LDS = 4096;     // labels of one row kept in LDS (16 KB); wider rows re-read the map
constexpr int SL_CCHUNK = 32;        // channels whose per-wave row sums wait in LDS for one barrier
constexpr int SL_FINAL_THREADS = 1024;
constexpr float SL_EPS = 1e-8f;      // torch.nn.functional.cosine_similarity's eps

struct SegLossArgs {
    const float* x[SL_MAX_VIEWS];
    float* dx[SL_MAX_VIEWS];
    const int* seg[SL_MAX_VIEWS];
    const float* table[SL_MAX_VIEWS];
    int n_seg[SL_MAX_VIEWS];
    int V, C, H, W;
    float lam, beta;
    const float* d_loss;
    double* row_l1;    // [V][H]        sum over (c, w) of |a - b|
    float* row_cos;    // [V][C][H][3]  (a.b, |a|^2, |b|^2) over w
    float* loss;
};

__device__ __forceinline__ int checked_label(int s, int n_seg) { return (unsigned)s < (unsigned)n_seg ? s : -1; }

// The row's labels, range-checked: from LDS when the row fits there, else from the map again.
struct RowLabels {
    const int* s_seg;
    const int* seg;
    int n_seg;
    bool staged;
    __device__ __forceinline__ int at(int w) const { return staged ? s_seg[w] : checked_label(seg[w], n_seg); }
    __device__ __forceinline__ int4 at4(int w) const {
        if (staged) return *reinterpret_cast<const int4*>(s_seg + w);
        const int4 s = *reinterpret_cast<const int4*>(seg + w);
        return make_int4(checked_label(s.x, n_seg), checked_label(s.y, n_seg), checked_label(s.z, n_seg),
                         checked_label(s.w, n_seg));
    }
};

__device__ __forceinline__ RowLabels stage_labels(int* s_seg, const int* seg, int n_seg, int W) {
    RowLabels r{s_seg, seg, n_seg, W <= SL_SEG_LDS};
    if (r.staged) {                                    // block-uniform
        for (int w = threadIdx.x; w < W; w += SL_THREADS) s_seg[w] = checked_label(seg[w], n_seg);
        __syncthreads();
    }
    return r;
}

template <bool COS>
struct FwdAcc {
    double l1 = 0.0;                       // the loss is the correctly rounded float of the exact sum
    float dot = 0.0f, na = 0.0f, nb = 0.0f;
    __device__ __forceinline__ void add(float x, int s, const float* __restrict__ tcol, int C) {
        if (s < 0) return;
        const float t = tcol[(size_t)s * C];
        l1 += (double)fabsf(x - t);
        if (COS) {
            dot += x * t;
            na += x * x;
            nb += t * t;
        }
    }
};

template <bool VEC, bool COS>
__global__ void __launch_bounds__(SL_THREADS) k_seg_fwd(SegLossArgs a) {
    __shared__ __attribute__((aligned(16))) int s_seg[SL_SEG_LDS];
    __shared__ float s_part[SL_CCHUNK][SL_WAVES][3];
    __shared__ double s_l1[SL_WAVES];
    const int v = blockIdx.y, h = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int C = a.C, H = a.H, W = a.W;
    const float* __restrict__ table = a.table[v];
    const RowLabels lab = stage_labels(s_seg, a.seg[v] + (int64_t)h * W, a.n_seg[v], W);

    FwdAcc<COS> acc;
    for (int c0 = 0; c0 < C; c0 += SL_CCHUNK) {
        const int cn = min(SL_CCHUNK, C - c0);
        for (int cc = 0; cc < cn; ++cc) {
            const int c = c0 + cc;
            const float* __restrict__ xr = a.x[v] + ((int64_t)c * H + h) * W;
            const float* __restrict__ tcol = table + c;
            acc.dot = acc.na = acc.nb = 0.0f;
            if (VEC) {
                for (int w = tid * 4; w < W; w += SL_THREADS * 4) {
                    const float4 xv = *reinterpret_cast<const float4*>(xr + w);
                    const int4 sv = lab.at4(w);
                    acc.add(xv.x, sv.x, tcol, C);
                    acc.add(xv.y, sv.y, tcol, C);
                    acc.add(xv.z, sv.z, tcol, C);
                    acc.add(xv.w, sv.w, tcol, C);
                }
            } else {
                for (int w = tid; w < W; w += SL_THREADS) acc.add(xr[w], lab.at(w), tcol, C);
            }
            if (COS) {
                const float d = wave_sum(acc.dot), na = wave_sum(acc.na), nb = wave_sum(acc.nb);
                if (lane == 0) {
                    s_part[cc][wave][0] = d;
                    s_part[cc][wave][1] = na;
                    s_part[cc][wave][2] = nb;
                }
            }
        }
        if (COS) {
            __syncthreads();
            if (tid < cn * 3) {
                const int cc = tid / 3, k = tid - cc * 3;
                a.row_cos[(((int64_t)v * C + c0 + cc) * H + h) * 3 + k] =
                    (s_part[cc][0][k] + s_part[cc][1][k]) + (s_part[cc][2][k] + s_part[cc][3][k]);
            }
            __syncthreads();
        }
    }
    const double l1 = wave_sum(acc.l1);
    if (lane == 0) s_l1[wave] = l1;
    __syncthreads();
    if (tid == 0) a.row_l1[(int64_t)v * H + h] = (s_l1[0] + s_l1[1]) + (s_l1[2] + s_l1[3]);
}

// loss = lam * sum|a - b| / N  (+ beta * (1 - mean cos)), the row sums added in double in a fixed order.
__global__ void __launch_bounds__(SL_FINAL_THREADS) k_seg_final(SegLossArgs a, int with_cos) {
    __shared__ double s_w[2][SL_FINAL_THREADS / 64];
    const int tid = threadIdx.x;
    const int64_t rows = (int64_t)a.V * a.H, crows = rows * a.C;
    double l1 = 0.0, cs = 0.0;
    for (int64_t i = tid; i < rows; i += SL_FINAL_THREADS) l1 += a.row_l1[i];
    if (with_cos) {
        for (int64_t i = tid; i < crows; i += SL_FINAL_THREADS) {
            const float d = a.row_cos[3 * i], na = a.row_cos[3 * i + 1], nb = a.row_cos[3 * i + 2];
            cs += (double)(d / (fmaxf(sqrtf(na), SL_EPS) * fmaxf(sqrtf(nb), SL_EPS)));
        }
    }
    l1 = wave_sum(l1);
    cs = wave_sum(cs);
    if ((tid & 63) == 0) {
        s_w[0][tid >> 6] = l1;
        s_w[1][tid >> 6] = cs;
    }
    __syncthreads();
    if (tid == 0) {
        double L = 0.0, S = 0.0;
        for (int k = 0; k < SL_FINAL_THREADS / 64; ++k) {
            L += s_w[0][k];
            S += s_w[1][k];
        }
        double out = (double)a.lam * (L / ((double)crows * (double)a.W));
        if (with_cos) out += (double)a.beta * (1.0 - S / (double)crows);
        a.loss[0] = (float)out;
    }
}

// d_x = m * (sign(x - t) * ((d_loss * lam) * (1 / N))          PyTorch's mul / mean / abs backward on the GPU
//            - (d_loss * beta / (V C H)) * d cos / d a)          cos = a.b / (A B), A = max(|a|, eps), B likewise:
// d cos / d a = b / (A B) - [|a| > eps] (a.b) a / (A^3 B).  Unlabelled pixels get +0.
template <bool COS>
struct BwdCoef {
    float s1, k1 = 0.0f, k2 = 0.0f;
    __device__ __forceinline__ float at(float x, int s, const float* __restrict__ tcol, int C) const {
        if (s < 0) return 0.0f;
        const float t = tcol[(size_t)s * C];
        const float v = x - t;
        const float g = v > 0.0f ? s1 : (v < 0.0f ? -s1 : 0.0f);
        return COS ? g + (k1 * t + k2 * x) : g;
    }
};

template <bool VEC, bool COS>
__global__ void __launch_bounds__(SL_THREADS) k_seg_bwd(SegLossArgs a) {
    __shared__ __attribute__((aligned(16))) int s_seg[SL_SEG_LDS];
    const int v = blockIdx.y, h = blockIdx.x, tid = threadIdx.x;
    const int C = a.C, H = a.H, W = a.W;
    const float* __restrict__ table = a.table[v];
    const RowLabels lab = stage_labels(s_seg, a.seg[v] + (int64_t)h * W, a.n_seg[v], W);
    const int64_t rows = (int64_t)a.V * C * H;
    const float g0 = a.d_loss[0];
    BwdCoef<COS> k;
    k.s1 = (g0 * a.lam) * (1.0f / (float)(rows * W));
    const float gc = COS ? g0 * a.beta / (float)rows : 0.0f;
    for (int c = 0; c < C; ++c) {
        const int64_t row = ((int64_t)c * H + h) * W;
        const float* __restrict__ xr = a.x[v] + row;
        float* __restrict__ dr = a.dx[v] + row;
        const float* __restrict__ tcol = table + c;
        if (COS) {
            const float* rc = a.row_cos + (((int64_t)v * C + c) * H + h) * 3;
            const float ra = sqrtf(rc[1]), rb = sqrtf(rc[2]);
            const float A = fmaxf(ra, SL_EPS), B = fmaxf(rb, SL_EPS);
            k.k1 = -gc / (A * B);
            k.k2 = ra > SL_EPS ? (gc * rc[0] / (A * B)) / (A * A) : 0.0f;
        }
        if (VEC) {
            for (int w = tid * 4; w < W; w += SL_THREADS * 4) {
                const float4 xv = *reinterpret_cast<const float4*>(xr + w);
                const int4 sv = lab.at4(w);
                *reinterpret_cast<float4*>(dr + w) = make_float4(k.at(xv.x, sv.x, tcol, C), k.at(xv.y, sv.y, tcol, C),
                                                                 k.at(xv.z, sv.z, tcol, C), k.at(xv.w, sv.w, tcol, C));
            }
        } else {
            for (int w = tid; w < W; w += SL_THREADS) dr[w] = k.at(xr[w], lab.at(w), tcol, C);
        }
    }
}

// the workspace carved into a's row sums; returns its bytes
size_t carve(SegLossArgs& a, void* base, int64_t V, int64_t C, int64_t H) {
    lsr::Carver c(base);
    a.row_l1 = c.take<double>((size_t)(V * H));
    a.row_cos = c.take<float>((size_t)(V * C * H) * 3);
    return c.total();
}

bool sizes_ok(int32_t V, int32_t C, int32_t H, int32_t W) {
    return V >= 1 && V <= SL_MAX_VIEWS && C >= 1 && H >= 1 && W >= 1;
}

// Everything both entry points check and fill; vec: every row of every tensor starts 16-byte aligned.
int seg_args(const std::string& what, int32_t V, int32_t C, int32_t H, int32_t W, const lsr_seg_view* views,
             bool backward, float lam, float beta, bool need_ws, void* workspace, SegLossArgs& a, bool& vec) {
    if (!sizes_ok(V, C, H, W)) return lsr::fail(LSR_EINVAL, what + ": 1 <= V <= 8 and C, H, W >= 1 required");
    if (!views) return lsr::fail(LSR_EINVAL, what + ": views required");
    if (need_ws && !workspace) return lsr::fail(LSR_EINVAL, what + ": workspace required");
    if (need_ws && !aligned16(workspace)) return lsr::fail(LSR_EINVAL, what + ": the workspace must be 16-byte aligned");
    a = SegLossArgs{};
    vec = W % 4 == 0;
    for (int v = 0; v < V; ++v) {
        const lsr_seg_view& s = views[v];
        if (s.n_seg < 1) return lsr::fail(LSR_EINVAL, what + ": n_seg >= 1 required");
        if (!s.image || !s.seg || !s.table) return lsr::fail(LSR_EINVAL, what + ": null image, seg or table");
        if (backward && !s.d_image) return lsr::fail(LSR_EINVAL, what + ": null gradient image");
        a.x[v] = s.image;
        a.dx[v] = s.d_image;
        a.seg[v] = s.seg;
        a.table[v] = s.table;
        a.n_seg[v] = s.n_seg;
        vec = vec && aligned16(s.image) && aligned16(s.seg) && (!backward || aligned16(s.d_image));
    }
    a.V = V; a.C = C; a.H = H; a.W = W;
    a.lam = lam; a.beta = beta;
    carve(a, workspace, V, C, H);
    return LSR_OK;
}

}  // namespace

extern "C" {

int64_t lsr_seg_loss_workspace_bytes(int32_t V, int32_t C, int32_t H, int32_t W) {
    if (!sizes_ok(V, C, H, W)) {
        lsr::fail(LSR_EINVAL, "lsr_seg_loss_workspace_bytes: 1 <= V <= 8 and C, H, W >= 1 required");
        return -1;
    }
    SegLossArgs a{};
    return (int64_t)carve(a, nullptr, V, C, H);
}

int lsr_seg_loss_views(int32_t V, int32_t C, int32_t H, int32_t W, const lsr_seg_view* views, float lam, float beta,
                       int32_t with_cos, float* loss, void* workspace, void* stream) {
    SegLossArgs a;
    bool vec;
    if (int rc = seg_args("lsr_seg_loss_views", V, C, H, W, views, false, lam, beta, true, workspace, a, vec))
        return rc;
    if (!loss) return lsr::fail(LSR_EINVAL, "lsr_seg_loss_views: loss required");
    a.loss = loss;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const dim3 grid(H, V), block(SL_THREADS);
    if (vec && with_cos) hipLaunchKernelGGL((k_seg_fwd<true, true>), grid, block, 0, st, a);
    else if (vec) hipLaunchKernelGGL((k_seg_fwd<true, false>), grid, block, 0, st, a);
    else if (with_cos) hipLaunchKernelGGL((k_seg_fwd<false, true>), grid, block, 0, st, a);
    else hipLaunchKernelGGL((k_seg_fwd<false, false>), grid, block, 0, st, a);
    hipLaunchKernelGGL(k_seg_final, dim3(1), dim3(SL_FINAL_THREADS), 0, st, a, with_cos ? 1 : 0);
    return launched("seg loss");
}

int lsr_seg_loss_views_backward(int32_t V, int32_t C, int32_t H, int32_t W, const lsr_seg_view* views, float lam,
                                float beta, int32_t with_cos, const float* d_loss, void* workspace, void* stream) {
    SegLossArgs a;
    bool vec;
    if (int rc = seg_args("lsr_seg_loss_views_backward", V, C, H, W, views, true, lam, beta, with_cos != 0,
                          workspace, a, vec))
        return rc;
    if (!d_loss) return lsr::fail(LSR_EINVAL, "lsr_seg_loss_views_backward: d_loss required");
    a.d_loss = d_loss;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const dim3 grid(H, V), block(SL_THREADS);
    if (vec && with_cos) hipLaunchKernelGGL((k_seg_bwd<true, true>), grid, block, 0, st, a);
    else if (vec) hipLaunchKernelGGL((k_seg_bwd<true, false>), grid, block, 0, st, a);
    else if (with_cos) hipLaunchKernelGGL((k_seg_bwd<false, true>), grid, block, 0, st, a);
    else hipLaunchKernelGGL((k_seg_bwd<false, false>), grid, block, 0, st, a);
    return launched("seg loss backward");
}

}  // extern "C"
