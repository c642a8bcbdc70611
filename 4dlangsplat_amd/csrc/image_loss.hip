// image_loss.hip -- the photometric loss of the training loop, l1_loss + lambda_dssim * (1 - ssim)
// (include/lsr_train.h: lsr_image_loss_views / _backward; train.py:284,335-337, utils/loss_utils.py:29-69
// with window_size 11, utils/image_utils.py:17-38 for the squared error PSNR needs).
//
// SSIM is a stencil: the five windowed statistics E[x], E[y], E[x^2], E[y^2], E[xy] are zero-padded
// correlations with one separable 11-tap Gaussian.  A workgroup owns a 64 x 16 pixel tile of one plane of
// one view: it stages the tile with its 5-pixel halo of x and y in LDS (zeros outside the image), runs the
// horizontal pass over the 26 halo rows, then the vertical pass, and evaluates ssim_map, |x - y| and
// (x - y)^2 per pixel.  The forward also leaves the three per-pixel partial derivatives of ssim_map
// (towards mu1, E[x^2], E[xy]) in the workspace; the backward is the same stencil over those three maps
// (the window is symmetric and the padding zero, so the transposed correlation is the correlation),
// gather-form: every thread writes its own gradient elements once, no atomics anywhere.
//
// A tile row is 64 floats, one wave: in both passes lane l reads word base + l of an LDS row, so every
// ds_read_b32 has its two 32-lane halves on 32 distinct banks (conflict-free without padding; the row
// strides need no particular residue).  Every sum is added in a fixed order (lanes by butterfly, waves,
// blocks and views in index order, the cross-block sums in double): two calls give the same bits.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>

#include "../../include/lsr.h"
#include "../../include/lsr_train.h"
#include "lsr_host.h"
#include "lsr_wave.h"

namespace {

using lsr::launched;
using lsr::wave_sum;

constexpr int IL_MAX_VIEWS = 8, IL_THREADS = 256, IL_WAVES = IL_THREADS / 64;
constexpr int IL_R = 5, IL_TAPS = 2 * IL_R + 1;            // the 11-tap window
constexpr int IL_TW = 64, IL_TH = 16;                      // the tile: one wave per row, 4 rows per thread
constexpr int IL_ROWS = IL_TH / IL_WAVES;                  // output rows per thread (consecutive)
constexpr int IL_HW = IL_TW + 2 * IL_R, IL_HH = IL_TH + 2 * IL_R;   // 74 x 26 with the halo
constexpr int IL_FINAL_THREADS = 1024;
constexpr float IL_C1 = 0.01f * 0.01f, IL_C2 = 0.03f * 0.03f;

// gaussian(11, 1.5) of utils/loss_utils.py:29-31 as float32 evaluates it: exp(-(i - 5)^2 / 4.5) over its
// float32 sum (image_loss.WINDOW_11 holds the same values; tests/test_image_loss.py compares both with the
// fixture's).
__device__ __forceinline__ constexpr float tap(int k) {
    constexpr float w[IL_TAPS] = {0x1.0d956cp-10f, 0x1.f1fe02p-8f, 0x1.26eb18p-5f, 0x1.bff0fep-4f,
                                  0x1.b43c3ep-3f,  0x1.10656p-2f,  0x1.b43c3ep-3f, 0x1.bff0fep-4f,
                                  0x1.26eb18p-5f,  0x1.f1fe02p-8f, 0x1.0d956cp-10f};
    return w[k];
}

struct ImageLossArgs {
    const float* x[IL_MAX_VIEWS];
    float* dx[IL_MAX_VIEWS];
    const float* gt;
    int64_t gt_stride;        // floats between the views' ground truths
    int V, C, H, W;
    int tiles_x, tiles_y;
    double* partial;          // [V][C][tiles][3]  block sums of |x - y|, ssim_map, (x - y)^2
    float* maps;              // [3][V][C][H][W]   d ssim_map / d (mu1, E[x^2], E[xy])
    int64_t map_stride;       // V C H W
    float* stats;             // [V][3]
    float* totals;            // [2]
    const float* d_l1;
    const float* d_ssim;
};

// Stage the 26 x 74 halo tile of `src` (an [H, W] plane) whose interior starts at (h0, w0); zeros outside.
// Every lane's loads (8 of them) are issued before the first LDS store, so that they are in flight together.
__device__ __forceinline__ void stage(float (*s)[IL_HW], const float* __restrict__ src, int h0, int w0, int H, int W) {
    constexpr int N = IL_HH * IL_HW, ITERS = (N + IL_THREADS - 1) / IL_THREADS;
    float v[ITERS];
#pragma unroll
    for (int it = 0; it < ITERS; ++it) {
        const int i = threadIdx.x + it * IL_THREADS;
        const int r = i / IL_HW, c = i - r * IL_HW;
        const int h = h0 - IL_R + r, w = w0 - IL_R + c;
        v[it] = (i < N && (unsigned)h < (unsigned)H && (unsigned)w < (unsigned)W) ? src[(int64_t)h * W + w] : 0.0f;
    }
#pragma unroll
    for (int it = 0; it < ITERS; ++it) {
        const int i = threadIdx.x + it * IL_THREADS;
        if (i < N) (&s[0][0])[i] = v[it];
    }
}

// The vertical pass of one statistic for this thread's IL_ROWS consecutive rows: 14 LDS reads for 4 outputs.
__device__ __forceinline__ void vertical(const float (*h)[IL_TW], int row0, int col, float out[IL_ROWS]) {
#pragma unroll
    for (int i = 0; i < IL_ROWS; ++i) out[i] = 0.0f;
#pragma unroll
    for (int j = 0; j < IL_ROWS + IL_TAPS - 1; ++j) {
        const float v = h[row0 + j][col];
#pragma unroll
        for (int i = 0; i < IL_ROWS; ++i)
            if (j - i >= 0 && j - i < IL_TAPS) out[i] = fmaf(tap(j - i), v, out[i]);
    }
}

__global__ void __launch_bounds__(IL_THREADS) k_image_loss_fwd(ImageLossArgs a) {
    __shared__ float s_x[IL_HH][IL_HW], s_y[IL_HH][IL_HW];
    __shared__ float s_h[5][IL_HH][IL_TW];
    __shared__ double s_red[IL_WAVES][3];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int tile = blockIdx.x, ty = tile / a.tiles_x, tx = tile - ty * a.tiles_x;
    const int plane = blockIdx.y, v = plane / a.C, c = plane - v * a.C;
    const int H = a.H, W = a.W, h0 = ty * IL_TH, w0 = tx * IL_TW;
    const int64_t plane_off = (int64_t)c * H * W;
    stage(s_x, a.x[v] + plane_off, h0, w0, H, W);
    stage(s_y, a.gt + (int64_t)v * a.gt_stride + plane_off, h0, w0, H, W);
    __syncthreads();

    for (int r = wave; r < IL_HH; r += IL_WAVES) {
        float mx = 0.0f, my = 0.0f, xx = 0.0f, yy = 0.0f, xy = 0.0f;
#pragma unroll
        for (int k = 0; k < IL_TAPS; ++k) {
            const float x = s_x[r][lane + k], y = s_y[r][lane + k], wk = tap(k);
            mx = fmaf(wk, x, mx);
            my = fmaf(wk, y, my);
            xx = fmaf(wk, x * x, xx);
            yy = fmaf(wk, y * y, yy);
            xy = fmaf(wk, x * y, xy);
        }
        s_h[0][r][lane] = mx;
        s_h[1][r][lane] = my;
        s_h[2][r][lane] = xx;
        s_h[3][r][lane] = yy;
        s_h[4][r][lane] = xy;
    }
    __syncthreads();

    const int row0 = wave * IL_ROWS, w = w0 + lane;
    float mu1[IL_ROWS], mu2[IL_ROWS], e11[IL_ROWS], e22[IL_ROWS], e12[IL_ROWS];
    vertical(s_h[0], row0, lane, mu1);
    vertical(s_h[1], row0, lane, mu2);
    vertical(s_h[2], row0, lane, e11);
    vertical(s_h[3], row0, lane, e22);
    vertical(s_h[4], row0, lane, e12);

    float l1 = 0.0f, ss = 0.0f, sq = 0.0f;
    float* __restrict__ m0 = a.maps + ((int64_t)plane * H) * W;
#pragma unroll
    for (int i = 0; i < IL_ROWS; ++i) {
        const int h = h0 + row0 + i;
        if (h < H && w < W) {
            const float m1 = mu1[i], m2 = mu2[i];
            const float m12 = m1 * m2;
            const float s1 = e11[i] - m1 * m1, s2 = e22[i] - m2 * m2, s12 = e12[i] - m12;
            const float A1 = 2.0f * m12 + IL_C1, A2 = 2.0f * s12 + IL_C2;
            const float B1 = m1 * m1 + m2 * m2 + IL_C1, B2 = s1 + s2 + IL_C2;
            const float inv = 1.0f / (B1 * B2);
            const float m = (A1 * A2) * inv;
            // d m / d mu1 with E[x^2] and E[xy] held (s1 and s12 move with mu1), d m / d E[x^2], d m / d E[xy]
            const float d_mu = 2.0f * m2 * (A2 - A1) * inv - 2.0f * m1 * m * (1.0f / B1 - 1.0f / B2);
            const float d_e11 = -m / B2;
            const float d_e12 = 2.0f * A1 * inv;
            const int64_t e = (int64_t)h * W + w;
            m0[e] = d_mu;
            m0[a.map_stride + e] = d_e11;
            m0[2 * a.map_stride + e] = d_e12;
            const float d = s_x[row0 + i + IL_R][lane + IL_R] - s_y[row0 + i + IL_R][lane + IL_R];
            l1 += fabsf(d);
            sq += d * d;
            ss += m;
        }
    }
    const double r0 = wave_sum((double)l1), r1 = wave_sum((double)ss), r2 = wave_sum((double)sq);
    if (lane == 0) {
        s_red[wave][0] = r0;
        s_red[wave][1] = r1;
        s_red[wave][2] = r2;
    }
    __syncthreads();
    if (tid < 3) {
        a.partial[((int64_t)plane * gridDim.x + tile) * 3 + tid] =
            (s_red[0][tid] + s_red[1][tid]) + (s_red[2][tid] + s_red[3][tid]);
    }
}

// stats[v] = the view's three means, totals = mean |x - y| and mean ssim_map over all views: the block sums
// added in double in a fixed order by one block.
__global__ void __launch_bounds__(IL_FINAL_THREADS) k_image_loss_final(ImageLossArgs a) {
    __shared__ double s_w[IL_FINAL_THREADS / 64][3];
    const int tid = threadIdx.x;
    const int64_t per_view = (int64_t)a.C * a.tiles_x * a.tiles_y;
    const double n_view = (double)a.C * (double)a.H * (double)a.W;
    double t0 = 0.0, t1 = 0.0;
    for (int v = 0; v < a.V; ++v) {
        const double* __restrict__ p = a.partial + (int64_t)v * per_view * 3;
        double s0 = 0.0, s1 = 0.0, s2 = 0.0;
        for (int64_t i = tid; i < per_view; i += IL_FINAL_THREADS) {
            s0 += p[3 * i];
            s1 += p[3 * i + 1];
            s2 += p[3 * i + 2];
        }
        s0 = wave_sum(s0);
        s1 = wave_sum(s1);
        s2 = wave_sum(s2);
        if ((tid & 63) == 0) {
            s_w[tid >> 6][0] = s0;
            s_w[tid >> 6][1] = s1;
            s_w[tid >> 6][2] = s2;
        }
        __syncthreads();
        if (tid == 0) {
            double S[3] = {0.0, 0.0, 0.0};
            for (int k = 0; k < IL_FINAL_THREADS / 64; ++k)
                for (int j = 0; j < 3; ++j) S[j] += s_w[k][j];
            for (int j = 0; j < 3; ++j) a.stats[3 * v + j] = (float)(S[j] / n_view);
            t0 += S[0];
            t1 += S[1];
        }
        __syncthreads();
    }
    if (tid == 0) {
        a.totals[0] = (float)(t0 / (n_view * (double)a.V));
        a.totals[1] = (float)(t1 / (n_view * (double)a.V));
    }
}

// d_x = sign(x - y) * (d_l1 * (1 / N))                                  lsr_l1_loss_views_backward's term, bit for bit
//     + (d_ssim * (1 / N)) * (conv(P_mu) + 2 x conv(P_11) + y conv(P_12))
// with conv the forward's zero-padded correlation and P the forward's maps.  Without an ssim gradient (NULL,
// or a 0 behind it) only the first term is computed and the maps are not read.
__global__ void __launch_bounds__(IL_THREADS) k_image_loss_bwd(ImageLossArgs a) {
    __shared__ float s_p[3][IL_HH][IL_HW];
    __shared__ float s_h[3][IL_HH][IL_TW];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int tile = blockIdx.x, ty = tile / a.tiles_x, tx = tile - ty * a.tiles_x;
    const int plane = blockIdx.y, v = plane / a.C, c = plane - v * a.C;
    const int H = a.H, W = a.W, h0 = ty * IL_TH, w0 = tx * IL_TW;
    const int64_t plane_off = (int64_t)c * H * W;
    const float* __restrict__ x = a.x[v] + plane_off;
    const float* __restrict__ y = a.gt + (int64_t)v * a.gt_stride + plane_off;
    float* __restrict__ dx = a.dx[v] + plane_off;
    const float rn = 1.0f / (float)((int64_t)a.V * a.C * H * W);
    const float g1 = a.d_l1 ? a.d_l1[0] * rn : 0.0f;
    const float gs_in = a.d_ssim ? a.d_ssim[0] : 0.0f;
    const bool with_ssim = gs_in != 0.0f;                  // block-uniform (grid-uniform)
    const float gs = gs_in * rn;
    const int row0 = wave * IL_ROWS, w = w0 + lane;

    float c0[IL_ROWS], c1[IL_ROWS], c2[IL_ROWS];
    if (with_ssim) {
        const float* __restrict__ m0 = a.maps + ((int64_t)plane * H) * W;
        for (int k = 0; k < 3; ++k) stage(s_p[k], m0 + k * a.map_stride, h0, w0, H, W);
        __syncthreads();
        for (int r = wave; r < IL_HH; r += IL_WAVES) {
            float q0 = 0.0f, q1 = 0.0f, q2 = 0.0f;
#pragma unroll
            for (int k = 0; k < IL_TAPS; ++k) {
                const float wk = tap(k);
                q0 = fmaf(wk, s_p[0][r][lane + k], q0);
                q1 = fmaf(wk, s_p[1][r][lane + k], q1);
                q2 = fmaf(wk, s_p[2][r][lane + k], q2);
            }
            s_h[0][r][lane] = q0;
            s_h[1][r][lane] = q1;
            s_h[2][r][lane] = q2;
        }
        __syncthreads();
        vertical(s_h[0], row0, lane, c0);
        vertical(s_h[1], row0, lane, c1);
        vertical(s_h[2], row0, lane, c2);
    }
#pragma unroll
    for (int i = 0; i < IL_ROWS; ++i) {
        const int h = h0 + row0 + i;
        if (h < H && w < W) {
            const int64_t e = (int64_t)h * W + w;
            const float xv = x[e], yv = y[e];
            const float d = xv - yv;
            float g = g1 * (d > 0.0f ? 1.0f : (d < 0.0f ? -1.0f : 0.0f));
            if (with_ssim) g += gs * fmaf(yv, c2[i], fmaf(2.0f * xv, c1[i], c0[i]));
            dx[e] = g;
        }
    }
}

// the workspace carved into a's block sums and maps; returns its bytes
size_t carve(ImageLossArgs& a, void* base, int64_t V, int64_t C, int64_t H, int64_t W) {
    const int64_t tiles = ((W + IL_TW - 1) / IL_TW) * ((H + IL_TH - 1) / IL_TH);
    lsr::Carver c(base);
    a.partial = c.take<double>((size_t)(V * C * tiles) * 3);
    a.maps = c.take<float>((size_t)(V * C * H * W) * 3);
    return c.total();
}

bool sizes_ok(int32_t V, int32_t C, int32_t H, int32_t W) {
    return V >= 1 && V <= IL_MAX_VIEWS && C >= 1 && H >= 1 && W >= 1 && (int64_t)V * C <= 65535;
}

int image_loss_args(const std::string& what, int32_t V, int32_t C, int32_t H, int32_t W, const float* const* images,
                    const float* gt, int64_t gt_view_stride, const void* workspace, ImageLossArgs& a) {
    if (!sizes_ok(V, C, H, W))
        return lsr::fail(LSR_EINVAL, what + ": 1 <= V <= 8, C, H, W >= 1 and V C <= 65535 required");
    if (!images || !gt) return lsr::fail(LSR_EINVAL, what + ": images and gt required");
    if (gt_view_stride < (int64_t)C * H * W && V > 1)
        return lsr::fail(LSR_EINVAL, what + ": gt_view_stride >= C H W required");
    if (!workspace) return lsr::fail(LSR_EINVAL, what + ": workspace required");
    if (!lsr::aligned16(workspace))
        return lsr::fail(LSR_EINVAL, what + ": the workspace must be 16-byte aligned");
    a = ImageLossArgs{};
    for (int v = 0; v < V; ++v) {
        if (!images[v]) return lsr::fail(LSR_EINVAL, what + ": null image");
        a.x[v] = images[v];
    }
    a.gt = gt;
    a.gt_stride = gt_view_stride;
    a.V = V; a.C = C; a.H = H; a.W = W;
    a.tiles_x = (W + IL_TW - 1) / IL_TW;
    a.tiles_y = (H + IL_TH - 1) / IL_TH;
    carve(a, const_cast<void*>(workspace), V, C, H, W);
    a.map_stride = (int64_t)V * C * H * W;
    return LSR_OK;
}

}  // namespace

extern "C" {

int64_t lsr_image_loss_workspace_bytes(int32_t V, int32_t C, int32_t H, int32_t W) {
    if (!sizes_ok(V, C, H, W)) {
        lsr::fail(LSR_EINVAL, "lsr_image_loss_workspace_bytes: 1 <= V <= 8, C, H, W >= 1 and V C <= 65535 required");
        return -1;
    }
    ImageLossArgs a{};
    return (int64_t)carve(a, nullptr, V, C, H, W);
}

int lsr_image_loss_views(int32_t V, int32_t C, int32_t H, int32_t W, const float* const* images, const float* gt,
                         int64_t gt_view_stride, float* stats, float* totals, void* workspace, void* stream) {
    ImageLossArgs a;
    if (int rc = image_loss_args("lsr_image_loss_views", V, C, H, W, images, gt, gt_view_stride, workspace, a))
        return rc;
    if (!stats || !totals) return lsr::fail(LSR_EINVAL, "lsr_image_loss_views: stats and totals required");
    a.stats = stats;
    a.totals = totals;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(k_image_loss_fwd, dim3(a.tiles_x * a.tiles_y, V * C), dim3(IL_THREADS), 0, st, a);
    hipLaunchKernelGGL(k_image_loss_final, dim3(1), dim3(IL_FINAL_THREADS), 0, st, a);
    return launched("image loss");
}

int lsr_image_loss_views_backward(int32_t V, int32_t C, int32_t H, int32_t W, const float* const* images,
                                  const float* gt, int64_t gt_view_stride, const float* d_l1, const float* d_ssim,
                                  float* const* d_images, const void* workspace, void* stream) {
    ImageLossArgs a;
    if (int rc = image_loss_args("lsr_image_loss_views_backward", V, C, H, W, images, gt, gt_view_stride, workspace,
                                 a))
        return rc;
    if (!d_images) return lsr::fail(LSR_EINVAL, "lsr_image_loss_views_backward: d_images required");
    for (int v = 0; v < V; ++v) {
        if (!d_images[v]) return lsr::fail(LSR_EINVAL, "lsr_image_loss_views_backward: null gradient image");
        a.dx[v] = d_images[v];
    }
    a.d_l1 = d_l1;
    a.d_ssim = d_ssim;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(k_image_loss_bwd, dim3(a.tiles_x * a.tiles_y, V * C), dim3(IL_THREADS), 0, st, a);
    return launched("image loss backward");
}

}  // extern "C"
