// autoencoder.hip -- the language autoencoder (include/lsr_autoencoder.h): eval-mode encode and
// reconstruction loss, and one training step, every product on the exact f32-input MFMA
// (v_mfma_f32_16x16x4_f32).  DESIGN.md 4.15.
//
// The layer boundary is the kernel boundary.  A block of 4 waves owns AE_BM = 64 rows (in training: the
// whole batch) and a slab of AE_BN = 32 columns; wave w the rows 16 w .. 16 w + 15 as two MFMA tiles.
// What a layer hands on is its raw pre-activation; the consumer applies BatchNorm's (x - mean) * scale + bias and
// the ReLU while it stages the operand (load_act), forward and backward alike.
//
// k_ae_fwd<EPI>     H = act(A) . W^T + b.  K runs in blocks of 32, global -> registers -> LDS (rows padded
//                   to 36 floats), the next block's loads in flight while this one is multiplied: lsr_dense.h's
//                   dense_k_loop, which k_ae_dx runs too and the video decoder's layers.  The MFMA
//                   is a k-ordered fmaf chain: a chain ends after 4 k blocks (128 terms) and the chains are
//                   added in order, which keeps the rounding of a 4096-term sum near a blocked sum's.
//                     STATS  the layer feeds a BatchNorm in train mode: the slab's column mean and biased
//                            variance over the batch (two passes over the accumulators), the consumer's
//                            scale = weight / std with the mean and the bias as this step read it, 1 / std
//                            for the backward, the running statistics
//                     NORM   the latent: also u = z / |z| (the latent fits one slab)
//                     EVAL   the reconstruction in eval mode: nothing feature_dim-wide is stored; per row
//                            and slab the float64 sums of y^2, y x and x^2
// k_ae_loss         one block per row: out = y / |y|, the row's sum of (out - x)^2 and cosine, and dL/dy
// k_ae_loss_sum     the rows' sums in row order -> (l2, cos)
// k_ae_dx<EPI>      dA = dH . W, then through what produced A:
//                     RELU   dHprev = dA [Hprev > 0]
//                     BN     ReLU and BatchNorm's backward (the column sums over the batch), Adam on the
//                            BatchNorm's weight and bias
//                     NORM   through u = z / |z|
// k_ae_dw_adam      dW = dH^T . act(A) for a 64 x 32 tile of W (the sum over the batch is the MFMA's k),
//                     Adam on that tile; the k tile 0 also sums the bias gradient and updates the bias.
//                     A layer's k_ae_dx runs before its k_ae_dw_adam: it reads W before the update.
// k_ae_bn_eval      eval mode: weight / std of every BatchNorm from its running variance
// k_ae_eval_rows / k_ae_eval_sum   per row the slabs' sums in slab order, then the rows in a fixed tree
// No atomics anywhere: two calls from the same state give the same bits.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <string>

#include "../../include/lsr.h"
#include "../../include/lsr_autoencoder.h"
#include "lsr_dense.h"
#include "lsr_host.h"
#include "lsr_mfma.h"
#include "lsr_wave.h"

namespace {

using lsr::f32x4;
using lsr::load4;
using lsr::mfma4;
using lsr::rows_vec;
using lsr::sum16;

constexpr int AE_BM = 64, AE_BN = 32, AE_BK = lsr::DENSE_BK;
constexpr int AE_LDK = lsr::DENSE_LDK;            // LDS row stride in floats (16-byte aligned rows)
constexpr int AE_THREADS = lsr::DENSE_THREADS;
constexpr int AE_CHAIN = 4;                       // k blocks of one fmaf chain of the layer kernels: 128 terms
constexpr int AE_DW_BN = 64, AE_DW_LDN = AE_DW_BN + 4;   // k_ae_dw_adam: rows of W of one block
constexpr int AE_L = LSR_AE_MAX_LAYERS;
constexpr float BN_EPS = 1e-5f, BN_MOMENTUM = 0.1f, COS_EPS = 1e-8f;
static_assert(AE_BM == LSR_AE_MAX_BATCH, "one block holds the whole batch");
static_assert(LSR_AE_MAX_LATENT <= AE_BN && LSR_AE_MAX_LATENT <= AE_BK, "the latent fits one slab and one k block");
static_assert(LSR_AE_MAX_WIDTH <= 16 * AE_THREADS, "k_ae_loss keeps a row in 16 registers per thread");

enum { PRO_NONE = 0, PRO_RELU = 1, PRO_BN = 2 };
enum { EPI_PLAIN = 0, EPI_STATS = 1, EPI_NORM = 2, EPI_EVAL = 3 };
enum { DX_RELU = 0, DX_BN = 1, DX_NORM = 2 };

// an operand [rows, width] as its producer stored it, and what turns it into the consumer's input
struct Act {
    const float* X;
    const float* scale;   // PRO_BN: [width] each: relu((x - mean) * scale + beta), scale = weight / std
    const float* mean;
    const float* beta;
    int64_t rows;
    int32_t width, pro, vec;
};

struct Hyper {            // Adam: p -= step * m / (sqrt(v) / sqrt_bc2 + eps)
    float step, w1, b2, w2, sqrt_bc2, eps;
};

struct Moments {          // a parameter tensor with Adam's moments
    float *p, *m, *v;
};

__device__ __forceinline__ void adam(const Moments& t, int64_t i, float g, const Hyper& h) {
    float m = t.m[i], v = t.v[i];
    m = m + (g - m) * h.w1;
    v = v * h.b2 + (h.w2 * g) * g;
    t.m[i] = m;
    t.v[i] = v;
    t.p[i] = t.p[i] - h.step * (m / (sqrtf(v) / h.sqrt_bc2 + h.eps));
}

__device__ __forceinline__ float relu(float t) { return t < 0.f ? 0.f : t; }   // a NaN stays one

__device__ __forceinline__ f32x4 load_act(const Act& a, int64_t row, int k) {
    f32x4 v = load4(a.X, row, a.rows, k, a.width, a.vec != 0);
    if (a.pro == PRO_NONE || row >= a.rows) return v;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        if (k + r >= a.width) continue;
        float t = v[r];
        if (a.pro == PRO_BN) t = (t - a.mean[k + r]) * a.scale[k + r] + a.beta[k + r];
        v[r] = relu(t);
    }
    return v;
}

// v[tn]: a lane's sum over its rows of column 16 tn + c -> the sum over the block's 64 rows, in every
// thread: the lane groups by butterfly, the waves in order.  red: 4 x AE_BN floats of LDS.
__device__ __forceinline__ void col_reduce(float (&v)[2], float* red, int wave, int c, int g) {
#pragma unroll
    for (int tn = 0; tn < 2; ++tn) {
        v[tn] += __shfl_xor(v[tn], 16);
        v[tn] += __shfl_xor(v[tn], 32);
    }
    __syncthreads();
    if (g == 0) {
        red[wave * AE_BN + c] = v[0];
        red[wave * AE_BN + 16 + c] = v[1];
    }
    __syncthreads();
#pragma unroll
    for (int tn = 0; tn < 2; ++tn) {
        const int e = 16 * tn + c;
        v[tn] = ((red[e] + red[AE_BN + e]) + red[2 * AE_BN + e]) + red[3 * AE_BN + e];
    }
}

// The layer kernels' sum over k in two levels: part, the fmaf chain of the MFMAs, ends after AE_CHAIN k blocks
// and at the last one, and the chains are added in order onto tot (which starts as the bias, or zero).
__device__ __forceinline__ void chain_fold(int k0, int K, f32x4 (&part)[2], f32x4 (&tot)[2]) {
    if ((k0 / AE_BK) % AE_CHAIN == AE_CHAIN - 1 || k0 + AE_BK >= K) {
#pragma unroll
        for (int tn = 0; tn < 2; ++tn) {
            tot[tn] += part[tn];
            part[tn] = f32x4{0.f, 0.f, 0.f, 0.f};
        }
    }
}

struct FwdArgs {
    Act in;
    const float* W;       // [N, K]
    const float* bias;    // [N]
    float* H;             // [M, N] (EPI_EVAL: unused; EPI_NORM: may be null)
    int32_t N, vec_w;
    // EPI_STATS: the BatchNorm this layer feeds
    const float *gamma, *beta;
    float *o_scale, *o_beta, *o_mean, *o_rstd, *run_mean, *run_var;   // o_beta: the bias as this step read it
    int64_t* count;
    float* U;             // EPI_NORM: [M, N]
    const float* X;       // EPI_EVAL: [M, N]
    double* partial;      // EPI_EVAL: [slabs][3][M]
};

template <int EPI>
__global__ void __launch_bounds__(AE_THREADS) k_ae_fwd(const FwdArgs a) {
    __shared__ __attribute__((aligned(16))) float lds[(AE_BM + AE_BN) * AE_LDK];
    float* As = lds;
    float* Ws = lds + AE_BM * AE_LDK;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, c = lane & 15, g = lane >> 4;
    const int64_t M = a.in.rows, m0 = (int64_t)blockIdx.y * AE_BM;
    const int n0 = blockIdx.x * AE_BN, K = a.in.width, N = a.N;
    const bool vw = a.vec_w != 0;

    f32x4 part[1][2] = {{f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}}}, tot[2];
#pragma unroll
    for (int tn = 0; tn < 2; ++tn) {
        const int col = n0 + 16 * tn + c;
        const float b = col < N ? a.bias[col] : 0.f;
        tot[tn] = f32x4{b, b, b, b};
    }
    // the 64 x 32 activation tile (2 float4 per thread) and the 32 x 32 weight tile (1)
    lsr::dense_k_loop<2, 1>(
        K, As, Ws, [=](int row, int k0, int k) { return load_act(a.in, m0 + row, k0 + k); },
        [=](int row, int k0, int k) { return load4(a.W, n0 + row, N, k0 + k, K, vw); },
        [&](int k0) {
            lsr::dense_tile_mma(As, Ws, 16 * wave, 0, k0, K, part);
            chain_fold(k0, K, part[0], tot);
        });
    const f32x4(&acc)[2] = tot;

    // lane (c, g), register r of tile tn: row m0 + 16 wave + 4 g + r, column n0 + 16 tn + c
    const int64_t row0 = m0 + 16 * wave + 4 * g;
    if constexpr (EPI != EPI_EVAL) {
        if (a.H) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                if (row0 + r >= M) continue;
#pragma unroll
                for (int tn = 0; tn < 2; ++tn) {
                    const int col = n0 + 16 * tn + c;
                    if (col < N) a.H[(row0 + r) * N + col] = acc[tn][r];
                }
            }
        }
    }
    if constexpr (EPI == EPI_STATS) {
        __syncthreads();                                   // every wave is done with the operand tiles
        float* red = lds;
        const float inv_m = 1.f / (float)M;
        float mean[2], var[2];
#pragma unroll
        for (int tn = 0; tn < 2; ++tn) {
            mean[tn] = 0.f;
#pragma unroll
            for (int r = 0; r < 4; ++r)
                if (row0 + r < M) mean[tn] += acc[tn][r];
        }
        col_reduce(mean, red, wave, c, g);
#pragma unroll
        for (int tn = 0; tn < 2; ++tn) {
            mean[tn] *= inv_m;
            var[tn] = 0.f;
#pragma unroll
            for (int r = 0; r < 4; ++r)
                if (row0 + r < M) {
                    const float d = acc[tn][r] - mean[tn];
                    var[tn] += d * d;
                }
        }
        col_reduce(var, red, wave, c, g);
        if (wave == 0 && g == 0) {
#pragma unroll
            for (int tn = 0; tn < 2; ++tn) {
                const int col = n0 + 16 * tn + c;
                if (col >= N) continue;
                const float vb = var[tn] * inv_m;
                const float rstd = 1.f / sqrtf(vb + BN_EPS);
                const float sc = a.gamma[col] * rstd;
                a.o_scale[col] = sc;
                a.o_beta[col] = a.beta[col];
                a.o_mean[col] = mean[tn];
                a.o_rstd[col] = rstd;
                const float unbiased = var[tn] / (float)(M - 1);
                a.run_mean[col] = (1.f - BN_MOMENTUM) * a.run_mean[col] + BN_MOMENTUM * mean[tn];
                a.run_var[col] = (1.f - BN_MOMENTUM) * a.run_var[col] + BN_MOMENTUM * unbiased;
            }
        }
        if (blockIdx.x == 0 && tid == 0) a.count[0] += 1;
    }
    if constexpr (EPI == EPI_NORM) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            float ss = acc[0][r] * acc[0][r] + acc[1][r] * acc[1][r];   // columns past N hold zero
            ss = sum16(ss);
            if (row0 + r >= M) continue;
            const float nrm = sqrtf(ss);
#pragma unroll
            for (int tn = 0; tn < 2; ++tn) {
                const int col = 16 * tn + c;
                if (col < N) a.U[(row0 + r) * N + col] = acc[tn][r] / nrm;
            }
        }
    }
    if constexpr (EPI == EPI_EVAL) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const bool ok = row0 + r < M;
            double yy = 0.0, yx = 0.0, xx = 0.0;
#pragma unroll
            for (int tn = 0; tn < 2; ++tn) {
                const int col = n0 + 16 * tn + c;
                if (!ok || col >= N) continue;
                const double y = (double)acc[tn][r], x = (double)a.X[(row0 + r) * N + col];
                yy += y * y;
                yx += y * x;
                xx += x * x;
            }
            yy = sum16(yy);
            yx = sum16(yx);
            xx = sum16(xx);
            if (ok && c == 0) {
                double* p = a.partial + (int64_t)blockIdx.x * 3 * M + row0 + r;
                p[0] = yy;
                p[M] = yx;
                p[2 * M] = xx;
            }
        }
    }
}

// the sum of v over the block's 256 threads, in every thread: a butterfly in the waves, the waves in order
__device__ __forceinline__ float block_sum(float v, float* red) {
    v = lsr::wave_sum(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return ((red[0] + red[1]) + red[2]) + red[3];
}

// Y [B, F] the last layer, X [B, F] the batch; dY [B, F] = dL/dY; rowloss [2][AE_BM]
__global__ void __launch_bounds__(AE_THREADS) k_ae_loss(const float* __restrict__ Y, const float* __restrict__ X,
                                                        float* __restrict__ dY, float* __restrict__ rowloss, int F,
                                                        float two_over_bf, float cw_over_b) {
    __shared__ float red[4];
    const int tid = threadIdx.x;
    const int64_t base = (int64_t)blockIdx.x * F;
    float y[16], x[16];
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        const int e = tid + AE_THREADS * i;
        y[i] = e < F ? Y[base + e] : 0.f;
        x[i] = e < F ? X[base + e] : 0.f;
        s += y[i] * y[i];
    }
    const float n = sqrtf(block_sum(s, red));
    float oo = 0.f, ox = 0.f, xx = 0.f, dd = 0.f;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        y[i] = y[i] / n;                                   // out
        oo += y[i] * y[i];
        ox += y[i] * x[i];
        xx += x[i] * x[i];
        const float d = y[i] - x[i];
        dd += d * d;
    }
    oo = block_sum(oo, red);
    ox = block_sum(ox, red);
    xx = block_sum(xx, red);
    dd = block_sum(dd, red);
    const float no = sqrtf(oo), cno = fmaxf(no, COS_EPS), cnx = fmaxf(sqrtf(xx), COS_EPS);
    const float cs = ox / (cno * cnx);
    // d cos / d out = x / (cno cnx) - cos out / (cno no) where |out| is above the clamp, else without the second term
    const float ka = 1.f / (cno * cnx), kb = no > COS_EPS ? cs / (cno * no) : 0.f;
    float t = 0.f;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        const float dout = two_over_bf * (y[i] - x[i]) - cw_over_b * (ka * x[i] - kb * y[i]);
        x[i] = dout;
        t += y[i] * dout;
    }
    t = block_sum(t, red);
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        const int e = tid + AE_THREADS * i;
        if (e < F) dY[base + e] = (x[i] - y[i] * t) / n;
    }
    if (tid == 0) {
        rowloss[blockIdx.x] = dd;
        rowloss[AE_BM + blockIdx.x] = cs;
    }
}

__global__ void k_ae_loss_sum(const float* __restrict__ rowloss, int B, float inv_bf, float inv_b, float* __restrict__ losses) {
    if (threadIdx.x != 0) return;
    float dd = 0.f, cs = 0.f;
    for (int b = 0; b < B; ++b) {
        dd += rowloss[b];
        cs += rowloss[AE_BM + b];
    }
    losses[0] = dd * inv_bf;
    losses[1] = 1.f - cs * inv_b;
}

struct DxArgs {
    const float* dH;      // [B, N]
    const float* W;       // [N, K]
    const float* Hprev;   // [B, K]: what the layer's input was made from (DX_NORM: z)
    float* dHprev;        // [B, K]
    int32_t B, N, K, vec_g, vec_w;
    const float *scale, *beta, *mean, *rstd;    // DX_BN: [K], as the forward pass left them
    Moments gamma, bn_bias;
    Hyper h;
    const float* U;       // DX_NORM: [B, K]
};

template <int EPI>
__global__ void __launch_bounds__(AE_THREADS) k_ae_dx(const DxArgs a) {
    __shared__ __attribute__((aligned(16))) float lds[(AE_BM + AE_BK) * AE_LDK];
    float* Gs = lds;                                       // dH tile [64 rows][32 n]
    float* Ws = lds + AE_BM * AE_LDK;                      // W tile [32 n][32 k]
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, c = lane & 15, g = lane >> 4;
    const int k0 = blockIdx.x * AE_BN, B = a.B, N = a.N, K = a.K;
    const bool vg = a.vec_g != 0, vw = a.vec_w != 0;

    f32x4 part[2] = {f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}}, tot[2] = {part[0], part[0]};
    // the reduction runs over n: the 64 x 32 tile of dH, and W's rows n0 .. n0 + 31 at the slab's columns
    lsr::dense_k_loop<2, 1>(
        N, Gs, Ws, [=](int row, int n0, int n) { return load4(a.dH, row, B, n0 + n, N, vg); },
        [=](int row, int n0, int k) { return load4(a.W, n0 + row, N, k0 + k, K, vw); },
        [&](int n0) {
#pragma unroll
            for (int s = 0; s < AE_BK / 16; ++s) {
                if (n0 + 16 * s >= N) break;               // a tail of at most 16: the second half is all zero
                const f32x4 fa = *reinterpret_cast<const f32x4*>(Gs + (16 * wave + c) * AE_LDK + 16 * s + 4 * g);
#pragma unroll
                for (int r = 0; r < 4; ++r)
#pragma unroll
                    for (int tn = 0; tn < 2; ++tn)         // B[k = n][col]: W's tile read down its rows
                        part[tn] = mfma4(fa[r], Ws[(16 * s + 4 * g + r) * AE_LDK + 16 * tn + c], part[tn]);
            }
            chain_fold(n0, N, part, tot);
        });
    const f32x4(&acc)[2] = tot;

    // lane (c, g), register r of tile tn: row 16 wave + 4 g + r, column k0 + 16 tn + c of dA
    const int row0 = 16 * wave + 4 * g;
    if constexpr (EPI == DX_RELU) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            if (row0 + r >= B) continue;
#pragma unroll
            for (int tn = 0; tn < 2; ++tn) {
                const int col = k0 + 16 * tn + c;
                if (col >= K) continue;
                const int64_t i = (int64_t)(row0 + r) * K + col;
                a.dHprev[i] = a.Hprev[i] > 0.f ? acc[tn][r] : 0.f;
            }
        }
    }
    if constexpr (EPI == DX_BN) {
        __syncthreads();
        float* red = lds;
        float dp[2][4], xh[2][4], sc[2], s1[2], s2[2];
#pragma unroll
        for (int tn = 0; tn < 2; ++tn) {
            const int col = k0 + 16 * tn + c;
            const bool cok = col < K;
            sc[tn] = cok ? a.scale[col] : 0.f;
            const float be = cok ? a.beta[col] : 0.f, mu = cok ? a.mean[col] : 0.f, rs = cok ? a.rstd[col] : 0.f;
            s1[tn] = s2[tn] = 0.f;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                dp[tn][r] = xh[tn][r] = 0.f;
                if (!cok || row0 + r >= B) continue;
                const float hp = a.Hprev[(int64_t)(row0 + r) * K + col];
                xh[tn][r] = (hp - mu) * rs;
                dp[tn][r] = (hp - mu) * sc[tn] + be > 0.f ? acc[tn][r] : 0.f;
                s1[tn] += dp[tn][r];
                s2[tn] += dp[tn][r] * xh[tn][r];
            }
        }
        col_reduce(s1, red, wave, c, g);
        col_reduce(s2, red, wave, c, g);
        const float inv_b = 1.f / (float)B;
#pragma unroll
        for (int tn = 0; tn < 2; ++tn) {
            const int col = k0 + 16 * tn + c;
            if (col >= K) continue;
#pragma unroll
            for (int r = 0; r < 4; ++r)
                if (row0 + r < B)
                    a.dHprev[(int64_t)(row0 + r) * K + col] =
                        sc[tn] * ((dp[tn][r] - s1[tn] * inv_b) - xh[tn][r] * (s2[tn] * inv_b));
            if (wave == 0 && g == 0) {
                adam(a.gamma, col, s2[tn], a.h);
                adam(a.bn_bias, col, s1[tn], a.h);
            }
        }
    }
    if constexpr (EPI == DX_NORM) {                        // K <= 32: the block holds whole rows
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const bool ok = row0 + r < B;
            float z[2], u[2], zz = 0.f, t = 0.f;
#pragma unroll
            for (int tn = 0; tn < 2; ++tn) {
                const int col = 16 * tn + c;
                const bool in = ok && col < K;
                z[tn] = in ? a.Hprev[(int64_t)(row0 + r) * K + col] : 0.f;
                u[tn] = in ? a.U[(int64_t)(row0 + r) * K + col] : 0.f;
                zz += z[tn] * z[tn];
                t += u[tn] * (in ? acc[tn][r] : 0.f);
            }
            zz = sum16(zz);
            t = sum16(t);
            const float nz = sqrtf(zz);
#pragma unroll
            for (int tn = 0; tn < 2; ++tn) {
                const int col = 16 * tn + c;
                if (ok && col < K) a.dHprev[(int64_t)(row0 + r) * K + col] = (acc[tn][r] - u[tn] * t) / nz;
            }
        }
    }
}

struct DwArgs {
    const float* dH;      // [B, N]
    Act in;               // [B, K]
    int32_t N, vec_g;
    Moments w, b;
    Hyper h;
};

__global__ void __launch_bounds__(AE_THREADS) k_ae_dw_adam(const DwArgs a) {
    __shared__ __attribute__((aligned(16))) float lds[AE_BM * AE_DW_LDN + AE_BM * AE_LDK];
    float* Gs = lds;                                       // dH tile [64 b][64 n]
    float* As = lds + AE_BM * AE_DW_LDN;                   // input tile [64 b][32 k]
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, c = lane & 15, g = lane >> 4;
    const int k0 = blockIdx.x * AE_BN, n0 = blockIdx.y * AE_DW_BN;
    const int B = (int)a.in.rows, N = a.N, K = a.in.width;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int b = (tid >> 4) + 16 * i, n = (tid & 15) * 4;
        *reinterpret_cast<f32x4*>(Gs + b * AE_DW_LDN + n) = load4(a.dH, b, B, n0 + n, N, a.vec_g != 0);
    }
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int b = (tid >> 3) + 32 * i, k = (tid & 7) * 4;
        *reinterpret_cast<f32x4*>(As + b * AE_LDK + k) = load_act(a.in, b, k0 + k);
    }
    __syncthreads();
    // D[row n][col k] = sum over b: lane (c, g) gives dH[b = 4 j + g][n = c] and A[b = 4 j + g][k = c]
    f32x4 acc[2] = {f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}};
    const int steps = (B + 3) / 4;                         // rows past B hold zero
    for (int j = 0; j < steps; ++j) {
        const int b = 4 * j + g;
        const float ga = Gs[b * AE_DW_LDN + 16 * wave + c];
#pragma unroll
        for (int tn = 0; tn < 2; ++tn) acc[tn] = mfma4(ga, As[b * AE_LDK + 16 * tn + c], acc[tn]);
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int n = n0 + 16 * wave + 4 * g + r;
        if (n >= N) continue;
#pragma unroll
        for (int tn = 0; tn < 2; ++tn) {
            const int k = k0 + 16 * tn + c;
            if (k < K) adam(a.w, (int64_t)n * K + k, acc[tn][r], a.h);
        }
    }
    if (blockIdx.x == 0 && tid < AE_DW_BN && n0 + tid < N) {
        double s = 0.0;                                    // 64 signed terms: float64 keeps the sum to its last bit
        for (int b = 0; b < B; ++b) s += (double)Gs[b * AE_DW_LDN + tid];
        adam(a.b, n0 + tid, (float)s, a.h);
    }
}

struct BnEvalArgs {
    const float *gamma[AE_L], *var[AE_L];
    float* scale[AE_L];
    int32_t width[AE_L];
};

__global__ void __launch_bounds__(AE_THREADS) k_ae_bn_eval(const BnEvalArgs a) {
    const int i = blockIdx.x + 1;
    for (int col = threadIdx.x; col < a.width[i]; col += AE_THREADS) {
        a.scale[i][col] = a.gamma[i][col] * (1.f / sqrtf(a.var[i][col] + BN_EPS));
    }
}

// partial [slabs][3][M] -> rowvals [2][M]: the row's sum of (out - x)^2 and its cosine
__global__ void __launch_bounds__(AE_THREADS) k_ae_eval_rows(const double* __restrict__ partial, int64_t M, int slabs,
                                                             double* __restrict__ rowvals) {
    const int64_t row = (int64_t)blockIdx.x * AE_THREADS + threadIdx.x;
    if (row >= M) return;
    double yy = 0.0, yx = 0.0, xx = 0.0;
    for (int t = 0; t < slabs; ++t) {
        const double* p = partial + (int64_t)t * 3 * M + row;
        yy += p[0];
        yx += p[M];
        xx += p[2 * M];
    }
    const double n = sqrt(yy), oo = yy / (n * n), ox = yx / n;
    rowvals[row] = (oo - 2.0 * ox) + xx;
    rowvals[M + row] = ox / (fmax(sqrt(oo), (double)COS_EPS) * fmax(sqrt(xx), (double)COS_EPS));
}

// sums[v] = (first ? 0 : sums[v]) + the sum of rowvals[v][0 .. M): thread t takes rows t, t + 256, ...
__global__ void __launch_bounds__(AE_THREADS) k_ae_eval_sum(const double* __restrict__ rowvals, int64_t M, int first,
                                                            double* __restrict__ sums) {
    __shared__ double red[2][4];
    const int tid = threadIdx.x;
    double v[2] = {0.0, 0.0};
    for (int64_t i = tid; i < M; i += AE_THREADS) {
        v[0] += rowvals[i];
        v[1] += rowvals[M + i];
    }
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        v[k] = lsr::wave_sum(v[k]);
        if ((tid & 63) == 0) red[k][tid >> 6] = v[k];
    }
    __syncthreads();
    if (tid < 2) {
        const double s = ((red[tid][0] + red[tid][1]) + red[tid][2]) + red[tid][3];
        sums[tid] = (first ? 0.0 : sums[tid]) + s;
    }
}

lsr::ApiGate g_ae_api{"lsr_ae", "LSR_AE_API_VERSION", LSR_AE_API_VERSION, "this library's lsr_autoencoder.h"};

bool width_ok(int32_t w) { return w >= 16 && w <= LSR_AE_MAX_WIDTH && w % 16 == 0; }

// the width of encoder layer i's input and of decoder layer j's
int enc_in(const lsr_autoencoder& n, int i) { return i ? n.enc_dims[i - 1] : n.feature_dim; }
int dec_in(const lsr_autoencoder& n, int j) { return j ? n.dec_dims[j - 1] : n.enc_dims[n.n_enc - 1]; }

// the checks the size query and the calls share: only the dims are read
int check_dims(const std::string& w, const lsr_autoencoder* net) {
    if (int rc = g_ae_api.check(w.c_str())) return rc;
    if (!net) return lsr::fail(LSR_EINVAL, w + ": null autoencoder");
    const std::string lim = std::to_string(LSR_AE_MAX_LAYERS);
    if (net->n_enc < 1 || net->n_enc > LSR_AE_MAX_LAYERS || net->n_dec < 1 || net->n_dec > LSR_AE_MAX_LAYERS)
        return lsr::fail(LSR_EINVAL, w + ": n_enc and n_dec must be in [1, " + lim + "]");
    const std::string rule = ": the feature width and every hidden width must be a multiple of 16 and at most " +
                             std::to_string(LSR_AE_MAX_WIDTH);
    if (!width_ok(net->feature_dim)) return lsr::fail(LSR_EINVAL, w + ": feature_dim " + std::to_string(net->feature_dim) + rule);
    for (int i = 0; i + 1 < net->n_enc; ++i)
        if (!width_ok(net->enc_dims[i])) return lsr::fail(LSR_EINVAL, w + ": encoder width " + std::to_string(net->enc_dims[i]) + rule);
    for (int j = 0; j < net->n_dec; ++j)
        if (!width_ok(net->dec_dims[j])) return lsr::fail(LSR_EINVAL, w + ": decoder width " + std::to_string(net->dec_dims[j]) + rule);
    const int latent = net->enc_dims[net->n_enc - 1];
    if (latent < 1 || latent > LSR_AE_MAX_LATENT)
        return lsr::fail(LSR_EINVAL, w + ": the latent width must be in [1, " + std::to_string(LSR_AE_MAX_LATENT) + "], got " +
                                         std::to_string(latent));
    if (net->dec_dims[net->n_dec - 1] != net->feature_dim)
        return lsr::fail(LSR_EINVAL, w + ": the decoder must end at feature_dim");
    return LSR_OK;
}

// every tensor of a parameter set is there
bool params_set(const lsr_autoencoder& n, const lsr_ae_params& p) {
    for (int i = 0; i < n.n_enc; ++i) {
        if (!p.enc_w[i] || !p.enc_b[i]) return false;
        if (i && (!p.bn_w[i] || !p.bn_b[i])) return false;
    }
    for (int j = 0; j < n.n_dec; ++j)
        if (!p.dec_w[j] || !p.dec_b[j]) return false;
    return true;
}

int check_net(const std::string& w, const lsr_autoencoder& n, bool counts) {
    if (!params_set(n, n.p)) return lsr::fail(LSR_EINVAL, w + ": a weight or bias of the autoencoder is null");
    for (int i = 1; i < n.n_enc; ++i)
        if (!n.bn_mean[i] || !n.bn_var[i] || (counts && !n.bn_count[i]))
            return lsr::fail(LSR_EINVAL, w + ": a BatchNorm buffer of encoder layer " + std::to_string(i) + " is null");
    return LSR_OK;
}

struct TrainWs {
    float *H[AE_L], *dH[AE_L], *G[AE_L], *dG[AE_L], *U;
    float *scale[AE_L], *beta[AE_L], *mean[AE_L], *rstd[AE_L], *rowloss;
    size_t total;
};

TrainWs train_layout(const lsr_autoencoder& n, int64_t B, void* base) {
    lsr::Carver cv(base);
    TrainWs l{};
    for (int i = 0; i < n.n_enc; ++i) {
        l.H[i] = cv.take<float>(B * n.enc_dims[i]);
        l.dH[i] = cv.take<float>(B * n.enc_dims[i]);
        if (i) {
            l.scale[i] = cv.take<float>(n.enc_dims[i - 1]);
            l.beta[i] = cv.take<float>(n.enc_dims[i - 1]);
            l.mean[i] = cv.take<float>(n.enc_dims[i - 1]);
            l.rstd[i] = cv.take<float>(n.enc_dims[i - 1]);
        }
    }
    l.U = cv.take<float>(B * n.enc_dims[n.n_enc - 1]);
    for (int j = 0; j < n.n_dec; ++j) {
        l.G[j] = cv.take<float>(B * n.dec_dims[j]);
        l.dG[j] = cv.take<float>(B * n.dec_dims[j]);
    }
    l.rowloss = cv.take<float>(2 * AE_BM);
    l.total = cv.total();
    return l;
}

struct EvalWs {
    float *scale[AE_L], *act[2], *U;
    double *partial, *rowvals;
    int64_t chunk;
    size_t total;
};

EvalWs eval_layout(const lsr_autoencoder& n, int64_t n_rows, void* base) {
    lsr::Carver cv(base);
    EvalWs l{};
    l.chunk = std::max<int64_t>(1, std::min<int64_t>(n_rows, LSR_AE_EVAL_CHUNK));
    for (int i = 1; i < n.n_enc; ++i) {
        l.scale[i] = cv.take<float>(n.enc_dims[i - 1]);
    }
    int64_t width = 16;                                    // the widest stored activation: the latent and the last layer are not
    for (int i = 0; i + 1 < n.n_enc; ++i) width = std::max<int64_t>(width, n.enc_dims[i]);
    for (int j = 0; j + 1 < n.n_dec; ++j) width = std::max<int64_t>(width, n.dec_dims[j]);
    l.act[0] = cv.take<float>(l.chunk * width);
    l.act[1] = cv.take<float>(l.chunk * width);
    l.U = cv.take<float>(l.chunk * n.enc_dims[n.n_enc - 1]);
    const int64_t slabs = (n.feature_dim + AE_BN - 1) / AE_BN;
    l.partial = cv.take<double>(slabs * 3 * l.chunk);
    l.rowvals = cv.take<double>(2 * l.chunk);
    l.total = cv.total();
    return l;
}

int check_ws(const std::string& w, const void* ws, int64_t ws_bytes, size_t need) {
    if (!ws) return lsr::fail(LSR_EINVAL, w + ": the workspace is required");
    return lsr::check_ws(w + ": ", ws, ws_bytes, (int64_t)need, "lsr_ae_workspace_size");
}

Act act_of(const float* X, int64_t rows, int width, int pro = PRO_NONE, const float* scale = nullptr,
           const float* mean = nullptr, const float* beta = nullptr) {
    Act a{};
    a.X = X; a.scale = scale; a.mean = mean; a.beta = beta; a.rows = rows; a.width = width; a.pro = pro;
    a.vec = rows_vec(X, width);
    return a;
}

template <int EPI>
void launch_fwd(FwdArgs& a, const float* W, const float* bias, int N, hipStream_t st) {
    a.W = W; a.bias = bias; a.N = N;
    a.vec_w = rows_vec(W, a.in.width);
    const dim3 grid((unsigned)((N + AE_BN - 1) / AE_BN), (unsigned)((a.in.rows + AE_BM - 1) / AE_BM));
    hipLaunchKernelGGL(k_ae_fwd<EPI>, grid, dim3(AE_THREADS), 0, st, a);
}

// the eval-mode encoder over rows [m, feature_dim]: unit latents to `latents` [m, latent]
void encode_chunk(const lsr_autoencoder& n, const EvalWs& l, int64_t m, const float* rows, float* latents, hipStream_t st) {
    for (int i = 0; i < n.n_enc; ++i) {
        FwdArgs a{};
        a.in = i ? act_of(l.act[(i - 1) & 1], m, enc_in(n, i), PRO_BN, l.scale[i], n.bn_mean[i], n.p.bn_b[i])
                 : act_of(rows, m, n.feature_dim);
        if (i + 1 < n.n_enc) {
            a.H = l.act[i & 1];
            launch_fwd<EPI_PLAIN>(a, n.p.enc_w[i], n.p.enc_b[i], n.enc_dims[i], st);
        } else {
            a.U = latents;
            launch_fwd<EPI_NORM>(a, n.p.enc_w[i], n.p.enc_b[i], n.enc_dims[i], st);
        }
    }
}

void bn_eval(const lsr_autoencoder& n, const EvalWs& l, hipStream_t st) {
    if (n.n_enc < 2) return;
    BnEvalArgs a{};
    for (int i = 1; i < n.n_enc; ++i) {
        a.gamma[i] = n.p.bn_w[i]; a.var[i] = n.bn_var[i];
        a.scale[i] = l.scale[i]; a.width[i] = n.enc_dims[i - 1];
    }
    hipLaunchKernelGGL(k_ae_bn_eval, dim3((unsigned)(n.n_enc - 1)), dim3(AE_THREADS), 0, st, a);
}

Moments moments_of(float* p, float* m, float* v) { return Moments{p, m, v}; }

}  // namespace

extern "C" int lsr_ae_require_api(int32_t caller_version) { return g_ae_api.require(caller_version); }

extern "C" int64_t lsr_ae_workspace_size(const lsr_autoencoder* net, int64_t n_rows, int32_t training) {
    const std::string w = "lsr_ae_workspace_size";
    if (int rc = check_dims(w, net)) return -(int64_t)rc;
    if (training) {
        if (n_rows < 2 || n_rows > LSR_AE_MAX_BATCH)
            return -(int64_t)lsr::fail(LSR_EINVAL, w + ": a training batch must be in [2, " + std::to_string(LSR_AE_MAX_BATCH) +
                                                       "], got " + std::to_string(n_rows));
        return (int64_t)train_layout(*net, n_rows, nullptr).total;
    }
    if (n_rows < 0) return -(int64_t)lsr::fail(LSR_EINVAL, w + ": n_rows must be >= 0");
    return (int64_t)eval_layout(*net, n_rows, nullptr).total;
}

extern "C" int lsr_ae_encode(const lsr_autoencoder* net, int64_t n_rows, const float* rows, float* latents, void* ws,
                             int64_t ws_bytes, void* stream) {
    const std::string w = "lsr_ae_encode";
    if (int rc = check_dims(w, net)) return rc;
    if (int rc = check_net(w, *net, false)) return rc;
    if (n_rows < 0) return lsr::fail(LSR_EINVAL, w + ": n_rows must be >= 0");
    if (!rows || !latents) return lsr::fail(LSR_EINVAL, w + ": rows and latents are required");
    if (int rc = check_ws(w, ws, ws_bytes, eval_layout(*net, n_rows, nullptr).total)) return rc;
    if (n_rows == 0) return LSR_OK;
    const EvalWs l = eval_layout(*net, n_rows, ws);
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    bn_eval(*net, l, st);
    const int64_t latent = net->enc_dims[net->n_enc - 1];
    for (int64_t r0 = 0; r0 < n_rows; r0 += l.chunk)
        encode_chunk(*net, l, std::min(l.chunk, n_rows - r0), rows + r0 * net->feature_dim, latents + r0 * latent, st);
    return lsr::launched("lsr_ae_encode launch failed");
}

extern "C" int lsr_ae_eval_loss(const lsr_autoencoder* net, int64_t n_rows, const float* rows, double* sums, void* ws,
                                int64_t ws_bytes, void* stream) {
    const std::string w = "lsr_ae_eval_loss";
    if (int rc = check_dims(w, net)) return rc;
    if (int rc = check_net(w, *net, false)) return rc;
    if (n_rows < 0) return lsr::fail(LSR_EINVAL, w + ": n_rows must be >= 0");
    if (!rows || !sums) return lsr::fail(LSR_EINVAL, w + ": rows and sums are required");
    if (int rc = check_ws(w, ws, ws_bytes, eval_layout(*net, n_rows, nullptr).total)) return rc;
    const lsr_autoencoder& n = *net;
    const EvalWs l = eval_layout(n, n_rows, ws);
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    if (n_rows == 0) {                                     // the empty sums
        hipLaunchKernelGGL(k_ae_eval_sum, dim3(1), dim3(AE_THREADS), 0, st, l.rowvals, (int64_t)0, 1, sums);
        return lsr::launched("lsr_ae_eval_loss launch failed");
    }
    bn_eval(n, l, st);
    const int slabs = (n.feature_dim + AE_BN - 1) / AE_BN;
    for (int64_t r0 = 0; r0 < n_rows; r0 += l.chunk) {
        const int64_t m = std::min(l.chunk, n_rows - r0);
        const float* x = rows + r0 * n.feature_dim;
        encode_chunk(n, l, m, x, l.U, st);
        for (int j = 0; j < n.n_dec; ++j) {
            const int li = n.n_enc + j;
            FwdArgs a{};
            a.in = j ? act_of(l.act[(li - 1) & 1], m, dec_in(n, j), PRO_RELU) : act_of(l.U, m, dec_in(n, 0));
            if (j + 1 < n.n_dec) {
                a.H = l.act[li & 1];
                launch_fwd<EPI_PLAIN>(a, n.p.dec_w[j], n.p.dec_b[j], n.dec_dims[j], st);
            } else {
                a.X = x; a.partial = l.partial;
                launch_fwd<EPI_EVAL>(a, n.p.dec_w[j], n.p.dec_b[j], n.dec_dims[j], st);
            }
        }
        hipLaunchKernelGGL(k_ae_eval_rows, dim3((unsigned)((m + AE_THREADS - 1) / AE_THREADS)), dim3(AE_THREADS), 0, st,
                           l.partial, m, slabs, l.rowvals);
        hipLaunchKernelGGL(k_ae_eval_sum, dim3(1), dim3(AE_THREADS), 0, st, l.rowvals, m, r0 == 0 ? 1 : 0, sums);
    }
    return lsr::launched("lsr_ae_eval_loss launch failed");
}

extern "C" int lsr_ae_train_step(const lsr_autoencoder* net, const lsr_ae_params* m, const lsr_ae_params* v, int32_t batch,
                                 const float* rows, double lr, double beta1, double beta2, double eps, int64_t t,
                                 double cos_weight, float* losses, void* ws, int64_t ws_bytes, void* stream) {
    const std::string w = "lsr_ae_train_step";
    if (int rc = check_dims(w, net)) return rc;
    if (int rc = check_net(w, *net, true)) return rc;
    const lsr_autoencoder& n = *net;
    if (!m || !v || !params_set(n, *m) || !params_set(n, *v))
        return lsr::fail(LSR_EINVAL, w + ": Adam's moments of every parameter are required");
    if (batch < 2 || batch > LSR_AE_MAX_BATCH)
        return lsr::fail(LSR_EINVAL, w + ": the batch must be in [2, " + std::to_string(LSR_AE_MAX_BATCH) + "], got " +
                                         std::to_string(batch));
    if (!rows || !losses) return lsr::fail(LSR_EINVAL, w + ": rows and losses are required");
    if (t < 1 || !(beta1 >= 0.0 && beta1 < 1.0) || !(beta2 >= 0.0 && beta2 < 1.0))
        return lsr::fail(LSR_EINVAL, w + ": t must be >= 1 and the betas in [0, 1)");
    if (int rc = check_ws(w, ws, ws_bytes, train_layout(n, batch, nullptr).total)) return rc;
    const TrainWs l = train_layout(n, batch, ws);
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const int B = batch, F = n.feature_dim, ne = n.n_enc, nd = n.n_dec, latent = n.enc_dims[ne - 1];
    Hyper h;
    h.step = (float)(lr / (1.0 - std::pow(beta1, (double)t)));
    h.w1 = (float)(1.0 - beta1);
    h.b2 = (float)beta2;
    h.w2 = (float)(1.0 - beta2);
    h.sqrt_bc2 = (float)std::sqrt(1.0 - std::pow(beta2, (double)t));
    h.eps = (float)eps;

    // what each layer's input is made from
    auto enc_act = [&](int i) {
        return i ? act_of(l.H[i - 1], B, enc_in(n, i), PRO_BN, l.scale[i], l.mean[i], l.beta[i]) : act_of(rows, B, F);
    };
    auto dec_act = [&](int j) { return j ? act_of(l.G[j - 1], B, dec_in(n, j), PRO_RELU) : act_of(l.U, B, latent); };

    for (int i = 0; i < ne; ++i) {
        FwdArgs a{};
        a.in = enc_act(i);
        a.H = l.H[i];
        if (i + 1 < ne) {
            a.gamma = n.p.bn_w[i + 1]; a.beta = n.p.bn_b[i + 1];
            a.o_scale = l.scale[i + 1]; a.o_beta = l.beta[i + 1]; a.o_mean = l.mean[i + 1]; a.o_rstd = l.rstd[i + 1];
            a.run_mean = n.bn_mean[i + 1]; a.run_var = n.bn_var[i + 1]; a.count = n.bn_count[i + 1];
            launch_fwd<EPI_STATS>(a, n.p.enc_w[i], n.p.enc_b[i], n.enc_dims[i], st);
        } else {
            a.U = l.U;
            launch_fwd<EPI_NORM>(a, n.p.enc_w[i], n.p.enc_b[i], n.enc_dims[i], st);
        }
    }
    for (int j = 0; j < nd; ++j) {
        FwdArgs a{};
        a.in = dec_act(j);
        a.H = l.G[j];
        launch_fwd<EPI_PLAIN>(a, n.p.dec_w[j], n.p.dec_b[j], n.dec_dims[j], st);
    }
    const double bf = (double)B * (double)F;
    hipLaunchKernelGGL(k_ae_loss, dim3((unsigned)B), dim3(AE_THREADS), 0, st, l.G[nd - 1], rows, l.dG[nd - 1], l.rowloss, F,
                       (float)(2.0 / bf), (float)(cos_weight / B));
    hipLaunchKernelGGL(k_ae_loss_sum, dim3(1), dim3(64), 0, st, l.rowloss, B, (float)(1.0 / bf), (float)(1.0 / B), losses);

    auto launch_dw = [&](const float* dH, const Act& in, int N, Moments wt, Moments bs) {
        DwArgs a{};
        a.dH = dH; a.in = in; a.N = N; a.vec_g = rows_vec(dH, N);
        a.w = wt; a.b = bs; a.h = h;
        const dim3 grid((unsigned)((in.width + AE_BN - 1) / AE_BN), (unsigned)((N + AE_DW_BN - 1) / AE_DW_BN));
        hipLaunchKernelGGL(k_ae_dw_adam, grid, dim3(AE_THREADS), 0, st, a);
    };
    auto dx_args = [&](const float* dH, const float* W, int N, int K, const float* Hprev, float* dHprev) {
        DxArgs a{};
        a.dH = dH; a.W = W; a.Hprev = Hprev; a.dHprev = dHprev; a.B = B; a.N = N; a.K = K;
        a.vec_g = rows_vec(dH, N);
        a.vec_w = rows_vec(W, K);
        a.h = h;
        return a;
    };
    for (int j = nd - 1; j >= 0; --j) {
        const int N = n.dec_dims[j], K = dec_in(n, j);
        const dim3 grid((unsigned)((K + AE_BN - 1) / AE_BN));
        if (j) {
            DxArgs a = dx_args(l.dG[j], n.p.dec_w[j], N, K, l.G[j - 1], l.dG[j - 1]);
            hipLaunchKernelGGL(k_ae_dx<DX_RELU>, grid, dim3(AE_THREADS), 0, st, a);
        } else {
            DxArgs a = dx_args(l.dG[0], n.p.dec_w[0], N, K, l.H[ne - 1], l.dH[ne - 1]);
            a.U = l.U;
            hipLaunchKernelGGL(k_ae_dx<DX_NORM>, grid, dim3(AE_THREADS), 0, st, a);
        }
        launch_dw(l.dG[j], dec_act(j), N, moments_of(n.p.dec_w[j], m->dec_w[j], v->dec_w[j]),
                  moments_of(n.p.dec_b[j], m->dec_b[j], v->dec_b[j]));
    }
    for (int i = ne - 1; i >= 0; --i) {
        const int N = n.enc_dims[i], K = enc_in(n, i);
        if (i) {
            DxArgs a = dx_args(l.dH[i], n.p.enc_w[i], N, K, l.H[i - 1], l.dH[i - 1]);
            a.scale = l.scale[i]; a.beta = l.beta[i]; a.mean = l.mean[i]; a.rstd = l.rstd[i];
            a.gamma = moments_of(n.p.bn_w[i], m->bn_w[i], v->bn_w[i]);
            a.bn_bias = moments_of(n.p.bn_b[i], m->bn_b[i], v->bn_b[i]);
            hipLaunchKernelGGL(k_ae_dx<DX_BN>, dim3((unsigned)((K + AE_BN - 1) / AE_BN)), dim3(AE_THREADS), 0, st, a);
        }
        launch_dw(l.dH[i], enc_act(i), N, moments_of(n.p.enc_w[i], m->enc_w[i], v->enc_w[i]),
                  moments_of(n.p.enc_b[i], m->enc_b[i], v->enc_b[i]));
    }
    return lsr::launched("lsr_ae_train_step launch failed");
}
