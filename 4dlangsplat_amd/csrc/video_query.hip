// video_query.hip -- the time-sensitive query's hot path (include/lsr_video.h): the wide video-feature
// decoder as a tiled GEMM on the exact f32-input MFMA (v_mfma_f32_16x16x4_f32), its last layer fused with
// the cosine against the phrase embeddings, and the per-mask means.  DESIGN.md 4.14.
//
// k_video_layer<LAST>  C = A . W^T + b for one layer: A [M, K] the (already ReLU'd) activations, W [N, K]
//                      nn.Linear's weight.  A block of 4 waves owns VQ_BM = 128 rows x VQ_BN = 128 output
//                      features, wave (wm, wn) a 64 x 64 quarter of it as 4 x 4 MFMA tiles (64 accumulator
//                      registers).  K runs in blocks of VQ_BK = 32 (lsr_dense.h's dense_k_loop and
//                      dense_tile_mma, shared with the autoencoder): both operands' 128 x 32 tiles go
//                      global -> registers -> LDS (rows padded to 36 floats), the next block's loads in flight
//                      while this one is multiplied, so each weight byte fetched meets 128 rows (64 FLOP) and
//                      each activation byte 128 features.  Rows past M, features past N and k past K are
//                      loaded as zero by predication; nothing is padded in memory.
//                        lane l = (c = l & 15, g = l >> 4) holds A[row c][k = g], B[k = g][col c] and
//                        D[row 4 g + reg][col c] (lsr_mfma.h).  One 16-byte LDS read per lane gives
//                        X[row c][k0 + 4 g + r], r = 0..3: register r is the operand of step r, whose k in lane
//                        group g is k0 + 4 g + r, for both operands alike.  The sum over a 16-wide k block
//                        therefore runs r-major (r = 0: k0 + 0, 4, 8, 12; r = 1: k0 + 1, 5, 9, 13; ...), on top
//                        of the bias, as one fmaf chain: a fixed order, the same for every row.
//                      Hidden layers store relu(C) to the workspace as the next layer's A.  The last layer
//                      stores nothing d_out-wide: per row it adds y^2 and y q_j over the block's 128 features
//                      (a lane's four column tiles in order, an xor butterfly over the 16 lanes, the two
//                      column waves in order) and writes 1 + n_q partial sums per row and column tile.
// k_video_finish       per row: the column tiles' partial sums in tile order, then dot_j / sqrt(ssq).
// k_video_segment_mean one block per segment: float64, thread t takes elements t, t + 256, ...; a butterfly
//                      inside the waves, the waves in order.
// No atomics anywhere: two calls give the same bits, and a row's result does not depend on its neighbours.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <string>

#include "../../include/lsr.h"
#include "../../include/lsr_video.h"
#include "lsr_dense.h"
#include "lsr_host.h"
#include "lsr_mfma.h"
#include "lsr_wave.h"

namespace {

using lsr::f32x4;
using lsr::load4;
using lsr::sum16;

constexpr int VQ_BM = LSR_VIDEO_ROW_TILE, VQ_BN = LSR_VIDEO_COL_TILE, VQ_BK = lsr::DENSE_BK;
constexpr int VQ_LDK = lsr::DENSE_LDK;            // LDS row stride in floats (16-byte aligned rows)
constexpr int VQ_THREADS = lsr::DENSE_THREADS;
constexpr int VQ_NV = 1 + LSR_VIDEO_MAX_QUERIES;  // values of one row's partial sum: ssq, then the dots
constexpr int VQ_LOADS = VQ_BM * VQ_BK / 4 / VQ_THREADS;   // float4 of one operand tile per thread: 4
static_assert(VQ_BM == 128 && VQ_BN == 128, "the wave layout is 2 x 2 quarters of 64 x 64");
static_assert(2 * VQ_NV * VQ_BM <= 2 * VQ_BM * VQ_LDK, "the reduction image reuses the operand tiles");

struct LayerArgs {
    const float* A;      // [M, K]
    const float* W;      // [N, K]
    const float* bias;   // [N]
    float* C;            // hidden: [M, N], relu'd
    const float* q;      // last: [n_q, N]
    float* partial;      // last: [col tiles][1 + n_q][M]
    int64_t M;
    int32_t K, N, n_q;
    int32_t vec_a, vec_w;   // rows of A / W can be fetched 16 bytes at a time
};

template <bool LAST>
__global__ void __launch_bounds__(VQ_THREADS) k_video_layer(const LayerArgs a) {
    __shared__ __attribute__((aligned(16))) float lds[2 * VQ_BM * VQ_LDK];
    float* As = lds;
    float* Ws = lds + VQ_BM * VQ_LDK;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, c = lane & 15, g = lane >> 4;
    const int wm = wave >> 1, wn = wave & 1;
    const int64_t m0 = (int64_t)blockIdx.x * VQ_BM;
    const int n0 = blockIdx.y * VQ_BN;
    const int K = a.K, N = a.N;
    const bool va = a.vec_a != 0, vw = a.vec_w != 0;
    // the wave's quarter lies wholly outside the matrix: it only helps staging
    const bool active = m0 + 64 * wm < a.M && n0 + 64 * wn < N;

    f32x4 acc[4][4];
#pragma unroll
    for (int tn = 0; tn < 4; ++tn) {
        const int col = n0 + 64 * wn + 16 * tn + c;
        const float b = col < N ? a.bias[col] : 0.f;
#pragma unroll
        for (int tm = 0; tm < 4; ++tm) acc[tm][tn] = f32x4{b, b, b, b};
    }

    lsr::dense_k_loop<VQ_LOADS, VQ_LOADS>(
        K, As, Ws, [=](int row, int k0, int k) { return load4(a.A, m0 + row, a.M, k0 + k, K, va); },
        [=](int row, int k0, int k) { return load4(a.W, n0 + row, N, k0 + k, K, vw); },
        [&](int k0) {
            if (active) lsr::dense_tile_mma(As, Ws, 64 * wm, 64 * wn, k0, K, acc);   // one fmaf chain, on the bias
        });

    if constexpr (!LAST) {
        if (!active) return;
#pragma unroll
        for (int tm = 0; tm < 4; ++tm)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int64_t row = m0 + 64 * wm + 16 * tm + 4 * g + r;
                if (row >= a.M) continue;
#pragma unroll
                for (int tn = 0; tn < 4; ++tn) {
                    const int col = n0 + 64 * wn + 16 * tn + c;
                    if (col < N) a.C[row * N + col] = fmaxf(acc[tm][tn][r], 0.f);
                }
            }
    } else {
        __syncthreads();                                   // every wave is done with the operand tiles
        float* red = lds;                                  // [wn][1 + n_q][128 rows]
        const int nv = 1 + a.n_q;
        bool ok[4];
#pragma unroll
        for (int tn = 0; tn < 4; ++tn) ok[tn] = n0 + 64 * wn + 16 * tn + c < N;   // uniform over the wave: N % 16 == 0
        for (int v = 0; v < nv; ++v) {
            float qv[4];
#pragma unroll
            for (int tn = 0; tn < 4; ++tn)
                qv[tn] = (v > 0 && ok[tn]) ? a.q[(int64_t)(v - 1) * N + n0 + 64 * wn + 16 * tn + c] : 0.f;
#pragma unroll
            for (int tm = 0; tm < 4; ++tm)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    float s = 0.f;
#pragma unroll
                    for (int tn = 0; tn < 4; ++tn) {
                        const float y = acc[tm][tn][r];
                        if (ok[tn]) s = fmaf(y, v == 0 ? y : qv[tn], s);
                    }
                    s = sum16(s);
                    if (c == 0) red[(wn * nv + v) * VQ_BM + 64 * wm + 16 * tm + 4 * g + r] = s;
                }
        }
        __syncthreads();
        for (int e = tid; e < nv * VQ_BM; e += VQ_THREADS) {
            const int v = e / VQ_BM, row = e - v * VQ_BM;
            if (m0 + row >= a.M) continue;
            a.partial[((int64_t)blockIdx.y * nv + v) * a.M + m0 + row] = red[e] + red[nv * VQ_BM + e];
        }
    }
}

__global__ void __launch_bounds__(256) k_video_finish(const float* __restrict__ partial, int64_t n_rows, int n_ct,
                                                      int n_q, float* __restrict__ cosine) {
    const int64_t row = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (row >= n_rows) return;
    const int nv = 1 + n_q;
    float ssq = 0.f;
    for (int t = 0; t < n_ct; ++t) ssq += partial[((int64_t)t * nv) * n_rows + row];
    const float norm = sqrtf(ssq);
    for (int j = 0; j < n_q; ++j) {
        float d = 0.f;
        for (int t = 0; t < n_ct; ++t) d += partial[((int64_t)t * nv + 1 + j) * n_rows + row];
        cosine[(int64_t)j * n_rows + row] = d / norm;
    }
}

__global__ void __launch_bounds__(256) k_video_segment_mean(const float* __restrict__ cosine, int64_t n_rows,
                                                            const int64_t* __restrict__ seg_offsets,
                                                            const int32_t* __restrict__ seg_query,
                                                            float* __restrict__ mean) {
    __shared__ double red[4];
    const int s = blockIdx.x, tid = threadIdx.x;
    const int64_t lo = seg_offsets[s], hi = seg_offsets[s + 1];
    const float* src = cosine + (int64_t)seg_query[s] * n_rows;
    double v = 0.0;
    for (int64_t i = lo + tid; i < hi; i += 256) v += (double)src[i];
    v = lsr::wave_sum(v);
    if ((tid & 63) == 0) red[tid >> 6] = v;
    __syncthreads();
    if (tid == 0) {
        for (int w = 1; w < 4; ++w) v += red[w];
        mean[s] = (float)(v / (double)(hi - lo));          // an empty segment: 0 / 0
    }
}

lsr::ApiGate g_video_api{"lsr_video", "LSR_VIDEO_API_VERSION", LSR_VIDEO_API_VERSION, "this library's lsr_video.h"};

int check_api(const char* what) { return g_video_api.check(what); }

// the checks the size query and the call share
int check_shapes(const char* what, const lsr_decoder* d, int64_t n_rows) {
    const std::string w(what);
    if (int rc = check_api(what)) return rc;
    if (int rc = lsr::check_decoder(w + ": ", d, LSR_VIDEO_MAX_WIDTH, false)) return rc;
    if (n_rows < 0) return lsr::fail(LSR_EINVAL, w + ": n_rows must be >= 0");
    if ((n_rows + VQ_BM - 1) / VQ_BM > 0x7fffffffLL) return lsr::fail(LSR_EINVAL, w + ": n_rows too large for one launch");
    return LSR_OK;
}

struct Layout {
    int64_t act[2];      // byte offsets of the activation images: layer i writes act[i & 1]
    int64_t partial;
    int64_t total;
};

Layout layout_of(const lsr_decoder& d, int64_t n_rows) {
    int64_t width[2] = {0, 0};
    for (int i = 0; i + 1 < d.n_layers; ++i) width[i & 1] = std::max<int64_t>(width[i & 1], d.dims[i + 1]);
    const int64_t n_ct = (d.dims[d.n_layers] + VQ_BN - 1) / VQ_BN;
    Layout l;
    l.act[0] = 0;
    l.act[1] = n_rows * width[0] * 4;                      // widths are multiples of 16: 16-byte aligned offsets
    l.partial = l.act[1] + n_rows * width[1] * 4;
    const int64_t part = (n_ct * VQ_NV * n_rows * 4 + 15) & ~(int64_t)15;
    l.total = std::max<int64_t>(l.partial + part, 16);
    return l;
}

}  // namespace

extern "C" int lsr_video_require_api(int32_t caller_version) { return g_video_api.require(caller_version); }

extern "C" int64_t lsr_video_workspace_bytes(const lsr_decoder* dec, int64_t n_rows) {
    if (int rc = check_shapes("lsr_video_workspace_bytes", dec, n_rows)) return -(int64_t)rc;
    return layout_of(*dec, n_rows).total;
}

extern "C" int lsr_video_cosine(const lsr_decoder* dec, int64_t n_rows, const float* rows, int32_t n_q,
                                const float* queries, float* cosine, void* ws, int64_t ws_bytes, void* stream) {
    if (int rc = check_shapes("lsr_video_cosine", dec, n_rows)) return rc;
    // the layers' tensors: refused after n_rows, so the dims pass once more
    if (int rc = lsr::check_decoder("lsr_video_cosine: ", dec, LSR_VIDEO_MAX_WIDTH, true)) return rc;
    const lsr_decoder& d = *dec;
    if (n_q < 1 || n_q > LSR_VIDEO_MAX_QUERIES)
        return lsr::fail(LSR_EINVAL, "lsr_video_cosine: n_q must be in [1, " + std::to_string(LSR_VIDEO_MAX_QUERIES) +
                                         "], got " + std::to_string(n_q));
    if (!rows || !queries || !cosine || !ws)
        return lsr::fail(LSR_EINVAL, "lsr_video_cosine: rows, queries, cosine and the workspace are required");
    const Layout l = layout_of(d, n_rows);
    if (int rc = lsr::check_ws("lsr_video_cosine: ", ws, ws_bytes, l.total, "lsr_video_workspace_bytes")) return rc;
    if (n_rows == 0) return LSR_OK;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    char* base = static_cast<char*>(ws);
    float* act[2] = {reinterpret_cast<float*>(base + l.act[0]), reinterpret_cast<float*>(base + l.act[1])};
    float* partial = reinterpret_cast<float*>(base + l.partial);
    const unsigned row_tiles = (unsigned)((n_rows + VQ_BM - 1) / VQ_BM);
    const float* in = rows;
    for (int i = 0; i < d.n_layers; ++i) {
        const bool last = i + 1 == d.n_layers;
        LayerArgs a{};
        a.A = in; a.W = d.weight[i]; a.bias = d.bias[i];
        a.M = n_rows; a.K = d.dims[i]; a.N = d.dims[i + 1];
        a.vec_a = lsr::rows_vec(a.A, a.K);
        a.vec_w = lsr::rows_vec(a.W, a.K);
        const dim3 grid(row_tiles, (unsigned)((a.N + VQ_BN - 1) / VQ_BN));
        if (last) {
            a.q = queries; a.n_q = n_q; a.partial = partial;
            hipLaunchKernelGGL(k_video_layer<true>, grid, dim3(VQ_THREADS), 0, st, a);
        } else {
            a.C = act[i & 1];
            hipLaunchKernelGGL(k_video_layer<false>, grid, dim3(VQ_THREADS), 0, st, a);
            in = a.C;
        }
    }
    const int n_ct = (d.dims[d.n_layers] + VQ_BN - 1) / VQ_BN;
    hipLaunchKernelGGL(k_video_finish, dim3((unsigned)((n_rows + 255) / 256)), dim3(256), 0, st, partial, n_rows, n_ct,
                       (int)n_q, cosine);
    return lsr::launched("lsr_video_cosine launch failed");
}

extern "C" int lsr_video_segment_mean(int64_t n_rows, int32_t n_q, const float* cosine, int32_t n_seg,
                                      const int64_t* seg_offsets, const int32_t* seg_query, float* mean, void* stream) {
    if (int rc = check_api("lsr_video_segment_mean")) return rc;
    if (n_rows < 0 || n_seg < 0) return lsr::fail(LSR_EINVAL, "lsr_video_segment_mean: n_rows and n_seg must be >= 0");
    if (n_q < 1 || n_q > LSR_VIDEO_MAX_QUERIES)
        return lsr::fail(LSR_EINVAL, "lsr_video_segment_mean: n_q must be in [1, " +
                                         std::to_string(LSR_VIDEO_MAX_QUERIES) + "], got " + std::to_string(n_q));
    if (!cosine || !seg_offsets || !seg_query || !mean)
        return lsr::fail(LSR_EINVAL, "lsr_video_segment_mean: cosine, seg_offsets, seg_query and mean are required");
    if (n_seg == 0) return LSR_OK;
    hipLaunchKernelGGL(k_video_segment_mean, dim3((unsigned)n_seg), dim3(256), 0, reinterpret_cast<hipStream_t>(stream),
                       cosine, n_rows, seg_offsets, seg_query, mean);
    return lsr::launched("lsr_video_segment_mean launch failed");
}
