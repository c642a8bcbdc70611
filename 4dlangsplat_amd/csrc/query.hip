// query.hip -- open-vocabulary query (include/lsr_query.h): the autoencoder's decoder MLP, the L2
// normalisation and the phrase relevancy fused in one kernel on the exact f32-input MFMA
// (v_mfma_f32_16x16x4_f32).  DESIGN.md "Open-vocabulary query".
//
// One block (8 waves) owns M = 16 * NPT pixels.  A layer's input lives in LDS as X[k][pixel]; the
// waves split the layer's OUTPUT features, 16 at a time, so every weight is fetched from L2 once
// per block, straight into the A operand, and meets all M pixels in registers:
//
//   lane l = (c = l & 15, g = l >> 4) of v_mfma_f32_16x16x4_f32 holds A[row c][k = g],
//   B[k = g][col c] and D[row 4 g + reg][col c].
//   One dwordx4 per lane fetches W[o0 + c][k0 + 4 g + r], r = 0..3: register r is the A operand of
//   step r, whose k index in lane group g is therefore k0 + 4 g + r.  The B operand of step r is
//   X[k0 + 4 g + r][pixel]: one LDS read of NPT consecutive pixels per step gives the fragments of
//   NPT pixel tiles, tile j holding pixel NPT * c + j in column c.  The sum over a 16-wide k block
//   runs in the order r-major, which is fixed, so results repeat bit for bit.
//   D gives the lane outputs o0 + 4 g + reg of pixels NPT * c + j: stored (ReLU'd) as the next
//   layer's X with one NPT-wide LDS write per reg, or, in the last layer, consumed in place: reg r
//   of the tile is the B operand of a second MFMA whose A operand is E[phrase 16 t + c][o0 + 4 g + r]
//   (the same k map), accumulating the phrase sums, while its squares add to the pixel's norm.
//
// When every hidden width is at most 256 a layer's whole output sits in the waves' accumulators, so
// it overwrites the input image once all waves have read it: one 64 KB image at 64 pixels, two
// blocks per CU.  Wider decoders ping-pong between two images, at 32 pixels if 64 do not fit.
// The waves' partial phrase sums and squared norms are added in wave order through LDS: no atomics.
// The decode epilogue keeps each wave's raw features in registers until the norm is known.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <string>

#include "../../include/lsr.h"
#include "../../include/lsr_query.h"
#include "lsr_dense.h"
#include "lsr_host.h"
#include "lsr_mfma.h"
#include "lsr_wave.h"

namespace {

using lsr::aligned16;
using lsr::f32x4;
using lsr::lds_float;

typedef float f32x2 __attribute__((ext_vector_type(2)));

constexpr int kWaves = 8;
constexpr int kThreads = 64 * kWaves;
constexpr int kSsqRow = LSR_QUERY_MAX_PHRASES;   // row of the reduction image holding the squared norms
constexpr int kLdsLimit = 160 * 1024;

struct QueryArgs {
    lsr_decoder dec;
    int64_t n_pix, pix_stride, chan_stride;
    const float* latent;
    const float* pos;
    const float* neg;
    int32_t n_pos, n_neg;
    float scale;
    float* out;          // relevancy [n_pos, n_pix] or features [n_pix, d_out]
    int32_t buf_floats[2];   // LDS: rows of the even / odd layers' input images
    int32_t in_place;    // every hidden layer overwrites its own input image (one LDS buffer)
    int32_t vec_ok;      // bit i: weight[i] rows can be fetched 16 bytes at a time; bit 8 / 9: pos / neg
};

// (the activation images are read through lds_float: through a generic pointer the reads would be flat
// loads, whose wait also waits for the weight prefetch in flight)
template <int NPT> struct PixVec;
template <> struct PixVec<4> { typedef f32x4 type; typedef LSR_LDS f32x4 lds_type; };
template <> struct PixVec<2> { typedef f32x2 type; typedef LSR_LDS f32x2 lds_type; };

using lsr::mfma4;   // lsr_mfma.h

// W[row][k .. k + 3] of a [rows, in] matrix; k past `in` reads as zero (the padded first layer)
template <bool VEC>
__device__ __forceinline__ f32x4 load_frag(const float* __restrict__ row, int k, int in) {
    if (VEC) return *reinterpret_cast<const f32x4*>(row + k);
    f32x4 v;
    for (int r = 0; r < 4; ++r) v[r] = k + r < in ? row[k + r] : 0.f;
    return v;
}

// TO output tiles (16 features each) x NPT pixel tiles of one layer: acc[t][j][reg] = feature
// o0 + 16 t + 4 g + reg of pixel NPT c + j, bias included.  Rows past `out` repeat the last row.
template <int NPT, int TO, bool VEC>
__device__ __forceinline__ void layer_tiles_v(const float* __restrict__ W, const float* __restrict__ bias, int in,
                                              int in_pad, int out, const lds_float* X, int o0, f32x4 (&acc)[TO][NPT]) {
    typedef typename PixVec<NPT>::type pv;
    typedef typename PixVec<NPT>::lds_type lds_pv;
    constexpr int M = 16 * NPT;
    const int lane = threadIdx.x & 63, c = lane & 15, g = lane >> 4;
    const float* rows[TO];
    for (int t = 0; t < TO; ++t) {
        const int o = min(o0 + 16 * t + c, out - 1);
        rows[t] = W + (size_t)o * in;
        f32x4 b;
        for (int r = 0; r < 4; ++r) b[r] = bias[min(o0 + 16 * t + 4 * g + r, out - 1)];
        for (int j = 0; j < NPT; ++j) acc[t][j] = b;
    }
    // Two k blocks per iteration on two fragment sets: while the MFMAs of one block run, the weights of
    // the next are in flight into the other set.  The scheduling barriers keep the compiler from
    // sinking a prefetch below the MFMAs it is meant to overlap.
    const int last = in_pad - 16;
    f32x4 a0[TO], a1[TO];
    pv x[4];
    for (int t = 0; t < TO; ++t) a0[t] = load_frag<VEC>(rows[t], 4 * g, in);
    for (int k0 = 0; k0 < in_pad; k0 += 32) {
        for (int t = 0; t < TO; ++t) a1[t] = load_frag<VEC>(rows[t], min(k0 + 16, last) + 4 * g, in);
        for (int r = 0; r < 4; ++r) x[r] = *(const lds_pv*)(X + (k0 + 4 * g + r) * M + NPT * c);
        __builtin_amdgcn_sched_barrier(0);
        for (int r = 0; r < 4; ++r)
            for (int t = 0; t < TO; ++t)
                for (int j = 0; j < NPT; ++j) acc[t][j] = mfma4(a0[t][r], x[r][j], acc[t][j]);
        __builtin_amdgcn_sched_barrier(0);
        if (k0 + 16 < in_pad) {
            for (int t = 0; t < TO; ++t) a0[t] = load_frag<VEC>(rows[t], min(k0 + 32, last) + 4 * g, in);
            for (int r = 0; r < 4; ++r) x[r] = *(const lds_pv*)(X + (k0 + 16 + 4 * g + r) * M + NPT * c);
            __builtin_amdgcn_sched_barrier(0);
            for (int r = 0; r < 4; ++r)
                for (int t = 0; t < TO; ++t)
                    for (int j = 0; j < NPT; ++j) acc[t][j] = mfma4(a1[t][r], x[r][j], acc[t][j]);
            __builtin_amdgcn_sched_barrier(0);
        }
    }
}

template <int NPT, int TO>
__device__ __forceinline__ void layer_tiles(const float* __restrict__ W, const float* __restrict__ bias, int in,
                                            int in_pad, int out, bool vec, const lds_float* X, int o0,
                                            f32x4 (&acc)[TO][NPT]) {
    if (vec) layer_tiles_v<NPT, TO, true>(W, bias, in, in_pad, out, X, o0, acc);
    else layer_tiles_v<NPT, TO, false>(W, bias, in, in_pad, out, X, o0, acc);
}

// one hidden layer: every wave computes its share of the output tiles and stores relu(x) as the
// next layer's input image
template <int NPT, int TO>
__device__ __forceinline__ void hidden_layer(const float* __restrict__ W, const float* __restrict__ bias, int in,
                                             int in_pad, int out, bool vec, const lds_float* X, lds_float* Y) {
    typedef typename PixVec<NPT>::type pv;
    typedef typename PixVec<NPT>::lds_type lds_pv;
    constexpr int M = 16 * NPT;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, c = lane & 15, g = lane >> 4;
    for (int o0 = 16 * TO * wave; o0 < out; o0 += 16 * TO * kWaves) {
        f32x4 acc[TO][NPT];
        layer_tiles<NPT, TO>(W, bias, in, in_pad, out, vec, X, o0, acc);
        for (int t = 0; t < TO; ++t) {
            if (o0 + 16 * t >= out) break;
            for (int r = 0; r < 4; ++r) {
                pv y;
                for (int j = 0; j < NPT; ++j) y[j] = fmaxf(acc[t][j][r], 0.f);
                *(lds_pv*)(Y + (o0 + 16 * t + 4 * g + r) * M + NPT * c) = y;
            }
        }
    }
}

// the same when the whole layer fits the waves' registers (at most one tile group per wave): the
// output overwrites the input image once every wave is done reading it, which halves the LDS
template <int NPT, int TO>
__device__ __forceinline__ void hidden_layer_in_place(const float* __restrict__ W, const float* __restrict__ bias,
                                                      int in, int in_pad, int out, bool vec, lds_float* XY) {
    typedef typename PixVec<NPT>::type pv;
    typedef typename PixVec<NPT>::lds_type lds_pv;
    constexpr int M = 16 * NPT;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, c = lane & 15, g = lane >> 4;
    const int o0 = 16 * TO * wave;
    f32x4 acc[TO][NPT];
    if (o0 < out) layer_tiles<NPT, TO>(W, bias, in, in_pad, out, vec, XY, o0, acc);
    __syncthreads();
    if (o0 < out) {
#pragma unroll
        for (int t = 0; t < TO; ++t) {
            if (o0 + 16 * t >= out) continue;
            for (int r = 0; r < 4; ++r) {
                pv y;
                for (int j = 0; j < NPT; ++j) y[j] = fmaxf(acc[t][j][r], 0.f);
                *(lds_pv*)(XY + (o0 + 16 * t + 4 * g + r) * M + NPT * c) = y;
            }
        }
    }
}

// phrase row j of the stacked [positives; negatives] embeddings, or NULL past the end
__device__ __forceinline__ const float* phrase_row(const QueryArgs& a, int j, int d_out) {
    if (j < a.n_pos) return a.pos + (size_t)j * d_out;
    if (j < a.n_pos + a.n_neg) return a.neg + (size_t)(j - a.n_pos) * d_out;
    return nullptr;
}

// NPH: 0 = the decode epilogue, else the relevancy epilogue for up to NPH phrase tiles of 16 (their
// accumulators are 16 NPH registers; at NPH = 1 two blocks fit a CU's register file)
template <int NPT, int NPH>
__global__ void __launch_bounds__(kThreads) __attribute__((amdgpu_waves_per_eu(NPH == 1 ? 4 : 2)))
k_query(const QueryArgs a) {
    constexpr bool RELEVANCY = NPH > 0;
    constexpr int NS = NPH > 0 ? NPH : 1;
    typedef typename PixVec<NPT>::type pv;
    typedef typename PixVec<NPT>::lds_type lds_pv;
    constexpr int M = 16 * NPT;
    extern __shared__ __attribute__((aligned(16))) float lds_generic[];
    lds_float* lds = (lds_float*)lds_generic;
    lds_float* buf[2] = {lds, a.in_place ? lds : lds + a.buf_floats[0] * M};
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, c = lane & 15, g = lane >> 4;
    const int64_t pix0 = (int64_t)blockIdx.x * M;
    const int n_layers = a.dec.n_layers, c_in = a.dec.dims[0], d_out = a.dec.dims[n_layers];
    const int c_pad = (c_in + 15) & ~15;

    // the latent, channel-major, zero in the padding rows and past the last pixel
    for (int e = tid; e < c_pad * M; e += kThreads) {
        const int ch = e / M, p = e - ch * M;
        float v = 0.f;
        if (ch < c_in && pix0 + p < a.n_pix) v = a.latent[(pix0 + p) * a.pix_stride + ch * a.chan_stride];
        buf[0][e] = v;
    }
    __syncthreads();

    for (int i = 0; i + 1 < n_layers; ++i) {
        const int in = a.dec.dims[i], out = a.dec.dims[i + 1], in_pad = (in + 15) & ~15;
        const bool vec = (a.vec_ok >> i) & 1;
        if (a.in_place) {
            if (out > 16 * kWaves)
                hidden_layer_in_place<NPT, 2>(a.dec.weight[i], a.dec.bias[i], in, in_pad, out, vec, lds);
            else
                hidden_layer_in_place<NPT, 1>(a.dec.weight[i], a.dec.bias[i], in, in_pad, out, vec, lds);
        } else if (out >= 32 * kWaves)
            hidden_layer<NPT, 2>(a.dec.weight[i], a.dec.bias[i], in, in_pad, out, vec, buf[i & 1], buf[(i + 1) & 1]);
        else
            hidden_layer<NPT, 1>(a.dec.weight[i], a.dec.bias[i], in, in_pad, out, vec, buf[i & 1], buf[(i + 1) & 1]);
        __syncthreads();
    }

    // the last layer: its tiles are consumed as they are produced
    const int li = n_layers - 1;
    const int in = a.dec.dims[li], in_pad = (in + 15) & ~15;
    const lds_float* X = buf[li & 1];
    const bool vec = (a.vec_ok >> li) & 1;
    const int n_phr = RELEVANCY ? a.n_pos + a.n_neg : 0;
    const int n_pt = (n_phr + 15) >> 4;                      // phrase tiles, <= 4
    f32x4 s[NS][NPT];                                        // s[t][j][reg]: phrase 16 t + 4 g + reg . x of pixel NPT c + j
    float ssq[NPT];
    for (int t = 0; t < NS; ++t)
        for (int j = 0; j < NPT; ++j) s[t][j] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int j = 0; j < NPT; ++j) ssq[j] = 0.f;
    constexpr int TO = 2;
    constexpr int NG = LSR_QUERY_MAX_WIDTH / (16 * TO * kWaves);   // tile groups of one wave: 2
    static_assert(NG * 16 * TO * kWaves == LSR_QUERY_MAX_WIDTH, "the widest last layer is NG groups per wave");
    f32x4 kept[RELEVANCY ? 1 : NG][TO][NPT];                 // decode: the wave's raw features, until the norm is known
#pragma unroll
    for (int gi = 0; gi < NG; ++gi) {
        const int o0 = 16 * TO * (wave + kWaves * gi);
        if (o0 >= d_out) continue;
        f32x4(&acc)[TO][NPT] = kept[RELEVANCY ? 0 : gi];
        layer_tiles<NPT, TO>(a.dec.weight[li], a.dec.bias[li], in, in_pad, d_out, vec, X, o0, acc);
#pragma unroll
        for (int t = 0; t < TO; ++t) {
            const int ot = o0 + 16 * t;
            if (ot >= d_out) continue;
            for (int j = 0; j < NPT; ++j)
                for (int r = 0; r < 4; ++r) ssq[j] = fmaf(acc[t][j][r], acc[t][j][r], ssq[j]);
            if constexpr (RELEVANCY) {
#pragma unroll
                for (int pt = 0; pt < NS; ++pt) {
                    if (pt >= n_pt) continue;
                    const float* row = phrase_row(a, 16 * pt + c, d_out);
                    f32x4 e = {0.f, 0.f, 0.f, 0.f};
                    if (row) {
                        if ((a.vec_ok >> (16 * pt + c < a.n_pos ? 8 : 9)) & 1) e = load_frag<true>(row, ot + 4 * g, d_out);
                        else e = load_frag<false>(row, ot + 4 * g, d_out);
                    }
                    for (int r = 0; r < 4; ++r)
                        for (int j = 0; j < NPT; ++j) s[pt][j] = mfma4(e[r], acc[t][j][r], s[pt][j]);
                }
            }
        }
    }
    // the four lane groups hold disjoint features of the same pixels
    for (int j = 0; j < NPT; ++j) {
        ssq[j] += __shfl_xor(ssq[j], 16);
        ssq[j] += __shfl_xor(ssq[j], 32);
    }
    __syncthreads();                                         // every wave is done reading X
    // the waves' partial sums, added in wave order into one [65][M] image
    lds_float* red = lds;
    for (int w = 0; w < kWaves; ++w) {
        if (wave == w) {
#pragma unroll
            for (int pt = 0; pt < NS; ++pt) {
                if (pt >= n_pt) continue;
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    lds_pv* dst = (lds_pv*)(red + (16 * pt + 4 * g + r) * M + NPT * c);
                    pv v;
                    for (int j = 0; j < NPT; ++j) v[j] = s[pt][j][r];
                    if (w > 0) v += *dst;
                    *dst = v;
                }
            }
            if (g == 0) {
                lds_pv* dst = (lds_pv*)(red + kSsqRow * M + NPT * c);
                pv v;
                for (int j = 0; j < NPT; ++j) v[j] = ssq[j];
                if (w > 0) v += *dst;
                *dst = v;
            }
        }
        __syncthreads();
    }
    if constexpr (RELEVANCY) {
        for (int e = tid; e < a.n_pos * M; e += kThreads) {
            const int j = e / M, p = e - j * M;
            if (pix0 + p >= a.n_pix) continue;
            const float norm = sqrtf(red[kSsqRow * M + p]);
            float mneg = red[a.n_pos * M + p] / norm;
            for (int i = 1; i < a.n_neg; ++i) {
                const float v = red[(a.n_pos + i) * M + p] / norm;
                mneg = (v > mneg || v != v) ? v : mneg;
            }
            const float d = a.scale * (red[j * M + p] / norm - mneg);
            a.out[(int64_t)j * a.n_pix + pix0 + p] = 1.f / (1.f + expf(-d));
        }
    } else {
        const pv sq = *(const lds_pv*)(red + kSsqRow * M + NPT * c);
#pragma unroll
        for (int gi = 0; gi < NG; ++gi)
#pragma unroll
            for (int t = 0; t < TO; ++t) {
                const int ot = 16 * TO * (wave + kWaves * gi) + 16 * t;
                if (ot >= d_out) continue;
                for (int j = 0; j < NPT; ++j) {
                    const int64_t p = pix0 + NPT * c + j;
                    if (p >= a.n_pix) continue;
                    const float norm = sqrtf(sq[j]);
                    f32x4 v = kept[RELEVANCY ? 0 : gi][t][j];
                    for (int r = 0; r < 4; ++r) v[r] = v[r] / norm;
                    *reinterpret_cast<f32x4*>(a.out + p * d_out + ot + 4 * g) = v;
                }
            }
    }
}

lsr::ApiGate g_query_api{"lsr_query", "LSR_QUERY_API_VERSION", LSR_QUERY_API_VERSION, "this library's lsr_query.h"};

int check_decoder(const lsr_decoder* d) {
    if (int rc = g_query_api.check()) return rc;
    return lsr::check_decoder("", d, LSR_QUERY_MAX_WIDTH, true);
}

template <bool RELEVANCY>
int launch(QueryArgs& a, hipStream_t st) {
    const lsr_decoder& d = a.dec;
    // LDS rows: one image that every hidden layer overwrites when each layer's output fits the waves'
    // registers, else the even and odd layers' input images side by side; the reduction image reuses them
    int rows[2] = {0, 0};
    a.in_place = 1;
    for (int i = 1; i < d.n_layers; ++i) a.in_place &= d.dims[i] <= 32 * kWaves;
    for (int i = 0; i < d.n_layers; ++i) {
        const int b = a.in_place ? 0 : i & 1;
        rows[b] = std::max(rows[b], (d.dims[i] + 15) & ~15);
    }
    const int need = std::max(rows[0] + rows[1], kSsqRow + 1);
    a.buf_floats[0] = rows[0];
    a.buf_floats[1] = rows[1];
    a.vec_ok = 0;
    for (int i = 0; i < d.n_layers; ++i)
        if (d.dims[i] % 16 == 0 && aligned16(d.weight[i])) a.vec_ok |= 1 << i;
    if (RELEVANCY) a.vec_ok |= (aligned16(a.pos) ? 1 << 8 : 0) | (aligned16(a.neg) ? 1 << 9 : 0);
    if (!RELEVANCY && !aligned16(a.out)) return lsr::fail(LSR_EINVAL, "features must be 16-byte aligned");
    const bool wide = (size_t)need * 64 * sizeof(float) <= (size_t)kLdsLimit;
    const int M = wide ? 64 : 32;
    const size_t lds = (size_t)need * M * sizeof(float);
    if (lds > (size_t)kLdsLimit) return lsr::fail(LSR_EINVAL, "decoder too wide for the on-chip activation image");
    const int64_t blocks = (a.n_pix + M - 1) / M;
    if (blocks > 0x7fffffffLL) return lsr::fail(LSR_EINVAL, "n_pix too large for one launch");
    const int n_pt = (a.n_pos + a.n_neg + 15) / 16;
    auto kern = !RELEVANCY ? (wide ? k_query<4, 0> : k_query<2, 0>)
                : n_pt <= 1 ? (wide ? k_query<4, 1> : k_query<2, 1>)
                : n_pt <= 2 ? (wide ? k_query<4, 2> : k_query<2, 2>)
                            : (wide ? k_query<4, 4> : k_query<2, 4>);
    if (hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize,
                            (int)lds) != hipSuccess)
        return lsr::fail(LSR_EHIP, "query: cannot reserve the activation image in LDS");
    hipLaunchKernelGGL(kern, dim3((unsigned)blocks), dim3(kThreads), lds, st, a);
    return lsr::launched("query launch failed");
}

}  // namespace

extern "C" int lsr_query_require_api(int32_t caller_version) { return g_query_api.require(caller_version); }

extern "C" int lsr_query_relevancy(const lsr_decoder* dec, int64_t n_pix, const float* latent, int64_t pix_stride,
                                   int64_t chan_stride, int32_t n_pos, const float* pos_embeds, int32_t n_neg,
                                   const float* neg_embeds, float scale, float* relevancy, void* stream) {
    int rc = check_decoder(dec);
    if (rc) return rc;
    if (n_pix < 0) return lsr::fail(LSR_EINVAL, "n_pix must be >= 0");
    if (n_pos < 1 || n_neg < 1 || n_pos + (int64_t)n_neg > LSR_QUERY_MAX_PHRASES)
        return lsr::fail(LSR_EINVAL, "n_pos >= 1, n_neg >= 1 and n_pos + n_neg <= " +
                                         std::to_string(LSR_QUERY_MAX_PHRASES) + " are required");
    if (!latent || !pos_embeds || !neg_embeds || !relevancy)
        return lsr::fail(LSR_EINVAL, "latent, pos_embeds, neg_embeds and relevancy are required");
    if (n_pix == 0) return LSR_OK;
    QueryArgs a{};
    a.dec = *dec;
    a.n_pix = n_pix; a.pix_stride = pix_stride; a.chan_stride = chan_stride;
    a.latent = latent; a.pos = pos_embeds; a.neg = neg_embeds;
    a.n_pos = n_pos; a.n_neg = n_neg; a.scale = scale; a.out = relevancy;
    return launch<true>(a, reinterpret_cast<hipStream_t>(stream));
}

extern "C" int lsr_query_decode(const lsr_decoder* dec, int64_t n_pix, const float* latent, int64_t pix_stride,
                                int64_t chan_stride, float* features, void* stream) {
    int rc = check_decoder(dec);
    if (rc) return rc;
    if (n_pix < 0) return lsr::fail(LSR_EINVAL, "n_pix must be >= 0");
    if (!latent || !features) return lsr::fail(LSR_EINVAL, "latent and features are required");
    if (n_pix == 0) return LSR_OK;
    QueryArgs a{};
    a.dec = *dec;
    a.n_pix = n_pix; a.pix_stride = pix_stride; a.chan_stride = chan_stride;
    a.latent = latent; a.out = features;
    return launch<false>(a, reinterpret_cast<hipStream_t>(stream));
}
