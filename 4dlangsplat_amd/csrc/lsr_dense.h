// lsr_dense.h -- what the dense-layer units on the exact f32-input MFMA share (video_query.hip,
// autoencoder.hip; query.hip takes the host checks): the staged k loop of a tiled C = A . B^T, the
// row-major tile multiply, the two small device helpers around them, and the host-side refusals of a
// decoder and a workspace.  DESIGN.md 4.14, 4.15.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>

#include "../../include/lsr.h"
#include "../../include/lsr_query.h"
#include "lsr_host.h"
#include "lsr_mfma.h"

namespace lsr {

constexpr int DENSE_BK = 32;                      // the k block of the staged loop
constexpr int DENSE_LDK = DENSE_BK + 4;           // LDS row stride in floats (16-byte aligned rows)
constexpr int DENSE_THREADS = 256;                // the block that dense_k_loop's staging slots assume

// X[row][k .. k + 3] of a [rows, K] matrix, zero outside it
__device__ __forceinline__ f32x4 load4(const float* __restrict__ X, int64_t row, int64_t n_rows, int k, int K, bool vec) {
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    if (row >= n_rows) return v;
    const float* p = X + row * K + k;
    if (vec) {
        if (k + 4 <= K) v = *reinterpret_cast<const f32x4*>(p);
    } else {
#pragma unroll
        for (int r = 0; r < 4; ++r)
            if (k + r < K) v[r] = p[r];
    }
    return v;
}

template <typename T>
__device__ __forceinline__ T sum16(T v) {      // over the 16 lanes that share g: every lane gets the sum
    v += __shfl_xor(v, 1);
    v += __shfl_xor(v, 2);
    v += __shfl_xor(v, 4);
    v += __shfl_xor(v, 8);
    return v;
}

// The k loop of a block of DENSE_THREADS threads over a reduction of length K, in blocks of DENSE_BK: both
// operands' tiles (32 NA and 32 NB rows x 32 k) go global -> registers -> LDS, the next block's loads in
// flight while block(k0) works on this one.  Thread t stages float4 number t + 256 i of each tile: row
// t / 8 + 32 i, k offset 4 (t % 8); fetch_a / fetch_b(row in tile, k block start, k offset) give it, zero
// outside the matrix.  block(k0) runs between the barrier after the stores and the next block's barrier
// before them, in every thread.  (The users' fetch callables capture by value: through references the
// autoencoder's kernels came out with 4 more VGPRs and 4 more AGPRs, profiles/dense_fold.)
template <int NA, int NB, typename FetchA, typename FetchB, typename Block>
__device__ __forceinline__ void dense_k_loop(int K, float* As, float* Bs, FetchA fetch_a, FetchB fetch_b, Block block) {
    f32x4 ra[NA], rb[NB];
    const int s_row = threadIdx.x >> 3, s_k = (threadIdx.x & 7) * 4;
#pragma unroll
    for (int i = 0; i < NA; ++i) ra[i] = fetch_a(s_row + 32 * i, 0, s_k);
#pragma unroll
    for (int i = 0; i < NB; ++i) rb[i] = fetch_b(s_row + 32 * i, 0, s_k);
    for (int k0 = 0; k0 < K; k0 += DENSE_BK) {
        __syncthreads();                                   // the previous block's reads are done
#pragma unroll
        for (int i = 0; i < NA; ++i) *reinterpret_cast<f32x4*>(As + (s_row + 32 * i) * DENSE_LDK + s_k) = ra[i];
#pragma unroll
        for (int i = 0; i < NB; ++i) *reinterpret_cast<f32x4*>(Bs + (s_row + 32 * i) * DENSE_LDK + s_k) = rb[i];
        __syncthreads();
        if (k0 + DENSE_BK < K) {
#pragma unroll
            for (int i = 0; i < NA; ++i) ra[i] = fetch_a(s_row + 32 * i, k0 + DENSE_BK, s_k);
#pragma unroll
            for (int i = 0; i < NB; ++i) rb[i] = fetch_b(s_row + 32 * i, k0 + DENSE_BK, s_k);
        }
        block(k0);
    }
}

// One staged block onto a wave's TM x TN MFMA tiles: acc[tm][tn] += A[a_row + 16 tm ..][k] . B[b_row + 16 tn ..][k]
// over the k of the block that starts at k0 (rows are the tiles' LDS rows).  One 16-byte LDS read per lane
// gives X[row c][16 s + 4 g + r], r = 0..3: register r is the operand of step r, so a 16-wide k block is
// summed r-major (lsr_mfma.h's lane map), one fmaf chain per accumulator.
template <int TM, int TN>
__device__ __forceinline__ void dense_tile_mma(const float* As, const float* Bs, int a_row, int b_row, int k0, int K,
                                               f32x4 (&acc)[TM][TN]) {
    const int lane = threadIdx.x & 63, c = lane & 15, g = lane >> 4;
#pragma unroll
    for (int s = 0; s < DENSE_BK / 16; ++s) {
        if (k0 + 16 * s >= K) break;                       // a K tail of at most 16: the second half is all zero
        f32x4 fa[TM], fb[TN];
#pragma unroll
        for (int t = 0; t < TM; ++t)
            fa[t] = *reinterpret_cast<const f32x4*>(As + (a_row + 16 * t + c) * DENSE_LDK + 16 * s + 4 * g);
#pragma unroll
        for (int t = 0; t < TN; ++t)
            fb[t] = *reinterpret_cast<const f32x4*>(Bs + (b_row + 16 * t + c) * DENSE_LDK + 16 * s + 4 * g);
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
            for (int tm = 0; tm < TM; ++tm)
#pragma unroll
                for (int tn = 0; tn < TN; ++tn) acc[tm][tn] = mfma4(fa[tm][r], fb[tn][r], acc[tm][tn]);
    }
}

#pragma GCC visibility push(hidden)

// rows of a [*, K] matrix at p can be fetched 16 bytes at a time
inline bool rows_vec(const void* p, int K) { return K % 4 == 0 && aligned16(p); }

// The rules of an lsr_decoder (after the unit's ApiGate): prefix is "" or "<entry point>: "; weights: the
// layers' tensors must be there too (a size query reads only the dims).
inline int check_decoder(const std::string& prefix, const lsr_decoder* d, int max_width, bool weights) {
    if (!d) return fail(LSR_EINVAL, prefix + "null decoder");
    if (d->n_layers < 1 || d->n_layers > LSR_QUERY_MAX_LAYERS)
        return fail(LSR_EINVAL, prefix + "n_layers must be in [1, " + std::to_string(LSR_QUERY_MAX_LAYERS) + "]");
    if (d->dims[0] < 1 || d->dims[0] > LSR_QUERY_MAX_INPUT)
        return fail(LSR_EINVAL, prefix + "c_in = dims[0] must be in [1, " + std::to_string(LSR_QUERY_MAX_INPUT) + "]");
    for (int i = 1; i <= d->n_layers; ++i)
        if (d->dims[i] < 16 || d->dims[i] > max_width || d->dims[i] % 16)
            return fail(LSR_EINVAL, prefix + "layer width " + std::to_string(d->dims[i]) + ": every width after c_in "
                                        "must be a multiple of 16 and at most " + std::to_string(max_width));
    for (int i = 0; weights && i < d->n_layers; ++i)
        if (!d->weight[i] || !d->bias[i])
            return fail(LSR_EINVAL, prefix + "missing weight or bias of decoder layer " + std::to_string(i));
    return LSR_OK;
}

// a caller's workspace (not null: the entry point says which arguments it requires) against what
// size_query, the unit's *_workspace_* entry point, returns
inline int check_ws(const std::string& prefix, const void* ws, int64_t ws_bytes, int64_t need, const char* size_query) {
    if (!aligned16(ws)) return fail(LSR_EINVAL, prefix + "the workspace must be 16-byte aligned");
    if (ws_bytes < need)
        return fail(LSR_EINVAL, prefix + "the workspace holds " + std::to_string(ws_bytes) + " bytes, " +
                                    std::to_string(need) + " are needed (" + size_query + ")");
    return LSR_OK;
}

#pragma GCC visibility pop

}  // namespace lsr
