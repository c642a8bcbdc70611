// pca.hip -- PCA colouring of language images (include/lsr_pca.h; render.py:52-65 pca_compress).
// DESIGN.md 4.11.
//
// Every sweep over a frame has the same shape: one block (4 waves) owns PCA_BLOCK_PIX = 2048 consecutive
// pixels and walks them in tiles of PCA_TILE = 256.  A tile goes to LDS as X[channel][pixel] (pitch
// 260 floats) by loads that are coalesced for either layout: pixel-fastest when chan_stride != 1 (the
// renderer's [C, H, W]), channel-fastest when chan_stride == 1 ([H, W, C]).  Where the strides and the
// alignment allow 16 bytes per lane, the loads of the next tile are issued before the current one is
// consumed.  Pixels past the end and channels past C are zero in the tile.
//
// k_pca_sums     per-channel sums of the tile in float64 (8 threads per channel), one float64 partial
//                [32] per block.  Float64 from the first add: the mean of a constant image is exact.
// k_pca_gram     the tile centred by float(m) as it is staged; each wave feeds its 64 pixels as 16
//                slabs of 4 to v_mfma_f32_16x16x4_f32: lane (c = l & 15, g = l >> 4) holds
//                x[pixel g of the slab][channel c] and x[pixel g][channel 16 + c], which are the A and
//                the B operand alike, so the three distinct 16 x 16 tiles of the symmetric 32 x 32 cost
//                two LDS reads and three MFMAs per slab.  The waves' accumulators are added in wave
//                order through LDS into one float32 partial [3][256] per block.
// k_pca_finish   the block partials added in a fixed order in float64 into the accumulator (sums [32],
//                or gram [32 * 32], which it unfolds from the three tiles).
// k_pca_basis    one block of 512: cyclic Jacobi on the 32 x 32 covariance in float64 in LDS.  A sweep
//                is 31 rounds of the round-robin (circle) ordering, 16 disjoint rotations each: 16
//                threads take the angles from the 2 x 2 pivots, then 256 threads apply J^T A J to the
//                16 x 16 disjoint 2 x 2 blocks of A while 256 more apply V J: two barriers a round.
//                A rotation is skipped when its pivot is negligible.  The iteration stops after the
//                first sweep that leaves the three largest diagonal entries alone in their rows with
//                the rest provably below them (or that rotated nothing; at most 30 sweeps): the small
//                eigenvalues, which converge last, are not waited for.  Then the sign rule and the
//                outputs.
// k_pca_project  y = (x - m) . v_k from the staged tile, one pixel per thread, explicit FMAs in channel
//                order; the block's min and max of y go to the workspace.
// k_pca_range    one block folds them into range[2] (min and max do not depend on the order).
// k_pca_colorize y through range to float32 or bytes.
// No atomics anywhere: two calls give the same bits.  Element offsets are 64-bit.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <string>

#include "../../include/lsr.h"
#include "../../include/lsr_pca.h"
#include "lsr_host.h"
#include "lsr_mfma.h"
#include "lsr_wave.h"

namespace {

using lsr::f32x4;
using lsr::lds_float;

constexpr int PCA_THREADS = 256, PCA_WAVES = PCA_THREADS / 64;
constexpr int PCA_TILE = LSR_PCA_TILE_PIXELS;          // pixels staged at once: 64 per wave
constexpr int PCA_PITCH = PCA_TILE + 4;                // floats between channel rows: the MFMA reads hit 64 banks
constexpr int PCA_BLOCK_PIX = LSR_PCA_BLOCK_PIXELS;    // pixels of one block and of one partial
constexpr int PCA_CMAX = LSR_PCA_MAX_CHANNELS;
constexpr int PCA_GRAM_PARTIAL = 3 * 256;              // floats of one block's Gram partial: tiles 00, 01, 11
constexpr int PCA_BASIS_THREADS = 512;
constexpr int PCA_MAX_SWEEPS = 30;
static_assert(PCA_BLOCK_PIX % PCA_TILE == 0, "a block walks whole tiles");
static_assert(PCA_CMAX == 32 && PCA_THREADS == 256 && PCA_TILE == 256,
              "the thread maps below are written for 32 channels, 256 threads and one pixel per thread");
static_assert(PCA_THREADS == LSR_PCA_RANGE_THREADS, "k_pca_range folds the block pairs LSR_PCA_RANGE_THREADS apart");

// three blocks of a sweep per CU (a frame of the headline size gives each CU 2.6): a third of the register
// file each; at a quarter the Gram sweep spills
#define PCA_SWEEP_OCCUPANCY __attribute__((amdgpu_waves_per_eu(3)))

using lsr::mfma4;   // lsr_mfma.h: v_mfma_f32_16x16x4_f32

struct Frame {
    const float* x;
    int64_t n_pix, pix_stride, chan_stride;
    int C;
    int vec;   // whole tiles can be fetched 16 bytes at a time (frame_of)
};

// rows C ... 31 of the tile image are never staged: zero them once
__device__ __forceinline__ void zero_pad_rows(lds_float* X, int C) {
    for (int e = C * PCA_PITCH + threadIdx.x; e < PCA_CMAX * PCA_PITCH; e += PCA_THREADS) X[e] = 0.f;
}

// One thread's share of a tile on its way from memory to LDS.  A whole tile of a frame that allows
// 16-byte loads is fetched ahead: its loads are issued before the current tile is consumed and land in
// these registers meanwhile (all indices into v are compile-time constants, so it stays in
// registers).  Any other tile is fetched by store_tile itself, 4 bytes per lane.
struct Tile {
    float v[PCA_CMAX];   // 8 x 16 bytes
    int64_t t0;          // first pixel
    int n;               // valid pixels of the tile
    int vec;             // fetched ahead
};

__device__ __forceinline__ void load_tile(const Frame& f, int64_t t0, Tile& T) {
    const int tid = threadIdx.x;
    T.t0 = t0;
    T.n = (int)min((int64_t)PCA_TILE, f.n_pix - t0);
    T.vec = f.vec && T.n == PCA_TILE;
    if (T.vec) {
        if (f.chan_stride == 1) {        // [pixel][C] contiguous: 16 bytes are 4 channels of one pixel
            const f32x4* src = reinterpret_cast<const f32x4*>(f.x + t0 * f.pix_stride);
#pragma unroll
            for (int i = 0; i < PCA_CMAX / 4; ++i) {
                const int j = tid + PCA_THREADS * i;
                if (4 * j < f.C * PCA_TILE) {
                    const f32x4 q = src[j];
                    T.v[4 * i] = q[0]; T.v[4 * i + 1] = q[1]; T.v[4 * i + 2] = q[2]; T.v[4 * i + 3] = q[3];
                }
            }
        } else {                         // channel rows of contiguous pixels: 16 bytes are 4 pixels of one channel
#pragma unroll
            for (int i = 0; i < PCA_CMAX / 4; ++i) {
                const int j = tid + PCA_THREADS * i, ch = j >> 6;
                if (ch < f.C) {
                    const f32x4 q = *reinterpret_cast<const f32x4*>(f.x + ch * f.chan_stride + t0 + 4 * (j & 63));
                    T.v[4 * i] = q[0]; T.v[4 * i + 1] = q[1]; T.v[4 * i + 2] = q[2]; T.v[4 * i + 3] = q[3];
                }
            }
        }
    }
}

// X[ch][p] = x[t0 + p, ch] - mean[ch] (CENTRE) for ch < C, p < PCA_TILE; zero past the last pixel
template <bool CENTRE>
__device__ __forceinline__ void store_tile(const Frame& f, const Tile& T, const float* mean, lds_float* X) {
    const int tid = threadIdx.x;
    if (T.vec) {
        if (f.chan_stride == 1) {
#pragma unroll
            for (int i = 0; i < PCA_CMAX / 4; ++i) {
                const int j = tid + PCA_THREADS * i;
                if (4 * j < f.C * PCA_TILE) {
                    const int p = 4 * j / f.C, ch = 4 * j - p * f.C;
#pragma unroll
                    for (int r = 0; r < 4; ++r)
                        X[(ch + r) * PCA_PITCH + p] = CENTRE ? T.v[4 * i + r] - mean[ch + r] : T.v[4 * i + r];
                }
            }
        } else {
#pragma unroll
            for (int i = 0; i < PCA_CMAX / 4; ++i) {
                const int j = tid + PCA_THREADS * i, ch = j >> 6;
                if (ch < f.C) {
                    const float m = CENTRE ? mean[ch] : 0.f;
                    const f32x4 q = {T.v[4 * i] - m, T.v[4 * i + 1] - m, T.v[4 * i + 2] - m, T.v[4 * i + 3] - m};
                    *(LSR_LDS f32x4*)(X + ch * PCA_PITCH + 4 * (j & 63)) = q;
                }
            }
        }
    } else if (f.chan_stride == 1) {     // channel-fastest: element e of the tile is pixel e / C, channel e % C
#pragma unroll 4
        for (int i = 0; i < f.C; ++i) {
            const int e = tid + PCA_THREADS * i, p = e / f.C, ch = e - p * f.C;
            float v = 0.f;
            if (p < T.n) {
                v = f.x[(T.t0 + p) * f.pix_stride + ch];
                if (CENTRE) v -= mean[ch];
            }
            X[ch * PCA_PITCH + p] = v;
        }
    } else {                             // pixel-fastest: channel i of pixel tid
#pragma unroll 4
        for (int i = 0; i < f.C; ++i) {
            float v = 0.f;
            if (tid < T.n) {
                v = f.x[(T.t0 + tid) * f.pix_stride + i * f.chan_stride];
                if (CENTRE) v -= mean[i];
            }
            X[i * PCA_PITCH + tid] = v;
        }
    }
}

// The walk every sweep shares: `consume(t0)` runs on each staged tile while the next one is in flight.
template <bool CENTRE, typename F>
__device__ __forceinline__ void for_each_tile(const Frame& f, int64_t p0, int64_t p1, const float* mean, lds_float* X,
                                              F consume) {
    Tile T;
    load_tile(f, p0, T);
    for (int64_t t0 = p0; t0 < p1; t0 += PCA_TILE) {
        __syncthreads();                                 // the last tile is consumed (and the mean is written)
        store_tile<CENTRE>(f, T, mean, X);
        __syncthreads();
        if (t0 + PCA_TILE < p1) load_tile(f, t0 + PCA_TILE, T);
        consume(t0);
    }
}

__global__ void __launch_bounds__(PCA_THREADS) PCA_SWEEP_OCCUPANCY k_pca_sums(const Frame f, double* __restrict__ partial) {
    __shared__ __attribute__((aligned(16))) float X_generic[PCA_CMAX * PCA_PITCH];
    lds_float* X = (lds_float*)X_generic;
    const int tid = threadIdx.x, ch = tid >> 3, sub = tid & 7;
    const int64_t p0 = (int64_t)blockIdx.x * PCA_BLOCK_PIX, p1 = min(p0 + PCA_BLOCK_PIX, f.n_pix);
    zero_pad_rows(X, f.C);
    double s = 0.0;
    for_each_tile<false>(f, p0, p1, nullptr, X, [&](int64_t) {
        for (int i = 0; i < PCA_TILE / 8; ++i) s += (double)X[ch * PCA_PITCH + sub + 8 * i];
    });
    s += __shfl_xor(s, 1);
    s += __shfl_xor(s, 2);
    s += __shfl_xor(s, 4);
    if (sub == 0) partial[(int64_t)blockIdx.x * PCA_CMAX + ch] = s;
}

__global__ void __launch_bounds__(PCA_THREADS) PCA_SWEEP_OCCUPANCY
k_pca_gram(const Frame f, const double* __restrict__ sums, double n_total, float* __restrict__ partial) {
    __shared__ __attribute__((aligned(16))) float X_generic[PCA_CMAX * PCA_PITCH];
    __shared__ float mean[PCA_CMAX];
    lds_float* X = (lds_float*)X_generic;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, c = lane & 15, g = lane >> 4;
    const int64_t p0 = (int64_t)blockIdx.x * PCA_BLOCK_PIX, p1 = min(p0 + PCA_BLOCK_PIX, f.n_pix);
    if (tid < PCA_CMAX) mean[tid] = tid < f.C ? (float)(sums[tid] / n_total) : 0.f;
    zero_pad_rows(X, f.C);
    const bool two = f.C > 16;                           // channels 16 ... 31 exist
    f32x4 acc[3];
    for (int t = 0; t < 3; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
    const lds_float* lo = X + c * PCA_PITCH + 64 * wave + g;
    const lds_float* hi = lo + 16 * PCA_PITCH;
    for_each_tile<true>(f, p0, p1, mean, X, [&](int64_t) {
        if (two) {
#pragma unroll 4
            for (int s = 0; s < 16; ++s) {
                const float a = lo[4 * s], b = hi[4 * s];
                acc[0] = mfma4(a, a, acc[0]);
                acc[1] = mfma4(a, b, acc[1]);
                acc[2] = mfma4(b, b, acc[2]);
            }
        } else {
#pragma unroll 4
            for (int s = 0; s < 16; ++s) {
                const float a = lo[4 * s];
                acc[0] = mfma4(a, a, acc[0]);
            }
        }
    });
    __syncthreads();
    // lane (c, g), register r holds D[4 g + r][c]; the waves' tiles side by side in the tile image
    lds_float* red = X;
    static_assert(PCA_WAVES * PCA_GRAM_PARTIAL <= PCA_CMAX * PCA_PITCH, "the waves' partials fit the tile image");
    for (int t = 0; t < 3; ++t)
        for (int r = 0; r < 4; ++r) red[wave * PCA_GRAM_PARTIAL + t * 256 + (4 * g + r) * 16 + c] = acc[t][r];
    __syncthreads();
    for (int t = 0; t < 3; ++t) {
        float v = red[t * 256 + tid];
        for (int w = 1; w < PCA_WAVES; ++w) v += red[w * PCA_GRAM_PARTIAL + t * 256 + tid];
        partial[(int64_t)blockIdx.x * PCA_GRAM_PARTIAL + t * 256 + tid] = v;
    }
}

// One wave-wide group of 64 accumulator entries per block, 16 waves: wave w adds the partials of
// blocks w, w + 16, ... in float64, and the first wave adds the 16 sums in wave order: a fixed order,
// with the loads of 16 waves in flight.  GRAM: entry u of the three tiles [3][256]; its upper triangle
// goes to gram [32 * 32] and is mirrored.  Else sums [32].
constexpr int PCA_FINISH_WAVES = LSR_PCA_FINISH_WAVES;
template <bool GRAM>
__global__ void __launch_bounds__(64 * PCA_FINISH_WAVES)
k_pca_finish(const void* __restrict__ partial, int64_t blocks, int reset, double* __restrict__ acc) {
    __shared__ double red[PCA_FINISH_WAVES][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int u = blockIdx.x * 64 + lane;
    double s = 0.0;
    if (GRAM) {
        const float* p = static_cast<const float*>(partial) + u;
#pragma unroll 8
        for (int64_t k = wave; k < blocks; k += PCA_FINISH_WAVES) s += (double)p[k * PCA_GRAM_PARTIAL];
    } else if (u < PCA_CMAX) {
        const double* p = static_cast<const double*>(partial) + u;
#pragma unroll 8
        for (int64_t k = wave; k < blocks; k += PCA_FINISH_WAVES) s += p[k * PCA_CMAX];
    }
    red[wave][lane] = s;
    __syncthreads();
    if (wave != 0) return;
    for (int w = 1; w < PCA_FINISH_WAVES; ++w) s += red[w][lane];
    if (GRAM) {
        const int t = u >> 8, r = (u >> 4) & 15, c = u & 15;
        if (t != 1 && r > c) return;                     // the lower triangle of a diagonal tile: mirrored below
        const int i = r + (t == 2 ? 16 : 0), j = c + (t >= 1 ? 16 : 0);
        const double v = reset ? s : acc[i * PCA_CMAX + j] + s;
        acc[i * PCA_CMAX + j] = v;
        if (i != j) acc[j * PCA_CMAX + i] = v;
    } else if (u < PCA_CMAX) {
        acc[u] = reset ? s : acc[u] + s;
    }
}

__global__ void __launch_bounds__(PCA_BASIS_THREADS)
k_pca_basis(int C, double n_total, const double* __restrict__ sums, const double* __restrict__ gram,
            float* __restrict__ mean, float* __restrict__ comps, float* __restrict__ evals) {
    constexpr int N = PCA_CMAX, LD = N + 1;
    constexpr double EPS2 = 1e-24;                       // (relative size of a negligible entry) squared
    __shared__ double A[N * LD], V[N * LD];
    // a round's rotations: written by the first 16 threads, read by all after the barrier; the next
    // round writes the other set, so no reader is overtaken
    __shared__ double rot_c[2][16], rot_s[2][16];
    __shared__ int rot_p[2][16], rot_q[2][16], rot_any[2];
    __shared__ double tiny2, sign[3];
    __shared__ int done, top[3];
    const int tid = threadIdx.x;
    for (int e = tid; e < N * N; e += PCA_BASIS_THREADS) {
        const int i = e >> 5, j = e & 31;
        A[i * LD + j] = (i < C && j < C) ? gram[e] / (n_total - 1.0) : 0.0;
        V[i * LD + j] = i == j ? 1.0 : 0.0;
    }
    __syncthreads();
    if (tid == 0) {
        double tr = 0.0;
        for (int i = 0; i < N; ++i) tr += fabs(A[i * LD + i]);
        tiny2 = 1e-12 * tr * tr;                         // diagonal entries a millionth of the trace count as this
    }
    __syncthreads();
    int round = 0;
    for (int sweep = 0; sweep < PCA_MAX_SWEEPS; ++sweep) {
        bool sweep_active = false;                       // thread 0's: some rotation was not skipped
        for (int k = 0; k < N - 1; ++k, ++round) {
            const int set = round & 1;
            if (tid < 64) {                              // the first wave, whole: the ballot below
                bool act = false;
                if (tid < 16) {
                    // the circle method: 31 stays, the others turn; round k pairs (k + i) with (k - i) mod 31
                    int p = tid == 0 ? N - 1 : (k + tid) % (N - 1);
                    int q = tid == 0 ? k : (k + (N - 1) - tid) % (N - 1);
                    if (p > q) { const int t = p; p = q; q = t; }
                    const double app = A[p * LD + p], aqq = A[q * LD + q], apq = A[p * LD + q];
                    double cs = 1.0, sn = 0.0;
                    const double d = aqq - app, r2 = d * d + 4.0 * apq * apq;
                    if (apq * apq > EPS2 * (fabs(app * aqq) + tiny2) && r2 > 1e-280) {
                        // cos(2 phi) = |d| / r, sin(2 phi) = sgn(d) 2 apq / r with r = sqrt(r2), |phi| <= pi / 4:
                        // cos = sqrt(x), sin = sin(2 phi) / (2 cos), x = (1 + cos(2 phi)) / 2 >= 1 / 2.
                        // Two reciprocal square roots in a row, no division: this chain is what a round waits for.
                        const double inv_r = rsqrt(r2), x = 0.5 + 0.5 * fabs(d) * inv_r, inv_c = rsqrt(x);
                        cs = x * inv_c;
                        sn = (d >= 0.0 ? apq : -apq) * inv_r * inv_c;
                        act = sn != 0.0;
                    }
                    rot_p[set][tid] = p; rot_q[set][tid] = q; rot_c[set][tid] = cs; rot_s[set][tid] = sn;
                }
                const bool any = __ballot(act) != 0;
                if (tid == 0) { rot_any[set] = any; sweep_active |= any; }
            }
            __syncthreads();
            if (!rot_any[set]) continue;                 // uniform: the whole block skips an idle round
            if (tid < 256) {
                // A <- J^T A J on the 2 x 2 block of rows (pa, qa) and columns (pb, qb): blocks are disjoint
                const int a = tid >> 4, b = tid & 15;
                const int pa = rot_p[set][a], qa = rot_q[set][a], pb = rot_p[set][b], qb = rot_q[set][b];
                const double ca = rot_c[set][a], sa = rot_s[set][a], cb = rot_c[set][b], sb = rot_s[set][b];
                if (sa != 0.0 || sb != 0.0) {
                    const double b00 = A[pa * LD + pb], b01 = A[pa * LD + qb], b10 = A[qa * LD + pb], b11 = A[qa * LD + qb];
                    const double c00 = cb * b00 - sb * b01, c01 = sb * b00 + cb * b01;   // columns: B J_b
                    const double c10 = cb * b10 - sb * b11, c11 = sb * b10 + cb * b11;
                    const bool pivot = a == b;           // the rotation makes its own off-diagonal pair zero
                    A[pa * LD + pb] = ca * c00 - sa * c10;                                 // rows: J_a^T (B J_b)
                    A[pa * LD + qb] = pivot ? 0.0 : ca * c01 - sa * c11;
                    A[qa * LD + pb] = pivot ? 0.0 : sa * c00 + ca * c10;
                    A[qa * LD + qb] = sa * c01 + ca * c11;
                }
            } else {
                // V <- V J: row r, the columns of two of the 16 pairs
                const int r = tid & 31;
#pragma unroll
                for (int h = 0; h < 2; ++h) {
                    const int b = ((tid - 256) >> 5) + 8 * h;
                    const int p = rot_p[set][b], q = rot_q[set][b];
                    const double cs = rot_c[set][b], sn = rot_s[set][b];
                    if (sn != 0.0) {
                        const double vp = V[r * LD + p], vq = V[r * LD + q];
                        V[r * LD + p] = cs * vp - sn * vq;
                        V[r * LD + q] = sn * vp + cs * vq;
                    }
                }
            }
            __syncthreads();
        }
        // Stop once the three largest diagonal entries (of the first C: the padding's stay exact zeros)
        // are eigenvalues, i.e. their rows hold nothing else, and no eigenvalue of the rest can exceed
        // the third (Gershgorin: a_ii + sum_j |a_ij|); or when a whole sweep found nothing to rotate.
        if (tid < 64) {                                  // the first wave: lane i < C owns row i
            const int i = tid & 31;
            const bool valid = tid < C;
            const double d = A[i * LD + i];
            double off2 = 0.0, radius = 0.0;
            for (int j = 0; j < N; ++j)
                if (j != i) {
                    const double v = A[i * LD + j];
                    off2 += v * v;
                    radius += fabs(v);
                }
            double key = valid ? d : -INFINITY;
            int pick[3];
            double third = 0.0;
            for (int k = 0; k < 3; ++k) {                // three arg-max butterflies; the lowest index wins ties
                double bv = key;
                int bi = tid;
                for (int o = 32; o > 0; o >>= 1) {
                    const double ov = __shfl_xor(bv, o);
                    const int oi = __shfl_xor(bi, o);
                    if (ov > bv || (ov == bv && oi < bi)) { bv = ov; bi = oi; }
                }
                pick[k] = bi;
                third = bv;
                if (tid == bi) key = -INFINITY;
            }
            const bool is_top = tid == pick[0] || tid == pick[1] || tid == pick[2];
            const bool alone = __ballot(is_top && !(off2 <= EPS2 * (d * d + tiny2))) == 0;
            const bool below = __ballot(valid && !is_top && d + radius > third) == 0;
            if (tid == 0) {
                top[0] = pick[0]; top[1] = pick[1]; top[2] = pick[2];
                done = (alone && below) || !sweep_active;
            }
        }
        __syncthreads();
        if (done) break;
    }
    if (tid < 3) {
        // sklearn's sign rule; the first entry of largest magnitude wins ties
        const int col = top[tid];
        int big = 0;
        for (int ch = 1; ch < C; ++ch)
            if (fabs(V[ch * LD + col]) > fabs(V[big * LD + col])) big = ch;
        sign[tid] = V[big * LD + col] < 0.0 ? -1.0 : 1.0;
        evals[tid] = (float)A[col * LD + col];
    }
    __syncthreads();
    if (tid < 3 * N) {
        const int k = tid >> 5, ch = tid & 31;
        if (ch < C) comps[k * C + ch] = (float)(sign[k] * V[ch * LD + top[k]]);
    }
    if (tid < C) mean[tid] = (float)(sums[tid] / n_total);
}

__global__ void __launch_bounds__(PCA_THREADS) PCA_SWEEP_OCCUPANCY
k_pca_project(const Frame f, const float* __restrict__ mean_in, const float* __restrict__ comps,
              float* __restrict__ y, float* __restrict__ partial) {
    __shared__ __attribute__((aligned(16))) float X_generic[PCA_CMAX * PCA_PITCH];
    __shared__ float mean[PCA_CMAX], v[3 * PCA_CMAX], red_mn[PCA_WAVES], red_mx[PCA_WAVES];
    lds_float* X = (lds_float*)X_generic;
    const int tid = threadIdx.x;
    const int64_t p0 = (int64_t)blockIdx.x * PCA_BLOCK_PIX, p1 = min(p0 + PCA_BLOCK_PIX, f.n_pix);
    if (tid < f.C) mean[tid] = mean_in[tid];
    if (tid < 3 * PCA_CMAX) v[tid] = (tid & 31) < f.C ? comps[(tid >> 5) * f.C + (tid & 31)] : 0.f;
    float mn = INFINITY, mx = -INFINITY;
    for_each_tile<true>(f, p0, p1, mean, X, [&](int64_t t0) {
        if (t0 + tid < f.n_pix) {
            float a0 = 0.f, a1 = 0.f, a2 = 0.f;
            for (int ch = 0; ch < f.C; ++ch) {
                const float xv = X[ch * PCA_PITCH + tid];
                a0 = fmaf(xv, v[ch], a0);
                a1 = fmaf(xv, v[PCA_CMAX + ch], a1);
                a2 = fmaf(xv, v[2 * PCA_CMAX + ch], a2);
            }
            if (y) {
                float* dst = y + (t0 + tid) * 3;
                dst[0] = a0; dst[1] = a1; dst[2] = a2;
            }
            mn = fminf(mn, fminf(a0, fminf(a1, a2)));
            mx = fmaxf(mx, fmaxf(a0, fmaxf(a1, a2)));
        }
    });
    for (int o = 32; o > 0; o >>= 1) {
        mn = fminf(mn, __shfl_xor(mn, o));
        mx = fmaxf(mx, __shfl_xor(mx, o));
    }
    if ((tid & 63) == 0) { red_mn[tid >> 6] = mn; red_mx[tid >> 6] = mx; }
    __syncthreads();
    if (tid == 0 && partial) {
        for (int w = 1; w < PCA_WAVES; ++w) { mn = fminf(mn, red_mn[w]); mx = fmaxf(mx, red_mx[w]); }
        partial[2 * (int64_t)blockIdx.x] = mn;
        partial[2 * (int64_t)blockIdx.x + 1] = mx;
    }
}

__global__ void __launch_bounds__(PCA_THREADS)
k_pca_range(const float* __restrict__ partial, int64_t blocks, int reset, float* __restrict__ range) {
    __shared__ float red_mn[PCA_WAVES], red_mx[PCA_WAVES];
    const int tid = threadIdx.x;
    float mn = INFINITY, mx = -INFINITY;
    for (int64_t k = tid; k < blocks; k += PCA_THREADS) {
        mn = fminf(mn, partial[2 * k]);
        mx = fmaxf(mx, partial[2 * k + 1]);
    }
    for (int o = 32; o > 0; o >>= 1) {
        mn = fminf(mn, __shfl_xor(mn, o));
        mx = fmaxf(mx, __shfl_xor(mx, o));
    }
    if ((tid & 63) == 0) { red_mn[tid >> 6] = mn; red_mx[tid >> 6] = mx; }
    __syncthreads();
    if (tid == 0) {
        for (int w = 1; w < PCA_WAVES; ++w) { mn = fminf(mn, red_mn[w]); mx = fmaxf(mx, red_mx[w]); }
        if (!reset) { mn = fminf(mn, range[0]); mx = fmaxf(mx, range[1]); }
        range[0] = mn;
        range[1] = mx;
    }
}

template <bool BYTES>
__global__ void __launch_bounds__(PCA_THREADS)
k_pca_colorize(int64_t n, const float* __restrict__ y, const float* __restrict__ range, void* __restrict__ out) {
    const int64_t e = (int64_t)blockIdx.x * PCA_THREADS + threadIdx.x;
    if (e >= n) return;
    const float mn = range[0], span = range[1] - mn;
    float v = 0.f;
    if (span > 0.f) v = fminf(fmaxf((y[e] - mn) / span, 0.f), 1.f);
    if (BYTES) static_cast<uint8_t*>(out)[e] = (uint8_t)(255.f * v);
    else static_cast<float*>(out)[e] = v;
}

// vec: a whole tile can be fetched 16 bytes at a time, as channel rows of contiguous pixels or as
// contiguous pixels of C channels
Frame frame_of(const float* x, int64_t n_pix, int64_t pix_stride, int64_t chan_stride, int C) {
    const bool aligned = lsr::aligned16(x);
    const bool rows = pix_stride == 1 && chan_stride != 1 && chan_stride % 4 == 0;
    const bool packed = chan_stride == 1 && pix_stride == C && C % 4 == 0;
    return Frame{x, n_pix, pix_stride, chan_stride, C, aligned && (rows || packed) ? 1 : 0};
}

int64_t block_count(int64_t n_pix) { return (n_pix + PCA_BLOCK_PIX - 1) / PCA_BLOCK_PIX; }

// the checks every sweep shares; 0 blocks: nothing to launch
int check_sweep(const char* what, int32_t C, int64_t n_pix, const void* frame, int64_t pix_stride, int64_t chan_stride,
                const void* workspace, bool need_workspace, int64_t* blocks) {
    if (C < LSR_PCA_MIN_CHANNELS || C > LSR_PCA_MAX_CHANNELS)
        return lsr::fail(LSR_EINVAL, std::string(what) + ": C must be in [" + std::to_string(LSR_PCA_MIN_CHANNELS) +
                                         ", " + std::to_string(LSR_PCA_MAX_CHANNELS) + "], got " + std::to_string(C));
    if (n_pix < 0) return lsr::fail(LSR_EINVAL, std::string(what) + ": n_pix must be >= 0");
    if (!frame || (need_workspace && !workspace))
        return lsr::fail(LSR_EINVAL, std::string(what) + ": frame and workspace are required");
    if (pix_stride < 0 || chan_stride < 0)
        return lsr::fail(LSR_EINVAL, std::string(what) + ": pix_stride and chan_stride must be >= 0");
    if (reinterpret_cast<uintptr_t>(workspace) & 7)
        return lsr::fail(LSR_EINVAL, std::string(what) + ": workspace must be 8-byte aligned");
    *blocks = block_count(n_pix);
    if (*blocks > 0x7fffffffLL) return lsr::fail(LSR_EINVAL, std::string(what) + ": n_pix too large for one launch");
    return LSR_OK;
}

}  // namespace

extern "C" int64_t lsr_pca_workspace_bytes(int32_t C, int64_t n_pix) {
    if (C < LSR_PCA_MIN_CHANNELS || C > LSR_PCA_MAX_CHANNELS || n_pix < 0) {
        lsr::fail(LSR_EINVAL, "lsr_pca_workspace_bytes: C in [4, 32] and n_pix >= 0 are required");
        return -1;
    }
    // per block: the Gram partial (3 KB); the float64 sums [32] and the min / max pair fit the same bytes
    static_assert(PCA_GRAM_PARTIAL * sizeof(float) >= PCA_CMAX * sizeof(double), "one size serves every sweep");
    const int64_t blocks = block_count(n_pix);
    return (blocks > 0 ? blocks : 1) * (int64_t)(PCA_GRAM_PARTIAL * sizeof(float));
}

extern "C" int lsr_pca_sums(int32_t C, int64_t n_pix, const float* frame, int64_t pix_stride, int64_t chan_stride,
                            int32_t reset, double* sums, void* workspace, void* stream) {
    int64_t blocks = 0;
    if (int rc = check_sweep("lsr_pca_sums", C, n_pix, frame, pix_stride, chan_stride, workspace, true, &blocks)) return rc;
    if (!sums) return lsr::fail(LSR_EINVAL, "lsr_pca_sums: sums is required");
    if (blocks == 0) return LSR_OK;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const Frame f = frame_of(frame, n_pix, pix_stride, chan_stride, C);
    hipLaunchKernelGGL(k_pca_sums, dim3((unsigned)blocks), dim3(PCA_THREADS), 0, st, f, static_cast<double*>(workspace));
    hipLaunchKernelGGL(k_pca_finish<false>, dim3(1), dim3(64 * PCA_FINISH_WAVES), 0, st, (const void*)workspace, blocks, (int)reset, sums);
    return lsr::launched("lsr_pca_sums launch failed");
}

extern "C" int lsr_pca_gram(int32_t C, int64_t n_pix, const float* frame, int64_t pix_stride, int64_t chan_stride,
                            const double* sums, int64_t n_total, int32_t reset, double* gram, void* workspace,
                            void* stream) {
    int64_t blocks = 0;
    if (int rc = check_sweep("lsr_pca_gram", C, n_pix, frame, pix_stride, chan_stride, workspace, true, &blocks)) return rc;
    if (!sums || !gram) return lsr::fail(LSR_EINVAL, "lsr_pca_gram: sums and gram are required");
    if (n_total < n_pix || n_total < 1)
        return lsr::fail(LSR_EINVAL, "lsr_pca_gram: n_total must be the pixel count of the sums, >= n_pix and >= 1");
    if (blocks == 0) return LSR_OK;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const Frame f = frame_of(frame, n_pix, pix_stride, chan_stride, C);
    hipLaunchKernelGGL(k_pca_gram, dim3((unsigned)blocks), dim3(PCA_THREADS), 0, st, f, sums, (double)n_total,
                       static_cast<float*>(workspace));
    hipLaunchKernelGGL(k_pca_finish<true>, dim3(PCA_GRAM_PARTIAL / 64), dim3(64 * PCA_FINISH_WAVES), 0, st, (const void*)workspace, blocks, (int)reset, gram);
    return lsr::launched("lsr_pca_gram launch failed");
}

extern "C" int lsr_pca_basis(int32_t C, int64_t n_total, const double* sums, const double* gram, float* mean,
                             float* components, float* eigenvalues, void* stream) {
    if (C < LSR_PCA_MIN_CHANNELS || C > LSR_PCA_MAX_CHANNELS)
        return lsr::fail(LSR_EINVAL, "lsr_pca_basis: C must be in [" + std::to_string(LSR_PCA_MIN_CHANNELS) + ", " +
                                         std::to_string(LSR_PCA_MAX_CHANNELS) + "], got " + std::to_string(C));
    if (n_total < 2) return lsr::fail(LSR_EINVAL, "lsr_pca_basis: a covariance needs n_total >= 2 pixels");
    if (!sums || !gram || !mean || !components || !eigenvalues)
        return lsr::fail(LSR_EINVAL, "lsr_pca_basis: sums, gram, mean, components and eigenvalues are required");
    hipLaunchKernelGGL(k_pca_basis, dim3(1), dim3(PCA_BASIS_THREADS), 0, reinterpret_cast<hipStream_t>(stream), (int)C,
                       (double)n_total, sums, gram, mean, components, eigenvalues);
    return lsr::launched("lsr_pca_basis launch failed");
}

extern "C" int lsr_pca_project(int32_t C, int64_t n_pix, const float* frame, int64_t pix_stride, int64_t chan_stride,
                               const float* mean, const float* components, int32_t reset, float* y, float* range,
                               void* workspace, void* stream) {
    int64_t blocks = 0;
    if (int rc = check_sweep("lsr_pca_project", C, n_pix, frame, pix_stride, chan_stride, workspace, range != nullptr,
                             &blocks))
        return rc;
    if (!mean || !components) return lsr::fail(LSR_EINVAL, "lsr_pca_project: mean and components are required");
    if (!y && !range) return lsr::fail(LSR_EINVAL, "lsr_pca_project: y or range is required (both NULL: nothing to do)");
    if (blocks == 0) return LSR_OK;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const Frame f = frame_of(frame, n_pix, pix_stride, chan_stride, C);
    hipLaunchKernelGGL(k_pca_project, dim3((unsigned)blocks), dim3(PCA_THREADS), 0, st, f, mean, components, y,
                       range ? static_cast<float*>(workspace) : nullptr);
    if (range)
        hipLaunchKernelGGL(k_pca_range, dim3(1), dim3(PCA_THREADS), 0, st, (const float*)workspace, blocks, (int)reset,
                           range);
    return lsr::launched("lsr_pca_project launch failed");
}

namespace {
template <bool BYTES>
int colorize(const char* what, int64_t n_pix, const float* y, const float* range, void* out, void* stream) {
    if (n_pix < 0) return lsr::fail(LSR_EINVAL, std::string(what) + ": n_pix must be >= 0");
    if (!y || !range || !out) return lsr::fail(LSR_EINVAL, std::string(what) + ": y, range and out are required");
    const int64_t n = 3 * n_pix, blocks = (n + PCA_THREADS - 1) / PCA_THREADS;
    if (blocks > 0x7fffffffLL) return lsr::fail(LSR_EINVAL, std::string(what) + ": n_pix too large for one launch");
    if (blocks == 0) return LSR_OK;
    hipLaunchKernelGGL(k_pca_colorize<BYTES>, dim3((unsigned)blocks), dim3(PCA_THREADS), 0,
                       reinterpret_cast<hipStream_t>(stream), n, y, range, out);
    return lsr::launched(std::string(what) + " launch failed");
}
}  // namespace

extern "C" int lsr_pca_colorize_f32(int64_t n_pix, const float* y, const float* range, float* out, void* stream) {
    return colorize<false>("lsr_pca_colorize_f32", n_pix, y, range, out, stream);
}

extern "C" int lsr_pca_colorize_u8(int64_t n_pix, const float* y, const float* range, uint8_t* out, void* stream) {
    return colorize<true>("lsr_pca_colorize_u8", n_pix, y, range, out, stream);
}
