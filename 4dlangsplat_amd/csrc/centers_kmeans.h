// centers_kmeans.h -- the per-row k-means of include/lsr_centers.h as the work of ONE wave on samples
// that sit in LDS.  Both entry points run this function (centers.hip on rows read from memory,
// deform_lang.hip on rows the language MLP has just produced), so their results are the same bits.
//
// Lane l owns samples l, l + 64, ... (at most 4: S <= 256): distances, the argmax of the seeding and the
// argmin of the assignment are per lane, folded over the wave by shuffles with (value, index) ties to
// the lowest index.  The centre update is one lane per (j, d) entry walking the samples in ascending s,
// so every sum has one order.  The wave never meets a block barrier here: waves of a block work on
// different rows and finish after different numbers of iterations.
#ifndef LSR_CENTERS_KMEANS_H_
#define LSR_CENTERS_KMEANS_H_
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace lsr {

constexpr int CK_MAX_K = 8, CK_MAX_S = 256, CK_MAX_D = 32;   // LSR_CENTERS_MAX_*
constexpr int CK_SPL = CK_MAX_S / 64;                          // samples per lane
// the samples of a block: rows of pitch D | 1 floats (odd: lanes reading one column of consecutive rows
// hit distinct banks), as many rows as fit
constexpr int CK_XFLOATS = CK_MAX_S * (CK_MAX_D | 1);
__host__ __device__ inline int ck_pitch(int D) { return D | 1; }

// LDS written by some lanes of the wave is read by others: order the accesses (the hardware runs a
// wave's LDS instructions in order; this keeps the compiler from moving them)
__device__ __forceinline__ void ck_wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

__device__ __forceinline__ float ck_dist2(const float* x, const float* c, int D) {
    float acc = 0.0f;
    for (int d = 0; d < D; ++d) {
        const float t = x[d] - c[d];
        acc += t * t;
    }
    return acc;
}

// the sample of largest v over the wave (ties: the lowest index), as an index inside [0, S)
__device__ __forceinline__ int ck_wave_argmax(float v, int i, int S) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const float ov = __shfl_xor(v, off);
        const int oi = __shfl_xor(i, off);
        if (ov > v || (ov == v && oi < i)) {
            v = ov;
            i = oi;
        }
    }
    return (unsigned)i < (unsigned)S ? i : 0;   // NaN samples compare false everywhere: stay in bounds
}

// x: [S] rows of pitch xp (LDS); c: [K * D] floats and asg: [S] bytes of LDS scratch private to the wave.
// Outputs: the row's centers [K, D], counts [K], inertia [1], iters [1] (global).
__device__ inline void kmeans_wave(const float* x, int xp, int S, int D, int K, int max_iter, float* c, uint8_t* asg,
                                   float* centers, int32_t* counts, float* inertia, int32_t* iters) {
    const int lane = threadIdx.x & 63;
    ck_wave_sync();   // the scratch may hold the wave's previous row
    // ---- maximin seeding ----
    for (int d = lane; d < D; d += 64) {   // m in c[0 .. D)
        float sum = 0.0f;
        for (int s = 0; s < S; ++s) sum += x[s * xp + d];
        c[d] = sum / (float)S;
    }
    ck_wave_sync();
    float mind[CK_SPL];
    float bv = -1.0f;
    int bi = 0x7fffffff;
#pragma unroll
    for (int q = 0; q < CK_SPL; ++q) {
        const int s = lane + 64 * q;
        if (s < S) {
            const float d2 = ck_dist2(x + s * xp, c, D);
            if (d2 > bv) {
                bv = d2;
                bi = s;
            }
        }
    }
    bi = ck_wave_argmax(bv, bi, S);
    ck_wave_sync();   // m read by every lane before c_0 replaces it
    for (int j = 0; j < K; ++j) {
        if (j > 0) {
            bv = -1.0f;
            bi = 0x7fffffff;
#pragma unroll
            for (int q = 0; q < CK_SPL; ++q) {
                const int s = lane + 64 * q;
                if (s < S && mind[q] > bv) {
                    bv = mind[q];
                    bi = s;
                }
            }
            bi = ck_wave_argmax(bv, bi, S);
        }
        for (int d = lane; d < D; d += 64) c[j * D + d] = x[bi * xp + d];
        ck_wave_sync();
#pragma unroll
        for (int q = 0; q < CK_SPL; ++q) {
            const int s = lane + 64 * q;
            if (s < S) {
                const float d2 = ck_dist2(x + s * xp, c + j * D, D);
                mind[q] = j == 0 ? d2 : fminf(mind[q], d2);
            }
        }
    }
    // ---- Lloyd ----
    float part = 0.0f;   // the lane's share of the inertia of the last assignment
    auto assign = [&](bool first) {
        bool changed = false;
        part = 0.0f;
#pragma unroll
        for (int q = 0; q < CK_SPL; ++q) {
            const int s = lane + 64 * q;
            if (s < S) {
                float best = ck_dist2(x + s * xp, c, D);
                int bj = 0;
                for (int j = 1; j < K; ++j) {
                    const float d2 = ck_dist2(x + s * xp, c + j * D, D);
                    if (d2 < best) {
                        best = d2;
                        bj = j;
                    }
                }
                if (!first) changed |= asg[s] != (uint8_t)bj;
                asg[s] = (uint8_t)bj;
                part += best;
            }
        }
        ck_wave_sync();
        return __ballot(changed) != 0ull;
    };
    assign(true);
    int it = 0;
    for (;;) {
        for (int e = lane; e < K * D; e += 64) {
            const int j = e / D, d = e - j * D;
            const float cj = c[e];
            float sum = 0.0f;
            int n = 0;
            for (int s = 0; s < S; ++s)
                if (asg[s] == (uint8_t)j) {
                    sum += x[s * xp + d] - cj;
                    ++n;
                }
            if (n > 0) c[e] = cj + sum / (float)n;
        }
        ++it;
        ck_wave_sync();
        if (!assign(false) || it >= max_iter) break;
    }
    // ---- outputs ----
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) part += __shfl_xor(part, off);
    for (int e = lane; e < K * D; e += 64) centers[e] = c[e];
    if (lane < K) {
        int n = 0;
        for (int s = 0; s < S; ++s) n += asg[s] == (uint8_t)lane;
        counts[lane] = n;
    }
    if (lane == 0) {
        inertia[0] = part;
        iters[0] = it;
    }
}

}  // namespace lsr
#endif  // LSR_CENTERS_KMEANS_H_
