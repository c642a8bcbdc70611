// Test program (tests/test_kernels_gpu.py): the staged k loop and the tile multiply of
// 4dlangsplat_amd/csrc/lsr_dense.h in the instantiations the library uses, on exact integer data.
//   k_wide    dense_k_loop<4, 4> + dense_tile_mma<4, 4>: 128 x 128 per block, a wave a 64 x 64 quarter
//             (video_query.hip's k_video_layer)
//   k_slab    dense_k_loop<2, 1> + dense_tile_mma<1, 2>: 64 rows x a 32-column slab (autoencoder.hip's k_ae_fwd)
//   k_slab_t  dense_k_loop<2, 1> alone, B walked down its rows with the reduction index and read from LDS
//             transposed (autoencoder.hip's k_ae_dx)
// Small integers stored as floats: every order of summation is exact, so each element must equal the host's
// integer sum.  Reduction lengths around the tail break at 16, one block (no prefetch), two blocks and more,
// each from a 16-byte aligned base and from one shifted by a float (the scalar fetch); row counts around the
// tile; output widths with columns past N in the last slab.  The output buffer is wider and longer than the
// matrix and filled with a sentinel: nothing outside [0, M) x [0, N) may change.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <vector>

#include "lsr_dense.h"

using lsr::f32x4;
using lsr::load4;
using lsr::mfma4;

constexpr int LDK = lsr::DENSE_LDK, BK = lsr::DENSE_BK;
constexpr float SENTINEL = -12345.f;

struct Args {
    const float* A;   // [M, R]
    const float* W;   // k_wide, k_slab: [N, R]; k_slab_t: [R, N]
    float* C;         // [M, N] in rows of ldc floats
    int M, R, N, ldc, vec_a, vec_w;
};

__global__ void __launch_bounds__(256) k_wide(const Args a) {
    __shared__ __attribute__((aligned(16))) float lds[2 * 128 * LDK];
    float* As = lds;
    float* Ws = lds + 128 * LDK;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, c = lane & 15, g = lane >> 4;
    const int wm = wave >> 1, wn = wave & 1, m0 = blockIdx.x * 128, n0 = blockIdx.y * 128;
    const bool active = m0 + 64 * wm < a.M && n0 + 64 * wn < a.N;
    f32x4 acc[4][4] = {};
    lsr::dense_k_loop<4, 4>(
        a.R, As, Ws, [=](int row, int k0, int k) { return load4(a.A, m0 + row, a.M, k0 + k, a.R, a.vec_a != 0); },
        [=](int row, int k0, int k) { return load4(a.W, n0 + row, a.N, k0 + k, a.R, a.vec_w != 0); },
        [&](int k0) {
            if (active) lsr::dense_tile_mma(As, Ws, 64 * wm, 64 * wn, k0, a.R, acc);
        });
    for (int tm = 0; tm < 4; ++tm)
        for (int r = 0; r < 4; ++r)
            for (int tn = 0; tn < 4; ++tn) {
                const int row = m0 + 64 * wm + 16 * tm + 4 * g + r, col = n0 + 64 * wn + 16 * tn + c;
                if (row < a.M && col < a.N) a.C[(size_t)row * a.ldc + col] = acc[tm][tn][r];
            }
}

template <bool TRANSPOSED>
__global__ void __launch_bounds__(256) k_slab(const Args a) {
    __shared__ __attribute__((aligned(16))) float lds[(64 + 32) * LDK];
    float* As = lds;
    float* Ws = lds + 64 * LDK;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, c = lane & 15, g = lane >> 4;
    const int n0 = blockIdx.x * 32, m0 = blockIdx.y * 64;
    f32x4 acc[1][2] = {};
    auto fetch_a = [=](int row, int k0, int k) { return load4(a.A, m0 + row, a.M, k0 + k, a.R, a.vec_a != 0); };
    if constexpr (!TRANSPOSED) {
        lsr::dense_k_loop<2, 1>(
            a.R, As, Ws, fetch_a,
            [=](int row, int k0, int k) { return load4(a.W, n0 + row, a.N, k0 + k, a.R, a.vec_w != 0); },
            [&](int k0) { lsr::dense_tile_mma(As, Ws, 16 * wave, 0, k0, a.R, acc); });
    } else {
        lsr::dense_k_loop<2, 1>(
            a.R, As, Ws, fetch_a,
            [=](int row, int k0, int n) { return load4(a.W, k0 + row, a.R, n0 + n, a.N, a.vec_w != 0); },
            [&](int k0) {
                for (int s = 0; s < BK / 16; ++s) {
                    if (k0 + 16 * s >= a.R) break;
                    const f32x4 fa = *reinterpret_cast<const f32x4*>(As + (16 * wave + c) * LDK + 16 * s + 4 * g);
                    for (int r = 0; r < 4; ++r)
                        for (int tn = 0; tn < 2; ++tn)
                            acc[0][tn] = mfma4(fa[r], Ws[(16 * s + 4 * g + r) * LDK + 16 * tn + c], acc[0][tn]);
                }
            });
    }
    for (int r = 0; r < 4; ++r)
        for (int tn = 0; tn < 2; ++tn) {
            const int row = m0 + 16 * wave + 4 * g + r, col = n0 + 16 * tn + c;
            if (row < a.M && col < a.N) a.C[(size_t)row * a.ldc + col] = acc[0][tn][r];
        }
}

static int ival_a(int i, int k) { return (i * 3 + k * 7) % 11 - 5; }
static int ival_w(int j, int k) { return (j * 5 + k * 2 + j * k) % 13 - 6; }

enum Kind { WIDE, SLAB, SLAB_T };

int main() {
    const int lengths[] = {1, 15, 16, 17, 31, 32, 33, 48, 64, 65, 128, 160}, widths[] = {16, 48};
    const int rows_wide[] = {1, 127, 129}, rows_slab[] = {1, 63, 64, 65};
    const int MAX_M = 129, MAX_R = 160, MAX_N = 48, PAD_ROWS = 8, PAD_COLS = 24;
    const size_t cap_a = (size_t)MAX_M * MAX_R + 4, cap_w = (size_t)MAX_N * MAX_R + 4;
    const size_t cap_c = (size_t)(256 + PAD_ROWS) * (MAX_N + PAD_COLS);
    float *dA, *dW, *dC;
    if (hipMalloc(&dA, cap_a * 4) != hipSuccess || hipMalloc(&dW, cap_w * 4) != hipSuccess ||
        hipMalloc(&dC, cap_c * 4) != hipSuccess) {
        printf("hipMalloc failed\n");
        return 2;
    }
    std::vector<float> hA(cap_a), hW(cap_w), hC(cap_c);
    const char* names[] = {"k_wide   <4, 4> x <4, 4>", "k_slab   <2, 1> x <1, 2>", "k_slab_t <2, 1>, transposed B"};
    int bad_total = 0;
    for (int kind = WIDE; kind <= SLAB_T; ++kind) {
        const int tile = kind == WIDE ? 128 : 64;
        const int* rows = kind == WIDE ? rows_wide : rows_slab;
        const int n_rows = kind == WIDE ? 3 : 4;
        int cases = 0, bad = 0;
        for (int R : lengths)
            for (int shift = 0; shift < 2; ++shift)
                for (int ri = 0; ri < n_rows; ++ri)
                    for (int N : widths) {
                        const int M = rows[ri], ldc = N + PAD_COLS, c_rows = (M + tile - 1) / tile * tile + PAD_ROWS;
                        for (int i = 0; i < M; ++i)
                            for (int k = 0; k < R; ++k) hA[shift + (size_t)i * R + k] = (float)ival_a(i, k);
                        for (int j = 0; j < N; ++j)
                            for (int k = 0; k < R; ++k)
                                hW[shift + (kind == SLAB_T ? (size_t)k * N + j : (size_t)j * R + k)] = (float)ival_w(j, k);
                        std::fill(hC.begin(), hC.begin() + (size_t)c_rows * ldc, SENTINEL);
                        (void)hipMemcpy(dA, hA.data(), cap_a * 4, hipMemcpyHostToDevice);
                        (void)hipMemcpy(dW, hW.data(), cap_w * 4, hipMemcpyHostToDevice);
                        (void)hipMemcpy(dC, hC.data(), (size_t)c_rows * ldc * 4, hipMemcpyHostToDevice);
                        Args a{dA + shift, dW + shift, dC, M, R, N, ldc, 0, 0};
                        // the library's rule (lsr::rows_vec): the row length, then the base
                        a.vec_a = lsr::rows_vec(a.A, R);
                        a.vec_w = lsr::rows_vec(a.W, kind == SLAB_T ? N : R);
                        if (kind == WIDE)
                            hipLaunchKernelGGL(k_wide, dim3((M + 127) / 128, (N + 127) / 128), dim3(256), 0, 0, a);
                        else if (kind == SLAB)
                            hipLaunchKernelGGL(k_slab<false>, dim3((N + 31) / 32, (M + 63) / 64), dim3(256), 0, 0, a);
                        else
                            hipLaunchKernelGGL(k_slab<true>, dim3((N + 31) / 32, (M + 63) / 64), dim3(256), 0, 0, a);
                        const hipError_t e = hipMemcpy(hC.data(), dC, (size_t)c_rows * ldc * 4, hipMemcpyDeviceToHost);
                        if (e != hipSuccess) {       // nothing more runs on the device after an error
                            printf("%s R=%d shift=%d M=%d N=%d: %s\n", names[kind], R, shift, M, N, hipGetErrorString(e));
                            return 2;
                        }
                        int wrong = 0;
                        for (int i = 0; i < c_rows; ++i)
                            for (int j = 0; j < ldc; ++j) {
                                float want = SENTINEL;
                                if (i < M && j < N) {
                                    int s = 0;
                                    for (int k = 0; k < R; ++k) s += ival_a(i, k) * ival_w(j, k);
                                    want = (float)s;
                                }
                                const float got = hC[(size_t)i * ldc + j];
                                if (got != want && wrong++ < 3)
                                    printf("%s R=%d shift=%d M=%d N=%d [%d][%d] = %f want %f\n", names[kind], R, shift, M, N,
                                           i, j, got, want);
                            }
                        ++cases;
                        bad += wrong != 0;
                    }
        printf("%s: %d cases, %d wrong: %s\n", names[kind], cases, bad, bad ? "FAIL" : "ok");
        bad_total += bad;
    }
    return bad_total ? 1 : 0;
}
