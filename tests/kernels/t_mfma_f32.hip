// Test program (tests/test_query_gpu.py): exact-integer checks of the f32-input MFMA lane maps the
// query kernel (4dlangsplat_amd/csrc/query.hip) is built on:
//   1. v_mfma_f32_16x16x4_f32: lane l = (c = l & 15, g = l >> 4) holds A[row c][k = g], B[k = g][col c]
//      and D[row 4 g + reg][col c];
//   2. the kernel's 16-wide k block: register r of a per-lane float4 A[row c][4 g + r] and
//      B[4 g + r][col c] as the operands of step r sums every k exactly once;
//   3. an accumulator tile as the next product's B operand: register r of D (row 4 g + r of X) against
//      E[row c][4 g + r] gives E . X with no lane movement.
// Asymmetric integer data: a swapped row / column or a wrong k map changes the result.
#include <hip/hip_runtime.h>
#include <cstdio>

typedef float f32x4 __attribute__((ext_vector_type(4)));

__global__ void k_one(const float* A, const float* B, float* D) {   // A [16][4], B [4][16], D [16][16]
    const int l = threadIdx.x, c = l & 15, g = l >> 4;
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(A[c * 4 + g], B[g * 16 + c], acc, 0, 0, 0);
    for (int i = 0; i < 4; ++i) D[(4 * g + i) * 16 + c] = acc[i];
}

__global__ void k_block(const float* A, const float* B, const float* E, float* D, float* S) {
    // A [16][16], B [16][16] -> D = A . B; E [16][16] -> S = E . D
    const int l = threadIdx.x, c = l & 15, g = l >> 4;
    const f32x4 a = *reinterpret_cast<const f32x4*>(A + c * 16 + 4 * g);
    const f32x4 e = *reinterpret_cast<const f32x4*>(E + c * 16 + 4 * g);
    f32x4 acc = {0.f, 0.f, 0.f, 0.f}, s = {0.f, 0.f, 0.f, 0.f};
    for (int r = 0; r < 4; ++r) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a[r], B[(4 * g + r) * 16 + c], acc, 0, 0, 0);
    for (int r = 0; r < 4; ++r) s = __builtin_amdgcn_mfma_f32_16x16x4f32(e[r], acc[r], s, 0, 0, 0);
    for (int i = 0; i < 4; ++i) {
        D[(4 * g + i) * 16 + c] = acc[i];
        S[(4 * g + i) * 16 + c] = s[i];
    }
}

static int compare(const char* what, const float* got, const float* want) {
    int b = 0;
    for (int i = 0; i < 256; ++i)
        if (got[i] != want[i]) {
            if (b < 5) printf("%s [%d][%d] = %f want %f\n", what, i / 16, i % 16, got[i], want[i]);
            ++b;
        }
    printf("%s %s\n", what, b ? "FAIL" : "ok");
    return b;
}

int main() {
    int bad = 0;
    float hA[256], hB[256], hE[256], hD[256], hS[256], rD[256], rS[256];
    float *dA, *dB, *dE, *dD, *dS;
    (void)hipMalloc(&dA, sizeof hA); (void)hipMalloc(&dB, sizeof hB); (void)hipMalloc(&dE, sizeof hE);
    (void)hipMalloc(&dD, sizeof hD); (void)hipMalloc(&dS, sizeof hS);
    {
        for (int i = 0; i < 16; ++i) for (int k = 0; k < 4; ++k) hA[i * 4 + k] = (float)((i * 3 + k * 7) % 11 - 5);
        for (int k = 0; k < 4; ++k) for (int j = 0; j < 16; ++j) hB[k * 16 + j] = (float)((k * 5 + j * 2 + k * j) % 13 - 6);
        for (int i = 0; i < 16; ++i) for (int j = 0; j < 16; ++j) {
            float s = 0;
            for (int k = 0; k < 4; ++k) s += hA[i * 4 + k] * hB[k * 16 + j];
            rD[i * 16 + j] = s;
        }
        (void)hipMemcpy(dA, hA, sizeof hA, hipMemcpyHostToDevice); (void)hipMemcpy(dB, hB, sizeof hB, hipMemcpyHostToDevice);
        hipLaunchKernelGGL(k_one, dim3(1), dim3(64), 0, 0, dA, dB, dD);
        (void)hipMemcpy(hD, dD, sizeof hD, hipMemcpyDeviceToHost);
        bad += compare("mfma 16x16x4 f32 layout", hD, rD);
    }
    {
        for (int i = 0; i < 16; ++i) for (int k = 0; k < 16; ++k) {
            hA[i * 16 + k] = (float)((i * 3 + k * 7) % 11 - 5);
            hB[i * 16 + k] = (float)((i * 5 + k * 2 + i * k) % 13 - 6);
            hE[i * 16 + k] = (float)((i * 7 + k * 3 + 2 * i * k) % 9 - 4);
        }
        for (int i = 0; i < 16; ++i) for (int j = 0; j < 16; ++j) {
            float s = 0;
            for (int k = 0; k < 16; ++k) s += hA[i * 16 + k] * hB[k * 16 + j];
            rD[i * 16 + j] = s;
        }
        for (int i = 0; i < 16; ++i) for (int j = 0; j < 16; ++j) {
            float s = 0;
            for (int k = 0; k < 16; ++k) s += hE[i * 16 + k] * rD[k * 16 + j];
            rS[i * 16 + j] = s;
        }
        (void)hipMemcpy(dA, hA, sizeof hA, hipMemcpyHostToDevice); (void)hipMemcpy(dB, hB, sizeof hB, hipMemcpyHostToDevice);
        (void)hipMemcpy(dE, hE, sizeof hE, hipMemcpyHostToDevice);
        hipLaunchKernelGGL(k_block, dim3(1), dim3(64), 0, 0, dA, dB, dE, dD, dS);
        (void)hipMemcpy(hD, dD, sizeof hD, hipMemcpyDeviceToHost);
        (void)hipMemcpy(hS, dS, sizeof hS, hipMemcpyDeviceToHost);
        bad += compare("16-wide k block (A . B)", hD, rD);
        bad += compare("accumulator as B operand (E . D)", hS, rS);
    }
    return bad ? 1 : 0;
}
