// deform_mfma.h -- device helpers of the 128-wide deformation kernels (deform.hip, deform_lang.hip,
// deform_wgrad.hip, deform_pack.hip): the bf16 hi/lo MFMA tile product, the block shape, the LDS poison.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace lsr {

// LDS poison build (-DLSR_LDS_POISON, build/variants/liblsr_ldspoison.so; tests/test_deform_lds_poison_gpu.py):
// every kernel of these units fills its shared memory with all-ones words (NaN as fp32 and as bf16)
// at block entry, so a read of LDS the block never wrote turns the results into NaN instead of
// silently reusing what an earlier block on the CU left there.
#ifdef LSR_LDS_POISON
__device__ __forceinline__ void lds_poison(void* p, size_t bytes) {
    uint32_t* w = static_cast<uint32_t*>(p);
    for (size_t i = threadIdx.x; i < bytes / 4; i += blockDim.x) w[i] = 0xFFFFFFFFu;
}
#define LDS_POISON(arr) lds_poison(&(arr), sizeof(arr))
#define LDS_POISON_DONE() __syncthreads()
#else
#define LDS_POISON(arr) do {} while (0)
#define LDS_POISON_DONE() do {} while (0)
#endif

typedef __bf16 dbf16x8 __attribute__((ext_vector_type(8)));
typedef float df32x16 __attribute__((ext_vector_type(16)));
#define DMFMA(a, b, c) __builtin_amdgcn_mfma_f32_32x32x16_bf16((a), (b), (c), 0, 0, 0)
typedef float df32x4 __attribute__((ext_vector_type(4)));
#define DMFMA16(a, b, c) __builtin_amdgcn_mfma_f32_16x16x32_bf16((a), (b), (c), 0, 0, 0)

constexpr int DN = 64;            // Gaussians per block
constexpr int DWID = 128;         // MLP width
constexpr int DAP = DWID + 8;     // LDS row pitch (bf16) of the hidden rows
constexpr int DLP = 64 + 8;       // LDS row pitch (bf16) of rows of up to 64 entries

__device__ __forceinline__ void dsplit(float x, __bf16& hi, __bf16& lo) {
    hi = (__bf16)x;
    lo = (__bf16)(x - (float)hi);
}
__device__ __forceinline__ int row_of(int mt, int q, int hh) { return 32 * mt + (q & 3) + 8 * (q >> 2) + 4 * hh; }

// Y[64 x 32] (+)= X[64 x K] W^T for N tile `nt`: both M tiles (the block's 64 Gaussians) share
// every weight fragment, so a block reads each weight once per layer.
template <int K>
__device__ __forceinline__ void mlp_ntile(df32x16 (&acc)[2], const __bf16* __restrict__ xh, const __bf16* __restrict__ xl,
                                          int xp, int nt, const __bf16* __restrict__ wh, const __bf16* __restrict__ wl) {
    const int lane = threadIdx.x & 63, r = lane & 31, h = lane >> 5;
    // every weight fragment of the tile in flight at once (L2-resident, one round trip)
    dbf16x8 bh[K / 16], bl[K / 16];
#pragma unroll
    for (int ks = 0; ks < K / 16; ++ks) {
        const size_t wo = (size_t)(32 * nt + r) * K + 16 * ks + 8 * h;
        bh[ks] = *reinterpret_cast<const dbf16x8*>(wh + wo);
        bl[ks] = *reinterpret_cast<const dbf16x8*>(wl + wo);
    }
    __builtin_amdgcn_sched_barrier(0);   // keep the loads issued here, ahead of the MFMAs
#pragma unroll
    for (int ks = 0; ks < K / 16; ++ks) {
        const int k0 = 16 * ks + 8 * h;
#pragma unroll
        for (int mt = 0; mt < 2; ++mt) {
            const dbf16x8 ah = *reinterpret_cast<const dbf16x8*>(xh + (32 * mt + r) * xp + k0);
            const dbf16x8 al = *reinterpret_cast<const dbf16x8*>(xl + (32 * mt + r) * xp + k0);
            acc[mt] = DMFMA(ah, bh[ks], acc[mt]);
            acc[mt] = DMFMA(ah, bl[ks], acc[mt]);
            acc[mt] = DMFMA(al, bh[ks], acc[mt]);
        }
    }
}
// the same with K a runtime multiple of 16 in [16, 64] (the lang_deform input width)
__device__ __forceinline__ void mlp_ntile_k(int K, df32x16 (&acc)[2], const __bf16* xh, const __bf16* xl, int xp, int nt,
                                            const __bf16* wh, const __bf16* wl) {
    switch (K) {
        case 16: mlp_ntile<16>(acc, xh, xl, xp, nt, wh, wl); break;
        case 32: mlp_ntile<32>(acc, xh, xl, xp, nt, wh, wl); break;
        case 48: mlp_ntile<48>(acc, xh, xl, xp, nt, wh, wl); break;
        default: mlp_ntile<64>(acc, xh, xl, xp, nt, wh, wl); break;
    }
}

// epilogue to LDS rows: relu(acc + bias) as bf16 hi/lo, N tile `nt`, both M tiles
__device__ __forceinline__ void store_hidden(const df32x16 (&acc)[2], int nt, const float* __restrict__ bias,
                                             __bf16* __restrict__ yh, __bf16* __restrict__ yl) {
    const int lane = threadIdx.x & 63, c = lane & 31, h = lane >> 5;
    const int col = 32 * nt + c;
    const float b = bias[col];
#pragma unroll
    for (int mt = 0; mt < 2; ++mt)
#pragma unroll
        for (int q = 0; q < 16; ++q) {
            const int row = row_of(mt, q, h);
            const float v = fmaxf(acc[mt][q] + b, 0.0f);
            __bf16 hi, lo;
            dsplit(v, hi, lo);
            yh[row * DAP + col] = hi;
            yl[row * DAP + col] = lo;
        }
}

// The heads with at most DEF_SMALL_OUT outputs (pos, scales, rotations, opacity: 3 / 3 / 4 / 1) take
// G W2 and G^T relu(Z1) on the VALU from fp32 G rows (a float4 per row in LDS, read as a
// broadcast by the half-wave that holds the row): as 64-padded MFMA products they were 61 / 64
// zeros, with their weight fragments re-read from L2 every tile.
constexpr int DEF_SMALL_OUT = 4;
// W2 rows 0..3 of column c as fp32 (hi + lo of the forward pack; rows past nout are the pack's zeros)
__device__ __forceinline__ void w2_column(const __bf16* w2h, const __bf16* w2l, int c, float (&w)[DEF_SMALL_OUT]) {
#pragma unroll
    for (int k = 0; k < DEF_SMALL_OUT; ++k) w[k] = (float)w2h[k * DWID + c] + (float)w2l[k * DWID + c];
}

constexpr int DGP = 64 + 8;   // LDS row pitch (bf16) of the upstream-gradient rows (K padded to 64)

}  // namespace lsr
