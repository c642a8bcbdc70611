// lsr_wave.h -- device helpers that the units outside the rasterizer share: the full-wave sum and the
// LDS address space.  (The compositors' and the sort's reductions are other trees or DPP: lsr_common.h.)
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

// LDS pointers carry their address space: through a generic pointer the reads become flat loads, whose
// wait (vmcnt and lgkmcnt) also waits for the global loads in flight
#define LSR_LDS __attribute__((address_space(3)))

namespace lsr {

typedef LSR_LDS float lds_float;
typedef LSR_LDS uint8_t lds_byte;

// the sum over the 64 lanes, in every lane: a fixed tree (partners 32, 16, ... 1 lanes away).  The
// kernels that still spell this loop out (train.hip, k_seg_mean's count, centers_kmeans.h, the
// deformation backward kernels) compile to other code through the call (registers, instruction order:
// profiles/host_wave_fold), so they keep theirs.
template <typename T>
__device__ __forceinline__ T wave_sum(T v) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off);
    return v;
}

}  // namespace lsr
