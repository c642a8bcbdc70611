// deform_narrow.h -- the 32-channel / 64-wide deformation field (deform_narrow.hip): the host entry
// points deform_api.hip hands a checked net of that shape to (include/lsr_deform.h semantics).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/lsr_deform.h"

namespace lsr {

constexpr int NARROW_CHANNELS = 32;   // output_coordinate_dim
constexpr int NARROW_WIDTH = 64;      // net_width

inline bool deform_is_narrow(const lsr_deform_net* n) {
    return n->channels == NARROW_CHANNELS && n->width == NARROW_WIDTH;
}

// every function takes a net that deform_api.hip's check() passed (PASS language mode, heads 0..4)
int64_t narrow_workspace_bytes(const lsr_deform_net* net);
void narrow_prepare(const lsr_deform_net* net, void* workspace, hipStream_t st);
void narrow_forward(const lsr_deform_net* net, const void* workspace, int32_t P, const float* means3D,
                    const float* time, const float* const (&in)[5], float* const (&out)[5], hipStream_t st);
int64_t narrow_backward_scratch_bytes(const lsr_deform_net* net, int64_t P);
// hipSuccess, or the error of the scratch memset
hipError_t narrow_backward(const lsr_deform_net* net, const void* workspace, int32_t P, const float* means3D,
                           const float* rotations, const float* time, const float* const (&up)[5], float* d_means3D,
                           float* d_rotations, const lsr_deform_grads* grads, void* scratch, hipStream_t st);

}  // namespace lsr
