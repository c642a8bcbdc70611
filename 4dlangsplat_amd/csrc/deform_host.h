// deform_host.h -- host-side geometry of the deformation field that both shapes share (deform_api.hip:
// 16 channels / width 128; deform_narrow.hip: 32 / 64): plane pairs and sizes, the channel-last plane
// layout of a workspace, layers and heads.
#pragma once
#include <algorithm>

#include "../../include/lsr_deform.h"
#include "deform_internal.h"
#include "lsr_host.h"

namespace lsr {
namespace deform_host {

constexpr int kCombos[6][2] = {{0, 1}, {0, 2}, {0, 3}, {1, 2}, {1, 3}, {2, 3}};   // xy, xz, xt, yz, yt, zt
constexpr int kHeadOut[5] = {3, 3, 4, 1, 48};   // pos, scales, rotations, opacity, shs

inline int nlayers(const lsr_deform_net* n) { return std::max(n->depth, 1); }
inline bool head_on(const lsr_deform_net* n, int hd) { return (n->heads >> hd) & 1u; }

// plane 6 s + ci: width (along coordinate c0) and height (along c1)
inline void plane_dims(const lsr_deform_net* n, int s, int ci, int& W, int& H) {
    auto res = [&](int c) { return c < 3 ? n->res[c] * n->multires[s] : n->res[3]; };
    W = res(kCombos[ci][0]);
    H = res(kCombos[ci][1]);
}

// the planes channel-last ([H][W][channels] floats) at the head of a workspace: byte offsets, 256-byte aligned
struct PlaneLayout {
    size_t off[24], end;
};
inline PlaneLayout plane_layout(const lsr_deform_net* n, int channels) {
    PlaneLayout L{};
    Carver c;
    for (int s = 0; s < n->n_scales; ++s)
        for (int ci = 0; ci < 6; ++ci) {
            int W, H;
            plane_dims(n, s, ci, W, H);
            L.off[6 * s + ci] = c.skip((size_t)W * H * channels * sizeof(float));
        }
    L.end = c.total();
    return L;
}
// the kernels' view of them: float offsets, widths and heights
inline void plane_args(const lsr_deform_net* n, const PlaneLayout& L, int64_t* poff, int* pw, int* ph) {
    for (int s = 0; s < n->n_scales; ++s)
        for (int ci = 0; ci < 6; ++ci) {
            plane_dims(n, s, ci, pw[6 * s + ci], ph[6 * s + ci]);
            poff[6 * s + ci] = (int64_t)(L.off[6 * s + ci] / sizeof(float));
        }
}
// the unpack's view: plane j = 6 s + ci at its offset into its gradient, one block per 256 / channels texels
inline void unpack_planes(const lsr_deform_net* n, const PlaneLayout& L, int channels, const lsr_deform_grads* grads,
                          UnpackBatch& u) {
    plane_args(n, L, u.off, u.W, u.H);
    const int tex = 256 / channels;
    for (u.n = 0; u.n < 6 * n->n_scales; ++u.n) {
        u.dst[u.n] = grads->planes[u.n / 6][u.n % 6];
        u.block0[u.n + 1] = u.block0[u.n] + (u.H[u.n] * u.W[u.n] + tex - 1) / tex;
        u.toff[u.n] = -1;
    }
}

}  // namespace deform_host
}  // namespace lsr
