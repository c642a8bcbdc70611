// deform_field.h -- what both shapes of the deformation field (deform.hip: 16 channels / width 128,
// deform_narrow.hip: 32 / 64) compute the same way.  A is the shape's kernel argument struct
// (means3D, time, aabb, pw, ph).
#pragma once
#include <hip/hip_runtime.h>

namespace lsr {

// normalised aabb coordinates + time of Gaussian g (normalize_aabb: (p - aabb[0]) * (2 / (aabb[1] -
// aabb[0])) - 1, aabb = [xyz_max, xyz_min])
template <class A>
__device__ __forceinline__ void coords(const A& a, int g, float (&crd)[4]) {
#pragma unroll
    for (int c = 0; c < 3; ++c)
        crd[c] = (a.means3D[3 * g + c] - a.aabb[c]) * (2.0f / (a.aabb[3 + c] - a.aabb[c])) - 1.0f;
    crd[3] = a.time[g];
}
// coordinate pair (c0, c1) of plane combo ci: xy, xz, xt, yz, yt, zt.  Functions, not a table: the
// unrolled loops index the coordinate arrays with compile-time constants (a table in constant
// memory would send those arrays to scratch).
__device__ constexpr int kC0(int ci) { return ci < 3 ? 0 : (ci < 5 ? 1 : 2); }
__device__ constexpr int kC1(int ci) { return ci == 0 ? 1 : (ci == 1 || ci == 3) ? 2 : 3; }

struct Tap {
    int x0, x1, y0, y1;
    float fx, fy;
};
// bilinear tap of plane pi at the coordinate pair of combo ci (grid_sample, align_corners, border)
template <class A>
__device__ __forceinline__ Tap tap_of(const A& a, int pi, int ci, const float (&crd)[4]) {
    const int W = a.pw[pi], H = a.ph[pi];
    const float ix = fminf(fmaxf((crd[kC0(ci)] + 1.0f) * 0.5f * (float)(W - 1), 0.0f), (float)(W - 1));
    const float iy = fminf(fmaxf((crd[kC1(ci)] + 1.0f) * 0.5f * (float)(H - 1), 0.0f), (float)(H - 1));
    Tap t;
    t.x0 = (int)floorf(ix); t.y0 = (int)floorf(iy);
    t.x1 = min(t.x0 + 1, W - 1); t.y1 = min(t.y0 + 1, H - 1);
    t.fx = ix - (float)t.x0; t.fy = iy - (float)t.y0;
    return t;
}

// The quaternion product of batch_quaternion_multiply (utils/graphics_utils.py:121-124)
__device__ __forceinline__ float4 quat_mul(const float4 a, const float4 b) {
    return make_float4(a.x * b.x - a.y * b.y - a.z * b.z - a.w * b.w, a.x * b.y + a.y * b.x + a.z * b.w - a.w * b.z,
                       a.x * b.z - a.y * b.w + a.z * b.x + a.w * b.y, a.x * b.w + a.y * b.z - a.z * b.y + a.w * b.x);
}

// Gradient of the rotation head's output under apply_rotation, Gaussian g: out = p / |p|,
// p = q1 (x) q2 with q2 = d_rot; dp = (d - out (out . d)) / |p|; d/dq1_k of sum(p dp) =
// quat_mul(e_k, q2) . dp, likewise q2.  Writes d_rotations (the input's gradient) and the head
// output's gradient (sG_rot, the upstream of the head's backward), which it returns.  B: the shape's
// backward arguments (up, d_rotations, sG_rot); rotations: the head's input.
template <class B>
__device__ __forceinline__ float4 quat_grad(const B& b, const float* rotations, int g, const float* dr) {
    const float4 q1 = reinterpret_cast<const float4*>(rotations)[g];
    const float4 q2 = make_float4(dr[0], dr[1], dr[2], dr[3]);
    const float4 p = quat_mul(q1, q2);
    const float inv = 1.0f / sqrtf(p.x * p.x + p.y * p.y + p.z * p.z + p.w * p.w);
    const float4 d = reinterpret_cast<const float4*>(b.up[2])[g];
    const float4 o = make_float4(p.x * inv, p.y * inv, p.z * inv, p.w * inv);
    const float od = o.x * d.x + o.y * d.y + o.z * d.z + o.w * d.w;
    const float4 dp = make_float4((d.x - o.x * od) * inv, (d.y - o.y * od) * inv, (d.z - o.z * od) * inv,
                                  (d.w - o.w * od) * inv);
    float d1[4], d2[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const float4 ek = make_float4(k == 0, k == 1, k == 2, k == 3);
        const float4 u = quat_mul(ek, q2), w = quat_mul(q1, ek);
        d1[k] = u.x * dp.x + u.y * dp.y + u.z * dp.z + u.w * dp.w;
        d2[k] = w.x * dp.x + w.y * dp.y + w.z * dp.z + w.w * dp.w;
    }
    reinterpret_cast<float4*>(b.d_rotations)[g] = make_float4(d1[0], d1[1], d1[2], d1[3]);
    const float4 G = make_float4(d2[0], d2[1], d2[2], d2[3]);
    reinterpret_cast<float4*>(b.sG_rot)[g] = G;
    return G;
}

}  // namespace lsr
