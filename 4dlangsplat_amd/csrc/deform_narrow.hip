// deform_narrow.hip -- the deformation field at 32 plane channels per scale and a 64-wide MLP (the
// reference's D-NeRF configs and its ModelHiddenParams defaults), language passed through.  Same
// semantics as deform.hip (include/lsr_deform.h); its own kernels, so the 16 / 128 family is untouched.
// What the two shapes compute the same way is shared: deform_field.h (device), deform_host.h (host).
//
// One block of 256 threads per 64 Gaussians, everything in fp32:
//   features: 4 threads per Gaussian, each owning 8 of a plane's 32 channels (planes packed
//     channel-last [H][W][32]: a bilinear tap is two float4 per thread, a Gaussian's tap one 128-byte
//     line); the six planes of a scale multiply, the S scales concatenate (32 S features).
//   MLP: the block's activation rows live in LDS transposed ([k][row], pitch NXP) and a layer is a
//     64 x 64 tile product on the VALU: thread (tr, tc) owns rows 4 tr.. and columns 4 tc.., reads one
//     float4 of activations (LDS, a broadcast across the 16 threads of a row group) and one float4 of
//     weights ([k][col] rows: 256 contiguous bytes per 16 threads, L1 / L2 resident) per 16 explicit
//     FMAs.  The forward reads weights transposed by lsr_deform_prepare ([in][out]); the backward's
//     data gradients (dY W) read the torch layout [out][in], which is already [k][col] for them.
//   backward: recompute, saved rows (features, chain activations and gradients, every head's
//     relu(Z1) and dZ1) for the weight gradients, which are the A^T B products of deform_wgrad.hip's
//     launch_atb (bf16 hi / lo on the matrix core, split-K over row blocks); the plane gradients are
//     float atomics into a channel-last copy (a Gaussian's tap: 32 channels = one 128-byte line; a
//     wave stages its 16 Gaussians in LDS so that one atomic instruction adds two whole lines),
//     transposed and added into the torch layout by deform_pack.hip's k_unpack_planes<32>.
// Every global read stays inside its tensor for S = 1..4: a tile product loads only the columns its
// weight has (ngemm's ncol: dX = dH_0 W_0 has 32 S columns, 32 or 96 of them no multiple of the
// 64-column tile), K runs over the weight's own rows, and row indices are clamped to P - 1.
#include "lsr_common.h"
#include "deform_field.h"
#include "deform_host.h"
#include "deform_narrow.h"

namespace lsr {

constexpr int NB = 64;            // Gaussians per block
constexpr int NC = NARROW_CHANNELS;
constexpr int NW = NARROW_WIDTH;
constexpr int NXP = NB + 4;       // LDS pitch (floats) of a transposed activation row
constexpr int NFMAX = NC * LSR_DEFORM_MAX_SCALES;   // 128 features at most
constexpr int NHEADS = 5;         // pos, scales, rotations, opacity, shs (no coff head: PASS only)

struct NarrowArgs {
    int P, S, nlayers;
    uint32_t heads;
    int apply_rotation;
    const float* means3D;
    const float* time;
    const float* aabb;
    const float* planes;              // packed channel-last [H][W][32]
    int64_t poff[24];                 // float offset of plane 6 s + ci
    int pw[24], ph[24];
    const float* wf_t[DEF_MAX_LAYERS];   // feature_out layer k transposed [K_k][64]
    const float* w1_t[NHEADS];           // [64 in][64 out]
    const float* w2_t[NHEADS];           // [64 in][64 out, zero padded]
    const float* wf[DEF_MAX_LAYERS];     // torch layouts (the net's own tensors)
    const float* w1[NHEADS];
    const float* w2[NHEADS];
    const float* b_feat[DEF_MAX_LAYERS];
    const float* b1[NHEADS];
    const float* b2[NHEADS];
    const float* in[NHEADS];
    float* out[NHEADS];
    // backward
    const float* up[NHEADS];
    float* d_means3D;
    float* d_rotations;
    float* sX;                        // saved [P, 32 S]
    float* sA[DEF_MAX_LAYERS];        // saved [P, 64] relu(H_k)
    float* sdH[DEF_MAX_LAYERS];       // saved [P, 64] gradients of H_k
    float* sR[NHEADS];                // saved [P, 64] relu(Z1) of head h
    float* sdZ[NHEADS];               // saved [P, 64] gradient of Z1
    float* sG_rot;                    // apply_rotation: [P, 4] gradient of the rotation head's output
    float* dplanes;                   // channel-last gradient planes (offsets as planes), zeroed per call
    float* daabb_part;                // [DEF_AABB_SLOTS][16], zeroed per call; null: no box gradient
};

__device__ __forceinline__ int nhead_out(int hd) { return hd < 2 ? 3 : hd == 2 ? 4 : hd == 3 ? 1 : 48; }

struct NTap {
    int o00, o01, o10, o11;   // float offsets of the four texels' channel 0
    float fx, fy;
};
// the bilinear tap of deform_field.h's tap_of as offsets into a [H][W][32] plane
__device__ __forceinline__ NTap ntap_of(const NarrowArgs& a, int pi, int ci, const float (&crd)[4]) {
    const Tap t = tap_of(a, pi, ci, crd);
    const int W = a.pw[pi];
    return NTap{(t.y0 * W + t.x0) * NC, (t.y0 * W + t.x1) * NC, (t.y1 * W + t.x0) * NC, (t.y1 * W + t.x1) * NC, t.fx, t.fy};
}
struct NTexels {
    float v00[8], v01[8], v10[8], v11[8];
};
__device__ __forceinline__ void nload8(const float* p, float (&v)[8]) {
    const float4 lo = *reinterpret_cast<const float4*>(p), hi = *reinterpret_cast<const float4*>(p + 4);
    v[0] = lo.x; v[1] = lo.y; v[2] = lo.z; v[3] = lo.w;
    v[4] = hi.x; v[5] = hi.y; v[6] = hi.z; v[7] = hi.w;
}
__device__ __forceinline__ void ntexels(const NarrowArgs& a, int pi, const NTap& t, int q, NTexels& x) {
    const float* pl = a.planes + a.poff[pi] + 8 * q;
    nload8(pl + t.o00, x.v00); nload8(pl + t.o01, x.v01);
    nload8(pl + t.o10, x.v10); nload8(pl + t.o11, x.v11);
}
// the weighted tap sum, left to right as the reference's
__device__ __forceinline__ void nsample8(const NTexels& x, const NTap& t, float (&v)[8]) {
    const float ufx = 1.0f - t.fx, ufy = 1.0f - t.fy;
    const float w00 = ufx * ufy, w01 = t.fx * ufy, w10 = ufx * t.fy, w11 = t.fx * t.fy;
#pragma unroll
    for (int i = 0; i < 8; ++i) v[i] = ((x.v00[i] * w00 + x.v01[i] * w01) + x.v10[i] * w10) + x.v11[i] * w11;
}

// the block's features into LDS, transposed ([feature][row]); optionally saved as [P, 32 S]
__device__ __forceinline__ void nfeatures(const NarrowArgs& a, int g0, float* s_x, float* save) {
    const int tid = threadIdx.x, gl = tid >> 2, q = tid & 3;
    const int g = min(g0 + gl, a.P - 1);
    float crd[4];
    coords(a, g, crd);
    for (int s = 0; s < a.S; ++s) {
        float prod[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) prod[i] = 1.0f;
#pragma unroll
        for (int ci = 0; ci < 6; ++ci) {
            const int pi = 6 * s + ci;
            const NTap t = ntap_of(a, pi, ci, crd);
            NTexels x;
            ntexels(a, pi, t, q, x);
            float v[8];
            nsample8(x, t, v);
#pragma unroll
            for (int i = 0; i < 8; ++i) prod[i] *= v[i];
        }
#pragma unroll
        for (int i = 0; i < 8; ++i) s_x[(NC * s + 8 * q + i) * NXP + gl] = prod[i];
        if (save && g0 + gl < a.P) {
            float* dst = save + (size_t)(g0 + gl) * (NC * a.S) + NC * s + 8 * q;
            *reinterpret_cast<float4*>(dst) = make_float4(prod[0], prod[1], prod[2], prod[3]);
            *reinterpret_cast<float4*>(dst + 4) = make_float4(prod[4], prod[5], prod[6], prod[7]);
        }
    }
}

// acc[i][j] += sum_k xt[k][4 tr + i] wt[k][4 tc + j]: the 64 x 64 tile of the block, K deep.  wt has
// ncol columns (a multiple of 4): a thread whose columns lie past them loads nothing and keeps its acc.
__device__ __forceinline__ void ngemm(float (&acc)[4][4], const float* xt, const float* __restrict__ wt, int ldw, int K,
                                      int ncol = NW) {
    const int tr = threadIdx.x >> 4, tc = threadIdx.x & 15;
    if (4 * tc >= ncol) return;
    const float* xp = xt + 4 * tr;
    const float* wp = wt + 4 * tc;
#pragma unroll 4
    for (int k = 0; k < K; ++k) {
        const float4 x4 = *reinterpret_cast<const float4*>(xp + k * NXP);
        const float4 w4 = *reinterpret_cast<const float4*>(wp + (size_t)k * ldw);
        const float x[4] = {x4.x, x4.y, x4.z, x4.w}, w[4] = {w4.x, w4.y, w4.z, w4.w};
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[i][j] = fmaf(x[i], w[j], acc[i][j]);
    }
}
__device__ __forceinline__ void nzero(float (&acc)[4][4]) {
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = 0.0f;
}
// the thread's tile into a transposed LDS buffer
__device__ __forceinline__ void nstore_t(const float (&v)[4][4], float* dst) {
    const int tr = threadIdx.x >> 4, tc = threadIdx.x & 15;
#pragma unroll
    for (int j = 0; j < 4; ++j)
        *reinterpret_cast<float4*>(dst + (4 * tc + j) * NXP + 4 * tr) = make_float4(v[0][j], v[1][j], v[2][j], v[3][j]);
}
// the thread's tile into rows [P, 64] of global memory
__device__ __forceinline__ void nsave_rows(const float (&v)[4][4], float* dst, int g0, int P) {
    const int tr = threadIdx.x >> 4, tc = threadIdx.x & 15;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int g = g0 + 4 * tr + i;
        if (g < P) *reinterpret_cast<float4*>(dst + (size_t)g * NW + 4 * tc) = make_float4(v[i][0], v[i][1], v[i][2], v[i][3]);
    }
}
// v = relu(acc + bias); returns bit 4 i + j = v > 0
__device__ __forceinline__ uint32_t nbias_relu(float (&v)[4][4], const float* __restrict__ bias) {
    const int tc = threadIdx.x & 15;
    const float4 b4 = *reinterpret_cast<const float4*>(bias + 4 * tc);
    const float b[4] = {b4.x, b4.y, b4.z, b4.w};
    uint32_t m = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            v[i][j] = fmaxf(v[i][j] + b[j], 0.0f);
            m |= v[i][j] > 0.0f ? 1u << (4 * i + j) : 0u;
        }
    return m;
}
// a head of at most 4 outputs: thread (row = tid / 4, c = tid % 4) takes one output from the hidden
// rows in LDS and the torch-layout W2 [nout][64]
__device__ __forceinline__ float nsmall_out(const float* ht, const float* __restrict__ w2, const float* __restrict__ b2,
                                            int nout) {
    const int row = threadIdx.x >> 2, c = threadIdx.x & 3;
    if (c >= nout) return 0.0f;
    float s = 0.0f;
#pragma unroll 8
    for (int k = 0; k < NW; ++k) s = fmaf(ht[k * NXP + row], w2[c * NW + k], s);
    return s + b2[c];
}

__global__ void __launch_bounds__(256) k_narrow_fwd(const NarrowArgs a) {
    __shared__ __attribute__((aligned(16))) float s_x[NFMAX * NXP];
    __shared__ __attribute__((aligned(16))) float s_h[2][NW * NXP];
    __shared__ __attribute__((aligned(16))) float s_q[NB][4];
    const int tid = threadIdx.x, tr = tid >> 4, tc = tid & 15;
    const int g0 = blockIdx.x * NB;

    nfeatures(a, g0, s_x, nullptr);
    __syncthreads();

    // feature_out chain
    int cur = 0;
    for (int k = 0; k < a.nlayers; ++k) {
        float acc[4][4];
        nzero(acc);
        if (k == 0) ngemm(acc, s_x, a.wf_t[0], NW, NC * a.S);
        else ngemm(acc, s_h[cur], a.wf_t[k], NW, NW);
        nbias_relu(acc, a.b_feat[k]);
        const int dst = k == 0 ? 0 : cur ^ 1;
        nstore_t(acc, s_h[dst]);
        __syncthreads();
        cur = dst;
    }
    const float* hid = s_h[cur];
    float* hb = s_h[cur ^ 1];

    // heads: out = in + relu(hidden W1^T + b1) W2^T + b2
    for (int hd = 0; hd < NHEADS; ++hd) {
        if (!((a.heads >> hd) & 1u)) continue;   // block-uniform
        const int nout = nhead_out(hd);
        const bool quat = hd == 2 && a.apply_rotation;
        {
            float acc[4][4];
            nzero(acc);
            ngemm(acc, hid, a.w1_t[hd], NW, NW);
            nbias_relu(acc, a.b1[hd]);
            nstore_t(acc, hb);
        }
        __syncthreads();
        if (nout > 4) {   // the SH head: a tile product against the zero-padded transposed W2
            float acc[4][4];
            nzero(acc);
            ngemm(acc, hb, a.w2_t[hd], NW, NW);
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int g = g0 + 4 * tr + i;
                if (g < a.P && 4 * tc < nout) {
                    const size_t o = (size_t)g * nout + 4 * tc;
                    const float4 r = *reinterpret_cast<const float4*>(a.in[hd] + o);
                    const float4 b = *reinterpret_cast<const float4*>(a.b2[hd] + 4 * tc);
                    *reinterpret_cast<float4*>(a.out[hd] + o) = make_float4(r.x + (acc[i][0] + b.x), r.y + (acc[i][1] + b.y),
                                                                            r.z + (acc[i][2] + b.z), r.w + (acc[i][3] + b.w));
                }
            }
        } else {
            const int row = tid >> 2, c = tid & 3, g = g0 + row;
            const float v = nsmall_out(hb, a.w2[hd], a.b2[hd], nout);
            if (quat) s_q[row][c] = v;
            else if (c < nout && g < a.P) a.out[hd][(size_t)g * nout + c] = a.in[hd][(size_t)g * nout + c] + v;
        }
        __syncthreads();   // the hidden rows read (and s_q complete) before they are reused
        if (quat && tid < NB && g0 + tid < a.P) {   // rotations = normalize(rotations (x) d_rot)
            const int g = g0 + tid;
            const float4 q1 = reinterpret_cast<const float4*>(a.in[2])[g];
            const float4 p = quat_mul(q1, make_float4(s_q[tid][0], s_q[tid][1], s_q[tid][2], s_q[tid][3]));
            const float inv = 1.0f / sqrtf(p.x * p.x + p.y * p.y + p.z * p.z + p.w * p.w);
            reinterpret_cast<float4*>(a.out[2])[g] = make_float4(p.x * inv, p.y * inv, p.z * inv, p.w * inv);
        }
    }
}

// Backward phase A.  LDS: the feature rows' buffer holds, in turn, the features (read by the first
// layer only), a head's upstream rows G (transposed, at most 48), and dX; every hand-over is a
// __syncthreads.
__global__ void __launch_bounds__(256) k_narrow_bwd(const NarrowArgs a) {
    __shared__ __attribute__((aligned(16))) float s_x[NFMAX * NXP];
    __shared__ __attribute__((aligned(16))) float s_h[2][NW * NXP];
    __shared__ __attribute__((aligned(16))) float s_q[NB][4];
    float* const s_g = s_x;
    const int tid = threadIdx.x;
    const int g0 = blockIdx.x * NB;
    const int F = NC * a.S;

    nfeatures(a, g0, s_x, a.sX);
    __syncthreads();

    // chain forward, A_k = relu(H_k) saved; bits 16 k + 4 i + j of amask: A_k > 0
    int cur = 0;
    uint64_t amask = 0;
    for (int k = 0; k < a.nlayers; ++k) {
        float acc[4][4];
        nzero(acc);
        if (k == 0) ngemm(acc, s_x, a.wf_t[0], NW, F);
        else ngemm(acc, s_h[cur], a.wf_t[k], NW, NW);
        amask |= (uint64_t)nbias_relu(acc, a.b_feat[k]) << (16 * k);
        nsave_rows(acc, a.sA[k], g0, a.P);
        const int dst = k == 0 ? 0 : cur ^ 1;
        nstore_t(acc, s_h[dst]);
        __syncthreads();
        cur = dst;
    }
    const float* hid = s_h[cur];
    float* hb = s_h[cur ^ 1];

    float dA[4][4];
    nzero(dA);
    for (int hd = 0; hd < NHEADS; ++hd) {
        if (!((a.heads >> hd) & 1u)) continue;   // block-uniform
        const int nout = nhead_out(hd);
        const bool quat = hd == 2 && a.apply_rotation;
        uint32_t zmask;
        {
            float z[4][4];
            nzero(z);
            ngemm(z, hid, a.w1_t[hd], NW, NW);
            zmask = nbias_relu(z, a.b1[hd]);
            nsave_rows(z, a.sR[hd], g0, a.P);
            if (quat) nstore_t(z, hb);
        }
        if (quat) {
            // the head's output again, then the quaternion product's gradient as its upstream
            __syncthreads();
            s_q[tid >> 2][tid & 3] = nsmall_out(hb, a.w2[hd], a.b2[hd], nout);
            __syncthreads();
            if (tid < NB) {
                const int g = g0 + tid;
                float4 G = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
                if (g < a.P) G = quat_grad(a, a.in[2], g, s_q[tid]);   // deform_field.h
                s_g[0 * NXP + tid] = G.x; s_g[1 * NXP + tid] = G.y;
                s_g[2 * NXP + tid] = G.z; s_g[3 * NXP + tid] = G.w;
            }
        } else {
            for (int i = tid; i < NB * nout; i += 256) {
                const int row = i / nout, n = i - row * nout, g = g0 + row;
                s_g[n * NXP + row] = g < a.P ? a.up[hd][(size_t)g * nout + n] : 0.0f;
            }
        }
        __syncthreads();   // G rows complete (and, quat, the hidden rows read)
        {
            // dZ1 = (G W2) [Z1 > 0]
            float dz[4][4];
            nzero(dz);
            ngemm(dz, s_g, a.w2[hd], NW, nout);
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) dz[i][j] = (zmask >> (4 * i + j)) & 1u ? dz[i][j] : 0.0f;
            nsave_rows(dz, a.sdZ[hd], g0, a.P);
            nstore_t(dz, hb);
        }
        __syncthreads();
        ngemm(dA, hb, a.w1[hd], NW, NW);   // dA += dZ1 W1
        __syncthreads();                    // dZ1 and G rows read before the next head rewrites them
    }

    // chain backward: dH_k = dA_k [A_k > 0] (saved), dA_{k-1} = dH_k W_k, dX = dH_0 W_0
    float* bd = hb;
    float* bo = s_h[cur];
    for (int k = a.nlayers - 1; k >= 0; --k) {
        const uint32_t m = (uint32_t)(amask >> (16 * k)) & 0xFFFFu;
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) dA[i][j] = (m >> (4 * i + j)) & 1u ? dA[i][j] : 0.0f;
        nsave_rows(dA, a.sdH[k], g0, a.P);
        nstore_t(dA, bd);
        __syncthreads();
        if (k > 0) {
            nzero(dA);
            ngemm(dA, bd, a.wf[k], NW, NW);
            float* t = bd; bd = bo; bo = t;
        } else {
            for (int c0 = 0; c0 < F; c0 += NW) {
                float dx[4][4];
                nzero(dx);
                ngemm(dx, bd, a.wf[0] + c0, F, NW, F - c0);   // W_0 is [64][F]: F - c0 columns are left
                nstore_t(dx, s_x + c0 * NXP);
            }
        }
    }
    __syncthreads();

    // HexPlane backward, 4 threads per Gaussian (8 channels each): each plane's sample gets dX times
    // the product of the other five planes of its scale, scattered to its 4 taps; the coordinate
    // gradient (zero where the border clips) goes to d_means3D
    const int gl = tid >> 2, q = tid & 3;
    const bool ok = g0 + gl < a.P;
    const int g = min(g0 + gl, a.P - 1);
    float crd[4];
    coords(a, g, crd);
    float dq[3] = {0.0f, 0.0f, 0.0f};
    // scatter staging, per wave, in the first hidden buffer (dead since the chain backward's last
    // barrier): the wave's 16 Gaussians' dv rows (32 channels, pitch NSP), tap offsets and weights
    constexpr int NSP = NC + 1, NSTAGE = 16 * NSP + 2 * 16 * 4;
    static_assert(4 * NSTAGE <= NW * NXP, "scatter staging fits one hidden buffer");
    const int wave = tid >> 6, lane = tid & 63, wl = gl & 15;
    float* const sdv = s_h[0] + wave * NSTAGE;
    int* const soff = reinterpret_cast<int*>(sdv + 16 * NSP);
    float* const sw = sdv + 16 * NSP + 16 * 4;
    for (int s = 0; s < a.S; ++s) {
        float v[6][8];
#pragma unroll
        for (int ci = 0; ci < 6; ++ci) {
            const int pi = 6 * s + ci;
            const NTap t = ntap_of(a, pi, ci, crd);
            NTexels x;
            ntexels(a, pi, t, q, x);
            nsample8(x, t, v[ci]);
        }
        float dx[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) dx[i] = s_x[(NC * s + 8 * q + i) * NXP + gl];
#pragma unroll
        for (int ci = 0; ci < 6; ++ci) {
            const int pi = 6 * s + ci;
            const int W = a.pw[pi], H = a.ph[pi];
            const NTap t = ntap_of(a, pi, ci, crd);
            NTexels x;
            ntexels(a, pi, t, q, x);
            const float ufx = 1.0f - t.fx, ufy = 1.0f - t.fy;
            const float w00 = ufx * ufy, w01 = t.fx * ufy, w10 = ufx * t.fy, w11 = t.fx * t.fy;
            float dix = 0.0f, diy = 0.0f;
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                float oth = 1.0f;
#pragma unroll
                for (int cj = 0; cj < 6; ++cj)
                    if (cj != ci) oth *= v[cj][i];
                const float dv = ok ? dx[i] * oth : 0.0f;
                dix += dv * ((x.v01[i] - x.v00[i]) * ufy + (x.v11[i] - x.v10[i]) * t.fy);
                diy += dv * ((x.v10[i] - x.v00[i]) * ufx + (x.v11[i] - x.v01[i]) * t.fx);
                sdv[wl * NSP + 8 * q + i] = dv;
            }
            if (q == 0) {
                soff[wl * 4 + 0] = t.o00; soff[wl * 4 + 1] = t.o01; soff[wl * 4 + 2] = t.o10; soff[wl * 4 + 3] = t.o11;
                sw[wl * 4 + 0] = w00; sw[wl * 4 + 1] = w01; sw[wl * 4 + 2] = w10; sw[wl * 4 + 3] = w11;
            }
            wave_lds_sync();
            {
                // lane = (tap of a pair, channel): one atomic instruction adds two whole 128-byte texels
                float* gp = a.dplanes + a.poff[pi];
                const int half = lane >> 5, ch = lane & 31;
#pragma unroll 4
                for (int j = 0; j < 16; ++j) {
                    const float dvj = sdv[j * NSP + ch];
#pragma unroll
                    for (int tp = 0; tp < 2; ++tp) {
                        const int tap = 2 * tp + half;
                        const float val = dvj * sw[j * 4 + tap];
                        if (val != 0.0f) atomicAdd(gp + soff[j * 4 + tap] + ch, val);
                    }
                }
            }
            wave_lds_sync();   // staging read before the next plane rewrites it
            const float rx = (crd[kC0(ci)] + 1.0f) * 0.5f * (float)(W - 1);
            const float ry = (crd[kC1(ci)] + 1.0f) * 0.5f * (float)(H - 1);
            if (kC0(ci) < 3 && rx > 0.0f && rx < (float)(W - 1)) dq[kC0(ci)] += dix * 0.5f * (float)(W - 1);
            if (kC1(ci) < 3 && ry > 0.0f && ry < (float)(H - 1)) dq[kC1(ci)] += diy * 0.5f * (float)(H - 1);
        }
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        dq[c] += __shfl_xor(dq[c], 1);
        dq[c] += __shfl_xor(dq[c], 2);
    }
    if (ok && q == 0) {
        const size_t gg = (size_t)(g0 + gl);
#pragma unroll
        for (int c = 0; c < 3; ++c)
            a.d_means3D[3 * gg + c] = a.up[0][3 * gg + c] + dq[c] * (2.0f / (a.aabb[3 + c] - a.aabb[c]));
    }
    if (a.daabb_part) {   // block-uniform
        // normalize_aabb's gradient w.r.t. the box: with n = (p - a0) s - 1, s = 2 / (a1 - a0):
        // dn/da0 = s (n - 1) / 2, dn/da1 = -s (n + 1) / 2, and dq = dL/dn
        float bv[6];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float gq = (ok && q == 0) ? dq[c] * (2.0f / (a.aabb[3 + c] - a.aabb[c])) : 0.0f;
            bv[c] = 0.5f * gq * (crd[c] - 1.0f);
            bv[3 + c] = -0.5f * gq * (crd[c] + 1.0f);
        }
#pragma unroll
        for (int k = 0; k < 6; ++k) {
#pragma unroll
            for (int off = 32; off >= 1; off >>= 1) bv[k] += __shfl_xor(bv[k], off);
        }
        if ((tid & 63) == 0) {
            float* row = a.daabb_part + (blockIdx.x % DEF_AABB_SLOTS) * 16;
#pragma unroll
            for (int k = 0; k < 6; ++k) atomicAdd(row + k, bv[k]);
        }
    }
}

// db[c] += sum_g rows[g][c] over [P, 64] rows.  k_atb's bias sums ride on its N tiles: a product with
// fewer N tiles than M tiles (the first layer's weight gradient at one scale, [64] x [32]) leaves the
// upper M tile's bias out, so that one bias gets its own column sums.
constexpr int NCOLSUM_ROWS = 1024;
__global__ void __launch_bounds__(256) k_narrow_colsum(const float* __restrict__ rows, int P, float* __restrict__ db) {
    __shared__ float s_p[4][NW];
    const int c = threadIdx.x & 63, grp = threadIdx.x >> 6;
    const int64_t r0 = (int64_t)blockIdx.x * NCOLSUM_ROWS;
    const int64_t r1 = min((int64_t)P, r0 + NCOLSUM_ROWS);
    float s = 0.0f;
    for (int64_t r = r0 + grp; r < r1; r += 4) s += rows[r * NW + c];
    s_p[grp][c] = s;
    __syncthreads();
    if (grp == 0) atomicAdd(db + c, (s_p[0][c] + s_p[1][c]) + (s_p[2][c] + s_p[3][c]));
}

// ---- packing (lsr_deform_prepare): batched transposes ------------------------------------------
// dst[c][r] (pitch ld, a multiple of 32) = r < rows ? src[r][c] : 0 for c < cols, r < ld: planes
// [32][H W] -> [H W][32], Linear weights [out][in] -> [in][out pad].  A block transposes one 32 x 32
// tile through LDS: reads run along src rows, writes along dst rows.
struct NPackJob {
    const float* src;
    float* dst;
    int rows, cols, ld;
    uint32_t block0;                  // first block of the job
};
constexpr int NPACK_MAX = 24 + DEF_MAX_LAYERS + 2 * NHEADS;
struct NPackBatch {
    NPackJob j[NPACK_MAX];
    int n;
};
__global__ void __launch_bounds__(256) k_narrow_pack(const NPackBatch pb) {
    __shared__ float s_t[32][33];
    int ji = 0;
    while (ji + 1 < pb.n && blockIdx.x >= pb.j[ji + 1].block0) ++ji;
    const NPackJob& j = pb.j[ji];
    const int rt = j.ld / 32;                                  // tiles along r
    const uint32_t tile = blockIdx.x - j.block0;
    const int r0 = 32 * (int)(tile % rt), c0 = 32 * (int)(tile / rt);
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int r = r0 + ty + 8 * k, c = c0 + tx;
        s_t[ty + 8 * k][tx] = (r < j.rows && c < j.cols) ? j.src[(size_t)r * j.cols + c] : 0.0f;
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int c = c0 + ty + 8 * k, r = r0 + tx;
        if (c < j.cols) j.dst[(size_t)c * j.ld + r] = s_t[tx][ty + 8 * k];
    }
}

// ==== host =========================================================================================
namespace {

using namespace deform_host;   // plane sizes and layout, layers, heads: shared with the 16 / 128 shape

// workspace: the planes channel-last, then the transposed weights; byte offsets
struct NLayout {
    PlaneLayout planes;
    size_t wf_t[DEF_MAX_LAYERS], w1_t[NHEADS], w2_t[NHEADS];
    size_t total;
};
NLayout nlayout(const lsr_deform_net* n) {
    NLayout L{};
    L.planes = plane_layout(n, NC);
    Carver c;
    c.skip(L.planes.end);
    auto floats = [&](size_t count) { return c.skip(count * sizeof(float)); };
    for (int k = 0; k < nlayers(n); ++k) L.wf_t[k] = floats((size_t)(k == 0 ? NC * n->n_scales : NW) * NW);
    for (int hd = 0; hd < NHEADS; ++hd) {
        if (!head_on(n, hd)) continue;
        L.w1_t[hd] = floats((size_t)NW * NW);
        L.w2_t[hd] = floats((size_t)NW * NW);
    }
    L.total = c.total();
    return L;
}

struct NScratch {
    size_t X, A[DEF_MAX_LAYERS], dH[DEF_MAX_LAYERS], R[NHEADS], dZ[NHEADS], Grot, daabb, dplanes, total;
};
NScratch nscratch(const lsr_deform_net* n, size_t P) {
    NScratch s{};
    Carver c;
    auto floats = [&](size_t count) { return c.skip(count * sizeof(float)); };
    s.X = floats(P * NC * n->n_scales);
    for (int k = 0; k < nlayers(n); ++k) {
        s.A[k] = floats(P * NW);
        s.dH[k] = floats(P * NW);
    }
    for (int hd = 0; hd < NHEADS; ++hd) {
        if (!head_on(n, hd)) continue;
        s.R[hd] = floats(P * NW);
        s.dZ[hd] = floats(P * NW);
    }
    s.Grot = floats(n->apply_rotation ? P * 4 : 1);
    s.daabb = floats(DEF_AABB_SLOTS * 16);   // zeroed with the gradient planes (contiguous)
    s.dplanes = c.skip(plane_layout(n, NC).end);
    s.total = c.total();
    return s;
}

NarrowArgs nargs(const lsr_deform_net* net, const void* workspace, int32_t P) {
    const NLayout L = nlayout(net);
    const char* ws = reinterpret_cast<const char*>(workspace);
    auto fp = [&](size_t off) { return reinterpret_cast<const float*>(ws + off); };
    NarrowArgs a{};
    a.P = P;
    a.S = net->n_scales;
    a.nlayers = nlayers(net);
    a.heads = net->heads;
    a.apply_rotation = net->apply_rotation;
    a.aabb = net->aabb;
    a.planes = fp(0);
    plane_args(net, L.planes, a.poff, a.pw, a.ph);
    for (int k = 0; k < a.nlayers; ++k) {
        a.wf_t[k] = fp(L.wf_t[k]);
        a.wf[k] = net->w_feat[k];
        a.b_feat[k] = net->b_feat[k];
    }
    for (int hd = 0; hd < NHEADS; ++hd) {
        if (!head_on(net, hd)) continue;
        a.w1_t[hd] = fp(L.w1_t[hd]);
        a.w2_t[hd] = fp(L.w2_t[hd]);
        a.w1[hd] = net->w1[hd];
        a.w2[hd] = net->w2[hd];
        a.b1[hd] = net->b1[hd];
        a.b2[hd] = net->b2[hd];
    }
    return a;
}

}  // namespace

int64_t narrow_workspace_bytes(const lsr_deform_net* net) { return (int64_t)nlayout(net).total; }

void narrow_prepare(const lsr_deform_net* net, void* workspace, hipStream_t st) {
    const NLayout L = nlayout(net);
    char* ws = reinterpret_cast<char*>(workspace);
    NPackBatch pb{};
    uint32_t blocks = 0;
    auto job = [&](const float* src, size_t off, int rows, int cols, int ld) {
        NPackJob& j = pb.j[pb.n++];
        j.src = src;
        j.dst = reinterpret_cast<float*>(ws + off);
        j.rows = rows; j.cols = cols; j.ld = ld;
        j.block0 = blocks;
        blocks += (uint32_t)(ld / 32) * (uint32_t)((cols + 31) / 32);
    };
    for (int s = 0; s < net->n_scales; ++s)
        for (int ci = 0; ci < 6; ++ci) {
            int W, H;
            plane_dims(net, s, ci, W, H);
            job(net->planes[s][ci], L.planes.off[6 * s + ci], NC, W * H, NC);
        }
    for (int k = 0; k < nlayers(net); ++k) job(net->w_feat[k], L.wf_t[k], NW, k == 0 ? NC * net->n_scales : NW, NW);
    for (int hd = 0; hd < NHEADS; ++hd) {
        if (!head_on(net, hd)) continue;
        job(net->w1[hd], L.w1_t[hd], NW, NW, NW);
        job(net->w2[hd], L.w2_t[hd], kHeadOut[hd], NW, NW);
    }
    hipLaunchKernelGGL(k_narrow_pack, dim3(blocks), dim3(256), 0, st, pb);
}

void narrow_forward(const lsr_deform_net* net, const void* workspace, int32_t P, const float* means3D,
                    const float* time, const float* const (&in)[5], float* const (&out)[5], hipStream_t st) {
    NarrowArgs a = nargs(net, workspace, P);
    a.means3D = means3D;
    a.time = time;
    for (int hd = 0; hd < NHEADS; ++hd) {
        a.in[hd] = in[hd];
        a.out[hd] = out[hd];
    }
    hipLaunchKernelGGL(k_narrow_fwd, dim3((P + NB - 1) / NB), dim3(256), 0, st, a);
}

int64_t narrow_backward_scratch_bytes(const lsr_deform_net* net, int64_t P) {
    return (int64_t)nscratch(net, (size_t)(P > 0 ? P : 1)).total;
}

hipError_t narrow_backward(const lsr_deform_net* net, const void* workspace, int32_t P, const float* means3D,
                           const float* rotations, const float* time, const float* const (&up)[5], float* d_means3D,
                           float* d_rotations, const lsr_deform_grads* grads, void* scratch, hipStream_t st) {
    const NLayout L = nlayout(net);
    const NScratch S = nscratch(net, (size_t)P);
    char* sc = reinterpret_cast<char*>(scratch);
    auto fp = [&](size_t off) { return reinterpret_cast<float*>(sc + off); };
    NarrowArgs a = nargs(net, workspace, P);
    a.means3D = means3D;
    a.time = time;
    a.in[2] = rotations;
    for (int hd = 0; hd < NHEADS; ++hd) a.up[hd] = up[hd];
    a.d_means3D = d_means3D;
    a.d_rotations = d_rotations;
    a.sX = fp(S.X);
    for (int k = 0; k < a.nlayers; ++k) {
        a.sA[k] = fp(S.A[k]);
        a.sdH[k] = fp(S.dH[k]);
    }
    for (int hd = 0; hd < NHEADS; ++hd) {
        if (!head_on(net, hd)) continue;
        a.sR[hd] = fp(S.R[hd]);
        a.sdZ[hd] = fp(S.dZ[hd]);
    }
    a.sG_rot = fp(S.Grot);
    a.dplanes = fp(S.dplanes);
    a.daabb_part = grads->aabb ? fp(S.daabb) : nullptr;
    const hipError_t e = hipMemsetAsync(sc + S.daabb, 0, S.total - S.daabb, st);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_narrow_bwd, dim3((P + NB - 1) / NB), dim3(256), 0, st, a);

    // weight gradients: A^T B products of the saved rows, split-K over row blocks (deform_wgrad.hip's k_atb)
    AtbArgs g{};
    g.P = P;
    const int64_t per = ((int64_t)P + 1023) / 1024;
    g.rows_per_block = (int)std::max<int64_t>(64, (per + 63) / 64 * 64);
    int nj = 0;
    const int F = NC * net->n_scales;
    for (int k = 0; k < a.nlayers; ++k)
        g.job[nj++] = AtbJob{a.sdH[k], k == 0 ? a.sX : a.sA[k - 1], grads->w_feat[k],
                             (k == 0 && F < NW) ? nullptr : grads->b_feat[k], NW, k == 0 ? F : NW};
    if (F < NW)   // one scale: see k_narrow_colsum
        hipLaunchKernelGGL(k_narrow_colsum, dim3((P + NCOLSUM_ROWS - 1) / NCOLSUM_ROWS), dim3(256), 0, st, a.sdH[0], P,
                           grads->b_feat[0]);
    for (int hd = 0; hd < NHEADS; ++hd) {
        if (!head_on(net, hd)) continue;
        const float* G = (hd == 2 && net->apply_rotation) ? a.sG_rot : up[hd];
        g.job[nj++] = AtbJob{a.sdZ[hd], a.sA[a.nlayers - 1], grads->w1[hd], grads->b1[hd], NW, NW};
        g.job[nj++] = AtbJob{G, a.sR[hd], grads->w2[hd], grads->b2[hd], kHeadOut[hd], NW};
    }
    static_assert(DEF_MAX_LAYERS + 2 * NHEADS <= LSR_ATB_MAX_JOBS, "one launch holds every job");
    launch_atb(g, nj, st);

    UnpackBatch u{};   // one copy of the gradient planes, no time rows
    u.src = a.dplanes;
    u.replicas = 1;
    u.daabb_part = a.daabb_part;
    u.daabb = grads->aabb;
    unpack_planes(net, L.planes, NC, grads, u);
    launch_unpack_planes(u, NC, st);
    return hipSuccess;
}

}  // namespace lsr
