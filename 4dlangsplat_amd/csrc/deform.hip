// deform.hip -- the 4D deformation field: HexPlane sampling + MLP heads, fused, one block per 64
// Gaussians (include/lsr_deform.h; reference scene/hexplane.py, scene/deformation.py).
//
// Stage 1 (features): 4 threads per Gaussian, each owning 4 of the 16 channels of every plane.
//   Planes are packed channel-last ([H][W][16], lsr_deform_prepare), so a bilinear tap is one
//   float4 per thread; the 6 planes of a scale multiply, the S scales concatenate (16 S features).
// Stage 2 (MLP): Y = X W^T on v_mfma_f32_32x32x16_bf16 with fp32 accuracy from a bf16 hi/lo split
//   of both operands (hi*hi + hi*lo + lo*hi).  A comes from the block's activation rows in LDS,
//   B straight from the packed bf16 weights ([N][K] rows = the torch layout), which stay
//   L2-resident.  feature_out is a chain of max(defor_depth, 1) layers (ReLU between, and before
//   every head: the heads' first module is a ReLU); bias, ReLU and the residual adds of the heads
//   are fused into the epilogues.  The rotation head's quaternion product (apply_rotation) and the
//   discrete language combination (coff head) are per-Gaussian epilogues through LDS.
// This unit: the forward and phase A of the backward.  On the same MFMA helpers (deform_mfma.h):
// lang_deform and the status centres (deform_lang.hip), the weight gradients (deform_wgrad.hip), the
// parameter pack and the gradient planes' unpack (deform_pack.hip).
#include "lsr_common.h"
#include "deform_internal.h"
#include "deform_mfma.h"
#include "deform_field.h"

namespace lsr {

// Diagnostic build (-DLSR_DEFORM_DIAG): the plane scatter checks every staged tap offset and value
// and counts the bad ones (lsr_debug_deform_diag) instead of adding them.
// Diagnostic build only (-DLSR_DEFORM_STAMPS): wave 0 of every phase-A block sums per-segment
// s_memtime cycles into g_deform_stamps (lsr_debug_deform_stamps; tools/deform_stamps.py).  Shares, not
// times: the stamps cost cycles and constrain the schedule.
#ifdef LSR_DEFORM_STAMPS
__device__ unsigned long long g_deform_stamps[16];
#define DSTAMP(seg)                                                                              \
    do {                                                                                         \
        __builtin_amdgcn_sched_barrier(0);                                                       \
        unsigned long long t_;                                                                   \
        asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t_)::"memory");             \
        __builtin_amdgcn_sched_barrier(0);                                                       \
        if ((seg) >= 0) ds_sum[(seg)] += t_ - ds_prev;                                           \
        ds_prev = t_;                                                                            \
    } while (0)
#else
#define DSTAMP(seg) do {} while (0)
#endif
#ifdef LSR_DEFORM_DIAG
__device__ unsigned long long g_deform_diag[8];
#endif

// head output widths {3, 3, 4, 1, 48} (pos, scales, rotations, opacity, SH), as arithmetic: no
// constant-memory load (a PC-relative s_getpc_b64 sequence) on the heads' paths
__device__ __forceinline__ int head_out(const DeformArgs& a, int hd) {
    return hd < 2 ? 3 : hd == 2 ? 4 : hd == 3 ? 1 : hd == 4 ? 48 : a.centers;
}

// Diagnostic builds (tools/deform_slp_bisect.sh): parts of the HexPlane sampling product's arithmetic
// as scalar VALU instructions the SLP vectorizer cannot pair (same IEEE operations, same bits), so a
// build with SLP on differs from the shipped one only there.  LSR_FEAT_SCALAR: all of it;
// LSR_FEAT_SCALAR_W: the bilinear weights; _SUM: the weighted tap sums; _PROD: the six-plane product.
#if defined(LSR_FEAT_SCALAR)
#define LSR_FEAT_SCALAR_W
#define LSR_FEAT_SCALAR_SUM
#define LSR_FEAT_SCALAR_PROD
#endif
#if defined(LSR_FEAT_SCALAR_W) || defined(LSR_FEAT_SCALAR_SUM) || defined(LSR_FEAT_SCALAR_PROD)
__device__ __forceinline__ float smul(float x, float y) { float r; asm volatile("v_mul_f32 %0, %1, %2" : "=v"(r) : "v"(x), "v"(y)); return r; }
__device__ __forceinline__ float sadd(float x, float y) { float r; asm volatile("v_add_f32 %0, %1, %2" : "=v"(r) : "v"(x), "v"(y)); return r; }
#endif
#ifdef LSR_FEAT_SCALAR_W
#define FW_MUL(x, y) smul((x), (y))
#define FW_SUB1(x) sadd(1.0f, -(x))
#else
#define FW_MUL(x, y) ((x) * (y))
#define FW_SUB1(x) (1.0f - (x))
#endif
#ifdef LSR_FEAT_SCALAR_SUM
#define FS_MUL(x, y) smul((x), (y))
#define FS_ADD(x, y) sadd((x), (y))
#else
#define FS_MUL(x, y) ((x) * (y))
#define FS_ADD(x, y) ((x) + (y))
#endif
#ifdef LSR_FEAT_SCALAR_PROD
#define FP_MUL(x, y) smul((x), (y))
#else
#define FP_MUL(x, y) ((x) * (y))
#endif
__device__ __forceinline__ float4 sample4(const DeformArgs& a, int pi, const Tap& t, int q) {
    const int W = a.pw[pi];
    const float4* pl = reinterpret_cast<const float4*>(a.planes + a.poff[pi]) + q;
    const float4 v00 = pl[(t.y0 * W + t.x0) * 4], v01 = pl[(t.y0 * W + t.x1) * 4];
    const float4 v10 = pl[(t.y1 * W + t.x0) * 4], v11 = pl[(t.y1 * W + t.x1) * 4];
    const float ufx = FW_SUB1(t.fx), ufy = FW_SUB1(t.fy);
#ifdef LSR_FEAT_BCAST_ASM
    // Diagnostic build: the four weights as the broadcast packed products the SLP build forms
    // (v_pk_mul_f32 op_sel:[0,1] op_sel_hi:[0,1]: both halves = A.lo * B.hi), but never in place
    // (early-clobber destinations), everything else left to the vectorizer
    typedef float f2v __attribute__((ext_vector_type(2)));
    const f2v U = {ufx, ufy}, F = {t.fx, t.fy};
    f2v P00, P01, P10, P11;
#if defined(LSR_FEAT_BCAST_NOP_BEFORE)   // A/B: wait states between the operands' producers and the broadcast
#define BC_PRE "s_nop 4\n\t"
#define BC_POST ""
#elif defined(LSR_FEAT_BCAST_NOP_AFTER)  // A/B: wait states between the broadcast and its consumers
#define BC_PRE ""
#define BC_POST "\n\ts_nop 4"
#else
#define BC_PRE ""
#define BC_POST ""
#endif
    asm volatile(BC_PRE "v_pk_mul_f32 %0, %1, %1 op_sel:[0,1] op_sel_hi:[0,1]" BC_POST : "=&v"(P00) : "v"(U));
    asm volatile(BC_PRE "v_pk_mul_f32 %0, %1, %2 op_sel:[0,1] op_sel_hi:[0,1]" BC_POST : "=&v"(P01) : "v"(F), "v"(U));
    asm volatile(BC_PRE "v_pk_mul_f32 %0, %1, %2 op_sel:[0,1] op_sel_hi:[0,1]" BC_POST : "=&v"(P10) : "v"(U), "v"(F));
    asm volatile(BC_PRE "v_pk_mul_f32 %0, %1, %1 op_sel:[0,1] op_sel_hi:[0,1]" BC_POST : "=&v"(P11) : "v"(F));
    const float w00 = P00.x, w01 = P01.x, w10 = P10.x, w11 = P11.x;
#else
    const float w00 = FW_MUL(ufx, ufy), w01 = FW_MUL(t.fx, ufy), w10 = FW_MUL(ufx, t.fy), w11 = FW_MUL(t.fx, t.fy);
#endif
    auto c = [&](float a0, float a1, float a2, float a3) {   // left to right, as the reference's sum
        return FS_ADD(FS_ADD(FS_ADD(FS_MUL(a0, w00), FS_MUL(a1, w01)), FS_MUL(a2, w10)), FS_MUL(a3, w11));
    };
    return make_float4(c(v00.x, v01.x, v10.x, v11.x), c(v00.y, v01.y, v10.y, v11.y), c(v00.z, v01.z, v10.z, v11.z),
                       c(v00.w, v01.w, v10.w, v11.w));
}

// Stage 1 of both passes: the block's features into LDS rows (bf16 hi/lo, pitch XP), optionally
// saved as fp32 [P, 16 S]
template <int S>
__device__ __forceinline__ void features_to_lds(const DeformArgs& a, int g0, __bf16* xh, __bf16* xl, int xp, float* save) {
    const int tid = threadIdx.x, gl = tid >> 2, q = tid & 3;
    const int g = min(g0 + gl, a.P - 1);
    float crd[4];
    coords(a, g, crd);
#pragma unroll
    for (int s = 0; s < S; ++s) {
        float4 prod = make_float4(1.0f, 1.0f, 1.0f, 1.0f);
#pragma unroll
        for (int ci = 0; ci < 6; ++ci) {
            const int pi = 6 * s + ci;
            const float4 v = sample4(a, pi, tap_of(a, pi, ci, crd), q);
            prod.x = FP_MUL(prod.x, v.x); prod.y = FP_MUL(prod.y, v.y); prod.z = FP_MUL(prod.z, v.z);
            prod.w = FP_MUL(prod.w, v.w);
#ifdef LSR_DEFORM_FEAT_WAIT
            asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
#endif
        }
        const float f[4] = {prod.x, prod.y, prod.z, prod.w};
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            __bf16 hi, lo;
            dsplit(f[i], hi, lo);
            xh[gl * xp + 16 * s + 4 * q + i] = hi;
            xl[gl * xp + 16 * s + 4 * q + i] = lo;
        }
        if (save && g0 + gl < a.P)
            *reinterpret_cast<float4*>(save + (size_t)(g0 + gl) * (16 * S) + 16 * s + 4 * q) = prod;
    }
}


// Discrete language combination of one Gaussian (deformation.py:156-163): centres e_c = lang rows
// [c][lang_dim] each normalised (no epsilon), m = sum_c coff_c e_c / |e_c|, out = m / (|m| + 1e-9)
__device__ __forceinline__ void discrete_combine(const DeformArgs& a, int g, const float* coff, float* out) {
    const int C = a.lang_dim, K = a.centers;
    const float* e = a.lang + (size_t)g * a.lang_in;
    float m[32];
#pragma unroll
    for (int j = 0; j < 32; ++j) m[j] = 0.0f;
    for (int c = 0; c < K; ++c) {
        float n2 = 0.0f;
        for (int j = 0; j < C; ++j) n2 += e[c * C + j] * e[c * C + j];
        const float w = coff[c] / sqrtf(n2);
#pragma unroll
        for (int j = 0; j < 32; ++j)
            if (j < C) m[j] += w * e[c * C + j];
    }
    float n2 = 0.0f;
#pragma unroll
    for (int j = 0; j < 32; ++j) n2 += m[j] * m[j];
    const float inv = 1.0f / (sqrtf(n2) + 1e-9f);
#pragma unroll
    for (int j = 0; j < 32; ++j)
        if (j < C) out[(size_t)g * C + j] = m[j] * inv;
}


// Gradient of the discrete combination (deformation.py:156-163), Gaussian g, coff = the head's
// output: dm from out = m / (|m| + eps); dcoff_c = u_c . dm (+ the upstream of coff itself);
// du_c = coff_c dm; de_c = (du_c - u_c (u_c . du_c)) / |e_c|.  m_j and dm_j are recomputed per
// pass (<= 8 terms) instead of held in registers.  Writes d_lang and sG_coff.
__device__ __forceinline__ void discrete_grad(const DeformBwdArgs& b, int g, const float* coff) {
    const DeformArgs& a = b.f;
    const int C = a.lang_dim, K = a.centers;
    const float* e = a.lang + (size_t)g * a.lang_in;
    const float* up = b.up_lang ? b.up_lang + (size_t)g * C : nullptr;
    float w[8], en[8];
    for (int c = 0; c < K; ++c) {
        float n2 = 0.0f;
        for (int j = 0; j < C; ++j) n2 += e[c * C + j] * e[c * C + j];
        en[c] = sqrtf(n2);
        w[c] = coff[c] / en[c];
    }
    auto m_at = [&](int j) {
        float m = 0.0f;
        for (int c = 0; c < K; ++c) m += w[c] * e[c * C + j];
        return m;
    };
    float n2 = 0.0f, md = 0.0f;
    for (int j = 0; j < C; ++j) {
        const float m = m_at(j);
        n2 += m * m;
        md += m * (up ? up[j] : 0.0f);
    }
    const float n = sqrtf(n2), ne = n + 1e-9f, f = md / (n * ne * ne);
    auto dm_at = [&](int j) { return (up ? up[j] : 0.0f) / ne - m_at(j) * f; };
    for (int c = 0; c < K; ++c) {
        float ud = 0.0f;
        for (int j = 0; j < C; ++j) ud += e[c * C + j] / en[c] * dm_at(j);
        b.sG_coff[(size_t)g * K + c] = ud + (b.up_coff ? b.up_coff[(size_t)g * K + c] : 0.0f);
        const float cc = coff[c];   // du_c . u_c = cc (dm . u_c) = cc ud
        for (int j = 0; j < C; ++j)
            b.d_lang[(size_t)g * a.lang_in + c * C + j] = (cc * dm_at(j) - e[c * C + j] / en[c] * (cc * ud)) / en[c];
    }
}

// GRAD = false: the forward.  GRAD = true (backward, apply_rotation / discrete only): the same
// recompute, but only the heads whose output feeds a nonlinear epilogue run, and that epilogue is
// the gradient (quat_grad, discrete_grad) the backward kernel then reads as the head's upstream.
template <int S, bool GRAD>
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2, 2))) k_deform_fwd(const DeformBwdArgs b) {
    const DeformArgs& a = b.f;
    constexpr int F = 16 * S, XP = F + 8;
    static_assert(XP <= DAP, "feature rows live in the second hidden buffer");
    __shared__ __attribute__((aligned(16))) __bf16 s_hh[2][DN * DAP];   // hidden rows, ping-pong
    __shared__ __attribute__((aligned(16))) __bf16 s_hl[2][DN * DAP];
    __shared__ float s_q[DN][9];                                         // per-Gaussian head outputs
    LDS_POISON(s_hh); LDS_POISON(s_hl); LDS_POISON(s_q); LDS_POISON_DONE();
    // the features are read by the first layer only, which writes buffer 0: they use buffer 1 (72 KB
    // of LDS in all: two blocks per CU)
    __bf16* const s_xh = s_hh[1];
    __bf16* const s_xl = s_hl[1];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int g0 = blockIdx.x * DN;

    features_to_lds<S>(a, g0, s_xh, s_xl, XP, nullptr);
    __syncthreads();

    // ---- feature_out chain: hidden = relu(... relu(feat W_0^T + b_0) ... W_k^T + b_k) ------------
    int cur = 0;
    {
        df32x16 acc[2] = {df32x16{}, df32x16{}};
        mlp_ntile<F>(acc, s_xh, s_xl, XP, wave, a.wf_h[0], a.wf_l[0]);
        store_hidden(acc, wave, a.b_feat[0], s_hh[0], s_hl[0]);
    }
    __syncthreads();
    for (int k = 1; k < a.nlayers; ++k) {
        df32x16 acc[2] = {df32x16{}, df32x16{}};
        mlp_ntile<DWID>(acc, s_hh[cur], s_hl[cur], DAP, wave, a.wf_h[k], a.wf_l[k]);
        store_hidden(acc, wave, a.b_feat[k], s_hh[cur ^ 1], s_hl[cur ^ 1]);
        __syncthreads();
        cur ^= 1;
    }
    const __bf16 *ah = s_hh[cur], *al = s_hl[cur];
    __bf16 *bh = s_hh[cur ^ 1], *bl = s_hl[cur ^ 1];

    // ---- heads: out = in + (relu(hidden W1^T + b1) W2^T + b2) ---------------------------------------
    for (int hd = 0; hd < DEF_HEADS; ++hd) {
        if (!((a.heads >> hd) & 1u)) continue;                       // block-uniform
        const int nout = head_out(a, hd);
        const bool quat = hd == 2 && a.apply_rotation, coff = hd == 5;
        const bool resid_add = !quat && !coff;
        if (GRAD && resid_add) continue;
        if (nout <= 16) {                                            // block-uniform
            // a head of at most 16 outputs (pos, scales, rotations, opacity, coff): its output layer as
            // 16 x 16 x 32 MFMAs, one 16-row tile per wave (the 32-column tile of one wave computed
            // 28-31 zero columns while the other three waved at the barrier)
            const int c16 = lane & 15, g4 = lane >> 4;
            float res16[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int g = g0 + 16 * wave + 4 * g4 + i;
                res16[i] = (resid_add && c16 < nout && g < a.P) ? __builtin_nontemporal_load(a.in[hd] + (size_t)g * nout + c16)
                                                               : 0.0f;
            }
            {
                df32x16 acc[2] = {df32x16{}, df32x16{}};
                mlp_ntile<DWID>(acc, ah, al, DAP, wave, a.w1_h[hd], a.w1_l[hd]);
                store_hidden(acc, wave, a.b1[hd], bh, bl);
            }
            __syncthreads();
            df32x4 o = df32x4{0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
            for (int ks = 0; ks < DWID / 32; ++ks) {
                const int k0 = 32 * ks + 8 * g4;
                const dbf16x8 xh = *reinterpret_cast<const dbf16x8*>(bh + (16 * wave + c16) * DAP + k0);
                const dbf16x8 xl = *reinterpret_cast<const dbf16x8*>(bl + (16 * wave + c16) * DAP + k0);
                const dbf16x8 wh = *reinterpret_cast<const dbf16x8*>(a.w2_h[hd] + (size_t)c16 * DWID + k0);
                const dbf16x8 wl = *reinterpret_cast<const dbf16x8*>(a.w2_l[hd] + (size_t)c16 * DWID + k0);
                o = DMFMA16(xh, wh, o);
                o = DMFMA16(xh, wl, o);
                o = DMFMA16(xl, wh, o);
            }
            if (c16 < nout) {
                const float b2 = a.b2[hd][c16];
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const int r = 16 * wave + 4 * g4 + i, g = g0 + r;
                    const float v = o[i] + b2;
                    if (resid_add) {
                        if (g < a.P) __builtin_nontemporal_store(res16[i] + v, a.out[hd] + (size_t)g * nout + c16);
                    } else {
                        s_q[r][c16] = v;
                        if (!GRAD && coff && a.out_coff && g < a.P) a.out_coff[(size_t)g * nout + c16] = v;
                    }
                }
            }
            __syncthreads();   // the hidden rows read (and s_q complete) before they are reused
            if (!resid_add && wave == 0) {                           // one Gaussian per lane
                const int g = g0 + lane;
                if (GRAD && g < a.P) {
                    if (quat) quat_grad(b, a.in[2], g, s_q[lane]);
                    else discrete_grad(b, g, s_q[lane]);
                } else if (g < a.P) {
                    if (quat) {   // rotations = normalize(rotations (x) d_rot)  (deformation.py:135-136)
                        const float4 q1 = reinterpret_cast<const float4*>(a.in[2])[g];
                        const float4 p = quat_mul(q1, make_float4(s_q[lane][0], s_q[lane][1], s_q[lane][2], s_q[lane][3]));
                        const float inv = 1.0f / sqrtf(p.x * p.x + p.y * p.y + p.z * p.z + p.w * p.w);
                        reinterpret_cast<float4*>(a.out[2])[g] = make_float4(p.x * inv, p.y * inv, p.z * inv, p.w * inv);
                    } else {
                        discrete_combine(a, g, s_q[lane], a.out_lang);
                    }
                }
            }
            if (!resid_add) __syncthreads();   // s_q read before the next head's outputs
            continue;
        }
        const bool owner = wave < (nout + 31) / 32;     // 1 N tile, or 2 for the 48 SH coefficients
        const int col = 32 * wave + (lane & 31), h = lane >> 5;
        // the residual inputs of this wave's outputs, loaded now so the head's first layer hides
        // their latency (streamed once: non-temporal, the weights and planes keep the L2)
        float resid[2][16];
#pragma unroll
        for (int mt = 0; mt < 2; ++mt)
#pragma unroll
            for (int q = 0; q < 16; ++q) {
                const int g = g0 + row_of(mt, q, h);
                resid[mt][q] = (resid_add && owner && col < nout && g < a.P)
                                   ? __builtin_nontemporal_load(a.in[hd] + (size_t)g * nout + col) : 0.0f;
            }
        {
            df32x16 acc[2] = {df32x16{}, df32x16{}};
            mlp_ntile<DWID>(acc, ah, al, DAP, wave, a.w1_h[hd], a.w1_l[hd]);
            store_hidden(acc, wave, a.b1[hd], bh, bl);
        }
        __syncthreads();
        if (owner) {
            df32x16 acc[2] = {df32x16{}, df32x16{}};
            mlp_ntile<DWID>(acc, bh, bl, DAP, wave, a.w2_h[hd], a.w2_l[hd]);
            if (col < nout) {
                const float b = a.b2[hd][col];
#pragma unroll
                for (int mt = 0; mt < 2; ++mt)
#pragma unroll
                    for (int q = 0; q < 16; ++q) {
                        const int r = row_of(mt, q, h), g = g0 + r;
                        const float v = acc[mt][q] + b;
                        if (resid_add) {
                            if (g < a.P) __builtin_nontemporal_store(resid[mt][q] + v, a.out[hd] + (size_t)g * nout + col);
                        } else {
                            s_q[r][col] = v;
                            if (!GRAD && coff && a.out_coff && g < a.P) a.out_coff[(size_t)g * nout + col] = v;
                        }
                    }
            }
            if (!resid_add) {                                        // wave 0: one Gaussian per lane
                wave_lds_sync();
                const int g = g0 + lane;
                if (GRAD && g < a.P) {
                    if (quat) quat_grad(b, a.in[2], g, s_q[lane]);
                    else discrete_grad(b, g, s_q[lane]);
                } else if (g < a.P) {
                    if (quat) {   // rotations = normalize(rotations (x) d_rot)  (deformation.py:135-136)
                        const float4 q1 = reinterpret_cast<const float4*>(a.in[2])[g];
                        const float4 p = quat_mul(q1, make_float4(s_q[lane][0], s_q[lane][1], s_q[lane][2], s_q[lane][3]));
                        const float inv = 1.0f / sqrtf(p.x * p.x + p.y * p.y + p.z * p.z + p.w * p.w);
                        reinterpret_cast<float4*>(a.out[2])[g] = make_float4(p.x * inv, p.y * inv, p.z * inv, p.w * inv);
                    } else {
                        discrete_combine(a, g, s_q[lane], a.out_lang);
                    }
                }
            }
        }
        __syncthreads();
    }
}

template <int S, bool GRAD>
static void go_fwd(const DeformBwdArgs& b, hipStream_t st) {
    hipLaunchKernelGGL((k_deform_fwd<S, GRAD>), dim3((b.f.P + DN - 1) / DN), dim3(256), 0, st, b);
}
template <bool GRAD>
static void go_fwd_s(const DeformBwdArgs& b, hipStream_t st) {
    switch (b.f.n_scales) {
        case 1: go_fwd<1, GRAD>(b, st); break;
        case 2: go_fwd<2, GRAD>(b, st); break;
        case 3: go_fwd<3, GRAD>(b, st); break;
        default: go_fwd<4, GRAD>(b, st); break;
    }
}
void launch_deform_fwd(const DeformArgs& a, hipStream_t st) {
    if (a.P <= 0) return;
    DeformBwdArgs b{};
    b.f = a;
    go_fwd_s<false>(b, st);
}

// ==== backward ====================================================================================
// Phase A, one block per 64 Gaussians (the forward's tiling): recompute the features X and the
// chain A_k = relu(H_k) (saved); per head, Z1 = A W1^T + b1, the gradient G of the head's output
// (the upstream gradient, or for the quaternion product / the discrete combination their
// per-Gaussian backward from the recomputed output), dZ1 = (G W2) * [Z1 > 0], and dA += dZ1 W1
// (the heads' Z1 / dZ1 are not saved: k_head_wgrad2 / k_head_wgrad3 recompute them for the weight
// gradients), all on the bf16 hi/lo MFMA of the forward with transposed weight packs; then back
// through the chain, dH_k = dA_k * [H_k > 0] (saved), dA_{k-1} = dH_k W_k, and dX = dH_0 W_0; and per Gaussian the HexPlane backward: each plane's sample gets dX times the
// product of the other five planes of its scale, scattered to the 4 bilinear taps (float atomics
// into a channel-last gradient copy: the 16 channels of a tap are one 64-byte segment), and the
// coordinate gradient (zero where border padding clips) goes to d_means3D.

// DEEP: a feature_out chain of more than one layer (defor_depth >= 2; runtime length).  The
// one-layer chain of every reference config gets its own instantiation: the runtime-length loops
// cost registers (spills) even when they run once.
template <int S, bool DEEP>
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(DEEP ? 1 : 2, 2))) k_deform_bwd_a(DeformBwdArgs b) {
    constexpr int F = 16 * S, XP = F + 8;
    static_assert(XP <= DAP, "feature rows live in the second hidden buffer");
    __shared__ __attribute__((aligned(16))) __bf16 s_hh[2][DN * DAP];
    __shared__ __attribute__((aligned(16))) __bf16 s_hl[2][DN * DAP];
    __bf16* const s_xh = s_hh[1];   // read by the first layer only, which writes buffer 0
    __bf16* const s_xl = s_hl[1];
    __shared__ __attribute__((aligned(16))) float4 s_g4[DN];   // small-output heads: fp32 G rows
    __shared__ uint32_t s_apos[DEEP ? 1 : 256];   // one layer: each thread's A_0 > 0 bits
    // Everything else lives in a hidden buffer while that buffer is dead (68 KB in all: two blocks
    // per CU): a head's G rows in the buffer its dZ1 rows take next (a barrier between the two), dX in
    // the chain's dead buffer, the plane-scatter staging in its lo half; every hand-over is a
    // __syncthreads, and the LDS-poison build checks that nothing reads a word its block never wrote.
    static_assert(DN * (F + 1) * 4 <= DN * DAP * 2, "dX rows fit one hidden buffer");
    static_assert((4 * 16 * 17 + 2 * 4 * 16 * 4) * 4 <= DN * DAP * 2, "scatter staging fits one hidden buffer");
    LDS_POISON(s_hh); LDS_POISON(s_hl); LDS_POISON(s_g4); LDS_POISON_DONE();
    const DeformArgs& a = b.f;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int g0 = blockIdx.x * DN;
    const int col = 32 * wave + (lane & 31), hh = lane >> 5;
    const int L = DEEP ? a.nlayers : 1;
#ifdef LSR_DEFORM_STAMPS
    unsigned long long ds_sum[13] = {}, ds_prev = 0;
#endif
    DSTAMP(-1);

    // ---- features (as the forward), saved as fp32 for the first layer's weight gradient ---------
    features_to_lds<S>(a, g0, s_xh, s_xl, XP, b.sX);
    __syncthreads();
    DSTAMP(0);

    // ---- chain forward, A_k = relu(H_k) saved ------------------------------------------------------
    int cur = 0;
    uint32_t apos = 0;   // one layer (!DEEP): bit 16 mt + q = A_0 > 0, the chain backward's ReLU mask,
                         // parked in LDS across the heads (a live register there spilled 38)
    for (int k = 0; k < L; ++k) {
        df32x16 acc[2] = {df32x16{}, df32x16{}};
        if (k == 0) mlp_ntile<F>(acc, s_xh, s_xl, XP, wave, a.wf_h[0], a.wf_l[0]);
        else mlp_ntile<DWID>(acc, s_hh[cur], s_hl[cur], DAP, wave, a.wf_h[k], a.wf_l[k]);
        const int dst = k == 0 ? 0 : cur ^ 1;
        store_hidden(acc, wave, a.b_feat[k], s_hh[dst], s_hl[dst]);
        const float bias = a.b_feat[k][col];
#pragma unroll
        for (int mt = 0; mt < 2; ++mt)
#pragma unroll
            for (int q = 0; q < 16; ++q) {
                const int g = g0 + row_of(mt, q, hh);
                const float av = fmaxf(acc[mt][q] + bias, 0.0f);
                if (g < a.P) b.sA[k][(size_t)g * DWID + col] = av;
                if (!DEEP) apos |= av > 0.0f ? 1u << (16 * mt + q) : 0u;
            }
        if (!DEEP) s_apos[tid] = apos;
        __syncthreads();
        cur = dst;
    }
    const __bf16 *ah = s_hh[cur], *al = s_hl[cur];
    __bf16 *bh = s_hh[cur ^ 1], *bl = s_hl[cur ^ 1];

    DSTAMP(1);
    df32x16 dA[2] = {df32x16{}, df32x16{}};
    for (int hd = 0; hd < DEF_HEADS; ++hd) {
        if (!((a.heads >> hd) & 1u)) continue;                       // block-uniform
        const int nout = head_out(a, hd);
        const bool quat = hd == 2 && a.apply_rotation, coff = hd == 5;
        const float* G = coff ? b.sG_coff : quat ? b.sG_rot : b.up[hd];   // saved by the GRAD pass
        // a large head's gradient rows (K padded to 64, 16 per thread) loaded before its Z1 product,
        // which hides their latency (issued after Z1, the conversion below waited for them: 12 % of
        // phase A in the stamp build)
        constexpr int NJ = DN * 64 / 256;
        float gv[NJ];
        if (nout > DEF_SMALL_OUT) {                                  // block-uniform
#pragma unroll
            for (int j = 0; j < NJ; ++j) {
                const int i = tid + 256 * j, r = i >> 6, k = i & 63, g = g0 + r;
                gv[j] = (k < nout && g < a.P) ? G[(size_t)g * nout + k] : 0.0f;
            }
        }
        // Z1 for this wave's 32 columns (its rows finish before the sync below)
        uint32_t zpos = 0;   // bit 16 mt + q: Z1 > 0 (the ReLU mask of dZ1; Z1 itself dies here)
        {
            df32x16 z[2] = {df32x16{}, df32x16{}};
            mlp_ntile<DWID>(z, ah, al, DAP, wave, a.w1_h[hd], a.w1_l[hd]);
            const float bias = a.b1[hd][col];
#pragma unroll
            for (int mt = 0; mt < 2; ++mt)
#pragma unroll
                for (int q = 0; q < 16; ++q) zpos |= z[mt][q] + bias > 0.0f ? 1u << (16 * mt + q) : 0u;
        }
        DSTAMP(2);
        if (nout <= DEF_SMALL_OUT) {                                 // block-uniform
            // dZ1 = (G W2) [Z1 > 0] on the VALU from fp32 G rows (as k_head_wgrad3)
            // (loaded after Z1: issued before it, as the SH head's rows, measured 10.65-10.72 vs
            // 10.47-10.54 ms at 2M, 13 VGPRs spilled)
            if (tid < DN) {
                const int g = g0 + tid;
                float v[DEF_SMALL_OUT] = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
                for (int k = 0; k < DEF_SMALL_OUT; ++k)
                    if (k < nout && g < a.P) v[k] = G[(size_t)g * nout + k];
                s_g4[tid] = make_float4(v[0], v[1], v[2], v[3]);
            }
            float w2c[DEF_SMALL_OUT];
            w2_column(a.w2_h[hd], a.w2_l[hd], col, w2c);
            DSTAMP(8);         // small head: G and W2 column loads issued, G rows stored
            __syncthreads();   // G rows complete
            DSTAMP(9);         // small head: the first barrier
#pragma unroll
            for (int mt = 0; mt < 2; ++mt)
#pragma unroll
                for (int q = 0; q < 16; ++q) {
                    const int r = row_of(mt, q, hh);
                    const float4 gv = s_g4[r];
                    float dv = gv.x * w2c[0];
                    dv = __builtin_fmaf(gv.y, w2c[1], dv);
                    dv = __builtin_fmaf(gv.z, w2c[2], dv);
                    dv = __builtin_fmaf(gv.w, w2c[3], dv);
                    const float v = (zpos >> (16 * mt + q)) & 1u ? dv : 0.0f;
                    __bf16 hi, lo;
                    dsplit(v, hi, lo);
                    bh[r * DAP + col] = hi;
                    bl[r * DAP + col] = lo;
                }
            __syncthreads();   // dZ1 rows complete
            DSTAMP(3);
            mlp_ntile<DWID>(dA, bh, bl, DAP, wave, b.w1t_h[hd], b.w1t_l[hd]);
            DSTAMP(4);
            __syncthreads();   // dZ1 rows and the G rows consumed before the next head rewrites them
            DSTAMP(5);
            continue;
        }
        // gradient rows of this head's output, K padded to 64, in the buffer dZ1 takes next: every load
        // of the thread issued before the first conversion (a load-convert-store loop waited one memory
        // latency per row)
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
            const int i = tid + 256 * j, r = i >> 6, k = i & 63;
            __bf16 hi, lo;
            dsplit(gv[j], hi, lo);
            bh[r * DGP + k] = hi;
            bl[r * DGP + k] = lo;
        }
        DSTAMP(10);        // SH head: G rows loaded and stored
        __syncthreads();   // G rows complete
        df32x16 d[2] = {df32x16{}, df32x16{}};
        mlp_ntile<64>(d, bh, bl, DGP, wave, b.w2t_h[hd], b.w2t_l[hd]);
        DSTAMP(11);        // SH head: barrier + G W2 product
        __syncthreads();   // every wave has read the G rows: dZ1 overwrites them
#pragma unroll
        for (int mt = 0; mt < 2; ++mt)
#pragma unroll
            for (int q = 0; q < 16; ++q) {
                const int r = row_of(mt, q, hh);
                const float v = (zpos >> (16 * mt + q)) & 1u ? d[mt][q] : 0.0f;
                __bf16 hi, lo;
                dsplit(v, hi, lo);
                bh[r * DAP + col] = hi;
                bl[r * DAP + col] = lo;
            }
        __syncthreads();   // dZ1 rows complete
        DSTAMP(3);
        mlp_ntile<DWID>(dA, bh, bl, DAP, wave, b.w1t_h[hd], b.w1t_l[hd]);
        DSTAMP(4);
        __syncthreads();   // dZ1 rows consumed before the next head's G rows overwrite them
        DSTAMP(5);
    }

    // ---- back through the chain: dH_k = dA_k * [H_k > 0] (saved), dA_{k-1} = dH_k W_k -------------
    for (int k = L - 1; k >= 0; --k) {
        // dH_k rows into the buffer that does not hold what the MFMA below still reads
        __bf16 *dh_h = s_hh[cur ^ 1], *dh_l = s_hl[cur ^ 1];
#pragma unroll
        for (int mt = 0; mt < 2; ++mt)
#pragma unroll
            for (int q = 0; q < 16; ++q) {
                const int r = row_of(mt, q, hh), g = g0 + r;
                // one layer: the mask parked in s_apos (reloading A_0 put 32 dependent loads of rows
                // this block had just written on the chain's critical path)
                const bool on = DEEP ? (g < a.P && b.sA[k][(size_t)g * DWID + col] > 0.0f)
                                     : (g < a.P && ((s_apos[tid] >> (16 * mt + q)) & 1u));
                const float v = on ? dA[mt][q] : 0.0f;
                __bf16 hi, lo;
                dsplit(v, hi, lo);
                dh_h[r * DAP + col] = hi;
                dh_l[r * DAP + col] = lo;
                if (g < a.P) b.sdH[k][(size_t)g * DWID + col] = v;
            }
        __syncthreads();
        cur ^= 1;
        if (k > 0) {
            df32x16 acc[2] = {df32x16{}, df32x16{}};
            mlp_ntile<DWID>(acc, dh_h, dh_l, DAP, wave, b.wft_h[k], b.wft_l[k]);
            dA[0] = acc[0];
            dA[1] = acc[1];
            __syncthreads();   // the dH rows read before the next iteration overwrites the other buffer
        } else if (wave < (F + 31) / 32) {
            df32x16 acc[2] = {df32x16{}, df32x16{}};
            mlp_ntile<DWID>(acc, dh_h, dh_l, DAP, wave, b.wft_h[0], b.wft_l[0]);
            const int c = 32 * wave + (lane & 31);
            // dX rows [64][F + 1] in the other hidden buffer (its rows died with the heads)
            float* dxw = reinterpret_cast<float*>(s_hh[cur ^ 1]);
            if (c < F) {
#pragma unroll
                for (int mt = 0; mt < 2; ++mt)
#pragma unroll
                    for (int q = 0; q < 16; ++q) dxw[row_of(mt, q, hh) * (F + 1) + c] = acc[mt][q];
            }
        }
    }
    __syncthreads();
    DSTAMP(6);
    const float* s_dx = reinterpret_cast<const float*>(s_hh[cur ^ 1]);   // [64][F + 1]
    // plane-scatter staging in the lo half of that buffer: per wave, dv of 16 Gaussians [16][17],
    // their 4 tap offsets and bilinear weights
    float* const s_sdv = reinterpret_cast<float*>(s_hl[cur ^ 1]);
    int* const s_soff = reinterpret_cast<int*>(s_sdv + 4 * 16 * 17);
    float* const s_sw = reinterpret_cast<float*>(s_soff + 4 * 16 * 4);

    // ---- HexPlane backward: 4 threads per Gaussian, 4 channels each ----------------------------------
    {
        const int gl = tid >> 2, q = tid & 3;
        const bool ok = g0 + gl < a.P;
        const int g = min(g0 + gl, a.P - 1);
        float crd[4];
        coords(a, g, crd);
        float dq[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        // every Gaussian of this wave at the call's first time (a vote, no barrier)
        const bool t_row = b.trow && __all(crd[3] == a.time[0]);
        // a scale's plane gradients dv (24 registers) and its coordinate gradient: each plane's 4 taps
        // loaded once for the sample (sample4's arithmetic) and its x / y derivatives
        auto grad_scale = [&](int s, float4 (&dvo)[6]) __attribute__((always_inline)) {
            float4 v[6], gxv[6], gyv[6];
#pragma unroll
            for (int ci = 0; ci < 6; ++ci) {
                const int pi = 6 * s + ci, W = a.pw[pi];
                const Tap t = tap_of(a, pi, ci, crd);
                const float4* pl = reinterpret_cast<const float4*>(a.planes + a.poff[pi]) + q;
                const float4 t00 = pl[(t.y0 * W + t.x0) * 4], t01 = pl[(t.y0 * W + t.x1) * 4];
                const float4 t10 = pl[(t.y1 * W + t.x0) * 4], t11 = pl[(t.y1 * W + t.x1) * 4];
                const float w00 = (1.0f - t.fx) * (1.0f - t.fy), w01 = t.fx * (1.0f - t.fy), w10 = (1.0f - t.fx) * t.fy,
                            w11 = t.fx * t.fy;
                v[ci] = make_float4(t00.x * w00 + t01.x * w01 + t10.x * w10 + t11.x * w11,
                                    t00.y * w00 + t01.y * w01 + t10.y * w10 + t11.y * w11,
                                    t00.z * w00 + t01.z * w01 + t10.z * w10 + t11.z * w11,
                                    t00.w * w00 + t01.w * w01 + t10.w * w10 + t11.w * w11);
                const float ux = 1.0f - t.fy, uy = 1.0f - t.fx;
                gxv[ci] = make_float4((t01.x - t00.x) * ux + (t11.x - t10.x) * t.fy, (t01.y - t00.y) * ux + (t11.y - t10.y) * t.fy,
                                      (t01.z - t00.z) * ux + (t11.z - t10.z) * t.fy, (t01.w - t00.w) * ux + (t11.w - t10.w) * t.fy);
                gyv[ci] = make_float4((t10.x - t00.x) * uy + (t11.x - t01.x) * t.fx, (t10.y - t00.y) * uy + (t11.y - t01.y) * t.fx,
                                      (t10.z - t00.z) * uy + (t11.z - t01.z) * t.fx, (t10.w - t00.w) * uy + (t11.w - t01.w) * t.fx);
            }
            const float* dxr = s_dx + gl * (F + 1) + 16 * s + 4 * q;
            const float dxv[4] = {dxr[0], dxr[1], dxr[2], dxr[3]};
#pragma unroll
            for (int ci = 0; ci < 6; ++ci) {
                float4 oth = make_float4(1.0f, 1.0f, 1.0f, 1.0f);
#pragma unroll
                for (int cj = 0; cj < 6; ++cj)
                    if (cj != ci) {
                        oth.x *= v[cj].x; oth.y *= v[cj].y; oth.z *= v[cj].z; oth.w *= v[cj].w;
                    }
                const float dv[4] = {dxv[0] * oth.x, dxv[1] * oth.y, dxv[2] * oth.z, dxv[3] * oth.w};
                dvo[ci] = make_float4(dv[0], dv[1], dv[2], dv[3]);
                const int pi = 6 * s + ci;
                const int W = a.pw[pi], H = a.ph[pi];
                const float rx = (crd[kC0(ci)] + 1.0f) * 0.5f * (float)(W - 1);
                const float ry = (crd[kC1(ci)] + 1.0f) * 0.5f * (float)(H - 1);
                const float gx4[4] = {gxv[ci].x, gxv[ci].y, gxv[ci].z, gxv[ci].w};
                const float gy4[4] = {gyv[ci].x, gyv[ci].y, gyv[ci].z, gyv[ci].w};
                float dix = 0.0f, diy = 0.0f;
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    dix += dv[i] * gx4[i];
                    diy += dv[i] * gy4[i];
                }
                if (rx > 0.0f && rx < (float)(W - 1)) dq[kC0(ci)] += dix * 0.5f * (float)(W - 1);
                if (ry > 0.0f && ry < (float)(H - 1)) dq[kC1(ci)] += diy * 0.5f * (float)(H - 1);
            }
        };
        // scatter: stage the wave's 16 Gaussians (16 channels, 4 taps each) in LDS, then one atomic
        // instruction per Gaussian covers its 4 taps x 16 channels = four full 64-byte segments (lane =
        // 16 tap + channel) instead of 16 partial ones; blocks add into one of b.replicas copies of the
        // gradient planes (summed by the unpack), so the few cells every Gaussian of a frame shares (the
        // time planes) are not one hot spot
        auto scatter_scale = [&](int s, const float4 (&dvo)[6]) __attribute__((always_inline)) {
#pragma unroll
            for (int ci = 0; ci < 6; ++ci) {
                const int pi = 6 * s + ci, W = a.pw[pi];
                const Tap t = tap_of(a, pi, ci, crd);
                const float dv[4] = {dvo[ci].x, dvo[ci].y, dvo[ci].z, dvo[ci].w};
                const int wl = gl & 15;
                if ((ci == 2 || ci >= 4) && t_row) {   // wave-uniform
                    // a time plane of a wave at time[0]: its x-row (b.trow), 2 taps x 16 channels per
                    // Gaussian, two Gaussians per atomic instruction (half the time planes' requests)
#pragma unroll
                    for (int i = 0; i < 4; ++i) s_sdv[(wave * 16 + wl) * 17 + 4 * q + i] = ok ? dv[i] : 0.0f;
                    if (q == 0) {
                        s_soff[(wave * 16 + wl) * 4 + 0] = t.x0 * 16;
                        s_soff[(wave * 16 + wl) * 4 + 1] = t.x1 * 16;
                        s_sw[(wave * 16 + wl) * 4 + 0] = 1.0f - t.fx;
                        s_sw[(wave * 16 + wl) * 4 + 1] = t.fx;
                    }
                    wave_lds_sync();
                    float* rp = b.trow + (size_t)(blockIdx.x % b.trow_reps) * b.trow_stride + b.toff[pi];
                    const int tap = (lane >> 4) & 1, ch = lane & 15, half = lane >> 5;
#pragma unroll 4
                    for (int j = 0; j < 8; ++j) {
                        const int e = wave * 16 + 2 * j + half;
                        const float val = s_sdv[e * 17 + ch] * s_sw[e * 4 + tap];
                        if (val != 0.0f) atomicAdd(rp + s_soff[e * 4 + tap] + ch, val);
                    }
                    wave_lds_sync();   // staging read before the next plane rewrites it
                    continue;
                }
                const float w00 = (1.0f - t.fx) * (1.0f - t.fy), w01 = t.fx * (1.0f - t.fy),
                            w10 = (1.0f - t.fx) * t.fy, w11 = t.fx * t.fy;
#pragma unroll
                for (int i = 0; i < 4; ++i) s_sdv[(wave * 16 + wl) * 17 + 4 * q + i] = ok ? dv[i] : 0.0f;
                if (q == 0) {
                    int* so = s_soff + (wave * 16 + wl) * 4;
                    float* sw = s_sw + (wave * 16 + wl) * 4;
                    so[0] = (t.y0 * W + t.x0) * 16; so[1] = (t.y0 * W + t.x1) * 16;
                    so[2] = (t.y1 * W + t.x0) * 16; so[3] = (t.y1 * W + t.x1) * 16;
                    sw[0] = w00; sw[1] = w01; sw[2] = w10; sw[3] = w11;
                }
                wave_lds_sync();
                float* gp = b.dplanes + (size_t)(blockIdx.x % b.replicas) * b.plane_stride + a.poff[pi];
                const int tap = lane >> 4, ch = lane & 15;
#pragma unroll 4
                for (int j = 0; j < 16; ++j) {
                    const float val = s_sdv[(wave * 16 + j) * 17 + ch] * s_sw[(wave * 16 + j) * 4 + tap];
#ifdef LSR_DEFORM_DIAG
                    const int off = s_soff[(wave * 16 + j) * 4 + tap];
                    const int H = a.ph[pi];
                    if (off < 0 || off >= W * H * 16 || !(fabsf(val) < 1e30f)) {
                        atomicAdd(&g_deform_diag[0], 1ull);
                        atomicAdd(&g_deform_diag[1 + tap], 1ull);
                        continue;
                    }
#endif
                    if (val != 0.0f) atomicAdd(gp + s_soff[(wave * 16 + j) * 4 + tap] + ch, val);
                }
                wave_lds_sync();   // staging read before the next plane rewrites it
            }
        };
        // every scale's taps loaded (and its coordinate gradient formed) before the first scatter:
        // vmcnt retires in order and counts the atomics, so tap loads issued behind a scale's
        // atomics waited for them; the scales' dv (24 registers each) stay live in between
        float4 dvo[S][6];
#pragma unroll
        for (int s = 0; s < S; ++s) grad_scale(s, dvo[s]);
        DSTAMP(12);        // taps, dv and the coordinate gradient of every scale
#pragma unroll
        for (int s = 0; s < S; ++s) scatter_scale(s, dvo[s]);
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            dq[c] += __shfl_xor(dq[c], 1);
            dq[c] += __shfl_xor(dq[c], 2);
        }
        if (ok && q == 0) {
            const size_t gg = (size_t)(g0 + gl);
#pragma unroll
            for (int c = 0; c < 3; ++c)
                b.d_means3D[3 * gg + c] = b.up[0][3 * gg + c] + dq[c] * (2.0f / (a.aabb[3 + c] - a.aabb[c]));
        }
        if (b.daabb) {   // block-uniform
            // normalize_aabb's gradient w.r.t. the box (hexplane.py:19-20): with n = (p - a0) s - 1,
            // s = 2 / (a1 - a0): dn/da0 = s (n - 1) / 2, dn/da1 = -s (n + 1) / 2, and dq = dL/dn
            float v[6];
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const float gp = (ok && q == 0) ? dq[c] * (2.0f / (a.aabb[3 + c] - a.aabb[c])) : 0.0f;
                v[c] = 0.5f * gp * (crd[c] - 1.0f);
                v[3 + c] = -0.5f * gp * (crd[c] + 1.0f);
            }
#pragma unroll
            for (int k = 0; k < 6; ++k) {
#pragma unroll
                for (int off = 32; off >= 1; off >>= 1) v[k] += __shfl_xor(v[k], off);
            }
            if ((tid & 63) == 0) {   // one of DEF_AABB_SLOTS partial rows: every wave of a
                                     // launch adding into the same six words serialised on one L2 line
                float* row = b.daabb_part + (blockIdx.x % DEF_AABB_SLOTS) * 16;
#pragma unroll
                for (int k = 0; k < 6; ++k) atomicAdd(row + k, v[k]);
            }
        }
    }
#ifdef LSR_DEFORM_STAMPS
    DSTAMP(7);
    if (tid == 0) {
#pragma unroll
        for (int k = 0; k < 13; ++k) atomicAdd(&g_deform_stamps[k], ds_sum[k]);
        atomicAdd(&g_deform_stamps[13], 1ull);
    }
#endif
}

template <int S>
static void go_bwd(const DeformBwdArgs& b, hipStream_t st) {
    if (b.f.nlayers > 1) hipLaunchKernelGGL((k_deform_bwd_a<S, true>), dim3((b.f.P + DN - 1) / DN), dim3(256), 0, st, b);
    else hipLaunchKernelGGL((k_deform_bwd_a<S, false>), dim3((b.f.P + DN - 1) / DN), dim3(256), 0, st, b);
}
void launch_deform_bwd_a(const DeformBwdArgs& b, hipStream_t st) {
    if (b.f.P <= 0) return;
    if (b.f.apply_rotation || (b.f.heads >> 5) & 1u) go_fwd_s<true>(b, st);   // the nonlinear heads' gradients
    switch (b.f.n_scales) {
        case 1: go_bwd<1>(b, st); break;
        case 2: go_bwd<2>(b, st); break;
        case 3: go_bwd<3>(b, st); break;
        default: go_bwd<4>(b, st); break;
    }
}

}  // namespace lsr

// lang_deform and the status centres have a file of their own and are compiled here: as a unit of
// their own the compiler's code for their three kernels is not the single file's (other registers,
// other address arithmetic)
#include "deform_lang.hip"

#ifdef LSR_DEFORM_STAMPS
extern "C" int lsr_debug_deform_stamps(unsigned long long* out14) {   // 13 segments + blocks; read and reset
    if (hipMemcpyFromSymbol(out14, HIP_SYMBOL(lsr::g_deform_stamps), 14 * sizeof(unsigned long long)) != hipSuccess) return 2;
    unsigned long long z[16] = {};
    return hipMemcpyToSymbol(HIP_SYMBOL(lsr::g_deform_stamps), z, sizeof(z)) == hipSuccess ? 0 : 2;
}
#endif
#ifdef LSR_DEFORM_DIAG
// diagnostic export (not part of include/lsr_deform.h): read and reset the counters
extern "C" int lsr_debug_deform_diag(unsigned long long* out8) {
    if (hipMemcpyFromSymbol(out8, HIP_SYMBOL(lsr::g_deform_diag), 8 * sizeof(unsigned long long)) != hipSuccess) return 2;
    unsigned long long z[8] = {};
    return hipMemcpyToSymbol(HIP_SYMBOL(lsr::g_deform_diag), z, sizeof(z)) == hipSuccess ? 0 : 2;
}
#endif
