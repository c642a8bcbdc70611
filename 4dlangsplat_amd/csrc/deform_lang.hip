// deform_lang.hip -- lang_deform, the deformation field's time-varying language MLP (it reads only
// the language rows and the time: its own kernels, on the MFMA helpers of deform_mfma.h), forward and
// backward, and the status centres sampled from it (k_centers_from_field).  Not a unit of the Makefile:
// deform.hip includes it at its end (the reason is given there).
#include "lsr_common.h"
#include "deform_internal.h"
#include "deform_mfma.h"
#include "centers_kmeans.h"

namespace lsr {

// ==== lang_deform (deformation.py:68, 172-180) ====================================================
// relu([lang, t, sin(2^i t), cos(2^i t)]) -> Linear(kin, 128), ReLU, Linear(128, 128), ReLU,
// Linear(128, lang_dim); lang_out = normalize((lang +) dl).  One block per 64 Gaussians; the input
// rows are K-padded to a multiple of 16 (<= 64).
__device__ __forceinline__ float lang_in_value(const LangDeformArgs& a, int g, int k) {
    const int C = a.lang_dim;
    if (k < C) return a.lang[(size_t)g * C + k];
    const float t = a.time[g];
    if (k == C) return t;
    const int j = k - C - 1;                                          // poc_fre: sin block, cos block
    if (j < a.time_pe) return sinf(t * (float)(1 << j));
    if (j < 2 * a.time_pe) return cosf(t * (float)(1 << (j - a.time_pe)));
    return 0.0f;
}

// forward of the MLP for the block's 64 rows; leaves v = (lang +) dl in s_v[64][33] (and with
// `save`, the saved activations).  kpad = 16-padded input width.
__device__ __forceinline__ void lang_mlp_fwd(const LangDeformArgs& a, int g0, int kpad, __bf16* xh, __bf16* xl,
                                             __bf16 (*hh)[DN * DAP], __bf16 (*hl)[DN * DAP], float (*s_v)[33], bool save) {
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, hh_ = lane >> 5;
    for (int i = tid; i < DN * 64; i += 256) {
        const int r = i >> 6, k = i & 63, g = g0 + r;
        const float v = (g < a.P && k < a.kin) ? fmaxf(lang_in_value(a, g, k), 0.0f) : 0.0f;
        if (k < kpad) {
            __bf16 hi, lo;
            dsplit(v, hi, lo);
            xh[r * DLP + k] = hi;
            xl[r * DLP + k] = lo;
        }
        if (save && g < a.P && k < a.kin) a.sU0[(size_t)g * a.kin + k] = v;
    }
    __syncthreads();
    const int col = 32 * wave + (lane & 31);
    for (int layer = 0; layer < 2; ++layer) {
        df32x16 acc[2] = {df32x16{}, df32x16{}};
        if (layer == 0) mlp_ntile_k(kpad, acc, xh, xl, DLP, wave, a.w_h[0], a.w_l[0]);
        else mlp_ntile<DWID>(acc, hh[0], hl[0], DAP, wave, a.w_h[1], a.w_l[1]);
        store_hidden(acc, wave, a.b[layer], hh[layer], hl[layer]);
        if (save) {
            const float bias = a.b[layer][col];
            float* dst = layer == 0 ? a.sU1 : a.sU2;
#pragma unroll
            for (int mt = 0; mt < 2; ++mt)
#pragma unroll
                for (int q = 0; q < 16; ++q) {
                    const int g = g0 + row_of(mt, q, hh_);
                    if (g < a.P) dst[(size_t)g * DWID + col] = fmaxf(acc[mt][q] + bias, 0.0f);
                }
        }
        __syncthreads();
    }
    if (wave == 0) {
        df32x16 acc[2] = {df32x16{}, df32x16{}};
        mlp_ntile<DWID>(acc, hh[1], hl[1], DAP, 0, a.w_h[2], a.w_l[2]);
        const int c = lane & 31;
        if (c < a.lang_dim) {
            const float bias = a.b[2][c];
#pragma unroll
            for (int mt = 0; mt < 2; ++mt)
#pragma unroll
                for (int q = 0; q < 16; ++q) {
                    const int r = row_of(mt, q, hh_), g = g0 + r;
                    float v = acc[mt][q] + bias;
                    if (a.residual && g < a.P) v += a.lang[(size_t)g * a.lang_dim + c];
                    s_v[r][c] = v;
                }
        }
    }
    __syncthreads();
}

__global__ void __launch_bounds__(256) k_lang_deform_fwd(LangDeformArgs a) {
    __shared__ __attribute__((aligned(16))) __bf16 s_xh[DN * DLP];
    __shared__ __attribute__((aligned(16))) __bf16 s_xl[DN * DLP];
    __shared__ __attribute__((aligned(16))) __bf16 s_hh[2][DN * DAP];
    __shared__ __attribute__((aligned(16))) __bf16 s_hl[2][DN * DAP];
    __shared__ float s_v[DN][33];
    LDS_POISON(s_xh); LDS_POISON(s_xl); LDS_POISON(s_hh); LDS_POISON(s_hl); LDS_POISON(s_v); LDS_POISON_DONE();
    const int g0 = blockIdx.x * DN, tid = threadIdx.x;
    const int kpad = (a.kin + 15) / 16 * 16;
    lang_mlp_fwd(a, g0, kpad, s_xh, s_xl, s_hh, s_hl, s_v, false);
    if (tid < DN && g0 + tid < a.P) {   // out = v / (|v| + 1e-9)
        float n2 = 0.0f;
        for (int c = 0; c < a.lang_dim; ++c) n2 += s_v[tid][c] * s_v[tid][c];
        const float inv = 1.0f / (sqrtf(n2) + 1e-9f);
        for (int c = 0; c < a.lang_dim; ++c) a.out_lang[(size_t)(g0 + tid) * a.lang_dim + c] = s_v[tid][c] * inv;
    }
}

__global__ void __launch_bounds__(256) k_lang_deform_bwd(LangDeformArgs a) {
    __shared__ __attribute__((aligned(16))) __bf16 s_xh[DN * DLP];
    __shared__ __attribute__((aligned(16))) __bf16 s_xl[DN * DLP];
    __shared__ __attribute__((aligned(16))) __bf16 s_hh[2][DN * DAP];
    __shared__ __attribute__((aligned(16))) __bf16 s_hl[2][DN * DAP];
    __shared__ __attribute__((aligned(16))) __bf16 s_gh[DN * DLP];
    __shared__ __attribute__((aligned(16))) __bf16 s_gl[DN * DLP];
    __shared__ float s_v[DN][33];
    LDS_POISON(s_xh); LDS_POISON(s_xl); LDS_POISON(s_hh); LDS_POISON(s_hl); LDS_POISON(s_gh); LDS_POISON(s_gl);
    LDS_POISON(s_v); LDS_POISON_DONE();
    const int g0 = blockIdx.x * DN, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, hh = lane >> 5;
    const int col = 32 * wave + (lane & 31);
    const int C = a.lang_dim, kpad = (a.kin + 15) / 16 * 16;
    lang_mlp_fwd(a, g0, kpad, s_xh, s_xl, s_hh, s_hl, s_v, true);
    // dv = d / (|v| + eps) - v (v . d) / (|v| (|v| + eps)^2), d = the upstream language gradient
    if (tid < DN) {
        const int g = g0 + tid;
        float n2 = 0.0f, vd = 0.0f;
        for (int c = 0; c < C; ++c) {
            const float up = (g < a.P && a.up_lang) ? a.up_lang[(size_t)g * C + c] : 0.0f;
            n2 += s_v[tid][c] * s_v[tid][c];
            vd += s_v[tid][c] * up;
        }
        const float n = sqrtf(n2), ne = n + 1e-9f, f = n > 0.0f ? vd / (n * ne * ne) : 0.0f;
        for (int c = 0; c < 32; ++c) {
            float dv = 0.0f;
            if (c < C && g < a.P) dv = (a.up_lang ? a.up_lang[(size_t)g * C + c] : 0.0f) / ne - s_v[tid][c] * f;
            s_v[tid][c] = dv;
            __bf16 hi, lo;
            dsplit(dv, hi, lo);
            s_gh[tid * DLP + c] = hi;
            s_gl[tid * DLP + c] = lo;
            if (c < C && g < a.P) a.sdv[(size_t)g * C + c] = dv;
        }
    }
    __syncthreads();
    // dZ2 = (dv W3) * [U2 > 0]; dZ1 = (dZ2 W2) * [U1 > 0]   (U_k > 0 <=> Z_k > 0)
    for (int layer = 1; layer >= 0; --layer) {
        df32x16 acc[2] = {df32x16{}, df32x16{}};
        if (layer == 1) mlp_ntile<32>(acc, s_gh, s_gl, DLP, wave, a.wt_h[2], a.wt_l[2]);
        else mlp_ntile<DWID>(acc, s_hh[1], s_hl[1], DAP, wave, a.wt_h[1], a.wt_l[1]);
        const __bf16 *uh = s_hh[layer], *ul = s_hl[layer];
        float dz[2][16];
#pragma unroll
        for (int mt = 0; mt < 2; ++mt)
#pragma unroll
            for (int q = 0; q < 16; ++q) {
                const int r = row_of(mt, q, hh);
                const bool on = (float)uh[r * DAP + col] + (float)ul[r * DAP + col] > 0.0f;
                dz[mt][q] = on ? acc[mt][q] : 0.0f;
            }
        float* save = layer == 1 ? a.sdZ2 : a.sdZ1;
        __syncthreads();   // U rows (and, for layer 0, the dZ2 rows in buffer 1) read
#pragma unroll
        for (int mt = 0; mt < 2; ++mt)
#pragma unroll
            for (int q = 0; q < 16; ++q) {
                const int r = row_of(mt, q, hh), g = g0 + r;
                __bf16 hi, lo;
                dsplit(dz[mt][q], hi, lo);
                s_hh[1][r * DAP + col] = hi;   // dZ rows replace U2 (the next step's A operand)
                s_hl[1][r * DAP + col] = lo;
                if (g < a.P) save[(size_t)g * DWID + col] = dz[mt][q];
            }
        __syncthreads();
    }
    // dU0 = dZ1 W1 (waves owning input columns), d_lang = (dv if residual) + dU0 * [U0 > 0]
    if (wave < (kpad + 31) / 32) {
        df32x16 acc[2] = {df32x16{}, df32x16{}};
        mlp_ntile<DWID>(acc, s_hh[1], s_hl[1], DAP, wave, a.wt_h[0], a.wt_l[0]);
        const int c = 32 * wave + (lane & 31);
        if (c < C) {
#pragma unroll
            for (int mt = 0; mt < 2; ++mt)
#pragma unroll
                for (int q = 0; q < 16; ++q) {
                    const int r = row_of(mt, q, hh), g = g0 + r;
                    if (g >= a.P) continue;
                    const bool on = (float)s_xh[r * DLP + c] + (float)s_xl[r * DLP + c] > 0.0f;
                    a.d_lang[(size_t)g * C + c] = (a.residual ? s_v[r][c] : 0.0f) + (on ? acc[mt][q] : 0.0f);
                }
        }
    }
}

void launch_lang_deform_fwd(const LangDeformArgs& a, hipStream_t st) {
    if (a.P > 0) hipLaunchKernelGGL(k_lang_deform_fwd, dim3((a.P + DN - 1) / DN), dim3(256), 0, st, a);
}
void launch_lang_deform_bwd(const LangDeformArgs& a, hipStream_t st) {
    if (a.P > 0) hipLaunchKernelGGL(k_lang_deform_bwd, dim3((a.P + DN - 1) / DN), dim3(256), 0, st, a);
}

// ==== status centres (include/lsr_centers.h): lang_deform at S times per Gaussian, then k-means ====
// A block takes gpb Gaussians.  Their gpb * S rows (normalised language, time s of Gaussian g) go
// through lang_mlp_fwd in tiles of 64 -- a tile spans Gaussians, so only the block's last tile has
// idle rows -- and each normalised output row lands in s_x[row][D | 1], the samples.  A tile is handed
// to lang_mlp_fwd as a 64-Gaussian problem of its own whose language rows and times sit in LDS (s_tl,
// s_time): the MLP's code and arithmetic are k_lang_deform_fwd's.  Then wave w runs the k-means
// (centers_kmeans.h) of Gaussians w, w + 4, ... on those rows.  The samples reach memory only when
// samples_out is given.
__device__ __forceinline__ float centers_time(uint32_t seed, uint32_t g, uint32_t s) {   // lsr_centers.h
    uint32_t h = seed ^ (g * 0x9E3779B1u) ^ (s * 0x85EBCA77u);
    h ^= h >> 16;
    h *= 0x7FEB352Du;
    h ^= h >> 15;
    h *= 0x846CA68Bu;
    h ^= h >> 16;
    return (float)(h >> 8) * (1.0f / 16777216.0f);
}

constexpr int CF_MAX_GPB = 16;
__global__ void __launch_bounds__(256) k_centers_from_field(CentersArgs ca) {
    __shared__ __attribute__((aligned(16))) __bf16 s_xh[DN * DLP];
    __shared__ __attribute__((aligned(16))) __bf16 s_xl[DN * DLP];
    __shared__ __attribute__((aligned(16))) __bf16 s_hh[2][DN * DAP];
    __shared__ __attribute__((aligned(16))) __bf16 s_hl[2][DN * DAP];
    __shared__ float s_v[DN][33];
    __shared__ float s_x[CK_XFLOATS];
    __shared__ float s_lang[CF_MAX_GPB * 32];   // the block's normalised languages
    __shared__ float s_tl[DN * CK_MAX_D];       // the tile's language rows [64][D]
    __shared__ float s_time[DN];                // the tile's times
    __shared__ float s_c[4][CK_MAX_K * CK_MAX_D];
    __shared__ uint8_t s_a[4][CK_MAX_S];
    LDS_POISON(s_xh); LDS_POISON(s_xl); LDS_POISON(s_hh); LDS_POISON(s_hl); LDS_POISON(s_v); LDS_POISON(s_x);
    LDS_POISON(s_lang); LDS_POISON(s_tl); LDS_POISON(s_time); LDS_POISON(s_c); LDS_POISON(s_a); LDS_POISON_DONE();
    const LangDeformArgs& a = ca.f;
    const int tid = threadIdx.x, wave = tid >> 6, S = ca.S, D = a.lang_dim, xp = ck_pitch(D);
    const int g0 = blockIdx.x * ca.gpb, ng = min(ca.gpb, a.P - g0), nrows = ng * S;
    const int kpad = (a.kin + 15) / 16 * 16;
    LangDeformArgs tile = a;
    tile.lang = s_tl;
    tile.time = s_time;
    if (tid < ng) {   // l = lang / (|lang| + 1e-9)
        const float* l = a.lang + (size_t)(g0 + tid) * D;
        float n2 = 0.0f;
        for (int c = 0; c < D; ++c) n2 += l[c] * l[c];
        const float inv = 1.0f / (sqrtf(n2) + 1e-9f);
        for (int c = 0; c < D; ++c) s_lang[tid * 32 + c] = l[c] * inv;
    }
    __syncthreads();
    for (int r0 = 0; r0 < nrows; r0 += DN) {
        tile.P = min(DN, nrows - r0);
        for (int i = tid; i < tile.P * D; i += 256) s_tl[i] = s_lang[((r0 + i / D) / S) * 32 + i % D];
        if (tid < DN && r0 + tid < nrows) {
            const int lg = (r0 + tid) / S, s = (r0 + tid) - lg * S;
            const size_t at = (size_t)(g0 + lg) * S + s;
            const float t = ca.times ? ca.times[at] : centers_time(ca.seed, (uint32_t)(g0 + lg), (uint32_t)s);
            s_time[tid] = t;
            if (ca.times_out) ca.times_out[at] = t;
        }
        __syncthreads();   // the tile's rows and times; the previous tile's s_v read
        lang_mlp_fwd(tile, 0, kpad, s_xh, s_xl, s_hh, s_hl, s_v, false);
        if (tid < DN && r0 + tid < nrows) {   // x = v / (|v| + 1e-9), as k_lang_deform_fwd
            float n2 = 0.0f;
            for (int c = 0; c < D; ++c) n2 += s_v[tid][c] * s_v[tid][c];
            const float inv = 1.0f / (sqrtf(n2) + 1e-9f);
            float* xr = s_x + (r0 + tid) * xp;
            for (int c = 0; c < D; ++c) xr[c] = s_v[tid][c] * inv;
            if (ca.samples_out) {
                float* o = ca.samples_out + ((size_t)g0 * S + r0 + tid) * D;
                for (int c = 0; c < D; ++c) o[c] = xr[c];
            }
        }
    }
    __syncthreads();
    for (int lg = wave; lg < ng; lg += 4) {
        const size_t g = (size_t)(g0 + lg);
        kmeans_wave(s_x + lg * S * xp, xp, S, D, ca.K, ca.max_iter, s_c[wave], s_a[wave], ca.centers + g * ca.K * D,
                    ca.counts + g * ca.K, ca.inertia + g, ca.iters + g);
    }
}

void launch_centers_from_field(const CentersArgs& a, hipStream_t st) {
    if (a.f.P > 0) hipLaunchKernelGGL(k_centers_from_field, dim3((a.f.P + a.gpb - 1) / a.gpb), dim3(256), 0, st, a);
}

}  // namespace lsr
