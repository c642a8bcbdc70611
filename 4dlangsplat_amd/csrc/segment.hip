// segment.hip -- relevancy maps to masks, level scores and IoU counts (include/lsr_segment.h;
// eval/eval.py:143-315 activate_stream, eval/eval_utils.py:95-100 smooth_cuda).
//
// k_seg_blend   one 64-wide tile of one map per workgroup: the tile with a scale / 2 halo (zeros outside
//               the image) goes to LDS, the window sum is taken from LDS in separable form (row sums
//               left to right, then column sums top to bottom: 2 * scale LDS reads per pixel and an
//               order that does not depend on where the pixel is), divided by the analytic in-image
//               count, blended and stored; the tile's min and max of the blend go to the workspace.
// k_seg_minmax  one workgroup per map: the tile partials to the map's min and max (NaN is kept, which
//               fminf / fmaxf would drop), the "point" score, and the zeroing of the IoU counts.
// k_seg_mask    one 32 x 64 tile with a 3 pixel halo per workgroup: stretch and threshold into bytes in
//               LDS, mask_raw out, the 7 x 7 majority as the integer test 2 * ones > valid, mask out,
//               intersection and union by integer atomics, and for "mean" the tile's sum of the blend
//               over mask_raw in double with its count.
// k_seg_mean    one workgroup per map: the tile sums in a fixed order to the "mean" score.
// No float atomics: two calls give the same bits.  Element offsets are 64-bit.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <string>

#include "../../include/lsr.h"
#include "../../include/lsr_segment.h"
#include "lsr_host.h"
#include "lsr_wave.h"

namespace {

using lsr::lds_byte;
using lsr::lds_float;
using lsr::wave_sum;

constexpr int SG_THREADS = 256, SG_WAVES = SG_THREADS / 64;
constexpr int SG_TW = 64;             // tile width: one wave per tile row
constexpr int SG_TH = 32;             // tile height of k_seg_mask, and of k_seg_blend while it fits 64 KB of LDS
constexpr int SG_TH_SMALL = 16;       // k_seg_blend's tile height for the widest windows
constexpr int SG_CR = 3, SG_CW = 2 * SG_CR + 1;    // the cleaning window (smooth_cuda: 7 x 7)
constexpr int SG_RAW_PITCH = SG_TW + 2 * SG_CR + 2;
constexpr int SG_MAX_MAPS_PER_LAUNCH = 65535;      // gridDim.y
constexpr size_t SG_LDS_LIMIT = 64 * 1024 - 256;   // a block's LDS, less k_seg_blend's static reduction scratch

struct SegArgs {
    const float* rel;
    const uint8_t* gt;
    float* blended;
    uint8_t* mask_raw;
    uint8_t* mask;
    float* score;
    unsigned long long* inter;
    unsigned long long* uni;
    int H, W, r, th, tiles_x, tiles_b, tiles_m, gt_count, strategy;
    float thresh;
    float* tile_min;    // [n_maps][tiles_b]
    float* tile_max;
    float* map_min;     // [n_maps]
    float* map_max;
    double* tile_sum;   // [n_maps][tiles_m]
    int* tile_cnt;
};

int cdiv(int a, int b) { return (a + b - 1) / b; }

// LDS of one k_seg_blend block: the halo tile and its row sums
size_t blend_lds(int r, int th) { return (size_t)(th + 2 * r) * (size_t)(2 * SG_TW + 2 * r) * sizeof(float); }

// min / max / NaN flag of a block, to thread 0
struct MinMax {
    float mn, mx;
    int nan;
    __device__ __forceinline__ void add(float v) {
        nan |= (v != v);
        mn = fminf(mn, v);
        mx = fmaxf(mx, v);
    }
};

__device__ __forceinline__ MinMax block_minmax(MinMax v, float (*s_f)[SG_WAVES], int* s_n) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        v.mn = fminf(v.mn, __shfl_xor(v.mn, off));
        v.mx = fmaxf(v.mx, __shfl_xor(v.mx, off));
        v.nan |= __shfl_xor(v.nan, off);
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) {
        s_f[0][wave] = v.mn;
        s_f[1][wave] = v.mx;
        s_n[wave] = v.nan;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int k = 1; k < SG_WAVES; ++k) {
            v.mn = fminf(v.mn, s_f[0][k]);
            v.mx = fmaxf(v.mx, s_f[1][k]);
            v.nan |= s_n[k];
        }
    }
    return v;
}

__global__ void __launch_bounds__(SG_THREADS) k_seg_blend(SegArgs a, int m0) {
    extern __shared__ __attribute__((aligned(16))) float s_dyn[];
    __shared__ float s_f[2][SG_WAVES];
    __shared__ int s_n[SG_WAVES];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int H = a.H, W = a.W, r = a.r, th = a.th;
    const int pw = SG_TW + 2 * r, ph = th + 2 * r, taps = 2 * r + 1;
    const int ty = blockIdx.x / a.tiles_x, tx = blockIdx.x - ty * a.tiles_x;
    const int x0 = tx * SG_TW, y0 = ty * th;
    const int64_t m = (int64_t)m0 + blockIdx.y;
    const float* __restrict__ src = a.rel + m * H * W;
    float* __restrict__ dst = a.blended + m * H * W;
    lds_float* tile = (lds_float*)s_dyn;               // [ph][pw]
    lds_float* rs = tile + ph * pw;                    // [ph][SG_TW]

    // four rows of a wave at a time, both halves of a row (pw <= 128): eight loads in flight per lane
    for (int ly0 = wave; ly0 < ph; ly0 += 4 * SG_WAVES) {
        float v[4][2];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int ly = ly0 + j * SG_WAVES, gy = y0 - r + ly;
            const bool row_in = ly < ph && gy >= 0 && gy < H;
#pragma unroll
            for (int c = 0; c < 2; ++c) {
                const int lx = lane + 64 * c, gx = x0 - r + lx;
                v[j][c] = (row_in && lx < pw && gx >= 0 && gx < W) ? src[(int64_t)gy * W + gx] : 0.0f;
            }
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int ly = ly0 + j * SG_WAVES;
#pragma unroll
            for (int c = 0; c < 2; ++c) {
                const int lx = lane + 64 * c;
                if (ly < ph && lx < pw) tile[ly * pw + lx] = v[j][c];
            }
        }
    }
    __syncthreads();
    for (int ly = wave; ly < ph; ly += SG_WAVES) {
        const lds_float* p = tile + ly * pw + lane;
        float s = p[0];
        for (int d = 1; d < taps; ++d) s += p[d];
        rs[ly * SG_TW + lane] = s;
    }
    __syncthreads();

    MinMax mm{INFINITY, -INFINITY, 0};
    const int gx = x0 + lane;
    const int nx = min(gx + r, W - 1) - max(gx - r, 0) + 1;
    for (int y = wave; y < th; y += SG_WAVES) {
        const int gy = y0 + y;
        if (gy >= H) break;                            // wave-uniform
        const lds_float* p = rs + y * SG_TW + lane;
        float s = p[0];
        for (int d = 1; d < taps; ++d) s += p[d * SG_TW];
        if (gx < W) {
            const int ny = min(gy + r, H - 1) - max(gy - r, 0) + 1;
            const float avg = s / (float)(nx * ny);
            const float b = 0.5f * (avg + tile[(y + r) * pw + lane + r]);
            dst[(int64_t)gy * W + gx] = b;
            mm.add(b);
        }
    }
    mm = block_minmax(mm, s_f, s_n);
    if (tid == 0) {
        const int64_t t = m * a.tiles_b + blockIdx.x;
        a.tile_min[t] = mm.nan ? NAN : mm.mn;
        a.tile_max[t] = mm.nan ? NAN : mm.mx;
    }
}

__global__ void __launch_bounds__(SG_THREADS) k_seg_minmax(SegArgs a, int m0) {
    __shared__ float s_f[2][SG_WAVES];
    __shared__ int s_n[SG_WAVES];
    const int64_t m = (int64_t)m0 + blockIdx.x;
    MinMax mm{INFINITY, -INFINITY, 0};
    for (int t = threadIdx.x; t < a.tiles_b; t += SG_THREADS) {
        mm.add(a.tile_min[m * a.tiles_b + t]);
        mm.add(a.tile_max[m * a.tiles_b + t]);
    }
    mm = block_minmax(mm, s_f, s_n);
    if (threadIdx.x == 0) {
        const float mn = mm.nan ? NAN : mm.mn, mx = mm.nan ? NAN : mm.mx;
        a.map_min[m] = mn;
        a.map_max[m] = mx;
        if (a.strategy == LSR_SEGMENT_POINT) a.score[m] = mx;
        if (a.inter) {
            a.inter[m] = 0ull;
            a.uni[m] = 0ull;
        }
    }
}

__global__ void __launch_bounds__(SG_THREADS) k_seg_mask(SegArgs a, int m0) {
    __shared__ __attribute__((aligned(16))) uint8_t s_raw_[(SG_TH + 2 * SG_CR) * SG_RAW_PITCH];
    __shared__ __attribute__((aligned(16))) uint8_t s_row_[(SG_TH + 2 * SG_CR) * SG_TW];
    __shared__ int s_i[3][SG_WAVES];
    __shared__ double s_d[SG_WAVES];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int H = a.H, W = a.W;
    constexpr int PH = SG_TH + 2 * SG_CR, PW = SG_TW + 2 * SG_CR;
    const int ty = blockIdx.x / a.tiles_x, tx = blockIdx.x - ty * a.tiles_x;
    const int x0 = tx * SG_TW, y0 = ty * SG_TH;
    const int64_t m = (int64_t)m0 + blockIdx.y;
    const int64_t base = m * H * W;
    const float* __restrict__ bl = a.blended + base;
    lds_byte* s_raw = (lds_byte*)s_raw_;
    lds_byte* s_row = (lds_byte*)s_row_;

    // eval.py:186-189: o = b - min; o = o / (max(o) + 1e-9); o = o * 2 + (-1); clip(o, 0, 1).
    // max(b - min) is max(b) - min rounded once: the subtraction is monotonic.
    const float mn = a.map_min[m];
    const float den = (a.map_max[m] - mn) + 1e-9f;
    const float thresh = a.thresh;
    double sum = 0.0;
    int cnt = 0;
    // the halo tile as one run of PH * PW pixels over the block, four loads in flight per thread
    for (int i0 = tid; i0 < PH * PW; i0 += 4 * SG_THREADS) {
        float bv[4];
        bool in[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int i = i0 + j * SG_THREADS, ly = i / PW, lx = i - ly * PW;
            const int gy = y0 - SG_CR + ly, gx = x0 - SG_CR + lx;
            in[j] = i < PH * PW && gy >= 0 && gy < H && gx >= 0 && gx < W;
            bv[j] = in[j] ? bl[(int64_t)gy * W + gx] : 0.0f;
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int i = i0 + j * SG_THREADS, ly = i / PW, lx = i - ly * PW;
            if (i >= PH * PW) break;
            uint8_t raw = 0;
            if (in[j]) {
                const float b = bv[j];
                float o = b - mn;
                o = o / den;
                o = o * 2.0f;
                o = o + (-1.0f);
                o = o < 0.0f ? 0.0f : (o > 1.0f ? 1.0f : o);      // keeps NaN, as torch.clip
                raw = o > thresh ? 1 : 0;
                if (ly >= SG_CR && ly < SG_CR + SG_TH && lx >= SG_CR && lx < SG_CR + SG_TW) {
                    const int gy = y0 - SG_CR + ly, gx = x0 - SG_CR + lx;
                    a.mask_raw[base + (int64_t)gy * W + gx] = raw;
                    if (raw) {
                        sum += (double)b;
                        ++cnt;
                    }
                }
            }
            s_raw[ly * SG_RAW_PITCH + lx] = raw;
        }
    }
    __syncthreads();
    for (int ly = wave; ly < PH; ly += SG_WAVES) {
        const lds_byte* p = s_raw + ly * SG_RAW_PITCH + lane;
        int s = 0;
#pragma unroll
        for (int d = 0; d < SG_CW; ++d) s += p[d];
        s_row[ly * SG_TW + lane] = (uint8_t)s;
    }
    __syncthreads();

    int inter = 0, uni = 0;
    const int gx = x0 + lane;
    const int nx = min(gx + SG_CR, W - 1) - max(gx - SG_CR, 0) + 1;
    const uint8_t* __restrict__ gt = a.gt ? a.gt + (m % a.gt_count) * H * W : nullptr;
    for (int y = wave; y < SG_TH; y += SG_WAVES) {
        const int gy = y0 + y;
        if (gy >= H) break;                            // wave-uniform
        const lds_byte* p = s_row + y * SG_TW + lane;
        int ones = 0;
#pragma unroll
        for (int d = 0; d < SG_CW; ++d) ones += p[d * SG_TW];
        if (gx < W) {
            const int ny = min(gy + SG_CR, H - 1) - max(gy - SG_CR, 0) + 1;
            const int mk = 2 * ones > nx * ny ? 1 : 0;
            const int64_t idx = (int64_t)gy * W + gx;
            a.mask[base + idx] = (uint8_t)mk;
            if (gt) {
                const int g = gt[idx] != 0 ? 1 : 0;
                inter += g & mk;
                uni += g | mk;
            }
        }
    }

    // the tile's counts and sum: lanes by butterfly, waves in index order
    const bool mean = a.strategy == LSR_SEGMENT_MEAN;
    if (gt) {
        inter = wave_sum(inter);
        uni = wave_sum(uni);
    }
    if (mean) {
        sum = wave_sum(sum);
        cnt = wave_sum(cnt);
    }
    if (lane == 0) {
        s_i[0][wave] = inter;
        s_i[1][wave] = uni;
        s_i[2][wave] = cnt;
        s_d[wave] = sum;
    }
    __syncthreads();
    if (tid == 0) {
        if (gt) {
            const int ti = (s_i[0][0] + s_i[0][1]) + (s_i[0][2] + s_i[0][3]);
            const int tu = (s_i[1][0] + s_i[1][1]) + (s_i[1][2] + s_i[1][3]);
            if (ti) atomicAdd(a.inter + m, (unsigned long long)ti);
            if (tu) atomicAdd(a.uni + m, (unsigned long long)tu);
        }
        if (mean) {
            const int64_t t = m * a.tiles_m + blockIdx.x;
            a.tile_sum[t] = (s_d[0] + s_d[1]) + (s_d[2] + s_d[3]);
            a.tile_cnt[t] = (s_i[2][0] + s_i[2][1]) + (s_i[2][2] + s_i[2][3]);
        }
    }
}

// eval.py:262-276: the mean of the blend over mask_raw, 0 where the mask is empty.
__global__ void __launch_bounds__(SG_THREADS) k_seg_mean(SegArgs a, int m0) {
    __shared__ double s_d[SG_WAVES];
    __shared__ long long s_c[SG_WAVES];
    const int64_t m = (int64_t)m0 + blockIdx.x;
    const int tid = threadIdx.x;
    double sum = 0.0;
    long long cnt = 0;
    for (int t = tid; t < a.tiles_m; t += SG_THREADS) {
        sum += a.tile_sum[m * a.tiles_m + t];
        cnt += a.tile_cnt[m * a.tiles_m + t];
    }
    sum = wave_sum(sum);
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) cnt += __shfl_xor(cnt, off);   // (as wave_sum<long long> the kernel's code differs)
    if ((tid & 63) == 0) {
        s_d[tid >> 6] = sum;
        s_c[tid >> 6] = cnt;
    }
    __syncthreads();
    if (tid == 0) {
        const double S = (s_d[0] + s_d[1]) + (s_d[2] + s_d[3]);
        const long long C = (s_c[0] + s_c[1]) + (s_c[2] + s_c[3]);
        a.score[m] = C ? (float)(S / (double)C) : 0.0f;
    }
}

bool sizes_ok(int32_t n_maps, int32_t H, int32_t W) {
    return n_maps >= 0 && H >= 1 && H <= LSR_SEGMENT_MAX_SIDE && W >= 1 && W <= LSR_SEGMENT_MAX_SIDE;
}

// The workspace for any scale (k_seg_blend's tile count is bounded by its small tile height), carved
// into a's pointers; returns its bytes.
size_t carve(SegArgs& a, void* base, int64_t n_maps, int H, int W) {
    const size_t tiles_x = cdiv(W, SG_TW);
    const size_t nb = (size_t)n_maps * tiles_x * cdiv(H, SG_TH_SMALL), nm = (size_t)n_maps * tiles_x * cdiv(H, SG_TH);
    lsr::Carver c(base);
    a.tile_sum = c.take<double>(nm);
    a.tile_min = c.take<float>(nb);
    a.tile_max = c.take<float>(nb);
    a.map_min = c.take<float>((size_t)n_maps);
    a.map_max = c.take<float>((size_t)n_maps);
    a.tile_cnt = c.take<int>(nm);
    return c.total();
}

}  // namespace

extern "C" {

int64_t lsr_segment_workspace_bytes(int32_t n_maps, int32_t H, int32_t W) {
    if (!sizes_ok(n_maps, H, W)) {
        lsr::fail(LSR_EINVAL, "lsr_segment_workspace_bytes: n_maps >= 0 and 1 <= H, W <= 16384 required");
        return -1;
    }
    SegArgs a{};
    return (int64_t)carve(a, nullptr, n_maps, H, W);
}

int lsr_segment(int32_t n_maps, int32_t H, int32_t W, const float* rel, int32_t scale, float thresh, int32_t strategy,
                const uint8_t* gt, int32_t gt_count, float* blended, uint8_t* mask_raw, uint8_t* mask, float* score,
                int64_t* inter_count, int64_t* union_count, void* workspace, void* stream) {
    const std::string what = "lsr_segment";
    if (!sizes_ok(n_maps, H, W)) return lsr::fail(LSR_EINVAL, what + ": n_maps >= 0 and 1 <= H, W <= 16384 required");
    if (scale < 1 || scale > LSR_SEGMENT_MAX_SCALE || scale % 2 == 0)
        return lsr::fail(LSR_EINVAL, what + ": scale must be odd and in 1 ... 63, got " + std::to_string(scale));
    if (strategy != LSR_SEGMENT_POINT && strategy != LSR_SEGMENT_MEAN)
        return lsr::fail(LSR_EINVAL, what + ": strategy must be 0 (point) or 1 (mean)");
    if ((gt != nullptr) != (inter_count != nullptr) || (gt != nullptr) != (union_count != nullptr))
        return lsr::fail(LSR_EINVAL, what + ": gt, inter_count and union_count are given together or not at all");
    if (gt && gt_count < 1) return lsr::fail(LSR_EINVAL, what + ": gt_count >= 1 required with gt");
    if (n_maps == 0) return LSR_OK;
    if (!rel || !blended || !mask_raw || !mask || !score)
        return lsr::fail(LSR_EINVAL, what + ": null rel, blended, mask_raw, mask or score");
    if (!workspace) return lsr::fail(LSR_EINVAL, what + ": workspace required");
    if (!lsr::aligned16(workspace))
        return lsr::fail(LSR_EINVAL, what + ": the workspace must be 16-byte aligned");

    SegArgs a{};
    a.rel = rel;
    a.gt = gt;
    a.blended = blended;
    a.mask_raw = mask_raw;
    a.mask = mask;
    a.score = score;
    a.inter = reinterpret_cast<unsigned long long*>(inter_count);
    a.uni = reinterpret_cast<unsigned long long*>(union_count);
    a.H = H;
    a.W = W;
    a.r = scale / 2;
    a.th = blend_lds(a.r, SG_TH) <= SG_LDS_LIMIT ? SG_TH : SG_TH_SMALL;
    a.tiles_x = cdiv(W, SG_TW);
    a.tiles_b = a.tiles_x * cdiv(H, a.th);
    a.tiles_m = a.tiles_x * cdiv(H, SG_TH);
    a.gt_count = gt ? gt_count : 1;
    a.strategy = strategy;
    a.thresh = thresh;
    carve(a, workspace, n_maps, H, W);

    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const size_t lds = blend_lds(a.r, a.th);
    for (int m0 = 0; m0 < n_maps; m0 += SG_MAX_MAPS_PER_LAUNCH) {
        const int n = n_maps - m0 < SG_MAX_MAPS_PER_LAUNCH ? n_maps - m0 : SG_MAX_MAPS_PER_LAUNCH;
        hipLaunchKernelGGL(k_seg_blend, dim3(a.tiles_b, n), dim3(SG_THREADS), lds, st, a, m0);
        hipLaunchKernelGGL(k_seg_minmax, dim3(n), dim3(SG_THREADS), 0, st, a, m0);
        hipLaunchKernelGGL(k_seg_mask, dim3(a.tiles_m, n), dim3(SG_THREADS), 0, st, a, m0);
        if (strategy == LSR_SEGMENT_MEAN) hipLaunchKernelGGL(k_seg_mean, dim3(n), dim3(SG_THREADS), 0, st, a, m0);
    }
    return lsr::launched(what);
}

}  // extern "C"
