// tiles.hip -- language-feature tiles: label census, segment maps and 224 x 224 crops
// (include/lsr_tiles.h; preprocess/generate_clip_features.py:319-379 sam_encoder / mask2segmap and
// :156-170 of create).
//
// k_tiles_census  one level's 4 image rows per workgroup.  The table (count, W-1-xmin, xmax, H-1-ymin,
//                 ymax for 1024 label slots: every field starts at 0 and only grows, so the workspace is
//                 cleared by one memset) is privatised in 20 KB of LDS.  A wave reads 64 consecutive
//                 pixels of one row, so y is wave-uniform and a label's x range in the segment is the
//                 first and last set bit of the ballot of its lanes: one lane issues the five LDS atomics
//                 for each distinct label of the segment (one iteration over a constant region, not 64
//                 updates of one address).  The workgroup then merges the labels it saw into the global
//                 table with integer atomics.
// k_tiles_plan    one workgroup: per level the keep flags of the 1024 slots (four consecutive labels per
//                 thread), an exclusive scan in label order, the ranks, the descriptors and the counts.
// k_tiles_remap   seg_maps = rank[level][label], a gather from the 16 KB rank table.
// k_tiles_resize  one output pixel of one tile per thread, its three channels together: the four taps'
//                 label tests and image bytes, the integer blend, the division by 255.
// The render step is these last two launches: the remap streams 2 x 4 bytes per pixel of the frame and the
// resize is bound by its 600 KB of output per tile; neither reads what the other writes.
// Only integer atomics: two calls give the same bits.  Element offsets are 64-bit.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>

#include "../../include/lsr.h"
#include "../../include/lsr_tiles.h"
#include "lsr_host.h"

namespace {

constexpr int TL_THREADS = 256, TL_WAVES = TL_THREADS / 64;
constexpr int TL_SLOTS = LSR_TILES_MAX_LABEL + 1;     // a level's table is indexed by the label: slot 0 stays empty
constexpr int TL_ROWS = LSR_TILES_CENSUS_ROWS;
constexpr int TL_SIDE = LSR_TILES_SIDE;
constexpr int TL_REMAP_PIXELS = 4 * TL_THREADS;       // pixels of one k_tiles_remap workgroup
enum { F_CNT, F_NXMIN, F_XMAX, F_NYMIN, F_YMAX, F_N };
static_assert(TL_SLOTS == 4 * TL_THREADS, "k_tiles_plan: four labels per thread");
static_assert((TL_SIDE * TL_SIDE) % TL_THREADS == 0, "k_tiles_resize: whole workgroups per tile");

struct Workspace {
    int* census;    // [L][F_N][TL_SLOTS]
    int* rank;      // [L][TL_SLOTS]
    int* state;     // [0]: a label above the maximum was seen; [1..4]: the levels' kept counts; [5]: their sum
};

size_t carve(Workspace& w, void* base) {
    lsr::Carver c(base);
    w.census = c.take<int>((size_t)LSR_TILES_LEVELS * F_N * TL_SLOTS);
    w.state = c.take<int>(8);
    w.rank = c.take<int>((size_t)LSR_TILES_LEVELS * TL_SLOTS);
    return c.total();
}

// the labels of one 64-pixel row segment (x0 + lane; 0 where the lane is outside the row) into the LDS table
__device__ __forceinline__ void census_segment(int* s_t, int lab, int lane, int x0, int y, int H, int W) {
    const bool counts = lab >= 1 && lab <= LSR_TILES_MAX_LABEL;
    unsigned long long todo = __ballot(counts);
    while (todo) {                                                     // wave-uniform
        const int leader = __ffsll((long long)todo) - 1;
        const int cur = __builtin_amdgcn_readlane(lab, leader);
        const unsigned long long mine = __ballot(counts && lab == cur);
        if (lane == leader) {
            const int first = __ffsll((long long)mine) - 1, last = 63 - __clzll((long long)mine);
            atomicAdd(s_t + F_CNT * TL_SLOTS + cur, __popcll(mine));
            atomicMax(s_t + F_NXMIN * TL_SLOTS + cur, W - 1 - (x0 + first));
            atomicMax(s_t + F_XMAX * TL_SLOTS + cur, x0 + last);
            atomicMax(s_t + F_NYMIN * TL_SLOTS + cur, H - 1 - y);
            atomicMax(s_t + F_YMAX * TL_SLOTS + cur, y);
        }
        todo &= ~mine;
    }
}

__global__ void __launch_bounds__(TL_THREADS) k_tiles_census(const int32_t* __restrict__ labels, int H, int W, int segs,
                                                             Workspace ws) {
    __shared__ int s_t[F_N * TL_SLOTS];
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    for (int i = tid; i < F_N * TL_SLOTS; i += TL_THREADS) s_t[i] = 0;
    __syncthreads();

    const int lvl = blockIdx.y, y0 = blockIdx.x * TL_ROWS;
    const int rows = min(TL_ROWS, H - y0), n_seg = rows * segs;
    const int32_t* __restrict__ src = labels + (int64_t)lvl * H * W;
    bool over = false;
    // four segments of a wave at a time: four loads in flight per lane
    for (int s0 = wave; s0 < n_seg; s0 += 4 * TL_WAVES) {
        int lab[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int s = s0 + j * TL_WAVES, r = s / segs, x = (s - r * segs) * 64 + lane;
            lab[j] = (s < n_seg && x < W) ? src[(int64_t)(y0 + r) * W + x] : 0;
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int s = s0 + j * TL_WAVES, r = s / segs;
            if (s >= n_seg) break;                                     // wave-uniform
            over |= lab[j] > LSR_TILES_MAX_LABEL;
            census_segment(s_t, lab[j], lane, (s - r * segs) * 64, y0 + r, H, W);
        }
    }
    __syncthreads();

    int* g = ws.census + (size_t)lvl * F_N * TL_SLOTS;
    for (int l = tid; l < TL_SLOTS; l += TL_THREADS) {
        const int c = s_t[F_CNT * TL_SLOTS + l];
        if (c) {
            atomicAdd(g + F_CNT * TL_SLOTS + l, c);
#pragma unroll
            for (int f = F_NXMIN; f < F_N; ++f) atomicMax(g + f * TL_SLOTS + l, s_t[f * TL_SLOTS + l]);
        }
    }
    if (__ballot(over) && lane == 0) atomicOr(ws.state, 1);
}

__global__ void __launch_bounds__(TL_THREADS) k_tiles_plan(Workspace ws, int H, int W, int32_t* __restrict__ desc,
                                                           int32_t* __restrict__ counts) {
    __shared__ int s_w[TL_WAVES];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int base = 0;
    for (int lvl = 0; lvl < LSR_TILES_LEVELS; ++lvl) {
        const int* g = ws.census + (size_t)lvl * F_N * TL_SLOTS;
        int x[4], y[4], w[4], h[4], kept = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int l = 4 * tid + k;
            x[k] = W - 1 - g[F_NXMIN * TL_SLOTS + l];
            y[k] = H - 1 - g[F_NYMIN * TL_SLOTS + l];
            w[k] = g[F_XMAX * TL_SLOTS + l] - x[k];
            h[k] = g[F_YMAX * TL_SLOTS + l] - y[k];
            if (g[F_CNT * TL_SLOTS + l] == 0 || w[k] == 0 || h[k] == 0) w[k] = 0;     // w == 0: not kept
            kept += w[k] != 0;
        }
        int incl = kept;                                               // inclusive scan over the wave's lanes
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const int t = __shfl_up(incl, off);
            if (lane >= off) incl += t;
        }
        if (lane == 63) s_w[wave] = incl;
        __syncthreads();
        int before = 0, total = 0;
#pragma unroll
        for (int k = 0; k < TL_WAVES; ++k) {
            before += k < wave ? s_w[k] : 0;
            total += s_w[k];
        }
        int pos = base + before + incl - kept;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int l = 4 * tid + k;
            ws.rank[lvl * TL_SLOTS + l] = w[k] != 0 ? pos : -1;
            if (w[k] != 0) {
                int32_t* d = desc + (size_t)pos * LSR_TILES_DESC_INTS;
                d[0] = lvl;
                d[1] = l;
                d[2] = x[k];
                d[3] = y[k];
                d[4] = w[k];
                d[5] = h[k];
                ++pos;
            }
        }
        if (tid == 0) {
            counts[lvl] = total;
            ws.state[1 + lvl] = total;
        }
        base += total;
        __syncthreads();                                               // s_w is written again
    }
    if (tid == 0) {
        counts[LSR_TILES_LEVELS] = ws.state[0] != 0;
        ws.state[1 + LSR_TILES_LEVELS] = base;
    }
}

__global__ void __launch_bounds__(TL_THREADS) k_tiles_remap(const int32_t* __restrict__ labels, int64_t n_pix,
                                                            const int* __restrict__ rank, int32_t* __restrict__ seg) {
    const int lvl = blockIdx.y;
    const int64_t at = (int64_t)lvl * n_pix, p0 = (int64_t)blockIdx.x * TL_REMAP_PIXELS + threadIdx.x;
    int lab[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int64_t p = p0 + j * TL_THREADS;
        lab[j] = p < n_pix ? labels[at + p] : 0;
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int64_t p = p0 + j * TL_THREADS;
        if (p < n_pix) seg[at + p] = (lab[j] >= 1 && lab[j] <= LSR_TILES_MAX_LABEL) ? rank[lvl * TL_SLOTS + lab[j]] : -1;
    }
}

// output index d of a side-l source: the first tap s and the weight a (of 448) of the second, min(s + 1, l - 1)
__device__ __forceinline__ void resize_tap(int d, int l, int& s, int& a) {
    const int t = (2 * d + 1) * l - TL_SIDE;
    s = t < 0 ? 0 : t / (2 * TL_SIDE);
    a = t < 0 ? 0 : t - s * (2 * TL_SIDE);
    if (s >= l - 1) {
        s = l - 1;
        a = 0;
    }
}

__global__ void __launch_bounds__(TL_THREADS) k_tiles_resize(const int32_t* __restrict__ labels,
                                                             const uint8_t* __restrict__ image, int H, int W,
                                                             const int32_t* __restrict__ desc, const int* __restrict__ state,
                                                             float* __restrict__ tiles) {
    const int t = blockIdx.y;
    const int idx = blockIdx.x * TL_THREADS + threadIdx.x, dy = idx / TL_SIDE, dx = idx - dy * TL_SIDE;
    float* __restrict__ out = tiles + (int64_t)t * 3 * TL_SIDE * TL_SIDE + idx;
    int S[3] = {0, 0, 0};
    if (t < state[1 + LSR_TILES_LEVELS]) {                             // (a tile the plan did not write: zeros)
        const int32_t* d = desc + (size_t)t * LSR_TILES_DESC_INTS;
        const int lvl = d[0], label = d[1], x = d[2], y = d[3], w = d[4], h = d[5];
        const int l = max(w, h), ox = h > w ? (h - w) / 2 : 0, oy = h > w ? 0 : (w - h) / 2;
        const int32_t* __restrict__ lab = labels + (int64_t)lvl * H * W;
        int sx, ax, sy, ay;
        resize_tap(dx, l, sx, ax);
        resize_tap(dy, l, sy, ay);
        const int cx[2] = {sx - ox, min(sx + 1, l - 1) - ox}, wx[2] = {2 * TL_SIDE - ax, ax};
        const int cy[2] = {sy - oy, min(sy + 1, l - 1) - oy}, wy[2] = {2 * TL_SIDE - ay, ay};
        int64_t at[4];
        int wgt[4], got[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int jx = j & 1, jy = j >> 1, ix = x + cx[jx], iy = y + cy[jy];
            wgt[j] = wx[jx] * wy[jy];
            const bool in = wgt[j] != 0 && cx[jx] >= 0 && cx[jx] < w && cy[jy] >= 0 && cy[jy] < h && ix < W && iy < H;
            at[j] = (int64_t)iy * W + ix;
            got[j] = in ? lab[at[j]] : 0;                              // (the tile's label is >= 1)
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (got[j] == label) {
                const uint8_t* __restrict__ px = image + at[j] * 3;
#pragma unroll
                for (int c = 0; c < 3; ++c) S[c] += wgt[j] * (int)px[c];
            }
        }
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const int byte = (S[c] + 2 * TL_SIDE * TL_SIDE) / (4 * TL_SIDE * TL_SIDE);
        out[(int64_t)c * TL_SIDE * TL_SIDE] = (float)byte / 255.0f;
    }
}

int cdiv(int a, int b) { return (a + b - 1) / b; }

// the checks every step shares; LSR_OK or the refusal
int frame_ok(const std::string& what, int32_t L, int32_t H, int32_t W, int64_t workspace_bytes, const void* workspace) {
    if (L != LSR_TILES_LEVELS) return lsr::fail(LSR_EINVAL, what + ": L must be 4, got " + std::to_string(L));
    if (H < 1 || H > LSR_TILES_MAX_SIDE || W < 1 || W > LSR_TILES_MAX_SIDE)
        return lsr::fail(LSR_EINVAL, what + ": 1 <= H, W <= 16384 required");
    if (!workspace) return lsr::fail(LSR_EINVAL, what + ": workspace required");
    Workspace w{};
    if (workspace_bytes < (int64_t)carve(w, nullptr))
        return lsr::fail(LSR_EINVAL, what + ": the workspace is smaller than lsr_tiles_workspace_size");
    if (!lsr::aligned16(workspace)) return lsr::fail(LSR_EINVAL, what + ": the workspace must be 16-byte aligned");
    return LSR_OK;
}

}  // namespace

extern "C" {

int64_t lsr_tiles_workspace_size(int32_t L) {
    if (L != LSR_TILES_LEVELS) {
        lsr::fail(LSR_EINVAL, "lsr_tiles_workspace_size: L must be 4, got " + std::to_string(L));
        return -1;
    }
    Workspace w{};
    return (int64_t)carve(w, nullptr);
}

int lsr_tiles_census(int32_t L, int32_t H, int32_t W, const int32_t* labels, int64_t workspace_bytes, void* workspace,
                     void* stream) {
    const std::string what = "lsr_tiles_census";
    if (int rc = frame_ok(what, L, H, W, workspace_bytes, workspace)) return rc;
    if (!labels) return lsr::fail(LSR_EINVAL, what + ": null labels");
    Workspace w{};
    carve(w, workspace);
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    // the census and the state, which are adjacent: every field starts at 0
    const size_t clear = (size_t)(reinterpret_cast<char*>(w.rank) - reinterpret_cast<char*>(w.census));
    if (hipError_t e = hipMemsetAsync(w.census, 0, clear, st); e != hipSuccess) return lsr::launched(what + " (clear)", e);
    hipLaunchKernelGGL(k_tiles_census, dim3(cdiv(H, TL_ROWS), L), dim3(TL_THREADS), 0, st, labels, H, W, cdiv(W, 64), w);
    return lsr::launched(what);
}

int lsr_tiles_plan(int32_t L, int32_t H, int32_t W, int64_t workspace_bytes, void* workspace, int32_t* desc,
                   int32_t* counts, void* stream) {
    const std::string what = "lsr_tiles_plan";
    if (int rc = frame_ok(what, L, H, W, workspace_bytes, workspace)) return rc;
    if (!desc || !counts) return lsr::fail(LSR_EINVAL, what + ": null desc or counts");
    Workspace w{};
    carve(w, workspace);
    // page-locked host memory is written through its device alias
    void* alias = nullptr;
    if (hipHostGetDevicePointer(&alias, counts, 0) != hipSuccess || !alias) {
        (void)hipGetLastError();   // device memory: clear the sticky error of the failed query
        alias = counts;
    }
    hipLaunchKernelGGL(k_tiles_plan, dim3(1), dim3(TL_THREADS), 0, reinterpret_cast<hipStream_t>(stream), w, H, W, desc,
                       static_cast<int32_t*>(alias));
    return lsr::launched(what);
}

int lsr_tiles_render(int32_t L, int32_t H, int32_t W, const int32_t* labels, const uint8_t* image,
                     int64_t workspace_bytes, const void* workspace, const int32_t* desc, const int32_t* lengths, int32_t n,
                     int32_t* seg_maps, float* tiles, void* stream) {
    const std::string what = "lsr_tiles_render";
    if (int rc = frame_ok(what, L, H, W, workspace_bytes, workspace)) return rc;
    if (!labels || !image || !desc || !lengths || !seg_maps)
        return lsr::fail(LSR_EINVAL, what + ": null labels, image, desc, lengths or seg_maps");
    int64_t sum = 0;
    for (int k = 0; k < LSR_TILES_LEVELS; ++k) {
        if (lengths[k] < 0 || lengths[k] > LSR_TILES_MAX_LABEL)
            return lsr::fail(LSR_EINVAL, what + ": lengths[" + std::to_string(k) + "] = " + std::to_string(lengths[k]) +
                                             " is outside 0 ... 1023");
        sum += lengths[k];
    }
    if (n != sum)
        return lsr::fail(LSR_EINVAL, what + ": n = " + std::to_string(n) + " tiles, but the plan's lengths sum to " +
                                         std::to_string(sum));
    if (n > 0 && !tiles) return lsr::fail(LSR_EINVAL, what + ": null tiles");
    Workspace w{};
    carve(w, const_cast<void*>(workspace));
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const int64_t n_pix = (int64_t)H * W;
    hipLaunchKernelGGL(k_tiles_remap, dim3((unsigned)((n_pix + TL_REMAP_PIXELS - 1) / TL_REMAP_PIXELS), L),
                       dim3(TL_THREADS), 0, st, labels, n_pix, w.rank, seg_maps);
    if (n > 0)
        hipLaunchKernelGGL(k_tiles_resize, dim3(TL_SIDE * TL_SIDE / TL_THREADS, n), dim3(TL_THREADS), 0, st, labels, image,
                           H, W, desc, w.state, tiles);
    return lsr::launched(what);
}

}  // extern "C"
