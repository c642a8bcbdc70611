// deform_pack.hip -- the deformation field's batched layout kernels: the gradient planes' unpack
// (k_unpack_planes, both shapes) and the parameter pack of lsr_deform_prepare (k_pack_batch, 16 / 128).
#include "lsr_common.h"
#include "deform_internal.h"
#include "deform_mfma.h"
#include <algorithm>

namespace lsr {

// packed channel-last gradient replicas [r][H][W][C] -> torch [C][H][W], summed over the replicas
// and added, every plane of a call in one launch (one per plane was 12 launches of ~10 us each at
// the Neu3D planes, mostly launch gaps).  One block per 256 / C texels (256 floats; C = 16: 16, the
// figures below; C = 32: 8): each thread sums one float over the replicas with coalesced reads, the
// block transposes through LDS (pitch C + 1) and writes each channel's texels as one run (64 or 32 bytes).
// (A thread per destination float read 64-byte-strided words of every replica: 0.38 ms per training
// iteration at configs[4]'s planes.)  One extra block folds the box gradient's partial rows.
template <int C>
__global__ void __launch_bounds__(256) k_unpack_planes(const UnpackBatch u) {
    constexpr int T = 256 / C;   // texels per block
    __shared__ float s_t[T][C + 1];
    const int bid = blockIdx.x, t = threadIdx.x;
    if (bid == u.block0[u.n]) {   // block-uniform: the box gradient
        if (t < 6) {
            float acc = 0.0f;
            for (int r = 0; r < DEF_AABB_SLOTS; ++r) acc += u.daabb_part[r * 16 + t];
            u.daabb[t] += acc;
        }
        return;
    }
    LDS_POISON(s_t); LDS_POISON_DONE();
    int j = 0;
    while (j + 1 < u.n && bid >= u.block0[j + 1]) ++j;
    const int H = u.H[j], W = u.W[j], HW = H * W, base = (bid - u.block0[j]) * T;
    const int tex = t / C, ch = t % C;
    float acc = 0.0f;
    if (base + tex < HW) {
        const float* p = u.src + u.off[j] + (size_t)base * C + t;
        for (int r = 0; r < u.replicas; ++r) acc += p[(size_t)r * u.stride];
    }
    if (u.trow && u.toff[j] >= 0 && base + tex < HW) {   // block-uniform plane: its x-row, folded into
        // the two rows of time0 (tap_of's arithmetic for the time coordinate)
        const float iy = fminf(fmaxf((u.time0[0] + 1.0f) * 0.5f * (float)(H - 1), 0.0f), (float)(H - 1));
        const int y0 = (int)floorf(iy), y1 = min(y0 + 1, H - 1);
        const float fy = iy - (float)y0;
        const int y = (base + tex) / W, x = (base + tex) - y * W;
        if (y == y0 || y == y1) {
            float r = 0.0f;
            const float* rp = u.trow + u.toff[j] + x * C + ch;
            for (int k = 0; k < u.trow_reps; ++k) r += rp[(size_t)k * u.trow_stride];
            if (y == y0) acc += r * (1.0f - fy);
            if (y == y1) acc += r * fy;
        }
    }
    s_t[tex][ch] = acc;
    __syncthreads();
    const int c = t / T, tl = t % T;
    if (base + tl < HW) u.dst[j][(size_t)c * HW + base + tl] += s_t[tl][c];
}

void launch_unpack_planes(const UnpackBatch& u, int channels, hipStream_t st) {
    const int nb = u.block0[u.n] + (u.daabb ? 1 : 0);
    if (nb <= 0) return;
    if (channels == 16) hipLaunchKernelGGL(k_unpack_planes<16>, dim3(nb), dim3(256), 0, st, u);
    else hipLaunchKernelGGL(k_unpack_planes<32>, dim3(nb), dim3(256), 0, st, u);
}

// ---- parameter packing ----------------------------------------------------------------------------
// Every packing job of lsr_deform_prepare (planes, weights, transposed weights: ~34 per field) in
// one launch: block b runs job j where first[j] <= b < first[j + 1] (a scalar search over <= 48
// jobs), one thread per destination element i of the job's layout:
//   plane:             fp32 [16][H][W] (torch) -> fp32 [H][W][16], dst[hw][c] = src[c][hw]
//   weight:            fp32 [rows][cols] -> bf16 hi / lo [rows_pad][cols_pad], zero past rows / cols
//   transposed weight: fp32 [rows][cols] -> bf16 hi / lo [cols_pad][k_pad], dst[c][r] = src[r][c],
//                      zero for r >= rows, c >= cols
// (One launch per job left the device idle between ~34 tiny kernels every training iteration.)
__global__ void __launch_bounds__(256) k_pack_batch(PackBatch pb) {
    const uint32_t b = blockIdx.x;
    int j = 0;
    while (j + 1 < pb.n && b >= pb.j[j + 1].first_block) ++j;
    const PackJob& q = pb.j[j];
    const int i = (int)(b - q.first_block) * 256 + (int)threadIdx.x;
    if (q.kind == PACK_PLANE) {   // [16][H][W] -> [H][W][16]; a = H * W
        if (i >= q.a * 16) return;
        reinterpret_cast<float*>(q.hi)[i] = q.src[(size_t)(i & 15) * q.a + (i >> 4)];
        return;
    }
    float v;
    if (q.kind == PACK_WEIGHT) {   // [rows][cols] -> [rows_pad][cols_pad]; a rows, b rows_pad, c cols, d cols_pad
        if (i >= q.b * q.d) return;
        const int r = i / q.d, c = i - r * q.d;
        v = (r < q.a && c < q.c) ? q.src[(size_t)r * q.c + c] : 0.0f;
    } else {                       // transposed: a rows, b cols, c k_pad, d cols_pad
        if (i >= q.d * q.c) return;
        const int c = i / q.c, r = i - c * q.c;
        v = (r < q.a && c < q.b) ? q.src[(size_t)r * q.b + c] : 0.0f;
    }
    __bf16 h, l;
    dsplit(v, h, l);
    reinterpret_cast<__bf16*>(q.hi)[i] = h;
    q.lo[i] = l;
}

void launch_pack_batch(PackJob* jobs, int n, hipStream_t st) {
    for (int j0 = 0; j0 < n; j0 += PACK_MAX_JOBS) {
        PackBatch pb{};
        pb.n = std::min(PACK_MAX_JOBS, n - j0);
        uint32_t blocks = 0;
        for (int k = 0; k < pb.n; ++k) {
            PackJob q = jobs[j0 + k];
            const int64_t elems = q.kind == PACK_PLANE ? (int64_t)q.a * 16
                                  : q.kind == PACK_WEIGHT ? (int64_t)q.b * q.d : (int64_t)q.d * q.c;
            q.first_block = blocks;
            blocks += (uint32_t)((elems + 255) / 256);
            pb.j[k] = q;
        }
        if (blocks) hipLaunchKernelGGL(k_pack_batch, dim3(blocks), dim3(256), 0, st, pb);
    }
}

}  // namespace lsr
