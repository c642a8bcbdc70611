// deform_wgrad.hip -- the deformation backward's weight gradients: the heads by recompute
// (k_head_wgrad2, k_head_wgrad3) and the split-K A^T B products of saved rows (k_atb, which the 32 / 64
// shape of deform_narrow.hip uses too), on the bf16 hi/lo MFMA helpers of deform_mfma.h.
#include "lsr_common.h"
#include "deform_internal.h"
#include "deform_mfma.h"
#include <algorithm>

namespace lsr {

// ==== head weight gradients by recompute ===========================================================
// Phase A saves no per-head rows (relu(Z1) and dZ1 would be 2 x 128 floats per Gaussian per head:
// 10 GB written and read back at 2M Gaussians with five heads).  A block of k_head_wgrad2 (the wide
// head) or k_head_wgrad3 (the small heads) walks its rows in tiles of 64 and recomputes them from the
// saved trunk activation A (512 B per row) and the head's output gradient G:
//   Z1 = A W1^T + b1 (as the forward),  dZ1 = (G W2) * [Z1 > 0] (as phase A),
//   dW1 += dZ1^T A,  dW2 += G^T relu(Z1),  db1 += sum dZ1,  db2 += sum G,
// accumulating the block's partial products in registers over all its tiles; one atomic per output
// element at the end.  The reduction index of the last two products is the row: wave w holds
// dZ1 and relu(Z1) for its 32 columns in the MFMA result layout, whose rows split 4 / 4 between the
// two half-waves, so one permlane32 swap per register pair turns them into the row-runs of 8 the
// 32x32x16 operands take; the A and G operands come from their LDS rows through transposing reads.
// Rows past P read as zero (their dZ1 and G vanish, so relu(b1) never reaches a product).
__device__ __forceinline__ void wg_regs_to_op(const df32x16& v, int u, dbf16x8& oh, dbf16x8& ol) {
    // rows 16u .. 16u + 15 of this 32-row M tile: lane half h gets rows 16u + 8h .. + 7
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        auto r = __builtin_amdgcn_permlane32_swap(__float_as_uint(v[8 * u + i]), __float_as_uint(v[8 * u + 4 + i]),
                                                  false, false);
        const float x0 = __uint_as_float(r[0]), x1 = __uint_as_float(r[1]);
        __bf16 h0, l0, h1, l1;
        dsplit(x0, h0, l0);
        dsplit(x1, h1, l1);
        oh[i] = h0; ol[i] = l0;
        oh[4 + i] = h1; ol[4 + i] = l1;
    }
}
// 8 consecutive rows (16 ks + 8 h ..) of column c0 + (lane & 31) of a row-major bf16 LDS array,
// through two ds_read_b64_tr_b16 (each 16-lane group reads a 4-row x 16-column block)
__device__ __forceinline__ dbf16x8 wg_lds_op(const __bf16* base, int pitch, int ks, int c0) {
    const int lane = threadIdx.x & 63, h = lane >> 5, l16 = lane & 15;
    const __bf16* p = base + (16 * ks + 8 * h + (l16 >> 2)) * pitch + c0 + 16 * ((lane >> 4) & 1) + 4 * (l16 & 3);
    typedef short s16x4 __attribute__((ext_vector_type(4)));
    typedef short s16x8 __attribute__((ext_vector_type(8)));
    const s16x4 a0 = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
        reinterpret_cast<__attribute__((address_space(3))) s16x4*>(reinterpret_cast<size_t>(p)));
    const s16x4 a1 = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
        reinterpret_cast<__attribute__((address_space(3))) s16x4*>(reinterpret_cast<size_t>(p + 4 * pitch)));
    const s16x8 v = __builtin_shufflevector(a0, a1, 0, 1, 2, 3, 4, 5, 6, 7);
    return __builtin_bit_cast(dbf16x8, v);
}

// The wide head (SH: more than DEF_SMALL_OUT outputs, every product on the matrix core), at ONE wave
// per SIMD: 512 registers per wave, the accumulators in AGPRs.  What every 64-row tile needs stays
// on the CU for the whole block -- the wave's W1 fragments in registers (its 32 columns, K = 128: 64
// registers) and W2^T in LDS (registers would spill) -- and the next tile's A and G rows are loaded
// into registers while the current tile computes, so a tile waits neither on an L2 round trip of
// weight fragments nor on its own rows.  256 blocks per wide head: one round of the 256 CUs.
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(1, 1))) k_head_wgrad2(HeadWgradArgs ha, int job0) {
    __shared__ __attribute__((aligned(16))) __bf16 s_ah[DN * DAP];   // A rows [64][128] hi / lo
    __shared__ __attribute__((aligned(16))) __bf16 s_al[DN * DAP];
    __shared__ __attribute__((aligned(16))) __bf16 s_gh[DN * DGP];   // G rows [64][64 pad] hi / lo
    __shared__ __attribute__((aligned(16))) __bf16 s_gl[DN * DGP];
    __shared__ __attribute__((aligned(16))) __bf16 s_w2h[DWID * DLP];   // W2^T [128][64 pad]
    __shared__ __attribute__((aligned(16))) __bf16 s_w2l[DWID * DLP];
    LDS_POISON(s_ah); LDS_POISON(s_al); LDS_POISON(s_gh); LDS_POISON(s_gl); LDS_POISON(s_w2h); LDS_POISON(s_w2l);
    LDS_POISON_DONE();
    typedef __bf16 bf4 __attribute__((ext_vector_type(4)));
    const HeadWgradJob& j = ha.job[job0 + blockIdx.y];
    const int64_t row0 = (int64_t)blockIdx.x * ha.rows_per_block;
    const int64_t row1 = min((int64_t)ha.P, row0 + ha.rows_per_block);
    if (row0 >= row1) return;                                            // block-uniform
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, r = lane & 31, hh = lane >> 5;
    const int nout = j.nout, Mo = (nout + 31) / 32;                      // G^T M tiles (1 or 2)
    const int col = 32 * wave + r;
    const float b1c = j.b1[col];
    // ---- the wave's weight fragments, once per block ---------------------------------------------------
    dbf16x8 w1h[DWID / 16], w1l[DWID / 16];
#pragma unroll
    for (int ks = 0; ks < DWID / 16; ++ks) {
        const size_t wo = (size_t)col * DWID + 16 * ks + 8 * hh;
        w1h[ks] = *reinterpret_cast<const dbf16x8*>(j.w1_h + wo);
        w1l[ks] = *reinterpret_cast<const dbf16x8*>(j.w1_l + wo);
    }
    for (int i = tid; i < DWID * 64 / 8; i += 256) {   // W2^T into LDS, visible after the first barrier
        const int rr = i >> 3, c8 = (i & 7) * 8;
        *reinterpret_cast<dbf16x8*>(s_w2h + rr * DLP + c8) = *reinterpret_cast<const dbf16x8*>(j.w2t_h + rr * 64 + c8);
        *reinterpret_cast<dbf16x8*>(s_w2l + rr * DLP + c8) = *reinterpret_cast<const dbf16x8*>(j.w2t_l + rr * 64 + c8);
    }
    df32x16 w1acc[4] = {df32x16{}, df32x16{}, df32x16{}, df32x16{}};   // dW1 rows 32 wave .., col tiles 0..3
    df32x16 w2acc[2] = {df32x16{}, df32x16{}};                           // dW2 o tiles 0..1, col tile wave
    float db1 = 0.0f, db2 = 0.0f;
    // ---- the tile's rows in registers: A (thread: 8 float4 of rows (tid + 256 i) >> 5), G ---------------
    float4 pa[DN * DWID / 4 / 256];
    float pg[DN * 64 / 256];
    auto load_tile = [&](int64_t t0) __attribute__((always_inline)) {
#pragma unroll
        for (int i = 0; i < DN * DWID / 4 / 256; ++i) {
            const int e = tid + 256 * i, rr = e >> 5, c4 = (e & 31) * 4;
            const int64_t g = t0 + rr;
            pa[i] = g < row1 ? *reinterpret_cast<const float4*>(ha.A + g * DWID + c4) : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        }
#pragma unroll
        for (int i = 0; i < DN * 64 / 256; ++i) {
            const int e = tid + 256 * i, rr = e >> 6, k = e & 63;
            const int64_t g = t0 + rr;
            pg[i] = (k < nout && g < row1) ? j.G[g * nout + k] : 0.0f;
        }
    };
    auto store_tile = [&]() __attribute__((always_inline)) {
#pragma unroll
        for (int i = 0; i < DN * DWID / 4 / 256; ++i) {
            const int e = tid + 256 * i, rr = e >> 5, c4 = (e & 31) * 4;
            const float f[4] = {pa[i].x, pa[i].y, pa[i].z, pa[i].w};
            bf4 h4, l4;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                __bf16 hi, lo;
                dsplit(f[q], hi, lo);
                h4[q] = hi; l4[q] = lo;
            }
            *reinterpret_cast<bf4*>(s_ah + rr * DAP + c4) = h4;
            *reinterpret_cast<bf4*>(s_al + rr * DAP + c4) = l4;
        }
#pragma unroll
        for (int i = 0; i < DN * 64 / 256; ++i) {   // column k = tid & 63 for every i: db2 in a register
            const int e = tid + 256 * i, rr = e >> 6, k = e & 63;
            db2 += pg[i];
            __bf16 hi, lo;
            dsplit(pg[i], hi, lo);
            s_gh[rr * DGP + k] = hi;
            s_gl[rr * DGP + k] = lo;
        }
    };
    load_tile(row0);
    for (int64_t t0 = row0; t0 < row1; t0 += DN) {
        store_tile();
        __syncthreads();
        if (t0 + DN < row1) load_tile(t0 + DN);   // in flight while this tile computes
        // ---- Z1 for this wave's 32 columns (both row tiles), then dW2 and dZ1 ------------------------------
        uint32_t zpos = 0;   // bit 16 mt + q: Z1 > 0
        df32x16 d[2] = {df32x16{}, df32x16{}};
        {
            df32x16 z[2] = {df32x16{}, df32x16{}};
#pragma unroll
            for (int ks = 0; ks < DWID / 16; ++ks) {
                const int k0 = 16 * ks + 8 * hh;
#pragma unroll
                for (int mt = 0; mt < 2; ++mt) {
                    const dbf16x8 ah = *reinterpret_cast<const dbf16x8*>(s_ah + (32 * mt + r) * DAP + k0);
                    const dbf16x8 al = *reinterpret_cast<const dbf16x8*>(s_al + (32 * mt + r) * DAP + k0);
                    z[mt] = DMFMA(ah, w1h[ks], z[mt]);
                    z[mt] = DMFMA(ah, w1l[ks], z[mt]);
                    z[mt] = DMFMA(al, w1h[ks], z[mt]);
                }
            }
#pragma unroll
            for (int mt = 0; mt < 2; ++mt)
#pragma unroll
                for (int q = 0; q < 16; ++q) {
                    const float zz = z[mt][q] + b1c;
                    zpos |= zz > 0.0f ? 1u << (16 * mt + q) : 0u;
                    z[mt][q] = fmaxf(zz, 0.0f);
                }
#pragma unroll
            for (int ks = 0; ks < DN / 16; ++ks) {
                dbf16x8 zh, zl;
                wg_regs_to_op(z[ks >> 1], ks & 1, zh, zl);
#pragma unroll
                for (int mo = 0; mo < 2; ++mo) {
                    if (mo >= Mo) break;
                    const dbf16x8 gh = wg_lds_op(s_gh, DGP, ks, 32 * mo), gl = wg_lds_op(s_gl, DGP, ks, 32 * mo);
                    w2acc[mo] = DMFMA(gh, zh, w2acc[mo]);
                    w2acc[mo] = DMFMA(gh, zl, w2acc[mo]);
                    w2acc[mo] = DMFMA(gl, zh, w2acc[mo]);
                }
            }
        }
        // ---- dZ1 = (G W2) [Z1 > 0] -> dW1 += dZ1^T A (rows 32 wave .. of dW1), db1 ------------------------
        {
#pragma unroll
            for (int ks = 0; ks < 4; ++ks) {
                const int k0 = 16 * ks + 8 * hh;
                const dbf16x8 w2h = *reinterpret_cast<const dbf16x8*>(s_w2h + col * DLP + k0);
                const dbf16x8 w2l = *reinterpret_cast<const dbf16x8*>(s_w2l + col * DLP + k0);
#pragma unroll
                for (int mt = 0; mt < 2; ++mt) {
                    const dbf16x8 gh = *reinterpret_cast<const dbf16x8*>(s_gh + (32 * mt + r) * DGP + k0);
                    const dbf16x8 gl = *reinterpret_cast<const dbf16x8*>(s_gl + (32 * mt + r) * DGP + k0);
                    d[mt] = DMFMA(gh, w2h, d[mt]);
                    d[mt] = DMFMA(gh, w2l, d[mt]);
                    d[mt] = DMFMA(gl, w2h, d[mt]);
                }
            }
#pragma unroll
            for (int mt = 0; mt < 2; ++mt)
#pragma unroll
                for (int q = 0; q < 16; ++q) {
                    d[mt][q] = (zpos >> (16 * mt + q)) & 1u ? d[mt][q] : 0.0f;
                    db1 += d[mt][q];
                }
#pragma unroll
            for (int ks = 0; ks < DN / 16; ++ks) {
                dbf16x8 dh, dl;
                wg_regs_to_op(d[ks >> 1], ks & 1, dh, dl);
#pragma unroll
                for (int nt = 0; nt < 4; ++nt) {
                    const dbf16x8 bh = wg_lds_op(s_ah, DAP, ks, 32 * nt), bl = wg_lds_op(s_al, DAP, ks, 32 * nt);
                    w1acc[nt] = DMFMA(dh, bh, w1acc[nt]);
                    w1acc[nt] = DMFMA(dh, bl, w1acc[nt]);
                    w1acc[nt] = DMFMA(dl, bh, w1acc[nt]);
                }
            }
        }
        __syncthreads();   // the tile's LDS rows read before the next tile's are stored
    }
    // ---- the block's partial products: one atomic per element ------------------------------------------
#pragma unroll
    for (int nt = 0; nt < 4; ++nt)
#pragma unroll
        for (int q = 0; q < 16; ++q) {
            const int m = 32 * wave + (q & 3) + 8 * (q >> 2) + 4 * hh;
            atomicAdd(j.dW1 + (size_t)m * DWID + 32 * nt + r, w1acc[nt][q]);
        }
    db1 += __shfl_xor(db1, 32);
    if (hh == 0) atomicAdd(j.db1 + col, db1);
#pragma unroll
    for (int mo = 0; mo < 2; ++mo) {
        if (mo >= Mo) break;
#pragma unroll
        for (int q = 0; q < 16; ++q) {
            const int o = 32 * mo + (q & 3) + 8 * (q >> 2) + 4 * hh;
            if (o < nout) atomicAdd(j.dW2 + (size_t)o * DWID + col, w2acc[mo][q]);
        }
    }
    if ((tid & 63) < nout) atomicAdd(j.db2 + (tid & 63), db2);   // one partial per wave
}

// The small heads (at most DEF_SMALL_OUT outputs: G W2 and G^T relu(Z1) on the VALU from fp32 G rows,
// Z1 and dW1 on the matrix core), software-pipelined across tiles so that one wave per SIMD keeps its
// matrix core fed.  The wave's W1 hi fragments stay in registers for the whole block and the
// accumulators in AGPRs.  Three LDS tile buffers; iteration t runs
//   A: Z1 of tile t + 1 (MFMA, buffer t + 1)  beside  relu / dZ1 / dW2 of tile t (VALU, Z1(t) in registers)
//   B: dW1 += dZ1(t)^T A(t) (MFMA, buffer t)   beside  tile t + 2's rows into buffer t + 2 (VALU + LDS stores)
// then tile t + 3's rows are loaded into registers and one barrier ends the iteration (buffer t is
// free for tile t + 3, tile t + 2 is visible).  An iteration is branch-free (loads at clamped rows,
// zeros selected past the block's rows; Z1 past the last tile is computed and dropped) and each stage
// interleaves its two chains by hand, K step by K step, fenced by sched_barrier (sched_group_barrier
// patterns did not take: the compiler hoisted the VALU chain out of the MFMA region).  With the two
// chains run one after the other, tile by tile, the four small heads took 2.27 ms at 2M; interleaved
// 2.03 ms.  W1's lo half sits in LDS (registers hold the hi half) so that nothing spills.  64 blocks
// per small head: the four share each row range on one XCD (grid x is a multiple of 8), so their A
// reads meet in that XCD's L2, and the launch is one round of the 256 CUs.
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(1, 1))) k_head_wgrad3(HeadWgradArgs ha, int job0) {
    constexpr int NB = 3;
    __shared__ __attribute__((aligned(16))) __bf16 s_ah[NB][DN * DAP];   // A rows [64][128] hi / lo
    __shared__ __attribute__((aligned(16))) __bf16 s_al[NB][DN * DAP];
    __shared__ __attribute__((aligned(16))) float4 s_g4[NB][DN];         // G rows fp32
    __shared__ __attribute__((aligned(16))) __bf16 s_w1l[DWID * DAP];    // W1 lo [128][128] (hi in registers)
    LDS_POISON(s_ah); LDS_POISON(s_al); LDS_POISON(s_g4); LDS_POISON(s_w1l); LDS_POISON_DONE();
    typedef __bf16 bf4 __attribute__((ext_vector_type(4)));
    const HeadWgradJob& j = ha.job[job0 + blockIdx.y];
    const int64_t row0 = (int64_t)blockIdx.x * ha.rows_per_block;
    const int64_t row1 = min((int64_t)ha.P, row0 + ha.rows_per_block);
    if (row0 >= row1) return;                                            // block-uniform
    const int T = (int)((row1 - row0 + DN - 1) / DN);                    // tiles of this block
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, r = lane & 31, hh = lane >> 5;
    const int nout = j.nout;
    const int col = 32 * wave + r;
    const float b1c = j.b1[col];
    dbf16x8 w1h[DWID / 16];
#pragma unroll
    for (int ks = 0; ks < DWID / 16; ++ks)
        w1h[ks] = *reinterpret_cast<const dbf16x8*>(j.w1_h + (size_t)col * DWID + 16 * ks + 8 * hh);
    for (int i = tid; i < DWID * DWID / 8; i += 256) {   // visible after the prologue's barrier
        const int rr = i >> 4, c8 = (i & 15) * 8;
        *reinterpret_cast<dbf16x8*>(&s_w1l[rr * DAP + c8]) = *reinterpret_cast<const dbf16x8*>(j.w1_l + rr * DWID + c8);
    }
    df32x16 w1acc[4] = {df32x16{}, df32x16{}, df32x16{}, df32x16{}};
    float w2s[DEF_SMALL_OUT] = {0.0f, 0.0f, 0.0f, 0.0f};
    float w2c[DEF_SMALL_OUT] = {0.0f, 0.0f, 0.0f, 0.0f};
    float4 db2v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    w2_column(j.w2_h, j.w2_l, col, w2c);
    float db1 = 0.0f;
    float4 pa[DN * DWID / 4 / 256];
    float pg[DEF_SMALL_OUT];
    // branch-free (so that an iteration stays one scheduling region): every load is issued at a clamped
    // row and rows past row1 (tiles past the block's last included) are selected to zero
    auto load_tile = [&](int t) __attribute__((always_inline)) {
        const int64_t t0 = row0 + (int64_t)t * DN;
#pragma unroll
        for (int i = 0; i < DN * DWID / 4 / 256; ++i) {
            const int e = tid + 256 * i, rr = e >> 5, c4 = (e & 31) * 4;
            const int64_t g = t0 + rr;
            const float4 v = *reinterpret_cast<const float4*>(ha.A + min(g, row1 - 1) * DWID + c4);
            const bool ok = g < row1;
            pa[i] = make_float4(ok ? v.x : 0.0f, ok ? v.y : 0.0f, ok ? v.z : 0.0f, ok ? v.w : 0.0f);
        }
        const int64_t g = t0 + (tid & (DN - 1));
#pragma unroll
        for (int k = 0; k < DEF_SMALL_OUT; ++k) {
            const float v = j.G[min(g, row1 - 1) * nout + min(k, nout - 1)];
            pg[k] = (tid < DN && k < nout && g < row1) ? v : 0.0f;
        }
    };
    auto store_tile = [&](int b) __attribute__((always_inline)) {
#pragma unroll
        for (int i = 0; i < DN * DWID / 4 / 256; ++i) {
            const int e = tid + 256 * i, rr = e >> 5, c4 = (e & 31) * 4;
            const float f[4] = {pa[i].x, pa[i].y, pa[i].z, pa[i].w};
            bf4 h4, l4;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                __bf16 hi, lo;
                dsplit(f[q], hi, lo);
                h4[q] = hi; l4[q] = lo;
            }
            *reinterpret_cast<bf4*>(&s_ah[b][rr * DAP + c4]) = h4;
            *reinterpret_cast<bf4*>(&s_al[b][rr * DAP + c4]) = l4;
        }
        if (tid < DN) {
            const float4 gv = make_float4(pg[0], pg[1], pg[2], pg[3]);
            s_g4[b][tid] = gv;
            db2v.x += gv.x; db2v.y += gv.y; db2v.z += gv.z; db2v.w += gv.w;
        }
    };
    auto z1 = [&](int b, df32x16 (&z)[2]) __attribute__((always_inline)) {
        z[0] = df32x16{}; z[1] = df32x16{};
#pragma unroll
        for (int ks = 0; ks < DWID / 16; ++ks) {
            const int k0 = 16 * ks + 8 * hh;
            const dbf16x8 wl = *reinterpret_cast<const dbf16x8*>(&s_w1l[col * DAP + k0]);
#pragma unroll
            for (int mt = 0; mt < 2; ++mt) {
                const dbf16x8 ah = *reinterpret_cast<const dbf16x8*>(&s_ah[b][(32 * mt + r) * DAP + k0]);
                const dbf16x8 al = *reinterpret_cast<const dbf16x8*>(&s_al[b][(32 * mt + r) * DAP + k0]);
                z[mt] = DMFMA(ah, w1h[ks], z[mt]);
                z[mt] = DMFMA(ah, wl, z[mt]);
                z[mt] = DMFMA(al, w1h[ks], z[mt]);
            }
        }
    };
    // one element of dz1 (e = 16 mt + q)
    auto dz1_elem = [&](int b, const df32x16 (&z)[2], df32x16 (&d)[2], int mt, int q) __attribute__((always_inline)) {
        const float zz = z[mt][q] + b1c;
        const float zr = fmaxf(zz, 0.0f);
        const float4 gv = s_g4[b][row_of(mt, q, hh)];
        w2s[0] = __builtin_fmaf(gv.x, zr, w2s[0]); w2s[1] = __builtin_fmaf(gv.y, zr, w2s[1]);
        w2s[2] = __builtin_fmaf(gv.z, zr, w2s[2]); w2s[3] = __builtin_fmaf(gv.w, zr, w2s[3]);
        float dv = gv.x * w2c[0];
        dv = __builtin_fmaf(gv.y, w2c[1], dv);
        dv = __builtin_fmaf(gv.z, w2c[2], dv);
        dv = __builtin_fmaf(gv.w, w2c[3], dv);
        dv = zz > 0.0f ? dv : 0.0f;
        db1 += dv;
        d[mt][q] = dv;
    };
    // row chunk i (of 8) of store_tile's A rows, and the G row with chunk 0
    auto store_part = [&](int b, int i) __attribute__((always_inline)) {
        const int e = tid + 256 * i, rr = e >> 5, c4 = (e & 31) * 4;
        const float f[4] = {pa[i].x, pa[i].y, pa[i].z, pa[i].w};
        bf4 h4, l4;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            __bf16 hi, lo;
            dsplit(f[q], hi, lo);
            h4[q] = hi; l4[q] = lo;
        }
        *reinterpret_cast<bf4*>(&s_ah[b][rr * DAP + c4]) = h4;
        *reinterpret_cast<bf4*>(&s_al[b][rr * DAP + c4]) = l4;
        if (i == 0 && tid < DN) {
            const float4 gv = make_float4(pg[0], pg[1], pg[2], pg[3]);
            s_g4[b][tid] = gv;
            db2v.x += gv.x; db2v.y += gv.y; db2v.z += gv.z; db2v.w += gv.w;
        }
    };
    // ---- prologue: tiles 0 and 1 in LDS, tile 2's rows in registers, Z1 of tile 0 --------------------------
    load_tile(0);
    store_tile(0);
    load_tile(1);
    store_tile(1);
    load_tile(2);
    __syncthreads();
    df32x16 zc[2];
    z1(0, zc);
    for (int t = 0; t < T; ++t) {
        // one scheduling region per iteration: past the block's last tiles, Z1 runs on a buffer whose
        // result is dropped and stage B stores zero rows (load_tile's selects), so nothing branches
        const int b0 = t % NB, b1 = (t + 1) % NB, b2 = (t + 2) % NB;
        df32x16 d[2];
        df32x16 zn[2];
        // stage A: Z1(t + 1) on the matrix core, tile t's relu / dZ1 / dW2 on the VALU, interleaved by
        // hand (4 of the 32 per-lane elements after each K step's 6 MFMAs; sched_barrier keeps the chunks)
        zn[0] = df32x16{}; zn[1] = df32x16{};
#pragma unroll
        for (int ks = 0; ks < DWID / 16; ++ks) {
            const int k0 = 16 * ks + 8 * hh;
            const dbf16x8 wl = *reinterpret_cast<const dbf16x8*>(&s_w1l[col * DAP + k0]);
#pragma unroll
            for (int mt = 0; mt < 2; ++mt) {
                const dbf16x8 ah = *reinterpret_cast<const dbf16x8*>(&s_ah[b1][(32 * mt + r) * DAP + k0]);
                const dbf16x8 al = *reinterpret_cast<const dbf16x8*>(&s_al[b1][(32 * mt + r) * DAP + k0]);
                zn[mt] = DMFMA(ah, w1h[ks], zn[mt]);
                zn[mt] = DMFMA(ah, wl, zn[mt]);
                zn[mt] = DMFMA(al, w1h[ks], zn[mt]);
            }
#pragma unroll
            for (int e = 4 * ks; e < 4 * ks + 4; ++e) dz1_elem(b0, zc, d, e >> 4, e & 15);
            __builtin_amdgcn_sched_barrier(0);
        }
        // stage B: dW1(t) on the matrix core, tile t + 2's rows into LDS on the VALU (2 row chunks per K step)
#pragma unroll
        for (int ks = 0; ks < DN / 16; ++ks) {
            dbf16x8 dh, dl;
            wg_regs_to_op(d[ks >> 1], ks & 1, dh, dl);
#pragma unroll
            for (int nt = 0; nt < 4; ++nt) {
                const dbf16x8 bh = wg_lds_op(s_ah[b0], DAP, ks, 32 * nt), bl = wg_lds_op(s_al[b0], DAP, ks, 32 * nt);
                w1acc[nt] = DMFMA(dh, bh, w1acc[nt]);
                w1acc[nt] = DMFMA(dh, bl, w1acc[nt]);
                w1acc[nt] = DMFMA(dl, bh, w1acc[nt]);
            }
            store_part(b2, 2 * ks);
            store_part(b2, 2 * ks + 1);
            __builtin_amdgcn_sched_barrier(0);
        }
        load_tile(t + 3);
        __syncthreads();
        zc[0] = zn[0]; zc[1] = zn[1];
    }
    // ---- the block's partial products: one atomic per element ------------------------------------------
#pragma unroll
    for (int nt = 0; nt < 4; ++nt)
#pragma unroll
        for (int q = 0; q < 16; ++q) {
            const int m = 32 * wave + (q & 3) + 8 * (q >> 2) + 4 * hh;
            atomicAdd(j.dW1 + (size_t)m * DWID + 32 * nt + r, w1acc[nt][q]);
        }
    db1 += __shfl_xor(db1, 32);
    if (hh == 0) atomicAdd(j.db1 + col, db1);
#pragma unroll
    for (int k = 0; k < DEF_SMALL_OUT; ++k) {
        const float v = w2s[k] + __shfl_xor(w2s[k], 32);
        if (hh == 0 && k < nout) atomicAdd(j.dW2 + (size_t)k * DWID + col, v);
    }
    if (wave == 0) {
        float v[DEF_SMALL_OUT] = {db2v.x, db2v.y, db2v.z, db2v.w};
#pragma unroll
        for (int k = 0; k < DEF_SMALL_OUT; ++k) {
#pragma unroll
            for (int off = 32; off >= 1; off >>= 1) v[k] += __shfl_xor(v[k], off);
            if (lane == 0 && k < nout) atomicAdd(j.db2 + k, v[k]);
        }
    }
}

void launch_head_wgrad(const HeadWgradArgs& a, int njobs, hipStream_t st) {
    if (a.P <= 0 || njobs <= 0) return;
    // the small-output heads first (one launch), then the rest: jobs are reordered into two runs
    HeadWgradArgs s = a;
    int ns = 0, nbig = 0;
    for (int i = 0; i < njobs; ++i)
        if (a.job[i].nout <= DEF_SMALL_OUT) s.job[ns++] = a.job[i];
    for (int i = 0; i < njobs; ++i)
        if (a.job[i].nout > DEF_SMALL_OUT) { s.job[ns + nbig] = a.job[i]; ++nbig; }
    // one round of 256 CUs per launch: 64 blocks per small head, 256 for a wide head (2M backward
    // 9.34 ms with the small heads unpipelined -> 9.13-9.15 ms)
    if (ns) {
        const int nb = ns <= 4 ? 256 / ns / 8 * 8 : 32;
        s.rows_per_block = std::max(64, ((a.P + nb - 1) / nb + 63) / 64 * 64);
        hipLaunchKernelGGL(k_head_wgrad3, dim3((a.P + s.rows_per_block - 1) / s.rows_per_block, ns), dim3(256), 0, st,
                           s, 0);
    }
    if (nbig) {
        const int nb = std::max(8, 256 / nbig / 8 * 8);
        s.rows_per_block = std::max(64, ((a.P + nb - 1) / nb + 63) / 64 * 64);
        hipLaunchKernelGGL(k_head_wgrad2, dim3((a.P + s.rows_per_block - 1) / s.rows_per_block, nbig), dim3(256), 0,
                           st, s, ns);
    }
}

// Phase B: C[M][N] += sum_g L[g][m] R[g][n] (M, N <= 128), bias[m] += sum_g L[g][m]; split-K over
// blocks of rows_per_block rows (blockIdx.x), one job per blockIdx.y.  The reduction index g is the
// MFMA's K, so both fragments come straight from the row-major operands: lane (r, h) loads
// L[g0 + 8h + j][32 mt + r] for j < 8 (each load instruction reads 2 x 128 contiguous bytes) and
// splits it into bf16 hi / lo in registers; no LDS.  A wave owns a strip of 32x32 output tiles (one
// M tile and every N tile when M = 128, else one N tile and every M tile), accumulates it over the
// block's rows and adds it to C with one atomic per element.
__device__ __forceinline__ void atb_frag(const float* __restrict__ src, int ld, int col, int64_t g, int64_t row1,
                                         dbf16x8& h8, dbf16x8& l8, float& sum) {
    float v[8];
#pragma unroll
    for (int jj = 0; jj < 8; ++jj) v[jj] = (g + jj < row1 && col < ld) ? src[(g + jj) * ld + col] : 0.0f;
#pragma unroll
    for (int jj = 0; jj < 8; ++jj) {
        __bf16 hi, lo;
        dsplit(v[jj], hi, lo);
        h8[jj] = hi;
        l8[jj] = lo;
        sum += v[jj];
    }
}

template <bool STRIP_M>   // STRIP_M: wave w owns M tile w and all N tiles (M = 128)
__device__ __forceinline__ void atb_body(const AtbJob& j, int64_t row0, int64_t row1) {
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, r = lane & 31, hh = lane >> 5;
    const int M = j.M, N = j.N, Mt = (M + 31) / 32, Nt = (N + 31) / 32;
    const int ntile = STRIP_M ? Nt : (wave < Nt ? Mt : 0);
    if (ntile == 0) return;
    df32x16 acc[4] = {df32x16{}, df32x16{}, df32x16{}, df32x16{}};
    float bsum = 0.0f, dummy = 0.0f;
    for (int64_t k0 = row0; k0 < row1; k0 += 16) {
        const int64_t g = k0 + 8 * hh;
        dbf16x8 ah[4], al[4], bh[4], bl[4];
        if (STRIP_M) {
            atb_frag(j.L, M, 32 * wave + r, g, row1, ah[0], al[0], bsum);
#pragma unroll
            for (int t = 0; t < 4; ++t)
                if (t < ntile) atb_frag(j.R, N, 32 * t + r, g, row1, bh[t], bl[t], dummy);
        } else {
#pragma unroll
            for (int t = 0; t < 4; ++t)
                if (t < ntile) atb_frag(j.L, M, 32 * t + r, g, row1, ah[t], al[t], t == wave ? bsum : dummy);
            atb_frag(j.R, N, 32 * wave + r, g, row1, bh[0], bl[0], dummy);
        }
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            if (t >= ntile) break;
            const dbf16x8& xh = STRIP_M ? ah[0] : ah[t];
            const dbf16x8& xl = STRIP_M ? al[0] : al[t];
            const dbf16x8& yh = STRIP_M ? bh[t] : bh[0];
            const dbf16x8& yl = STRIP_M ? bl[t] : bl[0];
            acc[t] = DMFMA(xh, yh, acc[t]);
            acc[t] = DMFMA(xh, yl, acc[t]);
            acc[t] = DMFMA(xl, yh, acc[t]);
        }
    }
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        if (t >= ntile) break;
        const int mt = STRIP_M ? wave : t, nt = STRIP_M ? t : wave;
        const int n = 32 * nt + r;
#pragma unroll
        for (int q = 0; q < 16; ++q) {
            const int m = 32 * mt + (q & 3) + 8 * (q >> 2) + 4 * hh;
            if (m < M && n < N) atomicAdd(j.C + (size_t)m * N + n, acc[t][q]);
        }
    }
    // bias: lanes r and r + 32 hold the two row halves of column 32 mt + r (mt = this wave's M tile)
    if (j.bias) {
        const float tot = bsum + __shfl_xor(bsum, 32);
        const int m = 32 * wave + r;
        if (hh == 0 && m < M && (STRIP_M || wave < Mt)) atomicAdd(j.bias + m, tot);
    }
    (void)dummy;
}

__global__ void __launch_bounds__(256) k_atb(AtbArgs ga) {
    const AtbJob& j = ga.job[blockIdx.y];
    const int64_t row0 = (int64_t)blockIdx.x * ga.rows_per_block;
    const int64_t row1 = min((int64_t)ga.P, row0 + ga.rows_per_block);
    if (row0 >= row1) return;
    if (j.M > 96) atb_body<true>(j, row0, row1);
    else atb_body<false>(j, row0, row1);
}

void launch_atb(const AtbArgs& a, int njobs, hipStream_t st) {
    if (a.P <= 0 || njobs <= 0) return;
    const int nb = (a.P + a.rows_per_block - 1) / a.rows_per_block;
    hipLaunchKernelGGL(k_atb, dim3(nb, njobs), dim3(256), 0, st, a);
}

}  // namespace lsr
