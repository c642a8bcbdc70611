// deform_internal.h -- kernel argument blocks and launchers of the deformation field (include/lsr_deform.h):
// what its units (deform*.hip), deform_api.hip and centers.hip share.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace lsr {

// deformation field forward (deform.hip)
constexpr int DEF_MAX_LAYERS = 4;     // feature_out Linear layers
constexpr int DEF_HEADS = 6;          // pos, scales, rotations, opacity, shs, coff
constexpr int DEF_W2ROWS = 64;        // output rows of every head's last layer, zero padded
constexpr int DEF_LANG_MODE_PASS = 0, DEF_LANG_MODE_RESIDUAL = 1, DEF_LANG_MODE_NORESNET = 2,
              DEF_LANG_MODE_DISCRETE = 3;
struct DeformArgs {
    int P;
    int n_scales, nlayers;
    uint32_t heads;                   // bit h: head h computed
    int apply_rotation, lang_mode, lang_dim, centers, lang_in;   // lang_in: input lang channels
    const float* means3D;
    const float* time;
    const float* aabb;                // [2][3] device: xyz_max, xyz_min
    const float* planes;              // packed channel-last planes
    int64_t poff[24];                 // float offset of plane 6 s + ci
    int pw[24], ph[24];               // its width / height
    const __bf16 *wf_h[DEF_MAX_LAYERS], *wf_l[DEF_MAX_LAYERS];   // layer k: [128][K_k], K_0 = 16 n_scales
    const __bf16 *w1_h[DEF_HEADS], *w1_l[DEF_HEADS];             // [128][128]
    const __bf16 *w2_h[DEF_HEADS], *w2_l[DEF_HEADS];             // [DEF_W2ROWS][128]
    const float* b_feat[DEF_MAX_LAYERS];
    const float* b1[DEF_HEADS];
    const float* b2[DEF_HEADS];
    const float* in[5];               // means3D, scales, rotations, opacity, shs
    const float* lang;                // [P, lang_in]
    float* out[5];
    float* out_lang;                  // DISCRETE: [P, lang_dim]
    float* out_coff;                  // DISCRETE: [P, centers] or null
};
void launch_deform_fwd(const DeformArgs& a, hipStream_t st);
// lsr_deform_prepare's packing jobs in one launch per PACK_MAX_JOBS (deform_pack.hip k_pack_batch)
enum PackKind { PACK_PLANE = 0, PACK_WEIGHT = 1, PACK_WEIGHT_T = 2 };
struct PackJob {
    int kind, a, b, c, d;             // PLANE: a = H * W; WEIGHT: rows, rows_pad, cols, cols_pad; T: rows, cols, k_pad, cols_pad
    uint32_t first_block;             // set by launch_pack_batch
    const float* src;
    void* hi;                         // PLANE: the float destination
    __bf16* lo;
};
constexpr int PACK_MAX_JOBS = 64;
struct PackBatch { PackJob j[PACK_MAX_JOBS]; int n; };
void launch_pack_batch(PackJob* jobs, int n, hipStream_t st);

// deformation backward (deform.hip): phase A per 64 Gaussians (recompute, data gradients, plane
// scatter, saved activations), phase B the weight gradients as split-K A^T B products (deform_wgrad.hip)
struct DeformBwdArgs {
    DeformArgs f;                     // planes, packed weights, biases, means3D, time, aabb, lang, in[2]
    const __bf16 *wft_h[DEF_MAX_LAYERS], *wft_l[DEF_MAX_LAYERS];   // layer k transposed: [K_k pad 32][128]
    const __bf16 *w1t_h[DEF_HEADS], *w1t_l[DEF_HEADS];             // [128 in][128 out]
    const __bf16 *w2t_h[DEF_HEADS], *w2t_l[DEF_HEADS];             // [128 in][64 out, zero padded]
    const float* up[5];               // gradients of the five outputs (null: head off)
    const float* up_lang;             // DISCRETE: [P, lang_dim] or null
    const float* up_coff;             // DISCRETE: [P, centers] or null
    float* d_means3D;
    float* d_rotations;               // apply_rotation: [P, 4]
    float* d_lang;                    // DISCRETE: [P, lang_in]
    float* dplanes;                   // packed channel-last gradient planes (same offsets as f.planes),
    int64_t plane_stride;             //   `replicas` copies plane_stride floats apart (block b adds
    int replicas;                     //   into copy b % replicas; the unpack sums them)
    // time planes (xt, yt, zt) of waves whose Gaussians all have time[0] (the render path's one time
    // per view): every tap lies in the rows y0, y1 of time[0] with weights 1 - fy, fy, so the wave adds
    // dv (1 - fx), dv fx into one x-row [W][16] per plane (at trow + toff[pi], copy b % trow_reps),
    // and the unpack adds (1 - fy) and fy times its sum into the two rows.  Null: off.
    float* trow;
    int64_t toff[24];
    int64_t trow_stride;
    int trow_reps;
    float* sX;                        // saved [P, 16 n_scales] features
    float* sA[DEF_MAX_LAYERS];        // saved [P,128] relu(H_k)
    float* sdH[DEF_MAX_LAYERS];       // saved [P,128] gradients of H_k
    float* sG_rot;                    // apply_rotation: [P,4] gradient of the rotation head's output
    float* sG_coff;                   // DISCRETE: [P, centers] gradient of coff
    float* daabb;                     // [2][3] gradient of the HexPlane box (accumulated), or null;
                                      //   phase A adds into DEF_AABB_SLOTS partial rows of daabb_part
                                      //   (block b: row b % slots, 64 B apart), the unpack sums them
    float* daabb_part;
};
constexpr int DEF_AABB_SLOTS = 64;
void launch_deform_bwd_a(const DeformBwdArgs& a, hipStream_t st);
// Weight gradients of the computed heads by recompute (deform_wgrad.hip: k_head_wgrad3 for the heads of
// at most 4 outputs, k_head_wgrad2 for the wide SH head): per head and block of rows, from the saved
// last trunk activation A and the head's output gradient G, Z1 = A W1^T + b1, dZ1 = (G W2) [Z1 > 0];
// dW1 += dZ1^T A, db1 += sum dZ1, dW2 += G^T relu(Z1), db2 += sum G.  One launch per kernel (grid
// row = job).
struct HeadWgradJob {
    const float* G;                   // [P][nout]
    const __bf16 *w1_h, *w1_l;        // forward pack [128][128]
    const float* b1;
    const __bf16 *w2t_h, *w2t_l;      // backward pack [128][64] (W2 transposed, K padded to 64)
    const __bf16 *w2_h, *w2_l;        // forward pack [64 pad][128] (the VALU path of nout <= 4)
    float *dW1, *db1, *dW2, *db2;     // accumulated
    int nout;
};
constexpr int DEF_WGRAD_MAX_JOBS = DEF_HEADS;
struct HeadWgradArgs {
    HeadWgradJob job[DEF_WGRAD_MAX_JOBS];
    const float* A;                   // [P][128] the trunk's last activation (phase A saved it)
    int P, rows_per_block;            // rows_per_block: set per launch by launch_head_wgrad
};
void launch_head_wgrad(const HeadWgradArgs& a, int njobs, hipStream_t st);
struct AtbJob {                        // C[M][N] += sum_g L[g][m] R[g][n]; bias[m] += sum_g L[g][m]
    const float* L;
    const float* R;
    float* C;
    float* bias;
    int M, N;
};
constexpr int LSR_ATB_MAX_JOBS = 20;
struct AtbArgs {
    AtbJob job[LSR_ATB_MAX_JOBS];
    int P;
    int rows_per_block;
};
void launch_atb(const AtbArgs& a, int njobs, hipStream_t st);
// Every gradient plane of a call in one launch: plane j's packed replicas at src + off[j] (floats)
// summed and added into dst[j] ([channels][H][W]); with daabb set, the last block also adds the
// DEF_AABB_SLOTS partial rows of daabb_part into daabb.
constexpr int DEF_UNPACK_MAX = 24;   // 6 planes x LSR_DEFORM_MAX_SCALES
struct UnpackBatch {
    const float* src;
    int64_t off[DEF_UNPACK_MAX];
    float* dst[DEF_UNPACK_MAX];
    int H[DEF_UNPACK_MAX], W[DEF_UNPACK_MAX];
    int block0[DEF_UNPACK_MAX + 1];   // first block of plane j; block0[n] = the planes' blocks
    int n, replicas;
    int64_t stride;
    const float* daabb_part;
    float* daabb;
    // DeformBwdArgs.trow: plane j's x-row copies at trow + toff[j] (toff[j] < 0: none), folded into
    // its rows of time time0[0]
    const float* trow;
    int64_t toff[DEF_UNPACK_MAX];
    int64_t trow_stride;
    int trow_reps;
    const float* time0;
};
void launch_unpack_planes(const UnpackBatch& u, int channels, hipStream_t st);   // 16 or 32 (deform_pack.hip)

// lang_deform (deform_lang.hip; RESIDUAL / NORESNET): relu([lang, poc_fre(t)]) -> Linear, ReLU, Linear, ReLU,
// Linear, (+ lang), normalised.  Separate kernels: the MLP reads only the language rows and the time.
struct LangDeformArgs {
    int P, lang_dim, time_pe, kin, residual;   // kin = lang_dim + 1 + 2 time_pe
    const float* lang;                // [P, lang_dim]
    const float* time;
    const __bf16 *w_h[3], *w_l[3];    // [128][kpad], [128][128], [32][128] (rows past lang_dim zero)
    const float* b[3];
    float* out_lang;
    // backward only
    const __bf16 *wt_h[3], *wt_l[3];  // transposed: [kpad 32][128], [128][128], [128][32]
    const float* up_lang;             // [P, lang_dim] or null
    float* d_lang;                    // [P, lang_dim]
    float *sU0, *sU1, *sU2;           // saved [P, kin], [P,128], [P,128]
    float *sdv, *sdZ2, *sdZ1;         // saved [P, lang_dim], [P,128], [P,128]
};
void launch_lang_deform_fwd(const LangDeformArgs& a, hipStream_t st);
void launch_lang_deform_bwd(const LangDeformArgs& a, hipStream_t st);

// The status centres (include/lsr_centers.h), fused: a block takes `gpb` Gaussians, runs lang_deform
// on their gpb * S (language, time) rows in tiles of 64 and the k-means of each Gaussian's S rows
// (centers_kmeans.h) on the samples in LDS.  f.lang is the raw language [P, lang_dim]; f.time and
// f.out_lang are unused.
struct CentersArgs {
    LangDeformArgs f;
    const float* times;               // [P, S] or null: the generator of (seed, g, s)
    uint32_t seed;
    int S, K, max_iter, gpb;
    float* centers;                   // [P, K, lang_dim]
    int32_t* counts;                  // [P, K]
    float* inertia;                   // [P]
    int32_t* iters;                   // [P]
    float *samples_out, *times_out;   // [P, S, lang_dim], [P, S] or null
};
void launch_centers_from_field(const CentersArgs& a, hipStream_t st);

}  // namespace lsr
