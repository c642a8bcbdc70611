// lsr_api.hip -- the C ABI (include/lsr.h): argument checks, workspace carving, launch order.
//
// Forward  = preprocess -> depth sort of the P Gaussians -> tile counts in depth order -> scan
//            -> (host reads K) -> emit K instances -> stable tile sort -> tile ranges -> composite.
// Backward = composite backward (per-Gaussian screen-space sums) -> preprocess backward.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstring>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/lsr.h"
#include "lsr_common.h"
#include "lsr_host.h"
#include "lsr_internal.h"

namespace {
thread_local std::string g_err;   // lsr_last_error
}

// the library's one error path (lsr_host.h): every unit reports through it
int lsr::fail(int code, const std::string& msg) {
    g_err = msg;
    return code;
}

namespace {

using lsr::Carver;
using lsr::fail;

// lsr_require_api: the lsr.h version the caller was built against
lsr::ApiGate g_api{"lsr", "LSR_API_VERSION", LSR_API_VERSION, "lsr.h version " + std::to_string(LSR_API_VERSION)};

#define LSR_HIP(expr)                                                  \
    do {                                                               \
        if (int rc_ = lsr::launched(#expr, (expr))) return rc_;        \
    } while (0)

// after a launch; debug: wait for the kernels too, so that a fault is reported by the phase that caused it
#define LSR_LAUNCHED(name, st, debug)                                   \
    do {                                                                \
        hipError_t e_ = hipGetLastError();                              \
        if (e_ == hipSuccess && (debug)) e_ = hipStreamSynchronize(st); \
        if (int rc_ = lsr::launched(name, e_)) return rc_;              \
    } while (0)

// ---- per-phase event timing (lsr_profile_*) ----------------------------------------------------
struct Profiler {
    std::mutex mu;
    bool on = false;
    uint32_t mask = ~0u;   // phases timed while on (bit LSR_PHASE_*)
    std::vector<hipEvent_t> pool;
    struct Rec { int phase; hipEvent_t a, b; };
    std::vector<Rec> pending;
    double ms[LSR_NUM_PHASES] = {};
    int64_t n[LSR_NUM_PHASES] = {};
    hipEvent_t get() {
        if (!pool.empty()) { hipEvent_t e = pool.back(); pool.pop_back(); return e; }
        hipEvent_t e = nullptr;
        if (hipEventCreate(&e) != hipSuccess) return nullptr;
        return e;
    }
};
Profiler g_prof;

struct PhaseTimer {
    int phase;
    hipStream_t st;
    hipEvent_t a = nullptr, b = nullptr;
    PhaseTimer(int p, hipStream_t s) : phase(p), st(s) {
        std::lock_guard<std::mutex> l(g_prof.mu);
        if (!g_prof.on || !((g_prof.mask >> p) & 1u)) return;
        a = g_prof.get();
        b = g_prof.get();
        if (a) (void)hipEventRecord(a, st);
    }
    ~PhaseTimer() {
        if (!a || !b) return;
        (void)hipEventRecord(b, st);
        std::lock_guard<std::mutex> l(g_prof.mu);
        g_prof.pending.push_back({phase, a, b});
    }
};

struct Geom {
    float2* xy;
    float4* conic_o;
    float4* rgbd;
    uint8_t* clamped;
    uint32_t* tiles;
    uint32_t *key_a, *key_b, *val_a, *val_b;
    uint32_t* counts;
    uint32_t* offsets;
    uint32_t* inst_off;
    int* radius;
    uint2* rect;          // by id, written by preprocess
    uint2* rect_sorted;   // depth order
    uint32_t* total;
    void* sort_tmp;
    void* scan_tmp;
    float4* acc;          // [P, ACC_PITCH] split-backward accumulators (rows of listed Gaussians
                          // zeroed by the preprocess; lsr_backward_composite adds into them)
};
Geom carve_geom(void* base, size_t P, size_t* bytes) {
    Carver c(base);
    Geom g;
    g.xy = c.take<float2>(P);
    g.conic_o = c.take<float4>(P);
    g.rgbd = c.take<float4>(P);
    g.clamped = c.take<uint8_t>(P);
    g.tiles = c.take<uint32_t>(P);
    g.key_a = c.take<uint32_t>(P);
    g.key_b = c.take<uint32_t>(P);
    g.val_a = c.take<uint32_t>(P);
    g.val_b = c.take<uint32_t>(P);
    g.counts = c.take<uint32_t>(P);
    g.offsets = c.take<uint32_t>(P);
    g.inst_off = c.take<uint32_t>(P);
    g.radius = c.take<int>(P);
    g.rect = c.take<uint2>(P);
    g.rect_sorted = c.take<uint2>(P);
    g.total = c.take<uint32_t>(4);
    g.sort_tmp = c.take<char>(lsr::radix_temp_bytes(P));
    g.scan_tmp = c.take<char>(lsr::scan_temp_bytes(P));
    g.acc = c.take<float4>(P * (lsr::ACC_PITCH / 4));
    if (bytes) *bytes = c.total();
    return g;
}

struct Binning {
    uint32_t *key_a, *key_b, *val_a, *val_b;
    void* sort_tmp;
    uint32_t* kept;   // the tile sort's listed-instance count (its first pass drops the unlisted)
};
Binning carve_binning(void* base, size_t K, size_t* bytes) {
    Carver c(base);
    Binning b;
    b.key_a = c.take<uint32_t>(K);
    b.key_b = c.take<uint32_t>(K);
    b.val_a = c.take<uint32_t>(K);
    b.val_b = c.take<uint32_t>(K);
    b.sort_tmp = c.take<char>(lsr::radix_temp_bytes(K));
    b.kept = c.take<uint32_t>(4);
    if (bytes) *bytes = c.total();
    return b;
}

// the tile-bucket binning's workspace: the sort path's layout (its point list buffer is where the
// compositors read; key_a..key_b hold the 64-bit bucket keys: 8K bytes <= 2 align256(4K)), then the
// per-block tile count table and the long buckets' merge workspace
struct BinningTb {
    Binning b;
    uint32_t* table;
    uint64_t* tmp;
};
BinningTb carve_binning_tb(void* base, size_t K, size_t P, size_t ntiles, size_t* bytes) {
    size_t head;
    BinningTb t;
    t.b = carve_binning(base, K, &head);
    Carver c(base);
    c.off = head;
    t.table = c.take<uint32_t>((size_t)lsr::tb_blocks((int)P) * ntiles);
    t.tmp = c.take<uint64_t>(K);
    if (bytes) *bytes = c.total();
    return t;
}

struct Img {
    uint2* ranges;
    uint32_t* tile_max;
    float* final_T;
    uint32_t* n_contrib;
    uint32_t* tile_order;   // backward scratch: tiles by descending replay length
};
// the tile grid of a W x H image
struct Grid { int x, y; size_t tiles() const { return (size_t)x * y; } };
Grid tile_grid(int W, int H) { return {(W + LSR_TILE_X - 1) / LSR_TILE_X, (H + LSR_TILE_Y - 1) / LSR_TILE_Y}; }
// focal length in pixels of an image axis
float focal(int extent, float tanfov) { return (float)extent / (2.0f * tanfov); }

Img carve_img(void* base, int W, int H, size_t* bytes) {
    const size_t ntiles = tile_grid(W, H).tiles();
    Carver c(base);
    Img m;
    m.ranges = c.take<uint2>(ntiles);
    m.tile_max = c.take<uint32_t>(ntiles);
    m.final_T = c.take<float>((size_t)W * H);
    m.n_contrib = c.take<uint32_t>((size_t)W * H);
    m.tile_order = c.take<uint32_t>(ntiles);
    if (bytes) *bytes = c.total();
    return m;
}

struct Scratch {
    float* acc_small;    // [P,12] atomic mode accumulators (zeroed per call)
    float* rec;          // [K, record_floats(C)] deterministic mode records
    uint8_t* flags;      // [K] record written
};
Scratch carve_scratch(void* base, size_t P, size_t K, int recq, bool det, size_t* bytes) {
    Carver c(base);
    Scratch s{};
    if (det) {
        s.rec = c.take<float>(K * (size_t)recq);
        s.flags = c.take<uint8_t>(K);
    } else {
        s.acc_small = c.take<float>(P * lsr::ACC_PITCH);
    }
    if (bytes) *bytes = c.total();
    return s;
}

// tile-sort key bits: keys are tile ids 0..ntiles-1 plus ntiles for instances whose splat
// reaches no quadrant of their tile (binning.hip k_emit): they sort past every tile's list
int tile_bits(int ntiles) {
    int b = 1;
    while ((1 << b) <= ntiles) ++b;
    return b;
}
bool tile_sort_in_b(int ntiles) { return ((tile_bits(ntiles) + 7) / 8) % 2 == 1; }
// the binning's sorted point list: where the compositors read
uint32_t* point_list(const Binning& b, Grid grid) { return tile_sort_in_b((int)grid.tiles()) ? b.val_b : b.val_a; }
int depth_sort_result_in_b() { return 0; }  // 4 passes, or 3 planned on the device: either way in the (a) buffers

int check_common(const lsr_settings* s, const lsr_fwd_in* in) {
    if (int rc = g_api.check()) return rc;   // the structs' layout is that of this lsr.h only
    if (!s || !in) return fail(LSR_EINVAL, "null settings or inputs");
    if (s->image_width <= 0 || s->image_height <= 0) return fail(LSR_EINVAL, "image size must be positive");
    if (s->image_width > 4095 * LSR_TILE_X || s->image_height > 4095 * LSR_TILE_Y)
        return fail(LSR_EINVAL, "image size exceeds 4095 tiles per axis");
    if (in->P < 0) return fail(LSR_EINVAL, "P must be >= 0");
    // point lists carry 28-bit Gaussian ids (the top 4 bits: the tile's quadrants the splat may
    // reach) and the compositors address rows with 32-bit byte offsets
    if (in->P >= (1 << 28)) return fail(LSR_EINVAL, "P must be < 2^28");
    if ((uint64_t)in->P * (uint64_t)(in->C > 16 ? in->C : 16) * 4u >= (1ull << 32))
        return fail(LSR_EINVAL, "P * max(C, 16) * 4 bytes must be < 2^32");
    if (!s->viewmatrix || !s->projmatrix || !s->bg || !s->campos)
        return fail(LSR_EINVAL, "viewmatrix, projmatrix, bg and campos are required");
    if (in->P > 0 && (!in->means3D || !in->opacities)) return fail(LSR_EINVAL, "means3D and opacities are required");
    if (in->P == 0) return LSR_OK;   // nothing to validate or render (upstream returns early too)
    if ((in->shs == nullptr) == (in->colors_precomp == nullptr))
        return fail(LSR_EINVAL, "Please provide excatly one of either SHs or precomputed colors!");
    const bool sr = in->scales != nullptr || in->rotations != nullptr;
    if ((!(in->scales && in->rotations) && !in->cov3D_precomp) || (sr && in->cov3D_precomp))
        return fail(LSR_EINVAL, "Please provide exactly one of either scale/rotation pair or precomputed 3D covariance!");
    if (in->shs && (s->sh_degree < 0 || s->sh_degree > 3 || in->M < (s->sh_degree + 1) * (s->sh_degree + 1)))
        return fail(LSR_EINVAL, "sh_degree must be in [0, 3] and shs must hold (sh_degree + 1)^2 coefficients");
    if (in->C < 0 || in->C > 64) return fail(LSR_EINVAL, "language feature channels must be in [0, 64]");
    if (s->include_feature && in->C > 0 && in->P > 0 && !in->language_feature)
        return fail(LSR_EINVAL, "language_feature is required when C > 0");
    return LSR_OK;
}

// ---- validation of a batch of views -------------------------------------------------------------
// What a batched entry point says when n_views < 1 and when a per-view array is null, and the
// settings its views must share with view 0 (share_first: compared before the entry point's own
// per-view requirements, the binnings' order; otherwise after them).
enum : unsigned { SHARE_SIZE = 1, SHARE_SH_DEGREE = 2, SHARE_SCALE = 4, SHARE_FEATURE = 8 };
struct ViewRules { const char *no_views, *null_array; unsigned share; const char* share_msg; bool share_first; };
const char kArrays[] = "n_views >= 1 and the per-view arrays are required";
const ViewRules kPreprocessViews{kArrays, kArrays, SHARE_SIZE | SHARE_SH_DEGREE | SHARE_SCALE,
                                 "batched views must share the image size, sh_degree and scale_modifier", false};
const ViewRules kBinningViews{kArrays, kArrays, SHARE_SIZE, "batched views must share the image size", true};
const ViewRules kCompositeViews{kArrays, kArrays, SHARE_SIZE | SHARE_FEATURE,
                                "batched views must share the image size and include_feature", false};
const ViewRules kBackwardViews{"n_views must be >= 1", "null argument", SHARE_SCALE,
                               "all views must share scale_modifier", false};

bool shares(const lsr_settings* a, const lsr_settings* b, unsigned what) {
    return (!(what & SHARE_SIZE) || (a->image_width == b->image_width && a->image_height == b->image_height)) &&
           (!(what & SHARE_SH_DEGREE) || a->sh_degree == b->sh_degree) &&
           (!(what & SHARE_SCALE) || a->scale_modifier == b->scale_modifier) &&
           (!(what & SHARE_FEATURE) || (a->include_feature != 0) == (b->include_feature != 0));
}

// Every view is validated before anything is launched: n_views and the per-view arrays (arrays:
// all non-null), then for each view check_common, the rules' shared settings and what the entry
// point itself requires of the view (need(v): LSR_OK or a fail()).
template <typename Need>
int check_each_view(const ViewRules& rules, int32_t n_views, bool arrays, const lsr_settings* const* s,
                    const lsr_fwd_in* in, Need need) {
    if (n_views < 1) return fail(LSR_EINVAL, rules.no_views);
    if (!arrays) return fail(LSR_EINVAL, rules.null_array);
    for (int v = 0; v < n_views; ++v) {
        int rc = check_common(s[v], in);
        if (rc) return rc;
        if (rules.share_first && !shares(s[v], s[0], rules.share)) return fail(LSR_EINVAL, rules.share_msg);
        if ((rc = need(v))) return rc;
        if (!rules.share_first && !shares(s[v], s[0], rules.share)) return fail(LSR_EINVAL, rules.share_msg);
    }
    return LSR_OK;
}
int need_radii(int32_t n_views, lsr_fwd_out* const* out, int P) {
    for (int v = 0; v < n_views; ++v)
        if (!out[v] || (!out[v]->radii && P > 0)) return fail(LSR_EINVAL, "radii output is required");
    return LSR_OK;
}
// a rendered view's workspaces (no binning workspace when nothing was listed)
int need_workspaces(const void* geom, const void* img, const void* binning, int64_t num_rendered) {
    if (!geom || !img || (num_rendered > 0 && !binning)) return fail(LSR_EINVAL, "workspaces are required");
    return LSR_OK;
}
// a view's upstream gradients, for the float-atomic reductions
int need_atomic_grads(const lsr_bwd_in* gin, const char* color_msg, const char* deterministic_msg) {
    if (!gin || !gin->dL_dout_color) return fail(LSR_EINVAL, color_msg);
    if (gin->deterministic) return fail(LSR_EINVAL, deterministic_msg);
    return LSR_OK;
}

// The Gaussians' side of a preprocess launch (shared by its views).
void preprocess_shared(lsr::PreprocessArgs& a, const lsr_settings* s, const lsr_fwd_in* in) {
    const int W = s->image_width, H = s->image_height;
    const Grid grid = tile_grid(W, H);
    a.P = in->P; a.M = in->M; a.deg = s->sh_degree; a.W = W; a.H = H;
    a.grid_x = grid.x; a.grid_y = grid.y;
    a.scale_modifier = s->scale_modifier;
    a.means3D = in->means3D; a.scales = in->scales; a.rotations = in->rotations; a.opacities = in->opacities;
    a.shs = in->shs; a.colors_precomp = in->colors_precomp; a.cov3D_precomp = in->cov3D_precomp;
}
// One view's camera and outputs.  The preprocess also writes the depth sort's initial values
// (ids), zeroes the split-backward accumulator rows of listed Gaussians, and clears the counters
// [0] K, [1..2] reserved (reported as 0), [3] visible count: no separate fill launches.
void preprocess_view(lsr::PreprocessView& v, const lsr_settings* s, const Geom& g, int* radii) {
    v.tanfovx = s->tanfovx; v.tanfovy = s->tanfovy;
    v.focal_x = focal(s->image_width, s->tanfovx);
    v.focal_y = focal(s->image_height, s->tanfovy);
    v.view = s->viewmatrix; v.proj = s->projmatrix; v.campos = s->campos;
    v.radii = radii; v.radius = g.radius; v.tiles = g.tiles; v.rect = g.rect; v.key = g.key_a; v.xy = g.xy;
    v.conic_o = g.conic_o; v.rgbd = g.rgbd; v.clamped = g.clamped;
    v.order = g.val_a;
    v.rank_counts = g.counts;
    v.acc = g.acc;
    v.clear.p[0] = g.total;
    v.clear.n[0] = 4;
}

// The device alias of page-locked host_counts (the instance scan then writes the counts itself), or
// null: pageable memory, the counts are copied.
uint32_t* mapped_counts(uint32_t* host_counts) {
    void* dptr = nullptr;
    if (hipHostGetDevicePointer(&dptr, host_counts, 0) == hipSuccess && dptr) return static_cast<uint32_t*>(dptr);
    (void)hipGetLastError();   // clear the sticky error of the failed query
    return nullptr;
}

// Instance scan of nv <= 8 views (their geom workspaces: the exclusive scan of g.counts into
// g.offsets, the total K into g.total[0]) and the delivery of each view's [K, reserved = 0] to
// host_counts: with `mapped`, host_counts' device alias, the scan writes K straight to the caller's
// pinned word (the preprocess zeroed a view's reserved word only on the device: the host clears it
// here); the views it did not write (one-tile scans; mapped == null) get a copy of g.total[0..1].
int scan_counts(int nv, void* const* geom, int P, uint32_t* host_counts, uint32_t* mapped, hipStream_t st, bool debug) {
    lsr::ScanSeg sc[lsr::LSR_MAX_VIEWS] = {};
    const uint32_t* total[lsr::LSR_MAX_VIEWS];
    for (int k = 0; k < nv; ++k) {
        Geom g = carve_geom(geom[k], (size_t)P, nullptr);
        sc[k] = lsr::ScanSeg{g.counts, g.offsets, g.total, reinterpret_cast<uint32_t*>(g.scan_tmp), (size_t)P};
        total[k] = g.total;
        if (mapped) {
            sc[k].host_total = mapped + 2 * k;
            host_counts[2 * k + 1] = 0;
        }
    }
    uint32_t wrote;
    {
        PhaseTimer t(LSR_PHASE_INSTANCE_SCAN, st);
        wrote = lsr::exclusive_scan_batch(sc, nv, st);
    }
    LSR_LAUNCHED("instance scan", st, debug);
    for (int k = 0; k < nv; ++k)
        if (!((wrote >> k) & 1u))
            LSR_HIP(hipMemcpyAsync(host_counts + 2 * k, total[k], 2 * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    return LSR_OK;
}

// ---- binning: the two algorithms' shared host path ----------------------------------------------
// the batch (view 0's image) and a view with instances to list: its carved geom and img workspaces,
// K and its binning workspace
struct BinBatch { int P, W, H; Grid grid; size_t ntiles; hipStream_t st; bool debug; };
struct BinView { Geom g; Img m; size_t K; void* binning; };
// Validation (max_tiles: the algorithm's limit, refused with too_many_tiles), then per 8 views: a view
// with K == 0 gets empty tile ranges and replay bounds, the others are handed to launch(batch, views,
// count), one call for the set, which enqueues the algorithm's kernels.
template <typename Launch>
int bin_views(int32_t n_views, const lsr_settings* const* s, const lsr_fwd_in* in, void* const* geom,
              void* const* binning, void* const* img, const int64_t* num_rendered, lsr_stream_t stream,
              size_t max_tiles, const char* too_many_tiles, Launch launch) {
    int rc = check_each_view(kBinningViews, n_views, s && geom && binning && img && num_rendered, s, in, [&](int v) {
        return need_workspaces(geom[v], img[v], binning[v], num_rendered[v]);
    });
    if (rc) return rc;
    const Grid grid = tile_grid(s[0]->image_width, s[0]->image_height);
    const BinBatch c{in->P, s[0]->image_width, s[0]->image_height, grid, grid.tiles(),
                     reinterpret_cast<hipStream_t>(stream), s[0]->debug != 0};
    if (c.ntiles > max_tiles) return fail(LSR_EINVAL, too_many_tiles);
    for (int v0 = 0; v0 < n_views; v0 += lsr::LSR_MAX_VIEWS) {
        const int nv = std::min(n_views - v0, lsr::LSR_MAX_VIEWS);
        BinView bv[lsr::LSR_MAX_VIEWS];
        int ne = 0;
        for (int v = v0; v < v0 + nv; ++v) {
            const size_t K = (size_t)num_rendered[v];
            Geom g = carve_geom(geom[v], (size_t)(c.P > 0 ? c.P : 1), nullptr);
            Img m = carve_img(img[v], c.W, c.H, nullptr);
            if (K == 0) {
                LSR_HIP(hipMemsetAsync(m.ranges, 0, sizeof(uint2) * c.ntiles, c.st));
                LSR_HIP(hipMemsetAsync(m.tile_max, 0, sizeof(uint32_t) * c.ntiles, c.st));
                continue;
            }
            bv[ne++] = BinView{g, m, K, binning[v]};
        }
        if (ne == 0) continue;
        if ((rc = launch(c, bv, ne))) return rc;
    }
    return LSR_OK;
}

// What the compositor backward reads of one view: its forward's workspaces, the inputs and the
// upstream gradients.  The caller adds the reduction (mode, records or accumulators, dL/dlanguage).
void render_bwd_view(lsr::RenderBwdArgs& r, const lsr_settings* s, const lsr_fwd_in* in, const lsr_bwd_in* gin,
                     const Geom& g, const Binning& b, const Img& m) {
    const int W = s->image_width, H = s->image_height;
    const Grid grid = tile_grid(W, H);
    r.W = W; r.H = H; r.grid_x = grid.x; r.grid_y = grid.y; r.C = in->C; r.include_feature = s->include_feature;
    r.ranges = m.ranges; r.point_list = point_list(b, grid);
    r.xy = g.xy; r.conic_o = g.conic_o; r.rgbd = g.rgbd;
    r.rect = g.rect; r.inst_off = g.inst_off;
    r.lang = in->language_feature;
    r.lang_split = in->C == 32 ? in->language_feature_split : nullptr;
    r.bg = s->bg; r.final_T = m.final_T; r.n_contrib = m.n_contrib;
    r.tile_max_contrib = m.tile_max; r.tile_order = m.tile_order;
    r.dL_dcolor = gin->dL_dout_color; r.dL_dlang = gin->dL_dout_language_feature; r.dL_ddepth = gin->dL_dout_depth;
}

}  // namespace

// ---- forward phase 1: one host path, for one view as for n ----------------------------------------
// These four helpers stay in an unnamed namespace inside extern "C": the compiler exports such
// names, and the library's exported symbol set does not change here.
extern "C" {
namespace {
// the preprocess family: each view needs its geom workspace
int check_views(int32_t n_views, const lsr_settings* const* s, const lsr_fwd_in* in, void* const* geom) {
    return check_each_view(kPreprocessViews, n_views, s && geom, s, in,
                           [&](int v) { return geom[v] ? LSR_OK : fail(LSR_EINVAL, "geom workspaces are required"); });
}

// preprocess of rows [row0, row1) of n_views validated views, one launch per 8 views; counts_tiles:
// each view's counts array gets the per-Gaussian instance counts by id (the tile-bucket binning's
// input) instead of zeros (the depth sort's last pass fills it by depth rank)
int preprocess_rows(int32_t n_views, int32_t row0, int32_t row1, int counts_tiles, const lsr_settings* const* s,
                    const lsr_fwd_in* in, lsr_fwd_out* const* out, void* const* geom, hipStream_t st) {
    const int P = in->P;
    if (row1 == row0) return LSR_OK;
    for (int v0 = 0; v0 < n_views; v0 += lsr::LSR_MAX_VIEWS) {
        const int nv = std::min(n_views - v0, lsr::LSR_MAX_VIEWS);
        lsr::PreprocessArgs a{};
        preprocess_shared(a, s[v0], in);
        a.nv = nv;
        a.row0 = row0;
        a.P = row1;   // the launch's bound (every per-Gaussian array is indexed by the global row)
        a.counts_tiles = counts_tiles;
        for (int k = 0; k < nv; ++k) {
            Geom g = carve_geom(geom[v0 + k], (size_t)P, nullptr);
            preprocess_view(a.v[k], s[v0 + k], g, out[v0 + k]->radii);
        }
        {
            PhaseTimer t(LSR_PHASE_PREPROCESS, st);
            lsr::launch_preprocess(a, st);
        }
        LSR_LAUNCHED("preprocess", st, s[v0]->debug);
    }
    return LSR_OK;
}

// depth order + instance count of n_views preprocessed views, one set of launches per 8 views
int depth_order_views(int32_t n_views, const lsr_settings* const* s, const lsr_fwd_in* in, void* const* geom,
                      uint32_t* host_counts, uint32_t* mapped, hipStream_t st) {
    const int P = in->P;
    for (int v0 = 0; v0 < n_views; v0 += lsr::LSR_MAX_VIEWS) {
        const int nv = std::min(n_views - v0, lsr::LSR_MAX_VIEWS);
        lsr::SortSeg ss[lsr::LSR_MAX_VIEWS] = {};
        for (int k = 0; k < nv; ++k) {
            Geom g = carve_geom(geom[v0 + k], (size_t)P, nullptr);
            // depth order of the visible Gaussians, stable in id (the first pass drops culled keys,
            // 0xFFFFFFFF, kept count in g.total[3]; the last pass writes the depth-ranked rectangles
            // and instance counts: the ranks of culled Gaussians keep the preprocess's zero counts)
            ss[k] = lsr::SortSeg{g.key_a, g.val_a, g.key_b, g.val_b, g.sort_tmp, g.total + 3,
                                 lsr::SortGather{g.rect, g.counts, g.rect_sorted}, (size_t)P};
            ss[k].vals_c = g.offsets;   // the device-planned passes' scratch (free until the instance scan)
        }
        {
            PhaseTimer t(LSR_PHASE_DEPTH_SORT, st);
            if (lsr::radix_sort_batch(ss, nv, 0, 32, st) != depth_sort_result_in_b())
                return fail(LSR_EHIP, "internal: depth sort batch or parity");
        }
        LSR_LAUNCHED("depth sort", st, s[v0]->debug);
        int rc = scan_counts(nv, geom + v0, P, host_counts + 2 * v0, mapped ? mapped + 2 * v0 : nullptr, st,
                             s[v0]->debug);
        if (rc) return rc;
    }
    return LSR_OK;
}

// the tile-bucket binning's instance count: the exclusive scan of the per-Gaussian counts in id
// order (no depth sort), one launch set per 8 views
int instance_scan_views(int32_t n_views, const lsr_fwd_in* in, void* const* geom, uint32_t* host_counts,
                        uint32_t* mapped, hipStream_t st, bool debug) {
    for (int v0 = 0; v0 < n_views; v0 += lsr::LSR_MAX_VIEWS) {
        int rc = scan_counts(std::min(n_views - v0, lsr::LSR_MAX_VIEWS), geom + v0, in->P, host_counts + 2 * v0,
                             mapped ? mapped + 2 * v0 : nullptr, st, debug);
        if (rc) return rc;
    }
    return LSR_OK;
}
}  // namespace
}  // extern "C"

namespace {
// Phase 1 of n_views validated views: the preprocess of all rows, then the depth order and instance
// count of the first n_ordered.  map_counts: host_counts is page-locked, its counts come through its
// device alias; otherwise it may be pageable and they are copied.
int preprocess_and_order(int32_t n_views, int32_t n_ordered, const lsr_settings* const* s, const lsr_fwd_in* in,
                         lsr_fwd_out* const* out, void* const* geom, uint32_t* host_counts, bool map_counts,
                         hipStream_t st) {
    if (in->P == 0) {
        for (int v = 0; v < 2 * n_ordered; ++v) host_counts[v] = 0;
        return LSR_OK;
    }
    int rc = preprocess_rows(n_views, 0, in->P, 0, s, in, out, geom, st);
    if (rc || n_ordered == 0) return rc;
    return depth_order_views(n_ordered, s, in, geom, host_counts, map_counts ? mapped_counts(host_counts) : nullptr, st);
}

// lsr_forward_preprocess_views_rows_async and its tile-bucket twin
int preprocess_rows_checked(int32_t n_views, int32_t row0, int32_t row1, int counts_tiles, const lsr_settings* const* s,
                            const lsr_fwd_in* in, lsr_fwd_out* const* out, void* const* geom, lsr_stream_t stream) {
    int rc = check_views(n_views, s, in, geom);
    if (rc) return rc;
    if (!out || row0 < 0 || row1 < row0 || row1 > in->P || row0 % 256 != 0)
        return fail(LSR_EINVAL, "0 <= row0 <= row1 <= P with row0 a multiple of 256, and the outputs are required");
    if ((rc = need_radii(n_views, out, in->P))) return rc;
    return preprocess_rows(n_views, row0, row1, counts_tiles, s, in, out, geom, reinterpret_cast<hipStream_t>(stream));
}

// lsr_forward_depth_order_views_async (depth_sort) and lsr_forward_instance_scan_views_async
int count_views(int32_t n_views, const lsr_settings* const* s, const lsr_fwd_in* in, void* const* geom,
                uint32_t* host_counts, lsr_stream_t stream, bool depth_sort) {
    int rc = check_views(n_views, s, in, geom);
    if (rc) return rc;
    if (!host_counts) return fail(LSR_EINVAL, "host_counts is required");
    if (in->P == 0) {
        for (int v = 0; v < 2 * n_views; ++v) host_counts[v] = 0;
        return LSR_OK;
    }
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    uint32_t* mapped = mapped_counts(host_counts);
    return depth_sort ? depth_order_views(n_views, s, in, geom, host_counts, mapped, st)
                      : instance_scan_views(n_views, in, geom, host_counts, mapped, st, s[0]->debug);
}

// The preprocess backward's Gaussian-side inputs and gradient outputs for rows [r0, r0 + n) (gout
// already addresses row r0), for lsr_backward and the batched entry points alike.
lsr::PreprocessBwdViewsArgs preprocess_bwd_args(const lsr_settings* s, const lsr_fwd_in* in, const lsr_bwd_out* gout,
                                                size_t r0, int n, int nv) {
    lsr::PreprocessBwdViewsArgs a{};
    a.P = n; a.M = in->M; a.nv = nv; a.scale_modifier = s->scale_modifier;
    a.means3D = in->means3D + 3 * r0;
    a.scales = in->scales ? in->scales + 3 * r0 : nullptr;
    a.rotations = in->rotations ? in->rotations + 4 * r0 : nullptr;
    a.shs = in->shs ? in->shs + (size_t)in->M * 3 * r0 : nullptr;
    a.cov3D_precomp = in->cov3D_precomp ? in->cov3D_precomp + 6 * r0 : nullptr;
    a.dopacity = gout->dL_dopacity;
    a.dmeans3D = gout->dL_dmeans3D; a.dmeans2D = gout->dL_dmeans2D; a.dcolors = gout->dL_dcolors;
    a.dcov3D = gout->dL_dcov3D; a.dsh = in->shs ? gout->dL_dsh : nullptr; a.dscales = gout->dL_dscales;
    a.drots = gout->dL_drotations;
    return a;
}
// One view's camera, with its geometry rows and summed records from row r0.
void view_cam(lsr::ViewCam& c, const lsr_settings* s, const Geom& g, const float* acc_small, size_t r0) {
    c.view = s->viewmatrix; c.proj = s->projmatrix; c.campos = s->campos;
    c.tanfovx = s->tanfovx; c.tanfovy = s->tanfovy;
    c.focal_x = focal(s->image_width, s->tanfovx);
    c.focal_y = focal(s->image_height, s->tanfovy);
    c.deg = s->sh_degree;
    c.tiles = g.tiles + r0; c.clamped = g.clamped + r0;
    c.acc_small = acc_small + lsr::ACC_PITCH * r0;
}

}  // namespace

extern "C" {

int lsr_version(void) { return LSR_API_VERSION; }
int lsr_require_api(int32_t caller_version) { return g_api.require(caller_version); }
const char* lsr_last_error(void) { return g_err.c_str(); }

int64_t lsr_geom_bytes(int32_t P) {
    size_t b;
    carve_geom(nullptr, (size_t)(P > 0 ? P : 1), &b);
    return (int64_t)b;
}
int64_t lsr_binning_bytes(int64_t K) {
    size_t b;
    carve_binning(nullptr, (size_t)(K > 0 ? K : 1), &b);
    return (int64_t)b;
}
int64_t lsr_binning_bytes_tb(int64_t K, int32_t P, int32_t W, int32_t H) {
    if (W <= 0 || H <= 0 || P < 0) return -1;
    size_t b;
    carve_binning_tb(nullptr, (size_t)(K > 0 ? K : 1), (size_t)(P > 0 ? P : 1), tile_grid(W, H).tiles(), &b);
    return (int64_t)b;
}
int64_t lsr_img_bytes(int32_t W, int32_t H) {
    size_t b;
    carve_img(nullptr, W, H, &b);
    return (int64_t)b;
}
int64_t lsr_backward_bytes(int32_t P, int64_t K, int32_t C, int32_t deterministic) {
    size_t b;
    carve_scratch(nullptr, (size_t)(P > 0 ? P : 1), (size_t)(K > 0 ? K : 1), lsr::record_floats(C > 0 ? C : 0),
                  deterministic != 0, &b);
    return (int64_t)b;
}

int lsr_forward_preprocess_async(const lsr_settings* s, const lsr_fwd_in* in, lsr_fwd_out* out, void* geom,
                                 uint32_t* host_count, lsr_stream_t stream) {
    int rc = check_common(s, in);
    if (rc) return rc;
    if ((rc = need_radii(1, &out, in->P))) return rc;
    if (!geom || !host_count) return fail(LSR_EINVAL, "geom workspace and host_count are required");
    // the one-view batch; host_count may be pageable (lsr_forward_preprocess's is): always copied
    return preprocess_and_order(1, 1, &s, in, &out, &geom, host_count, false, reinterpret_cast<hipStream_t>(stream));
}

int lsr_forward_preprocess_views_split_async(int32_t n_views, int32_t n_ordered, const lsr_settings* const* s,
                                             const lsr_fwd_in* in, lsr_fwd_out* const* out, void* const* geom,
                                             uint32_t* host_counts, lsr_stream_t stream) {
    int rc = check_views(n_views, s, in, geom);
    if (rc) return rc;
    if (!out || (n_ordered > 0 && !host_counts) || n_ordered < 0 || n_ordered > n_views)
        return fail(LSR_EINVAL, "0 <= n_ordered <= n_views, the outputs and host_counts are required");
    if ((rc = need_radii(n_views, out, in->P))) return rc;
    return preprocess_and_order(n_views, n_ordered, s, in, out, geom, host_counts, true,
                                reinterpret_cast<hipStream_t>(stream));
}

int lsr_forward_preprocess_views_rows_async(int32_t n_views, int32_t row0, int32_t row1, const lsr_settings* const* s,
                                            const lsr_fwd_in* in, lsr_fwd_out* const* out, void* const* geom,
                                            lsr_stream_t stream) {
    return preprocess_rows_checked(n_views, row0, row1, 0, s, in, out, geom, stream);
}

int lsr_forward_preprocess_views_tb_async(int32_t n_views, int32_t row0, int32_t row1, const lsr_settings* const* s,
                                          const lsr_fwd_in* in, lsr_fwd_out* const* out, void* const* geom,
                                          lsr_stream_t stream) {
    return preprocess_rows_checked(n_views, row0, row1, 1, s, in, out, geom, stream);
}

int lsr_forward_instance_scan_views_async(int32_t n_views, const lsr_settings* const* s, const lsr_fwd_in* in,
                                          void* const* geom, uint32_t* host_counts, lsr_stream_t stream) {
    return count_views(n_views, s, in, geom, host_counts, stream, false);
}

int lsr_forward_depth_order_views_async(int32_t n_views, const lsr_settings* const* s, const lsr_fwd_in* in,
                                        void* const* geom, uint32_t* host_counts, lsr_stream_t stream) {
    return count_views(n_views, s, in, geom, host_counts, stream, true);
}

int lsr_forward_preprocess_views_async(int32_t n_views, const lsr_settings* const* s, const lsr_fwd_in* in,
                                       lsr_fwd_out* const* out, void* const* geom, uint32_t* host_counts,
                                       lsr_stream_t stream) {
    if (!host_counts) return fail(LSR_EINVAL, "host_counts is required");
    return lsr_forward_preprocess_views_split_async(n_views, n_views, s, in, out, geom, host_counts, stream);
}

int lsr_forward_preprocess(const lsr_settings* s, const lsr_fwd_in* in, lsr_fwd_out* out, void* geom,
                           int64_t* num_rendered, lsr_stream_t stream) {
    if (!num_rendered) return fail(LSR_EINVAL, "geom workspace and num_rendered are required");
    uint32_t tot[2] = {0, 0};   // pageable: the copy completes by the synchronisation below
    int rc = lsr_forward_preprocess_async(s, in, out, geom, tot, stream);
    if (rc) return rc;
    LSR_HIP(hipStreamSynchronize(reinterpret_cast<hipStream_t>(stream)));
    *num_rendered = (int64_t)tot[0];
    return LSR_OK;
}

int lsr_forward_binning(const lsr_settings* s, const lsr_fwd_in* in, void* geom, void* binning, void* img,
                        int64_t num_rendered, lsr_stream_t stream) {
    return lsr_forward_binning_views(1, &s, in, &geom, &binning, &img, &num_rendered, stream);
}

int lsr_forward_binning_views(int32_t n_views, const lsr_settings* const* s, const lsr_fwd_in* in, void* const* geom,
                              void* const* binning, void* const* img, const int64_t* num_rendered,
                              lsr_stream_t stream) {
    const auto emit_and_sort = [](const BinBatch& c, const BinView* bv, int ne) {
        const size_t ntiles = c.ntiles;
        hipStream_t st = c.st;
        lsr::EmitBatch eb{};
        eb.P = c.P; eb.grid_x = c.grid.x; eb.grid_y = c.grid.y; eb.W = c.W; eb.H = c.H;
        lsr::SortSeg ss[lsr::LSR_MAX_VIEWS] = {};
        for (int k = 0; k < ne; ++k) {
            const Geom& g = bv[k].g;
            const Img& m = bv[k].m;
            Binning b = carve_binning(bv[k].binning, bv[k].K, nullptr);
            // the emission also presets the tile ranges (0xFFFFFFFF, 0) for the tile sort's last pass,
            // which makes them, and clears the per-tile replay bounds (no separate fill launches); the
            // forward compositor turns the ranges of empty tiles back into (0, 0)
            lsr::EmitView& e = eb.v[k];
            e.order = g.val_a; e.offsets = g.offsets; e.counts = g.counts; e.rect_sorted = g.rect_sorted;
            e.xy = g.xy; e.conic_o = g.conic_o; e.keys = b.key_a; e.vals = b.val_a;
            e.clear.p[0] = reinterpret_cast<uint32_t*>(m.ranges);
            e.clear.n[0] = (uint32_t)(2 * ntiles);
            e.clear.even[0] = 0xFFFFFFFFu;
            e.clear.p[1] = m.tile_max;
            e.clear.n[1] = (uint32_t)ntiles;
            // kept: the first pass drops the instances that reach no quadrant (key 0xFFFFFFFF, about
            // 10 % of them on the headline scene), the second sorts only the listed ones
            ss[k] = lsr::SortSeg{b.key_a, b.val_a, b.key_b, b.val_b, b.sort_tmp, b.kept,
                                 lsr::SortGather{nullptr, nullptr, nullptr}, bv[k].K, m.ranges, (uint32_t)ntiles};
        }
        {
            PhaseTimer t(LSR_PHASE_EMIT, st);
            lsr::launch_emit_instances(eb, ne, st);
        }
        LSR_LAUNCHED("emit", st, c.debug);
        {
            PhaseTimer t(LSR_PHASE_TILE_SORT, st);
            // one set of launches for all views
            const int in_b = lsr::radix_sort_batch(ss, ne, 0, tile_bits((int)ntiles), st);
            if (in_b < 0 || (in_b == 1) != tile_sort_in_b((int)ntiles))
                return fail(LSR_EHIP, "internal: tile sort batch or parity");
        }
        LSR_LAUNCHED("tile sort", st, c.debug);
        return LSR_OK;
    };
    return bin_views(n_views, s, in, geom, binning, img, num_rendered, stream, SIZE_MAX, nullptr, emit_and_sort);
}

int lsr_forward_binning_views_tb(int32_t n_views, const lsr_settings* const* s, const lsr_fwd_in* in, void* const* geom,
                                 void* const* binning, void* const* img, const int64_t* num_rendered,
                                 lsr_stream_t stream) {
    const auto bucket = [](const BinBatch& c, const BinView* bv, int ne) {
        lsr::TbBatch tb{};
        tb.P = c.P; tb.grid_x = c.grid.x; tb.grid_y = c.grid.y; tb.W = c.W; tb.H = c.H; tb.ntiles = (int)c.ntiles;
        for (int k = 0; k < ne; ++k) {
            const Geom& g = bv[k].g;
            const Img& m = bv[k].m;
            BinningTb b = carve_binning_tb(bv[k].binning, bv[k].K, (size_t)c.P, c.ntiles, nullptr);
            lsr::TbView& t = tb.v[k];
            t.counts = g.counts; t.offsets = g.offsets; t.rect = g.rect; t.xy = g.xy; t.conic_o = g.conic_o;
            t.depth = g.key_a;
            t.table = b.table;
            t.tile_total = m.tile_order;   // backward scratch, written by the backward's tile order
            t.tile_start = m.tile_max;     // zeroed again by the bucket sort
            t.ranges = m.ranges;
            t.keys = reinterpret_cast<uint64_t*>(b.b.key_a);
            t.tmp = b.tmp;
            t.words = point_list(b.b, c.grid);
            t.tile_max = m.tile_max;
        }
        {
            PhaseTimer t(LSR_PHASE_TILE_SORT, c.st);
            const hipError_t e = lsr::launch_tile_bucket_binning(tb, ne, c.st);
            if (e != hipSuccess)
                return fail(LSR_EHIP, std::string("tile-bucket binning: dynamic LDS attribute: ") + hipGetErrorString(e));
        }
        LSR_LAUNCHED("tile-bucket binning", c.st, c.debug);
        return LSR_OK;
    };
    // the per-block tile histograms live in LDS (4 bytes a tile)
    return bin_views(n_views, s, in, geom, binning, img, num_rendered, stream, 12288,
                     "tile-bucket binning: more than 12288 tiles (use lsr_forward_binning_views)", bucket);
}

int lsr_forward_composite(const lsr_settings* s, const lsr_fwd_in* in, lsr_fwd_out* out, const void* geom,
                          const void* binning, void* img, int64_t num_rendered, lsr_stream_t stream) {
    lsr_fwd_out* o[1] = {out};
    return lsr_forward_composite_views(1, &s, in, o, &geom, &binning, &img, &num_rendered, stream);
}

int lsr_forward_composite_views(int32_t n_views, const lsr_settings* const* s, const lsr_fwd_in* in,
                                lsr_fwd_out* const* out, const void* const* geom, const void* const* binning,
                                void* const* img, const int64_t* num_rendered, lsr_stream_t stream) {
    int rc = check_each_view(kCompositeViews, n_views, s && out && geom && binning && img && num_rendered, s, in, [&](int v) {
        if (!out[v] || !out[v]->out_color || !out[v]->out_depth) return fail(LSR_EINVAL, "color and depth outputs are required");
        if (in->C > 0 && !out[v]->out_language_feature)
            return fail(LSR_EINVAL, "language feature output is required when C > 0");
        return need_workspaces(geom[v], img[v], binning[v], num_rendered[v]);
    });
    if (rc) return rc;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const int P = in->P, W = s[0]->image_width, H = s[0]->image_height, C = in->C;
    const Grid grid = tile_grid(W, H);
    for (int v0 = 0; v0 < n_views; v0 += lsr::LSR_MAX_VIEWS) {
        const int nv = std::min(n_views - v0, lsr::LSR_MAX_VIEWS);
        lsr::RenderFwdArgs r[lsr::LSR_MAX_VIEWS] = {};
        for (int k = 0; k < nv; ++k) {
            const int v = v0 + k;
            const size_t K = (size_t)num_rendered[v];
            Geom g = carve_geom(const_cast<void*>(geom[v]), (size_t)(P > 0 ? P : 1), nullptr);
            Binning b = carve_binning(const_cast<void*>(binning[v]), K > 0 ? K : 1, nullptr);
            Img m = carve_img(img[v], W, H, nullptr);   // tile_max was zeroed by the binning (atomicMax: idempotent)
            lsr::RenderFwdArgs& a = r[k];
            a.W = W; a.H = H; a.grid_x = grid.x; a.grid_y = grid.y; a.C = C; a.include_feature = s[v]->include_feature;
            a.ranges = m.ranges; a.point_list = K > 0 ? point_list(b, grid) : nullptr;
            a.xy = g.xy; a.conic_o = g.conic_o; a.rgbd = g.rgbd;
            a.lang = in->language_feature;
            a.lang_split = in->C == 32 ? in->language_feature_split : nullptr;
            a.bg = s[v]->bg; a.final_T = m.final_T; a.n_contrib = m.n_contrib;
            a.tile_max_contrib = m.tile_max; a.tile_order = m.tile_order;
            a.out_color = out[v]->out_color; a.out_lang = out[v]->out_language_feature;
            a.out_depth = out[v]->out_depth;
            if (C > 0 && !s[v]->include_feature)
                LSR_HIP(hipMemsetAsync(out[v]->out_language_feature, 0, sizeof(float) * (size_t)C * W * H, st));
        }
        {
            PhaseTimer t(LSR_PHASE_RENDER_FWD, st);
            lsr::launch_render_fwd_views(r, nv, st);
        }
        LSR_LAUNCHED("render forward", st, s[0]->debug);
    }
    return LSR_OK;
}

int lsr_language_split(int32_t P, int32_t C, const float* language_feature, uint16_t* out, lsr_stream_t stream) {
    if (P < 0 || C != 32 || (P > 0 && (!language_feature || !out)))
        return fail(LSR_EINVAL, "lsr_language_split: P >= 0, C == 32 and both buffers are required");
    if ((size_t)P * 32 * 4 >= (size_t)1 << 32) return fail(LSR_EINVAL, "lsr_language_split: P * C * 4 must be < 2^32");
    if (P == 0) return LSR_OK;
    lsr::launch_language_split(P, language_feature, out, reinterpret_cast<hipStream_t>(stream));
    LSR_LAUNCHED("language split", reinterpret_cast<hipStream_t>(stream), false);
    return LSR_OK;
}

int lsr_forward_render(const lsr_settings* s, const lsr_fwd_in* in, lsr_fwd_out* out, void* geom, void* binning,
                       void* img, int64_t num_rendered, lsr_stream_t stream) {
    if (!out || !out->out_color || !out->out_depth) return fail(LSR_EINVAL, "color and depth outputs are required");
    int rc = lsr_forward_binning(s, in, geom, binning, img, num_rendered, stream);
    if (rc) return rc;
    return lsr_forward_composite(s, in, out, geom, binning, img, num_rendered, stream);
}

int lsr_backward(const lsr_settings* s, const lsr_fwd_in* in, const lsr_bwd_in* gin, lsr_bwd_out* gout,
                 const void* geom, const void* binning, const void* img, void* scratch, int64_t num_rendered,
                 int32_t accumulate, lsr_stream_t stream) {
    int rc = check_common(s, in);
    if (rc) return rc;
    if (!gin || !gin->dL_dout_color || !gout) return fail(LSR_EINVAL, "dL_dout_color and outputs are required");
    if (!geom || !img || !scratch || (num_rendered > 0 && !binning)) return fail(LSR_EINVAL, "workspaces are required");
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const int P = in->P, W = s->image_width, H = s->image_height, C = in->C;
    if (P == 0) return LSR_OK;
    const size_t K = (size_t)num_rendered;
    Geom g = carve_geom(const_cast<void*>(geom), (size_t)P, nullptr);
    Binning b = carve_binning(const_cast<void*>(binning), K > 0 ? K : 1, nullptr);
    Img m = carve_img(const_cast<void*>(img), W, H, nullptr);
    const int Ceff = s->include_feature ? C : 0;
    const int recq = lsr::record_floats(Ceff);
    const bool det = gin->deterministic != 0;
    Scratch sc = carve_scratch(scratch, (size_t)P, K > 0 ? K : 1, recq, det, nullptr);
    if (det && K > 0) {
        LSR_HIP(hipMemsetAsync(sc.flags, 0, K, st));
        lsr::launch_scatter_inst_off(P, g.val_a, g.offsets, g.counts, g.inst_off, st);
    }
    if (!det) LSR_HIP(hipMemsetAsync(sc.acc_small, 0, sizeof(float) * lsr::ACC_PITCH * (size_t)P, st));
    // dL/dlanguage: the atomic path adds into it, so zero it unless accumulating; with the language
    // channels off (include_feature = 0) it is exactly zero (the deterministic path writes it only
    // when they are on)
    if (!accumulate && C > 0 && gout->dL_dlanguage_feature && (!det || Ceff == 0))
        LSR_HIP(hipMemsetAsync(gout->dL_dlanguage_feature, 0, sizeof(float) * (size_t)P * C, st));
    if (K > 0) {
        lsr::RenderBwdArgs r{};
        render_bwd_view(r, s, in, gin, g, b, m);
        r.rec = sc.rec; r.flags = sc.flags; r.recq = recq; r.deterministic = det;
        r.acc_small = sc.acc_small; r.acc_lang = gout->dL_dlanguage_feature;
        {
            PhaseTimer t(LSR_PHASE_RENDER_BWD, st);
            lsr::launch_render_bwd(r, st);
        }
        LSR_LAUNCHED("render backward", st, s->debug);
    }
    lsr::PreprocessBwdViewsArgs a = preprocess_bwd_args(s, in, gout, 0, P, 1);
    view_cam(a.cam[0], s, g, sc.acc_small, 0);
    a.rec = sc.rec; a.flags = sc.flags; a.inst_off = g.inst_off; a.recq = recq;
    a.deterministic = det;
    {
        PhaseTimer t(LSR_PHASE_PREPROCESS_BWD, st);
        lsr::launch_preprocess_bwd_views(a, accumulate != 0, true, st);
        if (Ceff > 0 && det)
            lsr::launch_reduce_lang(P, C, lsr::lang_pad(C), recq, sc.rec, sc.flags, g.inst_off, g.tiles,
                                    gout->dL_dlanguage_feature, accumulate != 0, st);
    }
    LSR_LAUNCHED("preprocess backward", st, s->debug);
    return LSR_OK;
}

int lsr_backward_composite(const lsr_settings* s, const lsr_fwd_in* in, const lsr_bwd_in* gin, float* dL_dlanguage,
                           void* geom, const void* binning, const void* img, int64_t num_rendered,
                           lsr_stream_t stream) {
    return lsr_backward_composite_views(1, &s, in, &gin, dL_dlanguage, &geom, &binning, &img, &num_rendered, stream);
}

int lsr_backward_composite_views(int32_t n_views, const lsr_settings* const* s, const lsr_fwd_in* in,
                                 const lsr_bwd_in* const* gin, float* dL_dlanguage, void* const* geom,
                                 const void* const* binning, const void* const* img, const int64_t* num_rendered,
                                 lsr_stream_t stream) {
    int rc = check_each_view(kCompositeViews, n_views, s && gin && geom && binning && img && num_rendered, s, in, [&](int v) {
        int e = need_atomic_grads(gin[v], "dL_dout_color is required",
                                  "the split backward reduces with float atomics; use lsr_backward for deterministic "
                                  "gradients");
        return e ? e : need_workspaces(geom[v], img[v], binning[v], num_rendered[v]);
    });
    if (rc) return rc;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const int P = in->P, C = in->C, W = s[0]->image_width, H = s[0]->image_height;
    if (P == 0) return LSR_OK;
    const int recq = lsr::record_floats(s[0]->include_feature ? C : 0);
    lsr::RenderBwdArgs r[lsr::LSR_MAX_VIEWS] = {};
    int nr = 0;
    auto launch = [&]() {
        if (nr == 0) return;
        {
            PhaseTimer t(LSR_PHASE_RENDER_BWD, st);
            if (C <= 32) lsr::launch_render_bwd_wave_views(r, nr, st);
            else
                for (int k = 0; k < nr; ++k) lsr::launch_render_bwd(r[k], st);   // 64 channels: per-tile kernel
        }
        nr = 0;
    };
    for (int v = 0; v < n_views; ++v) {
        const size_t K = (size_t)num_rendered[v];
        if (K == 0) continue;   // nothing listed: no compositor work
        Geom g = carve_geom(geom[v], (size_t)P, nullptr);   // g.acc: rows of listed Gaussians zeroed by the preprocess
        Binning b = carve_binning(const_cast<void*>(binning[v]), K, nullptr);
        Img m = carve_img(const_cast<void*>(img[v]), W, H, nullptr);
        lsr::RenderBwdArgs& a = r[nr++];
        render_bwd_view(a, s[v], in, gin[v], g, b, m);
        a.recq = recq; a.deterministic = 0;
        a.acc_small = reinterpret_cast<float*>(g.acc); a.acc_lang = dL_dlanguage;
        if (nr == lsr::LSR_MAX_VIEWS) launch();
    }
    launch();
    LSR_LAUNCHED("render backward", st, s[0]->debug);
    return LSR_OK;
}

int lsr_backward_preprocess_views(int32_t n_views, const lsr_settings* const* s, const lsr_fwd_in* in,
                                  lsr_bwd_out* gout, const void* const* geom, int32_t accumulate,
                                  lsr_stream_t stream) {
    if (!in) return fail(LSR_EINVAL, "null argument");
    return lsr_backward_preprocess_views_rows(n_views, s, in, gout, geom, accumulate, 0, in->P, stream);
}

int lsr_backward_preprocess_views_rows(int32_t n_views, const lsr_settings* const* s, const lsr_fwd_in* in,
                                       lsr_bwd_out* gout, const void* const* geom, int32_t accumulate,
                                       int32_t row_begin, int32_t row_count, lsr_stream_t stream) {
    int rc = check_each_view(kBackwardViews, n_views, s && in && gout && geom, s, in, [&](int v) {
        return geom[v] ? LSR_OK : fail(LSR_EINVAL, "the geom workspace is required for every view");
    });
    if (rc) return rc;
    if (row_begin < 0 || row_count < 0 || (int64_t)row_begin + row_count > in->P)
        return fail(LSR_EINVAL, "rows [row_begin, row_begin + row_count) must lie inside [0, P)");
    if (row_begin % 256 != 0) return fail(LSR_EINVAL, "row_begin must be a multiple of 256");
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const int P = in->P, n = row_count;
    const size_t r0 = (size_t)row_begin;
    if (n == 0) return LSR_OK;
    // one launch per LSR_MAX_VIEWS views: Gaussian rows read and gradient rows written once; a row
    // range is the same kernel over pointers advanced to row_begin (gout already addresses it)
    for (int v0 = 0; v0 < n_views; v0 += lsr::LSR_MAX_VIEWS) {
        const int nv = std::min(lsr::LSR_MAX_VIEWS, n_views - v0);
        lsr::PreprocessBwdViewsArgs a = preprocess_bwd_args(s[0], in, gout, r0, n, nv);
        for (int j = 0; j < nv; ++j) {
            Geom g = carve_geom(const_cast<void*>(geom[v0 + j]), (size_t)P, nullptr);
            view_cam(a.cam[j], s[v0 + j], g, reinterpret_cast<const float*>(g.acc), r0);
        }
        {
            PhaseTimer t(LSR_PHASE_PREPROCESS_BWD_VIEWS, st);
            lsr::launch_preprocess_bwd_views(a, accumulate != 0 || v0 > 0, false, st);
        }
        LSR_LAUNCHED("preprocess backward (views)", st, s[0]->debug);
    }
    return LSR_OK;
}

int lsr_backward_views(int32_t n_views, const lsr_settings* const* s, const lsr_fwd_in* in,
                       const lsr_bwd_in* const* gin, lsr_bwd_out* gout, void* const* geom,
                       const void* const* binning, const void* const* img, const int64_t* num_rendered,
                       int32_t accumulate, lsr_stream_t stream) {
    int rc = check_each_view(kBackwardViews, n_views, s && in && gin && gout && geom && binning && img && num_rendered, s, in,
                         [&](int v) {
                             return need_atomic_grads(gin[v], "dL_dout_color is required for every view",
                                                      "lsr_backward_views reduces with float atomics; use lsr_backward "
                                                      "per view for deterministic gradients");
                         });
    if (rc) return rc;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const int P = in->P, C = in->C;
    if (P == 0) return LSR_OK;
    if (!accumulate && C > 0 && gout->dL_dlanguage_feature)
        LSR_HIP(hipMemsetAsync(gout->dL_dlanguage_feature, 0, sizeof(float) * (size_t)P * C, st));
    rc = lsr_backward_composite_views(n_views, s, in, gin, gout->dL_dlanguage_feature, geom, binning, img,
                                          num_rendered, stream);
    if (rc) return rc;
    return lsr_backward_preprocess_views(n_views, s, in, gout, const_cast<const void* const*>(geom), accumulate,
                                         stream);
}

int lsr_radii_max(int32_t P, int32_t n_views, const int32_t* const* radii, int32_t* out, int32_t accumulate,
                  lsr_stream_t stream) {
    if (P < 0 || n_views < 0 || (P > 0 && n_views > 0 && (!radii || !out))) return fail(LSR_EINVAL, "bad lsr_radii_max arguments");
    for (int v = 0; v < n_views; ++v)
        if (P > 0 && (!radii[v] || !lsr::aligned16(radii[v])))
            return fail(LSR_EINVAL, "lsr_radii_max: every radii array must be a 16-byte aligned device pointer");
    if (P > 0 && !lsr::aligned16(out)) return fail(LSR_EINVAL, "lsr_radii_max: out must be 16-byte aligned");
    if (P == 0 || n_views == 0) return LSR_OK;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    lsr::launch_radii_max(P, n_views, reinterpret_cast<const int* const*>(radii), out, accumulate != 0, st);
    LSR_LAUNCHED("radii max", st, false);
    return LSR_OK;
}

int lsr_mark_visible(int32_t P, const float* means3D, const float* viewmatrix, const float* projmatrix,
                     uint8_t* present, lsr_stream_t stream) {
    (void)projmatrix;
    if (P < 0 || (P > 0 && (!means3D || !viewmatrix || !present))) return fail(LSR_EINVAL, "bad mark_visible arguments");
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    lsr::launch_mark_visible(P, means3D, viewmatrix, present, st);
    LSR_LAUNCHED("mark_visible", st, false);
    return LSR_OK;
}

int lsr_profile_phases(uint32_t mask) {
    std::lock_guard<std::mutex> l(g_prof.mu);
    g_prof.mask = mask;
    return LSR_OK;
}

int lsr_profile_enable(int32_t on) {
    std::lock_guard<std::mutex> l(g_prof.mu);
    for (auto& r : g_prof.pending) {
        (void)hipEventSynchronize(r.b);
        g_prof.pool.push_back(r.a);
        g_prof.pool.push_back(r.b);
    }
    g_prof.pending.clear();
    for (int i = 0; i < LSR_NUM_PHASES; ++i) { g_prof.ms[i] = 0.0; g_prof.n[i] = 0; }
    g_prof.on = on != 0;
    return LSR_OK;
}

int lsr_profile_read(double* ms_total, int64_t* launches, int32_t n) {
    std::lock_guard<std::mutex> l(g_prof.mu);
    for (auto& r : g_prof.pending) {
        if (hipEventSynchronize(r.b) != hipSuccess) return fail(LSR_EHIP, "profile: event synchronize failed");
        float ms = 0.0f;
        if (hipEventElapsedTime(&ms, r.a, r.b) == hipSuccess) {
            g_prof.ms[r.phase] += ms;
            g_prof.n[r.phase] += 1;
        }
        g_prof.pool.push_back(r.a);
        g_prof.pool.push_back(r.b);
    }
    g_prof.pending.clear();
    for (int i = 0; i < n && i < LSR_NUM_PHASES; ++i) {
        if (ms_total) ms_total[i] = g_prof.ms[i];
        if (launches) launches[i] = g_prof.n[i];
    }
    return LSR_NUM_PHASES;
}

}  // extern "C"
