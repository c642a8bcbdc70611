"""GPU-side helpers for the parity tests: run the native rasterizer (through the C ABI) and the
oracle on the same seeded inputs, and decode the native workspaces (layout of lsr_api.hip)."""
import numpy as np
import torch

import diff_gaussian_rasterization as dgr
import oracle
from helpers import oracle_settings

ALIGN = 256


def _al(n):
    return (n + ALIGN - 1) // ALIGN * ALIGN


def raster_settings(cam, bg=(1.0, 1.0, 1.0), sh_degree=3, include_feature=True, scale_modifier=1.0, debug=False):
    dev = "cuda"
    return dgr.GaussianRasterizationSettings(
        image_height=cam.image_height, image_width=cam.image_width, tanfovx=cam.tanfovx, tanfovy=cam.tanfovy,
        bg=torch.tensor(bg, dtype=torch.float32, device=dev), scale_modifier=scale_modifier,
        viewmatrix=cam.world_view_transform.to(dev), projmatrix=cam.full_proj_transform.to(dev),
        sh_degree=sh_degree, campos=cam.camera_center.to(dev), prefiltered=False, debug=debug,
        include_feature=include_feature)


class DecodedState:
    """A forward's state as arrays, for the checks below where no native state exists (the oracle
    standing in for the kernels on a machine without a GPU): what decode_img and decode_point_list
    return, and the radii."""

    def __init__(self, ranges, tile_max, final_T, n_contrib, point_list, radii):
        self.ranges, self.tile_max, self.final_T, self.n_contrib = ranges, tile_max, final_T, n_contrib
        self.point_list, self.radii = point_list, radii


def tile_max_of(n_contrib):
    """Per 16 x 16 tile the largest n_contrib of its pixels inside the image [tiles]."""
    H, W = n_contrib.shape
    gx, gy = (W + 15) // 16, (H + 15) // 16
    pad = np.zeros((16 * gy, 16 * gx), np.int64)
    pad[:H, :W] = n_contrib
    return pad.reshape(gy, 16, gx, 16).max(axis=(1, 3)).reshape(-1)


def oracle_as_native(ref):
    """The oracle's own state in the native one's place (DecodedState), tile_max derived from its
    n_contrib."""
    st = ref.state()
    return DecodedState(st["ranges"], tile_max_of(st["n_contrib"]).astype(np.uint32), st["final_T"],
                        st["n_contrib"], st["point_list"], ref.radii)


def decode_img(state):
    """ranges [tiles,2], tile_max [tiles], final_T [H,W], n_contrib [H,W] from the img workspace."""
    if isinstance(state, DecodedState):
        return state.ranges, state.tile_max, state.final_T, state.n_contrib
    W, H = state.settings.c.image_width, state.settings.c.image_height
    gx, gy = (W + 15) // 16, (H + 15) // 16
    nt = gx * gy
    raw = state.img.cpu().numpy()
    off = 0
    ranges = raw[off:off + nt * 8].view(np.uint32).reshape(nt, 2); off += _al(nt * 8)
    tmax = raw[off:off + nt * 4].view(np.uint32); off += _al(nt * 4)
    fT = raw[off:off + W * H * 4].view(np.float32).reshape(H, W); off += _al(W * H * 4)
    nc = raw[off:off + W * H * 4].view(np.uint32).reshape(H, W)
    return ranges, tmax, fT, nc


def decode_point_words(state):
    """Raw point-list words: Gaussian id in the low 28 bits, the quadrant bits on top."""
    K = state.num_rendered
    W, H = state.settings.c.image_width, state.settings.c.image_height
    nt = ((W + 15) // 16) * ((H + 15) // 16)
    bits = 1
    while (1 << bits) <= nt:
        bits += 1
    in_b = ((bits + 7) // 8) % 2 == 1
    raw = state.binning.cpu().numpy()
    blk = _al(K * 4)
    off = 3 * blk if in_b else 2 * blk
    return raw[off:off + K * 4].view(np.uint32)


def decode_point_list(state):
    if isinstance(state, DecodedState):
        return state.point_list
    K = state.num_rendered
    W, H = state.settings.c.image_width, state.settings.c.image_height
    nt = ((W + 15) // 16) * ((H + 15) // 16)
    bits = 1
    while (1 << bits) <= nt:        # tile keys 0..nt-1 (instances reaching no quadrant are dropped)
        bits += 1
    in_b = ((bits + 7) // 8) % 2 == 1
    raw = state.binning.cpu().numpy()
    blk = _al(K * 4)
    off = 3 * blk if in_b else 2 * blk
    return raw[off:off + K * 4].view(np.uint32) & 0x0FFFFFFF   # low 28 bits: Gaussian id


def check_binning_against_upstream(state, ref_state, W, H):
    """The native binning drops (Gaussian, tile) instances whose splat cannot pass the alpha
    prefilter at any pixel of the tile (preprocess.hip, binning rectangle).  Checks, against the
    oracle's upstream binning: every tile list is an ordered subsequence of upstream's; every dropped
    entry has alpha < 1/255 at every pixel of its tile (so dropping it changes nothing); and each
    pixel's last contributor (n_contrib, a list position) is the same Gaussian."""
    ranges, _, fT, nc = decode_img(state)
    pl = decode_point_list(state).astype(np.int64)
    rr, rpl, rnc = ref_state["ranges"], ref_state["point_list"].astype(np.int64), ref_state["n_contrib"]
    xy, co = ref_state["xy"].astype(np.float64), ref_state["conic_o"].astype(np.float64)
    gx = (W + 15) // 16
    assert ranges[:, 1].max(initial=0) <= len(pl) and len(pl) <= len(rpl)
    dropped_total = 0
    for t in range(len(ranges)):
        g = pl[ranges[t, 0]:ranges[t, 1]]
        u = rpl[rr[t, 0]:rr[t, 1]]
        pos = {gid: k for k, gid in enumerate(u)}
        idx = np.array([pos[gid] for gid in g], dtype=np.int64)       # KeyError: entry not upstream
        assert (np.diff(idx) > 0).all(), f"tile {t}: order differs from upstream"
        dropped = np.setdiff1d(u, g)
        dropped_total += len(dropped)
        tx, ty = t % gx, t // gx
        px, py = np.meshgrid(np.arange(16 * tx, min(16 * tx + 16, W)), np.arange(16 * ty, min(16 * ty + 16, H)))
        px, py = px.ravel().astype(np.float64), py.ravel().astype(np.float64)
        if len(dropped):
            dx = xy[dropped, 0][:, None] - px[None]
            dy = xy[dropped, 1][:, None] - py[None]
            a, b, c, o = (co[dropped, k][:, None] for k in range(4))
            power = -0.5 * (a * dx * dx + c * dy * dy) - b * dx * dy
            alpha = np.minimum(0.99, o * np.exp(np.minimum(power, 0.0)))
            assert (alpha < (1.0 / 255.0) * (1 - 1e-6)).all(), f"tile {t}: a dropped entry contributes"
        # last contributor of each pixel of the tile: the same Gaussian
        for yy, xx in zip(py.astype(int), px.astype(int)):
            n, rn = int(nc[yy, xx]), int(rnc[yy, xx])
            assert (n == 0) == (rn == 0), (t, yy, xx)
            if n:
                assert g[n - 1] == u[rn - 1], (t, yy, xx)
    np.testing.assert_array_equal(fT, ref_state["final_T"])
    return dropped_total


def run_native(scene, cam, bg=(1.0, 1.0, 1.0), include_feature=True, use_precomp_cov=False, colors_precomp=None,
               sh_degree=3, scale_modifier=1.0):
    dev = "cuda"
    rs = raster_settings(cam, bg=bg, sh_degree=sh_degree, include_feature=include_feature,
                         scale_modifier=scale_modifier)
    kw = {}
    if use_precomp_cov:   # a precomputed covariance is taken as given: scale_modifier does not enter it
        kw["cov3D_precomp"] = torch.tensor(oracle.cov3d(scene.scales.numpy(), scene.rotations.numpy())).to(dev)
    else:
        kw["scales"], kw["rotations"] = scene.scales.to(dev), scene.rotations.to(dev)
    if colors_precomp is not None:
        kw["colors_precomp"] = torch.as_tensor(colors_precomp).to(dev)
    else:
        kw["shs"] = scene.shs.to(dev)
    lang = scene.lang.to(dev) if scene.lang.numel() > 0 else None
    return dgr.forward_native(rs, scene.means3D.to(dev), scene.opacities.to(dev), language_feature=lang, **kw)


def run_oracle(scene, cam, bg=(1.0, 1.0, 1.0), include_feature=True, use_precomp_cov=False, colors_precomp=None,
               sh_degree=3, nthreads=0, scale_modifier=1.0, double=False, lang=None):
    """lang: language rows to use instead of the scene's."""
    s = oracle_settings(cam, bg=bg, sh_degree=sh_degree, include_feature=include_feature,
                        scale_modifier=scale_modifier)
    kw = {}
    if use_precomp_cov:
        kw["cov3D_precomp"] = oracle.cov3d(scene.scales.numpy(), scene.rotations.numpy())
    else:
        kw["scales"], kw["rotations"] = scene.scales.numpy(), scene.rotations.numpy()
    if colors_precomp is not None:
        kw["colors_precomp"] = np.asarray(colors_precomp)
    else:
        kw["shs"] = scene.shs.numpy()
    if lang is None:
        lang = scene.lang.numpy() if scene.lang.numel() > 0 else None
    return oracle.forward(s, scene.means3D.numpy(), scene.opacities.numpy(), lang=lang, nthreads=nthreads,
                          double=double, **kw)


def grad_err(native, ref):
    """max |native - ref| relative to max |ref| (per tensor)"""
    native = np.asarray(native, np.float64)
    ref = np.asarray(ref, np.float64)
    scale = max(np.abs(ref).max(), 1e-12)
    return float(np.abs(native - ref).max() / scale)


GRAD_TOL = 1e-4
# the gradient rows the compositor accumulates directly, by the oracle's names (abs_terms covers these)
DIRECT_FIELDS = ("lang", "opacity", "means2D")
# backward_native's names -> the oracle's
NATIVE_TO_ORACLE = dict(means3D="means3D", means2D="means2D", colors="colors", opacities="opacity",
                        language_feature="lang", cov3D="cov3D", sh="sh", scales="scales", rotations="rotations")


def oracle_keyed(g):
    """backward_native's dict (device tensors, None for the absent fields) under the oracle's names,
    as float64 numpy."""
    return {NATIVE_TO_ORACLE[k]: v.detach().double().cpu().numpy() for k, v in g.items() if v is not None}


def grad_check(native, ref, abs_terms=None):
    """Per-element check of gradients against a reference; both are dicts under the oracle's names
    (oracle_keyed converts the native ones), and every field of `native` is checked.

    Every field: grad_err <= GRAD_TOL, the tensor-wide contract.  The directly accumulated fields
    (DIRECT_FIELDS), when `abs_terms` (the reference's backward(abs_terms=True)) has them, also per
    element
        |native - ref| <= 1e-4 |ref| + 1e-4 A
    with A the sum of the magnitudes of the element's per-pixel terms: an element is held to the
    rounding of what it was summed from, however small it is beside the tensor's largest (form and
    coefficients: tests/test_headline_gpu.py).  No floor: an element with A = 0 must be exactly 0.
    A non-finite value fails.

    Returns (bad, stats): bad[field] describes the offences (empty dict: passed); stats[field] has
    grad_err and, for the direct fields, max_err_over_A (over the elements with A > 0)."""
    bad, stats = {}, {}
    for key, n in native.items():
        r = np.asarray(ref[key], np.float64)
        n = np.asarray(n, np.float64).reshape(r.shape)
        if r.size == 0:
            continue
        err = np.abs(n - r)
        st = dict(grad_err=float(err.max() / max(np.abs(r).max(), 1e-12)))
        off = {}
        if not st["grad_err"] <= GRAD_TOL:
            off["grad_err"] = st["grad_err"]
        if abs_terms is not None and key in DIRECT_FIELDS:
            A = np.asarray(abs_terms[key], np.float64).reshape(r.shape)
            assert (A >= np.abs(r) * (1 - 1e-3) - 1e-30).all(), key      # |sum| <= sum |term|
            pos = A > 0
            st["max_err_over_A"] = float((err[pos] / A[pos]).max()) if pos.any() else 0.0
            over = ~(err <= 1e-4 * np.abs(r) + 1e-4 * A)
            if over.any():
                idx = np.argwhere(over)
                off["elements"] = int(over.sum())
                off["first"] = [(tuple(int(i) for i in ix), float(n[tuple(ix)]), float(r[tuple(ix)]),
                                 float(A[tuple(ix)])) for ix in idx[:6]]
        stats[key] = st
        if off:
            bad[key] = off
    return bad, stats


DEFORM_COEF = 1e-4


def deform_check(native, ref, A, coef=DEFORM_COEF):
    """Per-element check of the deformation field's outputs (as offsets) or gradients against the
    oracle; native, ref and A are dicts name -> array (entries of `native` that are None are skipped),
    ref from DeformOracle(coords="float32") and A its term scales (abs_terms=True).  Per element
        |native - ref| <= 1e-4 |ref| + coef A
    and exactly 0 where A = 0 (nothing flows into the element: a plane cell no Gaussian touches, a
    coordinate behind a border mask); a non-finite value fails.

    coef.  DEFORM_COEF = 1e-4 is grad_check's coefficient, the project's figure for sums of bf16
    hi / lo products (measured at 2.6e-5 A on the compositors).  It stands on a CPU judgement, not on
    the kernels' error: the oracle's products="bf16x3" emulation (every Linear product, forward and
    backward, as hi hi + hi lo + lo hi of bf16 halves accumulated in float32 -- it overstates the
    kernels, whose small heads form G W2 in fp32) against the float64 oracle on the same float32
    coordinates stays under half of it on every case of tests/deform_cases.py with P <= 12,300:
    largest err / A 2.3e-5 (tests/test_deform_check.py asserts the half and prints the figures).  One
    product of hi / lo halves is off by at most ~2^-16 of its magnitude and a chain of up to nine
    layers (forward and back) adds the layers' shares, all relative to A because A is carried through
    the chain; errors of the 16..128 products of an element do not line up, hence the distance to
    the worst case.  The 32 / 64 shape runs its MLP in fp32 and takes the same coefficient.  grid.aabb
    has a term scale of its own (DeformOracle's docstring), of which the emulation reaches 8.9e-6.

    Returns (bad, stats): bad[name] = dict(elements, first=[(index, native, ref, A, err / A)...]);
    stats[name] = dict(max_err_over_A, rel) with rel the tensor-wide max |err| / max |ref|."""
    bad, stats = {}, {}
    for key, n in native.items():
        if n is None:
            continue
        r = np.asarray(ref[key], np.float64)
        a = np.asarray(A[key], np.float64).reshape(r.shape)
        n = np.asarray(_np(n), np.float64).reshape(r.shape)
        if r.size == 0:
            continue
        assert (a >= np.abs(r) * (1 - 1e-9) - 1e-300).all(), key           # |sum| <= sum |term|
        finite = np.isfinite(n)
        err = np.where(finite, np.abs(np.where(finite, n, 0.0) - r), np.inf)
        pos = a > 0
        ratio = np.where(pos, err / np.where(pos, a, 1.0), 0.0)
        stats[key] = dict(max_err_over_A=float(ratio.max()), rel=float(err.max() / max(np.abs(r).max(), 1e-30)))
        over = ~(err <= 1e-4 * np.abs(r) + coef * a) | (~pos & (n != 0))
        if over.any():
            idx = np.argwhere(over)
            bad[key] = dict(elements=int(over.sum()),
                            first=[(tuple(int(i) for i in ix), float(n[tuple(ix)]), float(r[tuple(ix)]),
                                    float(a[tuple(ix)]), float(ratio[tuple(ix)])) for ix in idx[:6]])
    return bad, stats


U24 = 2.0 ** -24          # fp32 unit roundoff
IMAGE_COEF_MAX = 1e-4     # the cap of the derived coefficient; the matrix-core language coefficient
IMAGE_COEF_C = 8          # the constant c of image_coef


def image_coef(k):
    """min(1e-4, (2 k + c) 2^-24), the per-pixel coefficient of image_check for sums the kernels
    and the float oracle both keep in fp32; k = the pixel's n_contrib.

    Both sides blend the same entries with the same alpha and T bit for bit (image_check asserts the
    equal final_T and last contributor this rests on), so they differ only in how a term
    t = f alpha T enters the sum s, u = 2^-24, every partial sum bounded by A = sum |t|:
      float oracle (no contraction)  fl(fl(f alpha) T): 2 u |t|;  s = fl(s + .): u |s| <= u A
      kernel                         w = fl(alpha T):     u |t|;  s = fma(f, w, s): u |s| <= u A
    at most 3 u |t| + 2 u A apart per blended entry, (3 + 2 n) u A over a pixel's n entries.
    n_contrib is the list position of the last blended entry, so n <= k.  The colour then adds
    T bg: fl(T bg) and a rounded add in the oracle, the same or one contracted fma in the kernel,
    3 u A more (A includes T bg); language and depth have no final operation.  Two more units cover
    what the first-order count leaves out: the second-order terms, and A taken from a rounded
    float image (colour, depth) or from the double oracle's weights (language), either within
    1e-5 of the exact sum.  c = 3 + 3 + 2 = 8.  The cap 1e-4 (k >= 835) is grad_check's
    coefficient: errors of a long sum do not line up, and the reference itself is only that good
    against the double oracle (tests/test_forward_check.py)."""
    return np.minimum(IMAGE_COEF_MAX, (2.0 * np.asarray(k, np.float64) + IMAGE_COEF_C) * U24)


def _np(x):
    return x.detach().cpu().numpy() if hasattr(x, "detach") else np.asarray(x)


def image_elements(native, ref, A, coef):
    """One output image [c, H, W] against the reference, per element: finite, |native - ref| <=
    coef A (coef: scalar or [H, W]), exactly 0 where A == 0.  Returns (offences, stats)."""
    n, r, A = (np.asarray(x, np.float64) for x in (native, ref, A))
    assert n.shape == r.shape == A.shape, (n.shape, r.shape, A.shape)
    off, st = {}, dict(max_err_over_A=0.0, max_err_over_bound=0.0)
    if n.size == 0:
        return off, st
    bound = np.broadcast_to(np.asarray(coef, np.float64), n.shape[1:])[None] * A
    finite = np.isfinite(n)
    err = np.where(finite, np.abs(np.where(finite, n, 0.0) - r), np.inf)
    pos = A > 0
    if pos.any():
        st["max_err_over_A"] = float((err[pos] / A[pos]).max())
        st["max_err_over_bound"] = float((err[pos] / bound[pos]).max())
    over = ~finite | ~(err <= bound) | (~pos & (n != 0))
    if over.any():
        idx = np.argwhere(over)
        off["elements"] = int(over.sum())
        off["first"] = [(tuple(int(i) for i in ix), float(n[tuple(ix)]), float(r[tuple(ix)]), float(A[tuple(ix)]))
                        for ix in idx[:6]]
    return off, st


def uses_matrix_cores(C, include_feature=True):
    """The language sums run on k_render_fwd_wave_mfma (bf16 hi / lo products): 17..32 channels."""
    return bool(include_feature) and 17 <= C <= 32


def image_check(native, ref, A_lang, coef=None, exact=True):
    """The forward counterpart of grad_check: one view's native (color, lang, depth, state) against
    the float oracle's OracleResult `ref` of the same view.  state: a RasterizerState, or a
    DecodedState where the oracle stands in for the kernels.

    Exact: radii; final_T bit for bit; every pixel's last contributor the same Gaussian and every
    tile list an ordered subsequence of upstream's (check_binning_against_upstream);
    tile_max_contrib[t] == the largest native n_contrib over tile t's pixels inside the image (0
    where none blends); no tile range left at the preset (~0, 0): a tile without entries has
    exactly (0, 0); a pixel with n_contrib == 0 has colour bg, language 0, depth 0, final_T 1.

    Per element, no floor: |native - ref| <= coef A, exactly 0 where A == 0, non-finite fails.
    A: language -- `A_lang` [C, H, W], the double oracle's forward with |language rows| (the
    weights do not depend on them: the sum of |f| w); colour and depth -- the oracle's own image,
    valid because every term is non-negative (asserted: the activated colours, bg and the visible
    depths).  coef: image_coef(native n_contrib), except 1e-4 (IMAGE_COEF_MAX, grad_check's
    coefficient for the same arithmetic) for the language image of the matrix-core kernel, whose
    products are bf16 hi / lo splits (~2^-16 per term) summed in fp32.  `coef` overrides both
    (the float oracle against the double one rounds the projection too: 1e-4 throughout).

    Returns (bad, stats): bad[what] describes the offences (empty: passed); stats[output] has
    max_err_over_A and max_err_over_bound (over the elements with A > 0)."""
    color, lang, depth, state = native
    color, lang, depth = _np(color), _np(lang), _np(depth)
    H, W = color.shape[1], color.shape[2]
    C = lang.shape[0]
    rs = ref.state()
    bg = np.asarray(ref.settings.bg, color.dtype).reshape(3)
    vis = ref.radii > 0
    assert (rs["rgb"] >= 0).all() and (bg >= 0).all() and (rs["depth"][vis] > 0).all()
    include_feature = bool(ref.settings.include_feature)
    A_lang = np.zeros((C, H, W)) if A_lang is None else np.asarray(A_lang, np.float64)
    assert (A_lang >= np.abs(ref.lang) * (1 - 1e-3) - 1e-30).all()       # |sum| <= sum |term|
    bad, stats = {}, {}
    ranges, tmax, fT, nc = decode_img(state)
    if exact:
        if not np.array_equal(_np(state.radii), ref.radii):
            bad["radii"] = int((_np(state.radii) != ref.radii).sum())
        try:
            check_binning_against_upstream(state, rs, W, H)     # final_T, last contributors, lists
        except (AssertionError, KeyError) as e:
            bad["binning"] = repr(e)[:400]
        want = tile_max_of(nc)
        if not np.array_equal(tmax.astype(np.int64), want):
            t = np.nonzero(tmax.astype(np.int64) != want)[0]
            bad["tile_max_contrib"] = [(int(i), int(tmax[i]), int(want[i])) for i in t[:6]]
        r = ranges.astype(np.int64)
        upstream_empty = rs["ranges"][:, 0] == rs["ranges"][:, 1]
        wrong = ((r[:, 0] >= r[:, 1]) | upstream_empty) & ((r[:, 0] != 0) | (r[:, 1] != 0))
        if wrong.any():
            bad["empty_tile_range"] = [(int(i), int(r[i, 0]), int(r[i, 1])) for i in np.nonzero(wrong)[0][:6]]
        e = nc == 0
        ok = ((color[:, e] == bg[:, None]).all() and (lang[:, e] == 0).all() and (depth[:, e] == 0).all()
              and (fT[e] == 1).all())
        if not ok:
            bad["uncovered_pixels"] = int(e.sum())
    k = image_coef(nc) if coef is None else coef
    kl = IMAGE_COEF_MAX if coef is None and uses_matrix_cores(C, include_feature) else k
    for name, n, r, A, cf in (("color", color, ref.color, ref.color, k), ("lang", lang, ref.lang, A_lang, kl),
                              ("depth", depth, ref.depth, ref.depth, k)):
        off, st = image_elements(n, r, A, cf)
        stats[name] = st
        if off:
            bad[name] = off
    return bad, stats


# ---- the geom workspace of one view (carve_geom, lsr_api.hip) and the forward preprocess check ----
ACC_PITCH = 16            # floats per accumulator row (lsr_internal.h)
# (name, dtype, elements per Gaussian) in carve order; each array starts on a 256-byte boundary
GEOM_ARRAYS = (("xy", np.float32, 2), ("conic_o", np.float32, 4), ("rgbd", np.float32, 4), ("clamped", np.uint8, 1),
               ("tiles", np.uint32, 1), ("key_a", np.uint32, 1), ("key_b", np.uint32, 1), ("val_a", np.uint32, 1),
               ("val_b", np.uint32, 1), ("counts", np.uint32, 1), ("offsets", np.uint32, 1), ("inst_off", np.uint32, 1),
               ("radius", np.int32, 1), ("rect", np.uint32, 2), ("rect_sorted", np.uint32, 2))


def rect_pack(x0, y0, x1, y1, qmap):
    """lsr_internal.h rect_pack on arrays -> [n, 2] uint32."""
    x0, y0, x1, y1, qmap = (np.asarray(a, np.uint32) for a in (x0, y0, x1, y1, qmap))
    return np.stack([x0 | y0 << 12 | (qmap & 0xFF) << 24, x1 | y1 << 12 | (qmap >> 8) << 24], axis=-1).astype(np.uint32)


def rect_unpack(rect):
    """rect [n, 2] uint32 -> dict of int64 arrays: x0, y0, x1, y1 (rect_unpack), qmap (rect_quad_map),
    small (rect_small), mask (rect_tile_mask of qmap), area, count (rect_count)."""
    r = np.asarray(rect, np.uint32).astype(np.int64)
    x0, y0, x1, y1 = r[:, 0] & 0xFFF, (r[:, 0] >> 12) & 0xFFF, r[:, 1] & 0xFFF, (r[:, 1] >> 12) & 0xFFF
    qmap = (r[:, 0] >> 24) | (r[:, 1] >> 24) << 8
    small = (x1 - x0 <= 2) & (y1 - y0 <= 2)
    mask = ((qmap & 0x33) != 0) * 1 | ((qmap & 0xCC) != 0) * 2 | ((qmap & 0x3300) != 0) * 4 | ((qmap & 0xCC00) != 0) * 8
    area = (x1 - x0) * (y1 - y0)
    popc = np.array([bin(int(m)).count("1") for m in mask], np.int64)
    count = np.where((area > 0) & small, popc, area)
    return dict(x0=x0, y0=y0, x1=x1, y1=y1, qmap=qmap, small=small, mask=mask, area=area, count=count)


def decode_geom(geom_bytes, P):
    """One view's geom workspace (uint8 tensor or array of lsr_geom_bytes(P) bytes) as numpy arrays
    by the layout of carve_geom: the arrays of GEOM_ARRAYS, total [4] u32, then the sort's and the
    scan's workspaces, whose joint size is what lsr_geom_bytes(P) leaves between total and the last
    array, acc [P, ACC_PITCH] float32.  rect also comes unpacked under "rect_fields" (rect_unpack)."""
    raw = _np(geom_bytes).reshape(-1).view(np.uint8)
    total_bytes = int(dgr._lib.load().lsr_geom_bytes(P))
    assert raw.size == total_bytes, (raw.size, total_bytes)
    out, off = {}, 0
    for name, dt, n in GEOM_ARRAYS:
        nb = P * n * np.dtype(dt).itemsize
        a = raw[off:off + nb].view(dt)
        out[name] = a.reshape(P, n) if n > 1 else a
        off += _al(nb)
    out["total"] = raw[off:off + 16].view(np.uint32)
    off += _al(16)
    acc_bytes = P * ACC_PITCH * 4
    acc_off = total_bytes - _al(acc_bytes)
    assert acc_off >= off and (acc_off - off) % ALIGN == 0, (off, acc_off)   # sort_tmp + scan_tmp, each aligned
    out["tmp_bytes"] = acc_off - off
    out["acc"] = raw[acc_off:acc_off + acc_bytes].view(np.float32).reshape(P, ACC_PITCH)
    assert acc_off + _al(acc_bytes) == total_bytes       # the layout ends exactly at lsr_geom_bytes(P)
    out["rect_fields"] = rect_unpack(out["rect"])
    return out


def upstream_rect(xy, radii, W, H):
    """tile_rect (lsr_common.h; upstream getRect) in float32 on arrays: rmin_x, rmin_y, rmax_x, rmax_y."""
    gx, gy = (W + 15) // 16, (H + 15) // 16
    p, r = np.asarray(xy, np.float32), np.asarray(radii).astype(np.float32)
    f16, f15 = np.float32(16.0), np.float32(15.0)

    def clip(v, g):   # (int) truncates toward zero; clamped into [0, g]
        return np.clip(np.trunc(np.clip(v, -1e9, 1e9)).astype(np.int64), 0, g)
    return (clip((p[:, 0] - r) / f16, gx), clip((p[:, 1] - r) / f16, gy),
            clip((p[:, 0] + r + f15) / f16, gx), clip((p[:, 1] + r + f15) / f16, gy))


def _ulps(a, b):
    """Distance of float32 arrays in units in the last place (bit patterns on the number line;
    non-finite values count as 2^31)."""
    def line(x):
        i = np.asarray(x, np.float32).view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7FFFFFFF), i)
    d = np.abs(line(a) - line(b))
    return np.where(np.isfinite(a) & np.isfinite(b), d, 2 ** 31)


def preprocess_check(decoded, radii, ref, W, H, point_list=None, num_rendered=None, prefill=None):
    """One view's forward preprocess -- `decoded` (decode_geom of its geom workspace after phase 1)
    and the public `radii` -- against the float oracle's OracleResult `ref` of the same view.

    Rows with ref.radii > 0: radii and the workspace's radius equal ref.radii; xy, conic_o (a, b,
    c, opacity), the colour and the depth equal the oracle's bit for bit (uint32 views: -0.0 and
    NaN differ); the clamped bits equal the oracle's.  Rows with ref.radii == 0: radii, radius,
    tiles, both rect words and clamped are 0.
    Every row: tiles == rect_count(rect); a non-empty rectangle lies inside upstream's 3-sigma
    rectangle (upstream_rect of the oracle's xy and radii) and the grid; tiles <= the oracle's
    (upstream's) count; a rectangle wider or taller than 2 tiles has a zero quadrant map.
    Opacity <= 0.003 with a radius: tiles == 0 and rect == 0 (no pixel can pass 1 / 255; between
    0.003 and 0.005 the switch of skip_power's fast log is no contract, above it only the rules
    above hold).
    acc: all ACC_PITCH floats of a row with a non-empty rectangle are zero bits; with `prefill` (the
    byte the caller filled the workspace with) every other row still holds it.
    num_rendered (the native instance count), when given: sum(tiles) == num_rendered.  point_list
    (the ids of the native list's valid entries: the tile ranges' extent, the binning drops the
    instances that reach no quadrant), when given: id i is listed at most tiles[i] times, exactly
    tiles[i] times when its rectangle is at most 2 x 2 tiles.

    Returns (bad, stats): bad[what] describes the offences (empty: passed); stats has the row counts
    and, per float field, the number of differing elements and the largest distance in ulps."""
    st = ref.state()
    P = len(ref.radii)
    vis = ref.radii > 0
    radii = _np(radii).reshape(-1)
    gx, gy = (W + 15) // 16, (H + 15) // 16
    bad, stats = {}, dict(visible=int(vis.sum()))

    def rows(mask):
        return [int(i) for i in np.nonzero(mask)[0][:6]]

    for name, got in (("radii", radii), ("radius", decoded["radius"])):
        if not np.array_equal(got, ref.radii):
            bad[name] = rows(got != ref.radii)
    rgbd = decoded["rgbd"]
    for name, got, want in (("xy", decoded["xy"], st["xy"]), ("conic_o", decoded["conic_o"], st["conic_o"]),
                            ("rgb", rgbd[:, :3], st["rgb"]), ("depth", rgbd[:, 3:], st["depth"][:, None])):
        g, w = np.ascontiguousarray(got[vis], np.float32), np.ascontiguousarray(want[vis], np.float32)
        diff = g.view(np.uint32) != w.view(np.uint32)
        stats[name] = dict(differing=int(diff.sum()), max_ulps=int(_ulps(g, w).max(initial=0)))
        if diff.any():
            ix = np.argwhere(diff)[:6]
            bad[name] = dict(differing=int(diff.sum()), max_ulps=stats[name]["max_ulps"],
                             first=[(int(np.nonzero(vis)[0][i]), int(k), float(g[i, k]), float(w[i, k])) for i, k in ix])
    cl = decoded["clamped"].astype(np.int64)
    want_cl = (st["clamped"].astype(np.int64) * np.array([1, 2, 4])).sum(axis=1)
    if (cl != want_cl)[vis].any():
        bad["clamped"] = rows(vis & (cl != want_cl))
    rect, tiles = decoded["rect"], decoded["tiles"].astype(np.int64)
    f = rect_unpack(rect)
    for name, arr in (("radii", radii), ("radius", decoded["radius"]), ("tiles", tiles), ("rect", rect.any(axis=1)),
                      ("clamped", cl)):
        if (arr != 0)[~vis].any():
            bad["culled_" + name] = rows(~vis & (arr != 0))
    if (tiles != f["count"]).any():
        bad["tiles_vs_rect_count"] = rows(tiles != f["count"])
    full = f["area"] != 0
    ux0, uy0, ux1, uy1 = upstream_rect(st["xy"], ref.radii, W, H)
    inside = ((f["x0"] >= ux0) & (f["y0"] >= uy0) & (f["x1"] <= ux1) & (f["y1"] <= uy1) & (f["x1"] > f["x0"]) &
              (f["y1"] > f["y0"]) & (f["x1"] <= gx) & (f["y1"] <= gy))
    if (full & ~inside).any():
        bad["rect_outside_upstream"] = rows(full & ~inside)
    if (tiles > st["tiles"].astype(np.int64)).any():
        bad["tiles_above_upstream"] = rows(tiles > st["tiles"])
    if (~f["small"] & (f["qmap"] != 0)).any():
        bad["map_on_large_rect"] = rows(~f["small"] & (f["qmap"] != 0))
    opacity = st["conic_o"][:, 3]
    faint = vis & (opacity <= np.float32(0.003))
    if (faint & ((tiles != 0) | rect.any(axis=1))).any():
        bad["faint_listed"] = rows(faint & ((tiles != 0) | rect.any(axis=1)))
    accw = np.ascontiguousarray(decoded["acc"]).view(np.uint32).reshape(P, ACC_PITCH)
    if (accw[full] != 0).any():
        bad["acc_not_zeroed"] = rows(full & (accw != 0).any(axis=1))
    if prefill is not None:
        word = int(prefill) * 0x01010101
        if (accw[~full] != word).any():
            bad["acc_written_without_rect"] = rows(~full & (accw != word).any(axis=1))
    stats.update(rect_rows=int(full.sum()), listed_rows=int((tiles > 0).sum()), unlisted_visible=int((vis & (tiles == 0)).sum()),
                 faint_visible=int(faint.sum()), small_rects=int((full & f["small"]).sum()),
                 tiles=int(tiles.sum()), upstream_tiles=int(st["tiles"].astype(np.int64).sum()))
    if num_rendered is not None and int(tiles.sum()) != int(num_rendered):
        bad["num_rendered"] = (int(tiles.sum()), int(num_rendered))
    if point_list is not None:
        ids = np.asarray(point_list).astype(np.int64)
        if ids.size and ids.max() >= P:
            bad["list_id_out_of_range"] = int(ids.max())
        else:
            n = np.bincount(ids, minlength=P)
            wrong = (n > tiles) | (f["small"] & (n != tiles))
            if wrong.any():
                bad["list_counts"] = [(i, int(n[i]), int(tiles[i])) for i in rows(wrong)]
            stats["listed_instances"] = int(n.sum())
    return bad, stats
